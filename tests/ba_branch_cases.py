"""The bundle-adjustment cases that reach what the prototype scene does not (tests/test_ba_branches_ref.py on the CPU, tests/test_ba_branches_gpu.py
on the device): not a test module.  A case is a name -> (rows, camera, parameters); `reached` states, on the restatement's own records, log and
sit-out counts, the branch the case is named for, so that a case cannot lose its meaning silently.

All cases are 9 frames, about 160 points, stride 4 (two windows: frames 0 ... 4 and 4 ... 8) unless their builder says otherwise.
  aniso_*      fx != fy (the library's default camera, a 1 : 2 camera, a camera of 1e-3 px and one of 1e6 px focal length)
  sitout_*     points that sit a linearisation out (a pivot of their damped 3 x 3 block not > 0 or not finite): some of them while steps are
               accepted (the translations times 2^-502: Ju Ju of the nearer points overflows first), one point alone while the camera system is
               solved (a planted near point), points in every linearisation (2^-506: all of a window's; huber_px = 5e-324)
  denormal     huber_px = 1e-310: every weight on the linear branch is a denormal number, the cost is some 3e-307
  no_scale     the last free frame's input centre is the anchor's: VIS_BA_NO_SCALE
  clamp_*      lambda held at 1e12 and at 1e-12
  end_*        both ends of every parameter's accepted range, with a context, so that they reach the kernel
  scale_*      the translations times 2^k"""
import functools
import math
from collections import namedtuple

import numpy as np

import ba_cases as bc
import ba_ref as br
import ftrack_ref as fr

FILL = 0xEE
DEFAULT_CAM = (458.654, 457.296, 367.215, 248.375)                  # vis_default_params
WIDE_CAM = (300.0, 600.0, 100.0, 400.0)
TINY_CAM = (1e-3, 2e-3, 0.0, 0.0)
HUGE_CAM = (1e6, 2e6, -1e5, 1e5)
PROTO_CAM = (bc.CAM.fx, bc.CAM.fy, bc.CAM.cx, bc.CAM.cy)
MIN_NORMAL = 2.2250738585072014e-308
TRI_KW = dict(max_reproj_px=16.0, max_parallax_cos=1.0)            # the N-view triangulation with the adjustment's gate (the input poses are perturbed)

Case = namedtuple("Case", "rows cam kw reached")
Result = namedtuple("Result", "sc cam kw out win pts fl log stats live")


def camera(cam):
    return fr.Camera(*cam)


def _copy(sc):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in sc.items()}


def proto():
    return _copy(bc.scene(21, 9, 160))


def planted(cam):
    """the planted scene under its own camera"""
    return br.scene(21, camera(cam), n_cam=9, n_pts=160, span=(3, 9))


def reprojected(cam):
    """the prototype's pixels seen through another camera: x = (u - cx) / fx, then fx' x + cx' rounded to float"""
    sc, k = proto(), camera(cam)
    xy = sc["xy"].astype(np.float64)
    sc["xy"] = np.stack([k.fx * ((xy[..., 0] - bc.CAM.cx) / bc.CAM.fx) + k.cx, k.fy * ((xy[..., 1] - bc.CAM.cy) / bc.CAM.fy) + k.cy], -1).astype(np.float32)
    return sc


def scaled(k):
    sc = proto()
    sc["poses"][:, 9:] *= 2.0 ** k
    return sc


def near_point():
    """the scene at 2^-495 (every block finite) with one more track: a point 0.001 units in front of frame 4, seen from frames 3 and 4.  Ju Ju of
    its view from frame 4 overflows, so it alone sits out of every linearisation of window 0 and keeps its X, while its residual (458 px per 0.001
    units that frame 4 moves) turns steps down until the damping has made them small"""
    sc, s = scaled(-495), 2.0 ** -495
    P = sc["poses"][4]
    X = P[:9].reshape(3, 3).T @ (np.array([0.0003, 0.0002, 0.001]) * s - P[9:])
    pk = -1
    for f in (3, 4):
        P, q = sc["poses"][f], int(sc["nkp"][f])
        xc = P[:9].reshape(3, 3) @ X + P[9:]
        sc["xy"][f, q] = (bc.CAM.fx * xc[0] / xc[2] + bc.CAM.cx, bc.CAM.fy * xc[1] / xc[2] + bc.CAM.cy)
        sc["obs"][f, q] = (-1, -1, 0, pk)
        sc["nkp"][f], pk = q + 1, q
    return sc


def coincident():
    sc = proto()
    sc["poses"][4, 9:] = 0.0                                        # frame 4's centre is frame 0's: the input span of window 0 is zero
    return sc


# ---------------------------------------------------------------------------------------------- what a result must show
def whats(r, j=None):
    return [w for jj, _, w in r.log if j is None or jj == j]


def sitouts(r, j=None):
    return [s for jj, _, s in r.stats if j is None or jj == j]


def unchanged(r):
    return r.out.tobytes() == np.asarray(r.sc["poses"], np.float64).tobytes()


def refined(r):
    return (r.win["flags"] == br.BA_REFINED).all() and (r.win["n_accepted"] > 0).all() and (r.win["cost1"] < r.win["cost0"]).all()


def halves(r):
    ein, eout = br.relative_errors(r.sc["poses"], r.sc["truth"]), br.relative_errors(r.out, r.sc["truth"])
    return eout[0] <= 0.5 * ein[0] and eout[1] <= 0.5 * ein[1]


def all_rejected_at_the_gate(r):
    f = r.fl[r.live]
    return (f == br.BAP_INIT_REJECTED).any() and not (f == br.BAP_USED).any() and (r.win["flags"] == br.BA_FEW).all() and \
        (r.win["n_points"] == 0).all() and (r.win["cost0"] == 0.0).all() and (r.win["cost1"] == 0.0).all() and unchanged(r)


def some_sit_out_while_steps_are_accepted(r):
    return any(0 < s < int(r.win[j]["n_points"]) and int(r.win[j]["n_accepted"]) > 0 for j, _, s in r.stats) and \
        (r.win["flags"] == br.BA_REFINED).all()


def a_solved_step_with_a_point_sitting_out(r):
    """the camera system is solved while a point sits out: the candidate's cost (a rejection) and the accepted step's write both meet that point"""
    mixed = [w for (j, _, s), (_, _, w) in zip(r.stats, r.log) if 0 < s < int(r.win[j]["n_points"])]
    return "accept" in mixed and "reject" in mixed and (r.win["flags"] == br.BA_REFINED).all()


def points_sit_out_of_every_linearisation(r, whole):
    """no linearisation without a sit-out, so none is solved (whole: and in one of them EVERY point of the window sits out)"""
    return len(r.stats) == 20 and all(s > 0 for s in sitouts(r)) and whats(r) == ["pivot"] * 20 and (r.win["cost1"] == r.win["cost0"]).all() and \
        (r.win["flags"] == br.BA_REFINED).all() and (r.win["n_rejected"] == 10).all() and unchanged(r) and \
        (not whole or any(s == int(r.win[j]["n_points"]) for j, _, s in r.stats))


def denormal_weights(r):
    """every weight huber / e is a denormal number (e > 1 px wherever the linear branch is taken) and the cost is some 3e-307"""
    return r.kw["huber_px"] < MIN_NORMAL and (r.win["cost0"] > 0.0).all() and (r.win["cost0"] < 1e-300).all() and (r.win["cost1"] > 0.0).all() and \
        "accept" in whats(r) and "pivot" in whats(r)


def no_scale(r):
    w0, w1 = r.win[0], r.win[1]
    return int(w0["flags"]) == br.BA_REFINED | br.BA_NO_SCALE and int(w0["n_accepted"]) > 0 and float(w0["scale"]) == 1.0 and \
        int(w1["flags"]) == br.BA_REFINED and float(w1["scale"]) != 1.0


def upper_clamp(r):
    return whats(r) == ["pivot"] * 10 and float(r.win[0]["lambda_"]) == 1e12 and int(r.win[0]["n_rejected"]) == 10


def lower_clamp_from_the_start(r):
    """lambda0 = 1e-12: a first step that is accepted leaves lambda AT the clamp (1e-13 is below it)"""
    return (r.win["n_lin"] == 30).all() and any(whats(r, j)[0] == "accept" for j in range(2)) and "reject" in whats(r) and \
        (r.win["flags"] == br.BA_REFINED).all()


def lower_clamp_at_the_end(r):
    return (r.win["lambda_"] == 1e-12).all() and all(whats(r, j)[-1] == "accept" for j in range(2))


def seventeen_views(r):
    used = r.pts[r.fl == br.BAP_USED]
    return int(r.win[0]["flags"]) == br.BA_REFINED and int(r.win[0]["n_points"]) == len(used) > 0 and (used["n_views"] == 17).all() and \
        int(r.win[0]["n_free"]) == 16 and int(r.win[1]["flags"]) == br.BA_FEW


def few_by_the_gate(r):
    return (r.win["flags"] == br.BA_FEW).all() and 0 < int(r.win["n_points"].max()) < 12 and (r.fl[r.live] == br.BAP_INIT_REJECTED).sum() > 100 and \
        unchanged(r)


def solved_below_twelve_points(r):
    """min_points = 1: the window that has points is solved, the one without any is still VIS_BA_FEW"""
    return all(int(w["flags"]) == (br.BA_REFINED if w["n_points"] > 0 else br.BA_FEW) for w in r.win) and 0 < int(r.win["n_points"].max()) < 12 and \
        len(r.log) == 10 * int((r.win["n_points"] > 0).sum()) > 0


def differs_from(name, field="cost0"):
    return lambda r: refined(r) and (r.win[field] != restated(name).win[field]).all()


def huber_bites(r):
    """a Huber width of 0.1 px: most observations are on the linear branch, so the cost is below plain squares'"""
    return (r.win["flags"] == br.BA_REFINED).all() and (r.win["cost0"] < 0.5 * restated("plain").win["cost0"]).all()


def huber_never_bites(r):
    p = restated("plain")
    return whats(r) == whats(p) and r.win.tobytes() == p.win.tobytes() and r.out.tobytes() == p.out.tobytes()


def falls_from_the_upper_clamp(r):
    return whats(r) == ["accept"] * 20 and (r.win["lambda_"] < 1e3).all() and (r.win["lambda_"] > 10.0).all()


S4 = dict(stride=4)
CASES = {
    "aniso_default": Case(lambda: planted(DEFAULT_CAM), DEFAULT_CAM, S4, lambda r: refined(r) and halves(r) and "reject" in whats(r)),
    "aniso_wide": Case(lambda: planted(WIDE_CAM), WIDE_CAM, S4, lambda r: refined(r) and halves(r) and "reject" in whats(r)),
    "aniso_tiny": Case(lambda: reprojected(TINY_CAM), TINY_CAM, S4, refined),
    "aniso_huge": Case(lambda: reprojected(HUGE_CAM), HUGE_CAM, S4, all_rejected_at_the_gate),
    "sitout_mixed": Case(lambda: scaled(-502), PROTO_CAM, S4, some_sit_out_while_steps_are_accepted),
    "sitout_one_point": Case(near_point, PROTO_CAM, S4, a_solved_step_with_a_point_sitting_out),
    "sitout_all_scale": Case(lambda: scaled(-506), PROTO_CAM, S4, lambda r: points_sit_out_of_every_linearisation(r, True)),
    "sitout_all_huber": Case(proto, PROTO_CAM, dict(stride=4, huber_px=5e-324), lambda r: points_sit_out_of_every_linearisation(r, False)),
    "denormal": Case(proto, PROTO_CAM, dict(stride=4, huber_px=1e-310), denormal_weights),
    "no_scale": Case(coincident, PROTO_CAM, dict(stride=4, init_reproj_px=1e6), no_scale),
    "clamp_upper": Case(bc.pivot_case, PROTO_CAM, dict(lambda0=1e12), upper_clamp),
    "clamp_lower_start": Case(proto, PROTO_CAM, dict(stride=4, lambda0=1e-12, lm_iters=30), lower_clamp_from_the_start),
    "clamp_lower_end": Case(lambda: bc.scene(7, 9, 120, noise=1.0), PROTO_CAM, S4, lower_clamp_at_the_end),
    "end_min_views": Case(lambda: bc.chain(3, 18, 40, 64), PROTO_CAM, dict(stride=16, min_views=17, lm_iters=3), seventeen_views),
    "end_gn_0": Case(proto, PROTO_CAM, dict(stride=4, tri_gn_iters=0, init_reproj_px=1e6), differs_from("wide_gate")),
    "end_gn_10": Case(proto, PROTO_CAM, dict(stride=4, tri_gn_iters=10), refined),
    "end_gate_half": Case(proto, PROTO_CAM, dict(stride=4, init_reproj_px=0.5), few_by_the_gate),
    "end_gate_half_one_point": Case(proto, PROTO_CAM, dict(stride=4, init_reproj_px=0.5, min_points=1), solved_below_twelve_points),
    "end_huber_small": Case(proto, PROTO_CAM, dict(stride=4, huber_px=0.1), huber_bites),
    "end_huber_max": Case(proto, PROTO_CAM, dict(stride=4, huber_px=1.7976931348623157e308), huber_never_bites),
    "end_lambda_max": Case(proto, PROTO_CAM, dict(stride=4, lambda0=1e12), falls_from_the_upper_clamp),
    "scale_m500": Case(lambda: scaled(-500), PROTO_CAM, S4, refined),
    "scale_m300": Case(lambda: scaled(-300), PROTO_CAM, S4, refined),
    "scale_p300": Case(lambda: scaled(300), PROTO_CAM, S4, refined),
    "scale_p500": Case(lambda: scaled(500), PROTO_CAM, S4, refined),
    "scale_m600": Case(lambda: scaled(-600), PROTO_CAM, S4, all_rejected_at_the_gate),
    "scale_p600": Case(lambda: scaled(600), PROTO_CAM, S4, all_rejected_at_the_gate),
    "scale_p1000": Case(lambda: scaled(1000), PROTO_CAM, S4, all_rejected_at_the_gate),
}
# runs that only serve as the other side of a comparison
BASES = {
    "plain": Case(proto, PROTO_CAM, dict(stride=4, huber_px=0.0), refined),
    "wide_gate": Case(proto, PROTO_CAM, dict(stride=4, init_reproj_px=1e6), refined),
}


def run(sc, cam, **kw):
    """the restatement on the rows sc, its outputs pre-filled with 0xEE as the device tests pre-fill theirs"""
    n, R = sc["obs"].shape
    log, stats = [], []
    fill_p = np.full(n * R * 40, FILL, np.uint8).view(br.POINT_DTYPE).reshape(n, R)
    out, win, pts, fl = br.ba_rows(br.Params(**kw), camera(cam), sc["prev"], sc["nkp"], sc["obs"], sc["xy"], sc["poses"], fill_p,
                                   np.full((n, R), FILL, np.uint8), log, stats)
    live = np.arange(R)[None, :] < fr.counts(sc["prev"], sc["nkp"], R)[:, None]
    return Result(sc, cam, kw, out, win, pts, fl, log, stats, live)


@functools.lru_cache(maxsize=None)
def restated(name):
    """computed once per process and shared: nothing may write into it"""
    c = CASES.get(name) or BASES[name]
    r = run(c.rows(), c.cam, **c.kw)
    for a in (r.out, r.win, r.pts, r.fl):
        a.setflags(write=False)
    return r


def swapped(cam):
    return (cam[1], cam[0], cam[2], cam[3])


def finite(r):
    return bc.all_finite(r.sc["poses"], r.out, r.win, r.pts[r.live]) and all(math.isfinite(float(v)) for v in r.out.reshape(-1))
