"""The one world of the chain tests (CPU: test_vi_chain_ref.py; GPU: test_vi_chain_gpu.py): static 3-D points, a camera and an IMU moving through them
on the two-axis motion of tests/vi_align_ba_cases.py, pixels of those points and IMU samples of that same motion -- and THE CHAIN, written once for
both sides: essential RANSAC + recoverPose -> triangulation -> scale links -> trajectory -> preintegration with Jacobians -> alignment with the
accelerometer bias -> correction -> alignment again, every record handed on as the stage before wrote it.  A BACKEND supplies the stages: Cpu below
(the oracle and the restatements), and the device one of test_vi_chain_gpu.py (the library's bindings on device pointers).

THE SCENE.  40 frames at 20 frames/s from T0 + START, 200 Hz samples with both planted biases (vis_imu_params' bg = ba = 0, so the true steps are
the planted biases).  The baselines are 0.064 ... 0.10 m a frame.  recoverPose's cheirality vote and VIS_MP_FRONT -- so VIS_MP_KEPT, the scale links'
default `require` -- count a point only below 50 baselines, here 3.2 ... 5 m: a shell at 6 ... 10 m leaves the vote without a single point and the
links without a depth, so the points fill a shell of R_IN ... R_OUT metres around the middle of the path.  Pixels are the
projections with fx for both axes (the contexts of these tests have fy = fx), rounded to float, no other noise.  The keypoint index is the point's
id; a pair's row holds the MAX_PTS lowest ids both frames see (the highest from the thinned pair of `thin` on).

TRUTH is expressed in the chain's own gauge: the frame of the root camera, one trajectory unit = the metric length of the unit edge of the epoch
over the sigma it was held at (truth())."""
import math

import numpy as np

import essential_polish_ref as epr
import essential_refine_ref as er
import imu_cases as ic
import imu_jac_ref as jr
import imu_ref as ir
import scale_link_ref as sl
import trajectory_ref as tj
import triangulate_ref as tri
import vi_align_ba_cases as bc
import vi_align_ba_ref as br
import vi_align_cases as vc
import vi_align_ref as vr

N, FPS, HZ = 40, 20.0, 200.0
START = 1.0                                                           # seconds after T0: every baseline of `chain` is above 0.06 m
MIN_BASELINE = 0.03
W, H = 752, 480
N_PTS, R_IN, R_OUT, SEED = 6000, 2.0, 4.0, 20
MAX_PTS = 192                                                         # correspondences per pair (rows may hold 512)
ROW_CAP = N_PTS
SCENARIOS = ("chain", "gated", "lost", "thin", "cut")
LOST_AT, THIN_AT, THIN_KEEP = 12, 12, 3
CUTS = dict(chain=(N,), gated=(N,), lost=(10, 30), thin=(N,), cut=(23, 17))
GYRO_BIAS, ACC_BIAS = bc.GYRO_BIAS, bc.ACC_BIAS
VP, BP = vc.params(), br.BaParams()
IP = ir.Params(r_ic=vc.R_IC)                                          # bg = ba = 0
SP = sl.Params()                                                      # the defaults: require = VIS_MP_KEPT

FILL = 0xEE                                                           # what the device test fills its outputs with: a mask row without a pose keeps it

_cache = {}


def camera():
    """the intrinsics of the context: the library's default fx, cx, cy, with fy = fx"""
    if "cam" not in _cache:
        import vislam
        p = vislam.default_params()
        p.fy = p.fx
        _cache["cam"] = p
    return _cache["cam"]


def world():
    """dict(times, R (n, 3, 3) world -> camera, P (n, 3) camera centres, Pimu, Vimu, X (N_PTS, 3), xy (n, N_PTS, 2) float32, seen (n, N_PTS) bool,
    samples)"""
    if "world" in _cache:
        return _cache["world"]
    p = camera()
    times = np.asarray([vc.T0 + START + i / FPS for i in range(N)], np.float64)
    poses = [bc.camera_pose(float(t)) for t in times]
    R = np.asarray([po[0] for po in poses]).reshape(N, 3, 3)
    P = np.asarray([po[1] for po in poses])
    rng = np.random.default_rng(SEED)
    d = rng.normal(0, 1, (N_PTS, 3))
    r = np.cbrt(rng.uniform(R_IN ** 3, R_OUT ** 3, N_PTS))
    X = P.mean(0) + d / np.linalg.norm(d, axis=1)[:, None] * r[:, None]
    xy, seen = np.zeros((N, N_PTS, 2), np.float32), np.zeros((N, N_PTS), bool)
    for i in range(N):
        Xc = (X - P[i]) @ R[i].T
        with np.errstate(all="ignore"):
            u, v = p.fx * Xc[:, 0] / Xc[:, 2] + p.cx, p.fx * Xc[:, 1] / Xc[:, 2] + p.cy
        xy[i] = np.stack([u, v], 1).astype(np.float32)
        seen[i] = (Xc[:, 2] > 0.1) & (u >= 0) & (u <= W - 1) & (v >= 0) & (v <= H - 1)
    samples = ic.samples_between(float(times[0]) - 0.05, float(times[-1]) + 2.0 / HZ, HZ, bc.body_rate(GYRO_BIAS, ACC_BIAS), 0.11)
    w = dict(times=times, R=R, P=P, X=X, xy=xy, seen=seen, samples=samples,
             Pimu=np.asarray([vc.motion(float(t))[0] for t in times]), Vimu=np.asarray([vc.motion(float(t))[1] for t in times]))
    _cache["world"] = w
    return w


def scenario(name):
    """dict(name, prev, cuts, p1, p2 (n, MAX_PTS, 2) float32 with NaN behind a row's count, npts, links (n, MAX_PTS) DMATCH, nlinks, ids)"""
    if ("sc", name) in _cache:
        return _cache["sc", name]
    w = world()
    prev = ic.pairing("alternate" if name == "gated" else "chain", N)
    p1, p2 = np.full((N, MAX_PTS, 2), np.nan, np.float32), np.full((N, MAX_PTS, 2), np.nan, np.float32)
    npts, links, ids = np.zeros(N, np.int32), np.zeros((N, MAX_PTS), sl.DMATCH_DTYPE), [np.zeros(0, np.int64)] * N
    for i in range(N):
        q = int(prev[i])
        if q < 0:
            continue
        both = np.nonzero(w["seen"][q] & w["seen"][i])[0]
        sel = both[:MAX_PTS]
        if name == "thin" and i >= THIN_AT:                          # the highest ids; the thinned pair keeps THIN_KEEP points of its parent pair
            sel = both[-MAX_PTS:]
            if i == THIN_AT:
                fresh = both[~np.isin(both, ids[q])]
                sel = np.sort(np.concatenate([fresh[-(MAX_PTS - THIN_KEEP):], ids[q][np.isin(ids[q], both)][:THIN_KEEP]]))
        if name == "lost" and i == LOST_AT:
            sel = both[:4]
        m = len(sel)
        ids[i], npts[i] = sel, m
        p1[i, :m], p2[i, :m] = w["xy"][q][sel], w["xy"][i][sel]
        links[i, :m]["queryIdx"] = links[i, :m]["trainIdx"] = sel
    sc = dict(name=name, prev=prev, cuts=CUTS[name], p1=p1, p2=p2, npts=npts, links=links, nlinks=npts.copy(), ids=ids)
    _cache["sc", name] = sc
    return sc


def localise(prev, a, b):
    """vi_align_cases.localise for the pairing alone"""
    before = [i for i in range(a) if ir.norm_prev(prev, i) != ir.KF_NOT_SAVED]
    last = before[-1] if before else None
    out = []
    for i in range(a, b):
        q = ir.norm_prev(prev, i)
        out.append(q - a if q >= a else (q if q < 0 else (ir.KF_CARRIED if q == last else ir.KF_FIRST)))
    return np.asarray(out, np.int32)


# ---------------------------------------------------------------------------------------------- the chain
STAGES = ("pose0", "mask0", "polish", "pose", "mask", "points", "flags", "depth", "link", "traj", "delta", "jac", "imu_carry", "state1", "res1", "ba_carry1", "delta2", "status",
          "state2", "res2", "ba_carry2")


def run_chain(be, sc, w=None):
    """the chain of the module's docstring over the scenario's calls; `be` is the backend.  Returns one dict of handles per call (be.fetch turns
    them into records after be.sync()) -- the handles of a call are the inputs of the next stage as they stand, and the carries of the next call:
    the depth row and the trajectory record of the last saved frame (pointers into the rows), the IMU carry and the two alignments' carries.
    The pose record fed on is the one vis_essential_polish_batch writes (d_pose_out), with the mask it wrote: RANSAC's own record is the exact
    solution of five correspondences, which at these baselines (10 px of parallax) is 0.2 rad off in the direction of t on pixels rounded to
    float -- the polish over all inliers is the step that makes a pose of it."""
    w = world() if w is None else w
    calls, at = [], 0
    carry = dict(depth=None, traj=None, imu=None, ba1=None, ba2=None)
    for m in sc["cuts"]:
        a, b = at, at + m
        prev = localise(sc["prev"], a, b)
        h = dict(prev=prev, seq0=a, n=m)
        p1, p2, npts = sc["p1"][a:b], sc["p2"][a:b], sc["npts"][a:b]
        d_prev = be.upload(prev)
        h["pose0"], h["mask0"] = be.essential(p1, p2, npts)
        h["polish"], h["pose"], h["mask"] = be.polish(h["pose0"], h["mask0"], p1, p2, npts)
        h["points"], h["flags"] = be.triangulate(h["pose"], h["mask"], p1, p2, npts)               # (the one host step)
        h["depth"], h["link"] = be.scale_link(d_prev, sc["links"][a:b], sc["nlinks"][a:b], h["pose"], h["points"], h["flags"], carry["depth"], m)
        h["traj"] = be.trajectory(d_prev, h["pose"], h["link"], carry["traj"], a, m)
        h["delta"], h["jac"], h["imu_carry"] = be.imu(w["samples"], w["times"][a:b], d_prev, carry["imu"], m)
        h["state1"], h["res1"], h["ba_carry1"] = be.align(d_prev, h["traj"], h["delta"], h["jac"], carry["ba1"], m)
        h["delta2"], h["status"] = be.correct(h["delta"], h["jac"], h["res1"], m)
        h["state2"], h["res2"], h["ba_carry2"] = be.align(d_prev, h["traj"], h["delta2"], h["jac"], carry["ba2"], m)
        saved = [i for i in range(m) if ir.norm_prev(prev, i) != ir.KF_NOT_SAVED]
        assert saved, "a call of these scenarios saves a frame"
        carry = dict(depth=be.part(h["depth"], saved[-1], ROW_CAP * 8), traj=be.part(h["traj"], saved[-1], 128), imu=h["imu_carry"],
                     ba1=h["ba_carry1"], ba2=h["ba_carry2"])
        calls.append(h)
        at = b
    return calls


def pose_record(E, R, t, ninl, ngood, iters, m):
    r = np.zeros(1, sl.POSE_DTYPE)[0]
    if np.asarray(E).any():
        r["E"], r["R"], r["t"], r["n_pose_good"] = np.asarray(E).reshape(9), np.asarray(R).reshape(9), t, ngood
    r["n_inliers"], r["iters_run"], r["n_points"] = ninl, iters, m
    return r


class Cpu:
    """the stages by the oracle (pose) and the restatements (everything behind it); handles are the numpy records themselves.  poses: the
    (records, masks) of every call to use in the place of the oracle's -- the device's own, for the byte comparison behind the pose stage.
    break_: a broken convention of test_vi_chain_ref's negative controls."""

    def __init__(self, poses=None, break_=None):
        self.poses, self.k, self.break_ = poses, 0, break_

    def upload(self, a):
        return a

    def fetch(self, h):
        return h

    def sync(self):
        pass

    def part(self, h, i, nbytes):
        return h[i:i + 1] if h.ndim == 1 else h[i]

    def essential(self, p1, p2, npts):
        if self.poses is not None:
            pose, mask = self.poses[self.k]
            self.k += 1
        else:
            import oracle_bind as orc
            p = camera()
            n = len(npts)
            pose, mask = np.zeros(n, sl.POSE_DTYPE), np.zeros((n, MAX_PTS), np.uint8)
            for i in range(n):
                m = int(npts[i])
                if m == 0:
                    continue
                key = ("pose", p1[i, :m].tobytes(), p2[i, :m].tobytes())
                if key not in _cache:
                    E, mk, ninl, iters = orc.essential_ransac(p, p1[i, :m], p2[i, :m])
                    R, t, ngood = orc.recover_pose(p, E, p1[i, :m], p2[i, :m]) if E.any() else (0, 0, 0)
                    _cache[key] = pose_record(E, R, t, ninl, ngood, iters, m), mk
                pose[i], mask[i, :m] = _cache[key]
        return pose, mask

    def polish(self, pose, mask, p1, p2, npts):
        p = camera()
        out, mo, po = epr.polish_rows(er.Camera(p.fx, p.cx, p.cy), epr.default_params(), pose, p1, p2, npts, mask, np.full_like(mask, FILL))
        if self.break_ == "t negated":
            po["t"] = -po["t"]
        return out, po, mo

    def triangulate(self, pose, mask, p1, p2, npts):
        p = camera()
        n = len(npts)
        pts, fl = np.zeros((n, MAX_PTS), sl.MAP_POINT_DTYPE), np.zeros((n, MAX_PTS), np.uint8)
        for i in range(n):
            m = int(npts[i])
            if m == 0 or not pose[i]["R"].any():
                continue
            key = ("tri", pose[i]["R"].tobytes(), pose[i]["t"].tobytes(), p1[i, :m].tobytes(), p2[i, :m].tobytes(), mask[i, :m].tobytes())
            if key not in _cache:
                _cache[key] = tri.triangulate(pose[i]["R"], pose[i]["t"], p1[i, :m], p2[i, :m], p.fx, p.fy, p.cx, p.cy, mask[i, :m])[:2]
            pts[i, :m], fl[i, :m] = _cache[key]
        return pts, fl

    def scale_link(self, prev, links, nlinks, pose, points, flags, carry, n):
        depth, link = sl.scale_link_rows(SP, prev, links, nlinks, pose, points, flags, ROW_CAP, carry)
        if self.break_ == "link scales inverted":
            ok = link["scale"] > 0
            link["scale"][ok] = 1.0 / link["scale"][ok]
        return depth, link

    def trajectory(self, prev, pose, link, carry, seq0, n):
        return tj.trajectory_rows(prev, pose, link, None if carry is None else carry[0], seq0)[0]

    def imu(self, samples, tframe, prev, carry, n):
        delta, jac, _, out = jr.preintegrate_jac_rows(IP, samples, tframe, prev, carry)
        return delta, jac, out

    def align(self, prev, traj, delta, jac, carry, n):
        P = VP
        if self.break_ == "r_ic transposed in the alignment":
            P = vc.params()
            P.r_ic = [VP.r_ic[3 * (k % 3) + k // 3] for k in range(9)]
        if self.break_ == "p_ci = 0":
            P = vc.params()
            P.p_ci = [0.0, 0.0, 0.0]
        return br.align_ba_rows(P, BP, prev, traj, delta, jac, carry)

    def correct(self, delta, jac, res, n):
        dba = np.asarray(res["dba"]).reshape(3)
        out, _, status = jr.correct_rows(IP, delta, jac, np.asarray(res["a"]["dbg"]).reshape(3), -dba if self.break_ == "dba applied with the opposite sign" else dba)
        return out, status


def records(be, calls):
    """the handles of every call as records (after be.sync())"""
    return [{k: (be.fetch(v) if k in STAGES else v) for k, v in h.items()} for h in calls]


def joined(recs, key):
    return np.concatenate([r[key] for r in recs])


# ---------------------------------------------------------------------------------------------- truth
def truth(sc):
    """the planted truth in the gauge the chain's LAST call must report in, from the scenario alone (nothing is read off a record): root = the root
    frame of the newest segment, first = the unit edge below it, edge = the unit edge of the newest epoch.
    dict(root, first, edge, s, g, Rroot, p (n, 3), v (n, 3), dbg, dba, C (n, 3) centres from the root in metres, s_first, base)"""
    w = world()
    root = LOST_AT if sc["name"] == "lost" else 0
    Rr, Pr = w["R"][root], w["P"][root]
    base = lambda i: float(np.linalg.norm(w["P"][i] - w["P"][int(sc["prev"][i])]))
    first = [i for i in range(root + 1, N) if int(sc["prev"][i]) == root][0]              # the unit edge below the root
    edge, sigma = (THIN_AT if sc["name"] == "thin" else first), 1.0
    if edge != first:                                                # a held scale: the edge has the sigma of its parent, b_parent / b_first
        sigma = base(int(sc["prev"][edge])) / base(first)
    s = base(edge) / sigma
    return dict(root=root, edge=edge, first=first, s=s, Rroot=Rr, g=Rr @ np.asarray(vc.GRAVITY), p=(w["Pimu"] - Pr) @ Rr.T, v=w["Vimu"] @ Rr.T,
                C=(w["P"] - Pr) @ Rr.T, dbg=np.asarray(GYRO_BIAS), dba=np.asarray(ACC_BIAS), s_first=base(first), base=base)


def _angle(Ra, Rb):
    """the angle of Ra Rb^T: from the skew part (sin) where it is small -- acos resolves no angle below 1e-8 --, from the trace beyond"""
    D = np.asarray(Ra, np.float64).reshape(3, 3) @ np.asarray(Rb, np.float64).reshape(3, 3).T
    sn = 0.5 * math.sqrt((D[2, 1] - D[1, 2]) ** 2 + (D[0, 2] - D[2, 0]) ** 2 + (D[1, 0] - D[0, 1]) ** 2)
    c = (np.trace(D) - 1.0) / 2.0
    return math.asin(min(1.0, sn)) if c > 0.9 else math.acos(max(-1.0, min(1.0, c)))


def ladder(sc, recs):
    """the errors of every hand-over against the planted truth, one number each (the largest over the frames that have the quantity):
    pose_R (rad), pose_t (the angle between the directions, rad), link (relative), centre (relative to the path's extent), delta_R (rad), delta_v
    (m/s), delta_p (m) against vi_align_ba_cases.closed_records; s1, g1, dbg1, dba1 (the first alignment), s, g, dbg, dba (after the correction:
    the second alignment's s_ba and g_ba, the two steps summed), p (m), v (m/s)"""
    w, T = world(), truth(sc)
    prev = sc["prev"]
    pose, link, traj, delta = (joined(recs, k) for k in ("pose", "link", "traj", "delta"))
    e = dict(pose_R=0.0, pose_t=0.0, link=0.0, centre=0.0)
    for i in range(N):
        q = int(prev[i])
        if q < 0 or not pose[i]["R"].any():
            continue
        Rt = w["R"][i] @ w["R"][q].T
        tt = w["R"][i] @ (w["P"][q] - w["P"][i])
        tt /= np.linalg.norm(tt)
        e["pose_R"] = max(e["pose_R"], _angle(pose[i]["R"], Rt))
        e["pose_t"] = max(e["pose_t"], float(np.linalg.norm(np.cross(pose[i]["t"], tt))) if float(np.dot(pose[i]["t"], tt)) > 0 else math.pi)
        if int(link[i]["flags"]) == sl.SL_OK:
            e["link"] = max(e["link"], abs(float(link[i]["scale"]) / (T["base"](i) / T["base"](q)) - 1.0))
    extent = float(np.abs(T["C"]).max())
    for i in range(N):                                               # the frames of the reported segment, up to a held scale: one gauge
        r = traj[i]
        if int(r["flags"]) & tj.TJ_NOT_SAVED or int(r["segment_seq"]) != T["root"] or (T["edge"] != T["first"] and i >= T["edge"]):
            continue
        R = r["R"].reshape(3, 3)
        C = -(R.T @ r["t"]) * T["s_first"]
        e["centre"] = max(e["centre"], float(np.abs(C - T["C"][i]).max()) / extent)
    # the deltas of the last call: the raw ones carry both planted biases, so v and p are compared with the closed forms under the planted accelerometer bias (what
    # is left is the gyro bias' share); the corrected ones (delta2) with the closed forms of the motion alone, R with Rw_q^T Rw_i
    biased, clean = (bc.closed_records(w["times"], prev, None, b)[0] for b in (ACC_BIAS, (0.0, 0.0, 0.0)))
    delta2 = joined(recs, "delta2")
    e.update(delta_raw_v=0.0, delta_R=0.0, delta_v=0.0, delta_p=0.0)
    for i in range(N):
        if int(delta[i]["flags"]) & jr.VOID_FLAGS:
            continue
        if i < N - recs[-1]["n"]:                                      # (an earlier call corrected its records by its own, earlier estimate)
            continue
        e["delta_raw_v"] = max(e["delta_raw_v"], float(np.abs(delta[i]["v"] - biased[i]["v"]).max()))
        e["delta_R"] = max(e["delta_R"], _angle(delta2[i]["R"], ir.tmul(bc.rw(float(w["times"][int(prev[i])])), bc.rw(float(w["times"][i])))))
        e["delta_v"] = max(e["delta_v"], float(np.abs(delta2[i]["v"] - clean[i]["v"]).max()))
        e["delta_p"] = max(e["delta_p"], float(np.abs(delta2[i]["p"] - clean[i]["p"]).max()))
    r1, r2 = recs[-1]["res1"], recs[-1]["res2"]
    e["s1"], e["g1"] = abs(float(r1["s_ba"]) / T["s"] - 1.0), float(np.abs(r1["g_ba"] - T["g"]).max())
    e["dbg1"], e["dba1"] = float(np.abs(r1["a"]["dbg"] - T["dbg"]).max()), float(np.abs(r1["dba"] - T["dba"]).max())
    e["s"], e["g"] = abs(float(r2["s_ba"]) / T["s"] - 1.0), float(np.abs(r2["g_ba"] - T["g"]).max())
    e["dbg"] = float(np.abs(r1["a"]["dbg"] + r2["a"]["dbg"] - T["dbg"]).max())
    e["dba"] = float(np.abs(r1["dba"] + r2["dba"] - T["dba"]).max())
    st = joined(recs, "state2")
    has_p = [i for i in range(N) if int(st[i]["flags"]) & vr.VIS_HAS_P and i >= N - recs[-1]["n"]]
    a = has_p[0]
    absolute = T["edge"] == T["first"]                                # the epoch starts below the root: positions from the root camera centre
    e["p"] = max(float(np.abs((st[i]["p"] - (0.0 if absolute else st[a]["p"])) - (T["p"][i] - (0.0 if absolute else T["p"][a]))).max()) for i in has_p)
    e["v"] = max(float(np.abs(st[i]["v"] - T["v"][i]).max()) for i in has_p if int(st[i]["flags"]) & vr.VIS_HAS_V)
    return e
