"""CPU: the restatement of the homography pose (tests/homography_pose_ref.py) on the 48 cases of homography_ref.H_LIST x M 40 / 300 x noise
0 / 0.3 px x outliers 0 / 25 %, H and mask from homography_ref.homography with make_draws(7): the classification, the invariants of every
candidate, the truth on the planes without noise, and what a rotation hint decides.

Tolerances come from the independent method (numpy.linalg.svd + the closed form) on the same cases, times 100; the figures both methods
reach are printed (pytest -s) and recorded in DESIGN.md section 4.11."""
import numpy as np
import pytest

import homography_pose_ref as hp
import homography_ref as hr


@pytest.fixture(scope="module")
def cases():
    """per case: dict(key, H record, mask, x1, x2, dec, rec (no hint), rec_hint, truth, svd candidates)"""
    cam, hq, hh, draws = hr.Camera(), hp.default_params(), hr.default_params(), hr.make_draws(7)
    out = []
    for cls, m, noise, outl in hp.table_cases():
        x1, x2, _ = hr.make_rows(cls, m, noise, outl)
        hrec, mask = hr.homography(cam, hh, x1, x2, draws)
        assert int(hrec["best_iter"]) >= 0
        dec = hp.decompose(hrec["H"], hq.min_t_over_d)
        c = dict(key=(cls, m, noise, outl), hrec=hrec, mask=mask, x1=x1, x2=x2, dec=dec, truth=hp.truth(cls, m, noise))
        table = hp.vote_table(dec, hr.normalise(cam, x1, x2), hq.max_cos_parallax) if dec["kind"] == hp.HP_PLANE else None
        c["rec"] = hp.hpose(cam, hq, hrec, x1, x2, mask, None, table)
        c["rec_hint"] = hp.hpose(cam, hq, hrec, x1, x2, mask, np.asarray(c["truth"][0].T, np.float32), table)
        c["svd"] = hp.decompose_svd(hrec["H"])
        out.append(c)
    return out


def _planes(cases):
    return [c for c in cases if c["key"][0] in hp.PLANE_LIST]


def test_classification(cases):
    rot = [float(c["rec"]["t_norm"]) for c in cases if c["key"][0] in hp.ROTATION_LIST]
    pla = [float(c["rec"]["t_norm"]) for c in _planes(cases)]
    print(f"t_norm: rotation classes {min(rot):.3e} ... {max(rot):.3e}, plane classes {min(pla):.3e} ... {max(pla):.3e}")
    assert len(rot) == 32 and len(pla) == 16
    for c in cases:
        want = hp.HP_PLANE if c["key"][0] in hp.PLANE_LIST else hp.HP_ROTATION
        assert int(c["rec"]["kind"]) == want, (c["key"], float(c["rec"]["t_norm"]))
    d = hp.default_params().min_t_over_d
    assert max(rot) * 1.5 <= d <= min(pla) / 1.5                   # the default sits a factor 1.5 from both lists


def test_rotation_only_records(cases):
    worst = 0.0
    for c in cases:
        r = c["rec"]
        if int(r["kind"]) != hp.HP_ROTATION:
            continue
        assert int(r["solution"]) == 0 and int(r["second"]) == -1 and int(r["flags"]) == 0 and int(r["n_tested"]) == 0
        assert not r["t"].any() and not r["n"].any() and not r["R2"].any() and not r["n_good"].any()
        R = r["R"].reshape(3, 3)
        assert np.abs(R.T @ R - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(R) - 1) < 1e-12
        if c["key"][2] == 0.0 and c["key"][0] != "shift":              # (a pixel shift is no rotation: it has no true R)
            worst = max(worst, hp.rot_angle_deg(R, c["truth"][0]))
    print(f"rotation-only, noise 0: worst angle to the true R {worst:.3e} deg")
    # (printed for DESIGN.md, not bounded: the H is one four-point sample's, and rot / M 40 draws a badly conditioned one: 7e-2 deg)


def test_invariants_of_every_candidate(cases):
    ours, ref = [0.0] * 4, [0.0] * 4
    for c in _planes(cases):
        dec, H = c["dec"], c["hrec"]["H"]
        cands = [hp.candidate(dec, k) for k in range(4)]
        ours = [max(a, b) for a, b in zip(ours, hp.residuals(H, dec["sv"][1], cands))]
        sv, sc = c["svd"]
        assert len(sc) == 4
        ref = [max(a, b) for a, b in zip(ref, hp.residuals(H, sv[1], sc))]
        for a, b in ((3, 0), (2, 1)):                                 # exactly: the same R, t and n negated
            assert cands[a][0] == cands[b][0] and cands[a][1] == [-v for v in cands[b][1]] and cands[a][2] == [-v for v in cands[b][2]]
        assert np.abs(np.array(dec["sv"]) - sv).max() <= 1e-12
    names = ("R^T R - I", "det R - 1", "|n| - 1", "d2 (R + t n^T) - H")
    for nm, a, b in zip(names, ours, ref):
        print(f"{nm}: restatement {a:.3e}, independent method {b:.3e}, bound {100 * b:.3e}")
        assert a <= 100 * b, nm


def test_truth_on_the_planes_without_noise(cases):
    ours, ref = [0.0] * 4, [0.0] * 4
    for c in _planes(cases):
        if c["key"][2] != 0.0:
            continue
        r = c["rec"]
        two = [(r["R"], r["t"], r["n"]), (r["R2"], r["t2"], r["n2"])]
        e = min((hp.truth_errors(cd, c["truth"]) for cd in two), key=lambda v: v[0])
        ours = [max(a, b) for a, b in zip(ours, e)]
        e = min((hp.truth_errors(cd, c["truth"]) for cd in c["svd"][1]), key=lambda v: v[0] + v[1])
        ref = [max(a, b) for a, b in zip(ref, e)]
    for nm, a, b in zip(("R deg", "t deg", "n deg", "|t|/d rel"), ours, ref):
        print(f"truth, noise 0, {nm}: chosen-or-second {a:.3e}, independent method's best candidate {b:.3e}, bound {100 * b:.3e}")
        assert a <= 100 * b, nm


def test_hint_decides_and_flags(cases):
    n_rival = 0
    for c in _planes(cases):
        r, rh = c["rec"], c["rec_hint"]
        g = [int(v) for v in r["n_good"]]
        rival = sorted(g)[-2] >= hp.default_params().ambiguity_ratio * max(g)
        n_rival += rival
        assert bool(int(r["flags"]) & hp.HPF_AMBIGUOUS) == rival and not int(r["flags"]) & hp.HPF_HINTED, c["key"]
        assert bool(int(rh["flags"]) & hp.HPF_HINTED) == rival and not int(rh["flags"]) & hp.HPF_AMBIGUOUS, c["key"]
        assert rh["n_good"].tobytes() == r["n_good"].tobytes()
        errs = [hp.truth_errors(hp.candidate(c["dec"], k), c["truth"]) for k in range(4)]
        true_k = min(range(4), key=lambda k: errs[k][0] + errs[k][1])
        assert int(rh["solution"]) == true_k, (c["key"], g, errs)
        e, e2 = errs[int(rh["solution"])], errs[int(rh["second"])]
        print(f"{c['key']}: votes {g} par {int(rh['n_parallax'])} chosen {int(rh['solution'])} R {e[0]:.2e} t {e[1]:.2e} deg |t|/d {e[3]:.1e}; "
              f"second {int(rh['second'])} R {e2[0]:.2e} t {e2[1]:.2e} deg; no hint: {int(r['solution'])} flags {int(r['flags'])}")
    print(f"{n_rival} of 16 plane cases have a rival")
    assert n_rival >= 8                                               # the two-fold ambiguity is the normal case


def test_planted_planes(cases):
    """planes of other normals and distances: H from the four-point solver on exact correspondences, the truth among chosen and second"""
    cam, hq = hr.Camera(), hp.default_params()
    for seed in range(4):
        R, td, n, x1, x2 = hp.planted_plane(seed, 24)
        hrec, mask = hr.homography(cam, hr.default_params(), x1, x2, hr.make_draws(7))
        r = hp.hpose(cam, hq, hrec, x1, x2, mask, np.asarray(R.T, np.float32))
        assert int(r["kind"]) == hp.HP_PLANE and int(r["n_good"][int(r["solution"])]) == int(mask.sum())
        e = hp.truth_errors((r["R"], r["t"], r["n"]), (R, td, n))
        assert e[0] < 0.05 and e[1] < 1.0 and e[2] < 1.0 and e[3] < 0.02, (seed, e)      # float32 pixels: 1e-5 px of 458 -> these angles


def test_refused_inputs_give_the_zero_record():
    cam, hq = hr.Camera(), hp.default_params()
    x = np.zeros((5, 2), np.float32)
    h = hr.zero_record()
    assert hp.hpose(cam, hq, h, x, x).tobytes() == hp.zero_record().tobytes()          # best_iter = -1
    h["best_iter"], h["H"] = 3, np.eye(3).reshape(9)
    assert hp.hpose(cam, hq, h, x[:0], x[:0]).tobytes() == hp.zero_record().tobytes()  # no correspondences
    h["H"][4] = np.inf
    assert hp.hpose(cam, hq, h, x, x).tobytes() == hp.zero_record().tobytes()          # H not finite
    for Hd in (np.zeros(9), np.outer([1.0, 2.0, 3.0], [0.5, -1.0, 2.0]).reshape(9)):   # rank 0 and rank 1: d2 == 0, t_norm not finite
        h["H"] = Hd
        assert hp.hpose(cam, hq, h, x, x).tobytes() == hp.zero_record().tobytes()
    z = hp.zero_record()
    assert int(z["solution"]) == int(z["second"]) == -1 and int(z["kind"]) == hp.HP_NONE and hp.RESULT_DTYPE.itemsize == 320
