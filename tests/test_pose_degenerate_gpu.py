"""GPU: essential-matrix RANSAC and recoverPose on degenerate geometry (tests/pose_degenerate_cases.py) against the CPU oracle.

What is compared follows what was measured on two differently-rounded builds of the oracle (tests/golden/pose_degenerate_spread.json,
tools/pose_conditioning.py): inlier mask, inlier count and iterations run are identical everywhere; recoverPose of a GIVEN E agrees
to 1e-9 everywhere; E itself is compared entry by entry (1e-9) only where the two builds agreed to 1e-11, and everywhere it is held to
what it claims -- its mask is its own Sampson test, and it is an essential matrix as nearly as the oracle's own E of that case
(pose_degenerate_cases.check_model; tests/test_pose_degenerate_ref.py pins those invariants on the oracle and says for which classes
the essential-matrix bound is vacuous: static, rot, far, shift)."""
import numpy as np
import pytest

import pose_degenerate_cases as pdc

pytestmark = pytest.mark.gpu
TOL = 1e-9
SPREAD = pdc.load_spread()
KEPT = pdc.kept_cases(SPREAD)


@pytest.mark.parametrize("cls,m,noise,mode", KEPT, ids=[pdc.case_key(*c) for c in KEPT])
def test_essential_ransac_on_degenerate_geometry(vislam, orc, ctx, cls, m, noise, mode):
    p = pdc.set_mode(vislam.default_params(), mode)
    ctx.set_params(p)
    x1, x2 = pdc.make_case(cls, m, noise)
    E, mask, ninl, iters = ctx.essential_ransac(x1, x2)
    oE, omask, oninl, oiters = orc.essential_ransac(p, x1, x2)
    print(f"gpu ({ninl}, {iters}) oracle ({oninl}, {oiters}) mask bits off {int((mask != omask).sum())} dE {pdc.cmp_E(E, oE):.3e} "
          f"recorded spread {SPREAD[pdc.case_key(cls, m, noise, mode)]['spread']:.3e}")
    assert (ninl, iters) == (oninl, oiters)
    assert (mask == omask).all()
    assert np.isfinite(E).all()
    if oninl == 0:
        assert np.abs(E).max() == 0 and not mask.any() and iters == 0
        return
    if pdc.is_e_stable(SPREAD[pdc.case_key(cls, m, noise, mode)]):
        assert pdc.cmp_E(E, oE) <= TOL
    fig = pdc.check_model(E, mask, ninl, x1, x2, p, oE)
    print(fig)
    Rg, tg, ng = ctx.recover_pose(oE, x1, x2)
    Ro, to, no = orc.recover_pose(p, oE, x1, x2)
    assert ng == no
    assert np.abs(Rg - Ro).max() <= TOL and np.abs(tg - to).max() <= TOL


# ---- recoverPose in exact arithmetic: the theta == 0 fallback of cheirality_pair, directed and rank-deficient E ----------------------
def _same_pose(got, ref, tol):
    (Rg, tg, ng), (Ro, to, no) = got, ref
    assert ng == no, (ng, no)
    for a, b in ((Rg, Ro), (tg, to)):
        assert (np.isnan(a) == np.isnan(b)).all(), (a, b)
        f = ~np.isnan(b)
        assert np.abs(a[f] - b[f]).max(initial=0.0) <= tol, (a, b)


@pytest.mark.parametrize("row", sorted(pdc.zero_theta_rows()))
def test_zero_theta_fallback_votes(vislam, orc, ctx, row):
    """E = [e_z]x at fx = 256, c = 512: the candidates are exactly I / diag(-1, -1, 1) and +-e_z, and the listed correspondences meet
    theta == 0 in a rotation with column 3, so their wave decomposes [R | -t] on its own.  Rows of nothing else; one such lane among
    63 ordinary ones; one in the second of two waves; four in 1100 correspondences dealt over two workgroups (positions 0, 255, 256,
    1099).  `_back` rows are won by -t: the count compared is then made of second-pass votes."""
    p = pdc.zt_params(vislam.default_params())
    ctx.set_params(p)
    x1, x2 = pdc.zero_theta_rows()[row]
    for E in (pdc.E_Z, -pdc.E_Z):
        got, ref = ctx.recover_pose(E, x1, x2), orc.recover_pose(p, E, x1, x2)
        print(row, "gpu", got[2], got[1], "oracle", ref[2], ref[1])
        _same_pose(got, ref, TOL)
        assert abs(ref[1][2]) == 1.0 and (np.abs(ref[0]) == np.eye(3)).all()        # the exact candidates, whichever won
    if row.endswith("_back"):
        assert ref[1][2] == -1.0 and ref[2] > len(x1) // 2                            # the cloud is behind the first pass's camera


@pytest.mark.parametrize("name", sorted(pdc.directed_E()))
def test_recover_pose_of_directed_E(vislam, orc, ctx, name):
    """exact E with two EQUAL singular values (t = e_z, t = e_x, a quarter turn about z), the same scaled by 1e-12 and 1e+12, and E of
    rank 0, 1 and 3.  The oracle's answer is the specification: NaN R, t and n_good = 0 for the zero and the rank-1 matrix (NaN
    positions identical, equality elsewhere), 1e-9 on R, t for the others."""
    p = pdc.zt_params(vislam.default_params())
    ctx.set_params(p)
    E, x1, x2 = pdc.directed_E()[name]
    got, ref = ctx.recover_pose(E, x1, x2), orc.recover_pose(p, E, x1, x2)
    print(name, "gpu", got, "oracle", ref)
    _same_pose(got, ref, TOL)
    if name in ("zero", "rank1"):
        assert ref[2] == 0 and np.isnan(ref[0]).all() and np.isnan(ref[1]).all()
    elif name != "identity":
        assert ref[2] >= 50                                                           # the true motion wins with the cloud in front


# ---- a standing camera through the batched stream ---------------------------------------------------------------------------------
def test_standing_camera_through_the_batched_stream(vislam, orc, canvas):
    """68 frames of 320 x 240, nfeatures 300: frame 0 forty times (39 pairs with x2 == x1 bit for bit), then the moving sequence.  With 64
    pairs or more the first chunk's polynomials go through k_hyp_roots_packed, for the static pairs degenerate ones.  Counts against
    the oracle's per-frame pipeline; the batch's own E against its claims (check_model) and, through the oracle's recoverPose fed that E
    and the batch's matches, against the batch's pose (1e-7, as test_batch_pipeline_pose); E against the oracle's on the moving pairs."""
    import torch
    n, n_static = 68, 40
    p = vislam.default_params()
    p.fy = p.fx
    p.nfeatures = 300
    p.w_size, p.h_size = 320, 240
    assert p.keyframe_min_points == 0                                                 # the gate is off
    src = [0] * n_static + list(range(1, n - n_static + 1))
    frames = np.stack([vislam.synth_frame(canvas, t, 320, 240) for t in src])
    # the oracle, once per distinct pair (frames 1 .. 39 repeat the pair (0, 0))
    ref, prev = [], None
    for i in range(n):
        if 2 <= i < n_static:
            ref.append(ref[1])
            continue
        ok, od, r = orc.pipeline_frame(p, frames[i], prev)
        prev = (ok, od)
        ref.append(r)
    assert all(ref[i].n_good >= 6 for i in range(1, n_static)), ref[1].n_good
    c = vislam.Context(0, p)
    dev = torch.from_numpy(frames).cuda()
    c.batch_plan(320, 240, 320, n)
    c.batch_run(dev.data_ptr(), n)
    c.batch_sync()
    assert c.batch_status() == 0
    kps = [c.batch_keypoints(i)[0] for i in range(n)]
    with_model = 0
    for i in range(n):
        r = ref[i]
        g, nsym = c.batch_matches(i)
        pose = c.batch_pose(i)
        assert nsym == r.n_sym and len(g) == r.n_good, i
        assert pose["n_inliers"] == r.n_inliers and pose["iters_run"] == r.iters_run, (i, pose["n_inliers"], r.n_inliers, pose["iters_run"], r.iters_run)
        if i == 0 or not r.n_inliers:
            continue
        with_model += 1
        a, b = kps[i - 1][g["queryIdx"]], kps[i][g["trainIdx"]]
        x1, x2 = np.stack([a["x"], a["y"]], 1), np.stack([b["x"], b["y"]], 1)
        if i < n_static:
            assert (x1 == x2).all(), i
        oE = np.array(r.E).reshape(3, 3)
        mask = c.batch_inlier_mask(i)
        assert len(mask) == len(g), i
        pdc.check_model(pose["E"], mask, pose["n_inliers"], x1, x2, p, oE)
        Ro, to, no = orc.recover_pose(p, pose["E"], x1, x2)
        assert pose["n_pose_good"] == no, (i, pose["n_pose_good"], no)
        assert np.abs(pose["R"] - Ro).max() <= 1e-7 and np.abs(pose["t"] - to).max() <= 1e-7, i
        if i >= n_static:
            assert pdc.cmp_E(pose["E"], oE) <= TOL, i
    assert with_model >= n - 2
    c.close()
