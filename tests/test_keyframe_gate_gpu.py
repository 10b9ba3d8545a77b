"""GPU: the keyframe gate of the batched stream path (vis_params.keyframe_min_points).  Streams with featureless frames (flat: 0
keypoints) and sparse frames (one bright 5x5 square: between 2 and 10 keypoints) go through vis_batch_run in launches of 16 frames;
a Python frameList kept exactly like CameraGPU::addGPUKeyframe (K = 1, src/CameraGPU.cpp:138-173) and Camera::addKeyframe (K = 10,
src/Camera.cpp:197-235) -- save a frame when it has more than K keypoints (more than 1 while nothing has been saved since the reset),
match it against frameList.back() -- gives the expected pairing, and the oracle gives that pairing's matches, poses and alignment."""
import ctypes as C

import numpy as np
import pytest

import align_cases

pytestmark = pytest.mark.gpu
W, H, B = 752, 480, 16
FLAT, SPARSE, NORMAL = "F", "S", "N"

# launches of 16 frames; None = vis_batch_reset before the next launch
LAUNCHES = [
    # flat at stream position 0, flat mid-batch (3), two in a row (5, 6), a sparse frame (8), a flat LAST frame (15)
    "F N N F N F F N S N N N N N N F",
    # only flat frames: the carried record (frame 14 of the launch before) persists through it
    "F F F F F F F F F F F F F F F F",
    # frame 0 links to the record carried over two launches; a flat frame mid-batch again
    "N N F N N N N N S N N N N N N N",
    None,
    # a sparse frame first after the reset: saved under both rules (the first-frame test is > 1)
    "S N N F N N N N N N N N N N N N",
]


def _sparse(t):
    f = np.full((H, W), 128, np.uint8)
    x, y = 160 + 37 * (t % 11), 120 + 23 * (t % 7)
    f[y:y + 5, x:x + 5] = 255
    return f


def _stream(vislam, canvas):
    """(launches as lists of global frame indices, reset flags, frames (n, H, W), kinds)"""
    frames, kinds, launches, resets, reset_next = [], [], [], [], False
    for spec in LAUNCHES:
        if spec is None:
            reset_next = True
            continue
        idx = []
        for k in spec.split():
            t = len(frames)
            frames.append(np.full((H, W), 128, np.uint8) if k == FLAT else _sparse(t) if k == SPARSE else vislam.synth_frame(canvas, t, W, H))
            kinds.append(k)
            idx.append(t)
        launches.append(idx)
        resets.append(reset_next)
        reset_next = False
    return launches, resets, np.stack(frames), kinds


def _frame_list(launches, resets, nkp, K):
    """the reference's frameList walk: per launch the expected prev[] of vis_batch_get_keyframes, and {frame: saved frame it matches}"""
    saved, links, pair = [], [], {}
    for idx, reset in zip(launches, resets):
        if reset:
            saved = []
        start, lk = idx[0], []
        for g in idx:
            if nkp[g] > (K if saved else 1):                  # Camera.cpp:225 / CameraGPU.cpp:164 for the first frame
                if saved:
                    pair[g] = saved[-1]
                    lk.append(saved[-1] - start if saved[-1] >= start else -1)
                else:
                    lk.append(-3)
                saved.append(g)
            else:
                lk.append(-2)
        links.append(lk)
    return links, pair


@pytest.fixture(scope="module")
def mixed(vislam, orc, canvas):
    launches, resets, frames, kinds = _stream(vislam, canvas)
    p = vislam.default_params()
    p.fy = p.fx
    det = [orc.orb_detect_compute(p, f) for f in frames]
    nkp = [len(k) for k, _ in det]
    for g, k in enumerate(kinds):                             # what the stream exercises
        if k == FLAT:
            assert nkp[g] == 0, g
        elif k == SPARSE:
            assert 2 <= nkp[g] <= 10, (g, nkp[g])
        else:
            assert nkp[g] > 10, g
    return launches, resets, frames, det, nkp


def _run(vislam, frames, launches, resets, K, stages, per_launch):
    import torch
    p = vislam.default_params()
    p.fy = p.fx
    p.keyframe_min_points = K
    c = vislam.Context(0, p)
    c.batch_plan(W, H, W, B)
    dev = torch.from_numpy(frames).cuda()
    out = []
    for li, (idx, reset) in enumerate(zip(launches, resets)):
        if reset:
            c.batch_reset()
        c.batch_run(dev.data_ptr() + idx[0] * W * H, len(idx), stages)
        c.batch_sync()
        assert c.batch_status() == 0
        out.append(per_launch(c, li, idx, dev))
    c.close()
    return out


def _collect(c, li, idx, dev):
    n = len(idx)
    poses, goods, ngood = c.batch_results(n)
    return dict(links=c.batch_get_keyframes(), poses=poses.copy(), matches=[c.batch_matches(i) for i in range(n)],
                masks=[c.batch_inlier_mask(i) for i in range(n)], knn=[c.batch_knn(i) for i in range(n)], ngood=ngood.copy())


def _no_pair_record(vislam, frames, launches, resets):
    """the pose record of pair 0 after a reset with the gate off: what a pair without correspondences gets"""
    got = _run(vislam, frames, launches[:1], resets[:1], 0, vislam.STAGE_ALL, lambda c, li, idx, dev: c.batch_results(len(idx))[0].copy())
    return got[0][0].tobytes()


def test_gate_off_keeps_todays_pairing(vislam, mixed):
    launches, resets, frames, det, nkp = mixed
    got = _run(vislam, frames, launches, resets, 0, vislam.STAGE_ALL, lambda c, li, idx, dev: c.batch_get_keyframes())
    for li, (idx, reset) in enumerate(zip(launches, resets)):
        want = np.arange(-1, len(idx) - 1, dtype=np.int32)
        want[0] = -3 if (li == 0 or reset) else -1
        assert np.array_equal(got[li], want), li


@pytest.mark.parametrize("K", [1, 10])
def test_gate_against_the_frame_list(vislam, orc, mixed, K):
    launches, resets, frames, det, nkp = mixed
    p = vislam.default_params()
    p.fy = p.fx
    want_links, pair = _frame_list(launches, resets, nkp, K)
    got = _run(vislam, frames, launches, resets, K, vislam.STAGE_ALL, _collect)
    no_pair = _no_pair_record(vislam, frames, launches, resets)
    # the rules differ on the sparse frame of the first launch and agree on the sparse first frame after the reset
    s0 = launches[0][8]
    assert (want_links[0][8] == -2) == (K == 10) and want_links[-1][0] == -3
    assert want_links[0][0] == -2 and want_links[0][1] == -3 and want_links[1] == [-2] * B and want_links[2][0] == -1
    assert pair[launches[2][0]] == launches[0][14]
    assert (s0 in pair.values()) == (K == 1)
    checked = 0
    for li, idx in enumerate(launches):
        g_ = got[li]
        assert g_["links"].tolist() == want_links[li], (li, g_["links"].tolist(), want_links[li])
        for i, g in enumerate(idx):
            good, nsym = g_["matches"][i]
            rec = g_["poses"][i]
            if g not in pair:                                   # not saved, or saved with nothing to match: no pair
                assert len(good) == 0 and nsym == 0 and g_["ngood"][i] == 0, (li, i)
                assert rec.tobytes() == no_pair, (li, i)
                assert len(g_["knn"][i][0]) == 0 and len(g_["knn"][i][1]) == 0, (li, i)
                continue
            (pk, pd), (ok, od) = det[pair[g]], det[g]
            o12, o21 = orc.knn2_hamming(pd, od)
            og, osym = orc.good_matches(p, pk, ok, o12, o21)
            assert g_["knn"][i][0].tobytes() == o12.tobytes() and g_["knn"][i][1].tobytes() == o21.tobytes(), (li, i)
            assert good.tobytes() == og.tobytes() and nsym == len(osym), (li, i)
            p1 = np.stack([pk["x"][og["queryIdx"]], pk["y"][og["queryIdx"]]], 1)
            p2 = np.stack([ok["x"][og["trainIdx"]], ok["y"][og["trainIdx"]]], 1)
            _, _, r = orc.pipeline_frame(p, frames[g], (pk, pd))
            oE, omask, oninl, oiters = orc.essential_ransac(p, p1, p2)
            assert rec["n_points"] == r.n_good == len(og) and rec["n_inliers"] == r.n_inliers == oninl, (li, i)
            assert rec["iters_run"] == r.iters_run and rec["n_pose_good"] == r.n_pose_good, (li, i)
            assert len(g_["masks"][i]) == len(omask) and (g_["masks"][i] == omask).all(), (li, i)
            if r.n_inliers:
                E, rE = rec["E"].reshape(3, 3), np.array(r.E).reshape(3, 3)
                s = 1.0 if float((E * rE).sum()) >= 0 else -1.0
                assert np.abs(E - s * rE).max() <= 1e-9, (li, i)
                assert np.abs(rec["R"].reshape(3, 3) - np.array(r.R).reshape(3, 3)).max() <= 1e-9, (li, i)
                assert np.abs(rec["t"] - np.array(r.t)).max() <= 1e-9, (li, i)
            checked += 1
    assert checked == len(pair) >= 35


def test_alignment_across_a_flat_frame(vislam, orc, mixed):
    """vis_batch_align on the gated pairs: frame 4 of the first launch is matched against frame 2 (frame 3 is flat); the plan's
    gradients of frame 2 feed it, bit-identical to the oracle's EstimatePoseFeatures on that pair with those matched points"""
    import torch
    launches, resets, frames, det, nkp = mixed
    ap = vislam.default_align_params()

    def align(c, li, idx, dev):
        n = len(idx)
        out = torch.zeros(n * C.sizeof(vislam.AlignResult), dtype=torch.uint8, device="cuda")
        c.batch_align(ap, dev.data_ptr() + idx[0] * W * H, n, 0, 0, 0, 0, out.data_ptr())
        c.batch_sync()
        torch.cuda.synchronize()
        raw = out.cpu().numpy().tobytes()
        return c.batch_get_keyframes(), [vislam.AlignResult.from_buffer_copy(raw, i * C.sizeof(vislam.AlignResult)) for i in range(n)], \
            [c.batch_matches(i)[0] for i in range(n)], [c.batch_keypoints(i)[0] for i in range(n)]

    links, res, goods, kps = _run(vislam, frames, launches[:1], resets[:1], 1, vislam.STAGE_ALL | vislam.STAGE_GRADIENT, align)[0]
    assert links[4] == 2 and links[7] == 4
    for i in range(len(links)):
        if links[i] < 0:                                        # no pair, or the first pair: zeroed
            assert list(res[i].n_residuals) == [0] * 5 and list(res[i].iterations) == [0] * 5, i
    for i in (4, 7, 2):                                         # across one flat frame, across two, and a plain i-1 link
        j = links[i]
        prev_kp = kps[j][goods[i]["queryIdx"]]
        l0, l1 = orc.half_pyramid(frames[j]), orc.half_pyramid(frames[i])
        ogx, ogy = [], []
        for lv in l0:
            a, b, _ = orc.scharr_gradient(lv, 3)
            ogx.append(a); ogy.append(b)
        cand = [orc.patch_points(prev_kp, W, H, l) for l in range(5)]
        ref = orc.estimate_pose_features(orc.default_align_params(), W, H, l0, l1, ogx, ogy, cand)
        assert align_cases.result_tuple(res[i]) == align_cases.result_tuple(ref), i
        assert res[i].n_residuals[0] > 0, i


def test_gate_on_the_headline_geometry_changes_nothing_when_every_frame_passes(vislam):
    """S-752 at 1024 frames per launch, VIS_STAGE_FRAME, two launches: with K = 1 every frame is saved, so the results download is
    byte-identical to K = 0 and the links are today's pairing"""
    import torch
    n, seed, dim = 1024, 0xE0C00001, 4096
    canvas = torch.from_numpy(vislam.synth_canvas(dim, seed)).cuda()
    out = {}
    for K in (0, 1):
        p = vislam.default_params()
        p.fy = p.fx
        p.keyframe_min_points = K
        c = vislam.Context(0, p)
        frames = torch.empty((2 * n, H, W), dtype=torch.uint8, device="cuda")
        for t0 in range(0, 2 * n, 256):
            c.synth_frames_device(canvas.data_ptr(), dim, seed, t0, 256, W, H, W, frames.data_ptr() + t0 * W * H)
        torch.cuda.synchronize()
        c.batch_plan(W, H, W, n)
        rs = []
        for li in range(2):
            c.batch_run(frames.data_ptr() + li * n * W * H, n, vislam.STAGE_FRAME)
            poses, goods, ngood = c.batch_results(n)
            rs.append((poses.tobytes(), [goods[i, :ngood[i]].tobytes() for i in range(n)], ngood.tobytes(), c.batch_get_keyframes()))
        assert c.batch_status() == 0
        c.close()
        out[K] = rs
    for li in range(2):
        assert out[1][li][0] == out[0][li][0], li
        assert out[1][li][1] == out[0][li][1], li
        assert out[1][li][2] == out[0][li][2], li
        want = np.arange(-1, n - 1, dtype=np.int32)
        want[0] = -3 if li == 0 else -1
        assert np.array_equal(out[1][li][3], want) and np.array_equal(out[0][li][3], want), li


def test_out_of_range_values_are_refused(vislam):
    c = vislam.Context(0)
    for bad in (-1, 65536):
        p = vislam.default_params()
        p.keyframe_min_points = bad
        with pytest.raises(vislam.VisError):
            c.set_params(p)
    p = vislam.default_params()
    p.keyframe_min_points = 65535
    c.set_params(p)
    c.close()
