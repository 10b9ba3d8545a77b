"""GPU: k_filter (the ratio test, the symmetric list, the grid) over the parameter range vis_set_params accepts, against the CPU oracle byte
for byte on the hand-made cases of tests/match_param_cases.py -- through vis_good_matches_host, and with a non-default setting through the
filter's two other callers, vis_good_matches on slots and vis_batch_run -- and what vis_set_params refuses: a grid root above
VIS_MAX_GRID_ROOT, an unknown sym_mode."""
import numpy as np
import pytest

import match_param_cases as mc

pytestmark = pytest.mark.gpu
E_INVALID = -1                                                         # VIS_E_INVALID


@pytest.fixture(scope="module")
def c(vislam):
    ctx = vislam.Context(0)
    yield ctx
    ctx.close()


def _run(vislam, orc, c, case):
    p = mc.apply(vislam.default_params(), case)
    c.set_params(p)
    good, sym = c.good_matches_host(case["k1"], case["k2"], case["k12"], case["k21"])
    want_good, want_sym = orc.good_matches(p, case["k1"], case["k2"], case["k12"], case["k21"])
    assert sym.tobytes() == want_sym.tobytes(), (case["name"], "sym", len(sym), len(want_sym))
    assert good.tobytes() == want_good.tobytes(), (case["name"], "good", good["queryIdx"].tolist(), want_good["queryIdx"].tolist())
    return len(good), len(sym)


def test_ratio_sweep(vislam, orc, c):
    assert vislam.KEYPOINT_DTYPE == mc.KEYPOINT and vislam.DMATCH_DTYPE == mc.DMATCH
    sizes = {}
    for case in mc.ratio_cases():
        sizes[case["name"]] = _run(vislam, orc, c, case)[1]
    print("symmetric matches kept:", sizes)
    assert len(set(sizes.values())) > 6                            # the settings are seen to differ


def test_grid_sweep(vislam, orc, c):
    kept = {}
    for case in mc.grid_cases():
        kept[case["name"]] = _run(vislam, orc, c, case)[0]
    print("good matches:", kept)
    assert max(kept.values()) > 49 and min(kept.values()) == 1     # from one cell to more than the default grid holds


def test_refused_settings(vislam, c):
    import ctypes as C
    for n in mc.REFUSED_N_CELLS:
        p = vislam.default_params()
        p.n_cells = n
        assert vislam.lib.vis_set_params(c._h, C.byref(p)) == E_INVALID, n
        text = vislam.lib.vis_last_error(c._h).decode()
        assert "n_cells" in text and str(mc.MAX_GRID_ROOT) in text and "1088" in text, (n, text)
    for mode in (-1, 2, 3, 2 ** 31 - 1, -2 ** 31):
        p = vislam.default_params()
        p.sym_mode = mode
        assert vislam.lib.vis_set_params(c._h, C.byref(p)) == E_INVALID, mode
        assert "sym_mode" in vislam.lib.vis_last_error(c._h).decode(), mode
    q = vislam.Params()                                            # a refusal changes nothing
    assert vislam.lib.vis_get_params(c._h, C.byref(q)) == 0
    assert 1 <= q.n_cells <= 1088 and q.sym_mode in (0, 1)
    for n in (1088, 1):
        p = vislam.default_params()
        p.n_cells = n
        c.set_params(p)


SETTING = dict(ratio=0.75, sym_mode=1, n_cells=48, w_size=750, h_size=481)      # a 6 x 6 grid of 125 x 80.1666 cells


def test_slots_with_a_non_default_setting(vislam, orc, canvas):
    p = vislam.default_params()
    for k, v in SETTING.items():
        setattr(p, k, v)
    ctx = vislam.Context(0, p)
    a, b = vislam.synth_frame(canvas, 0, 752, 480), vislam.synth_frame(canvas, 1, 752, 480)
    k0, d0 = ctx.orb_detect_compute(a, slot=0)
    k1, d1 = ctx.orb_detect_compute(b, slot=1)
    o12, o21 = orc.knn2_hamming(d0, d1)
    good, sym = ctx.good_matches(0, 1)
    want_good, want_sym = orc.good_matches(p, k0, k1, o12, o21)
    assert sym.tobytes() == want_sym.tobytes() and good.tobytes() == want_good.tobytes()
    dflt_good, dflt_sym = orc.good_matches(vislam.default_params(), k0, k1, o12, o21)
    assert 10 < len(good) <= 36 and len(sym) < len(dflt_sym) and good.tobytes() != dflt_good.tobytes()
    ctx.close()


def test_batch_run_with_a_non_default_setting(vislam, orc, canvas):
    import torch
    W, H, N = 160, 120, 4
    p = vislam.default_params()
    for k, v in dict(SETTING, w_size=W - 1, h_size=H + 1, n_cells=24).items():       # 4 x 4 cells of 39.75 x 30.25
        setattr(p, k, v)
    ctx = vislam.Context(0, p)
    ctx.batch_plan(W, H, W, N)
    frames = np.stack([vislam.synth_frame(canvas, t, W, H) for t in range(N)])
    dev = torch.from_numpy(frames).cuda()
    torch.cuda.synchronize()
    ctx.batch_run(dev.data_ptr(), N, vislam.STAGE_ALL)
    ctx.batch_sync()
    assert ctx.batch_status() == 0
    recs = [ctx.batch_keypoints(i) for i in range(N)]
    seen = 0
    for i in range(1, N):
        (kq, dq), (kt, dt) = recs[i - 1], recs[i]
        o12, o21 = orc.knn2_hamming(dq, dt)
        good, nsym = ctx.batch_matches(i)
        want_good, want_sym = orc.good_matches(p, kq, kt, o12, o21)
        assert good.tobytes() == want_good.tobytes() and nsym == len(want_sym), i
        dflt = vislam.default_params()
        dflt.w_size, dflt.h_size = W, H
        seen += good.tobytes() != orc.good_matches(dflt, kq, kt, o12, o21)[0].tobytes()
    assert seen > 0
    ctx.close()
