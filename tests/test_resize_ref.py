"""CPU: the oracle's cv::resize restatement (oracle/orb.cpp orc_resize_linear, C++, pixel by pixel) against an independent numpy
restatement of the published algorithm (tests/resize_ref.py), byte for byte -- on every pyramid step of the configurations that
tests/test_param_range_gpu.py runs on the device, on lone steps at the ratios where the kernels change path (1.0, just above 1, either
side of 2, 2.5, 3.0 and 3.125, the largest the accepted range can produce) and on three kinds of image.  Every GPU assertion on the
pyramid leans on this equality: the device levels are compared with the oracle's."""
import numpy as np
import pytest

import param_range_cases as prc
import resize_ref


def _same(orc, src, dw, dh, what):
    a, b = orc.resize_linear(src, dw, dh), resize_ref.resize_linear(src, dw, dh)
    if not np.array_equal(a, b):
        ys, xs = np.nonzero(a != b)
        raise AssertionError((what, src.shape, (dh, dw), f"{len(ys)} bytes differ, first at (y, x) = ({ys[0]}, {xs[0]}): "
                                                          f"oracle {a[ys[0], xs[0]]}, numpy {b[ys[0], xs[0]]}"))
    return a


@pytest.mark.parametrize("case", prc.CASES, ids=[c.id for c in prc.CASES])
def test_every_pyramid_step_of_the_range_configurations(vislam, orc, canvas, case):
    p = case.params(vislam)
    ws, hs, _, _ = orc.level_geometry(p, case.w, case.h)
    sizes = [(int(a), int(b)) for a, b in zip(ws, hs)]
    assert sizes[0] == (case.w, case.h)
    if case.sizes is not None:
        assert sizes[1:] == case.sizes                              # the sizes the configuration was chosen for
    imgs = prc.step_images(case.w, case.h)
    imgs["frame"] = case.image(vislam, canvas)                      # what the GPU test detects on
    for kind, lv in imgs.items():
        for l in range(1, case.levels):
            # (all sixteen levels here: the yardstick costs milliseconds per step on the CPU; the GPU test thins them out)
            lv = _same(orc, lv, sizes[l][0], sizes[l][1], (case.id, kind, l))


@pytest.mark.parametrize("step", prc.LONE_STEPS, ids=[f"{s[0]}x{s[1]}-to-{d[0]}x{d[1]}" for s, d in prc.LONE_STEPS])
def test_lone_steps_at_the_path_changes(orc, step):
    (sw, sh), (dw, dh) = step
    for kind, img in prc.step_images(sw, sh).items():
        out = _same(orc, img, dw, dh, (step, kind))
        if (sw, sh) == (dw, dh):
            assert np.array_equal(out, img), kind                   # ratio 1.0: every fraction is 0, the step is a copy through the Q11 arithmetic


def test_the_largest_step_is_what_the_level_formula_gives(vislam, orc):
    """75 x 75 at scale 3.0 with 3 levels is 75 -> 25 -> 8: the 25 / 8 = 3.125 step of param_range_cases.LONE_STEPS is one the
    level formula really produces on an image the detector accepts (edge 22: 75 >= 2 * 22 + 8)"""
    p = vislam.default_params()
    p.scale_factor, p.nlevels, p.edge_threshold = 3.0, 3, 22
    ws, hs, _, _ = orc.level_geometry(p, 75, 75)
    assert [int(x) for x in ws] == [75, 25, 8] and [int(x) for x in hs] == [75, 25, 8]


def test_the_yardstick_itself_on_values_worked_by_hand():
    """2 x 2 -> 1 x 1: the source coordinate is 0.5 in both directions, all four Q11 coefficients are 1024:
    rows = (a + b) * 1024, out = ((1024 * (row0 >> 4)) >> 16) + ((1024 * (row1 >> 4)) >> 16) + 2 >> 2"""
    src = np.array([[10, 20], [30, 41]], np.uint8)
    r0, r1 = (10 + 20) * 1024, (30 + 41) * 1024
    want = (((1024 * (r0 >> 4)) >> 16) + ((1024 * (r1 >> 4)) >> 16) + 2) >> 2
    assert want == 25                                               # 25.25 in real arithmetic
    assert resize_ref.resize_linear(src, 1, 1)[0, 0] == want
    # a ramp stays a ramp under an integer ratio with aligned phase: 8 -> 4 averages neighbours (x.5 rounds through + 2 >> 2)
    ramp = np.tile(np.arange(0, 80, 10, dtype=np.uint8), (2, 1))
    assert resize_ref.resize_linear(ramp, 4, 1)[0].tolist() == [5, 25, 45, 65]
    # the horizontal clamp: the first output of an up-scale sits left of pixel 0 and takes pixel 0 alone
    assert resize_ref.resize_linear(np.array([[200, 0]], np.uint8), 4, 1)[0, 0] == 200
