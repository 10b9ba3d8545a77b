"""GPU: the narrow k_resize at the smallest shapes where its index decode, its workgroup- and wave-uniform values, its full / partial
row-group paths and its store addressing can go wrong (tests/resize_overhead_cases.py; tests/test_resize_index.py shows on the CPU
that the shapes reach what they were chosen for).

Every level >= 1 of the batch plan, read back with ctx.pyramid_level(l, frame, batch=True), equals -- byte for byte -- the oracle's
resize of the level below it as the device left it, chained from the frame.  Frames are random bytes on a padded stride; the frames
read back are 0, 7 and the last (8 of nine: one past the XCD map's group of eight)."""
import numpy as np
import pytest

import resize_overhead_cases as roc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("cid", [c.id for c in roc.CASES])
def test_levels_equal_the_oracle_resize(vislam, orc, cid):
    import torch
    c = next(k for k in roc.CASES if k.id == cid)
    p = c.params(vislam)
    frames = c.images()
    ctx = vislam.Context(0, p)
    try:
        ws, hs, _, _ = ctx.level_geometry(c.w, c.h)
        ows, ohs, _, _ = orc.level_geometry(p, c.w, c.h)
        assert ws.tolist() == ows.tolist() and hs.tolist() == ohs.tolist()
        dev = torch.from_numpy(frames).cuda()
        ctx.batch_plan(c.w, c.h, c.stride, c.frames)
        ctx.batch_run(dev.data_ptr(), c.frames, vislam.STAGE_DETECT)
        ctx.batch_sync()
        assert ctx.batch_status() == 0
        nbytes = 0
        for f in sorted({0, min(7, c.frames - 1), c.frames - 1}):
            below = np.ascontiguousarray(frames[f, :, :c.w])
            for l in range(1, c.levels):
                dw, dh = int(ws[l]), int(hs[l])
                got = ctx.pyramid_level(l, frame=f, batch=True, w=c.w, h=c.h)
                want = orc.resize_linear(below, dw, dh)
                assert got.shape == want.shape, (cid, f, l, got.shape, want.shape)
                if not np.array_equal(got, want):
                    ys, xs = np.nonzero(got != want)
                    raise AssertionError((cid, "frame", f, "step", l - 1, "->", l, (dw, dh), f"{len(ys)} of {got.size} bytes differ, first at (y, x) = "
                                          f"({ys[0]}, {xs[0]}): got {got[ys[0], xs[0]]}, want {want[ys[0], xs[0]]}; rows {sorted(set(ys.tolist()))[:12]}, "
                                          f"columns {sorted(set(xs.tolist()))[:12]}"))
                below = got
                nbytes += got.size
        print(cid, "narrow steps", roc.narrow_levels(ws, hs), f"{nbytes} bytes equal to the oracle's", flush=True)
    finally:
        ctx.close()
