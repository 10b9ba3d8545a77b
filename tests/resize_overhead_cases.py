"""The shapes at which the narrow k_resize's index decode, its workgroup- and wave-uniform values, its full / partial row-group paths and
its store addressing can go wrong, shared by the CPU coverage test (tests/test_resize_index.py) and the GPU parity test
(tests/test_resize_overhead_gpu.py).

A thread of k_resize<true> produces 4 pixels x 5 rows; bx_count = ceil(w_l / 4) column groups and ceil(h_l / 5) row groups are dealt to
threads by a flat index, 256 to a workgroup.  The narrow variant runs a step whose ratio is <= 2 and whose destination has >= 12 groups.

Two of the shapes asked for cannot be had as asked, and the nearest that exists stands in:
  * bx_count = 188 needs a level 749 .. 752 wide, hence a frame wider than 320; the frame is 900 x 60, fewer pixels than 320 x 240;
  * a level of a single row group would have <= 5 rows, and vis_set_params / vis_compute_levels accept no level under 8 x 8: the level of
    8 rows (one full group and a partial one of 3, both in the same wave) and the level of 10 rows (two full groups) stand in.
Every frame has edge_threshold = 22, the smallest accepted, so that 52 rows are a legal frame."""
import numpy as np

RS_ROWS = 5
EDGE = 22


class Case:
    def __init__(self, w, h, scale, levels, frames, pad):
        self.w, self.h, self.scale, self.levels, self.frames, self.pad = w, h, scale, levels, frames, pad
        self.stride = w + pad                                  # level 0's row pitch: the first step's source stride
        self.id = f"{w}x{h}-sf{scale}-L{levels}-n{frames}-pad{pad}"

    def params(self, vislam):
        p = vislam.default_params()
        p.w_size, p.h_size = self.w, self.h
        p.scale_factor, p.nlevels, p.edge_threshold, p.nfeatures = self.scale, self.levels, EDGE, 100
        return p

    def images(self):
        """frames x h x stride random bytes, the padding included (a read past the row's end would show)"""
        rng = np.random.default_rng(self.w * 4096 + self.h + self.frames)
        return rng.integers(0, 256, (self.frames, self.h, self.stride), dtype=np.uint8)


CASES = [
    # scale 1.2: the level-1 width sets bx_count, the level-1 height the last row group
    Case(56, 60, 1.2, 2, 9, 8),        # 47 x 50: bx_count 12 (the narrow variant's lower limit), h % 5 = 0
    Case(60, 61, 1.2, 2, 1, 4),        # 50 x 51: bx_count 13, h % 5 = 1; one frame
    Case(300, 65, 1.2, 2, 8, 20),      # 250 x 54: bx_count 63, h % 5 = 4; eight frames
    Case(306, 61, 1.2, 2, 9, 14),      # 255 x 51: bx_count 64 (a wave = one row group exactly), h % 5 = 1
    Case(310, 60, 1.2, 2, 9, 10),      # 258 x 50: bx_count 65, h % 5 = 0
    Case(900, 60, 1.2, 2, 9, 60),      # 750 x 50: bx_count 188
    # eleven levels down to 52 x 8: heights 43 36 30 25 21 17 15 12 10 8
    Case(320, 52, 1.2, 11, 9, 64),
    # scale 2.0: no listed sharing pattern matches, every wave loads every row
    Case(96, 240, 2.0, 2, 9, 32),      # 48 x 120: bx_count 12
    Case(320, 236, 2.0, 3, 8, 64),     # 160 x 118 (h % 5 = 3), 80 x 59 (h % 5 = 4)
    Case(100, 52, 2.0, 2, 1, 12),      # 50 x 26: bx_count 13, h % 5 = 1; one frame
]


def narrow_levels(ws, hs):
    """[(level, bx_count, h_l)] of the steps the narrow variant runs (csrc/detect.hip launch_detect: ratio <= 2 and >= 12 groups)"""
    out = []
    for l in range(1, len(ws)):
        bxc = (int(ws[l]) + 3) // 4
        if 1.0 / (float(ws[l]) / float(ws[l - 1])) <= 2.0 and bxc >= 12:
            out.append((l, bxc, int(hs[l])))
    return out
