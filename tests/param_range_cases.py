"""The configurations that walk the detector and its pyramid over the whole range vis_set_params accepts (scale_factor in (1, 3],
fast_threshold 1 .. 254, edge_threshold 22 .. 255, nlevels 1 .. 16, every level at least 8 x 8), shared by the CPU yardstick test
(tests/test_resize_ref.py: oracle resize == numpy restatement on every step) and the GPU tests (tests/test_param_range_gpu.py).

What each row is the first to reach (replayed from vis_compute_levels and resize_coef):
  752x480 3.0 / 4     wide k_resize at ratio 2.99 / 3.0 / 3.02, window offset >= 8 (third dword) on 62 / 21 / 7 outputs per row;
                      levels 2 and 3 are smaller than the border
  752x480 2.5 / 4     window offset 7 (third dword as the high word) on 38 / 14 outputs per row, offset 8 on 37 / 16 / 12; level 2 emits on 58 x 15 only
  752x480 2.2 / 4     wide variant just above 2 on every step; offset 7 on 51 / 23 / 10
  641x479 2.0 / 3     step 1 wide by 0.003; step 2 narrow at exactly 2.0
  640x480 3.0 / 3     a level-0 stride equal to the width: the wide variant's right-edge clamp wb = sstride - 12 binds on the last
                      group (the batch plan's 752-byte rows reach it too: offset 10 of the 11 the window allows)
  333x257 3.0 / 3     odd everything; level 2 below the border
  200x136 3.0 / 3     level 1's emit region is 5 x -17: positive in one direction only
  640x480 1.01 / 16   the maximum level count; narrow variant at ratios 1.009 .. 1.012
  640x480 1.001 / 16  steps whose x or y ratio is exactly 1.0
  96x72   1.2 / 8     the smallest image with the default level count: levels 1 - 7 emit nothing, levels 5 - 7 take the wide variant
  640x600 1.2 / 8, edge 255   the largest border: level 0 emits on 130 x 90, nothing above it
"""
import numpy as np


class Case:
    def __init__(self, w, h, scale, levels, edge, sizes, nfeatures, content="synth", floor_total=50, floor_level0=0):
        self.w, self.h, self.scale, self.levels, self.edge = w, h, scale, levels, edge
        self.sizes = sizes                  # (w_l, h_l) of levels >= 1 as the issue tabulated them (None: too many to list; level_geometry decides)
        self.nfeatures, self.content = nfeatures, content
        self.floor_total, self.floor_level0 = floor_total, floor_level0
        self.id = f"{w}x{h}-sf{scale}-L{levels}-e{edge}"

    def params(self, vislam):
        p = vislam.default_params()
        p.w_size, p.h_size = self.w, self.h
        p.scale_factor, p.nlevels, p.edge_threshold, p.nfeatures = self.scale, self.levels, self.edge, self.nfeatures
        return p

    def image(self, vislam, canvas, t=3):
        return make_image(vislam, canvas, self.content, self.w, self.h, t)


CASES = [
    Case(752, 480, 3.0, 4, 31, [(251, 160), (84, 53), (28, 18)], 1000),
    Case(752, 480, 2.5, 4, 31, [(301, 192), (120, 77), (48, 31)], 1000),
    Case(752, 480, 2.2, 4, 31, [(342, 218), (155, 99), (71, 45)], 1000),
    Case(641, 479, 2.0, 3, 31, [(320, 240), (160, 120)], 1000),
    Case(640, 480, 3.0, 3, 31, [(213, 160), (71, 53)], 1000),
    Case(333, 257, 3.0, 3, 31, [(111, 86), (37, 29)], 600),
    Case(200, 136, 3.0, 3, 31, [(67, 45), (22, 15)], 400),
    Case(640, 480, 1.01, 16, 31, None, 1600),
    Case(640, 480, 1.001, 16, 31, None, 1600),
    # the last two: level 0 alone can emit, so the floor is stated for it instead of the general 50
    Case(96, 72, 1.2, 8, 31, [(80, 60), (67, 50), (56, 42), (46, 35), (39, 29), (32, 24), (27, 20)], 1000, content="noise", floor_total=10, floor_level0=10),
    Case(640, 600, 1.2, 8, 255, None, 1000, floor_total=10, floor_level0=10),
]
# levels of the 16-level cases that the numpy yardstick is run on (it is cheap everywhere else)
YARDSTICK_LEVELS_16 = (1, 2, 8, 15)


def make_image(vislam, canvas, content, w, h, t=3, amp=6):
    """synth: a crop of the synthetic stream plus +-amp of uniform noise (corners on every level that can emit); noise: uniform bytes"""
    rng = np.random.default_rng(1000 * w + h + t)
    if content == "noise":
        return rng.integers(0, 256, (h, w), dtype=np.uint8)
    f = vislam.synth_frame(canvas, t, w, h).astype(np.int32)
    return np.clip(f + rng.integers(-amp, amp + 1, (h, w)), 0, 255).astype(np.uint8)


def emit_region(w_l, h_l, edge):
    return w_l - 2 * edge, h_l - 2 * edge


def must_emit(w_l, h_l, edge):
    """the octave has room for keypoints in both directions and at least 16 x 16 of it: the oracle must find one there"""
    ew, eh = emit_region(w_l, h_l, edge)
    return ew >= 16 and eh >= 16


def cannot_emit(w_l, h_l, edge):
    ew, eh = emit_region(w_l, h_l, edge)
    return ew <= 0 or eh <= 0


def check_not_vacuous(case, ws, hs, okps):
    """the conditions that keep a parity case from passing with nothing to compare, on the ORACLE's keypoints alone.  An octave whose
    emit region is positive but smaller than 16 x 16 (96 x 72 level 0: 34 x 10; 752 x 480 at 2.5 level 2: 58 x 15) is bound by
    neither rule: the case's own floor speaks for it where it matters."""
    per = np.bincount(okps["octave"], minlength=len(ws))
    for l in range(len(ws)):
        if must_emit(int(ws[l]), int(hs[l]), case.edge):
            assert per[l] >= 1, (case.id, l, "an octave with an emit region of 16 x 16 or more yields nothing", per.tolist())
        if cannot_emit(int(ws[l]), int(hs[l]), case.edge):
            assert per[l] == 0, (case.id, l, "an octave smaller than the border yields keypoints", per.tolist())
    assert len(okps) >= case.floor_total, (case.id, len(okps))
    assert per[0] >= case.floor_level0, (case.id, per.tolist())
    return per


# ---- lone resize steps (source size -> destination size), beside every step of the configurations above
LONE_STEPS = [
    ((100, 80), (100, 80)),        # ratio 1.0 exactly in both directions: every fraction 0
    ((640, 480), (639, 479)),      # just above 1
    ((641, 479), (321, 240)),      # just below 2 (1.9969 / 1.9958)
    ((641, 481), (320, 240)),      # just above 2 (2.0031 / 2.0042)
    ((300, 200), (120, 80)),       # 2.5
    ((300, 240), (100, 80)),       # 3.0
    ((75, 52), (25, 17)),          # the chain 75 -> 25 -> 8 of scale 3.0 ...
    ((25, 17), (8, 8)),            # ... ends in 25 -> 8 = 3.125, the largest step the accepted range can produce (see below)
]
# The largest step ratio: level sizes are round(w / s^l), so a step is round(3 x) / round(x) at most, x = w / 3^l.  round(x) >= 8 needs
# x >= 7.5 and the quotient falls with x: with round(x) = 8 (x <= 8.5) the numerator is at most round(25.5 - eps) = 25, 25 / 8 = 3.125;
# round(x) = 9 gives 28 / 9 = 3.11 at most.  (The wide k_resize's 12-byte window holds any ratio below 3.6.)


def step_images(w, h, seed=0):
    """random bytes, a 0 / 255 checker and a horizontal ramp (an off-by-one source index shows at once on the ramp)"""
    rng = np.random.default_rng(seed + 7919 * w + h)
    yy, xx = np.mgrid[0:h, 0:w]
    return {"random": rng.integers(0, 256, (h, w), dtype=np.uint8),
            "checker": (((yy + xx) & 1) * 255).astype(np.uint8),
            "ramp": (xx & 255).astype(np.uint8)}


# ---- extreme FAST thresholds on 320 x 240
def dots_image(w=320, h=240):
    """isolated 255 pixels on 0 (left half) and isolated 0 pixels on 255 (right half) on a lattice of pitch 8 inside the emit region of
    level 0 at edge 31 -- corners at every accepted threshold (|difference| 255 > 254) -- and, on the rows between, dots of 254 on 0:
    corners at 253, not at 254.  Returns (image, number of saturated dots, number of 254-dots)."""
    img = np.zeros((h, w), np.uint8)
    img[:, w // 2:] = 255
    n_sat = n_254 = 0
    for y in range(40, h - 40, 16):
        for x in range(40, w // 2 - 8, 8):
            img[y, x] = 255; n_sat += 1
        for x in range(w // 2 + 8, w - 40, 8):
            img[y, x] = 0; n_sat += 1
    for y in range(48, h - 40, 16):
        for x in range(40, w // 2 - 8, 16):
            img[y, x] = 254; n_254 += 1
    return img, n_sat, n_254
