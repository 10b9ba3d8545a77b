"""CPU: the bundle-adjustment entry points' place in the C ABI -- vis_ba_params (48 bytes), vis_ba_window (80) and vis_ba_point (40) in the C
compiler's layout and in the ctypes / numpy bindings and the restatement, the enums and defaults, the three symbols exported and listed, every
refusal that needs no device in the header's order, both ends of every parameter's range accepted and one step past each refused;
VIS_ABI_VERSION and vis_params unchanged."""
import ctypes as C
import math
import os
import subprocess

import ba_ref as br

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("vis_default_ba_params", "vis_ba_rows", "vis_batch_ba")
B_FIELDS = ("stride", "min_views", "min_points", "lm_iters", "tri_gn_iters", "reserved_", "huber_px", "init_reproj_px", "lambda0")
W_FIELDS = ("first", "last", "anchor", "n_free", "n_points", "n_obs", "n_lin", "n_accepted", "n_rejected", "flags", "reserved_", "cost0", "cost1",
            "lambda_", "scale")
P_FIELDS = ("X", "rms0_px", "rms1_px", "n_views", "flags")

SNIPPET = r"""
#include <stddef.h>
#include <stdio.h>
#include "vislam_hip.h"
#define B(f) (int)offsetof(vis_ba_params, f)
#define W(f) (int)offsetof(vis_ba_window, f)
#define P(f) (int)offsetof(vis_ba_point, f)
int main(void) {
    printf("%d %d %d %d %d %d %d %d %d %d\n", (int)sizeof(vis_ba_params), B(stride), B(min_views), B(min_points), B(lm_iters), B(tri_gn_iters),
           B(reserved_), B(huber_px), B(init_reproj_px), B(lambda0));
    printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n", (int)sizeof(vis_ba_window), W(first), W(last), W(anchor), W(n_free), W(n_points),
           W(n_obs), W(n_lin), W(n_accepted), W(n_rejected), W(flags), W(reserved_), W(cost0), W(cost1), W(lambda), W(scale));
    printf("%d %d %d %d %d %d\n", (int)sizeof(vis_ba_point), P(X), P(rms0_px), P(rms1_px), P(n_views), P(flags));
    printf("%d %d %d %d %d %d %d %d %d\n", VIS_ABI_VERSION, (int)sizeof(vis_params), (int)VIS_BA_REFINED, (int)VIS_BA_FEW, (int)VIS_BA_RESTART,
           (int)VIS_BA_NO_SCALE, (int)VIS_BAP_USED, (int)VIS_BAP_INIT_REJECTED, (int)VIS_BAP_FEW);
    return 0;
}
"""


def test_layout_in_c_ctypes_numpy_and_the_restatement(vislam, tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(SNIPPET)
    exe = str(tmp_path / "layout")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    rows = [list(map(int, l.split())) for l in subprocess.run([exe], capture_output=True, text=True, timeout=30).stdout.splitlines()]
    assert rows[0] == [48, 0, 4, 8, 12, 16, 20, 24, 32, 40]
    assert rows[1] == [80, 0, 4, 8, 12, 16, 20, 24, 28, 32, 36, 40, 48, 56, 64, 72] and rows[1][0] % 16 == 0
    assert rows[2] == [40, 0, 24, 28, 32, 36]
    S = vislam.BaParams
    assert [C.sizeof(S)] + [getattr(S, f).offset for f in B_FIELDS] == rows[0]
    for fields, row, dts in ((W_FIELDS, rows[1], (vislam.BA_WINDOW_DTYPE, br.WINDOW_DTYPE)), (P_FIELDS, rows[2], (vislam.BA_POINT_DTYPE, br.POINT_DTYPE))):
        for d in dts:
            assert d.names == fields and [d.itemsize] + [d.fields[k][1] for k in fields] == row, d
    assert rows[3][0] == 5                                         # VIS_ABI_VERSION: only new symbols and new structs
    assert rows[3][1] == 144 == C.sizeof(vislam.Params)            # vis_params did not grow
    assert rows[3][2:6] == [vislam.BA_REFINED, vislam.BA_FEW, vislam.BA_RESTART, vislam.BA_NO_SCALE] == \
        [br.BA_REFINED, br.BA_FEW, br.BA_RESTART, br.BA_NO_SCALE] == [1, 2, 4, 8]
    assert rows[3][6:] == [vislam.BAP_USED, vislam.BAP_INIT_REJECTED, vislam.BAP_FEW] == [br.BAP_USED, br.BAP_INIT_REJECTED, br.BAP_FEW] == [1, 2, 4]


def test_defaults(vislam):
    bp, want = vislam.default_ba_params(), br.Params()
    assert [getattr(bp, f) for f in B_FIELDS] == [8, 2, 12, 10, 5, 0, 2.4477, 16.0, 1e-4]
    assert [getattr(bp, f) for f in B_FIELDS if f != "reserved_"] == [getattr(want, f) for f in B_FIELDS if f != "reserved_"]
    vislam.lib.vis_default_ba_params(None)                         # a NULL pointer is ignored
    assert [vislam.ba_windows(n, 8) for n in (0, 1, 2, 9, 10, 17)] == [br.n_windows(n, 8) for n in (0, 1, 2, 9, 10, 17)] == [0, 0, 1, 1, 2, 2]


def test_symbols_exported_and_listed(vislam):
    for s in SYMBOLS:
        assert hasattr(vislam.lib, s) and s in vislam.ABI_SYMBOLS, s
    for name in ("ba_rows", "batch_ba"):
        assert callable(getattr(vislam.Context, name)), name
    out = subprocess.run(["nm", "-D", "--defined-only", vislam.LIB_PATH], capture_output=True, text=True, timeout=60).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    assert set(SYMBOLS) <= exported


def test_errors_that_need_no_device(vislam):
    L = vislam.lib
    a16, a8, a4, odd16, odd8, odd4 = (C.c_void_p(v) for v in (64, 72, 68, 72, 68, 66))   # never dereferenced: the argument / context checks come first
    bp = vislam.default_ba_params()
    ok = C.byref(bp)
    rows = lambda bp_=ok, n=2, prev=a4, nkp=a4, obs=a16, cap=8, xy=a8, poses=a8, out=a8, win=a8, pts=a8, fl=a4: \
        L.vis_ba_rows(None, bp_, n, prev, nkp, obs, cap, xy, poses, out, win, pts, fl)
    plan = lambda bp_=ok, n=2, obs=a16, cap=8, poses=a8, out=a8, win=a8, pts=a8, fl=a4: L.vis_batch_ba(None, bp_, n, obs, cap, poses, out, win, pts, fl)
    # VIS_E_STATE (no context) after every VIS_E_INVALID and before VIS_E_CAPACITY
    assert rows() == -5 and plan() == -5 and rows(n=0) == -5 and rows(n=1 << 20, cap=1 << 20) == -5 and plan(n=1 << 20, cap=1 << 20) == -5
    for k in ("bp_", "prev", "nkp", "obs", "xy", "poses", "out", "win", "pts", "fl"):
        assert rows(**{k: None}) == -1, k
    for k in ("bp_", "obs", "poses", "out", "win", "pts", "fl"):
        assert plan(**{k: None}) == -1, k
    assert rows(obs=odd16) == -1 and rows(xy=odd8) == -1 and rows(poses=odd8) == -1 and rows(out=odd8) == -1 and rows(win=odd8) == -1 and rows(pts=odd8) == -1
    assert rows(prev=odd4) == -1 and rows(nkp=odd4) == -1 and rows(n=-1) == -1 and rows(cap=-1) == -1
    assert plan(obs=odd16) == -1 and plan(poses=odd8) == -1 and plan(out=odd8) == -1 and plan(win=odd8) == -1 and plan(pts=odd8) == -1
    assert plan(n=-1) == -1 and plan(cap=-1) == -1
    assert rows(n=-1, cap=1 << 30) == -1 and rows(bp_=None, n=1 << 20, cap=1 << 20) == -1     # VIS_E_INVALID first
    nan, inf, up, down = float("nan"), float("inf"), lambda v: math.nextafter(v, inf), lambda v: math.nextafter(v, -inf)
    bad = [("stride", 0), ("stride", 17), ("min_views", 1), ("min_views", 18), ("min_points", 0), ("lm_iters", -1), ("lm_iters", 31),
           ("tri_gn_iters", -1), ("tri_gn_iters", 11), ("huber_px", down(0.0)), ("huber_px", inf), ("huber_px", nan), ("init_reproj_px", 0.0),
           ("init_reproj_px", up(1e6)), ("init_reproj_px", nan), ("init_reproj_px", inf), ("lambda0", down(1e-12)), ("lambda0", up(1e12)),
           ("lambda0", nan), ("lambda0", inf)]
    for f, v in bad:
        q = vislam.default_ba_params()
        setattr(q, f, v)
        assert rows(bp_=C.byref(q)) == -1 and plan(bp_=C.byref(q)) == -1, (f, v)
    good = [("stride", 1), ("stride", 16), ("min_views", 2), ("min_views", 17), ("min_points", 1), ("min_points", 2 ** 31 - 1), ("lm_iters", 0),
            ("lm_iters", 30), ("tri_gn_iters", 0), ("tri_gn_iters", 10), ("huber_px", 0.0), ("huber_px", 1.7976931348623157e308),
            ("init_reproj_px", 5e-324), ("init_reproj_px", 1e6), ("lambda0", 1e-12), ("lambda0", 1e12)]
    for f, v in good:
        q = vislam.default_ba_params()
        setattr(q, f, v)
        assert rows(bp_=C.byref(q)) == -5 and plan(bp_=C.byref(q)) == -5, (f, v)
