"""CPU: the visual-inertial alignment's place in the C ABI -- vis_vi_align_params (128 bytes), vis_vi_state (64), vis_vi_align (160), vis_vi_tail (136)
and vis_vi_carry (720) in the C compiler's layout (C99 and C++11, -pedantic -Werror), in the ctypes / numpy bindings and in the restatement; the
enums and the defaults; the four symbols exported and listed; every refusal that needs no device, in the header's order; VIS_ABI_VERSION and
vis_params unchanged."""
import ctypes as C
import os
import subprocess

import pytest

import imu_ref as ir
import vi_align_ref as vr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("vis_default_vi_align_params", "vis_vi_align_rows", "vis_batch_vi_align", "vis_batch_vi_align_init")
P_FIELDS = ("r_ic", "p_ci", "G", "g_tol", "min_pairs", "min_triples", "refine_iters", "reject")
S_FIELDS = ("p", "v", "res", "flags", "q")
A_FIELDS = ("dbg", "c0", "c0_call", "c1", "s", "g", "s_lin", "g_lin", "g_lin_norm", "rms", "n_pairs", "n_triples", "n_pairs_call", "n_triples_call",
            "segment_seq", "epoch_seq", "flags", "reserved_")
T_FIELDS = ("C", "Rw", "L", "segment_seq", "epoch_seq", "flags", "reserved_")
K_FIELDS = ("gyro", "lin", "n_pairs", "n_triples", "segment_seq", "epoch_seq", "last", "parent", "last_delta", "valid", "reserved_")

SNIPPET = r"""
#include <stddef.h>
#include <stdio.h>
#include "vislam_hip.h"
#define P(f) (int)offsetof(vis_vi_align_params, f)
#define S(f) (int)offsetof(vis_vi_state, f)
#define A(f) (int)offsetof(vis_vi_align, f)
#define T(f) (int)offsetof(vis_vi_tail, f)
#define K(f) (int)offsetof(vis_vi_carry, f)
int main(void) {
    printf("%d %d %d %d %d %d %d %d %d\n", (int)sizeof(vis_vi_align_params), P(r_ic), P(p_ci), P(G), P(g_tol), P(min_pairs), P(min_triples), P(refine_iters), P(reject));
    printf("%d %d %d %d %d %d\n", (int)sizeof(vis_vi_state), S(p), S(v), S(res), S(flags), S(q));
    printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n", (int)sizeof(vis_vi_align), A(dbg), A(c0), A(c0_call), A(c1), A(s), A(g), A(s_lin),
           A(g_lin), A(g_lin_norm), A(rms), A(n_pairs), A(n_triples), A(n_pairs_call), A(n_triples_call), A(segment_seq), A(epoch_seq), A(flags), A(reserved_));
    printf("%d %d %d %d %d %d %d %d\n", (int)sizeof(vis_vi_tail), T(C), T(Rw), T(L), T(segment_seq), T(epoch_seq), T(flags), T(reserved_));
    printf("%d %d %d %d %d %d %d %d %d %d %d %d\n", (int)sizeof(vis_vi_carry), K(gyro), K(lin), K(n_pairs), K(n_triples), K(segment_seq), K(epoch_seq), K(last),
           K(parent), K(last_delta), K(valid), K(reserved_));
    printf("%d %d %d\n", VIS_ABI_VERSION, (int)sizeof(vis_params), (int)VIS_VIA_MAX_FRAMES);
    printf("%d %d %d %d %d %d %d %d %d\n", (int)VIS_VIA_OK, (int)VIS_VIA_GYRO_FEW, (int)VIS_VIA_GYRO_SINGULAR, (int)VIS_VIA_FEW, (int)VIS_VIA_SINGULAR,
           (int)VIS_VIA_SCALE, (int)VIS_VIA_GRAVITY_NORM, (int)VIS_VIA_RESTART, (int)VIS_VIA_BAD_CARRY);
    printf("%d %d %d %d %d %d %d %d\n", (int)VIS_VIS_HAS_P, (int)VIS_VIS_HAS_V, (int)VIS_VIS_HAS_TRIPLE, (int)VIS_VIS_HAS_PAIR, (int)VIS_VIT_POSED,
           (int)VIS_VIT_EDGE, (int)VIS_VIT_DELTA, (int)VIS_VIC_VALID);
    return 0;
}
"""


@pytest.mark.parametrize("compiler", (["gcc", "-std=c99", "-x", "c"], ["g++", "-std=c++11", "-x", "c++"]), ids=("c99", "c++11"))
def test_layout_in_c_ctypes_numpy_and_the_restatement(vislam, tmp_path, compiler):
    src = tmp_path / "layout.src"
    src.write_text(SNIPPET)
    exe = str(tmp_path / "layout")
    r = subprocess.run(compiler + ["-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    rows = [list(map(int, l.split())) for l in subprocess.run([exe], capture_output=True, text=True, timeout=30).stdout.splitlines()]
    assert rows[0] == [128, 0, 72, 96, 104, 112, 116, 120, 124]
    assert rows[1] == [64, 0, 24, 48, 56, 60]
    assert rows[2] == [160, 0, 24, 32, 40, 48, 56, 80, 88, 112, 120, 128, 132, 136, 140, 144, 148, 152, 156]
    assert rows[3] == [136, 0, 24, 96, 120, 124, 128, 132]
    assert rows[4] == [720, 0, 80, 208, 212, 216, 220, 224, 360, 496, 712, 716]
    for cls, fields, row in ((vislam.ViAlignParams, P_FIELDS, rows[0]), (vislam.ViTail, T_FIELDS, rows[3]), (vislam.ViCarry, K_FIELDS, rows[4])):
        assert [C.sizeof(cls)] + [getattr(cls, f).offset for f in fields] == row, cls
    for fields, row, dts in ((S_FIELDS, rows[1], (vislam.VI_STATE_DTYPE, vr.STATE_DTYPE)), (A_FIELDS, rows[2], (vislam.VI_ALIGN_DTYPE, vr.RESULT_DTYPE)),
                             (T_FIELDS, rows[3], (vislam.VI_TAIL_DTYPE, vr.TAIL_DTYPE)), (K_FIELDS, rows[4], (vislam.VI_CARRY_DTYPE, vr.CARRY_DTYPE))):
        for d in dts:
            assert d.names == fields and [d.itemsize] + [d.fields[k][1] for k in fields] == row, d
    assert rows[5] == [5, 144, vislam.VIA_MAX_FRAMES] and vr.EXCITATION_REL == 9.094947017729282e-13 and C.sizeof(vislam.Params) == 144 and vr.VIA_MAX_FRAMES == 1024
    names = ("GYRO_FEW", "GYRO_SINGULAR", "FEW", "SINGULAR", "SCALE", "GRAVITY_NORM", "RESTART", "BAD_CARRY")
    assert rows[6] == [vislam.VIA_OK] + [getattr(vislam, "VIA_" + k) for k in names] == [0] + [getattr(vr, "VIA_" + k) for k in names] == [0, 1, 2, 4, 8, 16, 32, 64, 128]
    assert rows[7] == [vislam.VIS_HAS_P, vislam.VIS_HAS_V, vislam.VIS_HAS_TRIPLE, vislam.VIS_HAS_PAIR, vislam.VIT_POSED, vislam.VIT_EDGE, vislam.VIT_DELTA,
                       vislam.VIC_VALID] == [vr.VIS_HAS_P, vr.VIS_HAS_V, vr.VIS_HAS_TRIPLE, vr.VIS_HAS_PAIR, vr.VIT_POSED, vr.VIT_EDGE, vr.VIT_DELTA,
                                             vr.VIC_VALID] == [1, 2, 4, 8, 1, 2, 4, 1]


def test_defaults(vislam):
    vp, want = vislam.default_vi_align_params(), vr.Params()
    assert list(vp.r_ic) == want.r_ic == ir.EYE and list(vp.p_ci) == want.p_ci == [0.0] * 3
    assert (vp.G, vp.g_tol, vp.min_pairs, vp.min_triples, vp.refine_iters, vp.reject) == \
        (want.G, want.g_tol, want.min_pairs, want.min_triples, want.refine_iters, want.reject) == (9.81, 0.1, 8, 8, 4, ir.IMU_EMPTY | ir.IMU_GAP)
    vislam.lib.vis_default_vi_align_params(None)                   # a NULL pointer is ignored


def test_symbols_exported_and_listed(vislam):
    for s in SYMBOLS:
        assert hasattr(vislam.lib, s) and s in vislam.ABI_SYMBOLS, s
    for name in ("vi_align_rows", "batch_vi_align", "batch_vi_align_init"):
        assert callable(getattr(vislam.Context, name)), name
    out = subprocess.run(["nm", "-D", "--defined-only", vislam.LIB_PATH], capture_output=True, text=True, timeout=60).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    assert set(SYMBOLS) <= exported
    assert not hasattr(vislam.lib, "vis_vi_align")                 # no host-pointer single form: one interval aligns nothing


def test_errors_that_need_no_device(vislam):
    L = vislam.lib
    a8, a4, odd8, odd4 = (C.c_void_p(v) for v in (72, 68, 68, 66))   # never dereferenced: the argument / context checks come first
    b8 = C.c_void_p(80)
    ok = C.byref(vislam.default_vi_align_params())
    rows = lambda vp=ok, n=1, prev=a4, traj=a8, delta=a8, cin=None, state=None, result=a8, cout=None: \
        L.vis_vi_align_rows(None, vp, n, prev, traj, delta, cin, state, result, cout)
    assert rows() == -5 and rows(cin=a8, state=a8, cout=b8) == -5 and rows(n=0) == -5
    assert rows(n=vislam.VIA_MAX_FRAMES + 1) == -5                   # the capacity refusal comes after the context's
    for k in ("vp", "prev", "traj", "delta", "result"):
        assert rows(**{k: None}) == -1, k
    for k in ("traj", "delta", "cin", "state", "result", "cout"):
        assert rows(**{k: odd8}) == -1, k
    assert rows(prev=odd4) == -1 and rows(n=-1) == -1 and rows(cin=a8, cout=a8) == -1
    plan = lambda vp=ok, n=1, traj=a8, delta=a8, state=None, result=a8: L.vis_batch_vi_align(None, vp, n, traj, delta, state, result)
    assert plan() == -5 and plan(state=a8) == -5 and plan(n=vislam.VIA_MAX_FRAMES + 1) == -5
    for k in ("vp", "traj", "delta", "result"):
        assert plan(**{k: None}) == -1, k
    for k in ("traj", "delta", "state", "result"):
        assert plan(**{k: odd8}) == -1, k
    assert plan(n=-1) == -1
    assert L.vis_batch_vi_align_init(None, None) == -5 and L.vis_batch_vi_align_init(None, C.byref(vislam.ViCarry())) == -5
    # ---- the parameters: every field finite, G > 0, g_tol >= 0, the counts >= 1, refine_iters 0 ... 16
    nan, inf = float("nan"), float("inf")
    bad = [(f, i, v) for f, m in (("r_ic", 9), ("p_ci", 3)) for i in (0, m - 1) for v in (nan, inf, -inf)]
    bad += [("G", None, v) for v in (nan, inf, 0.0, -9.81)] + [("g_tol", None, v) for v in (nan, inf, -0.1)]
    bad += [("min_pairs", None, 0), ("min_triples", None, 0), ("min_pairs", None, -3), ("refine_iters", None, -1), ("refine_iters", None, 17)]
    for f, i, v in bad:
        q = vislam.default_vi_align_params()
        if i is None:
            setattr(q, f, v)
        else:
            getattr(q, f)[i] = v
        assert rows(vp=C.byref(q)) == -1 and plan(vp=C.byref(q)) == -1, (f, i, v)
    for f, v in (("G", 1e-9), ("g_tol", 0.0), ("g_tol", 1e9), ("refine_iters", 0), ("refine_iters", 16), ("min_pairs", 1), ("min_triples", 1 << 20),
                 ("reject", 0), ("reject", -1)):
        q = vislam.default_vi_align_params()
        setattr(q, f, v)
        assert rows(vp=C.byref(q)) == -5 and plan(vp=C.byref(q)) == -5, (f, v)
