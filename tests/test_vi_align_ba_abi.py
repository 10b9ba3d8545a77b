"""CPU: the alignment with the accelerometer bias in the C ABI -- vis_vi_align_ba_params (32 bytes), vis_vi_align_ba (304, dba at byte 160, a complete
vis_vi_align in front) and vis_vi_ba_carry (1280) in the C compiler's layout (C99 and C++11, -pedantic -Werror), in the ctypes / numpy bindings and in
the restatement; the enums and the defaults; the four symbols exported and listed; every refusal that needs no device, in the header's order;
VIS_ABI_VERSION, vis_params and the sizes of the existing alignment structs unchanged."""
import ctypes as C
import os
import subprocess

import pytest

import vi_align_ba_ref as br

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("vis_default_vi_align_ba_params", "vis_vi_align_ba_rows", "vis_batch_vi_align_ba", "vis_batch_vi_align_ba_init")
P_FIELDS = ("pivot_rel", "min_ba_triples", "reserved_")
A_FIELDS = ("a", "dba", "s_ba", "g_ba", "dba_lin", "s_lin7", "g_lin7", "g_lin7_norm", "rms_ba", "n_ba_triples", "n_ba_triples_call", "ba_flags", "reserved_")
K_FIELDS = ("carry", "ba", "n_ba_triples", "reserved_", "last_jac")

SNIPPET = r"""
#include <stddef.h>
#include <stdio.h>
#include "vislam_hip.h"
#define P(f) (int)offsetof(vis_vi_align_ba_params, f)
#define A(f) (int)offsetof(vis_vi_align_ba, f)
#define K(f) (int)offsetof(vis_vi_ba_carry, f)
int main(void) {
    printf("%d %d %d %d\n", (int)sizeof(vis_vi_align_ba_params), P(pivot_rel), P(min_ba_triples), P(reserved_));
    printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d\n", (int)sizeof(vis_vi_align_ba), A(a), A(dba), A(s_ba), A(g_ba), A(dba_lin), A(s_lin7), A(g_lin7),
           A(g_lin7_norm), A(rms_ba), A(n_ba_triples), A(n_ba_triples_call), A(ba_flags), A(reserved_));
    printf("%d %d %d %d %d %d\n", (int)sizeof(vis_vi_ba_carry), K(carry), K(ba), K(n_ba_triples), K(reserved_), K(last_jac));
    printf("%d %d %d %d %d %d %d\n", VIS_ABI_VERSION, (int)sizeof(vis_params), (int)sizeof(vis_vi_align_params), (int)sizeof(vis_vi_state),
           (int)sizeof(vis_vi_align), (int)sizeof(vis_vi_tail), (int)sizeof(vis_vi_carry));
    printf("%d %d %d %d %d %d\n", (int)VIS_VIAB_OK, (int)VIS_VIAB_FEW, (int)VIS_VIAB_UNOBSERVABLE, (int)VIS_VIAB_SCALE, (int)VIS_VIAB_BAD_CARRY, (int)VIS_VIAB_SUMS);
    printf("%d\n", VIS_VIAB_PIVOT_REL == 1.0 / 1073741824.0);
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
    assert rows[0] == [32, 0, 8, 12]
    assert rows[1] == [304, 0, 160, 184, 192, 216, 240, 248, 272, 280, 288, 292, 296, 300]
    assert rows[2] == [1280, 0, 720, 976, 980, 984]
    assert [C.sizeof(vislam.ViAlignBaParams)] + [getattr(vislam.ViAlignBaParams, f).offset for f in P_FIELDS] == rows[0]
    assert [C.sizeof(vislam.ViBaCarry)] + [getattr(vislam.ViBaCarry, f).offset for f in K_FIELDS] == rows[2]
    for fields, row, dts in ((A_FIELDS, rows[1], (vislam.VI_ALIGN_BA_DTYPE, br.BA_RESULT_DTYPE)), (K_FIELDS, rows[2], (vislam.VI_BA_CARRY_DTYPE, br.BA_CARRY_DTYPE))):
        for d in dts:
            assert d.names == fields and [d.itemsize] + [d.fields[k][1] for k in fields] == row, d
    assert vislam.VI_ALIGN_BA_DTYPE.fields["a"][0] == vislam.VI_ALIGN_DTYPE and vislam.VI_ALIGN_BA_DBA_OFFSET == 160    # the chain: dbg at 0, dba at 160
    assert vislam.VI_BA_CARRY_DTYPE.fields["carry"][0] == vislam.VI_CARRY_DTYPE
    assert rows[3] == [5, 144, 128, 64, 160, 136, 720]                 # VIS_ABI_VERSION stays 5 and no existing struct changes
    names = ("FEW", "UNOBSERVABLE", "SCALE", "BAD_CARRY")
    assert rows[4] == [vislam.VIAB_OK] + [getattr(vislam, "VIAB_" + k) for k in names] + [vislam.VIAB_SUMS] == \
        [0] + [getattr(br, "VIAB_" + k) for k in names] + [br.N_BA] == [0, 1, 2, 4, 8, 32]
    assert rows[5] == [1] and vislam.VIAB_PIVOT_REL == br.PIVOT_REL == 2.0 ** -30


def test_defaults(vislam):
    bp, want = vislam.default_vi_align_ba_params(), br.BaParams()
    assert (bp.pivot_rel, bp.min_ba_triples) == (want.pivot_rel, want.min_ba_triples) == (2.0 ** -30, 16) and list(bp.reserved_) == [0] * 5
    vislam.lib.vis_default_vi_align_ba_params(None)                # a NULL pointer is ignored


def test_symbols_exported_and_listed(vislam):
    for s in SYMBOLS:
        assert hasattr(vislam.lib, s) and s in vislam.ABI_SYMBOLS, s
    for name in ("vi_align_ba_rows", "batch_vi_align_ba", "batch_vi_align_ba_init"):
        assert callable(getattr(vislam.Context, name)), name
    out = subprocess.run(["nm", "-D", "--defined-only", vislam.LIB_PATH], capture_output=True, text=True, timeout=60).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    assert set(SYMBOLS) <= exported
    assert not hasattr(vislam.lib, "vis_vi_align_ba")              # no host-pointer single form


def test_errors_that_need_no_device(vislam):
    L = vislam.lib
    a8, a4, odd8, odd4 = (C.c_void_p(v) for v in (72, 68, 68, 66))   # never dereferenced: the argument / context checks come first
    b8 = C.c_void_p(80)
    ok, okb = C.byref(vislam.default_vi_align_params()), C.byref(vislam.default_vi_align_ba_params())
    rows = lambda vp=ok, bp=okb, n=1, prev=a4, traj=a8, delta=a8, jac=a8, cin=None, state=None, result=a8, cout=None: \
        L.vis_vi_align_ba_rows(None, vp, bp, n, prev, traj, delta, jac, cin, state, result, cout)
    assert rows() == -5 and rows(cin=a8, state=a8, cout=b8) == -5 and rows(n=0) == -5
    assert rows(n=vislam.VIA_MAX_FRAMES + 1) == -5                   # the capacity refusal comes after the context's
    for k in ("vp", "bp", "prev", "traj", "delta", "jac", "result"):
        assert rows(**{k: None}) == -1, k
    for k in ("traj", "delta", "jac", "cin", "state", "result", "cout"):
        assert rows(**{k: odd8}) == -1, k
    assert rows(prev=odd4) == -1 and rows(n=-1) == -1 and rows(cin=a8, cout=a8) == -1
    plan = lambda vp=ok, bp=okb, n=1, traj=a8, delta=a8, jac=a8, state=None, result=a8: L.vis_batch_vi_align_ba(None, vp, bp, n, traj, delta, jac, state, result)
    assert plan() == -5 and plan(state=a8) == -5 and plan(n=vislam.VIA_MAX_FRAMES + 1) == -5
    for k in ("vp", "bp", "traj", "delta", "jac", "result"):
        assert plan(**{k: None}) == -1, k
    for k in ("traj", "delta", "jac", "state", "result"):
        assert plan(**{k: odd8}) == -1, k
    assert plan(n=-1) == -1
    assert L.vis_batch_vi_align_ba_init(None, None) == -5 and L.vis_batch_vi_align_ba_init(None, C.byref(vislam.ViBaCarry())) == -5
    # ---- the parameters: the sibling's rules for vp; pivot_rel finite and in [0, 1), min_ba_triples >= 1
    nan, inf = float("nan"), float("inf")
    q = vislam.default_vi_align_params()
    q.G = nan
    assert rows(vp=C.byref(q)) == -1 and plan(vp=C.byref(q)) == -1
    for f, v in (("pivot_rel", nan), ("pivot_rel", inf), ("pivot_rel", -1e-12), ("pivot_rel", 1.0), ("min_ba_triples", 0), ("min_ba_triples", -4)):
        b = vislam.default_vi_align_ba_params()
        setattr(b, f, v)
        assert rows(bp=C.byref(b)) == -1 and plan(bp=C.byref(b)) == -1, (f, v)
    for f, v in (("pivot_rel", 0.0), ("pivot_rel", 0.5), ("min_ba_triples", 1), ("min_ba_triples", 1 << 20)):
        b = vislam.default_vi_align_ba_params()
        setattr(b, f, v)
        assert rows(bp=C.byref(b)) == -5 and plan(bp=C.byref(b)) == -5, (f, v)
