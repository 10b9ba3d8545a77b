"""CPU: the bias Jacobians' and the correction's place in the C ABI -- vis_imu_bias_jac (296 bytes) and vis_imu_jac_carry (528) in the C compiler's
layout (C99 and C++11, -pedantic -Werror), in the ctypes / numpy bindings and in the restatement; the enums; the six symbols exported and listed;
every refusal that needs no device, in the header's order; VIS_ABI_VERSION and the existing IMU records unchanged."""
import ctypes as C
import os
import subprocess

import pytest

import imu_jac_ref as jr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("vis_imu_preintegrate_jac", "vis_imu_preintegrate_jac_rows", "vis_batch_imu_jac", "vis_batch_imu_jac_init", "vis_imu_correct_rows",
           "vis_batch_imu_correct")
J_FIELDS = ("Jvg", "Jva", "Jpg", "Jpa", "flags", "q")
C_FIELDS = ("carry", "open_jac")

SNIPPET = r"""
#include <stddef.h>
#include <stdio.h>
#include "vislam_hip.h"
#define J(f) (int)offsetof(vis_imu_bias_jac, f)
#define K(f) (int)offsetof(vis_imu_jac_carry, f)
int main(void) {
    printf("%d %d %d %d %d %d %d\n", (int)sizeof(vis_imu_bias_jac), J(Jvg), J(Jva), J(Jpg), J(Jpa), J(flags), J(q));
    printf("%d %d %d\n", (int)sizeof(vis_imu_jac_carry), K(carry), K(open_jac));
    printf("%d %d %d %d %d\n", VIS_ABI_VERSION, (int)sizeof(vis_imu_delta), (int)sizeof(vis_imu_carry), (int)sizeof(vis_imu_params), (int)sizeof(vis_vi_align));
    printf("%d %d\n", (int)VIS_IMU_JAC_OK, (int)VIS_IMU_JAC_NONFINITE);
    printf("%d %d %d %d %d %d\n", (int)VIS_IMC_OK, (int)VIS_IMC_UNUSABLE, (int)VIS_IMC_JAC, (int)VIS_IMC_BIAS, (int)VIS_IMC_ANGLE, (int)VIS_IMC_NONFINITE);
    printf("%d\n", (int)offsetof(vis_vi_align, dbg));
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
    assert rows[0] == [296, 0, 72, 144, 216, 288, 292]
    assert rows[1] == [528, 0, 232]
    assert rows[2] == [5, 216, 232, 136, 160]
    for cls, fields, row in ((vislam.ImuBiasJac, J_FIELDS, rows[0]), (vislam.ImuJacCarry, C_FIELDS, rows[1])):
        assert [C.sizeof(cls)] + [getattr(cls, f).offset for f in fields] == row, cls
    for fields, row, dts in ((J_FIELDS, rows[0], (vislam.IMU_BIAS_JAC_DTYPE, jr.JAC_DTYPE)), (C_FIELDS, rows[1], (vislam.IMU_JAC_CARRY_DTYPE, jr.JAC_CARRY_DTYPE))):
        for d in dts:
            assert d.names == fields and [d.itemsize] + [d.fields[k][1] for k in fields] == row, d
    assert vislam.IMU_JAC_CARRY_DTYPE.fields["carry"][0] == vislam.IMU_CARRY_DTYPE and jr.JAC_CARRY_DTYPE.fields["carry"][0] == jr.ir.CARRY_DTYPE
    assert rows[3] == [vislam.IMU_JAC_OK, vislam.IMU_JAC_NONFINITE] == [jr.IMU_JAC_OK, jr.IMU_JAC_NONFINITE] == [0, 1]
    names = ("OK", "UNUSABLE", "JAC", "BIAS", "ANGLE", "NONFINITE")
    assert rows[4] == [getattr(vislam, "IMC_" + k) for k in names] == [getattr(jr, "IMC_" + k) for k in names] == [0, 1, 2, 4, 8, 16]
    assert rows[5] == [0] == [vislam.VI_ALIGN_DTYPE.fields["dbg"][1]]      # d_dbg may point at an alignment's record


def test_symbols_exported_and_listed(vislam):
    for s in SYMBOLS:
        assert hasattr(vislam.lib, s) and s in vislam.ABI_SYMBOLS, s
    for name in ("imu_preintegrate_jac", "imu_preintegrate_jac_rows", "batch_imu_jac", "batch_imu_jac_init", "imu_correct_rows", "batch_imu_correct"):
        assert callable(getattr(vislam.Context, name)), name
    out = subprocess.run(["nm", "-D", "--defined-only", vislam.LIB_PATH], capture_output=True, text=True, timeout=60).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    assert set(SYMBOLS) <= exported


def test_errors_that_need_no_device(vislam):
    L = vislam.lib
    a8, a4, odd8, odd4 = (C.c_void_p(v) for v in (72, 68, 68, 66))   # never dereferenced: the argument / context checks come first
    b8 = C.c_void_p(80)
    ok = C.byref(vislam.default_imu_params())
    rows = lambda ip=ok, n=1, s=a8, ns=4, tf=a8, prev=a4, cin=None, delta=a8, jac=a8, rot=None, cout=None: \
        L.vis_imu_preintegrate_jac_rows(None, ip, n, s, ns, tf, prev, cin, delta, jac, rot, cout)
    assert rows() == -5 and rows(cin=a8, rot=a4, cout=b8) == -5 and rows(n=0) == -5 and rows(s=None, ns=0) == -5
    assert rows(n=vislam.IMU_MAX_FRAMES + 1) == -5                   # the capacity refusal comes after the context's
    for k in ("ip", "tf", "prev", "delta", "jac", "s"):
        assert rows(**{k: None}) == -1, k
    for k in ("s", "tf", "cin", "delta", "jac", "cout"):
        assert rows(**{k: odd8}) == -1, k
    assert rows(prev=odd4) == -1 and rows(rot=odd4) == -1 and rows(n=-1) == -1 and rows(ns=-1) == -1 and rows(cin=a8, cout=a8) == -1
    plan = lambda ip=ok, n=1, s=a8, ns=4, tf=a8, delta=a8, jac=a8, rot=None: L.vis_batch_imu_jac(None, ip, n, s, ns, tf, delta, jac, rot)
    assert plan() == -5 and plan(rot=a4) == -5 and plan(s=None, ns=0) == -5 and plan(n=vislam.IMU_MAX_FRAMES + 1) == -5
    for k in ("ip", "tf", "delta", "jac", "s"):
        assert plan(**{k: None}) == -1, k
    for k in ("s", "tf", "delta", "jac"):
        assert plan(**{k: odd8}) == -1, k
    assert plan(rot=odd4) == -1 and plan(n=-1) == -1 and plan(ns=-1) == -1
    d, j = vislam.ImuDelta(), vislam.ImuBiasJac()
    one = lambda ip=ok, s=a8, ns=4, delta=C.byref(d), jac=C.byref(j): L.vis_imu_preintegrate_jac(None, ip, s, ns, 0.0, 1.0, delta, jac, None)
    assert one() == -5 and one(s=None, ns=0) == -5
    assert one(ip=None) == -1 and one(delta=None) == -1 and one(jac=None) == -1 and one(ns=-1) == -1 and one(s=None) == -1
    assert L.vis_batch_imu_jac_init(None, None) == -5 and L.vis_batch_imu_jac_init(None, C.byref(vislam.ImuJacCarry())) == -5
    # ---- the correction, both forms
    for f in (L.vis_imu_correct_rows, L.vis_batch_imu_correct):
        cor = lambda ip=ok, n=1, delta=a8, jac=a8, dbg=a8, dba=None, out=b8, rot=None, st=None: f(None, ip, n, delta, jac, dbg, dba, out, rot, st)
        assert cor() == -5 and cor(dba=a8, rot=a4, st=a4) == -5 and cor(n=0) == -5 and cor(n=vislam.IMU_MAX_FRAMES + 1) == -5
        for k in ("ip", "delta", "jac", "dbg", "out"):
            assert cor(**{k: None}) == -1, k
        for k in ("delta", "jac", "dbg", "dba", "out"):
            assert cor(**{k: odd8}) == -1, k
        assert cor(rot=odd4) == -1 and cor(st=odd4) == -1 and cor(n=-1) == -1 and cor(out=a8) == -1      # d_delta_out may not be d_delta
    # ---- the parameters: every field finite, both bounds > 0
    nan, inf = float("nan"), float("inf")
    for f, i, v in [(f, i, v) for f, m in (("bg", 3), ("ba", 3), ("r_ic", 9)) for i in (0, m - 1) for v in (nan, inf, -inf)] + \
                   [(f, None, v) for f in ("max_gap_s", "max_angle") for v in (nan, inf, 0.0, -1.0)]:
        q = vislam.default_imu_params()
        if i is None:
            setattr(q, f, v)
        else:
            getattr(q, f)[i] = v
        assert rows(ip=C.byref(q)) == -1 and plan(ip=C.byref(q)) == -1 and one(ip=C.byref(q)) == -1, (f, i, v)
        assert L.vis_imu_correct_rows(None, C.byref(q), 1, a8, a8, a8, None, b8, None, None) == -1, (f, i, v)
