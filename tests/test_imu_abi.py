"""CPU: the IMU preintegration's place in the C ABI -- vis_imu_sample (56 bytes), vis_imu_params (136), vis_imu_delta (216) and vis_imu_carry (232)
in the C compiler's layout (C99 and C++11, -pedantic -Werror), in the ctypes / numpy bindings and in the restatement; the enums, the series
coefficients and the defaults; the five symbols exported and listed; every refusal that needs no device, in the header's order; VIS_ABI_VERSION
and vis_params unchanged."""
import ctypes as C
import math
import os
import subprocess

import pytest

import imu_ref as ir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("vis_default_imu_params", "vis_imu_preintegrate", "vis_imu_preintegrate_rows", "vis_batch_imu", "vis_batch_imu_init")
S_FIELDS = ("t", "w", "a")
P_FIELDS = ("bg", "ba", "r_ic", "max_gap_s", "max_angle")
D_FIELDS = ("R", "v", "p", "dt", "JRg", "n_steps", "flags", "q", "reserved_")
C_FIELDS = ("t_last", "open", "valid", "reserved_")

SNIPPET = r"""
#include <stddef.h>
#include <stdio.h>
#include "vislam_hip.h"
#define S(f) (int)offsetof(vis_imu_sample, f)
#define P(f) (int)offsetof(vis_imu_params, f)
#define D(f) (int)offsetof(vis_imu_delta, f)
#define K(f) (int)offsetof(vis_imu_carry, f)
static const double cA[VIS_IMU_EXP_TERMS] = VIS_IMU_COEF_A, cB[VIS_IMU_EXP_TERMS] = VIS_IMU_COEF_B, cC[VIS_IMU_EXP_TERMS] = VIS_IMU_COEF_C;
int main(void) {
    int k;
    printf("%d %d %d %d\n", (int)sizeof(vis_imu_sample), S(t), S(w), S(a));
    printf("%d %d %d %d %d %d\n", (int)sizeof(vis_imu_params), P(bg), P(ba), P(r_ic), P(max_gap_s), P(max_angle));
    printf("%d %d %d %d %d %d %d %d %d %d\n", (int)sizeof(vis_imu_delta), D(R), D(v), D(p), D(dt), D(JRg), D(n_steps), D(flags), D(q), D(reserved_));
    printf("%d %d %d %d %d\n", (int)sizeof(vis_imu_carry), K(t_last), K(open), K(valid), K(reserved_));
    printf("%d %d %d %d\n", VIS_ABI_VERSION, (int)sizeof(vis_params), (int)VIS_IMU_MAX_FRAMES, (int)VIS_IMU_EXP_TERMS);
    printf("%d %d %d %d %d %d %d %d %d %d\n", (int)VIS_IMU_OK, (int)VIS_IMU_NO_PAIR, (int)VIS_IMU_NO_CARRY, (int)VIS_IMU_NO_START, (int)VIS_IMU_EMPTY,
           (int)VIS_IMU_EXTRAPOLATED, (int)VIS_IMU_GAP, (int)VIS_IMU_FAST, (int)VIS_IMU_ORDER, (int)VIS_IMU_NONFINITE);
    printf("%d %d\n", (int)VIS_IMU_CARRY_TIME, (int)VIS_IMU_CARRY_OPEN);
    for (k = 0; k < VIS_IMU_EXP_TERMS; k++) printf("%.17g %.17g %.17g\n", cA[k], cB[k], cC[k]);
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
    lines = subprocess.run([exe], capture_output=True, text=True, timeout=30).stdout.splitlines()
    rows = [list(map(int, l.split())) for l in lines[:7]]
    assert rows[0] == [56, 0, 8, 32]
    assert rows[1] == [136, 0, 24, 48, 120, 128]
    assert rows[2] == [216, 0, 72, 96, 120, 128, 200, 204, 208, 212]
    assert rows[3] == [232, 0, 8, 224, 228]
    for cls, fields, row in ((vislam.ImuSample, S_FIELDS, rows[0]), (vislam.ImuParams, P_FIELDS, rows[1]), (vislam.ImuDelta, D_FIELDS, rows[2]),
                             (vislam.ImuCarry, C_FIELDS, rows[3])):
        assert [C.sizeof(cls)] + [getattr(cls, f).offset for f in fields] == row, cls
    for fields, row, dts in ((S_FIELDS, rows[0], (vislam.IMU_SAMPLE_DTYPE, ir.SAMPLE_DTYPE)), (D_FIELDS, rows[2], (vislam.IMU_DELTA_DTYPE, ir.DELTA_DTYPE)),
                             (C_FIELDS, rows[3], (vislam.IMU_CARRY_DTYPE, ir.CARRY_DTYPE))):
        for d in dts:
            assert d.names == fields and [d.itemsize] + [d.fields[k][1] for k in fields] == row, d
    assert rows[4] == [5, 144, vislam.IMU_MAX_FRAMES, 10] and C.sizeof(vislam.Params) == 144 and ir.IMU_MAX_FRAMES == 1024 and ir.IMU_EXP_TERMS == 10
    names = ("OK", "NO_PAIR", "NO_CARRY", "NO_START", "EMPTY", "EXTRAPOLATED", "GAP", "FAST", "ORDER", "NONFINITE")
    assert rows[5] == [getattr(vislam, "IMU_" + k) for k in names] == [getattr(ir, "IMU_" + k) for k in names] == [0, 1, 2, 4, 8, 16, 32, 64, 128, 256]
    assert rows[6] == [vislam.IMU_CARRY_TIME, vislam.IMU_CARRY_OPEN] == [ir.IMU_CARRY_TIME, ir.IMU_CARRY_OPEN] == [1, 2]
    # the series coefficients: the header's literals are the restatement's doubles, each the double nearest to (-1)^k / (2k + j)!
    coef = [list(map(float, l.split())) for l in lines[7:17]]
    for k in range(10):
        assert coef[k] == [ir.COEF_A[k], ir.COEF_B[k], ir.COEF_C[k]] == [(-1) ** k / math.factorial(2 * k + j) for j in (1, 2, 3)], k


def test_defaults(vislam):
    ip, want = vislam.default_imu_params(), ir.Params()
    assert list(ip.bg) == want.bg == [0.0] * 3 and list(ip.ba) == want.ba == [0.0] * 3 and list(ip.r_ic) == want.r_ic == ir.EYE
    assert (ip.max_gap_s, ip.max_angle) == (want.max_gap_s, want.max_angle) == (0.05, 1.0)
    vislam.lib.vis_default_imu_params(None)                        # a NULL pointer is ignored


def test_symbols_exported_and_listed(vislam):
    for s in SYMBOLS:
        assert hasattr(vislam.lib, s) and s in vislam.ABI_SYMBOLS, s
    for name in ("imu_preintegrate", "imu_preintegrate_rows", "batch_imu", "batch_imu_init"):
        assert callable(getattr(vislam.Context, name)), name
    out = subprocess.run(["nm", "-D", "--defined-only", vislam.LIB_PATH], capture_output=True, text=True, timeout=60).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    assert set(SYMBOLS) <= exported


def test_errors_that_need_no_device(vislam):
    L = vislam.lib
    a8, a4, odd8, odd4 = (C.c_void_p(v) for v in (72, 68, 68, 66))   # never dereferenced: the argument / context checks come first
    b8 = C.c_void_p(80)
    ok = C.byref(vislam.default_imu_params())
    rows = lambda ip=ok, n=1, s=a8, ns=4, tf=a8, prev=a4, cin=None, delta=a8, rot=None, cout=None: \
        L.vis_imu_preintegrate_rows(None, ip, n, s, ns, tf, prev, cin, delta, rot, cout)
    assert rows() == -5 and rows(cin=a8, rot=a4, cout=b8) == -5 and rows(n=0) == -5 and rows(s=None, ns=0) == -5
    assert rows(n=vislam.IMU_MAX_FRAMES + 1) == -5                   # the capacity refusal comes after the context's
    for k in ("ip", "tf", "prev", "delta", "s"):
        assert rows(**{k: None}) == -1, k
    assert rows(s=odd8) == -1 and rows(tf=odd8) == -1 and rows(cin=odd8) == -1 and rows(delta=odd8) == -1 and rows(cout=odd8) == -1
    assert rows(prev=odd4) == -1 and rows(rot=odd4) == -1 and rows(n=-1) == -1 and rows(ns=-1) == -1 and rows(cin=a8, cout=a8) == -1
    plan = lambda ip=ok, n=1, s=a8, ns=4, tf=a8, delta=a8, rot=None: L.vis_batch_imu(None, ip, n, s, ns, tf, delta, rot)
    assert plan() == -5 and plan(rot=a4) == -5 and plan(s=None, ns=0) == -5 and plan(n=vislam.IMU_MAX_FRAMES + 1) == -5
    for k in ("ip", "tf", "delta", "s"):
        assert plan(**{k: None}) == -1, k
    assert plan(s=odd8) == -1 and plan(tf=odd8) == -1 and plan(delta=odd8) == -1 and plan(rot=odd4) == -1 and plan(n=-1) == -1 and plan(ns=-1) == -1
    d = vislam.ImuDelta()
    one = lambda ip=ok, s=a8, ns=4, delta=C.byref(d): L.vis_imu_preintegrate(None, ip, s, ns, 0.0, 1.0, delta, None)
    assert one() == -5 and one(s=None, ns=0) == -5
    assert one(ip=None) == -1 and one(delta=None) == -1 and one(ns=-1) == -1 and one(s=None) == -1
    assert L.vis_batch_imu_init(None, None) == -5 and L.vis_batch_imu_init(None, C.byref(vislam.ImuCarry())) == -5
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
    for f, v in (("max_gap_s", 1e-9), ("max_angle", 1e-9), ("max_gap_s", 1e9), ("max_angle", 1e9)):
        q = vislam.default_imu_params()
        setattr(q, f, v)
        assert rows(ip=C.byref(q)) == -5 and plan(ip=C.byref(q)) == -5 and one(ip=C.byref(q)) == -5, (f, v)
