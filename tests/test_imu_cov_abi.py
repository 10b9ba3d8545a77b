"""CPU: the covariance's place in the C ABI -- vis_imu_noise (16 bytes), vis_imu_cov (368) and vis_imu_cov_carry (600) in the C compiler's layout (C99
and C++11, -pedantic -Werror), in the ctypes / numpy bindings and in the restatement; the enums and the defaults; the symbols exported and listed;
every refusal that needs no device, in the header's order; VIS_ABI_VERSION and the existing IMU records unchanged."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import imu_cov_ref as cr
import imu_factor_ref as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("vis_default_imu_noise", "vis_imu_preintegrate_cov", "vis_imu_preintegrate_cov_rows", "vis_batch_imu_cov", "vis_batch_imu_cov_init",
           "vis_default_imu_factor_params", "vis_imu_factor_rows", "vis_batch_imu_factor")
F_FIELDS = ("r", "chi2", "chi2_rot", "flags", "q")
P_FIELDS = ("var_rot", "var_v", "var_p")
N_FIELDS = ("sigma_g", "sigma_a")
S_FIELDS = ("S", "flags", "q")
C_FIELDS = ("carry", "open_cov")

SNIPPET = r"""
#include <stddef.h>
#include <stdio.h>
#include "vislam_hip.h"
#define N(f) (int)offsetof(vis_imu_noise, f)
#define S(f) (int)offsetof(vis_imu_cov, f)
#define K(f) (int)offsetof(vis_imu_cov_carry, f)
int main(void) {
    printf("%d %d %d\n", (int)sizeof(vis_imu_noise), N(sigma_g), N(sigma_a));
    printf("%d %d %d %d\n", (int)sizeof(vis_imu_cov), S(S), S(flags), S(q));
    printf("%d %d %d\n", (int)sizeof(vis_imu_cov_carry), K(carry), K(open_cov));
    printf("%d %d %d %d %d %d %d\n", VIS_ABI_VERSION, (int)sizeof(vis_imu_delta), (int)sizeof(vis_imu_carry), (int)sizeof(vis_imu_params),
           (int)sizeof(vis_imu_bias_jac), (int)sizeof(vis_imu_jac_carry), (int)sizeof(vis_imu_sample));
    printf("%d %d\n", (int)VIS_IMU_COV_OK, (int)VIS_IMU_COV_NONFINITE);
    printf("%d %d %d %d %d %d\n", (int)sizeof(vis_imu_factor), (int)offsetof(vis_imu_factor, r), (int)offsetof(vis_imu_factor, chi2),
           (int)offsetof(vis_imu_factor, chi2_rot), (int)offsetof(vis_imu_factor, flags), (int)offsetof(vis_imu_factor, q));
    printf("%d %d %d %d\n", (int)sizeof(vis_imu_factor_params), (int)offsetof(vis_imu_factor_params, var_rot), (int)offsetof(vis_imu_factor_params, var_v),
           (int)offsetof(vis_imu_factor_params, var_p));
    printf("%d %d %d %d %d %d %d\n", (int)VIS_IMF_OK, (int)VIS_IMF_NO_PARENT, (int)VIS_IMF_NO_STATE, (int)VIS_IMF_NO_ALIGN, (int)VIS_IMF_UNUSABLE,
           (int)VIS_IMF_SINGULAR, (int)VIS_IMF_NONFINITE);
    printf("%d %d\n", (int)offsetof(vis_vi_align_ba, a), (int)sizeof(vis_vi_align));
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
    assert rows[0] == [16, 0, 8]
    assert rows[1] == [368, 0, 360, 364]
    assert rows[2] == [600, 0, 232]
    assert rows[3] == [5, 216, 232, 136, 296, 528, 56]                 # the ABI version and the existing IMU records are what they were
    for cls, fields, row in ((vislam.ImuNoise, N_FIELDS, rows[0]), (vislam.ImuCov, S_FIELDS, rows[1]), (vislam.ImuCovCarry, C_FIELDS, rows[2])):
        assert [C.sizeof(cls)] + [getattr(cls, f).offset for f in fields] == row, cls
    for fields, row, dts in ((N_FIELDS, rows[0], (cr.NOISE_DTYPE,)), (S_FIELDS, rows[1], (vislam.IMU_COV_DTYPE, cr.COV_DTYPE)),
                             (C_FIELDS, rows[2], (vislam.IMU_COV_CARRY_DTYPE, cr.COV_CARRY_DTYPE))):
        for d in dts:
            assert d.names == fields and [d.itemsize] + [d.fields[k][1] for k in fields] == row, d
    assert vislam.IMU_COV_CARRY_DTYPE.fields["carry"][0] == vislam.IMU_CARRY_DTYPE and cr.COV_CARRY_DTYPE.fields["carry"][0] == cr.ir.CARRY_DTYPE
    assert rows[4] == [vislam.IMU_COV_OK, vislam.IMU_COV_NONFINITE] == [cr.IMU_COV_OK, cr.IMU_COV_NONFINITE] == [0, 1]
    assert rows[5] == [96, 0, 72, 80, 88, 92] and rows[6] == [24, 0, 8, 16]
    for d in (vislam.IMU_FACTOR_DTYPE, fr.FACTOR_DTYPE):
        assert d.names == F_FIELDS and [d.itemsize] + [d.fields[k][1] for k in F_FIELDS] == rows[5], d
    assert [C.sizeof(vislam.ImuFactorParams)] + [getattr(vislam.ImuFactorParams, f).offset for f in P_FIELDS] == rows[6]
    assert fr.FACTOR_PARAMS_DTYPE.names == P_FIELDS and fr.FACTOR_PARAMS_DTYPE.itemsize == 24
    names = ("OK", "NO_PARENT", "NO_STATE", "NO_ALIGN", "UNUSABLE", "SINGULAR", "NONFINITE")
    assert rows[7] == [getattr(vislam, "IMF_" + k) for k in names] == [getattr(fr, "IMF_" + k) for k in names] == [0, 1, 2, 4, 8, 16, 32]
    assert rows[8] == [0, 160]                                        # d_result may point at a vis_vi_align_ba record


def test_defaults_and_the_matrix_of_a_record(vislam):
    nz = vislam.default_imu_noise()
    assert (nz.sigma_g, nz.sigma_a) == (1.6968e-4, 2.0e-3) == (cr.SIGMA_G, cr.SIGMA_A) == (cr.Noise().sigma_g, cr.Noise().sigma_a)
    vislam.lib.vis_default_imu_noise(None)                             # a NULL record is ignored
    rec = np.zeros(1, vislam.IMU_COV_DTYPE)
    rec[0]["S"] = np.arange(45.0)
    M = vislam.imu_cov_matrix(rec[0])
    assert (M == M.T).all() and M[np.triu_indices(9)].tolist() == list(range(45)) and (M == cr.matrix(rec[0])).all()
    assert M[0, 3] == 3.0 and M[3, 3] == 24.0 and M[8, 8] == 44.0     # row r starts at r 9 - r (r - 1) / 2


def test_symbols_exported_and_listed(vislam):
    for s in SYMBOLS:
        assert hasattr(vislam.lib, s) and s in vislam.ABI_SYMBOLS, s
    for name in ("imu_preintegrate_cov", "imu_preintegrate_cov_rows", "batch_imu_cov", "batch_imu_cov_init", "imu_factor_rows", "batch_imu_factor"):
        assert callable(getattr(vislam.Context, name)), name
    out = subprocess.run(["nm", "-D", "--defined-only", vislam.LIB_PATH], capture_output=True, text=True, timeout=60).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    assert set(SYMBOLS) <= exported


def test_errors_that_need_no_device(vislam):
    L = vislam.lib
    a8, a4, odd8, odd4 = (C.c_void_p(v) for v in (72, 68, 68, 66))   # never dereferenced: the argument / context checks come first
    b8 = C.c_void_p(80)
    ok, nz = C.byref(vislam.default_imu_params()), C.byref(vislam.default_imu_noise())
    rows = lambda ip=ok, np_=nz, n=1, s=a8, ns=4, tf=a8, prev=a4, cin=None, delta=a8, cov=a8, rot=None, cout=None: \
        L.vis_imu_preintegrate_cov_rows(None, ip, np_, n, s, ns, tf, prev, cin, delta, cov, rot, cout)
    assert rows() == -5 and rows(cin=a8, rot=a4, cout=b8) == -5 and rows(n=0) == -5 and rows(s=None, ns=0) == -5
    assert rows(n=vislam.IMU_MAX_FRAMES + 1) == -5                   # the capacity refusal comes after the context's
    for k in ("ip", "np_", "tf", "prev", "delta", "cov", "s"):
        assert rows(**{k: None}) == -1, k
    for k in ("s", "tf", "cin", "delta", "cov", "cout"):
        assert rows(**{k: odd8}) == -1, k
    assert rows(prev=odd4) == -1 and rows(rot=odd4) == -1 and rows(n=-1) == -1 and rows(ns=-1) == -1 and rows(cin=a8, cout=a8) == -1
    plan = lambda ip=ok, np_=nz, n=1, s=a8, ns=4, tf=a8, delta=a8, cov=a8, rot=None: L.vis_batch_imu_cov(None, ip, np_, n, s, ns, tf, delta, cov, rot)
    assert plan() == -5 and plan(rot=a4) == -5 and plan(s=None, ns=0) == -5 and plan(n=vislam.IMU_MAX_FRAMES + 1) == -5
    for k in ("ip", "np_", "tf", "delta", "cov", "s"):
        assert plan(**{k: None}) == -1, k
    for k in ("s", "tf", "delta", "cov"):
        assert plan(**{k: odd8}) == -1, k
    assert plan(rot=odd4) == -1 and plan(n=-1) == -1 and plan(ns=-1) == -1
    d, q = vislam.ImuDelta(), vislam.ImuCov()
    one = lambda ip=ok, np_=nz, s=a8, ns=4, delta=C.byref(d), cov=C.byref(q): L.vis_imu_preintegrate_cov(None, ip, np_, s, ns, 0.0, 1.0, delta, cov, None)
    assert one() == -5 and one(s=None, ns=0) == -5
    assert one(ip=None) == -1 and one(np_=None) == -1 and one(delta=None) == -1 and one(cov=None) == -1 and one(ns=-1) == -1 and one(s=None) == -1
    assert L.vis_batch_imu_cov_init(None, None) == -5 and L.vis_batch_imu_cov_init(None, C.byref(vislam.ImuCovCarry())) == -5
    # ---- the densities: both finite and >= 0 (zero is a valid density)
    nan, inf = float("nan"), float("inf")
    for f in N_FIELDS:
        for v in (nan, inf, -inf, -1e-300):
            z = vislam.default_imu_noise()
            setattr(z, f, v)
            assert rows(np_=C.byref(z)) == -1 and plan(np_=C.byref(z)) == -1 and one(np_=C.byref(z)) == -1, (f, v)
        z = vislam.default_imu_noise()
        setattr(z, f, 0.0)
        assert rows(np_=C.byref(z)) == -5 and plan(np_=C.byref(z)) == -5 and one(np_=C.byref(z)) == -5, f
    # ---- the factor, both forms: vp, fp, the pointers, their alignment, n; then the context; then the capacity
    vap, fp0 = C.byref(vislam.default_vi_align_params()), C.byref(vislam.default_imu_factor_params())
    assert (vislam.default_imu_factor_params().var_rot, vislam.default_imu_factor_params().var_v, vislam.default_imu_factor_params().var_p) == (0.0, 0.0, 0.0)
    L.vis_default_imu_factor_params(None)
    frow = lambda vp_=vap, fp=fp0, n=1, prev=a4, traj=a8, delta=a8, cov=a8, state=a8, res=a8, out=b8: \
        L.vis_imu_factor_rows(None, vp_, fp, n, prev, traj, delta, cov, state, res, out)
    fplan = lambda vp_=vap, fp=fp0, n=1, traj=a8, delta=a8, cov=a8, state=a8, res=a8, out=b8: L.vis_batch_imu_factor(None, vp_, fp, n, traj, delta, cov, state, res, out)
    for f, ptrs in ((frow, ("prev", "traj", "delta", "cov", "state", "res", "out")), (fplan, ("traj", "delta", "cov", "state", "res", "out"))):
        assert f() == -5 and f(n=0) == -5 and f(n=1025) == -5                 # (the capacity refusal comes after the context's)
        assert f(vp_=None) == -1 and f(fp=None) == -1 and f(n=-1) == -1
        for k in ptrs:
            assert f(**{k: None}) == -1, k
            assert f(**{k: odd4 if k == "prev" else odd8}) == -1, k
        for name in P_FIELDS:
            for v in (nan, inf, -1e-300):
                z = vislam.default_imu_factor_params()
                setattr(z, name, v)
                assert f(fp=C.byref(z)) == -1, (name, v)
        bad = vislam.default_vi_align_params()
        bad.G = 0.0
        assert f(vp_=C.byref(bad)) == -1
    # ---- the parameters are checked as in the siblings
    for f, v in (("max_gap_s", 0.0), ("max_angle", nan)):
        p = vislam.default_imu_params()
        setattr(p, f, v)
        assert rows(ip=C.byref(p)) == -1 and plan(ip=C.byref(p)) == -1 and one(ip=C.byref(p)) == -1, (f, v)
