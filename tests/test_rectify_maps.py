"""CPU: the rectification tables (vis_optimal_new_camera_matrix, vis_undistort_rectify_map) against the independent numpy restatement
in tests/rectify_ref.py, byte for byte; identity tables; K' of the EuRoC calibration unchanged to the float bit; the invalid arguments;
vis_rectify_create without a device; the new declarations in a C99 -pedantic snippet.  Parity with OpenCV itself is unpinned."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import rectify_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EUROC_K = (458.654, 457.296, 367.215, 248.375)
EUROC_D = (-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05)
TUM_K, TUM_D = (517.306408, 516.469215, 318.643040, 255.313989), (0.262383, -0.953104, -0.005358, 0.002628)      # fr1 RGB, 640 x 480
KITTI_K, KITTI_D = (984.2439, 980.8141, 690.0, 233.1966), (-0.3728755, 0.2037299, 0.002219027, 0.001383707)      # 1392 x 512
# strong enough that source coordinates run far past +-1024 px (int16 wrap) and past 2^26 px (INT_MIN), and off the image
STRONG_K, STRONG_D, STRONG_KN = (400.0, 410.0, 320.0, 240.0), (0.9, 0.4, 0.01, -0.02), (2.0, 2.5, 320.0, 240.0)
STRONG_NEG_D = (-0.9, 0.05, 0.0, 0.0)


def _cases(vislam):
    kn = lambda K, D, i, o: tuple(float(v) for v in vislam.optimal_new_camera_matrix(K, D, i, o))
    return {
        "euroc": (EUROC_K, EUROC_D, kn(EUROC_K, EUROC_D, (752, 480), (736, 480)), (736, 480)),
        "tum": (TUM_K, TUM_D, kn(TUM_K, TUM_D, (640, 480), (640, 480)), (640, 480)),
        "kitti": (KITTI_K, KITTI_D, kn(KITTI_K, KITTI_D, (1392, 512), (1392, 512)), (1392, 512)),
        "odd": (EUROC_K, EUROC_D, kn(EUROC_K, EUROC_D, (333, 217), (301, 199)), (301, 199)),
        "strong": (STRONG_K, STRONG_D, STRONG_KN, (640, 480)),
        "strong_barrel": (STRONG_K, STRONG_NEG_D, STRONG_KN, (97, 61)),
    }


@pytest.mark.parametrize("name", ["euroc", "tum", "kitti", "odd", "strong", "strong_barrel"])
def test_tables_match_the_numpy_restatement(vislam, name):
    K, D, Kn, (w, h) = _cases(vislam)[name]
    m1, m2 = vislam.undistort_rectify_map(K, D, Kn, (w, h))
    r1, r2 = rectify_ref.undistort_rectify_map(K, D, Kn, w, h)
    assert m1.shape == (h, w, 2) and m2.shape == (h, w) and m1.dtype == np.int16 and m2.dtype == np.uint16
    assert m1.tobytes() == r1.tobytes() and m2.tobytes() == r2.tobytes()
    assert int(m2.max()) < 1024
    if name == "strong":
        # the branches the strong lens has to reach: sources beyond +-1024 px before the wrap, the INT_MIN of saturate_cast, off-image
        assert (np.abs(m1.astype(np.int64)) > 1024).any()
        assert ((m1[..., 0] == 0) & (m1[..., 1] == 0) & (m2 == 0)).any()       # INT_MIN >> 5 wraps to 0, INT_MIN & 31 = 0
        assert ((m1[..., 0] < -1) | (m1[..., 0] >= 640)).any()


def test_identity_tables(vislam):
    for K, (w, h) in ((EUROC_K, (752, 480)), ((300.5, 301.25, 100.0, 80.0), (211, 163))):
        m1, m2 = vislam.undistort_rectify_map(K, (0, 0, 0, 0), K, (w, h))
        u, v = np.meshgrid(np.arange(w), np.arange(h))
        assert (m1[..., 0] == u).all() and (m1[..., 1] == v).all() and (m2 == 0).all()


def test_new_camera_matrix_is_the_adapters_to_the_bit(vislam):
    Kn = vislam.optimal_new_camera_matrix(EUROC_K, EUROC_D, (752, 480), (736, 480))
    want = np.array([326.878448, 332.678375, 358.490997, 248.256042], np.float32)   # the adapter's K' before it moved into the library
    assert Kn.dtype == np.float32 and Kn.view(np.uint32).tolist() == want.view(np.uint32).tolist()


def test_invalid_arguments(vislam):
    lib, f4 = vislam.lib, lambda *v: np.array(v, np.float32)
    K, D, Kn = f4(*EUROC_K), f4(*EUROC_D), f4(326.9, 332.7, 358.5, 248.3)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    out = np.zeros(4, np.float32)
    m1 = np.zeros(2 * 4095 * 2, np.int16); m2 = np.zeros(4095 * 2, np.uint16)
    assert lib.vis_optimal_new_camera_matrix(p(K), p(D), 752, 480, 736, 480, p(out)) == 0
    assert lib.vis_undistort_rectify_map(p(K), p(D), p(Kn), 4095, 2, p(m1), p(m2)) == 0
    for args in ((None, p(D), 752, 480, 736, 480, p(out)), (p(K), None, 752, 480, 736, 480, p(out)), (p(K), p(D), 752, 480, 736, 480, None),
                 (p(K), p(D), 0, 480, 736, 480, p(out)), (p(K), p(D), 752, 4096, 736, 480, p(out)), (p(K), p(D), 752, 480, -1, 480, p(out)),
                 (p(K), p(D), 752, 480, 736, 4096, p(out))):
        assert lib.vis_optimal_new_camera_matrix(*args) == -1, args
    for args in ((None, p(D), p(Kn), 8, 8, p(m1), p(m2)), (p(K), None, p(Kn), 8, 8, p(m1), p(m2)), (p(K), p(D), None, 8, 8, p(m1), p(m2)),
                 (p(K), p(D), p(Kn), 8, 8, None, p(m2)), (p(K), p(D), p(Kn), 8, 8, p(m1), None), (p(K), p(D), p(Kn), 0, 8, p(m1), p(m2)),
                 (p(K), p(D), p(Kn), 8, 4096, p(m1), p(m2)), (p(K), p(D), p(Kn), 4096, 1, p(m1), p(m2))):
        assert lib.vis_undistort_rectify_map(*args) == -1, args
    for bad in (0.0, -1.0, np.inf, np.nan):
        for i in (0, 1):
            Kb = K.copy(); Kb[i] = bad
            assert lib.vis_optimal_new_camera_matrix(p(Kb), p(D), 752, 480, 736, 480, p(out)) == -1, (bad, i)
            assert lib.vis_undistort_rectify_map(p(Kb), p(D), p(Kn), 8, 8, p(m1), p(m2)) == -1, (bad, i)
            Knb = Kn.copy(); Knb[i] = bad
            assert lib.vis_undistort_rectify_map(p(K), p(D), p(Knb), 8, 8, p(m1), p(m2)) == -1, (bad, i)


def test_rectify_create_without_a_device(vislam):
    K, D, Kn = (np.array(v, np.float32) for v in (EUROC_K, EUROC_D, (326.9, 332.7, 358.5, 248.3)))
    r = C.c_void_p()
    rc = vislam.lib.vis_rectify_create(None, K.ctypes.data, D.ctypes.data, Kn.ctypes.data, 752, 480, 736, 480, C.byref(r))
    assert rc == (-2 if vislam.device_count() == 0 else -1) and not r.value      # VIS_E_NODEVICE (no context can exist without one)
    for fn in (vislam.lib.vis_rectify_batch,):
        assert fn(None, None, 0, 1, 0, 0, 1, 1, None, 1) == -1
    assert vislam.lib.vis_rectify_host(None, None, 0, None, 0) == -1
    assert vislam.lib.vis_rectify_maps(None, None, None) == -1
    vislam.lib.vis_rectify_destroy(None)


SNIPPET = r"""
#include <stdio.h>
#include "vislam_hip.h"
int main(void) {
    const float K[4] = {458.654f, 457.296f, 367.215f, 248.375f}, d[4] = {-0.28340811f, 0.07395907f, 0.00019359f, 1.76187114e-05f};
    float Kn[4];
    static int16_t m1[2 * 16 * 8];
    static uint16_t m2[16 * 8];
    vis_rectify* r = NULL;
    int a = vis_optimal_new_camera_matrix(K, d, 752, 480, 16, 8, Kn);
    int b = vis_undistort_rectify_map(K, d, Kn, 16, 8, m1, m2);
    int c = vis_rectify_create(NULL, K, d, Kn, 752, 480, 16, 8, &r);
    int e = vis_rectify_batch(r, NULL, 752, 1, 0, 0, 16, 8, NULL, 16);
    int f = vis_rectify_host(r, NULL, 752, NULL, 16);
    int g = vis_rectify_maps(r, m1, m2);
    vis_rectify_destroy(r);
    printf("%d %d %d %d %d %d\n", a, b, c, e, f, g);
    return 0;
}
"""


def test_header_declarations_compile_as_c99(vislam, tmp_path):
    src = tmp_path / "rect.c"
    src.write_text(SNIPPET)
    exe = str(tmp_path / "rect")
    libdir = os.path.join(ROOT, "vi-slam_amd", "lib")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe,
                        "-L", libdir, "-lvislam_hip", "-Wl,-rpath," + libdir], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    a, b, c, e, f, g = map(int, out.stdout.split())
    assert (a, b, e, f, g) == (0, 0, -1, -1, -1) and c == (-2 if vislam.device_count() == 0 else -1)
