"""CPU: the guided matcher's place in the C ABI -- the five new symbols exported, declared in the header (a C99 translation unit takes
their addresses) and listed in the binding; VIS_ABI_VERSION and vis_params unchanged; every refusal that needs no device."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("vis_warp_keypoints", "vis_bf_knn2_hamming_guided", "vis_bf_knn2_hamming_guided_host", "vis_good_matches_guided",
           "vis_batch_run_guided")
STAGE_ALL, STAGE_DETECT, STAGE_POSE = 7, 1, 4

SNIPPET = r"""
#include "vislam_hip.h"
typedef int (*warp_t)(vis_ctx*, const vis_keypoint*, int, const float[9], float*);
typedef int (*knn_t)(vis_ctx*, int, int, const float[9], float, vis_dmatch*, vis_dmatch*);
typedef int (*host_t)(vis_ctx*, const uint8_t*, const vis_keypoint*, int, const uint8_t*, const vis_keypoint*, int, const float[9], float,
                      vis_dmatch*, vis_dmatch*);
typedef int (*good_t)(vis_ctx*, int, int, const float[9], float, vis_dmatch*, int, int*, vis_dmatch*, int, int*);
typedef int (*run_t)(vis_ctx*, const uint8_t*, int, int, const float*, float);
/* the declared types are these, or the initialisers do not compile under -Werror */
warp_t p_warp = vis_warp_keypoints; knn_t p_knn = vis_bf_knn2_hamming_guided; host_t p_host = vis_bf_knn2_hamming_guided_host;
good_t p_good = vis_good_matches_guided; run_t p_run = vis_batch_run_guided;
typedef char abi_version_is_5[(VIS_ABI_VERSION == 5) ? 1 : -1];
typedef char params_are_144_bytes[(sizeof(vis_params) == 144) ? 1 : -1];
"""


def test_header_declares_them_and_the_abi_did_not_move(vislam, tmp_path):
    src = tmp_path / "decl.c"
    src.write_text(SNIPPET)
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                        str(tmp_path / "decl.o")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert C.sizeof(vislam.Params) == 144


def test_symbols_exported_and_listed(vislam):
    for s in SYMBOLS:
        assert hasattr(vislam.lib, s) and s in vislam.ABI_SYMBOLS, s
    for name in ("warp_keypoints", "bf_knn2_hamming_guided", "bf_knn2_hamming_guided_host", "good_matches_guided", "batch_run_guided"):
        assert callable(getattr(vislam.Context, name)), name


def test_errors_that_need_no_device(vislam):
    L = vislam.lib
    some = C.c_void_p(64)                                          # never dereferenced: the argument / context checks come first
    rot = np.eye(3, dtype=np.float32).reshape(9)
    R = rot.ctypes.data_as(C.c_void_p)
    nan, inf = float("nan"), float("inf")
    bad_rots = []
    for v in (nan, inf, -inf):
        b = rot.copy(); b[4] = v
        bad_rots.append(b)
    ng, ns = C.c_int(7), C.c_int(7)
    calls = {
        "warp": lambda rot_p=R, n=1, kps=some, out=some: L.vis_warp_keypoints(None, kps, n, rot_p, out),
        "knn": lambda rot_p=R, radius=8.0: L.vis_bf_knn2_hamming_guided(None, 0, 1, rot_p, radius, some, some),
        "host": lambda rot_p=R, radius=8.0, dq=some, kq=some, nq=1, dt=some, kt=some, nt=1:
            L.vis_bf_knn2_hamming_guided_host(None, dq, kq, nq, dt, kt, nt, rot_p, radius, some, some),
        "good": lambda rot_p=R, radius=8.0: L.vis_good_matches_guided(None, 0, 1, rot_p, radius, some, 49, C.byref(ng), some, 49, C.byref(ns)),
        "run": lambda rot_p=some, radius=8.0, frames=some, stages=STAGE_ALL: L.vis_batch_run_guided(None, frames, 1, stages, rot_p, radius),
    }
    # arguments in order, no context -> VIS_E_STATE
    for name, f in calls.items():
        assert f() == -5, name
    assert calls["knn"](radius=0.0) == -5 and calls["run"](radius=0.0) == -5          # a window of zero pixels is a window
    # NULL rotation -> VIS_E_INVALID
    for name, f in calls.items():
        assert f(rot_p=None) == -1, name
    # a radius that is negative or not finite -> VIS_E_INVALID
    for name in ("knn", "host", "good", "run"):
        for bad in (-1.0, -1e-30, nan, inf, -inf):
            assert calls[name](radius=bad) == -1, (name, bad)
    # a non-finite entry of a host rotation -> VIS_E_INVALID
    for name in ("warp", "knn", "host", "good"):
        for b in bad_rots:
            assert calls[name](rot_p=b.ctypes.data_as(C.c_void_p)) == -1, name
    # what the unguided twins refuse
    assert calls["warp"](n=-1) == -1 and calls["warp"](kps=None) == -1 and calls["warp"](out=None) == -1
    assert calls["warp"](n=0, kps=None, out=None) == -5            # nothing to read or write: the arguments are in order
    assert calls["host"](dq=None) == -1 and calls["host"](kq=None) == -1 and calls["host"](dt=None) == -1 and calls["host"](kt=None) == -1
    assert calls["host"](nq=-1) == -1 and calls["host"](nt=65536) == -1
    assert calls["run"](frames=None) == -1
    # the match stage is what is guided: stages without it -> VIS_E_INVALID
    assert calls["run"](stages=STAGE_DETECT) == -1 and calls["run"](stages=STAGE_DETECT | STAGE_POSE) == -1
    assert ng.value == 7 and ns.value == 7                         # a refused call writes nothing
