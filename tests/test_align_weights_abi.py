"""CPU: vis_align_weights in the C ABI -- 16 bytes, the same in the C compiler's layout and in ctypes; the VIS_W_* values; the three
symbols exported and listed; the defaults; every refusal of vis_set_align_weights that needs no device; VIS_ABI_VERSION and the sizes of
vis_params, vis_align_params and vis_align_result unchanged (only symbols and one struct were added)."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SNIPPET = r"""
#include <math.h>
#include <stddef.h>
#include <stdio.h>
#include "vislam_hip.h"
int main(void) {
    vis_align_weights d, z;
    printf("%d %d %d %d %d\n", (int)sizeof(vis_align_weights), (int)offsetof(vis_align_weights, mode), (int)offsetof(vis_align_weights, tukey_b),
           (int)offsetof(vis_align_weights, mad_scale), (int)offsetof(vis_align_weights, reserved_));
    printf("%d %d %d %d\n", VIS_W_IDENTITY, VIS_W_TUKEY, VIS_W_TUKEY_SIGNED, VIS_ABI_VERSION);
    printf("%d %d %d\n", (int)sizeof(vis_params), (int)sizeof(vis_align_params), (int)sizeof(vis_align_result));
    vis_default_align_weights(&d);
    vis_default_align_weights(NULL);
    printf("%d %d %d %d\n", d.mode, d.tukey_b == 4.6851f, d.mad_scale == 1.4826f, d.reserved_);
    z = d;
    printf("%d %d %d\n", vis_set_align_weights(NULL, &d), vis_set_align_weights(NULL, NULL), vis_get_align_weights(NULL, &z));
    return 0;
}
"""


def test_layout_values_and_defaults_in_c(vislam, tmp_path):
    src = tmp_path / "weights.c"
    src.write_text(SNIPPET)
    exe = str(tmp_path / "weights")
    lib = os.path.join(ROOT, "vi-slam_amd", "lib")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe,
                        "-L", lib, "-lvislam_hip", "-Wl,-rpath," + lib], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stderr
    rows = [list(map(int, l.split())) for l in run.stdout.splitlines()]
    assert rows[0] == [16, 0, 4, 8, 12]
    A = vislam.AlignWeights
    assert [C.sizeof(A), A.mode.offset, A.tukey_b.offset, A.mad_scale.offset, A.reserved_.offset] == rows[0]
    assert rows[1] == [0, 1, 2, 5]                                 # VIS_W_*; VIS_ABI_VERSION: only new symbols and one struct
    assert (vislam.W_IDENTITY, vislam.W_TUKEY, vislam.W_TUKEY_SIGNED) == (0, 1, 2)
    assert rows[2] == [144, 36, 156]                               # vis_params, vis_align_params, vis_align_result did not change
    assert rows[2] == [C.sizeof(vislam.Params), C.sizeof(vislam.AlignParams), C.sizeof(vislam.AlignResult)]
    assert rows[3] == [0, 1, 1, 0]
    assert rows[4] == [-1, -1, -1]                                 # a NULL context: VIS_E_INVALID


def test_symbols_exported_and_listed(vislam):
    for s in ("vis_default_align_weights", "vis_set_align_weights", "vis_get_align_weights"):
        assert hasattr(vislam.lib, s) and s in vislam.ABI_SYMBOLS, s


def test_defaults(vislam):
    aw = vislam.default_align_weights()
    assert (aw.mode, aw.reserved_) == (vislam.W_IDENTITY, 0)
    assert aw.tukey_b == C.c_float(4.6851).value and aw.mad_scale == C.c_float(1.4826).value
    vislam.lib.vis_default_align_weights(None)                     # tolerated


def test_refusals_that_need_no_device(vislam):
    """the argument checks of vis_set_align_weights come before anything touches the context: with a NULL context every call is
    VIS_E_INVALID, the valid settings included (the refusals on a live context are in tests/test_align_weights_gpu.py)"""
    aw = vislam.default_align_weights()
    assert vislam.lib.vis_set_align_weights(None, C.byref(aw)) == -1
    assert vislam.lib.vis_set_align_weights(None, None) == -1
    assert vislam.lib.vis_get_align_weights(None, C.byref(aw)) == -1
    for mode, b, s, rsv in [(3, 4.6851, 1.4826, 0), (-1, 4.6851, 1.4826, 0), (1, 0.0, 1.4826, 0), (1, float("nan"), 1.4826, 0),
                            (1, float("inf"), 1.4826, 0), (1, 4.6851, -1.0, 0), (1, 4.6851, float("nan"), 0), (1, 4.6851, 1.4826, 7)]:
        aw.mode, aw.tukey_b, aw.mad_scale, aw.reserved_ = mode, b, s, rsv
        assert vislam.lib.vis_set_align_weights(None, C.byref(aw)) == -1
