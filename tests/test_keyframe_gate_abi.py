"""CPU: the keyframe gate's place in the C ABI -- vis_params.keyframe_min_points at offset 136 (sizeof 144), the same in the C
compiler's layout and in the ctypes binding; off by default; vis_batch_get_keyframes exported."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SNIPPET = r"""
#include <stddef.h>
#include <stdio.h>
#include "vislam_hip.h"
int main(void) {
    printf("%d %d %d %d %d %d\n", (int)offsetof(vis_params, keyframe_min_points), (int)sizeof(vis_params), VIS_ABI_VERSION,
           VIS_KF_CARRIED, VIS_KF_NOT_SAVED, VIS_KF_FIRST);
    return 0;
}
"""


def test_layout_in_c_and_ctypes(vislam, tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(SNIPPET)
    exe = str(tmp_path / "layout")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    off, size, abi, carried, not_saved, first = map(int, subprocess.run([exe], capture_output=True, text=True, timeout=30).stdout.split())
    assert (off, size, abi) == (136, 144, 5)
    assert vislam.Params.keyframe_min_points.offset == off and C.sizeof(vislam.Params) == size
    assert (carried, not_saved, first) == (vislam.KF_CARRIED, vislam.KF_NOT_SAVED, vislam.KF_FIRST) == (-1, -2, -3)


def test_default_is_off_and_getter_exported(vislam):
    assert vislam.default_params().keyframe_min_points == 0
    assert hasattr(vislam.lib, "vis_batch_get_keyframes") and "vis_batch_get_keyframes" in vislam.ABI_SYMBOLS


def test_getter_without_a_plan_is_a_state_error(vislam):
    assert vislam.lib.vis_batch_get_keyframes(None, None, 0, None) == -5          # VIS_E_STATE, no context
