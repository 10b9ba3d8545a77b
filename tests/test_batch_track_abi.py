"""CPU: batched camera tracking's place in the C ABI -- vis_track_result (32 bytes: the pose, then `composed` at offset 28), the same in
the C compiler's layout and in the ctypes binding; VIS_TRACK_NONE; the two entry points exported and listed; the state errors that need
no device; VIS_ABI_VERSION unchanged (only new symbols and structs)."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SNIPPET = r"""
#include <stddef.h>
#include <stdio.h>
#include "vislam_hip.h"
int main(void) {
    printf("%d %d %d %d %d\n", (int)sizeof(vis_track_result), (int)offsetof(vis_track_result, pose),
           (int)offsetof(vis_track_result, composed), VIS_TRACK_NONE, VIS_ABI_VERSION);
    return 0;
}
"""


def test_layout_in_c_and_ctypes(vislam, tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(SNIPPET)
    exe = str(tmp_path / "layout")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    size, off_pose, off_composed, none, abi = map(int, subprocess.run([exe], capture_output=True, text=True, timeout=30).stdout.split())
    assert (size, off_pose, off_composed) == (32, 0, 28)
    assert C.sizeof(vislam.TrackResult) == size
    assert vislam.TrackResult.pose.offset == off_pose and vislam.TrackResult.composed.offset == off_composed
    assert none == vislam.TRACK_NONE == -4
    assert abi == 5


def test_symbols_exported_and_listed(vislam):
    for s in ("vis_batch_track_init", "vis_batch_track"):
        assert hasattr(vislam.lib, s) and s in vislam.ABI_SYMBOLS, s


def test_state_errors_without_a_context_or_plan(vislam):
    ap = vislam.default_align_params()
    assert vislam.lib.vis_batch_track(None, C.byref(ap), None, 1, None, None, None) == -5        # VIS_E_STATE: no context
    assert vislam.lib.vis_batch_track_init(None, None) == -5
    assert vislam.lib.vis_batch_track(None, C.byref(ap), C.c_void_p(64), 1, None, C.c_void_p(64), C.c_void_p(64)) == -5
