"""CPU: the flat work index of k_resize (csrc/resize_index.h).

  - host/resize_index_check.cpp sweeps the multiply-high decode against / and % for every bx_count 3 ... 1024 and every index a launch
    on a 4095-row level can hold (430 million decodes, about two seconds), under the sanitizers where g++ has their static runtimes;
  - the shapes of tests/test_resize_overhead_gpu.py reach what they were chosen for, by the oracle's level geometry alone."""
import os
import subprocess

import resize_overhead_cases as roc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_decode_is_exact_for_every_legal_level(built):
    exe = os.path.join(ROOT, "vi-slam_amd", "lib", "resize_index_check")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout[-500:], flush=True)
    assert r.returncode == 0 and "resize_index_check passed" in r.stdout and "FAIL" not in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    assert "runtime error" not in r.stdout + r.stderr, r.stderr[-2000:]


def test_shapes_reach_what_they_were_chosen_for(vislam, orc):
    groups, rests, scales, batches = set(), set(), set(), set()
    straddle = sparse_last = two_groups = False
    for c in roc.CASES:
        assert c.w * c.h <= 320 * 240 and c.stride > c.w and c.stride % 4 == 0, c.id
        ws, hs, _, _ = orc.level_geometry(c.params(vislam), c.w, c.h)
        narrow = roc.narrow_levels(ws, hs)
        assert narrow, c.id
        for l, bxc, dh in narrow:
            groups.add(bxc); rests.add(dh % roc.RS_ROWS); scales.add(c.scale); batches.add(c.frames)
            nrg = (dh + roc.RS_ROWS - 1) // roc.RS_ROWS
            straddle |= 64 % bxc != 0 and nrg > 1                         # 64 consecutive indices cross a row group's end
            sparse_last |= 0 < (bxc * nrg) % 256 <= 32                     # the last workgroup: at most half a wave of threads
            two_groups |= nrg == 2                                         # the fewest row groups a level of >= 8 rows has
    assert {12, 13, 63, 64, 65, 188} <= groups, sorted(groups)
    assert {0, 1, 4} <= rests and scales == {1.2, 2.0} and batches == {1, 8, 9}, (rests, scales, batches)
    assert straddle and sparse_last and two_groups
