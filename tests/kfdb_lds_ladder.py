"""The loop scorer's dynamic LDS between 48 KB and 128 KB, in a process of its own (not a test module: tests/test_kfdb_limits_gpu.py starts it once).
k_loop_score keeps 4 * (kp_cap + query capacity) bytes of winner tables in dynamic LDS beside 10,256 bytes of static LDS, and the library raises
hipFuncAttributeMaxDynamicSharedMemorySize once the tables pass 48 KB.  The attribute is process-wide, so whether a launch at a middle size is
accepted can only be seen in a process that has not raised it: this one creates a database per step IN RISING ORDER, adds 2 entries of about 100
keypoints, runs a 2-row query and a match and compares with the restatement byte for byte (the LDS size depends on the capacities, not on the
counts, so the couples stay tiny).  One line per step; the first difference or library error ends the process with a non-zero status and nothing
further is started on the GPU."""
import os
import sys

# (kp_cap, row_cap): kp_cap + row_cap = 12288 (48 KB exactly: the last size below the attribute), 12289 (the first above), 13568 (53 KB: static +
# dynamic just under 64 KB), 13952 (just over 64 KB), 16384, 24576 (96 KB), 32768 (128 KB, the contract's limit)
LADDER = ((6144, 6144), (6145, 6144), (6784, 6784), (6976, 6976), (8192, 8192), (12288, 12288), (16384, 16384))
STATIC_LDS = 10256


def main():
    here = os.path.dirname(os.path.abspath(__file__))
    for p in (here, os.path.join(os.path.dirname(here), "vi-slam_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import numpy as np
    import torch                                                    # noqa: F401  (test_kfdb_gpu's helpers put the rows on the device with it)
    import vislam
    import kfdb_cases as kc
    import kfdb_ref as kr
    from test_kfdb_gpu import Pair, params

    E, Q, _ = kc.planted_sets(77, 300, 300)
    c = vislam.Context(0)
    for kp_cap, row_cap in LADDER:
        dyn = 4 * (kp_cap + min(row_cap, kp_cap))
        what = f"lds ladder: {kp_cap} + {row_cap} keypoints, dynamic {dyn} + static {STATIC_LDS} = {dyn + STATIC_LDS} bytes, limit {'raised' if dyn > 48 * 1024 else 'as it was'}:"
        try:
            rng = np.random.default_rng(kp_cap)
            pr = Pair(vislam, c, 2, kp_cap)
            kps, desc, nkp = kc.rows(rng, [E[:100], E[100:197]], row_cap)
            pr.add(kps, desc, nkp, [0, 1])
            qk, qd, qn = kc.rows(rng, [Q[:300], Q[:120]], row_cap)
            lp, lq = params(vislam, min_gap=0, min_score=0, topk=2)
            scores, cand, _ = pr.query(lp, lq, qd, qn, [5, 6])
            cd = np.zeros((2, 2), kr.CAND_DTYPE)
            cd[:] = cand
            want = pr.match(lp, lq, qk, qd, qn, cd, 2, 0, 128)
            assert scores.min() >= 10 and (want[3] >= 10).all(), scores               # not a comparison of empty lists
            pr.close()
        except BaseException as e:                                   # a library error or a difference: say which step, start nothing further
            print(what, "FAILED", type(e).__name__, str(e)[:1500], flush=True)
            sys.exit(1)
        print(what, "scores", scores.reshape(-1).tolist(), "ok", flush=True)
    c.close()


if __name__ == "__main__":
    main()
