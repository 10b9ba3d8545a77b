#!/usr/bin/env python3
"""tools/pose_conditioning.py [--zero-theta] -- how rounding-robust is each degenerate pose case?  CPU only.

Builds the CPU oracle a second time into a temporary directory, from the same sources and with the flags of oracle/Makefile except
`-ffp-contract=fast -mfma` in place of `-ffp-contract=off`: the same algorithm, rounded differently (the host must have FMA).  Runs
every case of tests/pose_degenerate_cases.py through both builds and writes tests/golden/pose_degenerate_spread.json: per case,
whether inlier mask, inlier count and iterations agree, and the sign-normalised largest difference of E.  A case whose integer
outcomes differ is marked dropped (the GPU tests skip it from their list; at most 5 % may be; one of 208 is); a case whose spread is at
most 1e-11 is E-stable and gets its E compared entry by entry.  Nothing of the second build is kept.

--zero-theta: instead, search the grid {-2, -1.75, ..., 2}^4 exhaustively for the correspondences whose DLT decomposition meets
theta == 0 in a rotation with column 3 under R = I and R = diag(-1, -1, 1), t = +-e_z, and compare with the list the cases module
keeps (a minute on 8 cores)."""
import ctypes as C
import itertools
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vi-slam_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import pose_degenerate_cases as pdc  # noqa: E402


def _zt_work(args):
    from test_independent_numpy import _jacobi
    ri, tz, q = args
    return q if _jacobi(pdc.dlt_ata(pdc.R_CANDS[ri], (0.0, 0.0, tz), *[v / 4.0 for v in q]))[2] else None


def zero_theta_search():
    from multiprocessing import Pool
    ok = True
    with Pool(min(16, os.cpu_count() or 1)) as pool:
        for ri, name in enumerate(("I", "R2")):
            for tz in (1.0, -1.0):
                found = sorted(r for r in pool.imap(_zt_work, ((ri, tz, q) for q in itertools.product(range(-8, 9), repeat=4)), chunksize=512) if r)
                same = found == pdc.ZERO_THETA_Q[name]
                ok &= same
                print(f"R = {name}, t = {tz:+g} e_z: {len(found)} zero-theta correspondences, {'the list of the cases module' if same else 'NOT the list of the cases module'}")
    return 0 if ok else 1


def build_contracted(tmp):
    mk = open(os.path.join(ROOT, "oracle", "Makefile")).read()
    flags = re.search(r"^CXXFLAGS \?= (.*)$", mk, re.M).group(1).split()
    src = re.search(r"^SRC = (.*)$", mk, re.M).group(1).split()
    assert "-ffp-contract=off" in flags
    flags = [f for f in flags if f != "-ffp-contract=off"] + ["-ffp-contract=fast", "-mfma"]
    if "fma" not in open("/proc/cpuinfo").read():
        sys.exit("pose_conditioning: this host has no FMA; the contracted build cannot run here")
    out = os.path.join(tmp, "libvis_oracle_fma.so")
    subprocess.run([os.environ.get("CXX", "g++")] + flags + ["-shared", "-o", out] + src, check=True, cwd=os.path.join(ROOT, "oracle"))
    return out


def main():
    import oracle_bind as orc
    subprocess.run(["make", "-C", os.path.join(ROOT, "oracle")], check=True, stdout=subprocess.DEVNULL)
    with tempfile.TemporaryDirectory() as tmp:
        alt = C.CDLL(build_contracted(tmp))
        alt.orc_essential_ransac.argtypes = orc.lib.orc_essential_ransac.argtypes

        def run(lib, p, x1, x2):
            E = np.zeros(9); mask = np.zeros(len(x1), np.uint8); ni, it = C.c_int(0), C.c_int(0)
            assert lib.orc_essential_ransac(C.byref(p), x1.ctypes.data_as(C.c_void_p), x2.ctypes.data_as(C.c_void_p), len(x1),
                                            E.ctypes.data_as(C.c_void_p), mask.ctypes.data_as(C.c_void_p), C.byref(ni), C.byref(it)) == 0
            return E.reshape(3, 3), mask, ni.value, it.value

        import vislam
        cases = {}
        for cls, m, noise, mode in pdc.all_cases():
            p = pdc.set_mode(vislam.default_params(), mode)
            x1, x2 = pdc.make_case(cls, m, noise)
            E0, m0, n0, i0 = run(orc.lib, p, x1, x2)
            E1, m1, n1, i1 = run(alt, p, x1, x2)
            agree = bool((n0, i0) == (n1, i1) and (m0 == m1).all())
            cases[pdc.case_key(cls, m, noise, mode)] = dict(agree=agree, dropped=not agree, spread=pdc.cmp_E(E0, E1) if agree else None,
                                                            n_inliers=n0, iters_run=i0)
    kept = [v for v in cases.values() if not v["dropped"]]
    stable = sum(v["spread"] <= pdc.E_STABLE_SPREAD for v in kept)
    rec = dict(about="tools/pose_conditioning.py: the committed CPU oracle against the same sources built with -ffp-contract=fast -mfma",
               n_cases=len(cases), n_dropped=len(cases) - len(kept), n_e_stable=stable, cases=cases)
    with open(pdc.SPREAD_JSON, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"pose_conditioning: {len(cases)} cases, {len(cases) - len(kept)} dropped, {stable} E-stable (spread <= {pdc.E_STABLE_SPREAD:g}), "
          f"{len(kept) - stable} not -> {os.path.relpath(pdc.SPREAD_JSON, ROOT)}")
    return 0


if __name__ == "__main__":
    sys.exit(zero_theta_search() if "--zero-theta" in sys.argv[1:] else main())
