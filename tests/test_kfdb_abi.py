"""CPU: the loop-candidate entry points' place in the C ABI -- vis_loop_params (24 bytes), vis_loop_cand (16) and vis_loop_query (32) in the C
compiler's layout and in the ctypes / numpy bindings and the restatement, the enums and defaults, every symbol exported and bound, every refusal
that needs no device in the header's order, both ends of every parameter's range accepted and one step past each refused; VIS_ABI_VERSION and
vis_params unchanged."""
import ctypes as C
import os
import subprocess

import kfdb_ref as kr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("vis_default_loop_params", "vis_kfdb_create", "vis_kfdb_destroy", "vis_kfdb_reset", "vis_kfdb_info", "vis_kfdb_get_entry", "vis_kfdb_add_rows",
           "vis_batch_kfdb_add", "vis_kfdb_query_rows", "vis_batch_kfdb_query", "vis_kfdb_match_rows", "vis_batch_kfdb_match")
C_FIELDS = ("id", "slot", "score", "n_keypoints")
Q_FIELDS = ("id", "n_keypoints", "n_scored", "n_cand", "best_score", "flags", "reserved_")

SNIPPET = r"""
#include <stddef.h>
#include <stdio.h>
#include "vislam_hip.h"
#define L(f) (int)offsetof(vis_loop_params, f)
#define K(f) (int)offsetof(vis_loop_cand, f)
#define Q(f) (int)offsetof(vis_loop_query, f)
#define I(f) (int)offsetof(vis_kfdb_info_t, f)
int main(void) {
    printf("%d %d %d %d %d %d %d\n", (int)sizeof(vis_loop_params), L(ratio), L(sym_mode), L(min_gap), L(topk), L(min_score), L(reserved_));
    printf("%d %d %d %d %d\n", (int)sizeof(vis_loop_cand), K(id), K(slot), K(score), K(n_keypoints));
    printf("%d %d %d %d %d %d %d %d\n", (int)sizeof(vis_loop_query), Q(id), Q(n_keypoints), Q(n_scored), Q(n_cand), Q(best_score), Q(flags), Q(reserved_));
    printf("%d %d %d %d %d %d\n", (int)sizeof(vis_kfdb_info_t), I(entry_cap), I(kp_cap), I(head), I(reserved_), I(total_added));
    printf("%d %d %d %d %d\n", VIS_ABI_VERSION, (int)sizeof(vis_params), (int)VIS_LOOP_SKIPPED, (int)VIS_SYM_REFERENCE_EFFECTIVE, (int)VIS_SYM_INTENDED);
    return 0;
}
"""


def test_layout_in_c_ctypes_numpy_and_the_restatement(vislam, tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(SNIPPET)
    exe = str(tmp_path / "layout")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    rows = [list(map(int, l.split())) for l in subprocess.run([exe], capture_output=True, text=True, timeout=30).stdout.splitlines()]
    assert rows[0] == [24, 0, 4, 8, 12, 16, 20]
    assert rows[1] == [16, 0, 4, 8, 12]
    assert rows[2] == [32, 0, 4, 8, 12, 16, 20, 24]
    assert rows[3] == [24, 0, 4, 8, 12, 16]
    S = vislam.LoopParams
    assert [C.sizeof(S)] + [getattr(S, f).offset for f in kr.PARAM_FIELDS] == rows[0]
    I = vislam.KfDbInfo
    assert [C.sizeof(I)] + [getattr(I, f).offset for f in ("entry_cap", "kp_cap", "head", "reserved_", "total_added")] == rows[3]
    for fields, row, dts in ((C_FIELDS, rows[1], (vislam.LOOP_CAND_DTYPE, kr.CAND_DTYPE)), (Q_FIELDS, rows[2], (vislam.LOOP_QUERY_DTYPE, kr.QUERY_DTYPE))):
        for d in dts:
            assert d.names == fields and [d.itemsize] + [d.fields[k][1] for k in fields] == row, d
    assert rows[4][0] == 5                                         # VIS_ABI_VERSION: only new symbols and new structs
    assert rows[4][1] == 144 == C.sizeof(vislam.Params)            # vis_params did not grow
    assert rows[4][2] == vislam.LOOP_SKIPPED == kr.LOOP_SKIPPED == 1
    assert rows[4][3:] == [vislam.SYM_REFERENCE_EFFECTIVE, vislam.SYM_INTENDED] == [kr.SYM_REFERENCE_EFFECTIVE, kr.SYM_INTENDED] == [0, 1]


def test_defaults(vislam):
    lp, want = vislam.default_loop_params(), kr.Params()
    assert [getattr(lp, f) for f in kr.PARAM_FIELDS] == [C.c_float(0.8).value, vislam.SYM_INTENDED, 30, 4, 30, 0]
    assert [getattr(lp, f) for f in kr.PARAM_FIELDS] == [getattr(want, f) for f in kr.PARAM_FIELDS]
    vislam.lib.vis_default_loop_params(None)                       # a NULL pointer is ignored
    assert (kr.MAX_ENTRY_CAP, kr.MAX_KP_CAP, kr.MAX_TOPK) == (65536, 16384, 16)


def test_symbols_exported_and_listed(vislam):
    for s in SYMBOLS:
        assert hasattr(vislam.lib, s) and s in vislam.ABI_SYMBOLS, s
    for name in ("close", "reset", "info", "get_entry", "add_rows", "batch_add", "query_rows", "batch_query", "match_rows", "batch_match"):
        assert callable(getattr(vislam.KfDb, name)), name
    assert callable(vislam.Context.kfdb)
    out = subprocess.run(["nm", "-D", "--defined-only", vislam.LIB_PATH], capture_output=True, text=True, timeout=60).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    assert set(SYMBOLS) <= exported


def test_errors_that_need_no_device(vislam):
    L = vislam.lib
    a8, a4, odd8, odd4 = (C.c_void_p(v) for v in (64, 68, 68, 66))   # never dereferenced: the argument / database checks come first
    lp = vislam.default_loop_params()
    ok = C.byref(lp)
    INVALID, STATE = -1, -5
    # lifetime and bookkeeping
    out = C.c_void_p()
    assert L.vis_kfdb_create(None, 4, 4, None) == INVALID
    for ecap, kcap in ((0, 4), (65537, 4), (4, 0), (4, 16385), (-1, 4), (4, -1)):
        assert L.vis_kfdb_create(None, ecap, kcap, C.byref(out)) == INVALID, (ecap, kcap)
    for ecap, kcap in ((1, 1), (65536, 16384), (1, 16384), (65536, 1)):
        assert L.vis_kfdb_create(None, ecap, kcap, C.byref(out)) == STATE and not out.value, (ecap, kcap)   # in range: no context comes next
    L.vis_kfdb_destroy(None)                                          # ignored
    assert L.vis_kfdb_reset(None) == STATE
    info = vislam.KfDbInfo()
    assert L.vis_kfdb_info(None, None) == INVALID and L.vis_kfdb_info(None, C.byref(info)) == STATE
    i32 = C.c_int32(0)
    assert L.vis_kfdb_get_entry(None, 0, None, C.byref(i32), a4, 1) == INVALID and L.vis_kfdb_get_entry(None, 0, C.byref(i32), None, a4, 1) == INVALID
    assert L.vis_kfdb_get_entry(None, 0, C.byref(i32), C.byref(i32), None, 1) == INVALID and L.vis_kfdb_get_entry(None, 0, C.byref(i32), C.byref(i32), a4, -1) == INVALID
    assert L.vis_kfdb_get_entry(None, 0, C.byref(i32), C.byref(i32), odd4, 1) == INVALID
    assert L.vis_kfdb_get_entry(None, 0, C.byref(i32), C.byref(i32), None, 0) == STATE and L.vis_kfdb_get_entry(None, 0, C.byref(i32), C.byref(i32), a4, 1) == STATE
    # the rows forms: VIS_E_STATE (no database) after every VIS_E_INVALID
    add = lambda n=2, kps=a4, desc=a4, nkp=a4, cap=8, ids=a4: L.vis_kfdb_add_rows(None, n, kps, desc, nkp, cap, ids)
    query = lambda lp_=ok, n=2, desc=a4, nkp=a4, cap=8, ids=a4, sc=a4, cand=a4, q=a4: L.vis_kfdb_query_rows(None, lp_, n, desc, nkp, cap, ids, sc, cand, q)
    match = lambda lp_=ok, n=2, kps=a4, desc=a4, nkp=a4, cap=8, cand=a4, stride=4, mp=8, m=a4, p1=a8, p2=a8, npts=a4: \
        L.vis_kfdb_match_rows(None, lp_, n, kps, desc, nkp, cap, cand, stride, mp, m, p1, p2, npts)
    badd = lambda n=2, step=1: L.vis_batch_kfdb_add(None, n, step)
    bquery = lambda lp_=ok, n=2, step=1, sc=a4, cand=a4, q=a4: L.vis_batch_kfdb_query(None, lp_, n, step, sc, cand, q)
    bmatch = lambda lp_=ok, n=2, cand=a4, stride=4, mp=8, m=a4, p1=a8, p2=a8, npts=a4: L.vis_batch_kfdb_match(None, lp_, n, cand, stride, mp, m, p1, p2, npts)
    for f in (add, query, match, badd, bquery, bmatch):
        assert f() == STATE and f(n=0) == STATE and f(n=-1) == INVALID, f
    assert query(sc=None) == STATE and bquery(sc=None) == STATE and match(m=None) == STATE and bmatch(m=None) == STATE      # the optional outputs
    assert query(n=1 << 30) == STATE and bquery(n=1 << 30) == STATE                                                         # VIS_E_CAPACITY comes after the database
    for k in ("kps", "desc", "nkp", "ids"):
        assert add(**{k: None}) == INVALID and add(**{k: odd4}) == INVALID, k
    for k in ("lp_", "desc", "nkp", "ids", "cand", "q"):
        assert query(**{k: None}) == INVALID, k
    for k in ("desc", "nkp", "ids", "sc", "cand", "q"):
        assert query(**{k: odd4}) == INVALID, k
    for k in ("lp_", "kps", "desc", "nkp", "cand", "p1", "p2", "npts"):
        assert match(**{k: None}) == INVALID, k
    for k in ("kps", "desc", "nkp", "cand", "m", "npts"):
        assert match(**{k: odd4}) == INVALID, k
    assert match(p1=odd8) == INVALID and match(p2=odd8) == INVALID and bmatch(p1=odd8) == INVALID and bmatch(p2=odd8) == INVALID
    assert add(cap=-1) == INVALID and query(cap=-1) == INVALID and match(cap=-1) == INVALID and match(stride=-1) == INVALID and match(mp=-1) == INVALID
    assert add(cap=0) == STATE and match(stride=0) == STATE and match(mp=0) == STATE and bmatch(stride=0) == STATE and bmatch(mp=0) == STATE
    assert badd(step=0) == INVALID and badd(step=-3) == INVALID and bquery(step=0) == INVALID and badd(step=2 ** 31 - 1) == STATE
    for k in ("lp_", "cand", "q"):
        assert bquery(**{k: None}) == INVALID, k
    for k in ("sc", "cand", "q"):
        assert bquery(**{k: odd4}) == INVALID, k
    for k in ("lp_", "cand", "p1", "p2", "npts"):
        assert bmatch(**{k: None}) == INVALID, k
    for k in ("cand", "m", "npts"):
        assert bmatch(**{k: odd4}) == INVALID, k
    assert bmatch(stride=-1) == INVALID and bmatch(mp=-1) == INVALID
    # the parameter ranges: one step past each end refused, both ends accepted; ratio and min_score are taken as written
    bad = [("topk", 0), ("topk", 17), ("min_gap", -1), ("sym_mode", -1), ("sym_mode", 2)]
    for f, v in bad:
        q = vislam.default_loop_params()
        setattr(q, f, v)
        for call in (query, match, bquery, bmatch):
            assert call(lp_=C.byref(q)) == INVALID, (f, v)
    good = [("topk", 1), ("topk", 16), ("min_gap", 0), ("min_gap", 2 ** 31 - 1), ("sym_mode", 0), ("sym_mode", 1), ("ratio", float("nan")),
            ("ratio", float("inf")), ("ratio", -0.5), ("ratio", 0.0), ("min_score", -2 ** 31), ("min_score", 2 ** 31 - 1)]
    for f, v in good:
        q = vislam.default_loop_params()
        setattr(q, f, v)
        for call in (query, match, bquery, bmatch):
            assert call(lp_=C.byref(q)) == STATE, (f, v)
