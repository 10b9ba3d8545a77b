"""CPU: the visual-inertial chain END TO END on the one planted world of tests/vi_chain_cases.py, through the oracle's essential RANSAC + recoverPose
and the restatements of every stage behind it, each record handed on as the stage before wrote it -- and the end of the chain against the planted
truth.  The stages' own tests pin each paragraph of include/vislam_hip.h; this one pins that the paragraphs AGREE: (R, t) of a pose record, sigma and
the unit first edge as the gauge of s, the identity root as the frame of g and Rw, r_ic and p_ci on both sides of the IMU, dba as the step the
correction applies.

a. THE LADDER: one error per hand-over against truth (vi_chain_cases.ladder), printed for every scenario and asserted at 4 x MEASURED -- the errors
   this module measured on the unbroken chain; the margin is for another libm or rounding, nothing more.  The figures are in DESIGN.md 4.24.
b. The conditions that keep (a) from being vacuous: poses with at least 100 inliers, links VIS_SL_OK on 30 shared points and more, no flag in
   `chain`, exactly the flags and sequence numbers `lost` and `thin` are built to show, the scale of the NEW gauge there.
c. NEGATIVE CONTROLS: the chain with one convention broken raises an error of (a) to CONTROL_RATIO times the unbroken value or more (measured:
   4.8e3 times at the least).
d. `cut` against `chain`: links, depth rows, deltas and Jacobians byte for byte (their contracts say so), the trajectory within 16 x DOUBLING_BOUND,
   the carried sums of the first alignment within CUT_BOUND of the restatement over the cut's own records as one call."""
import functools

import numpy as np
import pytest

import imu_jac_ref as jr
import scale_link_ref as sl
import trajectory_ref as tj
import vi_align_ba_ref as br
import vi_align_cases as vc
import vi_align_ref as vr
import vi_chain_cases as cc
from test_trajectory_ref import DOUBLING_BOUND, differences, path_lengths
from test_vi_align_ba_ref import CUT_BOUND as CUT_BOUND_BA
from test_vi_align_ref import CUT_BOUND

# the unbroken chain's errors against truth, measured by test_the_ladder_against_truth below (it prints them); units in vi_chain_cases.ladder
MEASURED = {
    "chain": dict(pose_R=5.4e-08, pose_t=1.9e-06, link=2.5e-06, centre=7.3e-07, delta_raw_v=1.7e-04, delta_R=9.0e-08, delta_v=1.1e-04, delta_p=2.9e-06, s1=3.3e-04,
                   g1=2.9e-03, dbg1=1.8e-06, dba1=2.2e-03, s=8.3e-06, g=1.2e-05, dbg=1.8e-06, dba=8.4e-05, p=1.5e-05, v=1.4e-05),
    "gated": dict(pose_R=6.2e-08, pose_t=1.1e-06, link=1.4e-06, centre=7.0e-07, delta_raw_v=6.8e-04, delta_R=1.9e-07, delta_v=3.5e-04, delta_p=1.9e-05, s1=6.0e-04,
                   g1=6.0e-03, dbg1=1.9e-06, dba1=3.7e-03, s=7.7e-06, g=1.7e-05, dbg=1.9e-06, dba=1.8e-04, p=1.4e-05, v=9.4e-06),
    "lost": dict(pose_R=5.4e-08, pose_t=1.9e-06, link=2.5e-06, centre=1.2e-06, delta_raw_v=1.7e-04, delta_R=4.6e-08, delta_v=2.5e-04, delta_p=6.5e-06, s1=8.4e-04,
                  g1=4.7e-03, dbg1=1.8e-06, dba1=5.1e-03, s=3.1e-06, g=2.4e-05, dbg=2.1e-06, dba=1.2e-04, p=6.8e-06, v=4.4e-06),
    "thin": dict(pose_R=5.4e-08, pose_t=1.9e-06, link=3.1e-06, centre=1.5e-07, delta_raw_v=1.7e-04, delta_R=8.8e-08, delta_v=2.3e-04, delta_p=5.9e-06, s1=7.8e-04,
                  g1=4.2e-03, dbg1=1.8e-06, dba1=4.6e-03, s=9.1e-06, g=7.2e-06, dbg=1.8e-06, dba=9.5e-05, p=1.4e-05, v=1.3e-05),
    "cut": dict(pose_R=5.4e-08, pose_t=1.9e-06, link=2.5e-06, centre=7.3e-07, delta_raw_v=1.5e-04, delta_R=4.7e-08, delta_v=1.1e-04, delta_p=2.9e-06, s1=3.3e-04,
                 g1=2.9e-03, dbg1=1.8e-06, dba1=2.2e-03, s=6.6e-04, g=5.9e-03, dbg=1.9e-06, dba=5.9e-03, p=1.1e-03, v=1.3e-03),
}
CONTROLS = ("r_ic transposed in the alignment", "p_ci = 0", "t negated", "link scales inverted", "dba applied with the opposite sign")
CONTROL_RATIO = 10.0


@functools.lru_cache(maxsize=None)
def chain(name, control=None):
    """(scenario, the records of every call, the ladder) of the CPU chain"""
    sc = cc.scenario(name)
    be = cc.Cpu(break_=control)
    recs = cc.records(be, cc.run_chain(be, sc))
    return sc, recs, cc.ladder(sc, recs)


def conditions(sc, recs, where):
    """(b), for the records of either side"""
    name, prev = sc["name"], sc["prev"]
    pose, link, traj = (cc.joined(recs, k) for k in ("pose", "link", "traj"))
    lost = cc.LOST_AT if name == "lost" else -1
    since = {}                                                        # saved frames since the epoch's parent
    for i in range(cc.N):
        if int(prev[i]) < 0:
            continue
        if i == lost:
            assert not pose[i]["R"].any() and int(traj[i]["flags"]) == tj.TJ_ROOT | tj.TJ_NO_POSE, (where, i)
            continue
        assert int(pose[i]["n_inliers"]) >= 100 and pose[i]["R"].any(), (where, i, pose[i]["n_inliers"])
        e = int(traj[i]["epoch_seq"])
        since[e] = since.get(e, 0) + 1
        if since[e] >= 2:                                             # the third saved frame of the epoch (its parent, its unit edge, this one) on
            assert int(link[i]["flags"]) == sl.SL_OK and int(link[i]["n_shared"]) >= 30, (where, i, link[i])
        else:
            assert int(traj[i]["flags"]) == tj.TJ_UNIT_EDGE, (where, i)
    r1, r2 = recs[-1]["res1"], recs[-1]["res2"]
    for r in (r1, r2):
        assert int(r["ba_flags"]) == 0 and int(r["n_ba_triples"]) >= 16 and int(r["n_ba_triples"]) == int(r["a"]["n_triples"]), (where, r)
    if name in ("chain", "cut"):
        assert int(r1["a"]["flags"]) == 0 and int(r1["a"]["n_triples"]) == cc.N - 2 and (int(r1["a"]["segment_seq"]), int(r1["a"]["epoch_seq"])) == (0, 1)
    if name == "gated":
        assert int(r1["a"]["flags"]) == 0 and int(r1["a"]["n_triples"]) == cc.N // 2 - 2 and int(r1["a"]["epoch_seq"]) == 2
    if name == "lost":                                                # a new root, and the carried sums are another segment's
        assert int(r1["a"]["flags"]) == vr.VIA_RESTART and (int(r1["a"]["segment_seq"]), int(r1["a"]["epoch_seq"])) == (lost, lost + 1)
        assert int(r1["a"]["n_triples"]) == cc.N - lost - 2
        assert int(link[lost]["flags"]) & sl.SL_FEW and int(link[lost + 1]["flags"]) == sl.SL_NO_DEPTH
    if name == "thin":                                                # a held scale: a new epoch of the same segment
        k = cc.THIN_AT
        assert int(link[k]["flags"]) == sl.SL_FEW and int(link[k]["n_shared"]) <= cc.THIN_KEEP and int(traj[k]["flags"]) == tj.TJ_UNIT_EDGE
        assert abs(float(traj[k]["sigma"]) / float(traj[k - 1]["sigma"]) - 1.0) <= 16 * DOUBLING_BOUND    # (the doubling rounds the two products apart)
        assert int(r1["a"]["flags"]) == 0 and (int(r1["a"]["segment_seq"]), int(r1["a"]["epoch_seq"])) == (0, k) and int(r1["a"]["n_triples"]) == cc.N - k - 1
    # the second round: both steps shrink, and the gyro cost fell in the first.  (The gyro problem is linear in dbg up to |JRg dbg|^2 = 1e-6, the
    # second dba is what the first alignment's uncorrected gyro bias cost it, a few percent of the planted bias: three and one decade of room.)
    assert np.abs(r2["a"]["dbg"]).max() < 1e-3 * np.abs(r1["a"]["dbg"]).max() and np.abs(r2["dba"]).max() < 0.1 * np.abs(r1["dba"]).max(), (where, r1, r2)
    assert float(r1["a"]["c1"]) < 1e-6 * float(r1["a"]["c0_call"]), (where, r1["a"])


def test_the_world_meets_the_conditions_the_chain_needs():
    """baselines of 0.03 m and more, 150 common points a pair inside the 752 x 480 image, 30 shared by three consecutive saved frames, rows within 512"""
    w = cc.world()
    for name in cc.SCENARIOS:
        sc = cc.scenario(name)
        prev, ids = sc["prev"], sc["ids"]
        for i in range(cc.N):
            q = int(prev[i])
            if q < 0:
                continue
            assert np.linalg.norm(w["P"][i] - w["P"][q]) >= cc.MIN_BASELINE, (name, i)
            assert int((w["seen"][q] & w["seen"][i]).sum()) >= 150, (name, i)
            assert len(ids[i]) == (4 if (name, i) == ("lost", cc.LOST_AT) else cc.MAX_PTS) and len(ids[i]) <= 512
            if int(prev[q]) >= 0 and (name, i) != ("thin", cc.THIN_AT) and not (name == "lost" and i in (cc.LOST_AT, cc.LOST_AT + 1)):
                assert len(np.intersect1d(ids[i], ids[q])) >= 30, (name, i)
    assert w["xy"].dtype == np.float32 and len(w["samples"]) > cc.N * cc.HZ / cc.FPS


@pytest.mark.parametrize("name", cc.SCENARIOS)
def test_the_ladder_against_truth(name):
    sc, recs, e = chain(name)
    print(f"\n{name}: " + ", ".join(f"{k} {v:.2e}" for k, v in e.items()))
    conditions(sc, recs, name)
    T = cc.truth(sc)
    if name == "lost":                                                # the scale of the new gauge, not the old one's
        assert abs(T["s"] / T["base"](1) - 1.0) > 0.05 and T["root"] == cc.LOST_AT
    if name == "thin":
        assert abs(T["s"] / T["base"](1) - 1.0) > 1e-3 and T["edge"] == cc.THIN_AT
    for k, v in e.items():
        assert v <= 4 * MEASURED[name][k], (name, k, v, MEASURED[name][k])


@pytest.mark.parametrize("control", CONTROLS)
def test_a_broken_convention_shows(control):
    base, e = chain("chain")[2], chain("chain", control)[2]
    ratio = {k: e[k] / base[k] for k in e}
    worst = max(ratio, key=ratio.get)
    print(f"\n{control}: {worst} {e[worst]:.2e}, {ratio[worst]:.1e} times the unbroken chain's")
    assert ratio[worst] >= CONTROL_RATIO, (control, ratio)


def as_one_call(sc, recs, delta="delta"):
    """the calls of a cut as the rows of one call, in stream numbering"""
    prev = sc["prev"]
    traj, d, jac = cc.joined(recs, "traj").copy(), cc.joined(recs, delta).copy(), cc.joined(recs, "jac").copy()
    traj["parent"] = np.where(traj["flags"] & (tj.TJ_NOT_SAVED | tj.TJ_OVERFLOW), 0, prev)
    d["q"] = jac["q"] = prev
    return prev, traj, d, jac


def compare_cut_with_chain(sc, cut, whole):
    """(d): the records of the two cuts of one stream, within the bounds the stages document"""
    same = lambda k, f=None: cc.joined(cut, k).tobytes() == cc.joined(whole, k).tobytes() if f is None else \
        all(cc.joined(cut, k)[x].tobytes() == cc.joined(whole, k)[x].tobytes() for x in f)
    for k in ("pose0", "mask0", "polish", "pose", "mask", "points", "flags", "depth"):
        assert same(k), k
    assert same("link", ("scale", "q25", "q75", "n_shared", "flags"))
    assert same("delta", ("R", "v", "p", "dt", "JRg", "n_steps", "flags")) and same("jac", jr.BLOCKS + ("flags",))
    a, b = cc.joined(cut, "traj"), cc.joined(whole, "traj")
    for f in ("segment_seq", "epoch_seq", "hops", "unit_edges", "flags"):
        assert (a[f] == b[f]).all(), f
    d = differences(a, b, path_lengths(b))
    assert max(d) <= 16 * DOUBLING_BOUND, d
    # the first alignment's carried sums against the restatement over the cut's own records as ONE call
    scale = {}
    rows = as_one_call(sc, cut)
    _, res, co = br.align_ba_rows(cc.VP, cc.BP, *rows, detail=scale)
    vr.align_rows(cc.VP, *rows[:3], detail=scale)
    got, carry = cut[-1]["res1"], cut[-1]["ba_carry1"]
    for f in ("n_pairs", "n_triples", "segment_seq", "epoch_seq"):
        assert int(got["a"][f]) == int(res["a"][f]), f
    assert int(got["n_ba_triples"]) == int(res["n_ba_triples"]) == cc.N - 2
    dg, dl = vc.sum_differences(carry["carry"], co["carry"], scale)
    db = float((np.abs(carry[0]["ba"] - co[0]["ba"]) / np.maximum(scale["ba"], 1e-300)).max())
    assert dg <= CUT_BOUND["gyro"] and dl <= CUT_BOUND["lin"] and db <= CUT_BOUND_BA["ba"], (dg, dl, db)
    return d, (dg, dl, db)


def test_cut_against_chain():
    sc, cut, _ = chain("cut")
    _, whole, _ = chain("chain")
    d, sums = compare_cut_with_chain(sc, cut, whole)
    print(f"\ncut (23, 17) against chain: trajectory dR {d[0]:.1e}, d sigma {d[1]:.1e}, dt {d[2]:.1e}; carried sums gyro {sums[0]:.1e}, lin {sums[1]:.1e}, ba {sums[2]:.1e}")
