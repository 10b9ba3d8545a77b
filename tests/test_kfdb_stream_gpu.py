"""GPU: the batch forms of the keyframe database (vis_batch_kfdb_add, _query, _match) behind vis_batch_run on nine 320 x 240 synthetic frames in two
launches, keyframe gate off and on (two flat frames are not saved): byte-equal to the rows forms fed the read-back keypoints, and to the
restatement's replay of the same call sequence; query -> add -> query on one database across the context's stream and the pose stream with no
synchronisation in between; steps 1 and 4; vis_batch_reset, which keeps the database; VIS_E_CAPACITY when the plan's capacity exceeds kp_cap."""
import numpy as np
import pytest

import ftrack_stream_cases as sc
import kfdb_ref as kr

pytestmark = pytest.mark.gpu
FILL = 0xEE
W, H = sc.W, sc.H
CUT, FLAT, ECAP, TOPK, MAXP = (5, 4), (2, 6), 8, 3, 128
KF_NOT_SAVED = -2


def _filled(torch, nbytes):
    t = torch.full((nbytes + 16,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return t


def _dev(torch, a):
    t = torch.from_numpy(np.concatenate([np.ascontiguousarray(a).reshape(-1).view(np.uint8), np.zeros(16, np.uint8)])).cuda()
    torch.cuda.synchronize()
    return t


def _params(vislam):
    lp, lq = vislam.default_loop_params(), kr.Params(min_gap=2, min_score=1, topk=TOPK)
    lp.min_gap, lp.min_score, lp.topk = 2, 1, TOPK
    return lp, lq


class Outs:
    def __init__(self, torch, n):
        self.n = n
        self.sizes = dict(scores=n * ECAP * 4, cand=n * TOPK * 16, query=n * 32, m=n * MAXP * 16, p1=n * MAXP * 8, p2=n * MAXP * 8, npts=n * 4)
        self.t = {k: _filled(torch, v) for k, v in self.sizes.items()}

    def p(self, k):
        return self.t[k].data_ptr()

    def bytes(self):
        out = {}
        for k, v in self.sizes.items():
            raw = self.t[k].cpu().numpy()
            assert (raw[v:] == FILL).all(), k
            out[k] = raw[:v].tobytes()
        return out


def _readback(c, n, KC, seq0, step, gate):
    """the rows of the last launch as the batch forms use them: (kps, desc, nkp, ids); a frame the gate did not save or one off the step has count 0"""
    prev = c.batch_get_keyframes()
    kps, desc, nkp = np.zeros((n, KC), kr.KEYPOINT_DTYPE), np.zeros((n, KC, 32), np.uint8), np.zeros(n, np.int32)
    for i in range(n):
        k, d = c.batch_keypoints(i)
        kps[i, :len(k)], desc[i, :len(k)], nkp[i] = k, d, len(k)
        if (gate and prev[i] == KF_NOT_SAVED) or (seq0 + i) % step:
            nkp[i] = 0
    return kps, desc, nkp, seq0 + np.arange(n, dtype=np.int32)


@pytest.fixture(scope="module")
def frames(vislam, canvas):
    return {gate: sc.stream_frames(vislam, canvas, n=sum(CUT), flat=FLAT if gate else ()) for gate in (False, True)}


@pytest.mark.parametrize("step", [1, 4])
@pytest.mark.parametrize("gate", [False, True], ids=["gate_off", "gate_on"])
def test_batch_forms_equal_the_rows_forms_and_the_restatement(vislam, frames, gate, step):
    import torch
    c = vislam.Context(0, sc.stream_params(vislam, gate))
    c.batch_plan(W, H, W, max(CUT))
    KC = c.keypoint_capacity(W, H)
    dev = _dev(torch, frames[gate])
    lp, lq = _params(vislam)
    if step > 1:
        lp.min_gap = lq.min_gap = 1
    db_b, db_r, ref = c.kfdb(ECAP, KC), c.kfdb(ECAP, KC), kr.KfDb(ECAP, KC)
    at, n_scored, n_matched = 0, 0, 0
    for n in CUT:
        ob, orw = Outs(torch, n), Outs(torch, n)
        c.batch_run(dev.data_ptr() + at * W * H, n, vislam.STAGE_ALL)
        db_b.batch_query(n, ob.p("scores"), ob.p("cand"), ob.p("query"), step, lp)          # query, emit, add: queued with no host step
        db_b.batch_match(n, ob.p("cand"), TOPK, MAXP, ob.p("m"), ob.p("p1"), ob.p("p2"), ob.p("npts"), lp)
        db_b.batch_add(n, step)
        c.batch_sync()
        assert c.batch_status() == 0
        kps, desc, nkp, ids = _readback(c, n, KC, at, step, gate)
        t = [_dev(torch, a) for a in (kps, desc, nkp, ids)]
        db_r.query_rows(n, t[1].data_ptr(), t[2].data_ptr(), KC, t[3].data_ptr(), orw.p("scores"), orw.p("cand"), orw.p("query"), lp)
        db_r.match_rows(n, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), KC, orw.p("cand"), TOPK, MAXP, orw.p("m"), orw.p("p1"), orw.p("p2"), orw.p("npts"), lp)
        on = [i for i in range(n) if (at + i) % step == 0]
        if on:
            u = [_dev(torch, a[on]) for a in (kps, desc, nkp, ids)]
            db_r.add_rows(len(on), u[0].data_ptr(), u[1].data_ptr(), u[2].data_ptr(), KC, u[3].data_ptr())
        c.batch_sync()
        got, rows = ob.bytes(), orw.bytes()
        scores, cand, query = ref.query_rows(lq, desc, nkp, ids)
        fill = lambda dt, shape: np.full(int(np.prod(shape)) * np.dtype(dt).itemsize, FILL, np.uint8).view(dt).reshape(shape)
        m, p1, p2, npts = ref.match_rows(lq, kps, desc, nkp, cand[:, 0], MAXP, fill(kr.DMATCH_DTYPE, (n, MAXP)), fill(np.float32, (n, MAXP, 2)),
                                         fill(np.float32, (n, MAXP, 2)), fill(np.int32, (n,)))
        if on:
            ref.add_rows(kps[on], desc[on], nkp[on], ids[on])
        want = dict(scores=scores, cand=cand, query=query, m=m, p1=p1, p2=p2, npts=npts)
        for k in got:
            assert got[k] == rows[k], (k, "the batch form differs from the rows form", at)
            assert got[k] == want[k].tobytes(), (k, "the device differs from the restatement", at)
        n_scored += int(query["n_scored"].sum())
        n_matched += int(npts.sum())
        at += n
    ib, ir_ = db_b.info(), db_r.info()
    assert (ib.head, ib.total_added) == (ir_.head, ir_.total_added) == (ref.head, ref.total)
    for s in range(ECAP):
        a, b, r = db_b.get_entry(s), db_r.get_entry(s), ref.get_entry(s)
        assert a[:2] == b[:2] == r[:2] and a[2].tobytes() == b[2].tobytes() == r[2].tobytes(), s
    if gate and step == 1:
        assert [ref.cnt[s] for s in ((2 % ECAP), (6 % ECAP))] == [0, 0]                       # the flat frames became empty entries
    print(f"\ngate {gate} step {step}: {n_scored} couples scored, {n_matched} matches emitted, ring total {ref.total}")
    assert n_scored > 0 and (n_matched > 0 or step > 1)
    # vis_batch_reset keeps the database; the stream numbers restart at 0
    c.batch_reset()
    assert db_b.info().total_added == ref.total and db_b.get_entry(0)[:2] == ref.get_entry(0)[:2]
    c.batch_run(dev.data_ptr(), CUT[0], vislam.STAGE_ALL)
    o = Outs(torch, CUT[0])
    big = vislam.default_loop_params()
    big.min_gap, big.min_score, big.topk = 0, 1, TOPK
    db_b.batch_query(CUT[0], o.p("scores"), o.p("cand"), o.p("query"), 1, big)
    c.batch_sync()
    q = np.frombuffer(o.bytes()["query"], kr.QUERY_DTYPE)
    assert q["id"].tolist() == list(range(CUT[0])) and int(q["n_scored"].sum()) > 0              # the entries of the stream before the reset are scored
    c.close()


def test_query_add_query_across_the_two_streams_without_a_sync(vislam, frames):
    """rows query (context's stream), batch add (pose stream), rows query (context's stream), batch query (pose stream), queued back to back: the
    first query does not see the add, the other two do"""
    import torch
    c = vislam.Context(0, sc.stream_params(vislam, False))
    c.batch_plan(W, H, W, 5)
    KC = c.keypoint_capacity(W, H)
    dev = _dev(torch, frames[False])
    lp, lq = _params(vislam)
    lp.min_gap = lq.min_gap = 0
    db, ref = c.kfdb(ECAP, KC), kr.KfDb(ECAP, KC)
    c.batch_run(dev.data_ptr(), 5, vislam.STAGE_ALL)
    c.batch_sync()
    kps, desc, nkp, ids = _readback(c, 5, KC, 0, 1, False)
    t = [_dev(torch, a) for a in (kps, desc, nkp, ids + 100)]
    warm = Outs(torch, 5)
    db.query_rows(5, t[1].data_ptr(), t[2].data_ptr(), KC, t[3].data_ptr(), warm.p("scores"), warm.p("cand"), warm.p("query"), lp)   # (grows the workspace: synchronises)
    c.batch_sync()
    o1, o2, o3 = Outs(torch, 5), Outs(torch, 5), Outs(torch, 5)
    db.query_rows(5, t[1].data_ptr(), t[2].data_ptr(), KC, t[3].data_ptr(), o1.p("scores"), o1.p("cand"), o1.p("query"), lp)
    db.batch_add(5, 1)
    db.query_rows(5, t[1].data_ptr(), t[2].data_ptr(), KC, t[3].data_ptr(), o2.p("scores"), o2.p("cand"), o2.p("query"), lp)
    db.batch_query(5, o3.p("scores"), o3.p("cand"), o3.p("query"), 1, lp)
    c.batch_sync()
    before = ref.query_rows(lq, desc, nkp, ids + 100)
    ref.add_rows(kps, desc, nkp, ids)
    after, plan = ref.query_rows(lq, desc, nkp, ids + 100), ref.query_rows(lq, desc, nkp, ids)
    for o, want in ((o1, before), (o2, after), (o3, plan)):
        got = o.bytes()
        for k, w in zip(("scores", "cand", "query"), want):
            assert got[k] == w.tobytes(), k
    assert (before[0] == -1).all() and (after[0][:, :5] >= 0).all() and after[1]["id"][0, 0] == 0 and int(nkp[0]) >= int(after[1]["score"][0, 0]) >= 0.9 * nkp[0] > 50      # a frame against itself (identical descriptors apart)
    c.close()


def test_capacity_is_refused_not_cut(vislam, frames):
    import torch
    c = vislam.Context(0, sc.stream_params(vislam, False))
    c.batch_plan(W, H, W, 5)
    KC = c.keypoint_capacity(W, H)
    dev = _dev(torch, frames[False])
    c.batch_run(dev.data_ptr(), 5, vislam.STAGE_ALL)
    small, o = c.kfdb(4, KC - 1), Outs(torch, 5)
    lp, _ = _params(vislam)
    for call in (lambda: small.batch_add(5, 1), lambda: small.batch_query(5, o.p("scores"), o.p("cand"), o.p("query"), 1, lp),
                 lambda: small.batch_match(5, o.p("cand"), TOPK, MAXP, o.p("m"), o.p("p1"), o.p("p2"), o.p("npts"), lp)):
        with pytest.raises(vislam.VisError) as e:
            call()
        assert e.value.code == -4 and "kp_cap" in str(e.value)
    with pytest.raises(vislam.VisError) as e:
        small.batch_add(4, 1)                                     # n differs from the last run
    assert e.value.code == -5
    c.batch_sync()
    assert small.info().total_added == 0
    c.close()


def test_run_directory_writes_the_loop_candidates(vislam, canvas, tmp_path):
    """tools/run_directory.py --loops on an out-and-back walk over the synthetic stream (frames 0 ... 7, then 7 ... 0): one row per query with a
    candidate, the rows the calls give for the same frames in the same batches; the way back finds the way out"""
    import json
    import os
    import subprocess
    import sys

    import torch
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out8 = sc.stream_frames(vislam, canvas, n=8)
    f = np.concatenate([out8, out8[::-1]])
    n, nb, gap = len(f), 4, 3
    d = tmp_path / "cam0" / "data"
    d.mkdir(parents=True)
    stamp = lambda t: 1403636579763555584 + 50000000 * t
    for t in range(n):
        (d / f"{stamp(t)}.pgm").write_bytes(b"P5\n%d %d\n255\n" % (W, H) + f[t].tobytes())
    csv = tmp_path / "loops.csv"
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(root, "tools", "run_directory.py"), str(d), "--batch", str(nb),
                        "--loops", str(csv), "--loop-step", "1", "--loop-gap", str(gap), "--loop-entries", "32"], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    j = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    rows = [[int(v) for v in l.split(",")] for l in csv.read_text().splitlines()]
    p = vislam.default_params()                                    # the tool's parameters: ORB::create(200), fy = fx
    p.fy, p.nfeatures, p.w_size, p.h_size = p.fx, 200, W, H
    c = vislam.Context(0, p)
    c.batch_plan(W, H, W, nb)
    KC = c.keypoint_capacity(W, H)
    db = c.kfdb(32, KC)
    lp = vislam.default_loop_params()
    lp.min_gap = gap
    dev = _dev(torch, f)
    want = []
    for first in range(0, n, nb):
        ca, qu, p1, p2, npts, rec = (_filled(torch, b) for b in (nb * lp.topk * 16, nb * 32, nb * KC * 8, nb * KC * 8, nb * 4, nb * 192))
        c.batch_run(dev.data_ptr() + first * W * H, nb, vislam.STAGE_FRAME)
        db.batch_query(nb, 0, ca.data_ptr(), qu.data_ptr(), 1, lp)
        db.batch_match(nb, ca.data_ptr(), lp.topk, KC, 0, p1.data_ptr(), p2.data_ptr(), npts.data_ptr(), lp)
        db.batch_add(nb, 1)
        c.batch_sync()
        c.essential_batch(nb, p1.data_ptr(), p2.data_ptr(), npts.data_ptr(), KC, 0, 0, rec.data_ptr())
        c.batch_sync()
        cand = ca.cpu().numpy()[:nb * lp.topk * 16].view(kr.CAND_DTYPE).reshape(nb, lp.topk)
        m, pose = npts.cpu().numpy()[:nb * 4].view(np.int32), rec.cpu().numpy()[:nb * 192].view(vislam.POSE_RESULT_DTYPE)
        want += [[first + i, stamp(first + i), int(cand[i, 0]["id"]), int(cand[i, 0]["score"]), int(m[i]), int(pose[i]["n_inliers"])]
                 for i in range(nb) if cand[i, 0]["slot"] >= 0]
    c.close()
    assert rows == want and j["loops_csv"] == str(csv) and j["loops"]["candidates"] == len(rows) > 0
    back = {r_[0]: r_[2] for r_ in rows if r_[0] >= 8}
    print("\nway back -> candidate:", back)
    assert all(back.get(t) == 15 - t for t in range(12, 16))       # frames 12 ... 15 are frames 3 ... 0 again, an earlier batch and the gap behind them
