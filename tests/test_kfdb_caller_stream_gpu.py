"""GPU: the rows forms of the keyframe database (vis_kfdb_add_rows, _query_rows, _match_rows) on a CALLER's stream (vis_set_stream), under the rules
and with the rig of tests/stream_order_cases.py: the producer of every device input is still pending on the stream S when the call is queued -- only
stream order can make the call see the real inputs -- and the outputs are read by a consumer on S.  Per input a decoy run shows that a stale read
would be seen.  The database's own state is set up synchronised (prepare), or, in the add case, by the late call itself."""
import numpy as np
import pytest

import kfdb_cases as kc
import kfdb_ref as kr
import stream_order_cases as so
from test_imu_caller_stream_gpu import Env, _check

pytestmark = pytest.mark.gpu
NE, NQ, CAP, TOPK = 5, 3, 96, 2


def _data():
    E, Q, _ = kc.planted_sets(31, 96, 96)
    rng = np.random.default_rng(2)
    ek, ed, en = kc.rows(rng, [E[:96], E[:80], E[10:90], E[:33], E[40:96]], CAP)
    qk, qd, qn = kc.rows(rng, [Q[:96], Q[:70], Q[20:96]], CAP)
    return dict(ek=ek, ed=ed, en=en, ei=np.arange(NE, dtype=np.int32), qk=qk, qd=qd, qn=qn, qi=np.array([10, 11, 12], np.int32))


def _lp(vislam):
    lp, lq = vislam.default_loop_params(), kr.Params(min_gap=2, min_score=1, topk=TOPK)
    lp.min_gap, lp.min_score, lp.topk = 2, 1, TOPK
    return lp, lq


def _reference(D, lq):
    db = kr.KfDb(4, CAP)                                          # (five rows into four slots: the ring wraps inside the call)
    db.add_rows(D["ek"], D["ed"], D["en"], D["ei"])
    scores, cand, query = db.query_rows(lq, D["qd"], D["qn"], D["qi"])
    fill = lambda dt, shape: np.full(int(np.prod(shape)) * np.dtype(dt).itemsize, so.FILL, np.uint8).view(dt).reshape(shape)
    m, p1, p2, npts = db.match_rows(lq, D["qk"], D["qd"], D["qn"], cand[:, 0], CAP, fill(kr.DMATCH_DTYPE, (NQ, CAP)), fill(np.float32, (NQ, CAP, 2)),
                                    fill(np.float32, (NQ, CAP, 2)), fill(np.int32, (NQ,)))
    return dict(scores=scores, cand=cand, query=query, m=m, p1=p1, p2=p2, npts=npts)


@pytest.fixture(scope="module")
def env(vislam):
    import torch
    E = Env()
    E.torch, E.S = torch, torch.cuda.Stream()
    E.cA = vislam.Context(0)
    E.cA.set_stream(E.S)
    E.db = E.cA.kfdb(4, CAP)
    E.D = _data()
    E.held = {k: so._upload(torch, v) for k, v in E.D.items()}    # synchronised twins of every row, for the calls that set the database up
    E.delay = so.Delay(torch, E.S)
    E.delay.measure()
    rig = so.Rig(torch, case_query(vislam, E))
    host = [so.run_sync(torch, E.cA, rig)[1] for _ in range(4)][2:]
    chain_ms, ok = E.delay.size(max(host))
    if not ok:
        pytest.fail(f"a chain of {so.FACTOR:g} x the host time {max(host):.3f} ms is {chain_ms:.1f} ms > {so.CHAIN_MAX_MS:g} ms")
    yield E
    torch.cuda.synchronize()
    E.cA.close()


def _setup(E):
    h = E.held

    def prepare(c, p):
        E.db.reset()
        E.db.add_rows(NE, h["ek"].data_ptr(), h["ed"].data_ptr(), h["en"].data_ptr(), CAP, h["ei"].data_ptr())
    return prepare


def case_query(vislam, E):
    D, (lp, _) = E.D, _lp(vislam)
    ins = dict(qd=(D["qd"], so.zeros(D["qd"])), qn=(D["qn"], D["qn"] // 2), qi=(D["qi"], so.zeros(D["qi"])))
    return so.Case("vis_kfdb_query_rows", so.CTX, ins, dict(scores=NQ * 4 * 4, cand=NQ * TOPK * 16, query=NQ * 32),
                   lambda c, p: E.db.query_rows(NQ, p("qd"), p("qn"), CAP, p("qi"), p("scores"), p("cand"), p("query"), lp), _setup(E))


def case_add(vislam, E):
    """the late inputs are the rows that are ADDED; the same call sequence then queries and emits, so every added byte shows"""
    D, h, (lp, _) = E.D, E.held, _lp(vislam)
    ins = dict(ek=(D["ek"], so.zeros(D["ek"])), ed=(D["ed"], so.zeros(D["ed"])), en=(D["en"], D["en"] // 2), ei=(D["ei"], D["ei"] + 9))

    def call(c, p):
        E.db.reset()
        E.db.add_rows(NE, p("ek"), p("ed"), p("en"), CAP, p("ei"))
        E.db.query_rows(NQ, h["qd"].data_ptr(), h["qn"].data_ptr(), CAP, h["qi"].data_ptr(), p("scores"), p("cand"), p("query"), lp)
        E.db.match_rows(NQ, h["qk"].data_ptr(), h["qd"].data_ptr(), h["qn"].data_ptr(), CAP, p("cand"), TOPK, CAP, p("m"), p("p1"), p("p2"), p("npts"), lp)
    return so.Case("vis_kfdb_add_rows", so.CTX, ins,
                   dict(scores=NQ * 4 * 4, cand=NQ * TOPK * 16, query=NQ * 32, m=NQ * CAP * 16, p1=NQ * CAP * 8, p2=NQ * CAP * 8, npts=NQ * 4), call)


def case_match(vislam, E, cand):
    D, (lp, _) = E.D, _lp(vislam)
    none = np.zeros_like(cand)
    none["id"], none["slot"] = -1, -1
    ins = dict(qk=(D["qk"], so.zeros(D["qk"])), qd=(D["qd"], so.zeros(D["qd"])), qn=(D["qn"], D["qn"] // 2), cand=(cand, none))
    return so.Case("vis_kfdb_match_rows", so.CTX, ins, dict(m=NQ * CAP * 16, p1=NQ * CAP * 8, p2=NQ * CAP * 8, npts=NQ * 4),
                   lambda c, p: E.db.match_rows(NQ, p("qk"), p("qd"), p("qn"), CAP, p("cand"), TOPK, CAP, p("m"), p("p1"), p("p2"), p("npts"), lp), _setup(E))


def test_query_rows_on_a_caller_stream(vislam, env):
    want, ref = _check(env, env.cA, case_query(vislam, env)), _reference(env.D, _lp(vislam)[1])
    for k in ("scores", "cand", "query"):
        assert want[k] == ref[k].tobytes(), k
    assert (ref["cand"]["score"][:, 0] > 10).all()


def test_add_rows_on_a_caller_stream(vislam, env):
    want, ref = _check(env, env.cA, case_add(vislam, env)), _reference(env.D, _lp(vislam)[1])
    for k in want:
        assert want[k] == ref[k].tobytes(), k


def test_match_rows_on_a_caller_stream(vislam, env):
    ref = _reference(env.D, _lp(vislam)[1])
    want = _check(env, env.cA, case_match(vislam, env, ref["cand"]))
    for k in want:
        assert want[k] == ref[k].tobytes(), k
    assert (ref["npts"] > 10).all()
