"""GPU: the visual-inertial alignment as a stream, through vis_batch_run on the 37 small synthetic frames of tests/ftrack_stream_cases.py with the
200 Hz IMU of tests/imu_cases.py beside them, keyframe gate off and on.  (The synthetic images and the synthetic IMU are unrelated motions: the
solution is flagged or meaningless, which is part of what is compared -- the planted motion is tests/test_vi_align_gpu.py's, and the chain from
pixels to the biases on ONE world is tests/test_vi_chain_gpu.py's, row level: a frame-stream version needs an image generator whose camera
accelerates -- these frames move at constant velocity, which never excites the alignment -- and is out of scope.)

a. Per launch: vis_batch_vi_align behind triangulate -> scale links -> trajectory -> imu, against vis_vi_align_rows fed with the downloaded records,
   vis_batch_get_keyframes' pairing and the carry so far, BYTE FOR BYTE, and both against the restatement.
b. Cuts A - D: the trajectory records of two cuts differ themselves, so each cut's carried sums are compared with the restatement's
   over the cut's own records taken as ONE call, within CUT_BOUND of tests/test_vi_align_ref.py relative to the summed absolute terms; the counts
   and (S, E) exactly, there and between the cuts.
c. A call repeated within a run gives the same bytes; a launch that was not aligned leaves the next one without a carry; vis_batch_reset and
   vis_batch_plan forget the carry; vis_batch_vi_align_init sets it.
d. The chain queued with no wait equals the same calls synchronised one by one with the records taken through the host, byte for byte.
Output buffers are pre-filled with 0xEE and everything behind the written extent must keep it."""
import numpy as np
import pytest

import ftrack_ref as fr
import ftrack_stream_cases as sc
import imu_cases as ic
import imu_ref as ir
import test_trajectory_stream_gpu as ts
import trajectory_ref as tj
import vi_align_cases as vc
import vi_align_ref as vr
from test_vi_align_gpu import rows_on_device
from test_vi_align_ref import CUT_BOUND

pytestmark = pytest.mark.gpu
FILL = ts.FILL
W, H, N = sc.W, sc.H, sc.N
IP = ic.params()
VP = vr.Params(r_ic=IP.r_ic, p_ci=vc.P_CI, min_pairs=3, min_triples=3)
SAMPLES, TFRAME, T_BEFORE = ic.stream(40, 10)


class Stream(ts.Stream):
    """the trajectory stream's context and buffers with the IMU rows and the alignment's outputs beside them, and the carry the next launch continues"""

    def __init__(self, vislam, torch, frames, gate, B):
        super().__init__(vislam, torch, frames, gate, B)
        self.s, self.tf = ts._dev(torch, SAMPLES.view(np.uint8)), ts._dev(torch, TFRAME)
        self.ip, self.vp = ic.struct_params(vislam, IP), vc.struct_params(vislam, VP)

    def forget(self):
        super().forget()
        self.via = None

    def buffers(self, n):
        b = super().buffers(n)
        b.update(delta=ts._filled(self.torch, (n + 1) * 216), state=ts._filled(self.torch, (n + 1) * 64), result=ts._filled(self.torch, 160 + 64))
        return b

    def follow(self, b, align=True, **kw):
        super().follow(b, **kw)
        self.c.batch_imu(self.n, self.s.data_ptr(), len(SAMPLES), self.tf.data_ptr() + 8 * self.at, b["delta"].data_ptr(), 0, self.ip)
        if align:
            self.align(b)

    def align(self, b):
        self.c.batch_vi_align(self.n, b["traj"].data_ptr(), b["delta"].data_ptr(), b["result"].data_ptr(), b["state"].data_ptr(), self.vp)

    def records(self, b):
        n = self.n
        self.c.batch_sync()
        assert self.c.batch_status() == 0
        raw = {k: b[k].cpu().numpy() for k in ("traj", "delta", "state", "result")}
        for k, size in (("traj", n * 128), ("delta", n * 216), ("state", n * 64), ("result", 160)):
            assert (raw[k][size:] == FILL).all(), k
        return dict(traj=raw["traj"][:n * 128].view(tj.TRAJ_DTYPE).copy(), delta=raw["delta"][:n * 216].view(ir.DELTA_DTYPE).copy(),
                    state=raw["state"][:n * 64].view(vr.STATE_DTYPE).copy(), result=raw["result"][:160].view(vr.RESULT_DTYPE)[0].copy(),
                    prev=self.c.batch_get_keyframes())

    def check(self, b, where):
        g = self.records(b)
        want = vr.align_rows(VP, g["prev"], g["traj"], g["delta"], self.via)
        assert g["result"].tobytes() == want[1].tobytes(), (where, g["result"], want[1])
        assert g["state"].tobytes() == want[0].tobytes(), (where, [i for i in range(self.n) if g["state"][i].tobytes() != want[0][i].tobytes()])
        rows = rows_on_device(self.v, self.c, VP, g["prev"], g["traj"], g["delta"], self.via)
        assert rows[0].tobytes() == g["state"].tobytes() and rows[1].tobytes() == g["result"].tobytes() and rows[2].tobytes() == want[2].tobytes(), where
        assert vc.all_finite(*want), where
        g["carry"] = want[2]
        return g

    def advance(self, g, aligned=True):
        self.via = g["carry"] if aligned else None
        g["gprev"] = sc.globalise(g["prev"], self.at, self.last_saved)
        saved = [i for i in range(self.n) if int(g["prev"][i]) != fr.KF_NOT_SAVED]
        if saved:
            self.last_saved = self.at + saved[-1]
        self.at += self.n

    def step(self, n, where):
        b = self.buffers(n)
        self.run(n)
        self.follow(b)
        g = self.check(b, where)
        self.advance(g)
        return g


@pytest.fixture(scope="module")
def frames(vislam, canvas):
    plain = sc.stream_frames(vislam, canvas, n=40)
    out = {}
    for gate in (False, True):
        f = plain.copy()
        if gate:
            f[sc.FLAT] = 128
        out[gate] = f
    return out


def as_one_call(gs):
    """the launches of a cut as the rows of one call: the pairing, the records' parents and the deltas' q in stream numbering"""
    gprev = np.array(sum((g["gprev"] for g in gs), []), np.int32)
    traj, delta = np.concatenate([g["traj"] for g in gs]), np.concatenate([g["delta"] for g in gs])
    traj["parent"] = np.where(traj["flags"] & (tj.TJ_NOT_SAVED | tj.TJ_OVERFLOW), 0, gprev)
    delta["q"] = gprev
    return gprev, traj, delta


@pytest.mark.parametrize("gate", [False, True], ids=["gate_off", "gate_on"])
def test_cuts_of_the_stream(vislam, frames, gate):
    import torch
    streams = {B: Stream(vislam, torch, frames[gate][:N], gate, B) for B in sorted(set(sc.PLAN_B.values()))}
    last = {}
    for name, cut in sc.CUTS.items():
        s = streams[sc.PLAN_B[name]]
        s.c.batch_reset()
        s.forget()
        s.at = 0
        gs = [s.step(n, (name, k)) for k, n in enumerate(cut)]
        scale = {}
        _, res, co = vr.align_rows(VP, *as_one_call(gs), detail=scale)
        got, carry = gs[-1]["result"], gs[-1]["carry"]
        for f in ("n_pairs", "n_triples", "segment_seq", "epoch_seq"):
            assert int(got[f]) == int(res[f]), (name, f)
        d = vc.sum_differences(carry, co, scale)
        print(f"\ngate {gate}, cut {name}: {int(got['n_pairs'])} pairs, {int(got['n_triples'])} triples, flags {int(got['flags'])}, sums differ by {d}")
        assert d[0] <= CUT_BOUND["gyro"] and d[1] <= CUT_BOUND["lin"], (name, d)
        last[name] = got
    for s in streams.values():
        s.close()
    whole = last["B"]
    assert int(whole["n_pairs"]) >= 20 and int(whole["n_triples"]) >= 3           # not a comparison of empty sums
    for name in sc.CUTS:
        for f in ("n_pairs", "n_triples", "segment_seq", "epoch_seq"):
            assert int(last[name][f]) == int(whole[f]), (name, f)


@pytest.mark.parametrize("gate", [False, True], ids=["gate_off", "gate_on"])
def test_call_patterns(vislam, frames, gate):
    """cut C: the call twice per run; launch 1 of 5 not aligned; a reset before the last launch; then a new plan, and vis_batch_vi_align_init"""
    import torch
    s = Stream(vislam, torch, frames[gate][:N], gate, 8)
    for k, n in enumerate(sc.CUTS["C"]):
        if k == 4:
            s.c.batch_reset()
            s.forget()
        b = s.buffers(n)
        s.run(n)
        s.follow(b, align=k != 1)
        if k == 1:                                                   # not aligned: the next launch has no carry
            g = s.records(b)
            assert (np.frombuffer(g["result"].tobytes(), np.uint8) == FILL).all()
            s.advance(dict(prev=g["prev"]), aligned=False)
            continue
        b2 = dict(b, state=ts._filled(torch, (n + 1) * 64), result=ts._filled(torch, 160 + 64))
        s.align(b2)
        g1, g2 = s.check(b, ("first", k)), s.check(b2, ("again", k))
        assert g1["state"].tobytes() == g2["state"].tobytes() and g1["result"].tobytes() == g2["result"].tobytes()
        if k in (2, 4):
            assert int(g1["result"]["n_pairs"]) == int(g1["result"]["n_pairs_call"])      # nothing carried
        if k == 3:
            assert int(g1["result"]["n_pairs"]) > int(g1["result"]["n_pairs_call"])
        s.advance(g1)
    s.c.batch_plan(W, H, W, 8)                                       # a new plan forgets the carry
    s.forget()
    s.at = 0
    g = s.step(8, "after plan")
    assert int(g["result"]["n_pairs"]) == int(g["result"]["n_pairs_call"])
    rec = vc.scene(8, "chain", "sums")["carry"]                     # vis_batch_vi_align_init: the next run continues from this record
    s.c.batch_vi_align_init(rec[0])
    s.via = rec
    g = s.step(8, "after init")
    assert int(g["result"]["n_pairs"]) == int(g["result"]["n_pairs_call"]) + int(rec[0]["n_pairs"])
    s.c.batch_vi_align_init(None)
    s.via = None
    g = s.step(8, "after init(None)")
    assert int(g["result"]["n_pairs"]) == int(g["result"]["n_pairs_call"])
    s.close()


def _sequence(vislam, torch, f, gate, through_host):
    """four launches of 8: run, triangulate, scale links, trajectory, imu, alignment, every launch into buffers of its own"""
    s = Stream(vislam, torch, f, gate, 8)
    bufs = [s.buffers(8) for _ in range(4)]
    for k in range(4):
        b = bufs[k]
        s.run(8)
        if not through_host:
            s.follow(b)
        else:
            s.follow(b, align=False)
            s.c.batch_sync()
            again = {name: torch.from_numpy(b[name].cpu().numpy().copy()).cuda() for name in ("traj", "delta")}
            torch.cuda.synchronize()
            s.align(dict(b, **again))
            s.c.batch_sync()
        s.at += 8
    s.c.batch_sync()
    assert s.c.batch_status() == 0
    got = {name: [b[name].cpu().numpy().tobytes() for b in bufs] for name in ("state", "result", "traj", "delta")}
    s.close()
    return got


@pytest.mark.parametrize("gate", [False, True], ids=["gate_off", "gate_on"])
def test_the_chain_queued_equals_the_chain_through_the_host(vislam, frames, gate):
    import torch
    f = frames[gate][:32]
    queued, synced = _sequence(vislam, torch, f, gate, False), _sequence(vislam, torch, f, gate, True)
    res = [np.frombuffer(r[:160], vr.RESULT_DTYPE)[0] for r in synced["result"]]
    print(f"\ngate {gate}: pairs {[int(r['n_pairs']) for r in res]}, triples {[int(r['n_triples']) for r in res]}, flags {[int(r['flags']) for r in res]}")
    assert int(res[-1]["n_pairs"]) >= 16 and int(res[-1]["n_pairs"]) > int(res[-1]["n_pairs_call"])   # not empty, and carried across the launches
    for name in synced:
        for k in range(4):
            assert queued[name][k] == synced[name][k], (name, k)


def test_run_directory_writes_the_states(vislam, frames, tmp_path):
    """tools/run_directory.py --imu --trajectory --vi-align: one state per frame under its batch's solution, the last batch's record in the JSON line,
    the sums carried across the batches"""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    n, nb, base = 12, 6, 1403636579763555584
    f = frames[False][:n]
    d = tmp_path / "cam0" / "data"
    d.mkdir(parents=True)
    stamps = [base + 50000000 * t for t in range(n)]
    for t in range(n):
        (d / f"{stamps[t]}.pgm").write_bytes(b"P5\n%d %d\n255\n" % (W, H) + f[t].tobytes())
    ns = [base - 100000000 + 5000000 * k + 1234567 for k in range(160)]
    rows = [(t,) + tuple(v for part in ic.body_rate(100.0 + (t - base) * 1e-9) for v in part) for t in ns]
    imu = tmp_path / "imu.csv"
    imu.write_text("#timestamp [ns],w_x,w_y,w_z,a_x,a_y,a_z\n" + "".join("%d,%r,%r,%r,%r,%r,%r\n" % r for r in rows))
    out = {k: tmp_path / f"{k}.csv" for k in ("imu", "traj", "via")}
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(root, "tools", "run_directory.py"), str(d), "--batch", str(nb),
                        "--imu", str(imu), "--imu-out", str(out["imu"]), "--trajectory", str(out["traj"]), "--vi-align", str(out["via"])],
                       capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    j = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    got = [l.split(",") for l in out["via"].read_text().splitlines()]
    deltas = [l.split(",") for l in out["imu"].read_text().splitlines()]
    assert len(got) == n and all(len(row) == 11 for row in got) and j["vi_align_csv"] == str(out["via"])
    for i, row in enumerate(got):
        assert [int(row[0]), int(row[1])] == [i, stamps[i]] and int(row[3]) == int(deltas[i][3])        # the state's q is the delta's
        assert all(np.isfinite(float(v)) for v in row[4:])
    pairs = sum(1 for row in got if int(row[2]) & vr.VIS_HAS_PAIR)
    assert j["vi_align"]["pairs"] == pairs >= 8 and int(got[6][3]) == ir.KF_CARRIED and int(got[6][2]) & vr.VIS_HAS_PAIR   # the pair across the batches
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "run_directory.py"), str(d), "--vi-align", str(out["via"])], capture_output=True, text=True)
    assert r.returncode != 0 and "--vi-align needs --imu and --trajectory" in r.stderr
