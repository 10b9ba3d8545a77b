"""GPU: the IMU preintegration as a stream, through vis_batch_run on the 37 small synthetic frames of tests/ftrack_stream_cases.py with a 200 Hz
IMU beside them, keyframe gate off and on.

a. Per launch: vis_batch_imu against vis_imu_preintegrate_rows fed with vis_batch_get_keyframes' pairing and the carry so far, BYTE FOR BYTE, and
   both against the restatement.
b. Cuts A - D of the stream against each other (q in stream numbering).  Gate off: the same bytes.  Gate on: a pair across a launch boundary is
   carry.open o (its intervals of the launch), another association of the same intervals: R within 16 x the bound tests/test_imu_ref.py measured
   between the lifting table and the left-to-right order, v, p, JRg relative to their largest entry alike, integers and flags equal, d_rot within
   2^-23 an entry.
c. The call repeated within a run gives the same bytes; a launch that was not integrated makes the carried pair VIS_IMU_NO_CARRY;
   vis_batch_reset and vis_batch_plan forget the carry; vis_batch_imu_init sets it.
d. vis_batch_imu -> vis_batch_f2f -> vis_batch_filter_keypoints queued with no wait equal the same calls with the rotations downloaded,
   uploaded again and synchronised, byte for byte.
e. Gate off: vis_imu_preintegrate_rows -> vis_batch_run_guided queued on the context's stream, each call's d_carry_out the next call's d_carry_in,
   equals the guided run given the same rotations from the host.
Every output sits between 0xEE guards."""
import numpy as np
import pytest

import ftrack_ref as fr
import ftrack_stream_cases as sc
import imu_cases as ic
import imu_ref as ir
from test_imu_gpu import GUARD, _dev, _guarded, _payload, rows_on_device
from test_imu_ref import LIFT_BOUND

pytestmark = pytest.mark.gpu
W, H, N = sc.W, sc.H, sc.N
P = ic.params()
SAMPLES, TFRAME, T_BEFORE = ic.stream(40, 10)                        # 200 Hz beside 20 frames a second


class Stream:
    """a context with a plan of B frames over the device frames, the whole stream's samples and frame times on the device; beside it the carry the
    next launch continues, as the rows form and the restatement produce it"""

    def __init__(self, vislam, torch, frames, gate, B):
        self.v, self.torch = vislam, torch
        self.c = vislam.Context(0, sc.stream_params(vislam, gate))
        self.dev = _dev(torch, frames)
        self.s, self.tf = _dev(torch, SAMPLES), _dev(torch, TFRAME)
        self.ip = ic.struct_params(vislam, P)
        self.c.batch_plan(W, H, W, B)
        self.forget()

    def forget(self):
        self.carry, self.at, self.last_saved = None, 0, None

    def close(self):
        self.c.close()

    def buffers(self, n):
        return _guarded(self.torch, n * 216), _guarded(self.torch, n * 36)

    def run(self, n):
        self.c.batch_run(self.dev.data_ptr() + self.at * W * H, n, self.v.STAGE_ALL)
        self.n = n

    def imu(self, b):
        self.c.batch_imu(self.n, self.s.data_ptr(), len(SAMPLES), self.tf.data_ptr() + 8 * self.at, b[0].data_ptr() + GUARD, b[1].data_ptr() + GUARD, self.ip)

    def check(self, b, where):
        n = self.n
        self.c.batch_sync()
        assert self.c.batch_status() == 0
        delta, rot = _payload(b[0], n * 216).view(ir.DELTA_DTYPE), _payload(b[1], n * 36).view(np.float32).reshape(n, 9)
        prev = self.c.batch_get_keyframes()
        tf = TFRAME[self.at:self.at + n]
        want = ir.preintegrate_rows(P, SAMPLES, tf, prev, self.carry)
        assert delta.tobytes() == want[0].tobytes(), (where, [i for i in range(n) if delta[i].tobytes() != want[0][i].tobytes()], prev)
        assert rot.tobytes() == want[1].tobytes(), where
        rows = rows_on_device(self.v, self.c, P, SAMPLES, tf, prev, self.carry)
        assert rows[0].tobytes() == delta.tobytes() and rows[1].tobytes() == rot.tobytes() and rows[2].tobytes() == want[2].tobytes(), where
        return dict(delta=delta.copy(), rot=rot.copy(), prev=prev, carry=want[2])

    def advance(self, g, integrated=True):
        self.carry = g["carry"] if integrated else None
        g["gprev"] = sc.globalise(g["prev"], self.at, self.last_saved)
        saved = [i for i in range(self.n) if int(g["prev"][i]) != fr.KF_NOT_SAVED]
        if saved:
            self.last_saved = self.at + saved[-1]
        self.at += self.n

    def step(self, n, where):
        b = self.buffers(n)
        self.run(n)
        self.imu(b)
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


def whole(gs):
    delta, rot = np.concatenate([g["delta"] for g in gs]), np.concatenate([g["rot"] for g in gs])
    delta["q"] = np.array(sum((g["gprev"] for g in gs), []), np.int32)
    return delta, rot


@pytest.mark.parametrize("gate", [False, True], ids=["gate_off", "gate_on"])
def test_cuts_of_the_stream(vislam, frames, gate):
    import torch
    streams = {B: Stream(vislam, torch, frames[gate][:N], gate, B) for B in sorted(set(sc.PLAN_B.values()))}
    out = {}
    for name, cut in sc.CUTS.items():
        s = streams[sc.PLAN_B[name]]
        s.c.batch_reset()
        s.forget()
        out[name] = whole([s.step(n, (name, k)) for k, n in enumerate(cut)])
    for s in streams.values():
        s.close()
    delta, rot = out["B"]                                           # one launch: the stream as a whole
    paired = ~(delta["flags"] & (ir.IMU_NO_PAIR | ir.IMU_NO_CARRY)).astype(bool)
    lengths = [i - int(delta[i]["q"]) for i in range(N) if paired[i]]
    print(f"\ngate {gate}: {int(paired.sum())} of {N} frames with a pair, lengths up to {max(lengths)}, flags {sorted(set(delta['flags'].tolist()))}")
    assert paired.sum() >= 25 and (delta["flags"][paired] == 0).all() and (max(lengths) >= 5 if gate else max(lengths) == 1)
    assert [i for i in range(N) if int(delta[i]["q"]) == fr.KF_NOT_SAVED] == (sc.FLAT if gate else [])
    assert (np.abs(rot[paired] - np.eye(3, dtype=np.float32).reshape(9)).max(axis=1) > 1e-3).all()      # not a comparison of identities
    for name, cut in sc.CUTS.items():
        d, r = out[name]
        for f in ("n_steps", "flags", "q"):
            assert (d[f] == delta[f]).all(), (name, f)
        if not gate:
            assert d.tobytes() == delta.tobytes() and r.tobytes() == rot.tobytes(), (name, [i for i in range(N) if d[i].tobytes() != delta[i].tobytes()])
            continue
        assert d["dt"] == pytest.approx(delta["dt"], rel=1e-14, abs=0)
        assert np.abs(d["R"] - delta["R"]).max() <= LIFT_BOUND["R"], name
        for f in ("v", "p", "JRg"):
            scale = np.abs(delta[f]).max(axis=1, keepdims=True)
            assert (np.abs(d[f] - delta[f]) <= LIFT_BOUND[f] * scale).all(), (name, f)
        assert np.abs(r.astype(np.float64) - rot).max() <= 2.0 ** -23, name
        firsts = np.cumsum([0] + cut[:-1])[1:]                      # the pairs across a launch boundary exist
        assert name == "B" or any(paired[i] for i in firsts)


@pytest.mark.parametrize("gate", [False, True], ids=["gate_off", "gate_on"])
def test_call_patterns(vislam, frames, gate):
    """cut C: the call twice per run; launch 1 of 5 not integrated; a reset before the last launch; then a new plan, and vis_batch_imu_init"""
    import torch
    s = Stream(vislam, torch, frames[gate][:N], gate, 8)
    for k, n in enumerate(sc.CUTS["C"]):
        if k == 4:
            s.c.batch_reset()
            s.forget()
            s.at = 32
        s.run(n)
        if k == 1:                                                   # not integrated: the next launch's carried pair has no carry
            s.c.batch_sync()
            g = dict(prev=s.c.batch_get_keyframes())
            s.advance(g, integrated=False)
            continue
        b1, b2 = s.buffers(n), s.buffers(n)
        s.imu(b1)
        s.imu(b2)
        g1, g2 = s.check(b1, ("first", k)), s.check(b2, ("again", k))
        assert g1["delta"].tobytes() == g2["delta"].tobytes() and g1["rot"].tobytes() == g2["rot"].tobytes()
        carried = [i for i in range(n) if int(g1["prev"][i]) == fr.KF_CARRIED]
        if k == 2:
            assert carried and all(int(g1["delta"][i]["flags"]) == ir.IMU_NO_CARRY for i in carried)
        if k == 3:
            assert carried and all(int(g1["delta"][i]["flags"]) == 0 for i in carried)
        if k == 4:
            assert int(g1["prev"][0]) == fr.KF_FIRST and int(g1["delta"][0]["flags"]) == ir.IMU_NO_PAIR
        s.advance(g1)
    s.c.batch_plan(W, H, W, 8)                                       # a new plan forgets the carry
    s.forget()
    g = s.step(8, "after plan")
    assert int(g["delta"][0]["flags"]) == ir.IMU_NO_PAIR
    rec = ic.carried(float(TFRAME[7]) - 0.004, True)                # vis_batch_imu_init: the next run continues from this record
    s.c.batch_imu_init(rec[0])
    s.carry = rec
    g = s.step(8, "after init")
    first = [i for i in range(8) if int(g["prev"][i]) == fr.KF_CARRIED][0]
    assert int(g["delta"][first]["flags"]) == 0 and int(g["delta"][first]["n_steps"]) > int(rec[0]["open"]["n_steps"])
    s.c.batch_imu_init(None)
    s.carry = None
    g = s.step(8, "after init(None)")
    first = [i for i in range(8) if int(g["prev"][i]) == fr.KF_CARRIED][0]
    assert int(g["delta"][first]["flags"]) == ir.IMU_NO_CARRY
    s.close()


def _f2f_sequence(vislam, torch, f, gate, through_host):
    """four launches of 8: run, vis_batch_imu, vis_batch_f2f, vis_batch_filter_keypoints, every call into buffers of its own"""
    s = Stream(vislam, torch, f, gate, 8)
    cap = int(np.floor(np.sqrt(s.c.params.n_cells))) ** 2
    draws = _dev(torch, np.random.default_rng(5).integers(0, 2 ** 31, (s.c.params.f2f_iters, 2)).astype(np.int32))
    tdir = _dev(torch, np.tile(np.array([0.6, 0.0, 0.8], np.float32), (8, 1)))
    bufs = [dict(delta=_guarded(torch, 8 * 216), rot=_guarded(torch, 8 * 36), f2f=_guarded(torch, 8 * 32), keep=_guarded(torch, 8 * cap), nkeep=_guarded(torch, 32))
            for _ in range(4)]
    again = [torch.zeros(8 * 36, dtype=torch.uint8, device="cuda") for _ in range(4)]
    torch.cuda.synchronize()
    for k in range(4):
        b = bufs[k]
        s.run(8)
        s.imu((b["delta"], b["rot"]))
        rot = b["rot"].data_ptr() + GUARD
        if through_host:
            s.c.batch_sync()
            again[k].copy_(torch.from_numpy(_payload(b["rot"], 8 * 36).copy()))
            torch.cuda.synchronize()
            rot = again[k].data_ptr()
        s.c.batch_f2f(8, rot, 0, draws.data_ptr(), b["f2f"].data_ptr() + GUARD)
        if through_host:
            s.c.batch_sync()
        s.c.batch_filter_keypoints(8, rot, tdir.data_ptr(), 2000.0, cap, b["keep"].data_ptr() + GUARD, b["nkeep"].data_ptr() + GUARD)
        if through_host:
            s.c.batch_sync()
        s.at += 8
    s.c.batch_sync()
    assert s.c.batch_status() == 0
    sizes = dict(delta=8 * 216, rot=8 * 36, f2f=8 * 32, keep=8 * cap, nkeep=32)
    got = {name: [_payload(b[name], sizes[name]).tobytes() for b in bufs] for name in sizes}
    s.close()
    return got


@pytest.mark.parametrize("gate", [False, True], ids=["gate_off", "gate_on"])
def test_queued_follow_ups_read_the_rotations_with_no_host_step(vislam, frames, gate):
    import torch
    f = frames[gate][:32]
    queued, synced = _f2f_sequence(vislam, torch, f, gate, False), _f2f_sequence(vislam, torch, f, gate, True)
    rec = np.frombuffer(b"".join(synced["f2f"]), vislam.F2F_RESULT_DTYPE)
    nkeep = np.frombuffer(b"".join(synced["nkeep"]), np.int32)
    print(f"\ngate {gate}: F2F count_max {rec['count_max'].tolist()}, kept {nkeep.tolist()}")
    assert (rec["count_max"] > 0).sum() >= 16 and (nkeep > 0).sum() >= 8                    # not a comparison of empty records
    for name in synced:
        for k in range(4):
            assert queued[name][k] == synced[name][k], (name, k)


def _guided_sequence(vislam, torch, f, from_device):
    """two guided launches of 8, gate off: the rotations from vis_imu_preintegrate_rows queued ahead on the context's stream, or from the host"""
    s = Stream(vislam, torch, f, False, 8)
    carry = [_guarded(torch, 232), _guarded(torch, 232)]
    got, host_carry = [], None
    for k in range(2):
        prev = ic.pairing("chain", 8, ir.KF_CARRIED if k else ir.KF_FIRST)
        tf = TFRAME[8 * k:8 * k + 8]
        delta, rot = s.buffers(8)
        if from_device:
            d_prev = _dev(torch, prev)
            s.c.imu_preintegrate_rows(8, s.s.data_ptr(), len(SAMPLES), s.tf.data_ptr() + 64 * k, d_prev.data_ptr(), delta.data_ptr() + GUARD, rot.data_ptr() + GUARD,
                                      carry[k ^ 1].data_ptr() + GUARD if k else 0, carry[k].data_ptr() + GUARD, ip=s.ip)
            d_rot = rot
        else:
            want = ir.preintegrate_rows(P, SAMPLES, tf, prev, host_carry)
            host_carry = want[2]
            d_rot = _guarded(torch, 8 * 36)
            d_rot[GUARD:GUARD + 8 * 36] = torch.from_numpy(want[1].reshape(-1).view(np.uint8).copy()).cuda()
            torch.cuda.synchronize()
        s.c.batch_run_guided(s.dev.data_ptr() + 8 * k * W * H, 8, d_rot.data_ptr() + GUARD, 24.0)
        pose, good, ng = s.c.batch_results(8)
        lists = b"".join(good[i, :int(ng[i])].tobytes() for i in range(8))     # (a list's entries behind its count are not written)
        got.append((pose.tobytes(), lists, ng.tobytes(), _payload(d_rot, 8 * 36).tobytes(), ng.copy()))
    s.close()
    return got


def test_rows_feed_the_guided_run_on_the_context_stream(vislam, frames):
    import torch
    dev, host = _guided_sequence(vislam, torch, frames[False][:16], True), _guided_sequence(vislam, torch, frames[False][:16], False)
    print(f"\nguided matches per pair: {[int(x) for k in range(2) for x in host[k][4]]}")
    assert sum(int((host[k][4] > 0).sum()) for k in range(2)) >= 12  # not a comparison of empty lists; pair 0 of launch 1 is the carried pair
    assert int(host[1][4][0]) > 0
    for k in range(2):
        for j in range(4):
            assert dev[k][j] == host[k][j], (k, j)


def test_run_directory_writes_the_pair_deltas(vislam, frames, tmp_path):
    """tools/run_directory.py --imu --imu-out: the CSV holds what the plan form gives for the same frames in the same batches with the samples and
    frame times the tool derives from the files, the carry continuing across the batches"""
    import json
    import os
    import subprocess
    import sys

    import torch
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
    csv = tmp_path / "imu_out.csv"
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(root, "tools", "run_directory.py"), str(d), "--batch", str(nb),
                        "--imu", str(imu), "--imu-out", str(csv)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    j = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    got = [l.split(",") for l in csv.read_text().splitlines()]
    samples = np.zeros(len(rows), ir.SAMPLE_DTYPE)
    for k, row in enumerate(rows):
        samples[k]["t"], samples[k]["w"], samples[k]["a"] = (row[0] - base) * 1e-9, row[1:4], row[4:7]
    tf = np.asarray([(t - base) * 1e-9 for t in stamps], np.float64)
    p = vislam.default_params()                                    # the tool's parameters: ORB::create(200), fy = fx
    p.fy, p.nfeatures, p.w_size, p.h_size = p.fx, 200, W, H
    c = vislam.Context(0, p)
    c.batch_plan(W, H, W, nb)
    dev, d_s, d_t = _dev(torch, f), _dev(torch, samples), _dev(torch, tf)
    want = []
    for first in range(0, n, nb):
        delta = _guarded(torch, nb * 216)
        c.batch_run(dev.data_ptr() + first * W * H, nb, vislam.STAGE_FRAME)
        c.batch_imu(nb, d_s.data_ptr(), len(samples), d_t.data_ptr() + 8 * first, delta.data_ptr() + GUARD)
        c.batch_sync()
        want += list(_payload(delta, nb * 216).view(ir.DELTA_DTYPE).copy())
    c.close()
    assert len(got) == n and j["imu_csv"] == str(csv) and j["imu"] == {"paired": n - 1, "flagged": 0, "samples": 160}
    for i, (row, w) in enumerate(zip(got, want)):
        assert [int(v) for v in row[:5]] == [i, stamps[i], int(w["flags"]), int(w["q"]), int(w["n_steps"])], i
        assert [float(v) for v in row[5:]] == [float(w["dt"])] + [float(v) for k in ("R", "v", "p") for v in w[k]], i
    assert int(want[6]["flags"]) == 0 and int(want[6]["q"]) == ir.KF_CARRIED and int(want[6]["n_steps"]) == 11      # the pair across the batches
