"""GPU: the bias Jacobians and the correction as a stream, through vis_batch_run on the 37 small synthetic frames of tests/ftrack_stream_cases.py
with a 200 Hz IMU beside them, keyframe gate off and on.

a. Per launch: vis_batch_imu_jac against vis_imu_preintegrate_jac_rows fed with vis_batch_get_keyframes' pairing and the carry so far, BYTE FOR BYTE,
   and both against the restatement; vis_batch_imu of the same run still writes its own bytes, which are the Jacobian variant's delta rows.
b. Cuts A - D of the stream against each other.  Gate off: the same bytes.  Gate on: each block within 16 x the bound tests/test_imu_jac_ref.py measured
   between the lifting table and the left-to-right order, relative to the block's largest entry; flags equal.
c. The call repeated within a run gives the same bytes; a launch that was not integrated makes the carried pair VIS_IMU_NO_CARRY; vis_batch_reset and
   vis_batch_plan forget the carry; vis_batch_imu_jac_init sets it.
d. The chain vis_batch_imu_jac -> vis_batch_vi_align -> vis_batch_imu_correct -> vis_batch_vi_align queued with no wait equals the same steps
   synchronised one by one with the records taken through the host, byte for byte, and the restatement's.
Every output sits between 0xEE guards or is followed by 0xEE bytes that must stay."""
import numpy as np
import pytest

import ftrack_ref as fr
import ftrack_stream_cases as sc
import imu_cases as ic
import imu_jac_ref as jr
import imu_ref as ir
import test_imu_stream_gpu as ti
import test_trajectory_stream_gpu as ts
import test_vi_align_stream_gpu as tv
import vi_align_ref as vr
from test_imu_gpu import GUARD, _guarded, _payload
from test_imu_jac_gpu import jac_rows_on_device
from test_imu_jac_ref import LIFT_BOUND, jc

pytestmark = pytest.mark.gpu
W, H, N = sc.W, sc.H, sc.N
P, SAMPLES, TFRAME = ti.P, ti.SAMPLES, ti.TFRAME
FILL = ts.FILL


class Stream(ti.Stream):
    """test_imu_stream_gpu's stream with the Jacobian variant beside vis_batch_imu: carries of its own on both sides"""

    def forget(self):
        super().forget()
        self.jcarry = None

    def jbuffers(self, n):
        return _guarded(self.torch, n * 216), _guarded(self.torch, n * 296), _guarded(self.torch, n * 36)

    def imu_jac(self, b):
        self.c.batch_imu_jac(self.n, self.s.data_ptr(), len(SAMPLES), self.tf.data_ptr() + 8 * self.at, b[0].data_ptr() + GUARD, b[1].data_ptr() + GUARD,
                             b[2].data_ptr() + GUARD, self.ip)

    def check_jac(self, b, where):
        n = self.n
        self.c.batch_sync()
        assert self.c.batch_status() == 0
        delta, jac, rot = _payload(b[0], n * 216).view(ir.DELTA_DTYPE), _payload(b[1], n * 296).view(jr.JAC_DTYPE), _payload(b[2], n * 36).view(np.float32).reshape(n, 9)
        prev = self.c.batch_get_keyframes()
        tf = TFRAME[self.at:self.at + n]
        want = jr.preintegrate_jac_rows(P, SAMPLES, tf, prev, self.jcarry)
        assert delta.tobytes() == want[0].tobytes(), (where, [i for i in range(n) if delta[i].tobytes() != want[0][i].tobytes()], prev)
        assert jac.tobytes() == want[1].tobytes(), (where, [i for i in range(n) if jac[i].tobytes() != want[1][i].tobytes()], prev)
        assert rot.tobytes() == want[2].tobytes(), where
        rows = jac_rows_on_device(self.v, self.c, P, SAMPLES, tf, prev, self.jcarry)
        assert rows[0].tobytes() == delta.tobytes() and rows[1].tobytes() == jac.tobytes() and rows[2].tobytes() == rot.tobytes(), where
        assert rows[3].tobytes() == want[3].tobytes(), where
        return dict(delta=delta.copy(), jac=jac.copy(), rot=rot.copy(), prev=prev, jcarry=want[3])

    def step(self, n, where, plain=True):
        bj, b = self.jbuffers(n), self.buffers(n)
        self.run(n)
        self.imu_jac(bj)
        if plain:
            self.imu(b)
        gj = self.check_jac(bj, where)
        if plain:                                                     # vis_batch_imu of the same run: its own bytes, the variant's delta rows
            g = self.check(b, where)
            assert g["delta"].tobytes() == gj["delta"].tobytes() and g["rot"].tobytes() == gj["rot"].tobytes(), where
            assert g["carry"].tobytes() == gj["jcarry"]["carry"].tobytes(), where
            gj["carry"] = g["carry"]
        else:
            gj["carry"] = None
        self.jcarry = gj["jcarry"]
        self.advance(gj, integrated=plain)
        return gj


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


@pytest.mark.parametrize("gate", [False, True], ids=["gate_off", "gate_on"])
def test_cuts_of_the_stream(vislam, frames, gate):
    import torch
    streams = {B: Stream(vislam, torch, frames[gate][:N], gate, B) for B in sorted(set(sc.PLAN_B.values()))}
    out = {}
    for name, cut in sc.CUTS.items():
        s = streams[sc.PLAN_B[name]]
        s.c.batch_reset()
        s.forget()
        gs = [s.step(n, (name, k)) for k, n in enumerate(cut)]
        out[name] = (np.concatenate([g["delta"] for g in gs]), np.concatenate([g["jac"] for g in gs]))
    for s in streams.values():
        s.close()
    delta, jac = out["B"]                                             # one launch: the stream as a whole
    paired = ~(delta["flags"] & (ir.IMU_NO_PAIR | ir.IMU_NO_CARRY)).astype(bool)
    assert paired.sum() >= 25 and not jac["flags"].any()
    for f in jr.BLOCKS:
        assert (np.abs(jac[f][paired]).max(axis=1) > 0).all() and not jac[f][~paired].any(), f      # not a comparison of zeros
    for name in sc.CUTS:
        d, j = out[name]
        assert (d["flags"] == delta["flags"]).all() and (j["flags"] == jac["flags"]).all(), name
        for f in jr.BLOCKS:
            if not gate:
                assert j[f].tobytes() == jac[f].tobytes(), (name, f)
            else:
                scale = np.abs(jac[f]).max(axis=1, keepdims=True)
                assert (np.abs(j[f] - jac[f]) <= LIFT_BOUND[f] * scale).all(), (name, f)


@pytest.mark.parametrize("gate", [False, True], ids=["gate_off", "gate_on"])
def test_call_patterns(vislam, frames, gate):
    """cut C: the call twice per run; launch 1 of 5 not integrated; a reset before the last launch; then a new plan, and vis_batch_imu_jac_init"""
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
            s.jcarry = None
            s.advance(dict(prev=s.c.batch_get_keyframes()), integrated=False)
            continue
        b1, b2 = s.jbuffers(n), s.jbuffers(n)
        s.imu_jac(b1)
        s.imu_jac(b2)
        g1, g2 = s.check_jac(b1, ("first", k)), s.check_jac(b2, ("again", k))
        assert all(g1[f].tobytes() == g2[f].tobytes() for f in ("delta", "jac", "rot"))
        carried = [i for i in range(n) if int(g1["prev"][i]) == fr.KF_CARRIED]
        if k == 2:
            assert carried and all(int(g1["delta"][i]["flags"]) == ir.IMU_NO_CARRY and not g1["jac"][i]["Jva"].any() for i in carried)
        if k == 3:
            assert carried and all(int(g1["delta"][i]["flags"]) == 0 and g1["jac"][i]["Jva"].any() for i in carried)
        s.jcarry = g1["jcarry"]
        s.advance(dict(prev=g1["prev"], carry=None), integrated=False)
    s.c.batch_plan(W, H, W, 8)                                       # a new plan forgets the carry
    s.forget()
    g = s.step(8, "after plan", plain=False)
    assert int(g["delta"][0]["flags"]) == ir.IMU_NO_PAIR
    base = ic.carried(float(TFRAME[7]) - 0.004, True)               # vis_batch_imu_jac_init: the next run continues from this record
    rec = jc(base)
    t = float(base[0]["t_last"])
    rec[0]["open_jac"] = jr.preintegrate_jac(ic.params(), ic.samples_between(t - 0.3, t + 0.1, 200.0), t - 0.21, t)[1]
    rec[0]["open_jac"]["q"] = 0
    s.c.batch_imu_jac_init(rec[0])
    s.jcarry = rec
    g = s.step(8, "after init", plain=False)
    first = [i for i in range(8) if int(g["prev"][i]) == fr.KF_CARRIED][0]
    assert int(g["delta"][first]["flags"]) == 0 and int(g["delta"][first]["n_steps"]) > int(base[0]["open"]["n_steps"])
    s.c.batch_imu_jac_init(None)
    s.jcarry = None
    g = s.step(8, "after init(None)", plain=False)
    first = [i for i in range(8) if int(g["prev"][i]) == fr.KF_CARRIED][0]
    assert int(g["delta"][first]["flags"]) == ir.IMU_NO_CARRY
    s.close()


class Chain(tv.Stream):
    """test_vi_align_stream_gpu's stream with the Jacobian variant in vis_batch_imu's place and, behind the alignment, the correction by its dbg and a
    second alignment on the corrected records"""

    def buffers(self, n):
        b = super().buffers(n)
        f = lambda nb: ts._filled(self.torch, nb)
        b.update(jac=f((n + 1) * 296), delta2=f((n + 1) * 216), rot2=f((n + 1) * 36), status=f((n + 1) * 4), state2=f((n + 1) * 64), result2=f(160 + 64))
        return b

    def integrate(self, b):
        ts.Stream.follow(self, b)
        self.c.batch_imu_jac(self.n, self.s.data_ptr(), len(SAMPLES), self.tf.data_ptr() + 8 * self.at, b["delta"].data_ptr(), b["jac"].data_ptr(), 0, self.ip)

    def correct(self, b):
        self.c.batch_imu_correct(self.n, b["delta"].data_ptr(), b["jac"].data_ptr(), b["result"].data_ptr(), b["delta2"].data_ptr(), 0, b["rot2"].data_ptr(),
                                 b["status"].data_ptr(), self.ip)

    def align2(self, b):
        self.c.batch_vi_align(self.n, b["traj"].data_ptr(), b["delta2"].data_ptr(), b["result2"].data_ptr(), b["state2"].data_ptr(), self.vp)


SIZES = dict(traj=128, delta=216, jac=296, state=64, delta2=216, rot2=36, status=4, state2=64)


def _chain(vislam, torch, f, gate, through_host):
    """four launches of 8: run, triangulate, scale links, trajectory, imu with Jacobians, alignment, correction, alignment; buffers of their own"""
    s = Chain(vislam, torch, f, gate, 8)
    bufs = [s.buffers(8) for _ in range(4)]
    prevs = []
    for k in range(4):
        b = bufs[k]
        s.run(8)
        s.integrate(b)
        if not through_host:
            s.align(b)
            s.correct(b)
            s.align2(b)
        else:
            def again(*names):
                s.c.batch_sync()
                t = {name: torch.from_numpy(b[name].cpu().numpy().copy()).cuda() for name in names}
                torch.cuda.synchronize()
                return t
            s.align(dict(b, **again("traj", "delta")))
            s.correct(dict(b, **again("delta", "jac", "result")))
            s.align2(dict(b, **again("traj", "delta2")))
        s.c.batch_sync()
        prevs.append(s.c.batch_get_keyframes())
        s.at += 8
    assert s.c.batch_status() == 0
    got = {name: [b[name].cpu().numpy() for b in bufs] for name in list(SIZES) + ["result", "result2"]}
    s.close()
    return got, prevs


@pytest.mark.parametrize("gate", [False, True], ids=["gate_off", "gate_on"])
def test_the_chain_queued_equals_the_chain_through_the_host(vislam, frames, gate):
    import torch
    f = frames[gate][:32]
    (queued, prevs), (synced, _) = _chain(vislam, torch, f, gate, False), _chain(vislam, torch, f, gate, True)
    for name in synced:
        for k in range(4):
            assert queued[name][k].tobytes() == synced[name][k].tobytes(), (name, k)
            size = 8 * SIZES[name] if name in SIZES else 160
            assert (queued[name][k][size:] == FILL).all(), (name, k)
    # against the restatement: the correction by the first alignment's dbg, and the second alignment from the carry the first one read
    via, corrected = None, 0
    for k in range(4):
        rec = lambda name, dt: queued[name][k][:8 * SIZES[name]].view(dt)
        traj, delta, jac = rec("traj", tv.tj.TRAJ_DTYPE), rec("delta", ir.DELTA_DTYPE), rec("jac", jr.JAC_DTYPE)
        res1 = queued["result"][k][:160].view(vr.RESULT_DTYPE)[0]
        want1 = vr.align_rows(tv.VP, prevs[k], traj, delta, via)
        assert res1.tobytes() == want1[1].tobytes(), k
        d2, rot2, st = jr.correct_rows(tv.IP, delta, jac, np.asarray(res1["dbg"]).reshape(3))
        assert rec("delta2", ir.DELTA_DTYPE).tobytes() == d2.tobytes() and rec("rot2", np.float32).tobytes() == rot2.tobytes(), k
        assert rec("status", np.int32).tobytes() == st.tobytes(), k
        want2 = vr.align_rows(tv.VP, prevs[k], traj, d2, via)
        assert queued["result2"][k][:160].tobytes() == want2[1].tobytes() and rec("state2", vr.STATE_DTYPE).tobytes() == want2[0].tobytes(), k
        via = want2[2]
        corrected += int((st == jr.IMC_OK).sum())
    res = [queued["result2"][k][:160].view(vr.RESULT_DTYPE)[0] for k in range(4)]
    print(f"\ngate {gate}: corrected records {corrected}, pairs {[int(r['n_pairs']) for r in res]}, |dbg| of the first alignments "
          f"{[float(np.abs(queued['result'][k][:24].view(np.float64)).max()) for k in range(4)]}")
    assert corrected >= 8 and int(res[-1]["n_pairs"]) >= 16 and int(res[-1]["n_pairs"]) > int(res[-1]["n_pairs_call"])   # not empty, and carried on


def test_run_directory_closes_the_loop(vislam, frames, tmp_path):
    """tools/run_directory.py --imu --imu-jac --trajectory --vi-align --recorrect: the deltas are those of the run without --imu-jac, one row of
    Jacobians per frame, the second alignment's record and the first one's dbg in the JSON line"""
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
    out = {k: tmp_path / f"out_{k}.csv" for k in ("imu", "plain", "jac", "traj", "via")}    # (not the name of the input file)
    tool = ["timeout", "-k", "10", "240", sys.executable, os.path.join(root, "tools", "run_directory.py"), str(d), "--batch", str(nb), "--imu", str(imu)]
    r = subprocess.run(tool + ["--imu-out", str(out["imu"]), "--imu-jac", str(out["jac"]), "--trajectory", str(out["traj"]), "--vi-align", str(out["via"]),
                               "--recorrect"], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    j = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    r = subprocess.run(tool + ["--imu-out", str(out["plain"])], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    assert out["imu"].read_text() == out["plain"].read_text()         # a Jacobian never changes a delta
    jac, deltas = ([l.split(",") for l in out[k].read_text().splitlines()] for k in ("jac", "imu"))
    assert len(jac) == n and all(len(row) == 40 for row in jac) and j["imu_jac_csv"] == str(out["jac"])
    for i, row in enumerate(jac):
        assert [int(row[0]), int(row[1]), int(row[2])] == [i, stamps[i], 0] and int(row[3]) == int(deltas[i][3])
        paired = not int(deltas[i][2]) & (ir.IMU_NO_PAIR | ir.IMU_NO_CARRY)
        assert any(float(v) != 0.0 for v in row[4:]) == paired and all(np.isfinite(float(v)) for v in row[4:]), i
    rc = j["recorrect"]
    assert rc["corrected_in_the_last_batch"] >= nb - 1 and len(rc["dbg_first"]) == 3 and j["vi_align"]["pairs"] >= 8
    # the second alignment starts from the rotations the first one evaluated its c1 with, R Exp(JRg dbg): the same sum.  (It need not be below the
    # first c0 here: the images and the IMU of this stream are unrelated motions, far outside the step's linear range; one world through the whole
    # chain is tests/test_vi_chain_gpu.py's, row level -- a frame stream of it needs an image generator whose camera accelerates: out of scope.)
    assert any(rc["dbg_first"]) and rc["c0_call"] == pytest.approx(rc["c1_first"], rel=1e-9) and rc["c0_call"] != rc["c0_call_first"]
    r = subprocess.run(tool + ["--imu-out", str(out["plain"]), "--recorrect"], capture_output=True, text=True)
    assert r.returncode != 0 and "--recorrect needs --vi-align and --imu-jac" in r.stderr
