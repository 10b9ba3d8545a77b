"""GPU: the alignment with the accelerometer bias as a stream, through vis_batch_run on the 37 small synthetic frames of tests/ftrack_stream_cases.py
with the 200 Hz IMU of tests/imu_cases.py beside them, keyframe gate off and on.  (The synthetic images and the synthetic IMU are unrelated motions:
the solution is flagged or meaningless, which is part of what is compared -- the planted motion is tests/test_vi_align_ba_gpu.py's, and
the chain from pixels to the biases on ONE world is tests/test_vi_chain_gpu.py's, row level: a frame-stream version needs an image generator whose
camera accelerates -- these frames move at constant velocity, which never excites the alignment -- and is out of scope.)

a. Per launch: vis_batch_vi_align_ba behind triangulate -> scale links -> trajectory -> imu_jac, beside vis_batch_vi_align of the same run, whose
   records stay its own (test_vi_align_stream_gpu's check) and are the embedded record; against vis_vi_align_ba_rows fed with the downloaded records,
   vis_batch_get_keyframes' pairing and the carry so far, BYTE FOR BYTE, and both against the restatement.
b. Cuts A - D: each cut's carried bias sums against the restatement's over the cut's own records taken as ONE call, within CUT_BOUND of
   tests/test_vi_align_ba_ref.py relative to the summed absolute terms; the counts exactly, there and between the cuts.
c. A call repeated within a run gives the same bytes; a launch that was not aligned leaves the next one without a carry; vis_batch_reset and
   vis_batch_plan forget the carry; vis_batch_vi_align_ba_init sets it.
d. The chain imu_jac -> align_ba -> correct(d_result, &d_result->dba) -> align_ba queued with no wait equals the same steps synchronised one by one with
   the records taken through the host, byte for byte, and the restatement's.
Output buffers are pre-filled with 0xEE and everything behind the written extent must keep it."""
import numpy as np
import pytest

import ftrack_stream_cases as sc
import imu_jac_ref as jr
import imu_ref as ir
import test_imu_jac_stream_gpu as tjs
import test_trajectory_stream_gpu as ts
import test_vi_align_stream_gpu as tv
import trajectory_ref as tj
import vi_align_ba_cases as bc
import vi_align_ba_ref as br
import vi_align_ref as vr
from test_vi_align_ba_gpu import ba_rows_on_device, struct_ba_params
from test_vi_align_ba_ref import CUT_BOUND

pytestmark = pytest.mark.gpu
FILL = ts.FILL
W, H, N = sc.W, sc.H, sc.N
VP, IP = tv.VP, tv.IP
BP = br.BaParams(min_ba_triples=3)
frames = tv.frames                                                     # (the fixture)


class Stream(tjs.Chain):
    """test_imu_jac_stream_gpu's chain (trajectory, imu with Jacobians, alignment, correction, second alignment) with vis_batch_vi_align_ba and the
    carry its next launch continues"""

    def __init__(self, vislam, torch, frames, gate, B):
        super().__init__(vislam, torch, frames, gate, B)
        self.bp = struct_ba_params(vislam, BP)

    def forget(self):
        super().forget()
        self.viab = None

    def buffers(self, n):
        b = super().buffers(n)
        f = lambda nb: ts._filled(self.torch, nb)
        b.update(state_ba=f((n + 1) * 64), result_ba=f(304 + 64), state_ba2=f((n + 1) * 64), result_ba2=f(304 + 64))
        return b

    def align_ba(self, b, delta="delta", out=""):
        self.c.batch_vi_align_ba(self.n, b["traj"].data_ptr(), b[delta].data_ptr(), b["jac"].data_ptr(), b["result_ba" + out].data_ptr(),
                                 b["state_ba" + out].data_ptr(), self.vp, self.bp)

    def correct_ba(self, b):
        r = b["result_ba"].data_ptr()
        self.c.batch_imu_correct(self.n, b["delta"].data_ptr(), b["jac"].data_ptr(), r, b["delta2"].data_ptr(), r + self.v.VI_ALIGN_BA_DBA_OFFSET,
                                 b["rot2"].data_ptr(), b["status"].data_ptr(), self.ip)

    def ba_records(self, b, out=""):
        n = self.n
        self.c.batch_sync()
        raw = {k: b[k + out].cpu().numpy() for k in ("state_ba", "result_ba")}
        jac = b["jac"].cpu().numpy()
        assert (raw["state_ba"][n * 64:] == FILL).all() and (raw["result_ba"][304:] == FILL).all() and (jac[n * 296:] == FILL).all()
        return raw["state_ba"][:n * 64].view(vr.STATE_DTYPE).copy(), raw["result_ba"][:304].view(br.BA_RESULT_DTYPE)[0].copy(), jac[:n * 296].view(jr.JAC_DTYPE).copy()

    def check_ba(self, b, where, sibling=True):
        """both alignments of the launch: the sibling's records by test_vi_align_stream_gpu's check, this call's against the restatement and the rows form"""
        g = tv.Stream.check(self, b, where) if sibling else tv.Stream.records(self, b)
        st, res, jac = self.ba_records(b)
        want = br.align_ba_rows(VP, BP, g["prev"], g["traj"], g["delta"], jac, self.viab)
        assert res.tobytes() == want[1].tobytes(), (where, res, want[1])
        assert st.tobytes() == want[0].tobytes(), (where, [i for i in range(self.n) if st[i].tobytes() != want[0][i].tobytes()])
        rows = ba_rows_on_device(self.v, self.c, VP, BP, g["prev"], g["traj"], g["delta"], jac, self.viab)
        assert rows[0].tobytes() == st.tobytes() and rows[1].tobytes() == res.tobytes() and rows[2].tobytes() == want[2].tobytes(), where
        if sibling and (self.viab is None) == (self.via is None):      # the embedded record is vis_batch_vi_align's of the same run
            assert res["a"].tobytes() == g["result"].tobytes(), where
        assert bc.all_finite(*want), where
        g.update(jac=jac, state_ba=st, result_ba=res, carry_ba=want[2])
        return g

    def advance(self, g, aligned=True):
        self.viab = g["carry_ba"] if aligned else None
        if "carry" not in g:
            g["carry"] = None
        super().advance(g, aligned and g["carry"] is not None)

    def step(self, n, where):
        b = self.buffers(n)
        self.run(n)
        self.integrate(b)
        self.align(b)
        self.align_ba(b)
        g = self.check_ba(b, where)
        self.advance(g)
        return g


def as_one_call(gs):
    gprev, traj, delta = tv.as_one_call(gs)
    jac = np.concatenate([g["jac"] for g in gs])
    jac["q"] = gprev
    return gprev, traj, delta, jac


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
        _, res, co = br.align_ba_rows(VP, BP, *as_one_call(gs), detail=scale)
        got, carry = gs[-1]["result_ba"], gs[-1]["carry_ba"]
        assert int(got["n_ba_triples"]) == int(res["n_ba_triples"]), name
        d = float((np.abs(carry[0]["ba"] - co[0]["ba"]) / np.maximum(scale["ba"], 1e-300)).max())
        print(f"\ngate {gate}, cut {name}: {int(got['n_ba_triples'])} bias triples, ba_flags {int(got['ba_flags'])}, sums differ by {d:.2e}")
        assert d <= CUT_BOUND["ba"], (name, d)
        last[name] = got
    for s in streams.values():
        s.close()
    assert int(last["B"]["n_ba_triples"]) >= 3                          # not a comparison of empty sums
    for name in sc.CUTS:
        assert int(last[name]["n_ba_triples"]) == int(last["B"]["n_ba_triples"]), name


@pytest.mark.parametrize("gate", [False, True], ids=["gate_off", "gate_on"])
def test_call_patterns(vislam, frames, gate):
    """cut C: the call twice per run; launch 1 of 5 not aligned; a reset before the last launch; then a new plan, and vis_batch_vi_align_ba_init"""
    import torch
    s = Stream(vislam, torch, frames[gate][:N], gate, 8)
    for k, n in enumerate(sc.CUTS["C"]):
        if k == 4:
            s.c.batch_reset()
            s.forget()
        b = s.buffers(n)
        s.run(n)
        s.integrate(b)
        if k == 1:                                                   # not aligned: the next launch has no carry
            g = tv.Stream.records(s, b)
            assert (b["result_ba"].cpu().numpy() == FILL).all()
            s.advance(dict(prev=g["prev"], carry_ba=None), aligned=False)
            continue
        s.align_ba(b)
        s.align_ba(b, out="2")
        g = s.check_ba(b, ("first", k), sibling=False)
        st2, res2, _ = s.ba_records(b, "2")
        assert st2.tobytes() == g["state_ba"].tobytes() and res2.tobytes() == g["result_ba"].tobytes(), k
        if k in (2, 4):
            assert int(res2["a"]["n_pairs"]) == int(res2["a"]["n_pairs_call"]) and int(res2["n_ba_triples"]) == int(res2["n_ba_triples_call"])
        if k == 3:
            assert int(res2["a"]["n_pairs"]) > int(res2["a"]["n_pairs_call"])
        s.advance(g)
    s.c.batch_plan(W, H, W, 8)                                       # a new plan forgets the carry
    s.forget()
    s.at = 0

    def one(where):
        b = s.buffers(8)
        s.run(8)
        s.integrate(b)
        s.align_ba(b)
        g = s.check_ba(b, where, sibling=False)
        s.advance(g)
        return g["result_ba"]
    res = one("after plan")
    assert int(res["a"]["n_pairs"]) == int(res["a"]["n_pairs_call"])
    rec = bc.scene(8, "chain", "sums")["carry"]                     # vis_batch_vi_align_ba_init: the next run continues from this record
    s.c.batch_vi_align_ba_init(rec[0])
    s.viab = rec
    res = one("after init")
    assert int(res["a"]["n_pairs"]) == int(res["a"]["n_pairs_call"]) + int(rec[0]["carry"]["n_pairs"])
    s.c.batch_vi_align_ba_init(None)
    s.viab = None
    res = one("after init(None)")
    assert int(res["a"]["n_pairs"]) == int(res["a"]["n_pairs_call"])
    s.close()


SIZES = dict(traj=128, delta=216, jac=296, state_ba=64, delta2=216, rot2=36, status=4, state_ba2=64, result_ba=304, result_ba2=304)


def _chain(vislam, torch, f, gate, through_host):
    """four launches of 8: run, triangulate, scale links, trajectory, imu with Jacobians, align_ba, correction by (dbg, dba), align_ba"""
    s = Stream(vislam, torch, f, gate, 8)
    bufs = [s.buffers(8) for _ in range(4)]
    prevs = []
    for k in range(4):
        b = bufs[k]
        s.run(8)
        s.integrate(b)
        if not through_host:
            s.align_ba(b)
            s.correct_ba(b)
            s.align_ba(b, delta="delta2", out="2")
        else:
            def again(*names):
                s.c.batch_sync()
                t = {name: torch.from_numpy(b[name].cpu().numpy().copy()).cuda() for name in names}
                torch.cuda.synchronize()
                return t
            s.align_ba(dict(b, **again("traj", "delta", "jac")))
            s.correct_ba(dict(b, **again("delta", "jac", "result_ba")))
            s.align_ba(dict(b, **again("traj", "delta2", "jac")), delta="delta2", out="2")
        s.c.batch_sync()
        prevs.append(s.c.batch_get_keyframes())
        s.at += 8
    assert s.c.batch_status() == 0
    got = {name: [b[name].cpu().numpy() for b in bufs] for name in SIZES}
    s.close()
    return got, prevs


@pytest.mark.parametrize("gate", [False, True], ids=["gate_off", "gate_on"])
def test_the_chain_queued_equals_the_chain_through_the_host(vislam, frames, gate):
    import torch
    f = frames[gate][:32]
    (queued, prevs), (synced, _) = _chain(vislam, torch, f, gate, False), _chain(vislam, torch, f, gate, True)
    size = lambda name: SIZES[name] * (1 if name.startswith("result") else 8)
    for name in synced:
        for k in range(4):
            assert queued[name][k].tobytes() == synced[name][k].tobytes(), (name, k)
            assert (queued[name][k][size(name):] == FILL).all(), (name, k)
    # against the restatement: the correction by the first alignment's dbg AND dba, the second alignment from the carry the first one read
    viab, corrected, flags = None, 0, []
    for k in range(4):
        rec = lambda name, dt: queued[name][k][:size(name)].view(dt)
        traj, delta, jac = rec("traj", tj.TRAJ_DTYPE), rec("delta", ir.DELTA_DTYPE), rec("jac", jr.JAC_DTYPE)
        res1 = rec("result_ba", br.BA_RESULT_DTYPE)[0]
        want1 = br.align_ba_rows(VP, BP, prevs[k], traj, delta, jac, viab)
        assert res1.tobytes() == want1[1].tobytes() and rec("state_ba", vr.STATE_DTYPE).tobytes() == want1[0].tobytes(), k
        d2, rot2, st = jr.correct_rows(IP, delta, jac, np.asarray(res1["a"]["dbg"]).reshape(3), np.asarray(res1["dba"]).reshape(3))
        assert rec("delta2", ir.DELTA_DTYPE).tobytes() == d2.tobytes() and rec("rot2", np.float32).tobytes() == rot2.tobytes(), k
        assert rec("status", np.int32).tobytes() == st.tobytes(), k
        want2 = br.align_ba_rows(VP, BP, prevs[k], traj, d2, jac, viab)
        assert rec("result_ba2", br.BA_RESULT_DTYPE)[0].tobytes() == want2[1].tobytes() and rec("state_ba2", vr.STATE_DTYPE).tobytes() == want2[0].tobytes(), k
        viab = want2[2]
        corrected += int((st == jr.IMC_OK).sum())
        flags.append((int(res1["ba_flags"]), int(want2[1]["ba_flags"])))
    last = queued["result_ba2"][3][:304].view(br.BA_RESULT_DTYPE)[0]
    print(f"\ngate {gate}: corrected records {corrected}, ba_flags {flags}, bias triples {int(last['n_ba_triples'])}, pairs {int(last['a']['n_pairs'])}")
    assert corrected >= 8 and int(last["a"]["n_pairs"]) >= 16 and int(last["a"]["n_pairs"]) > int(last["a"]["n_pairs_call"])   # not empty, and carried on


def test_run_directory_writes_the_states_under_the_bias(vislam, frames, tmp_path):
    """tools/run_directory.py --imu --imu-jac --trajectory --vi-align-ba [--recorrect]: one state per frame, the last batch's record in the JSON line;
    --recorrect passes dbg and dba of the first alignment to the correction"""
    import json
    import os
    import subprocess
    import sys
    import imu_cases as ic
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
    out = {k: tmp_path / f"out_{k}.csv" for k in ("imu", "jac", "traj", "viab")}
    tool = ["timeout", "-k", "10", "240", sys.executable, os.path.join(root, "tools", "run_directory.py"), str(d), "--batch", str(nb), "--imu", str(imu)]
    r = subprocess.run(tool + ["--imu-out", str(out["imu"]), "--imu-jac", str(out["jac"]), "--trajectory", str(out["traj"]), "--vi-align-ba", str(out["viab"]),
                               "--recorrect"], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    j = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    got = [l.split(",") for l in out["viab"].read_text().splitlines()]
    assert len(got) == n and all(len(row) == 11 for row in got) and j["vi_align_ba_csv"] == str(out["viab"])
    for i, row in enumerate(got):
        assert [int(row[0]), int(row[1])] == [i, stamps[i]] and all(np.isfinite(float(v)) for v in row[4:])
    ba = j["vi_align_ba"]
    assert len(ba["dba"]) == 3 and len(ba["g_ba"]) == 3 and ba["pairs"] >= 8 and "ba_flags" in ba and all(np.isfinite(ba["dba"]))
    assert len(j["recorrect"]["dba_first"]) == 3 and len(j["recorrect"]["dbg_first"]) == 3
    r = subprocess.run(tool + ["--imu-out", str(out["imu"]), "--trajectory", str(out["traj"]), "--vi-align-ba", str(out["viab"])], capture_output=True, text=True)
    assert r.returncode != 0 and "--vi-align-ba needs --imu-jac and --trajectory" in r.stderr
