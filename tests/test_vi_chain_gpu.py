"""GPU: the chain of tests/vi_chain_cases.py on the device, every hand-over a DEVICE pointer to the buffer the call before wrote:
vis_essential_batch -> vis_essential_polish_batch (its d_pose_out and d_mask_out are the record and the mask fed on) -> vis_triangulate per pair ->
vis_scale_link_rows -> vis_trajectory_rows -> vis_imu_preintegrate_jac_rows -> vis_vi_align_ba_rows -> vis_imu_correct_rows(d_dbg = d_result, d_dba =
&d_result->dba) -> vis_vi_align_ba_rows, for the five scenarios (the two calls of `cut` and `lost` with every carry a pointer into the first call's
buffers).  vis_triangulate is a host-pointer call and rows have no device form of it: the chain waits once in front of it to read the pose records
and uploads its points; everything behind it is queued on the context's stream with ONE vis_batch_sync at the end.

a. The pose stage against the CPU oracle within test_pose_gpu's stated tolerance (E sign-normalised, R, t 1e-9; mask and counts identical): that
   stage is pinned to the oracle within a tolerance, not byte for byte.
b. Every stage behind it against the CPU chain (the restatements) fed with THE DEVICE'S OWN pose-stage records, BYTE FOR BYTE, in the chain's
   order: the first stage that differs is named.
c. The final records against the planted truth within 4 x test_vi_chain_ref.MEASURED -- the CPU chain's errors, never the device's --, and the
   conditions of test_vi_chain_ref on the device's records.
d. The queued chain equals the same calls synchronised one by one, byte for byte; `cut` against `chain` within the stages' documented bounds.
Every output sits between 0xEE guards that must keep their bytes."""
import numpy as np
import pytest

import essential_polish_ref as epr
import imu_cases as ic
import imu_jac_ref as jr
import imu_ref as ir
import scale_link_ref as sl
import trajectory_ref as tj
import vi_align_ba_ref as br
import vi_align_cases as vc
import vi_align_ref as vr
import vi_chain_cases as cc
from test_pose_gpu import TOL, _cmpE
from test_vi_align_ba_gpu import struct_ba_params
from test_vi_chain_ref import MEASURED, compare_cut_with_chain, conditions

pytestmark = pytest.mark.gpu
FILL, GUARD = cc.FILL, 64
DTYPES = dict(pose0=sl.POSE_DTYPE, mask0=np.uint8, polish=epr.RESULT_DTYPE, pose=sl.POSE_DTYPE, mask=np.uint8, points=sl.MAP_POINT_DTYPE, flags=np.uint8,
              depth=np.float64, link=sl.LINK_DTYPE, traj=tj.TRAJ_DTYPE, delta=ir.DELTA_DTYPE, jac=jr.JAC_DTYPE, imu_carry=jr.JAC_CARRY_DTYPE,
              state1=vr.STATE_DTYPE, res1=br.BA_RESULT_DTYPE, ba_carry1=br.BA_CARRY_DTYPE, delta2=ir.DELTA_DTYPE, status=np.int32, state2=vr.STATE_DTYPE,
              res2=br.BA_RESULT_DTYPE, ba_carry2=br.BA_CARRY_DTYPE)
ROWS = dict(mask0=cc.MAX_PTS, mask=cc.MAX_PTS, points=cc.MAX_PTS, flags=cc.MAX_PTS, depth=cc.ROW_CAP)       # entries per frame of the 2-D stages
SCALARS = ("res1", "res2")


class Buf:
    """a device buffer, or a part of one: ptr is what a call gets; an output lies between two guards"""

    def __init__(self, t, nbytes, guard=0, at=0):
        self.t, self.nbytes, self.guard, self.ptr = t, nbytes, guard, t.data_ptr() + guard + at

    def host(self):
        h = self.t.cpu().numpy()
        g = self.guard
        assert (h[:g] == FILL).all() and (h[g + self.nbytes:] == FILL).all(), "a guard was written"
        return h[g:g + self.nbytes].copy()


class Dev:
    """the stages by the library's bindings on device pointers.  each: synchronise behind every call (what the queued chain must equal)"""

    def __init__(self, vislam, torch, c, each=False):
        self.v, self.torch, self.c, self.each = vislam, torch, c, each
        self.vp, self.bp, self.ip = vc.struct_params(vislam, cc.VP), struct_ba_params(vislam, cc.BP), ic.struct_params(vislam, cc.IP)
        self.keep = []

    def upload(self, a):
        a = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
        t = self.torch.from_numpy(a if len(a) else np.zeros(8, np.uint8)).cuda()
        self.torch.cuda.synchronize()
        self.keep.append(t)
        return Buf(t, len(a))

    def out(self, nbytes):
        t = self.torch.full((nbytes + 2 * GUARD,), FILL, dtype=self.torch.uint8, device="cuda")
        self.torch.cuda.synchronize()                                 # (the fill ran on torch's stream: finished before the library's stream writes)
        return Buf(t, nbytes, GUARD)

    def part(self, h, i, nbytes):
        return Buf(h.t, nbytes, 0, h.guard + i * nbytes)

    def sync(self):
        self.c.batch_sync()

    def done(self):
        if self.each:
            self.sync()

    def fetch(self, h):
        return h.host()

    def essential(self, p1, p2, npts):
        n = len(npts)
        self.rows = self.upload(p1), self.upload(p2), self.upload(npts)
        pose, mask = self.out(n * 192), self.out(n * cc.MAX_PTS)
        self.c.essential_batch(n, self.rows[0].ptr, self.rows[1].ptr, self.rows[2].ptr, cc.MAX_PTS, cc.MAX_PTS, mask.ptr, pose.ptr)
        self.done()
        return pose, mask

    def polish(self, pose, mask, p1, p2, npts):
        n = len(npts)
        out, po, mo = self.out(n * 224), self.out(n * 192), self.out(n * cc.MAX_PTS)
        self.c.essential_polish_batch(n, pose.ptr, self.rows[0].ptr, self.rows[1].ptr, self.rows[2].ptr, cc.MAX_PTS, cc.MAX_PTS, mask.ptr, mo.ptr, out.ptr, po.ptr)
        self.done()
        return out, po, mo

    def triangulate(self, pose, mask, p1, p2, npts):
        """the host step: the pose records and masks come down, the points go up"""
        self.sync()
        n = len(npts)
        rec, mk = pose.host().view(sl.POSE_DTYPE), mask.host().reshape(n, cc.MAX_PTS)
        pts, fl = np.zeros((n, cc.MAX_PTS), sl.MAP_POINT_DTYPE), np.zeros((n, cc.MAX_PTS), np.uint8)
        for i in range(n):
            m = int(npts[i])
            if m and rec[i]["R"].any():
                pts[i, :m], fl[i, :m], _ = self.c.triangulate(rec[i]["R"], rec[i]["t"], p1[i, :m], p2[i, :m], mk[i, :m])
        return self.upload(pts), self.upload(fl)

    def scale_link(self, prev, links, nlinks, pose, points, flags, carry, n):
        d_links, d_n = self.upload(links), self.upload(nlinks)
        depth, link = self.out(n * cc.ROW_CAP * 8), self.out(n * 40)
        self.c.scale_link_rows(n, prev.ptr, d_links.ptr, d_n.ptr, cc.MAX_PTS, pose.ptr, points.ptr, flags.ptr, cc.MAX_PTS, cc.ROW_CAP, depth.ptr, link.ptr,
                               carry.ptr if carry is not None else 0)
        self.done()
        return depth, link

    def trajectory(self, prev, pose, link, carry, seq0, n):
        traj = self.out(n * 128)
        self.c.trajectory_rows(n, prev.ptr, pose.ptr, link.ptr, traj.ptr, 0, carry.ptr if carry is not None else 0, seq0)
        self.done()
        return traj

    def imu(self, samples, tframe, prev, carry, n):
        d_s, d_t = self.upload(samples), self.upload(tframe)
        delta, jac, out = self.out(n * 216), self.out(n * 296), self.out(528)
        self.c.imu_preintegrate_jac_rows(n, d_s.ptr, len(samples), d_t.ptr, prev.ptr, delta.ptr, jac.ptr, 0, carry.ptr if carry is not None else 0, out.ptr, self.ip)
        self.done()
        return delta, jac, out

    def align(self, prev, traj, delta, jac, carry, n):
        state, res, out = self.out(n * 64), self.out(304), self.out(1280)
        self.c.vi_align_ba_rows(n, prev.ptr, traj.ptr, delta.ptr, jac.ptr, res.ptr, state.ptr, carry.ptr if carry is not None else 0, out.ptr, self.vp, self.bp)
        self.done()
        return state, res, out

    def correct(self, delta, jac, res, n):
        out, status = self.out(n * 216), self.out(n * 4)
        self.c.imu_correct_rows(n, delta.ptr, jac.ptr, res.ptr, out.ptr, res.ptr + self.v.VI_ALIGN_BA_DBA_OFFSET, 0, status.ptr, self.ip)
        self.done()
        return out, status


def shaped(recs):
    """the downloaded bytes of every call as the records the CPU chain returns"""
    out = []
    for r in recs:
        s = dict(r)
        for k, dt in DTYPES.items():
            a = r[k].view(dt)
            s[k] = a.reshape(r["n"], ROWS[k]) if k in ROWS else (a[0] if k in SCALARS else a)
        out.append(s)
    return out


@pytest.fixture(scope="module")
def chains(vislam):
    """the device's records of a scenario, queued or synchronised call by call -- run once each"""
    import torch
    c = vislam.Context(0, cc.camera())
    got = {}

    def of(name, each=False):
        if (name, each) not in got:
            be = Dev(vislam, torch, c, each)
            calls = cc.run_chain(be, cc.scenario(name))
            be.sync()
            got[name, each] = shaped(cc.records(be, calls))
        return got[name, each]
    yield of
    c.close()


def oracle_pose_stage(sc, recs):
    """(a)"""
    at, worst = 0, [0.0, 0.0, 0.0]
    for r in recs:
        a, b = at, at + r["n"]
        want, wmask = cc.Cpu().essential(sc["p1"][a:b], sc["p2"][a:b], sc["npts"][a:b])
        for i in range(r["n"]):
            g, o, m = r["pose0"][i], want[i], int(sc["npts"][a + i])
            for f in ("n_inliers", "n_pose_good", "iters_run", "n_points"):
                assert int(g[f]) == int(o[f]), ("vis_essential_batch", sc["name"], a + i, f, g, o)
            assert r["mask0"][i, :m].tobytes() == wmask[i, :m].tobytes() and (r["mask0"][i, m:] == FILL).all(), ("vis_essential_batch: mask", sc["name"], a + i)
            d = [float(_cmpE(g["E"], o["E"])), float(np.abs(g["R"] - o["R"]).max()), float(np.abs(g["t"] - o["t"]).max())]
            worst = [max(x, y) for x, y in zip(worst, d)]
        at = b
    print(f"\n{sc['name']}: the pose stage against the oracle: E {worst[0]:.1e}, R {worst[1]:.1e}, t {worst[2]:.1e}")
    assert max(worst) <= TOL, ("vis_essential_batch", sc["name"], worst)


def same_bytes(got, want, where):
    """(b): the stages in the chain's order"""
    for k, (g, w) in enumerate(zip(got, want)):
        for stage in cc.STAGES[2:]:
            a, b = np.ascontiguousarray(g[stage]), np.ascontiguousarray(w[stage])
            if a.tobytes() != b.tobytes():
                rows = [i for i in range(len(a))] if a.ndim == 0 or a.shape != b.shape else [i for i in range(len(a)) if a[i].tobytes() != b[i].tobytes()]
                raise AssertionError(f"{where}, call {k}: the first stage that differs is `{stage}`, records {rows[:8]}")


@pytest.mark.parametrize("name", cc.SCENARIOS)
def test_the_chain_on_the_device(chains, name):
    sc, got = cc.scenario(name), chains(name)
    oracle_pose_stage(sc, got)
    cpu = cc.Cpu(poses=[(r["pose0"], r["mask0"]) for r in got])
    want = cc.records(cpu, cc.run_chain(cpu, sc))
    same_bytes(got, want, name)
    e = cc.ladder(sc, got)
    print(f"{name}: " + ", ".join(f"{k} {v:.2e}" for k, v in e.items()))
    conditions(sc, got, name)
    for k, v in e.items():
        assert v <= 4 * MEASURED[name][k], (name, k, v, MEASURED[name][k])


@pytest.mark.parametrize("name", ("gated", "lost"))
def test_queued_equals_synchronised_call_by_call(chains, name):
    queued, synced = chains(name), chains(name, True)
    for k, (g, w) in enumerate(zip(queued, synced)):
        for stage in cc.STAGES:
            assert np.ascontiguousarray(g[stage]).tobytes() == np.ascontiguousarray(w[stage]).tobytes(), (name, k, stage)


def test_cut_against_chain(chains):
    d, sums = compare_cut_with_chain(cc.scenario("cut"), chains("cut"), chains("chain"))
    print(f"\ncut (23, 17) against chain: trajectory dR {d[0]:.1e}, d sigma {d[1]:.1e}, dt {d[2]:.1e}; carried sums gyro {sums[0]:.1e}, lin {sums[1]:.1e}, ba {sums[2]:.1e}")
