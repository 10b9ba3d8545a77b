"""GPU: the scale links and the chained trajectory as a stream, through vis_batch_run on the 37 small synthetic frames of
tests/ftrack_stream_cases.py, keyframe gate off and on.

a. Per launch: vis_batch_scale_links / vis_batch_trajectory against vis_scale_link_rows / vis_trajectory_rows fed with the downloaded lists, pose
   records, map points and the row / record carried so far, BYTE FOR BYTE, and both against the restatements.
b. Cuts A - D of the stream: the links are the same bytes however the stream is cut (q is launch-local: compared in stream numbering); the poses
   agree within 16 x the bound tests/test_trajectory_ref.py measured, their integers exactly.
c. The calls repeated within a run give the same bytes; a launch that was not linked makes the carried pair VIS_SL_NO_DEPTH and the frame a root
   with VIS_TJ_NO_CARRY; vis_batch_reset and vis_batch_plan forget row and record; vis_batch_trajectory_init sets the record.
d. run + triangulate + scale links + trajectory + ftrack + N-view triangulation + results download queued with no wait equal the same calls
   synchronised one by one, byte for byte.
Output buffers are pre-filled with 0xEE and everything behind the written extent must keep it."""
import numpy as np
import pytest

import ftrack_ref as fr
import ftrack_stream_cases as sc
import scale_link_ref as sl
import trajectory_ref as tj
from test_scale_link_gpu import c_params, links_on_device
from test_trajectory_gpu import chain_on_device
from test_trajectory_ref import DOUBLING_BOUND, differences, path_lengths

pytestmark = pytest.mark.gpu
FILL = 0xEE
W, H, N = sc.W, sc.H, sc.N
# a pair of this stream has at most root^2 = 49 correspondences, and consecutive pairs of its grid-filtered lists share 0 ... 5 kept map points:
# one ratio makes a link here, so that chains of scaled edges do form
SP = sl.Params(min_shared=1, min_scale=1.0 / 1024.0, max_scale=1024.0)


def _dev(torch, a):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def _filled(torch, nbytes):
    t = torch.full((nbytes,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()                                       # (the fill ran on torch's stream: finished before the library's streams write)
    return t


class Stream:
    """a context with a plan of B frames over the device frames; beside it the depth row and the record the next launch continues, as the rows
    forms and the restatements produce them"""

    def __init__(self, vislam, torch, frames, gate, B):
        self.v, self.torch, self.gate, self.B = vislam, torch, gate, B
        self.p = sc.stream_params(vislam, gate)
        self.c = vislam.Context(0, self.p)
        self.dev = _dev(torch, frames)
        self.c.batch_plan(W, H, W, B)
        self.KC = self.c.keypoint_capacity(W, H)
        self.ROOT2 = int(np.floor(np.sqrt(self.p.n_cells))) ** 2
        self.CAP = self.ROOT2 + 3                                   # the row length of the map-point buffers
        self.forget()
        self.at = 0

    def forget(self):
        self.depth, self.rec, self.seq, self.last_saved = None, None, 0, None

    def close(self):
        self.c.close()

    def buffers(self, n):
        f = lambda b: _filled(self.torch, b)
        return dict(points=f((n * self.CAP + 1) * 32), flags=f(n * self.CAP + 8), summary=f((n + 1) * 16), link=f((n + 2) * 40), traj=f((n + 2) * 128),
                    poses=f((n * 12 + 5) * 8))

    def run(self, n):
        self.c.batch_run(self.dev.data_ptr() + self.at * W * H, n, self.v.STAGE_ALL)
        self.n = n

    def follow(self, b, links=True, chain=True, tri=True):
        """triangulate, scale links and trajectory of the last run, queued"""
        n = self.n
        if tri:
            self.c.batch_triangulate(n, self.CAP, b["points"].data_ptr(), b["flags"].data_ptr(), b["summary"].data_ptr())
        if links:
            self.c.batch_scale_links(n, b["points"].data_ptr(), b["flags"].data_ptr(), self.CAP, b["link"].data_ptr(), c_params(self.v, SP))
        if chain:
            self.c.batch_trajectory(n, b["link"].data_ptr(), b["traj"].data_ptr(), b["poses"].data_ptr())

    def fetch(self, b):
        n = self.n
        self.c.batch_sync()
        assert self.c.batch_status() == 0
        raw = {k: t.cpu().numpy() for k, t in b.items()}
        assert (raw["link"][n * 40:] == FILL).all() and (raw["traj"][n * 128:] == FILL).all() and (raw["poses"][n * 96:] == FILL).all()
        return dict(points=raw["points"][:n * self.CAP * 32].view(sl.MAP_POINT_DTYPE).reshape(n, self.CAP), flags=raw["flags"][:n * self.CAP].reshape(n, self.CAP),
                    link=raw["link"][:n * 40].view(sl.LINK_DTYPE), traj=raw["traj"][:n * 128].view(tj.TRAJ_DTYPE),
                    poses=raw["poses"][:n * 96].view(np.float64).reshape(n, 12))

    def check(self, b, where, links=True, chain=True):
        """the plan forms of the launch against the rows forms and the restatements on what the launch downloads; returns the launch's results"""
        g, n = self.fetch(b), self.n
        prev = self.c.batch_get_keyframes()
        pose, good, ng = self.c.batch_results(n)
        g.update(prev=prev, pose=pose)
        if links:
            case = (prev, good, ng, pose, g["points"], g["flags"])
            depth, want = sl.scale_link_rows(SP, *case, self.KC, self.depth)
            assert g["link"].tobytes() == want.tobytes(), (where, g["link"], want)
            rdepth, rows = links_on_device(self.v, self.c, SP, *case, self.KC, self.depth)
            assert rows.tobytes() == g["link"].tobytes() and rdepth.tobytes() == depth.tobytes(), where
            g["depth"] = depth
        if chain:
            want, wposes = tj.trajectory_rows(prev, pose, g["link"], self.rec, self.seq)
            assert g["traj"].tobytes() == want.tobytes(), (where, [i for i in range(n) if g["traj"][i].tobytes() != want[i].tobytes()])
            assert g["poses"].tobytes() == wposes.tobytes(), where
            rows, rposes = chain_on_device(self.v, self.c, prev, pose, g["link"], self.rec, self.seq)
            assert rows.tobytes() == g["traj"].tobytes() and rposes.tobytes() == g["poses"].tobytes(), where
        return g

    def advance(self, g, links=True, chain=True):
        """the run is over: what its calls left is carried (nothing when a call was left out)"""
        self.depth = sl.carry_out(g["prev"], g["depth"], self.depth, self.KC) if links else None
        self.rec = tj.carry_out(g["prev"], g["traj"], self.rec) if chain else None
        g["gprev"] = sc.globalise(g["prev"], self.at, self.last_saved)
        saved = [i for i in range(self.n) if int(g["prev"][i]) != fr.KF_NOT_SAVED]
        if saved:
            self.last_saved = self.at + saved[-1]
        self.at += self.n
        self.seq += self.n

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


def whole(gs):
    """the launches of a cut as one stream: links with q in stream numbering, records with the parent so"""
    link, traj = np.concatenate([g["link"] for g in gs]), np.concatenate([g["traj"] for g in gs])
    gprev = np.array(sum((g["gprev"] for g in gs), []), np.int32)
    link["q"] = gprev
    traj["parent"] = np.where(traj["flags"] & (tj.TJ_NOT_SAVED | tj.TJ_OVERFLOW), 0, gprev)
    return link, traj


@pytest.mark.parametrize("gate", [False, True], ids=["gate_off", "gate_on"])
def test_cuts_of_the_stream(vislam, frames, gate):
    import torch
    streams = {B: Stream(vislam, torch, frames[gate][:N], gate, B) for B in sorted(set(sc.PLAN_B.values()))}
    out = {}
    for name, cut in sc.CUTS.items():
        s = streams[sc.PLAN_B[name]]
        s.c.batch_reset()
        s.forget()
        s.at = 0
        out[name] = whole([s.step(n, (name, k)) for k, n in enumerate(cut)])
    for s in streams.values():
        s.close()
    link, traj = out["B"]                                           # one launch: the stream as a whole
    ok = link["flags"] == sl.SL_OK
    print(f"\ngate {gate}: {int(ok.sum())} of {N} links OK, n_shared {link['n_shared'].tolist()}, epochs {sorted(set(traj['epoch_seq'].tolist()))}, "
          f"unit edges of the last frame {int(traj[-1]['unit_edges'])}")
    assert ok.sum() >= 5 and (traj["hops"] >= 5).any()              # not a comparison of empty records
    assert [i for i in range(N) if int(link[i]["q"]) == fr.KF_NOT_SAVED] == (sc.FLAT if gate else [])
    path = path_lengths(traj)
    for name, cut in sc.CUTS.items():
        l, t = out[name]
        assert l.tobytes() == link.tobytes(), (name, [i for i in range(N) if l[i].tobytes() != link[i].tobytes()])
        firsts = np.cumsum([0] + cut[:-1])                          # the links of the pairs across a launch boundary exist
        assert name == "B" or any(int(l[i]["n_shared"]) > 0 for i in firsts[1:])
        for f in ("segment_seq", "epoch_seq", "hops", "unit_edges", "parent", "flags"):
            assert (t[f] == traj[f]).all(), (name, f)
        d = differences(t, traj, path)
        assert max(d) <= 16 * DOUBLING_BOUND, (name, d)


@pytest.mark.parametrize("gate", [False, True], ids=["gate_off", "gate_on"])
def test_call_patterns(vislam, frames, gate):
    """cut C: the calls twice per run; launch 2 of 5 without the scale links, launch 3 without the trajectory; a reset before the last launch"""
    import torch
    s = Stream(vislam, torch, frames[gate][:N], gate, 8)
    for k, n in enumerate(sc.CUTS["C"]):
        if k == 4:
            s.c.batch_reset()
            s.forget()
        b1, b2 = s.buffers(n), s.buffers(n)
        links, chain = k != 1, k != 2                               # (the chain of launch 1 reads the buffer's fill: flags that are not VIS_SL_OK, unit edges)
        s.run(n)
        s.follow(b1, links, chain)
        s.follow(b2, links, chain)
        g1, g2 = s.check(b1, ("first", k), links, chain), s.check(b2, ("again", k), links, chain)
        for f in ("link", "traj", "poses"):
            assert g1[f].tobytes() == g2[f].tobytes(), (k, f)
        carried = [i for i in range(n) if int(g1["prev"][i]) == fr.KF_CARRIED]
        if k == 2:                                                  # launch 1 was not linked
            assert carried and all(int(g1["link"][i]["flags"]) == sl.SL_NO_DEPTH for i in carried)
        if k == 3:                                                  # launch 2 was not chained
            assert carried and all(int(g1["traj"][i]["flags"]) == tj.TJ_ROOT | tj.TJ_NO_CARRY for i in carried)
            assert all(int(g1["link"][i]["flags"]) != sl.SL_NO_DEPTH for i in carried)
        if k == 4:                                                  # after the reset
            assert int(g1["prev"][0]) == fr.KF_FIRST and int(g1["link"][0]["flags"]) == sl.SL_NO_PAIR and int(g1["traj"][0]["flags"]) == tj.TJ_ROOT
            assert int(g1["traj"][0]["segment_seq"]) == 0
        s.advance(g1, links, chain)
    # vis_batch_plan forgets too; vis_batch_trajectory_init sets the record the next run continues
    s.c.batch_plan(W, H, W, 8)
    s.forget()
    s.at = 0
    s.step(8, "after plan")
    rec = tj.zero_record(tj.TJ_UNIT_EDGE)
    rec["R"], rec["t"], rec["sigma"], rec["segment_seq"], rec["epoch_seq"], rec["hops"], rec["unit_edges"] = tj.IDENTITY, [1.0, 2.0, 3.0], 2.5, 70, 71, 4, 1
    s.c.batch_trajectory_init(rec)
    s.rec = rec
    g = s.step(8, "after init")
    first = [i for i in range(8) if int(g["prev"][i]) == fr.KF_CARRIED][0]
    assert int(g["traj"][first]["segment_seq"]) == 70 and int(g["traj"][first]["hops"]) == 5
    s.c.batch_trajectory_init(None)
    s.rec = None
    g = s.step(8, "after init(None)")
    assert int(g["traj"][first]["flags"]) & tj.TJ_NO_CARRY
    s.close()


def _sequence(vislam, torch, f, gate, sync_each):
    """four launches of 8, every call of every launch into buffers of its own taken before the first call"""
    s = Stream(vislam, torch, f, gate, 8)
    KC = s.KC
    bufs = [s.buffers(8) for _ in range(4)]
    ft = [dict(obs=_filled(torch, 8 * KC * 16), frames=_filled(torch, 8 * 32), pts=_filled(torch, 8 * KC * 40), fl=_filled(torch, 8 * KC),
               sm=_filled(torch, 8 * 32)) for _ in range(4)]
    poses = [np.zeros(8, vislam.POSE_RESULT_DTYPE) for _ in range(4)]
    tp = vislam.default_ftrack_tri_params()
    tp.max_views, tp.gn_iters = 8, 2

    def step():
        if sync_each:
            s.c.batch_sync()

    for k in range(4):
        s.run(8)
        step()
        s.follow(bufs[k], True, False)
        step()
        s.follow(bufs[k], False, True, tri=False)
        step()
        s.c.batch_ftrack(8, KC, ft[k]["obs"].data_ptr(), ft[k]["frames"].data_ptr())
        step()
        s.c.batch_ftrack_triangulate(8, ft[k]["obs"].data_ptr(), KC, bufs[k]["poses"].data_ptr(), ft[k]["pts"].data_ptr(), ft[k]["fl"].data_ptr(),
                                     ft[k]["sm"].data_ptr(), tp)
        step()
        s.c.batch_results_async(8, poses[k].ctypes.data)
        step()
        s.at += 8
    s.c.batch_sync()
    assert s.c.batch_status() == 0
    got = {name: [b[name].cpu().numpy().tobytes() for b in bufs] for name in bufs[0]}
    got.update({name: [b[name].cpu().numpy().tobytes() for b in ft] for name in ft[0]})
    got["pose"] = [q.tobytes() for q in poses]
    s.close()
    return got


@pytest.mark.parametrize("gate", [False, True], ids=["gate_off", "gate_on"])
def test_queued_launches_equal_synchronised_ones(vislam, frames, gate):
    import torch
    f = frames[gate][:32]
    queued, synced = _sequence(vislam, torch, f, gate, False), _sequence(vislam, torch, f, gate, True)
    traj = np.frombuffer(b"".join(b[:8 * 128] for b in synced["traj"]), tj.TRAJ_DTYPE)
    sm = np.frombuffer(b"".join(synced["sm"]), fr.TRI_SUMMARY_DTYPE)
    print(f"\ngate {gate}: hops of the last frame {int(traj[-1]['hops'])}, {int(sm['n_points'].sum())} N-view points of {int(sm['n_ends'].sum())} ends")
    assert int(traj["hops"].max()) >= 8 and int(sm["n_ends"].sum()) > 100     # not a comparison of empty records: chains longer than a launch
    for name in synced:
        for k in range(4):
            assert queued[name][k] == synced[name][k], (name, k)


def test_run_directory_writes_the_trajectory(vislam, frames, tmp_path):
    """tools/run_directory.py --trajectory: the CSV holds what the plan forms give for the same frames in the same batches, the chain continuing
    across the batches"""
    import json
    import os
    import subprocess
    import sys

    import torch
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    n, nb = 12, 6
    f = frames[False][:n]
    d = tmp_path / "cam0" / "data"
    d.mkdir(parents=True)
    for t in range(n):
        (d / f"{1403636579763555584 + 50000000 * t}.pgm").write_bytes(b"P5\n%d %d\n255\n" % (W, H) + f[t].tobytes())
    csv = tmp_path / "trajectory.csv"
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(root, "tools", "run_directory.py"), str(d), "--batch", str(nb),
                        "--trajectory", str(csv)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    j = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    rows = [l.split(",") for l in csv.read_text().splitlines()]
    p = vislam.default_params()                                    # the tool's parameters: ORB::create(200), fy = fx
    p.fy, p.nfeatures, p.w_size, p.h_size = p.fx, 200, W, H
    c = vislam.Context(0, p)
    c.batch_plan(W, H, W, nb)
    cap = int(np.floor(np.sqrt(p.n_cells))) ** 2
    dev = _dev(torch, f)
    want = []
    for first in range(0, n, nb):
        pts, fl, sm, link, traj = (_filled(torch, b) for b in (nb * cap * 32, nb * cap, nb * 16, nb * 40, nb * 128))
        c.batch_run(dev.data_ptr() + first * W * H, nb, vislam.STAGE_FRAME)
        c.batch_triangulate(nb, cap, pts.data_ptr(), fl.data_ptr(), sm.data_ptr())
        c.batch_scale_links(nb, pts.data_ptr(), fl.data_ptr(), cap, link.data_ptr())
        c.batch_trajectory(nb, link.data_ptr(), traj.data_ptr())
        c.batch_sync()
        want += list(zip(traj.cpu().numpy().view(tj.TRAJ_DTYPE), link.cpu().numpy().view(sl.LINK_DTYPE)))
    c.close()
    assert len(rows) == n and j["trajectory_csv"] == str(csv)
    for i, (row, (t, l)) in enumerate(zip(rows, want)):
        ints = [int(t[k]) for k in ("flags", "parent", "segment_seq", "epoch_seq", "hops", "unit_edges")] + [int(l["n_shared"]), int(l["flags"])]
        assert [int(v) for v in row[:10]] == [i, 1403636579763555584 + 50000000 * i] + ints, i
        assert [float(v) for v in row[10:]] == [float(l["scale"]), float(t["sigma"])] + [float(v) for v in t["R"]] + [float(v) for v in t["t"]], i
    assert int(want[-1][0]["hops"]) >= 6 and j["trajectory"]["roots"] >= 1      # the chain crossed the batch boundary
