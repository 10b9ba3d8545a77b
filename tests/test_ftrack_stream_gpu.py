"""GPU: feature tracks as a stream -- cuts, gaps, repeated calls, queued launches.  vis_batch_ftrack is the one stage of the batch plan whose
result depends on every launch before it; everything here runs three launches or more and compares BYTE FOR BYTE with the restatement
tests/ftrack_ref.py driven the same way and with the whole-stream dictionary walk of tests/ftrack_stream_cases.py, which knows no launches.
Output buffers are pre-filled with 0xEE and everything behind the written extent must keep it (tests/test_ftrack_gpu.py's convention).

a. vis_ftrack_link_rows chained by the caller ON THE DEVICE: d_carry_in of a launch points into the d_obs of an earlier one.
b. vis_batch_ftrack over cuts A - D of the gated stream (a one-frame launch, an all-flat launch while a row is held, one launch, launches of
   one frame), gate on and off, every list source, the pose stage's mask and a caller's mask: per launch against the restatement on the lists
   the getters return, per cut against the walker, across cuts identical.
c. Call patterns on cut C: the call twice per run, twice with another source or another mask (the last call's row is carried), a run without
   VIS_STAGE_DETECT in between, a launch that was not linked, vis_batch_reset and vis_batch_plan in mid-stream, an all-flat first launch.
d. run + ftrack + N-view triangulation + results download queued back to back (every buffer taken before the first call: nothing waits in
   between) equal the same calls synchronised one by one.

The vacuity guards of ftrack_stream_cases.guards are asserted on the restatement's rows of the DEVICE's lists: a carry that links nothing
shows nothing."""
import numpy as np
import pytest

import ftrack_ref as fr
import ftrack_stream_cases as sc
from test_ftrack_ref import random_stream

pytestmark = pytest.mark.gpu
FILL = 0xEE
W, H, N = sc.W, sc.H, sc.N


def _dev(torch, a):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def _filled(torch, nbytes):
    t = torch.full((nbytes,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()                                       # (the fill ran on torch's stream: finished before the library's streams write)
    return t


# ---------------------------------------------------------------------------------------------- a. rows form, chained on the device
@pytest.mark.parametrize("seed,n,row_cap,link_cap", sc.RANDOM_STREAMS)
def test_rows_chained_on_the_device(vislam, ctx, seed, n, row_cap, link_cap):
    """every launch of a cut queued without a word from the host: d_carry_in is the row of the last saved frame inside an earlier launch's d_obs,
    or the pointer the launch before was given when that launch saved nothing"""
    import torch
    prev, nkp, links, nlinks, mask = random_stream(seed, n, row_cap, link_cap, hostile=True)
    d_nkp, d_links, d_nl, d_mask = _dev(torch, nkp), _dev(torch, links.reshape(-1).view(np.uint8)), _dev(torch, nlinks), _dev(torch, mask)
    assert mask.shape == (n, link_cap)
    for masked in (False, True):
        w_obs, w_fr = sc.walk_link(prev, nkp, links, nlinks, row_cap, mask if masked else None)
        for name, cut in sc.cuts_of(prev).items():
            at, local = 0, []
            for m in cut:
                local.append(sc.localise(prev, at, m))
                at += m
            d_prev = _dev(torch, np.concatenate(local))
            obs, frames = _filled(torch, (n * row_cap + 3) * 16), _filled(torch, (n + 2) * 32)
            at, carry_ptr = 0, 0
            for m in cut:
                assert at + m <= n
                ctx.ftrack_link_rows(m, d_prev.data_ptr() + at * 4, d_nkp.data_ptr() + at * 4, d_links.data_ptr() + at * link_cap * 16,
                                     d_nl.data_ptr() + at * 4, link_cap, row_cap, obs.data_ptr() + at * row_cap * 16, frames.data_ptr() + at * 32, at,
                                     d_mask.data_ptr() + at * link_cap if masked else 0, link_cap if masked else 0, carry_ptr)
                saved = [i for i in range(at, at + m) if int(prev[i]) != fr.KF_NOT_SAVED]
                if saved:
                    carry_ptr = obs.data_ptr() + saved[-1] * row_cap * 16
                at += m
            ctx.batch_sync()
            ro, rf = obs.cpu().numpy(), frames.cpu().numpy()
            assert (ro[n * row_cap * 16:] == FILL).all() and (rf[n * 32:] == FILL).all()
            g_obs = ro[:n * row_cap * 16].view(fr.OBS_DTYPE).reshape(n, row_cap)
            assert rf[:n * 32].tobytes() == w_fr.tobytes(), (name, masked, rf[:n * 32].view(fr.FRAME_DTYPE), w_fr)
            assert g_obs.tobytes() == w_obs.tobytes(), (name, masked, np.argwhere(g_obs != w_obs)[:5])
        assert n < 30 or int(w_obs["len"].max()) >= 3


# ---------------------------------------------------------------------------------------------- the plan driven as a stream
class Stream:
    """one context with a plan of B frames over device frames, and the restatement's state beside it.
    The device side:  c the context, dev the frames, at the stream index of frame 0 of the next (or last) run, n the frames of the last run,
                      d_mask / h_mask the whole-stream mask (rows of KC bytes), KC the keypoint capacity, CAP the row length of the buffers.
    The restatement:  carry the row the next run continues (None: none is held), seq the stream number of frame 0 of the last run since the
                      reset, carried_kps the keypoints of the last saved frame (the symmetric list of a pair with the carried keyframe is
                      rebuilt from them), last the restatement of the last checked call of the run (its row is the one carried),
                      _lists what the getters returned for the run.
    The log:          everything linked since the last reset in STREAM numbering (origin = the frame index of the reset), for the walker."""

    def __init__(self, vislam, orc, torch, frames, gate, B):
        self.v, self.orc, self.torch, self.gate, self.B = vislam, orc, torch, gate, B
        self.at = 0
        self.p = sc.stream_params(vislam, gate)
        self.c = vislam.Context(0, self.p)
        self.dev = _dev(torch, frames)
        self.plan()
        self.KC = self.c.keypoint_capacity(W, H)
        self.CAP = self.KC + 5
        self.ROOT2 = int(np.floor(np.sqrt(self.p.n_cells))) ** 2
        self.d_mask = _dev(torch, sc.stream_mask(self.KC))
        self.h_mask = sc.stream_mask(self.KC)

    def plan(self):
        self.c.batch_plan(W, H, W, self.B)
        self.reset(call=False)

    def reset(self, call=True):
        if call:
            self.c.batch_reset()
        self.carry, self.carried_kps, self.seq, self.last, self.n = None, None, 0, None, 0
        self.log = dict(prev=[], nkp=[], links={}, nl={}, mask={}, last_saved=None, origin=self.at)

    def close(self):
        self.c.close()

    # -- the device
    def run(self, n, stages=None, at=None):
        assert 1 <= n <= self.B
        self.at = self.at if at is None else at
        assert self.at + n <= len(self.dev)
        self.c.batch_run(self.dev.data_ptr() + self.at * W * H, n, self.v.STAGE_ALL if stages is None else stages)
        self.n, self._lists, self.last = n, None, None

    def buffers(self, n):
        """filled output buffers of one vis_batch_ftrack call over n frames (the fill synchronises the device: a test that queues calls takes
        its buffers BEFORE the first of them)"""
        return dict(obs=_filled(self.torch, (n * self.CAP + 2) * 16), frames=_filled(self.torch, (n + 2) * 32))

    def ftrack(self, src, inl=False, masked=False, into=None):
        """queue vis_batch_ftrack for the last run into buffers of its own; with `into` (from buffers) nothing but the call itself happens"""
        n = self.n
        into = self.buffers(n) if into is None else into
        obs, frames = into["obs"], into["frames"]
        assert obs.numel() == (n * self.CAP + 2) * 16 and frames.numel() == (n + 2) * 32
        self.c.batch_ftrack(n, self.CAP, obs.data_ptr(), frames.data_ptr(), src, inl, self.d_mask.data_ptr() + self.at * self.KC if masked else 0,
                            self.KC if masked else 0)                # mask_cap exactly the symmetric list's row length
        assert not masked or src == self.v.FT_SYM
        return dict(obs=obs, frames=frames, src=src, inl=inl, masked=masked)

    def fetch(self, h):
        """(rows (n, KC), records (n)) of a call, after the sync; the guard entries and the entries behind the keypoint capacity keep the fill"""
        n = self.n
        ro, rf = h["obs"].cpu().numpy(), h["frames"].cpu().numpy()
        assert (ro[n * self.CAP * 16:] == FILL).all() and (rf[n * 32:] == FILL).all()
        g = ro[:n * self.CAP * 16].view(fr.OBS_DTYPE).reshape(n, self.CAP)
        assert (g[:, self.KC:].view(np.uint8) == FILL).all()
        return np.ascontiguousarray(g[:, :self.KC]), rf[:n * 32].view(fr.FRAME_DTYPE)

    # -- the restatement
    def lists(self):
        """what the getters return for the last run (read once per run)"""
        if self._lists is None:
            c, n = self.c, self.n
            c.batch_sync()
            assert c.batch_status() == 0
            prev = c.batch_get_keyframes()
            kps = [c.batch_keypoints(i)[0] for i in range(n)]
            good = [c.batch_matches(i)[0] for i in range(n)]
            sym = []
            for i in range(n):
                kq = kps[prev[i]] if prev[i] >= 0 else self.carried_kps if prev[i] == fr.KF_CARRIED else None
                sym.append(np.zeros(0, fr.DMATCH_DTYPE) if kq is None else self.orc.good_matches(self.p, kq, kps[i], *c.batch_knn(i))[1])
            self._lists = dict(prev=prev, kps=kps, nkp=np.array([len(k) for k in kps], np.int32), good=good, sym=sym)
        return self._lists

    def want(self, h, carry="held"):
        """the restatement of a call on the lists of the run, continuing self.carry"""
        L, n = self.lists(), self.n
        sym = h["src"] == self.v.FT_SYM
        links, nl = sc.as_rows(L["sym"] if sym else L["good"], self.KC if sym else self.ROOT2)
        mask = None
        if h["inl"]:
            mask = np.zeros((n, links.shape[1]), np.uint8)
            for i in range(n):
                m = self.c.batch_inlier_mask(i)
                mask[i, :len(m)] = m
                nl[i] = min(nl[i], len(m))                         # (the pose stage's first n_points bytes)
        elif h["masked"]:
            mask = self.h_mask[self.at:self.at + n]
        o, f = fr.link_rows(L["prev"], L["nkp"], links, nl, self.KC, mask, self.carry if carry == "held" else carry, seq0=self.seq)
        return dict(obs=o, frames=f, links=links, nl=nl, mask=mask)

    def check(self, h, where):
        """the call's bytes against the restatement; remembered as the last call of the run (its row is the one carried)"""
        self.c.batch_sync()
        assert self.c.batch_status() == 0
        g_obs, g_fr = self.fetch(h)
        w = self.want(h)
        assert g_fr.tobytes() == w["frames"].tobytes(), (where, self.at, g_fr, w["frames"])
        assert g_obs.tobytes() == w["obs"].tobytes(), (where, self.at, np.argwhere(g_obs != w["obs"])[:5])
        self.last = dict(w, got=g_obs, got_frames=g_fr, key=(h["src"], h["inl"], h["masked"]))
        return self.last

    def advance(self):
        """the run is over: the row of its last call is carried (none when it was not linked), the stream moves on"""
        L, n, log = self.lists(), self.n, self.log
        prev = L["prev"]
        log["prev"] += sc.globalise(prev, self.at - log["origin"], log["last_saved"])
        log["nkp"] += L["nkp"].tolist()
        if self.last is not None:
            for i in range(n):
                g = self.at - log["origin"] + i
                log["links"][g], log["nl"][g] = self.last["links"][i], int(self.last["nl"][i])
                log["mask"][g] = None if self.last["mask"] is None else self.last["mask"][i]
        self.carry = fr.carry_out(prev, self.last["obs"], self.carry, self.KC) if self.last is not None else None
        saved = [i for i in range(n) if int(prev[i]) != fr.KF_NOT_SAVED]
        if saved:
            self.carried_kps, log["last_saved"] = L["kps"][saved[-1]], self.at - log["origin"] + saved[-1]
        self.at += n
        self.seq += n

    def step(self, n, src, inl=False, masked=False, where=None):
        self.run(n)
        r = self.check(self.ftrack(src, inl, masked), where)
        self.advance()
        return r

    def walker(self):
        """the whole-stream walk over everything linked since the last reset: (obs, frames, global prev)"""
        log = self.log
        n = len(log["prev"])
        cap = len(log["links"][0])
        links, nl = np.zeros((n, cap), fr.DMATCH_DTYPE), np.zeros(n, np.int32)
        mask = None if log["mask"][0] is None else np.zeros((n, cap), np.uint8)
        for i in range(n):
            links[i], nl[i] = log["links"][i], log["nl"][i]
            if mask is not None:
                mask[i] = log["mask"][i]
        prev = np.array(log["prev"], np.int32)
        return sc.walk_link(prev, np.array(log["nkp"], np.int32), links, nl, self.KC, mask) + (prev,)


@pytest.fixture(scope="module")
def frames(vislam, canvas):
    plain = sc.stream_frames(vislam, canvas, n=40)
    out = {}
    for gate in (False, True):
        f = plain[:N].copy()
        if gate:
            f[sc.FLAT] = 128
        g = plain.copy()
        if gate:
            g[[5, 21]] = 128
        out[gate] = dict(stream=f, five=g)
    return out


# ---------------------------------------------------------------------------------------------- b. cuts A - D
def _variants(vislam, kind):
    """(source, pose_inliers, caller's mask): the unmasked list first, then its masked twin.  The pose stage sees the good lists (the default
    vis_params.pose_input), so its mask goes with VIS_FT_GOOD; the caller's whole-stream mask goes with VIS_FT_SYM."""
    return [(vislam.FT_SYM, False, False), (vislam.FT_SYM, False, True)] if kind == "sym" else [(vislam.FT_GOOD, False, False), (vislam.FT_GOOD, True, False)]


@pytest.mark.parametrize("kind", ["sym", "good"])
@pytest.mark.parametrize("gate", [True, False], ids=["gate_on", "gate_off"])
def test_plan_over_the_cuts(vislam, orc, frames, gate, kind):
    import torch
    streams = {B: Stream(vislam, orc, torch, frames[gate]["stream"], gate, B) for B in sorted(set(sc.PLAN_B.values()))}
    rows, pose_masks, unmasked = {}, {}, {}
    for v, (src, inl, masked) in enumerate(_variants(vislam, kind)):
        for name, cut in sc.CUTS.items():
            s = streams[sc.PLAN_B[name]]
            s.at = 0
            s.reset()
            got, want, recs = [], [], []
            for launch, n in enumerate(cut):
                r = s.step(n, src, inl, masked, where=(kind, v, name, launch))      # per launch: the device against the restatement on the getters' lists
                got.append(r["got"])
                want.append(r["obs"])
                recs.append(r["frames"])
            got, want, recs = np.concatenate(got), np.concatenate(want), np.concatenate(recs)
            w_obs, w_fr, prev = s.walker()                                          # per cut: against the walk over the global prev[]
            assert got.tobytes() == w_obs.tobytes(), (kind, v, name, np.argwhere(got != w_obs)[:5])
            assert recs.tobytes() == w_fr.tobytes(), (kind, v, name)
            assert [i for i in range(N) if int(prev[i]) == fr.KF_NOT_SAVED] == (sc.FLAT if gate else [])
            if inl:
                pose_masks[name] = [None if m is None else m.tobytes() for m in (s.log["mask"][i] for i in range(N))]
            rows[(v, name)] = got
            if v == 0:
                unmasked[name] = want
            crossing = sc.guards(kind, want, recs, prev, cut, unmasked=unmasked[name] if v else None, gated=gate and name == "A")
            if name == "A":
                print(f"\ngate {gate}, {kind}, variant {v}: tracks crossing into the launches of cut A {[g[2] for g in crossing]}, longest {int(want['len'].max())}")
        if inl:                                                     # the pose stage's masks themselves, before the rows built on them
            for name in sc.CUTS:
                assert pose_masks[name] == pose_masks["A"], (name, [i for i in range(N) if pose_masks[name][i] != pose_masks["A"][i]])
        for name in sc.CUTS:                                        # across cuts: the same observations
            assert rows[(v, name)].tobytes() == rows[(v, "A")].tobytes(), (kind, v, name, np.argwhere(rows[(v, name)] != rows[(v, "A")])[:5])
    for s in streams.values():
        s.close()


# ---------------------------------------------------------------------------------------------- c. call patterns on cut C
CUT_C = sc.CUTS["C"]


@pytest.fixture(scope="module")
def once(vislam, orc, frames):
    """cut C with the call once per run: {gate: [(rows, records) per launch]} for VIS_FT_SYM"""
    import torch
    out = {}
    for gate in (True, False):
        s = Stream(vislam, orc, torch, frames[gate]["stream"], gate, 8)
        out[gate] = [(r["got"], r["got_frames"]) for r in (s.step(n, vislam.FT_SYM, where=("once", k)) for k, n in enumerate(CUT_C))]
        s.close()
    return out


@pytest.fixture()
def stream_c(vislam, orc, frames, request):
    import torch
    gate = request.param
    s = Stream(vislam, orc, torch, frames[gate]["stream"], gate, 8)
    yield s
    s.close()


both_gates = pytest.mark.parametrize("stream_c", [True, False], ids=["gate_on", "gate_off"], indirect=True)


@both_gates
def test_the_call_twice_for_every_run(vislam, once, stream_c):
    s = stream_c
    bufs = [(s.buffers(n), s.buffers(n)) for n in CUT_C]            # taken before the stream starts: the two calls of a run go out back to back
    for k, n in enumerate(CUT_C):
        s.run(n)
        h1, h2 = s.ftrack(vislam.FT_SYM, into=bufs[k][0]), s.ftrack(vislam.FT_SYM, into=bufs[k][1])
        r1, r2 = s.check(h1, ("first", k)), s.check(h2, ("again", k))
        assert r1["got"].tobytes() == r2["got"].tobytes() and r1["got_frames"].tobytes() == r2["got_frames"].tobytes()
        assert r2["got"].tobytes() == once[s.gate][k][0].tobytes() and r2["got_frames"].tobytes() == once[s.gate][k][1].tobytes(), k
        s.advance()
    sc.guards("sym", *s.walker(), CUT_C)


@pytest.mark.parametrize("second", ["source", "mask"])
@both_gates
def test_twice_with_different_calls_the_last_call_is_carried(vislam, stream_c, second):
    """VIS_FT_SYM, then for the same run VIS_FT_GOOD (another source) or VIS_FT_SYM with the caller's mask (another mask): both calls continue
    the row the run was given, and the row of the LAST call is the one the next run continues (include/vislam_hip.h says so)"""
    s = stream_c
    differs = 0
    bufs = [(s.buffers(n), s.buffers(n)) for n in CUT_C]            # taken before the stream starts: the two calls of a run go out back to back
    for k, n in enumerate(CUT_C):
        s.run(n)
        h1 = s.ftrack(vislam.FT_SYM, into=bufs[k][0])
        h2 = s.ftrack(vislam.FT_GOOD, into=bufs[k][1]) if second == "source" else s.ftrack(vislam.FT_SYM, masked=True, into=bufs[k][1])
        r1 = s.check(h1, ("first", k))
        other = fr.carry_out(s.lists()["prev"], r1["obs"], s.carry, s.KC)      # the row a first-call-wins rule would carry
        r2 = s.check(h2, (second, k))
        if k + 1 < len(CUT_C):
            differs += other.tobytes() != fr.carry_out(s.lists()["prev"], r2["obs"], s.carry, s.KC).tobytes()
        s.advance()
    assert differs >= 3                                             # (the two rules differ: the comparison of the next launch tells them apart)
    w_obs, w_fr, prev = s.walker()                                  # the last calls form a stream of their own
    got = sc.crossing(w_obs, prev, CUT_C)
    assert len(got) == len(CUT_C) - 1 and all(g[2] >= (sc.FLOOR["good"] if second == "source" else 1) for g in got), got
    assert not (w_fr["flags"] & fr.FT_NO_CARRY).any()


@both_gates
def test_a_run_without_detect_between_two_calls_is_the_same_run(vislam, once, stream_c):
    s = stream_c
    for k, n in enumerate(CUT_C):
        s.run(n)
        r1 = s.check(s.ftrack(vislam.FT_SYM), ("before", k))
        if k in (1, 2):
            s.run(n, stages=vislam.STAGE_MATCH)                    # the matcher again on the same records: no new frames, the same run
            r2 = s.check(s.ftrack(vislam.FT_SYM), ("after", k))
            assert r2["got"].tobytes() == r1["got"].tobytes() and r2["got_frames"].tobytes() == r1["got_frames"].tobytes()
        assert s.last["got"].tobytes() == once[s.gate][k][0].tobytes() and s.last["got_frames"].tobytes() == once[s.gate][k][1].tobytes(), k
        s.advance()


@both_gates
def test_a_launch_that_was_not_linked(vislam, stream_c):
    """launch 2 of 5 runs without the call: the frame of launch 3 whose pair is the carried keyframe is VIS_FT_NO_CARRY and no other, launch 4
    continues launch 3's tracks, seq counts the frames that were not linked"""
    s = stream_c
    rs = []
    for k, n in enumerate(CUT_C):
        s.run(n)
        rs.append(s.check(s.ftrack(vislam.FT_SYM), ("unlinked", k)) if k != 1 else None)
        if k == 2:
            prev, flags = s.lists()["prev"], rs[2]["got_frames"]["flags"]
            assert int(prev[0]) == fr.KF_CARRIED and (prev == fr.KF_CARRIED).sum() == 1
            assert [int(x) & fr.FT_NO_CARRY for x in flags] == [fr.FT_NO_CARRY if q == fr.KF_CARRIED else 0 for q in prev]
            assert (rs[2]["got"]["birth_seq"][rs[2]["got"]["len"] > 0] >= 16).all()
        s.advance()
    assert rs[2]["got_frames"]["seq"].tolist() == list(range(16, 24)) and rs[4]["got_frames"]["seq"].tolist() == list(range(32, 37))
    assert not (rs[3]["got_frames"]["flags"] & fr.FT_NO_CARRY).any() and not (rs[4]["got_frames"]["flags"] & fr.FT_NO_CARRY).any()
    first = rs[3]["got"][0]                                         # frame 24: its tracks were born in launch 3
    born = first["birth_seq"][first["len"] > 1]
    assert len(born) >= sc.FLOOR["sym"] and ((born >= 16) & (born < 24)).all()


@pytest.mark.parametrize("how", ["reset", "plan"])
@both_gates
def test_reset_and_plan_in_mid_stream(vislam, stream_c, how):
    """vis_batch_reset / vis_batch_plan after launch 2: seq restarts at 0, no track predates it, frame 0 has no pair"""
    s = stream_c
    for k, n in enumerate(CUT_C):
        if k == 2:
            s.reset() if how == "reset" else s.plan()
        r = s.step(n, vislam.FT_SYM, where=(how, k))
        if k >= 2:
            live = r["got"]["len"] > 0
            assert r["got_frames"]["seq"].tolist() == list(range(s.seq - n, s.seq)) and s.seq == sum(CUT_C[2:k + 1])
            assert (r["got"]["birth_seq"][live] >= 0).all() and (r["got"]["birth_seq"] <= r["got_frames"]["seq"][:, None]).all()
        if k == 2:
            assert int(r["got_frames"][0]["flags"]) == fr.FT_NO_PAIR and int(r["got_frames"][0]["seq"]) == 0 and int(s.lists()["prev"][0]) == fr.KF_FIRST
            assert (r["got"][0]["len"][:int(r["got_frames"][0]["n_keypoints"])] == 1).all() and int(r["got_frames"][0]["n_keypoints"]) > 100
    w_obs, w_fr, prev = s.walker()                                  # the stream since the reset, against the walk
    assert len(prev) == sum(CUT_C[2:])
    sc.guards("sym", w_obs, w_fr, prev, CUT_C[2:])


def test_an_all_flat_first_launch(vislam, orc, frames):
    """eight flat frames, then the gated stream: every row of launch 1 is empty, nothing was saved, and the first saved frame of launch 2 has no
    pair -- VIS_FT_NO_PAIR, not NO_CARRY; launch 3 continues launch 2"""
    import torch
    f = np.concatenate([np.full((8, H, W), 128, np.uint8), frames[True]["stream"][:16]])
    s = Stream(vislam, orc, torch, f, True, 8)
    r = [s.step(8, vislam.FT_SYM, where=("flat first", k)) for k in range(3)]
    s.close()
    assert r[0]["got"].tobytes() == np.tile(fr.empty_row(s.KC), (8, 1)).tobytes() and not r[0]["got_frames"]["n_keypoints"].any()
    assert (r[0]["got_frames"]["flags"] == fr.FT_NO_PAIR).all() and r[0]["got_frames"]["seq"].tolist() == list(range(8))
    assert int(r[1]["got_frames"][0]["n_keypoints"]) > 100 and int(r[1]["got_frames"][0]["flags"]) == fr.FT_NO_PAIR and not r[1]["got_frames"][0]["n_continued"]
    assert not any(int(x) & fr.FT_NO_CARRY for q in r for x in q["got_frames"]["flags"])
    first = r[2]["got"][0]
    assert int(((first["len"] > 1) & (first["birth_seq"] >= 8) & (first["birth_seq"] < 16)).sum()) >= sc.FLOOR["sym"]      # launch 3 continues launch 2


# ---------------------------------------------------------------------------------------------- d. queued equals synchronised
STEPS = 5


def _poses(n):
    poses = np.zeros((n, 12))
    for i in range(n):
        a = 0.002 * i
        poses[i, :9] = [np.cos(a), 0, np.sin(a), 0, 1, 0, -np.sin(a), 0, np.cos(a)]
        poses[i, 9:] = [-0.05 * i, 0.0, 0.0]
    return poses


def _tri_buffers(torch, s, n):
    return dict(points=_filled(torch, (n * s.CAP + 1) * 40), flags=_filled(torch, n * s.CAP + 8), summary=_filled(torch, (n + 1) * 32))


def _triangulate(vislam, s, n, h, d_poses, t):
    tp = vislam.default_ftrack_tri_params()
    tp.max_views, tp.gn_iters = 8, 2
    s.c.batch_ftrack_triangulate(n, h["obs"].data_ptr(), s.CAP, d_poses.data_ptr(), t["points"].data_ptr(), t["flags"].data_ptr(), t["summary"].data_ptr(), tp)


def _sequence(vislam, orc, torch, f, gate, src, inl, sync_each):
    """{buffer name: [bytes of launch 0, ...]} of five launches of 8 on a plan of 8, every launch into buffers of its own"""
    s = Stream(vislam, orc, torch, f, gate, 8)
    d_poses = _dev(torch, _poses(8))
    hs, poses, rows = [], [np.zeros(8, vislam.POSE_RESULT_DTYPE) for _ in range(STEPS)], []
    # every buffer of every launch before the first call: filling one synchronises the device, and between batch_run(k), the follow-ups and
    # batch_run(k + 1) of the queued pass there is no torch call and no wait
    bufs, ts = [s.buffers(8) for _ in range(STEPS)], [_tri_buffers(torch, s, 8) for _ in range(STEPS)]

    def step():
        if sync_each:
            s.c.batch_sync()

    for k in range(STEPS):
        s.run(8)
        step()
        hs.append(s.ftrack(src, inl, into=bufs[k]))
        step()
        _triangulate(vislam, s, 8, hs[-1], d_poses, ts[k])
        step()
        s.c.batch_results_async(8, poses[k].ctypes.data)
        step()
        if sync_each:                                               # the rows against the restatement, launch by launch
            rows.append(s.check(hs[-1], ("synchronised", k)))
            s.advance()
        else:
            s.at += 8
    s.c.batch_sync()
    assert s.c.batch_status() == 0
    got = dict(obs=[h["obs"].cpu().numpy().tobytes() for h in hs], frames=[h["frames"].cpu().numpy().tobytes() for h in hs], poses=[q.tobytes() for q in poses])
    for name in ("points", "flags", "summary"):
        got[name] = [t[name].cpu().numpy().tobytes() for t in ts]
    walk = s.walker() if sync_each else None
    s.close()
    return got, rows, walk


@pytest.mark.parametrize("inliers", [False, True], ids=["sym", "pose_inliers"])
@pytest.mark.parametrize("gate", [False, True], ids=["gate_off", "gate_on"])
def test_queued_launches_equal_synchronised_ones(vislam, orc, frames, gate, inliers):
    import torch
    src = vislam.FT_GOOD if inliers else vislam.FT_SYM
    queued, _, _ = _sequence(vislam, orc, torch, frames[gate]["five"], gate, src, inliers, False)
    synced, rows, (w_obs, w_fr, prev) = _sequence(vislam, orc, torch, frames[gate]["five"], gate, src, inliers, True)
    # not a comparison of empty records (conditions on the synchronised run)
    assert np.concatenate([r["obs"] for r in rows]).tobytes() == w_obs.tobytes()
    assert [i for i in range(40) if int(prev[i]) == fr.KF_NOT_SAVED] == ([5, 21] if gate else [])
    crossing = sc.crossing(w_obs, prev, [8] * STEPS)
    sm = np.frombuffer(b"".join(b[:8 * 32] for b in synced["summary"]), fr.TRI_SUMMARY_DTYPE)
    print(f"\ngate {gate}, pose_inliers {inliers}: tracks crossing {[g[2] for g in crossing]}, {int(sm['n_points'].sum())} points of {int(sm['n_ends'].sum())} ends")
    assert len(crossing) == STEPS - 1 and all(g[2] >= (1 if inliers else sc.FLOOR["sym"]) for g in crossing) and not (w_fr["flags"] & fr.FT_NO_CARRY).any()
    assert int(sm["n_points"].sum()) >= 50
    for name in synced:
        for k in range(STEPS):
            assert queued[name][k] == synced[name][k], (name, k)


def test_triangulation_of_a_one_frame_launch(vislam, orc, frames):
    """cut A's second launch is one frame: every keypoint ends its track inside the call with one view -- VIS_FTP_FEW"""
    import torch
    s = Stream(vislam, orc, torch, frames[True]["stream"], True, 8)
    s.step(8, vislam.FT_SYM, where="launch 0")
    bufs, t, d_poses = s.buffers(1), _tri_buffers(torch, s, 1), _dev(torch, _poses(1))
    s.run(1)
    h = s.ftrack(vislam.FT_SYM, into=bufs)
    _triangulate(vislam, s, 1, h, d_poses, t)
    r = s.check(h, "launch 1")
    nk = int(r["got_frames"][0]["n_keypoints"])
    pts, fl, sm = t["points"].cpu().numpy(), t["flags"].cpu().numpy(), t["summary"].cpu().numpy()
    s.close()
    assert nk > 100 and int(r["got_frames"][0]["n_continued"]) >= sc.FLOOR["sym"]
    assert (fl[:nk] == fr.FTP_FEW).all() and (fl[nk:] == FILL).all() and (sm[32:] == FILL).all() and (pts[nk * 40:] == FILL).all()
    p = pts[:nk * 40].view(fr.POINT_DTYPE)
    assert (p["flags"] == fr.FTP_FEW).all() and (p["n_views"] == 1).all() and not p["X"].any()
    assert sm[:32].view(fr.TRI_SUMMARY_DTYPE)[0].tolist() == (nk, 0, 0, 0, 0, 0, nk, 0)
