"""GPU: the stream-ordering rules of the asynchronous entry points towards a CALLER's stream (vis_set_stream).

Every other GPU test synchronises the host between torch's work and the library, so it only ever hands the library inputs that are complete and
reads outputs after vis_batch_sync.  Here the context runs on S = torch.cuda.Stream() and every caller input arrives LATE: a delay chain and the
device-to-device copies of the real inputs over decoys are still pending on S when the call is queued (asserted: `not event.query()` right
after the call returns), so only the ordering the header promises -- stream order for a call on the context's stream, the fork from the
context's stream for a call on the pose or match stream -- can make the call read the real inputs.  Outputs are compared byte for byte with the
same call on host-synchronised inputs; per input, the same call with that input's decoy must give other bytes (tests/stream_order_cases.py).

The chain is sized by the `env` fixture, not fixed: at least 20 x the host time of the slowest call sequence (two guided launches of
vis_batch_run with every stage and their result downloads) and at least 64 ops, at most 200 ms.  Measured on the MI355X: one chain op (int32 add over 512 MiB)
0.177 ms on the device, host time of that sequence 0.35 - 0.44 ms over three runs, which asks for 41 - 50 ops = 7.3 - 8.9 ms (the chain is never shorter than 64
ops = 11.3 ms); the largest host time of any case's late call sequence was 0.40 ms (vis_batch_run_guided; the row calls take 0.01 - 0.06 ms).

Groups: A the calls the header places on the context's stream (outputs cloned on S, no synchronisation) and one chain of four of them; B
vis_batch_run / vis_batch_run_guided over two launches, also with d_frames overwritten right behind the call and behind vis_rectify_batch; C
the plan follow-ups that take caller device inputs (read after vis_batch_sync); D vis_set_stream itself."""
import math

import numpy as np
import pytest

import stream_order_cases as so

pytestmark = pytest.mark.gpu


class Env:
    pass


@pytest.fixture(scope="module")
def env(vislam, canvas):
    import torch
    E = Env()
    E.torch, E.S = torch, torch.cuda.Stream()
    assert E.S.cuda_stream != 0
    E.cA = vislam.Context(0)                                        # rows and frames without a plan, the reference's parameters
    E.cP = so.plan_context(vislam)                                   # the plan of 320 x 240, B = 8
    E.cA.set_stream(E.S)                                             # (a stream object)
    E.cP.set_stream(E.S.cuda_stream)                                 # (a raw handle)
    E.pinned = so.Pinned(vislam, torch)
    E.frames = so.PlanFrames(vislam, torch, canvas)
    E.rect = so.make_rectifier(vislam, E.cP)
    E.delay = so.Delay(torch, E.S)
    E.hosts = {}
    op_ms = E.delay.measure()
    # the slowest call sequence: warm it twice, then take the slower of two timings
    rig = so.Rig(torch, so.case_batch_run(vislam, torch, E.cP, canvas, E.pinned, guided=True))
    host = [so.run_sync(torch, E.cP, rig)[1] for _ in range(4)][2:]
    chain_ms, ok = E.delay.size(max(host))
    print(f"\nchain op {op_ms:.4f} ms on the device; host time of two guided launches {host[0]:.3f} / {host[1]:.3f} ms; "
          f"chain {E.delay.n_ops} ops = {chain_ms:.1f} ms")
    if not ok:
        pytest.fail(f"a chain of {so.FACTOR:g} x the host time {max(host):.3f} ms is {chain_ms:.1f} ms > {so.CHAIN_MAX_MS:g} ms")
    yield E
    torch.cuda.synchronize()
    print(f"\nlargest host time of a late call sequence: {max(E.hosts.values(), default=0.0):.3f} ms ({E.hosts})")
    E.rect.close()
    E.cP.close()
    E.cA.close()


def _check(E, c, case):
    """sync run, late run (lateness guard, bytes), decoy guard per input; -> the sync run's outputs"""
    torch = E.torch
    rig = so.Rig(torch, case)
    want, _ = so.run_sync(torch, c, rig)
    got, late, host_ms = so.run_late(torch, c, E.S, E.delay, rig)
    E.hosts[case.name] = round(host_ms, 3)
    print(f"\n{case.name}: host {host_ms:.3f} ms of the late call sequence, chain {E.delay.chain_ms:.1f} ms")
    assert late, (case.name, "the producer had finished when the call returned", host_ms, E.delay.chain_ms)
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k] == want[k], (case.name, k, "differs from the synchronised run")
    for name in case.inputs:
        decoy, _ = so.run_sync(torch, c, rig, (name,))
        assert any(decoy[k] != want[k] for k in want), (case.name, name, "its decoy gives the bytes of the real input")
    again, _ = so.run_sync(torch, c, rig)                            # (the runs in between left nothing behind)
    assert all(again[k] == want[k] for k in want), case.name
    return want


# ---------------------------------------------------------------------------------------------- A: on the context's stream
ROW_CASES = dict(f2f=so.case_f2f, filter_keypoints=so.case_filter, homography=so.case_homography, homography_polish=so.case_homography_polish,
                 homography_pose=so.case_homography_pose, essential=so.case_essential, essential_refine=so.case_essential_refine,
                 essential_polish=so.case_essential_polish, pnp=so.case_pnp, ftrack_link_rows=so.case_ftrack_link,
                 ftrack_triangulate_rows=so.case_ftrack_triangulate)
FRAME_CASES = dict(gradient=so.case_gradient, klt=so.case_klt, align=so.case_align, klt_chain=so.case_klt_chain)


@pytest.mark.parametrize("which", sorted(ROW_CASES))
def test_rows_on_the_context_stream(vislam, env, which):
    _check(env, env.cA, ROW_CASES[which](vislam, env.torch, env.cA))


@pytest.mark.parametrize("which", sorted(FRAME_CASES))
def test_frames_on_the_context_stream(vislam, canvas, env, which):
    want = _check(env, env.cA, FRAME_CASES[which](vislam, env.torch, env.cA, canvas))
    if which == "klt_chain":                                         # not a chain of empty records
        pairs = np.frombuffer(want["pair"], vislam.KLT_PAIR_DTYPE)
        h = np.frombuffer(want["h"], vislam.HOMOGRAPHY_RESULT_DTYPE)
        pose = np.frombuffer(want["pose"], vislam.HPOSE_RESULT_DTYPE)
        print(f"tracked {pairs['n_tracked'].tolist()}, H inliers {h['n_inliers'].tolist()}, pose kinds {pose['kind'].tolist()}")
        assert (pairs["n_tracked"][1:] >= 8).all() and (h["best_iter"][1:] >= 0).all()


def test_synth_frames_device_is_ordered_on_the_stream_and_blocks(vislam, canvas, env):
    """vis_synth_frames_device queues its kernel on the context's stream behind the producer of d_canvas, but it is NOT asynchronous: it uploads
    a per-frame table from pageable memory and blocks the host until the stream has drained (csrc/synth.hip; the header said "asynchronous" until
    this test).  So the lateness guard cannot hold for it; what holds is the stream order and the bytes -- those of the HOST generator."""
    torch, case = env.torch, so.case_synth(vislam, env.torch, env.cA, canvas)
    rig = so.Rig(torch, case)
    want, _ = so.run_sync(torch, env.cA, rig)
    got, late, host_ms = so.run_late(torch, env.cA, env.S, env.delay, rig)
    print(f"\nvis_synth_frames_device: late {late}, host {host_ms:.3f} ms, chain {env.delay.chain_ms:.1f} ms")
    host = np.stack([vislam.synth_frame(canvas, t, so.W, so.H, parallax=True) for t in range(3, 3 + so.NF)])
    assert got["frames"] == want["frames"] == host.tobytes()
    decoy, _ = so.run_sync(torch, env.cA, rig, ("canvas",))
    assert decoy["frames"] != want["frames"]


def test_rectify_on_the_context_stream(vislam, canvas, env):
    _check(env, env.cP, so.case_rectify(vislam, env.torch, env.cP, canvas, env.rect))


# ---------------------------------------------------------------------------------------------- B: vis_batch_run
@pytest.mark.parametrize("guided", [False, True], ids=["plain", "guided"])
@pytest.mark.parametrize("reuse", [False, True], ids=["late_frames", "frames_overwritten_behind"])
def test_batch_run_reads_late_frames(vislam, orc, canvas, env, guided, reuse):
    want = _check(env, env.cP, so.case_batch_run(vislam, env.torch, env.cP, canvas, env.pinned, guided, reuse))
    # the anchor is not the library's batch path: frame 0 of the second launch is the CPU oracle's detection of that frame
    ok, od = orc.orb_detect_compute(env.cP.params, so.plan_frames(vislam, canvas)[0][so.B])
    assert len(ok) >= 100 and want["keypoints0"] == ok.tobytes() and want["descriptors0"] == od.tobytes()
    ngood = np.frombuffer(want["results0_ngood"] + want["results1_ngood"], np.int32)
    pose = np.frombuffer(want["results0_pose"] + want["results1_pose"], vislam.POSE_RESULT_DTYPE)
    print(f"good matches per pair {ngood.tolist()}, inliers {pose['n_inliers'].tolist()}")
    assert ngood[0] == 0 and (ngood[1:] >= 8).all() and (pose["n_inliers"][1:] >= 5).sum() >= 8      # the carried pair included


def test_rectified_frames_overwritten_behind_the_run(vislam, canvas, env):
    want = _check(env, env.cP, so.case_rectify_run(vislam, env.torch, env.cP, canvas, env.pinned, env.rect))
    ngood = np.frombuffer(want["results0_ngood"] + want["results1_ngood"], np.int32)
    assert (ngood[1:] >= 8).all(), ngood


# ---------------------------------------------------------------------------------------------- C: plan follow-ups
@pytest.fixture(scope="module")
def plan_cases(vislam, env):
    return so.plan_cases(vislam, env.torch, env.cP, env.frames)


@pytest.mark.parametrize("name", so.PLAN_CASE_NAMES)
def test_follow_up_reads_late_inputs(vislam, env, plan_cases, name):
    want = _check(env, env.cP, plan_cases[name])
    if name == "vis_batch_f2f":
        assert (np.frombuffer(want["rec"], vislam.F2F_RESULT_DTYPE)["best_iter"] >= 0).all()
    if name == "vis_batch_filter_keypoints":
        nkeep = np.frombuffer(want["nkeep"], np.int32)
        print(f"kept per pair {nkeep.tolist()}")
        assert (nkeep > 0).any() and nkeep.min() < nkeep.max()       # rows of kept and of dropped points
    if name == "vis_batch_homography":
        assert (np.frombuffer(want["rec"], vislam.HOMOGRAPHY_RESULT_DTYPE)["best_iter"] >= 0).all()
    if name == "vis_batch_klt":
        assert (np.frombuffer(want["pair"], vislam.KLT_PAIR_DTYPE)["n_points"][1:] > 0).all()
    if name == "vis_batch_track":
        assert (np.frombuffer(want["track"], np.dtype([("pose", "<f4", (7,)), ("composed", "<i4")]))["composed"] != vislam.TRACK_NONE).all()


# ---------------------------------------------------------------------------------------------- D: vis_set_stream
def test_set_stream_drains_the_old_stream(vislam, env):
    torch, c, S = env.torch, env.cP, env.S
    fe = vislam.gradient_frame_elems(so.W, so.H)
    out = [torch.empty(so.B * fe * k, dtype=torch.uint8, device="cuda") for k in (1, 2, 2, 1)]
    torch.cuda.synchronize()
    ev = torch.cuda.Event()
    with torch.cuda.stream(S):
        env.delay.queue()
    c.gradient_batch(env.frames.ptr(0), so.W, so.H, so.W, so.B, *[t.data_ptr() for t in out])   # queued through S, behind the chain
    ev.record(S)
    assert not ev.query()
    try:
        c.set_stream(0)
        assert ev.query()                                            # everything queued through the old stream is complete
    finally:
        c.set_stream(S)


def test_handle_zero_is_the_own_stream_not_torchs_default(vislam, env):
    """vis_set_stream(ctx, NULL) selects the context's own non-blocking stream: work queued through it is not ordered with S (nor with torch's
    default stream, whose handle is 0 too -- the binding refuses that stream object instead of silently taking the own stream)"""
    torch, c, S = env.torch, env.cP, env.S
    fe = vislam.gradient_frame_elems(so.W, so.H)
    out = [torch.empty(so.B * fe * k, dtype=torch.uint8, device="cuda") for k in (1, 2, 2, 1)]
    torch.cuda.synchronize()
    assert torch.cuda.default_stream().cuda_stream == 0
    with pytest.raises(ValueError):
        c.set_stream(torch.cuda.default_stream())
    done = {}
    try:
        for how in ("own", "caller"):
            c.set_stream(0 if how == "own" else S)
            ev = torch.cuda.Event()
            with torch.cuda.stream(S):
                env.delay.queue()
                ev.record(S)
            c.gradient_batch(env.frames.ptr(0), so.W, so.H, so.W, so.B, *[t.data_ptr() for t in out])
            c.batch_sync()
            done[how] = ev.query()
            S.synchronize()
    finally:
        c.set_stream(S)
    assert done == dict(own=False, caller=True), done                # on S the call waits for the chain; on the own stream it does not


def _cut_sequence(vislam, E, streams):
    """16 frames as 8 + 8 with every stage, vis_batch_track behind each launch; launch k on streams[k] -> (everything the host can read, timings)"""
    torch, c = E.torch, E.cP
    ap = vislam.default_align_params()
    import ctypes as C
    ar = C.sizeof(vislam.AlignResult)
    bufs = [dict(align=torch.empty(so.B * ar, dtype=torch.uint8, device="cuda"), track=torch.empty(so.B * 32, dtype=torch.uint8, device="cuda")) for _ in range(2)]
    for d in bufs:
        for t in d.values():
            t.fill_(so.FILL)
    torch.cuda.synchronize()
    c.batch_reset()
    E.pinned.clear()
    got, tm = {}, []
    for k in range(2):
        c.set_stream(streams[k])
        c.batch_run(E.frames.ptr(k), so.B, so.ALL_GRAD)
        c.batch_track(ap, E.frames.ptr(k), so.B, 0, bufs[k]["align"].data_ptr(), bufs[k]["track"].data_ptr())
        E.pinned.queue(c, k)
        if k == 1:
            c.batch_sync()
            tm.append(c.timings())
            got["tau"] = c.batch_fast_thresholds()[0].tobytes()
    assert c.batch_status() == 0
    got.update(so.plan_state(vislam, c))
    got.update(E.pinned.read())
    for k in range(2):
        got.update({f"{n}{k}": t.cpu().numpy().tobytes() for n, t in bufs[k].items()})
    return got, tm[0]


def test_a_stream_cut_between_the_own_and_a_caller_stream(vislam, env):
    S = env.S
    try:
        base, tm0 = _cut_sequence(vislam, env, (0, 0))
        for streams in ((0, S), (S, 0), (S, S)):
            got, tm = _cut_sequence(vislam, env, streams)
            for k in base:
                assert got[k] == base[k], (k, streams)
            ms = [getattr(tm, f) for f, _ in tm._fields_ if f.startswith("ms_")]
            assert all(math.isfinite(v) and v >= 0.0 for v in ms), (streams, ms)
            assert tm.launches_total == tm0.launches_total > 0 and tm.launches_fast == tm0.launches_fast
        track = np.frombuffer(base["track1"], np.dtype([("pose", "<f4", (7,)), ("composed", "<i4")]))
        assert (track["composed"] != vislam.TRACK_NONE).all()        # the chain crossed the cut
    finally:
        env.cP.set_stream(S)


def test_close_with_the_caller_stream_still_set(vislam, env):
    torch, S = env.torch, env.S
    c = vislam.Context(0)
    c.set_stream(S)
    case = so.case_f2f(vislam, torch, c)
    rig = so.Rig(torch, case)
    want, _ = so.run_sync(torch, c, rig)
    rig.load()
    case.call(c, rig.p)                                              # work still queued on S when the context goes
    c.close()
    with torch.cuda.stream(S):
        got = rig.out["rec"].clone()
    S.synchronize()
    assert got.cpu().numpy()[:so.NR * 32].tobytes() == want["rec"]
