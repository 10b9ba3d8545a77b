"""The late-producer rig of tests/test_caller_stream_gpu.py and its cases: every asynchronous entry point of include/vislam_hip.h that
reads caller device memory, called on a caller's stream S (vis_set_stream) while the producer of its inputs is still pending on S.

A case is a list of caller INPUT buffers, each with its real content and a decoy, a list of OUTPUT buffers, and the library call(s).  The
rig runs it three ways on ONE context whose stream is S:
  sync    inputs loaded and host-synchronised, the call, vis_batch_sync                      (tests compare against this; it also grows workspaces)
  late    decoys loaded and synchronised; then on S: a delay chain, device-to-device copies of the real inputs over the decoys, an event;
          the call with no host synchronisation; `not event.query()` right after it returns (the producer was still pending when the call
          was queued: only stream order can make it see the real inputs); the consumer -- outputs cloned on S for a call the header places
          on the context's stream, vis_batch_sync for a call it places on the pose / match stream
  decoy   the sync run with ONE input replaced by its decoy, per input: its bytes must differ from the real run's, else a stale read of that
          input could not show
Shapes are the smallest that reach the code: plans of 320 x 240 with B = 8 over two launches, rows of at most 96 points (one row longer than 64:
the lane-parallel RANSAC kernels switch from one wave to four there) in 6 rows."""
import ctypes as C
import math
import time

import numpy as np

import f2f_ref
import homography_ref as hr
import pnp_ref as pr
import stride_range_cases as src

FILL = 0xEE
W, H, B = 320, 240, 8
NR, MAX_PTS = 6, 96
ROW_M = (40, 96, 70, 5, 64, 33)                # valid points per row: one row of 96 > 64, one at 64, one below every minimal sample but F2F's
MC = 49                                         # correspondences per pair of a plan: floor(sqrt(n_cells))^2 with the default n_cells
CTX, POSE = "context stream", "pose stream"    # where the header places a call = how its outputs may be read
FACTOR, CHAIN_MAX_MS = 20.0, 200.0


# ------------------------------------------------------------------------------------------------------------ the delay chain
class Delay:
    """a chain of cheap elementwise torch ops over one large tensor, queued on S; sized by the module fixture"""

    def __init__(self, torch, stream, nbytes=1 << 29):
        self.torch, self.S = torch, stream
        self.x = torch.zeros(nbytes // 4, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        self.n_ops, self.op_ms, self.host_ms = 0, 0.0, 0.0

    def queue(self, n=None):
        """(the caller is inside torch.cuda.stream(S))"""
        for _ in range(self.n_ops if n is None else n):
            self.x.add_(1)

    def measure(self, n=32):
        """device milliseconds of one op, from torch events around n of them (after n unmeasured ones: clocks up, allocator quiet)"""
        torch = self.torch
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(self.S):
            self.queue(n)
            a.record(self.S)
            self.queue(n)
            b.record(self.S)
        self.S.synchronize()
        self.op_ms = a.elapsed_time(b) / n
        return self.op_ms

    def size(self, host_ms):
        """the chain is at least FACTOR x host_ms long, and at least 64 ops; (chain_ms, ok)"""
        self.host_ms = host_ms
        self.n_ops = max(64, int(math.ceil(FACTOR * host_ms / self.op_ms)))
        return self.n_ops * self.op_ms, self.n_ops * self.op_ms <= CHAIN_MAX_MS

    @property
    def chain_ms(self):
        return self.n_ops * self.op_ms


# ------------------------------------------------------------------------------------------------------------ buffers
def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


def fetch(ptr, nbytes):
    """nbytes of device memory the library owns (the plan's pyramids and gradients), after a synchronisation"""
    hip = C.CDLL("libamdhip64.so")
    host = np.empty(nbytes, np.uint8)
    assert hip.hipMemcpy(C.c_void_p(host.ctypes.data), C.c_void_p(ptr), C.c_size_t(nbytes), 2) == 0     # device to host
    return host


class Case:
    """inputs {name: (real, decoy)} numpy arrays of equal size; outputs {name: bytes}; scratch {name: bytes}: buffers `prepare` fills (synchronised,
    before the producer is queued) for `call` to read; call(c, p) / prepare(c, p) take p(name) -> device pointer; read(c) -> {name: bytes} of what
    only host getters reach, after the synchronisation; where = CTX or POSE; after = the names overwritten with their decoys on S right behind
    the call (the reuse rule of vis_batch_run's d_frames)"""

    def __init__(self, name, where, inputs, outputs, call, prepare=None, scratch=None, read=None, after=()):
        self.name, self.where, self.inputs, self.outputs, self.call = name, where, inputs, outputs, call
        self.prepare, self.scratch, self.read, self.after = prepare, scratch or {}, read, tuple(after)
        for k, (r, d) in inputs.items():
            assert _bytes(r).size == _bytes(d).size > 0 and _bytes(r).tobytes() != _bytes(d).tobytes(), (name, k)


class Rig:
    """the device buffers of one case: per input the buffer the call reads and its staged twins (real, decoy); per output a buffer of FILL"""

    def __init__(self, torch, case):
        self.torch, self.case = torch, case
        up = lambda a: torch.from_numpy(_bytes(a).copy()).cuda()
        self.real = {k: up(r) for k, (r, d) in case.inputs.items()}
        self.decoy = {k: up(d) for k, (r, d) in case.inputs.items()}
        self.buf = {k: torch.empty_like(v) for k, v in self.real.items()}
        self.out = {k: torch.empty(max(n, 16), dtype=torch.uint8, device="cuda") for k, n in list(case.outputs.items()) + list(case.scratch.items())}
        torch.cuda.synchronize()

    def p(self, name):
        return (self.buf[name] if name in self.buf else self.out[name]).data_ptr()

    def load(self, decoyed=()):
        """every input = its real content, those named in `decoyed` (or all: True) their decoy; outputs = FILL; host-synchronised"""
        torch = self.torch
        torch.cuda.synchronize()
        for k in self.buf:
            self.buf[k].copy_(self.decoy[k] if decoyed is True or k in decoyed else self.real[k])
        for t in self.out.values():
            t.fill_(FILL)
        torch.cuda.synchronize()

    def outputs(self, c, src_=None):
        got = {k: (src_ or self.out)[k].cpu().numpy()[:n].tobytes() for k, n in self.case.outputs.items()}
        if self.case.read:
            got.update(self.case.read(c))
        return got


def run_sync(torch, c, rig, decoyed=()):
    """-> ({output name: bytes}, host milliseconds of the call sequence)"""
    case = rig.case
    rig.load(decoyed)
    if case.prepare:
        case.prepare(c, rig.p)
    c.batch_sync()
    t0 = time.perf_counter()
    case.call(c, rig.p)
    host_ms = (time.perf_counter() - t0) * 1e3
    c.batch_sync()
    torch.cuda.synchronize()
    if getattr(c, "_stream_order_has_plan", False):
        assert c.batch_status() == 0
    return rig.outputs(c), host_ms


def run_late(torch, c, S, delay, rig):
    """-> ({output name: bytes}, late, host milliseconds of the call sequence): late = the producer's event had not completed when the call returned"""
    case = rig.case
    rig.load(True)
    if case.prepare:
        case.prepare(c, rig.p)
    c.batch_sync()
    torch.cuda.synchronize()
    ev = torch.cuda.Event()
    with torch.cuda.stream(S):
        delay.queue()
        for k in rig.buf:
            rig.buf[k].copy_(rig.real[k])                            # device to device, behind the chain
        ev.record(S)
    t0 = time.perf_counter()
    case.call(c, rig.p)
    late = not ev.query()
    host_ms = (time.perf_counter() - t0) * 1e3
    clones = None
    with torch.cuda.stream(S):
        if case.where == CTX:
            clones = {k: rig.out[k].clone() for k in case.outputs}   # the consumer: on S right behind the call, no host synchronisation
        for k in case.after:                                         # the caller reuses its buffers right behind the call
            if k in rig.buf:
                rig.buf[k].copy_(rig.decoy[k])
            else:
                rig.out[k].fill_(128)
    if case.where == CTX:
        S.synchronize()
        got = rig.outputs(c, clones)
        c.batch_sync()
    else:
        c.batch_sync()                                               # the header: outputs of the pose / match stream are read after vis_batch_sync
        got = rig.outputs(c)
    torch.cuda.synchronize()
    return got, late, host_ms


# ------------------------------------------------------------------------------------------------------------ shared data
_cache = {}


def plan_frames(vislam, canvas):
    """16 frames of the parallax stream at 320 x 240 (two launches of 8) and their decoy: flat frames of 128"""
    if "frames" not in _cache:
        f = np.stack([vislam.synth_frame(canvas, t, W, H, parallax=True) for t in range(2 * B)])
        _cache["frames"] = (f, np.full_like(f, 128))
    return _cache["frames"]


def two_view_rows():
    """(p1, p2 NR x MAX_PTS x 2 float32, npts, rot NR x 9 float32, t NR x 3 float32): f2f_ref.pair_inputs per row, noise and outliers in"""
    if "rows" not in _cache:
        p1, p2 = np.zeros((NR, MAX_PTS, 2), np.float32), np.zeros((NR, MAX_PTS, 2), np.float32)
        rot, t = np.zeros((NR, 9), np.float32), np.zeros((NR, 3), np.float32)
        for i, m in enumerate(ROW_M):
            a, b, r, tt = f2f_ref.pair_inputs(m, 300 + i, 0.1, 0.5)
            p1[i, :m], p2[i, :m], rot[i], t[i] = a, b, r.reshape(9), tt
        _cache["rows"] = (p1, p2, np.array(ROW_M, np.int32), rot, t)
    return _cache["rows"]


def plane_rows():
    """(p1, p2, npts): homography_ref.make_rows of the planar classes, so that a homography wins and its pose has candidates to choose from"""
    if "plane" not in _cache:
        p1, p2 = np.zeros((NR, MAX_PTS, 2), np.float32), np.zeros((NR, MAX_PTS, 2), np.float32)
        for i, m in enumerate(ROW_M):
            a, b, _ = hr.make_rows(("plane", "tilted")[i % 2], m, 0.3, 0.1, 400 + i)
            p1[i, :m], p2[i, :m] = a, b
        _cache["plane"] = (p1, p2, np.array(ROW_M, np.int32))
    return _cache["plane"]


def zeros(a):
    return np.zeros_like(a)


def eye_rows(n):
    return np.tile(np.eye(3, dtype=np.float32).reshape(9), (n, 1))


def f2f_draws(seed, iters=1000):
    return np.random.default_rng(seed).integers(0, 2 ** 31, (iters, 2)).astype(np.int32)


def hint_params(vislam):
    """every candidate with a vote is a rival, so that the rotation hint decides every PLANE pair"""
    hq = vislam.default_hpose_params()
    hq.ambiguity_ratio = 1e-6
    return hq


def _download(torch, c, sizes, run):
    """run(pointer of name) queued on host-synchronised buffers of FILL -> {name: numpy bytes}: how a case's build makes the inputs that an
    upstream call of the library writes (the records a polish reads, the gradients an alignment reads)"""
    bufs = {k: torch.full((max(n, 16),), FILL, dtype=torch.uint8, device="cuda") for k, n in sizes.items()}
    torch.cuda.synchronize()
    run(lambda k: bufs[k].data_ptr())
    c.batch_sync()
    torch.cuda.synchronize()
    return {k: bufs[k].cpu().numpy()[:n].copy() for k, n in sizes.items()}


def _upload(torch, a):
    t = torch.from_numpy(_bytes(a).copy()).cuda()
    torch.cuda.synchronize()
    return t


# ------------------------------------------------------------------------------------------------------------ group A: rows on the context's stream
def case_f2f(vislam, torch, c):
    p1, p2, n, rot, t = two_view_rows()
    ins = dict(p1=(p1, zeros(p1)), p2=(p2, zeros(p2)), npts=(n, zeros(n)), rot=(rot, eye_rows(NR)), tref=(t, -t), draws=(f2f_draws(1), f2f_draws(2)))
    return Case("vis_f2f_batch", CTX, ins, dict(rec=NR * 32),
                lambda c, p: c.f2f_batch(NR, p("p1"), p("p2"), p("npts"), MAX_PTS, p("rot"), p("tref"), p("draws"), p("rec")))


def case_filter(vislam, torch, c):
    p1, p2, n, rot, t = two_view_rows()
    other = np.roll(t, 1, axis=1).copy()
    ins = dict(p1=(p1, zeros(p1)), p2=(p2, zeros(p2)), npts=(n, zeros(n)), rot=(rot, eye_rows(NR)), t=(t, other))
    return Case("vis_filter_keypoints_batch", CTX, ins, dict(keep=NR * MAX_PTS, nkeep=NR * 4),
                lambda c, p: c.filter_keypoints_batch(NR, p("p1"), p("p2"), p("npts"), MAX_PTS, p("rot"), p("t"), 500.0, MAX_PTS, p("keep"), p("nkeep")))


def case_homography(vislam, torch, c):
    p1, p2, n = plane_rows()
    ins = dict(p1=(p1, zeros(p1)), p2=(p2, zeros(p2)), npts=(n, zeros(n)), draws=(hr.make_draws(7), hr.make_draws(8)))
    return Case("vis_homography_batch", CTX, ins, dict(mask=NR * MAX_PTS, rec=NR * 112),
                lambda c, p: c.homography_batch(NR, p("p1"), p("p2"), p("npts"), MAX_PTS, p("draws"), 0, MAX_PTS, p("mask"), p("rec")))


def _homography_records(vislam, torch, c):
    """(records, mask rows) of vis_homography_batch on plane_rows, synchronised: the inputs of the polish and of the pose"""
    if "hrec" not in _cache:
        p1, p2, n = plane_rows()
        d = [_upload(torch, a) for a in (p1, p2, n, hr.make_draws(7))]
        got = _download(torch, c, dict(mask=NR * MAX_PTS, rec=NR * 112),
                        lambda q: c.homography_batch(NR, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), MAX_PTS, d[3].data_ptr(), 0, MAX_PTS, q("mask"), q("rec")))
        recs = got["rec"].view(vislam.HOMOGRAPHY_RESULT_DTYPE)
        assert (recs["best_iter"][[0, 1, 2, 4, 5]] >= 0).all(), recs        # (not a polish of empty records)
        _cache["hrec"] = (got["rec"], got["mask"])
    return _cache["hrec"]


def case_homography_polish(vislam, torch, c):
    p1, p2, n = plane_rows()
    h, m = _homography_records(vislam, torch, c)
    ins = dict(h=(h, zeros(h)), p1=(p1, zeros(p1)), p2=(p2, zeros(p2)), npts=(n, zeros(n)), mask=(m, zeros(m)))
    return Case("vis_homography_polish_batch", CTX, ins, dict(mask_out=NR * MAX_PTS, rec=NR * 128, h_out=NR * 112),
                lambda c, p: c.homography_polish_batch(NR, p("h"), p("p1"), p("p2"), p("npts"), MAX_PTS, MAX_PTS, p("mask"), p("mask_out"), p("rec"), p("h_out")))


def case_homography_pose(vislam, torch, c):
    p1, p2, n = plane_rows()
    h, m = _homography_records(vislam, torch, c)
    hq = hint_params(vislam)
    ins = dict(h=(h, zeros(h)), p1=(p1, zeros(p1)), p2=(p2, zeros(p2)), npts=(n, zeros(n)), mask=(m, zeros(m)), rot=(eye_rows(NR), -eye_rows(NR)))
    return Case("vis_homography_pose_batch", CTX, ins, dict(rec=NR * 320),
                lambda c, p: c.homography_pose_batch(NR, p("h"), p("p1"), p("p2"), p("npts"), MAX_PTS, MAX_PTS, p("mask"), p("rot"), p("rec"), hq))


def case_essential(vislam, torch, c):
    p1, p2, n, _, _ = two_view_rows()
    ins = dict(p1=(p1, zeros(p1)), p2=(p2, zeros(p2)), npts=(n, zeros(n)))
    return Case("vis_essential_batch", CTX, ins, dict(mask=NR * MAX_PTS, rec=NR * 192),
                lambda c, p: c.essential_batch(NR, p("p1"), p("p2"), p("npts"), MAX_PTS, MAX_PTS, p("mask"), p("rec")))


def _pose_records(vislam, torch, c):
    if "pose" not in _cache:
        p1, p2, n, _, _ = two_view_rows()
        d = [_upload(torch, a) for a in (p1, p2, n)]
        got = _download(torch, c, dict(mask=NR * MAX_PTS, rec=NR * 192),
                        lambda q: c.essential_batch(NR, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), MAX_PTS, MAX_PTS, q("mask"), q("rec")))
        recs = got["rec"].view(vislam.POSE_RESULT_DTYPE)
        assert (recs["n_inliers"][[0, 1, 2, 4, 5]] >= 8).all(), recs["n_inliers"]
        _cache["pose"] = (got["rec"], got["mask"])
    return _cache["pose"]


def case_essential_refine(vislam, torch, c):
    p1, p2, n, _, _ = two_view_rows()
    r, m = _pose_records(vislam, torch, c)
    ins = dict(pose=(r, zeros(r)), p1=(p1, zeros(p1)), p2=(p2, zeros(p2)), npts=(n, zeros(n)), mask=(m, zeros(m)))
    return Case("vis_essential_refine_batch", CTX, ins, dict(rec=NR * 216),
                lambda c, p: c.essential_refine_batch(NR, p("pose"), p("p1"), p("p2"), p("npts"), MAX_PTS, MAX_PTS, p("mask"), p("rec")))


def case_essential_polish(vislam, torch, c):
    p1, p2, n, _, _ = two_view_rows()
    r, m = _pose_records(vislam, torch, c)
    ins = dict(pose=(r, zeros(r)), p1=(p1, zeros(p1)), p2=(p2, zeros(p2)), npts=(n, zeros(n)), mask=(m, zeros(m)))
    return Case("vis_essential_polish_batch", CTX, ins, dict(mask_out=NR * MAX_PTS, rec=NR * 224, pose_out=NR * 192),
                lambda c, p: c.essential_polish_batch(NR, p("pose"), p("p1"), p("p2"), p("npts"), MAX_PTS, MAX_PTS, p("mask"), p("mask_out"), p("rec"),
                                                      p("pose_out")))


def case_pnp(vislam, torch, c):
    X, xy = np.zeros((NR, MAX_PTS, 3)), np.zeros((NR, MAX_PTS, 2), np.float32)
    for i, m in enumerate(ROW_M):
        a, b, _, _, _ = pr.make_scene(("general", "tilted")[i % 2], max(m, 8), 0.3, 0.1, 500 + i)
        X[i, :m], xy[i, :m] = a[:m], b[:m]
    n = np.array(ROW_M, np.int32)
    ins = dict(X=(X, zeros(X)), xy=(xy, zeros(xy)), npts=(n, zeros(n)), draws=(pr.make_draws(7), pr.make_draws(8)))
    return Case("vis_pnp_batch", CTX, ins, dict(mask=NR * MAX_PTS, rec=NR * 240),
                lambda c, p: c.pnp_batch(NR, p("X"), 3, p("xy"), p("npts"), MAX_PTS, p("draws"), MAX_PTS, p("mask"), p("rec")))


# ------------------------------------------------------------------------------------------------------------ group A: frames on the context's stream
NF = 3                                          # frames of the frame-shaped calls: pairs (0 -> 1) and (1 -> 2)


def _fe(vislam):
    return vislam.gradient_frame_elems(W, H)


def case_gradient(vislam, torch, c, canvas):
    f, flat = plan_frames(vislam, canvas)
    fe = _fe(vislam)
    return Case("vis_gradient_batch", CTX, dict(frames=(f[:NF], flat[:NF])), dict(gray=NF * fe, gx=NF * fe * 2, gy=NF * fe * 2, g=NF * fe),
                lambda c, p: c.gradient_batch(p("frames"), W, H, W, NF, p("gray"), p("gx"), p("gy"), p("g")))


def _gradient_set(vislam, torch, c, canvas):
    """(gray, gx, gy) bytes of vis_gradient_batch on the first NF frames, synchronised; gray's level-0 part zeroed (the call leaves it alone)"""
    if "grad" not in _cache:
        f, _ = plan_frames(vislam, canvas)
        fe = _fe(vislam)
        d = _upload(torch, f[:NF])
        got = _download(torch, c, dict(gray=NF * fe, gx=NF * fe * 2, gy=NF * fe * 2, g=NF * fe),
                        lambda q: c.gradient_batch(d.data_ptr(), W, H, W, NF, q("gray"), q("gx"), q("gy"), q("g")))
        got["gray"].reshape(NF, fe)[:, :W * H] = 0
        _cache["grad"] = (got["gray"], got["gx"], got["gy"])
    return _cache["grad"]


def grid_points(n, m, seed):
    """n rows of m points inside the frame, a margin of 24 px from its border"""
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(24.0, W - 24.0, (n, m)), rng.uniform(24.0, H - 24.0, (n, m))], 2).astype(np.float32)


def _klt_inputs(vislam, torch, c, canvas):
    f, flat = plan_frames(vislam, canvas)
    gray, gx, gy = _gradient_set(vislam, torch, c, canvas)
    pts, other = grid_points(NF, MAX_PTS, 11), grid_points(NF, MAX_PTS, 12)
    n = np.array([0, MAX_PTS, 70], np.int32)
    guess = pts + np.float32(1.5)
    return dict(frames=(f[:NF], flat[:NF]), gray=(gray, zeros(gray)), gx=(gx, zeros(gx)), gy=(gy, zeros(gy)), pts=(pts, other), npts=(n, zeros(n)),
                guess=(guess, np.full_like(guess, np.nan)))


def _klt_params(vislam):
    kp = vislam.default_klt_params()
    kp.fb_max_px = 1.0                                               # the forward-backward pass reads the second frame's gradients as well
    return kp


def case_klt(vislam, torch, c, canvas):
    kp = _klt_params(vislam)
    outs = dict(rec=NF * MAX_PTS * 32, pair=NF * 32, k1=NF * MAX_PTS * 8, k2=NF * MAX_PTS * 8, nt=NF * 4)
    return Case("vis_klt_batch", CTX, _klt_inputs(vislam, torch, c, canvas), outs,
                lambda c, p: c.klt_batch(p("frames"), W, H, W, NF, p("gray"), p("gx"), p("gy"), p("pts"), p("npts"), MAX_PTS, p("rec"), p("pair"), p("guess"),
                                         p("k1"), p("k2"), p("nt"), kp))


def case_klt_chain(vislam, torch, c, canvas):
    """vis_klt_batch -> vis_homography_batch -> vis_homography_polish_batch -> vis_homography_pose_batch on S, each reading what the one before wrote,
    no host synchronisation between them"""
    kp = _klt_params(vislam)
    ins = _klt_inputs(vislam, torch, c, canvas)
    ins["draws"] = (hr.make_draws(7), hr.make_draws(8))
    outs = dict(rec=NF * MAX_PTS * 32, pair=NF * 32, k1=NF * MAX_PTS * 8, k2=NF * MAX_PTS * 8, nt=NF * 4, hmask=NF * MAX_PTS, h=NF * 112,
                qmask=NF * MAX_PTS, q=NF * 128, qh=NF * 112, pose=NF * 320)

    def call(c, p):
        c.klt_batch(p("frames"), W, H, W, NF, p("gray"), p("gx"), p("gy"), p("pts"), p("npts"), MAX_PTS, p("rec"), p("pair"), p("guess"), p("k1"), p("k2"),
                    p("nt"), kp)
        c.homography_batch(NF, p("k1"), p("k2"), p("nt"), MAX_PTS, p("draws"), 0, MAX_PTS, p("hmask"), p("h"))
        c.homography_polish_batch(NF, p("h"), p("k1"), p("k2"), p("nt"), MAX_PTS, MAX_PTS, p("hmask"), p("qmask"), p("q"), p("qh"))
        c.homography_pose_batch(NF, p("qh"), p("k1"), p("k2"), p("nt"), MAX_PTS, MAX_PTS, p("qmask"), 0, p("pose"))
    return Case("klt -> homography -> polish -> pose", CTX, ins, outs, call)


def align_params(vislam):
    ap = vislam.default_align_params()
    ap.fx = ap.fy = 200.0
    ap.cx, ap.cy = W / 2.0, H / 2.0
    return ap


def small_poses(n, seed):
    """n Se3f records (28 bytes each) a little off the identity"""
    rng = np.random.default_rng(seed)
    out = np.zeros((n, 7), np.float32)
    for i in range(n):
        w = rng.normal(0, 0.004, 3)
        q = np.concatenate([w / 2, [1.0]])
        out[i, :4] = q / np.linalg.norm(q)
        out[i, 4:] = rng.normal(0, 0.01, 3)
    return out


def identity_poses(n):
    out = np.zeros((n, 7), np.float32)
    out[:, 3] = 1.0
    return out


def case_align(vislam, torch, c, canvas):
    f, flat = plan_frames(vislam, canvas)
    gray, gx, gy = _gradient_set(vislam, torch, c, canvas)
    pts, other = grid_points(NF, MAX_PTS, 21), grid_points(NF, MAX_PTS, 22)
    n = np.array([0, MAX_PTS, 70], np.int32)
    ap = align_params(vislam)
    ins = dict(frames=(f[:NF], flat[:NF]), gray=(gray, zeros(gray)), gx=(gx, zeros(gx)), gy=(gy, zeros(gy)), pts=(pts, other), npts=(n, zeros(n)),
               init=(small_poses(NF, 3), identity_poses(NF)))
    return Case("vis_align_batch", CTX, ins, dict(rec=NF * C.sizeof(vislam.AlignResult)),
                lambda c, p: c.align_batch(ap, p("frames"), W, H, W, NF, p("gray"), p("gx"), p("gy"), p("pts"), p("npts"), MAX_PTS, p("init"), p("rec")))


def case_synth(vislam, torch, c, canvas):
    cv = np.ascontiguousarray(canvas, np.uint8)
    dim = cv.shape[0]
    return Case("vis_synth_frames_device", CTX, dict(canvas=(cv, zeros(cv))), dict(frames=NF * W * H),
                lambda c, p: c.synth_frames_device(p("canvas"), dim, 0xE0C00001, 3, NF, W, H, W, p("frames"), True))


RECT_K, RECT_D = (200.0, 199.4, 160.1, 124.2), (-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05)


def make_rectifier(vislam, c):
    kn = vislam.optimal_new_camera_matrix(RECT_K, RECT_D, (W, H), (W, H))
    return c.rectify(RECT_K, RECT_D, kn, (W, H), (W, H))


def case_rectify(vislam, torch, c, canvas, rectifier):
    f, flat = plan_frames(vislam, canvas)
    return Case("vis_rectify_batch", CTX, dict(raw=(f[:NF], flat[:NF])), dict(rect=NF * W * H),
                lambda c, p: rectifier.batch(p("raw"), W, NF, p("rect"), W))


# ------------------------------------------------------------------------------------------------------------ group A: feature-track rows
FT_N, FT_K = 5, 80                              # frames, keypoints per frame (= row_cap = link_cap)


def ftrack_scene():
    """5 frames of 80 keypoints: keypoint k of every frame is map point k seen from a camera moving along x; the match lists link k -> k and drop
    every seventh keypoint (another one per frame), so tracks end and start inside the call.  (prev, nkp, links, nlinks, xy, poses)"""
    if "ft" not in _cache:
        rng = np.random.default_rng(31)
        X = np.stack([rng.uniform(-2, 2, FT_K), rng.uniform(-1.5, 1.5, FT_K), rng.uniform(4, 9, FT_K)], 1)
        prev = np.array([-3] + list(range(FT_N - 1)), np.int32)       # VIS_KF_FIRST, then the frame before
        nkp = np.full(FT_N, FT_K, np.int32)
        links = np.zeros((FT_N, FT_K), [("queryIdx", "<i4"), ("trainIdx", "<i4"), ("imgIdx", "<i4"), ("distance", "<f4")])
        nlinks = np.zeros(FT_N, np.int32)
        xy, poses = np.zeros((FT_N, FT_K, 2), np.float32), np.zeros((FT_N, 12))
        for i in range(FT_N):
            keep = [k for k in range(FT_K) if (k + i) % 7] if i else []
            nlinks[i] = len(keep)
            links["queryIdx"][i, :len(keep)] = links["trainIdx"][i, :len(keep)] = keep
            links["distance"][i, :len(keep)] = 10.0
            t = np.array([-0.3 * i, 0.0, 0.0])
            poses[i, :9], poses[i, 9:] = np.eye(3).reshape(9), t
            xc = X + t
            xy[i, :, 0] = 458.654 * xc[:, 0] / xc[:, 2] + 367.215
            xy[i, :, 1] = 457.296 * xc[:, 1] / xc[:, 2] + 248.375
        _cache["ft"] = (prev, nkp, links, nlinks, xy, poses)
    return _cache["ft"]


def case_ftrack_link(vislam, torch, c):
    prev, nkp, links, nlinks, _, _ = ftrack_scene()
    other = links.copy()
    other["trainIdx"] = (other["trainIdx"] + 1) % FT_K
    none = np.full_like(prev, -3)
    ins = dict(prev=(prev, none), nkp=(nkp, np.full_like(nkp, FT_K // 2)), links=(links, other), nlinks=(nlinks, zeros(nlinks)))
    return Case("vis_ftrack_link_rows", CTX, ins, dict(obs=FT_N * FT_K * 16, frame=FT_N * 32),
                lambda c, p: c.ftrack_link_rows(FT_N, p("prev"), p("nkp"), p("links"), p("nlinks"), FT_K, FT_K, p("obs"), p("frame")))


def case_ftrack_triangulate(vislam, torch, c):
    prev, nkp, links, nlinks, xy, poses = ftrack_scene()
    if "ftobs" not in _cache:
        d = [_upload(torch, a) for a in (prev, nkp, links, nlinks)]
        got = _download(torch, c, dict(obs=FT_N * FT_K * 16, frame=FT_N * 32),
                        lambda q: c.ftrack_link_rows(FT_N, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), FT_K, FT_K, q("obs"), q("frame")))
        _cache["ftobs"] = got["obs"]
    obs = _cache["ftobs"]
    alone = np.tile(np.array([-1, -1, 0, -1], np.int32), FT_N * FT_K)  # every keypoint a track of its own: nothing to triangulate
    none = np.full_like(prev, -3)
    ins = dict(prev=(prev, none), nkp=(nkp, np.full_like(nkp, FT_K // 2)), obs=(obs, alone), xy=(xy, xy[::-1].copy()), poses=(poses, zeros(poses)))
    return Case("vis_ftrack_triangulate_rows", CTX, ins, dict(points=FT_N * FT_K * 40, flags=FT_N * FT_K, summary=FT_N * 32),
                lambda c, p: c.ftrack_triangulate_rows(FT_N, p("prev"), p("nkp"), p("obs"), FT_K, p("xy"), p("poses"), p("points"), p("flags"), p("summary")))


# ------------------------------------------------------------------------------------------------------------ groups B and C: the plan
ALL_GRAD = 7 | 16                               # VIS_STAGE_ALL | VIS_STAGE_GRADIENT


def plan_context(vislam):
    p = src.plan_params(vislam, W, H, False)
    c = vislam.Context(0, p)
    c.batch_plan(W, H, W, B)
    c._stream_order_has_plan = True
    return c


def plan_state(vislam, c):
    """what only host getters reach of the last launch (after a synchronisation): keypoints and descriptors, both 2-NN lists, the good matches and
    the pose of every frame, the half pyramid and the gradients"""
    got = {}
    for i in range(B):
        k, d = c.batch_keypoints(i)
        o12, o21 = c.batch_knn(i)
        g, ns = c.batch_matches(i)
        q = c.batch_pose(i)
        if i == 0:
            got["keypoints0"], got["descriptors0"] = k.tobytes(), d.tobytes()
        got[f"frame{i}"] = b"".join([k.tobytes(), d.tobytes(), o12.tobytes(), o21.tobytes(), g.tobytes(), np.int32(ns).tobytes(), q["E"].tobytes(),
                                     q["R"].tobytes(), q["t"].tobytes(), np.array([q["n_inliers"], q["n_pose_good"], q["iters_run"]], np.int32).tobytes()])
    gray, gx, gy, g, fe = c.batch_gradients()
    got["half"], got["gx"], got["gy"], got["g"] = fetch(gray, B * fe).tobytes(), fetch(gx, B * fe * 2).tobytes(), fetch(gy, B * fe * 2).tobytes(), fetch(g, B * fe).tobytes()
    return got


class Pinned:
    """pinned host buffers for vis_batch_results_async of two launches (pageable memory would make the copy block the host)"""

    def __init__(self, vislam, torch):
        self.sizes = dict(pose=B * vislam.POSE_RESULT_DTYPE.itemsize, good=B * MC * 16, ngood=B * 4)
        self.t = [{k: torch.empty(n, dtype=torch.uint8).pin_memory() for k, n in self.sizes.items()} for _ in range(2)]

    def clear(self):
        for d in self.t:
            for v in d.values():
                v.fill_(FILL)

    def queue(self, c, launch):
        d = self.t[launch]
        c.batch_results_async(B, d["pose"].data_ptr(), d["good"].data_ptr(), d["ngood"].data_ptr())

    def read(self):
        return {f"results{l}_{k}": v.numpy().tobytes() for l, d in enumerate(self.t) for k, v in d.items()}


def guide_rotations():
    """(real, decoy) 2 B x 9 float32: the identity (the stream barely rotates) and a turn of 0.3 rad about y, whose windows miss the matches"""
    a = 0.3
    turn = np.array([np.cos(a), 0, np.sin(a), 0, 1, 0, -np.sin(a), 0, np.cos(a)], np.float32)
    return eye_rows(2 * B), np.tile(turn, (2 * B, 1))


def case_batch_run(vislam, torch, c, canvas, pinned, guided=False, reuse=False):
    f, flat = plan_frames(vislam, canvas)
    ins = dict(frames=(f, flat))
    if guided:
        ins["rot"] = guide_rotations()

    def call(c, p):
        for l in range(2):
            ptr = p("frames") + l * B * W * H
            if guided:
                c.batch_run_guided(ptr, B, p("rot") + l * B * 36, 40.0, ALL_GRAD)
            else:
                c.batch_run(ptr, B, ALL_GRAD)
            pinned.queue(c, l)

    def prepare(c, p):
        c.batch_reset()
        pinned.clear()

    def read(c):
        got = plan_state(vislam, c)
        got.update(pinned.read())
        return got
    name = ("vis_batch_run_guided" if guided else "vis_batch_run") + (", d_frames overwritten behind it" if reuse else "")
    return Case(name, POSE, ins, {}, call, prepare, read=read, after=("frames",) if reuse else ())


def case_rectify_run(vislam, torch, c, canvas, pinned, rectifier):
    """vis_rectify_batch -> vis_batch_run on what it wrote, twice, and the raw and the rectified frames overwritten right behind the second run"""
    f, flat = plan_frames(vislam, canvas)
    ins = dict(raw=(f, flat))

    def call(c, p):
        for l in range(2):
            off = l * B * W * H
            rectifier.batch(p("raw") + off, W, B, p("rect") + off, W)
            c.batch_run(p("rect") + off, B, ALL_GRAD)
            pinned.queue(c, l)

    def prepare(c, p):
        c.batch_reset()
        pinned.clear()

    def read(c):
        got = plan_state(vislam, c)
        got.update(pinned.read())
        return got
    return Case("vis_rectify_batch -> vis_batch_run, both overwritten behind it", POSE, ins, {}, call, prepare, scratch=dict(rect=2 * B * W * H), read=read,
                after=("raw", "rect"))


class PlanFrames:
    """the 16 frames on the device, host-synchronised: group C's launches read them before the producer is queued"""

    def __init__(self, vislam, torch, canvas):
        self.t = _upload(torch, plan_frames(vislam, canvas)[0])

    def ptr(self, launch):
        return self.t.data_ptr() + launch * B * W * H


def _two_launches(fr, between=None):
    """prepare(): vis_batch_reset, launch 0, `between` (the follow-up a stream needs after EVERY launch), launch 1 -- all before the producer"""
    def prepare(c, p):
        c.batch_reset()
        c.batch_run(fr.ptr(0), B, ALL_GRAD)
        if between:
            between(c, p)
        c.batch_run(fr.ptr(1), B, ALL_GRAD)
    return prepare


def plan_cases(vislam, torch, c, fr):
    """group C: {name: Case}, every caller device input of a plan follow-up late on S, the result read after vis_batch_sync"""
    kc = c.keypoint_capacity(W, H)
    rng = np.random.default_rng(41)
    rot = f2f_ref.pair_inputs(8, 77, 0.0, 0.0)[2].reshape(9)
    rots = np.tile(rot, (B, 1)).astype(np.float32)
    tdir = rng.normal(0, 1, (B, 3)).astype(np.float32)
    cases = {}

    def add(case):
        cases[case.name] = case

    add(Case("vis_batch_f2f", POSE, dict(rot=(rots, eye_rows(B)), tref=(tdir, -tdir), draws=(f2f_draws(1), f2f_draws(2))), dict(rec=B * 32),
             lambda c, p: c.batch_f2f(B, p("rot"), p("tref"), p("draws"), p("rec")), _two_launches(fr)))
    # FilterKeypoints keeps |t . n| < 10^(-1000 / T) = 0.32 of unit normals: of these eight directions at least one keeps and one drops whatever the
    # normals of a pair are (a unit vector has a component >= 0.577, and (1, -1, 0) or another of the mixed ones is nearly orthogonal to it)
    axes = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [1, 0, 1], [0, 1, 1], [1, 1, 1], [1, -1, 0]], np.float32)
    quarter = np.tile(np.array([0, -1, 0, 1, 0, 0, 0, 0, 1], np.float32), (B, 1))     # a quarter turn about the optical axis: other epipolar planes
    add(Case("vis_batch_filter_keypoints", POSE, dict(rot=(eye_rows(B), quarter), t=(axes, np.roll(axes, 1, axis=0).copy())), dict(keep=B * MC, nkeep=B * 4),
             lambda c, p: c.batch_filter_keypoints(B, p("rot"), p("t"), 2000.0, MC, p("keep"), p("nkeep")), _two_launches(fr)))
    add(Case("vis_batch_homography", POSE, dict(draws=(hr.make_draws(7), hr.make_draws(8))), dict(mask=B * MC, rec=B * 112),
             lambda c, p: c.batch_homography(B, p("draws"), MC, p("mask"), p("rec")), _two_launches(fr)))

    d_draws = _upload(torch, hr.make_draws(7))
    cases["_keep"] = [d_draws]
    hq = hint_params(vislam)

    def hprepare(c, p):
        _two_launches(fr)(c, p)
        c.batch_homography(B, d_draws.data_ptr(), MC, p("hmask"), p("h"))
    add(Case("vis_batch_homography_pose", POSE, dict(rot=(eye_rows(B), -eye_rows(B))), dict(rec=B * 320),
             lambda c, p: c.batch_homography_pose(B, p("h"), MC, p("hmask"), p("rot"), p("rec"), hq), hprepare, scratch=dict(h=B * 112, hmask=B * MC)))

    # the polish reads the records and mask rows vis_batch_homography wrote into CALLER buffers: they are its late inputs
    def homography_of_launch_1():
        got = {}

        def run(q):
            _two_launches(fr)(c, q)
            c.batch_homography(B, d_draws.data_ptr(), MC, q("hmask"), q("h"))
        got = _download(torch, c, dict(h=B * 112, hmask=B * MC), run)
        return got["h"], got["hmask"]
    h, hm = homography_of_launch_1()
    add(Case("vis_batch_homography_polish", POSE, dict(h=(h, zeros(h)), hmask=(hm, zeros(hm))), dict(mask_out=B * MC, rec=B * 128, h_out=B * 112),
             lambda c, p: c.batch_homography_polish(B, p("h"), MC, p("hmask"), MC, p("mask_out"), p("rec"), p("h_out")), _two_launches(fr)))

    pp = vislam.default_pnp_params()
    pp.min_inliers = 6

    def pprepare(c, p):
        _two_launches(fr)(c, p)
        c.batch_triangulate(B, MC, p("points"), p("flags"), p("summary"))
    add(Case("vis_batch_pnp", POSE, dict(draws=(pr.make_draws(7), pr.make_draws(8))), dict(rec=B * 240, link=B * 120, mask=B * MC),
             lambda c, p: c.batch_pnp(B, p("draws"), p("points"), p("flags"), MC, p("rec"), p("link"), vislam.MP_KEPT, MC, p("mask"), pp), pprepare,
             scratch=dict(points=B * MC * 32, flags=B * MC, summary=B * 16)))

    mask = (rng.integers(0, 4, (B, kc)) > 0).astype(np.uint8)         # three of four symmetric matches linked
    link0 = lambda c, p: c.batch_ftrack(B, kc, p("obs0"), p("frame0"))
    add(Case("vis_batch_ftrack (d_mask)", POSE, dict(mask=(mask, np.ones_like(mask))), dict(obs=B * kc * 16, frame=B * 32),
             lambda c, p: c.batch_ftrack(B, kc, p("obs"), p("frame"), vislam.FT_SYM, False, p("mask"), kc), _two_launches(fr, link0),
             scratch=dict(obs0=B * kc * 16, frame0=B * 32)))

    poses = np.zeros((B, 12))
    for i in range(B):
        poses[i, :9], poses[i, 9:] = np.eye(3).reshape(9), [-0.05 * i, 0.0, 0.0]

    def tprepare(c, p):
        _two_launches(fr, link0)(c, p)
        c.batch_ftrack(B, kc, p("obs"), p("frame"))
    add(Case("vis_batch_ftrack_triangulate", POSE, dict(poses=(poses, zeros(poses))), dict(points=B * kc * 40, flags=B * kc, summary=B * 32),
             lambda c, p: c.batch_ftrack_triangulate(B, p("obs"), kc, p("poses"), p("points"), p("flags"), p("summary")), tprepare,
             scratch=dict(obs0=B * kc * 16, frame0=B * 32, obs=B * kc * 16, frame=B * 32)))

    kp = _klt_params(vislam)
    guess = np.stack([rng.uniform(24.0, W - 24.0, (B, kc)), rng.uniform(24.0, H - 24.0, (B, kc))], 2).astype(np.float32)
    add(Case("vis_batch_klt", POSE, dict(guess=(guess, np.full_like(guess, np.nan))),
             dict(rec=B * kc * 32, pair=B * 32, k1=B * kc * 8, k2=B * kc * 8, nt=B * 4),
             lambda c, p: c.batch_klt(fr.ptr(1), B, kc, p("rec"), p("pair"), p("guess"), p("k1"), p("k2"), p("nt"), kp), _two_launches(fr)))

    ap = vislam.default_align_params()
    ar = C.sizeof(vislam.AlignResult)
    init = (small_poses(B, 5), identity_poses(B))
    add(Case("vis_batch_align", POSE, dict(init=init), dict(rec=B * ar),
             lambda c, p: c.batch_align(ap, fr.ptr(1), B, 0, 0, 0, p("init"), p("rec")), _two_launches(fr)))
    track0 = lambda c, p: c.batch_track(ap, fr.ptr(0), B, 0, p("align0"), p("track0"))
    add(Case("vis_batch_track", POSE, dict(init=init), dict(align=B * ar, track=B * 32),
             lambda c, p: c.batch_track(ap, fr.ptr(1), B, p("init"), p("align"), p("track")), _two_launches(fr, track0),
             scratch=dict(align0=B * ar, track0=B * 32)))
    return cases


PLAN_CASE_NAMES = ("vis_batch_f2f", "vis_batch_filter_keypoints", "vis_batch_homography", "vis_batch_homography_pose", "vis_batch_homography_polish",
                   "vis_batch_pnp", "vis_batch_ftrack (d_mask)", "vis_batch_ftrack_triangulate", "vis_batch_klt", "vis_batch_align", "vis_batch_track")
