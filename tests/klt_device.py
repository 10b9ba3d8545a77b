"""Device helpers of the KLT GPU tests (tests/test_klt_gpu.py, tests/test_klt_limits_gpu.py): frames and their gradient set on the
device, one vis_klt_batch with 0xEE guard fills, the comparison with the restatement tests/klt_ref.py byte for byte, and the plan path
(vis_batch_run(DETECT | GRADIENT) + vis_batch_klt) in two launches of 8."""
import ctypes as C

import numpy as np

import klt_ref as kr
import stride_range_cases as src

FILL = 0xEE
REC = 32
PW, PH, PB = 320, 240, 8                                           # the plan path: frame size and frames per launch


def dev(torch, a):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def filled(torch, nbytes):
    t = torch.full((max(nbytes, 16),), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()                                       # (the fill ran on torch's stream: finished before the library's streams write)
    return t


def levels(flat, w, h):
    """one frame of a gradient set -> its five level arrays"""
    lw, lh = kr.half_dims(w, h)
    out, off = [], 0
    for l in range(5):
        out.append(flat[off:off + lw[l] * lh[l]].reshape(lh[l], lw[l]))
        off += lw[l] * lh[l]
    return out


class Set:
    """n frames on the device at a row stride, their gradient set made by vis_gradient_batch, and the same as host frames for the restatement"""
    def __init__(self, vislam, torch, c, frames, stride, scale):
        self.n, self.h, self.w = frames.shape
        self.stride, self.scale = stride, scale
        fe = vislam.gradient_frame_elems(self.w, self.h)
        self.d_frames = dev(torch, src.padded(frames, stride))
        self.d_gray = torch.zeros(self.n * fe, dtype=torch.uint8, device="cuda")
        self.d_gx = torch.zeros(self.n * fe, dtype=torch.int16, device="cuda")
        self.d_gy = torch.zeros(self.n * fe, dtype=torch.int16, device="cuda")
        d_g = torch.zeros(self.n * fe, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        c.gradient_batch(self.d_frames.data_ptr(), self.w, self.h, stride, self.n, self.d_gray.data_ptr(), self.d_gx.data_ptr(), self.d_gy.data_ptr(),
                         d_g.data_ptr(), scale)
        c.batch_sync()
        gray, gx, gy = self.d_gray.cpu().numpy(), self.d_gx.cpu().numpy(), self.d_gy.cpu().numpy()
        self.host = []
        for i in range(self.n):
            g = levels(gray[i * fe:(i + 1) * fe], self.w, self.h)
            g[0] = frames[i]                                       # level 0 of the intensities is the frame itself
            self.host.append((g, levels(gx[i * fe:(i + 1) * fe], self.w, self.h), levels(gy[i * fe:(i + 1) * fe], self.w, self.h)))


def want(S, kp, pts, npts, guess, max_pts):
    """the restatement of every pair of one vis_klt_batch"""
    out = []
    for i in range(1, S.n):
        m = min(max(int(npts[i]), 0), max_pts)
        out.append(kr.track(kp, S.host[i - 1], S.host[i], pts[i, :m], None if guess is None else guess[i, :m]))
    return out


def launch(vislam, torch, c, S, kp, pts, npts, guess, max_pts, compacted=True):
    """one vis_klt_batch -> (record rows n x max_pts, pair records, p1 rows, p2 rows, ntracked); the guard bytes behind every buffer checked"""
    n = S.n
    d_pts, d_npts = dev(torch, pts), dev(torch, npts)
    d_guess = None if guess is None else dev(torch, guess)
    out, pair = filled(torch, (n * max_pts + 2) * REC), filled(torch, (n + 2) * 32)
    p1, p2, nt = filled(torch, n * max_pts * 8 + 64), filled(torch, n * max_pts * 8 + 64), filled(torch, n * 4 + 64)
    vkp = vislam.KltParams(*[getattr(kp, f) for f in kr.P_FIELDS])
    c.klt_batch(S.d_frames.data_ptr(), S.w, S.h, S.stride, n, S.d_gray.data_ptr(), S.d_gx.data_ptr(), S.d_gy.data_ptr(), d_pts.data_ptr(),
                d_npts.data_ptr(), max_pts, out.data_ptr(), pair.data_ptr(), 0 if d_guess is None else d_guess.data_ptr(),
                p1.data_ptr() if compacted else 0, p2.data_ptr() if compacted else 0, nt.data_ptr() if compacted else 0, vkp)
    c.batch_sync()
    raw, praw, r1, r2, rn = (t.cpu().numpy() for t in (out, pair, p1, p2, nt))
    assert (raw[n * max_pts * REC:] == FILL).all() and (praw[n * 32:] == FILL).all()
    assert (r1[n * max_pts * 8:] == FILL).all() and (r2[n * max_pts * 8:] == FILL).all() and (rn[n * 4:] == FILL).all()
    if not compacted:
        assert (r1 == FILL).all() and (r2 == FILL).all() and (rn == FILL).all()
    return (raw[:n * max_pts * REC].view(vislam.KLT_POINT_DTYPE).reshape(n, max_pts), praw[:n * 32].view(vislam.KLT_PAIR_DTYPE),
            r1[:n * max_pts * 8].reshape(n, max_pts * 8), r2[:n * max_pts * 8].reshape(n, max_pts * 8), rn[:n * 4].view(np.int32))


def compare(got, want, pts, npts, max_pts, where, compacted=True):
    recs, pairs, r1, r2, rn = got
    n = len(recs)
    assert not recs[0].tobytes().strip(b"\0"), where               # row 0: zeroed records, the pair record of no pair
    assert pairs[0].tobytes() == kr.pair_record(None, no_pair=True).tobytes(), where
    flags = 0
    for i in range(1, n):
        m = min(max(int(npts[i]), 0), max_pts)
        w = want[i - 1]
        assert len(w) == m
        if recs[i, :m].tobytes() != w.tobytes():
            bad = [k for k in range(m) if recs[i, k].tobytes() != w[k].tobytes()]
            raise AssertionError((where, i, bad[:5], [(pts[i, k].tolist(), recs[i, k], w[k]) for k in bad[:3]]))
        assert (recs[i, m:].view(np.uint8) == FILL).all(), (where, i)     # records behind the pair's points are left alone
        assert pairs[i].tobytes() == kr.pair_record(w).tobytes(), (where, i, pairs[i])
        if compacted:
            a, b = kr.compact(pts[i, :m], w)
            k = len(a)
            assert int(rn[i]) == k == int(pairs[i]["n_tracked"]), (where, i)
            assert r1[i, :k * 8].tobytes() == a.tobytes() and r2[i, :k * 8].tobytes() == b.tobytes(), (where, i)
            assert (r1[i, k * 8:] == FILL).all() and (r2[i, k * 8:] == FILL).all(), (where, i)
        flags |= int(np.bitwise_or.reduce(w["flags"])) if m else 0
    if compacted:
        assert int(rn[0]) == 0 and (r1[0] == FILL).all() and (r2[0] == FILL).all(), where
    return flags


# ---------------------------------------------------------------------------------------------- the plan's pairs
def fetch(ptr, nbytes):
    hip = C.CDLL("libamdhip64.so")
    host = np.empty(nbytes, np.uint8)
    assert hip.hipMemcpy(C.c_void_p(host.ctypes.data), C.c_void_p(ptr), C.c_size_t(nbytes), 2) == 0     # device to host
    return host


def plan_launches(vislam, torch, frames, gate, kp, extra=0, runs=()):
    """two launches of 8 through vis_batch_run(DETECT | GRADIENT) + vis_batch_klt -> per launch what the call wrote, the pairing, the
    keypoints and the plan's pyramids and gradients as host frames.

    extra: the caller's rows are row_cap = the plan's keypoint capacity + extra long.
    runs: further vis_batch_klt calls on the same vis_batch_run, each (params, make_guess or None); make_guess(links, kps, row_cap) gives
    the guess rows (n x row_cap x 2 float32) from the pairing and the keypoints downloaded after the run.  Their outputs come as
    L["runs"][j], dicts like L itself with the guess that was given."""
    p = src.plan_params(vislam, PW, PH, gate)
    p.nfeatures = 200
    c = vislam.Context(0, p)
    c.batch_plan(PW, PH, PW, PB)
    cap = c.keypoint_capacity(PW, PH)
    rc = cap + extra
    d_frames = dev(torch, frames)
    fe = vislam.gradient_frame_elems(PW, PH)
    vkp = vislam.KltParams(*[getattr(kp, f) for f in kr.P_FIELDS])

    def buffers():
        return (filled(torch, (PB * rc + 1) * REC), filled(torch, (PB + 1) * 32), filled(torch, PB * rc * 8 + 16), filled(torch, PB * rc * 8 + 16),
                filled(torch, PB * 4 + 16))

    def download(bufs):
        raw, praw, r1, r2, rn = (t.cpu().numpy() for t in bufs)
        assert (raw[PB * rc * REC:] == FILL).all() and (praw[PB * 32:] == FILL).all() and (rn[PB * 4:] == FILL).all()
        assert (r1[PB * rc * 8:] == FILL).all() and (r2[PB * rc * 8:] == FILL).all()
        return dict(recs=raw[:PB * rc * REC].view(vislam.KLT_POINT_DTYPE).reshape(PB, rc), pairs=praw[:PB * 32].view(vislam.KLT_PAIR_DTYPE),
                    p1=r1[:PB * rc * 8].reshape(PB, rc * 8), p2=r2[:PB * rc * 8].reshape(PB, rc * 8), nt=rn[:PB * 4].view(np.int32))

    out = []
    for li in range(2):
        ptr = d_frames.data_ptr() + li * PB * PW * PH
        c.batch_run(ptr, PB, vislam.STAGE_DETECT | vislam.STAGE_GRADIENT)
        bufs = buffers()
        recs, pair, p1, p2, nt = bufs
        if li == 0:
            bad = vislam.default_klt_params()
            bad.scharr_scale = 1
            args = (C.c_void_p(ptr), PB, None, rc, C.c_void_p(recs.data_ptr()), C.c_void_p(pair.data_ptr()), None, None, None)
            assert vislam.lib.vis_batch_klt(c._h, C.byref(bad), *args) == -1                                   # the plan's gradients have scale 3
            assert vislam.lib.vis_batch_klt(c._h, C.byref(vkp), C.c_void_p(ptr), PB - 1, *args[2:]) == -5       # VIS_E_STATE: n differs
            assert vislam.lib.vis_batch_klt(c._h, C.byref(vkp), C.c_void_p(ptr), PB, None, cap - 1, *args[4:]) == -4   # VIS_E_CAPACITY
        c.batch_klt(ptr, PB, rc, recs.data_ptr(), pair.data_ptr(), 0, p1.data_ptr(), p2.data_ptr(), nt.data_ptr(), vkp)
        c.batch_sync()
        assert c.batch_status() == 0
        pg, px, py, _, pfe = c.batch_gradients()
        assert pfe == fe
        gray, gx, gy = fetch(pg, PB * fe), fetch(px, 2 * PB * fe).view(np.int16), fetch(py, 2 * PB * fe).view(np.int16)
        host = []
        for i in range(PB):
            g = levels(gray[i * fe:(i + 1) * fe], PW, PH)
            g[0] = frames[li * PB + i]
            host.append((g, levels(gx[i * fe:(i + 1) * fe], PW, PH), levels(gy[i * fe:(i + 1) * fe], PW, PH)))
        L = download(bufs)
        L.update(links=c.batch_get_keyframes(), kps=[c.batch_keypoints(i)[0] for i in range(PB)], host=host, cap=cap, row_cap=rc, guess=None, kp=kp, runs=[])
        for rkp, make_guess in runs:
            guess = None if make_guess is None else make_guess(L["links"], L["kps"], rc)
            d_guess = None if guess is None else dev(torch, guess)
            rbufs = buffers()
            c.batch_klt(ptr, PB, rc, rbufs[0].data_ptr(), rbufs[1].data_ptr(), 0 if d_guess is None else d_guess.data_ptr(), rbufs[2].data_ptr(),
                        rbufs[3].data_ptr(), rbufs[4].data_ptr(), vislam.KltParams(*[getattr(rkp, f) for f in kr.P_FIELDS]))
            c.batch_sync()
            assert c.batch_status() == 0
            R = download(rbufs)
            R.update(links=L["links"], kps=L["kps"], host=host, cap=cap, row_cap=rc, guess=guess, kp=rkp)
            L["runs"].append(R)
        out.append(L)
    # a run without the gradient stage, or without detection, leaves nothing to track on
    c.batch_run(d_frames.data_ptr(), PB, vislam.STAGE_DETECT | vislam.STAGE_MATCH)
    args = (C.byref(vkp), C.c_void_p(d_frames.data_ptr()), PB, None, rc, C.c_void_p(recs.data_ptr()), C.c_void_p(pair.data_ptr()), None, None, None)
    assert vislam.lib.vis_batch_klt(c._h, *args) == -5
    c.batch_sync()
    c.close()
    return out
