"""Feature tracks as a STREAM: the cases of tests/test_ftrack_stream_ref.py and tests/test_ftrack_stream_gpu.py (numpy only, not a test module;
nothing here calls the code under test).

The truth for a whole stream is walk_link: frames in order, one dictionary of track identities per frame, a GLOBAL prev[] and no launches.
A stream cut into launches is the restatement tests/ftrack_ref.py driven launch by launch (chain: link_rows + carry_out, each launch seeing
its own prev[] -- localise) or the device driven the same way; whatever the cut, the concatenated rows must be the walker's.

The gated stream: 37 frames of vis_synth_frame_parallax at 320 x 240, t = stream index, nfeatures 200, fy = fx, keyframe_min_points 10, flat
frames (all 128: no keypoints, the gate does not save them) as drawn in PATTERN, which is also cut A -- a one-frame launch, a launch that
saves nothing while a row is held, a flat last frame and a flat first frame.  The second stream has the same frames, none flat, the gate off.

The vacuity guards (guards): conditions on the restatement's rows that make a wrong carry visible -- enough tracks cross every launch boundary,
the all-flat launch included.  Measured on the CPU oracle's lists: saved frames have 189 ... 196 keypoints, the symmetric lists 21 ... 68
entries, the good lists 7 ... 17; the first saved frame of the launches of cut A continues 45, 24, 21, 47, 43 tracks born before the launch
(symmetric; 12, 11, 7, 13, 17 good), the 24 / 11 across the all-flat launch; 12 tracks of stream frame 13 were born in launch 0; the longest
track has 8 observations (symmetric), 7 (good).  The floors below are those figures with margin, not tuned to any device result."""
import numpy as np

import ftrack_ref as fr


# ---------------------------------------------------------------------------------------------- the independent walker
def walk_link(prev, nkp, links, nlinks, row_cap, mask=None, carry=None, seq0=0):
    """the independent implementation: frames in order, one dictionary of track identities per frame, no pointer doubling"""
    n = len(prev)
    obs = np.zeros((n, row_cap), fr.OBS_DTYPE)
    obs[:] = fr.EMPTY_OBS
    frames = np.zeros(n, fr.FRAME_DTYPE)
    ident = []                                                      # per frame {keypoint: (birth_seq, birth_kp, len)}
    carried = None if carry is None else {k: (int(c["birth_seq"]), int(c["birth_kp"]), int(c["len"])) for k, c in enumerate(carry) if int(c["len"]) > 0}
    for i in range(n):
        p = int(prev[i])
        nk = 0 if p == fr.KF_NOT_SAVED else min(max(int(nkp[i]), 0), row_cap)
        parent = ident[p] if 0 <= p < i else carried if (p == fr.KF_CARRIED and carried is not None) else None
        m = min(max(int(nlinks[i]), 0), links.shape[1])
        if mask is not None:
            m = min(m, mask.shape[1])
        seen_t, seen_q, linked = set(), set(), {}
        if parent is not None:
            for c in range(m):
                q, t = int(links[i, c]["queryIdx"]), int(links[i, c]["trainIdx"])
                if not (0 <= t < nk) or q not in parent or (mask is not None and mask[i, c] == 0):
                    continue
                if t not in seen_t and q not in seen_q:
                    linked[t] = q
                seen_t.add(t)
                seen_q.add(q)
        cur = {}
        for k in range(nk):
            if k in linked:
                b = parent[linked[k]]
                cur[k] = (b[0], b[1], b[2] + 1)
            else:
                cur[k] = (seq0 + i, k, 1)
            obs[i, k] = cur[k] + (linked.get(k, -1),)
        ident.append(cur)
        lens = [v[2] for v in cur.values()]
        frames[i] = (seq0 + i, nk, len(linked), nk - len(linked), 0 if parent is None else len(parent) - len(linked), max(lens, default=0),
                     sum(lens), 0 if parent is not None else fr.FT_NO_CARRY if p == fr.KF_CARRIED else fr.FT_NO_PAIR)
    return obs, frames


# ---------------------------------------------------------------------------------------------- a stream in launches
def localise(prev_global, at, m):
    """the prev[] of the launch of m frames that starts at stream index `at`, in the launch's own numbering: an index before `at` becomes
    KF_CARRIED (the carried row is that of the last SAVED frame before the launch, which is what prev[] names: the gate links to nothing older)"""
    g = np.asarray(prev_global[at:at + m], np.int64)
    return np.where(g < 0, g, np.where(g - at < 0, fr.KF_CARRIED, g - at)).astype(np.int32)


def globalise(prev_local, at, last_saved):
    """the inverse, for a launch the device paired: KF_CARRIED names the last saved frame before the launch (KF_FIRST when there is none)"""
    out = []
    for q in prev_local:
        q = int(q)
        out.append(at + q if q >= 0 else (last_saved if last_saved is not None else fr.KF_FIRST) if q == fr.KF_CARRIED else q)
    return out


def last_saved_of(prev_global, upto, before=None):
    """the stream index of the last saved frame below `upto`, else `before`"""
    for i in range(upto - 1, -1, -1):
        if int(prev_global[i]) != fr.KF_NOT_SAVED:
            return i
    return before


def chain(prev_global, nkp, links, nlinks, row_cap, cuts, mask=None):
    """the restatement launch by launch: link_rows on the launch's own prev[] with the row carry_out kept; the concatenated (obs, frames)"""
    carry, at, rows, recs = None, 0, [], []
    for m in cuts:
        local = localise(prev_global, at, m)
        o, f = fr.link_rows(local, nkp[at:at + m], links[at:at + m], nlinks[at:at + m], row_cap, None if mask is None else mask[at:at + m], carry, seq0=at)
        carry = fr.carry_out(local, o, carry, row_cap)
        rows.append(o)
        recs.append(f)
        at += m
    assert at == len(prev_global)
    return np.concatenate(rows), np.concatenate(recs)


# (seed, n, row_cap, link_cap) of the random streams; every one has a KF_NOT_SAVED frame behind a saved one (asserted where they are used)
RANDOM_STREAMS = [(24, 40, 24, 24), (45, 33, 65, 70), (33, 9, 8, 8)]


def cuts_of(prev_global):
    """{name: launch sizes}: one launch, one frame per launch, an uneven cut, and a cut one launch of which holds only KF_NOT_SAVED frames (the
    first run of such frames behind a saved one, so that a row is held while nothing is saved)"""
    n = len(prev_global)
    uneven, left = [], n
    for m in (3, 1, 7, 2, 16, 5, 1, 11):                           # no multiple of anything, a launch of 1 in the middle, one past 2^k
        if left:
            uneven.append(min(m, left))
            left -= uneven[-1]
    if left:
        uneven.append(left)
    saved = np.asarray(prev_global) != fr.KF_NOT_SAVED
    a = next(i for i in range(1, n) if not saved[i] and saved[:i].any())
    b = a
    while b < n and not saved[b]:
        b += 1
    return {"whole": [n], "ones": [1] * n, "uneven": uneven, "nothing_saved": [m for m in (a, b - a, n - b) if m]}


# ---------------------------------------------------------------------------------------------- the gated stream
W, H, N = 320, 240, 37
NFEATURES, MIN_POINTS = 200, 10
PATTERN = "N N N F N N N N | N | F F F F | N N N N N N N F | F N N | N N N N N N N N | N N N N N"
FLAT = [i for i, ch in enumerate(PATTERN.replace("|", "").split()) if ch == "F"]
CUTS = {"A": [len(part.split()) for part in PATTERN.split("|")], "B": [N], "C": [8, 8, 8, 8, 5], "D": [1] * N}
PLAN_B = {"A": 8, "B": N, "C": 8, "D": 8}
MASK_SEED, MASK_WIDTH = 77, 4096


def stream_frames(vislam, canvas, n=N, flat=()):
    f = np.stack([vislam.synth_frame(canvas, t, W, H, parallax=True) for t in range(n)])
    for i in flat:
        f[i] = 128                                                  # flat: no keypoints, the gate does not save it
    return f


def stream_params(vislam, gate):
    p = vislam.default_params()
    p.nfeatures = NFEATURES
    p.w_size, p.h_size = W, H                                      # (the matcher's grid covers the frame, as in the other 320 x 240 plan tests)
    p.fy = p.fx
    p.keyframe_min_points = MIN_POINTS if gate else 0
    return p


def gate_walk(n_kp, gate):
    """the keyframe gate's global prev[]: gate off, frame i pairs with frame i - 1; gate on, a frame is saved with more than MIN_POINTS keypoints
    (more than 1 until the first is saved) and pairs with the last saved frame before it"""
    prev, last = [], None
    for i, k in enumerate(n_kp):
        if gate and not (k > (MIN_POINTS if last is not None else 1)):
            prev.append(fr.KF_NOT_SAVED)
            continue
        prev.append(fr.KF_FIRST if last is None else last)
        last = i
    return np.array(prev, np.int32)


def stream_mask(cap):
    """the whole-stream mask, keyed by (stream index, list position), about 80 % ones; the first cap columns (the same bits whatever the cap)"""
    return np.ascontiguousarray((np.random.default_rng(MASK_SEED).random((N, MASK_WIDTH)) < 0.8).astype(np.uint8)[:, :cap])


def as_rows(lists, cap):
    rows, cnt = np.zeros((len(lists), cap), fr.DMATCH_DTYPE), np.zeros(len(lists), np.int32)
    for i, l in enumerate(lists):
        rows[i, :len(l)], cnt[i] = l, len(l)
    return rows, cnt


def oracle_stream(vislam, orc, canvas, gate):
    """the gated (or the plain) stream on the CPU oracle: dict(prev, nkp, sym, good) with the lists of frame i against frame prev[i]"""
    p = stream_params(vislam, gate)
    frames = stream_frames(vislam, canvas, flat=FLAT if gate else ())
    det = [orc.orb_detect_compute(p, f) for f in frames]
    nkp = np.array([len(k) for k, _ in det], np.int32)
    prev = gate_walk(nkp, gate)
    sym, good = [], []
    for i in range(N):
        q = int(prev[i])
        if q < 0:
            sym.append(np.zeros(0, fr.DMATCH_DTYPE))
            good.append(np.zeros(0, fr.DMATCH_DTYPE))
            continue
        g, s = orc.good_matches(p, det[q][0], det[i][0], *orc.knn2_hamming(det[q][1], det[i][1]))
        sym.append(s.astype(fr.DMATCH_DTYPE))
        good.append(g.astype(fr.DMATCH_DTYPE))
    return dict(prev=prev, nkp=nkp, sym=sym, good=good)


# ---------------------------------------------------------------------------------------------- vacuity guards
FLOOR = {"sym": 15, "good": 5}
# tracks born in launch 0 of cut A and alive in launch 3, keyed by (list, masked).  On the oracle's lists: 12 symmetric, 3 good, 5 symmetric under
# the caller's mask, none of the good ones under a mask -- floors with margin, and no condition where the oracle has none to show
BORN0_FLOOR = {("sym", False): 5, ("good", False): 1, ("sym", True): 1}


def crossing(obs, prev_global, cuts):
    """per launch of the cut that has a saved frame, with a saved frame somewhere before it: (launch, stream index of its first saved frame,
    the tracks of that frame born before the launch)"""
    out, at = [], 0
    for launch, m in enumerate(cuts):
        first = next((i for i in range(at, at + m) if int(prev_global[i]) != fr.KF_NOT_SAVED), None)
        if first is not None and last_saved_of(prev_global, at) is not None:
            row = obs[first]
            out.append((launch, first, int(((row["len"] > 0) & (row["birth_seq"] < at)).sum())))
        at += m
    return out


def guards(kind, obs, frames, prev_global, cuts, unmasked=None, gated=False):
    """the conditions of a cut's rows of the list `kind` ("sym" / "good").  Without `unmasked`: the list's floor at every boundary.  With the
    rows `unmasked` of the same list: these are a masked variant's -- at least one track crosses every boundary, none more than there and fewer
    in all.  gated: the cut is cut A of the gated stream -- the all-flat
    launch and the tracks of launch 0 that live in launch 3.  Returns the crossing counts."""
    assert not (frames["flags"] & fr.FT_NO_CARRY).any(), (kind, cuts, np.nonzero(frames["flags"] & fr.FT_NO_CARRY)[0])
    got = crossing(obs, prev_global, cuts)
    assert len(got) >= (1 if len(cuts) > 1 else 0)
    masked = unmasked is not None
    if masked:
        ref = crossing(unmasked, prev_global, cuts)
        assert [g[:2] for g in got] == [r[:2] for r in ref]
        assert all(1 <= g[2] <= r[2] for g, r in zip(got, ref)), (cuts, got, ref)
        assert not got or sum(g[2] for g in got) < sum(r[2] for r in ref), (cuts, got, ref)
    else:
        assert all(g[2] >= FLOOR[kind] for g in got), (kind, cuts, got)
    if gated:
        assert cuts == CUTS["A"]
        bounds = np.cumsum([0] + cuts)
        assert all(int(q) == fr.KF_NOT_SAVED for q in prev_global[bounds[2]:bounds[3]])      # launch 2 saves nothing ...
        assert [g[0] for g in got] == [1, 3, 4, 5, 6]                                       # ... and launch 3's tracks cross it
        rows = obs[bounds[3]:bounds[4]]
        born0 = {(int(o["birth_seq"]), int(o["birth_kp"])) for o in rows.reshape(-1) if int(o["len"]) > 0 and int(o["birth_seq"]) < bounds[1]}
        if (kind, masked) in BORN0_FLOOR:                                                   # born in launch 0, alive in launch 3
            assert len(born0) >= BORN0_FLOOR[(kind, masked)], (kind, masked, len(born0))
    return got
