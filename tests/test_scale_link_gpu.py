"""GPU: vis_scale_link_rows against the restatement tests/scale_link_ref.py, BYTE FOR BYTE: the depth rows and the records.  Output buffers are
pre-filled with 0xEE (the FILL convention of tests/test_pnp_gpu.py) and everything behind the written extent must keep it.

Shared counts 0, 1, min_shared - 1, min_shared, 63, 64, 65, 255, 256, 257 and -- the list length at which the ratio pass moves its keys from LDS to
the workspace -- 1023, 1024, 1025 (odd and even counts among them), all ratios equal, ties at the three ranks, duplicate trainIdx (the first
wins), negative and out-of-range indices, require 0 and VIS_MP_KEPT, z of 0, negative, NaN and +-inf, pose records of zeros, a carried depth row
and none."""
import ctypes as C

import numpy as np
import pytest

import scale_link_ref as sl
from test_scale_link_ref import random_case, shared_case

pytestmark = pytest.mark.gpu
FILL = 0xEE


def _dev(torch, a):
    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a.reshape(-1).view(np.uint8) if a.size else np.zeros(16, np.uint8)).cuda()
    torch.cuda.synchronize()
    return t


def _filled(torch, nbytes):
    t = torch.full((nbytes,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()                                       # (the fill ran on torch's stream: finished before the library's streams write)
    return t


def c_params(vislam, sp):
    p = vislam.ScaleLinkParams()
    p.require, p.min_shared, p.max_rel_spread, p.min_scale, p.max_scale = sp.require, sp.min_shared, sp.max_rel_spread, sp.min_scale, sp.max_scale
    return p


def prepare_links(vislam, sp, prev, links, nlinks, pose, points, flags, row_cap, carry=None):
    """the inputs of one vis_scale_link_rows uploaded and its outputs filled (both synchronise the device); the answer is call(c), which queues the
    call on context c and synchronises nothing.  call(c) answers collect() -> (depth (n, row_cap), link (n)), for after a synchronise: it checks the
    guard bytes behind both outputs"""
    import torch
    n = len(prev)
    keep = [_dev(torch, a) for a in (np.asarray(prev, np.int32), links, np.asarray(nlinks, np.int32), pose, points, flags)]
    d_carry = _dev(torch, np.asarray(carry, np.float64)) if carry is not None else None
    depth, link = _filled(torch, (n * row_cap + 3) * 8), _filled(torch, (n + 2) * 40)

    def collect():
        rd, rl = depth.cpu().numpy(), link.cpu().numpy()
        assert (rd[n * row_cap * 8:] == FILL).all() and (rl[n * 40:] == FILL).all()
        return rd[:n * row_cap * 8].view(np.float64).reshape(n, row_cap), rl[:n * 40].view(vislam.SCALE_LINK_DTYPE)

    def call(c):
        c.scale_link_rows(n, keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), links.shape[1], keep[3].data_ptr(), keep[4].data_ptr(), keep[5].data_ptr(),
                          points.shape[1], row_cap, depth.data_ptr(), link.data_ptr(), d_carry.data_ptr() if carry is not None else 0, c_params(vislam, sp))
        return collect
    return call


def links_on_device(vislam, c, sp, *rows):
    """(depth (n, row_cap), link (n)) of one vis_scale_link_rows; the guard bytes behind both outputs checked"""
    collect = prepare_links(vislam, sp, *rows)(c)
    c.batch_sync()
    return collect()


def check(vislam, c, sp, case, row_cap, carry=None, where=None):
    got = links_on_device(vislam, c, sp, *case, row_cap, carry)
    want = sl.scale_link_rows(sp, *case, row_cap, carry)
    assert got[1].tobytes() == want[1].tobytes(), (where, got[1], want[1])
    assert got[0].tobytes() == want[0].tobytes(), (where, np.argwhere(got[0] != want[0])[:5])
    return want


@pytest.mark.parametrize("ns", [0, 1, 7, 8, 63, 64, 65, 255, 256, 257])
def test_shared_counts(vislam, ctx, ns):
    (*case, row_cap, _), _ = shared_case(ns)
    _, link = check(vislam, ctx, sl.Params(), case, row_cap, where=ns)
    assert int(link[2]["n_shared"]) == ns and bool(int(link[2]["flags"]) & sl.SL_FEW) == (ns < 8)
    (*case, row_cap, carry), _ = shared_case(ns, carried=True)     # the same frame through a carried depth row, and without one
    _, clink = check(vislam, ctx, sl.Params(), case, row_cap, carry, where=("carried", ns))
    assert int(clink[0]["n_shared"]) == ns and float(clink[0]["scale"]) == float(link[2]["scale"])
    _, clink = check(vislam, ctx, sl.Params(), case, row_cap, None, where=("no row", ns))
    assert int(clink[0]["flags"]) == sl.SL_NO_DEPTH


@pytest.mark.parametrize("m", [sl.SL_LDS_CAP - 1, sl.SL_LDS_CAP, sl.SL_LDS_CAP + 1])
def test_both_sides_of_the_lds_size(vislam, ctx, m):
    """the list length at which the keys leave LDS, every entry shared and (extra = 2) two of them not"""
    for extra in (0, 2):
        (*case, row_cap, _), _ = shared_case(m - extra, extra=extra)
        _, link = check(vislam, ctx, sl.Params(), case, row_cap, where=(m, extra))
        assert int(link[2]["n_shared"]) == m - extra and int(link[2]["flags"]) == sl.SL_OK


@pytest.mark.parametrize("ns", [9, 64, 258])
def test_equal_ratios_and_ties_at_the_ranks(vislam, ctx, ns):
    (*case, row_cap, _), _ = shared_case(ns, values=np.full(ns, 1.25))
    _, link = check(vislam, ctx, sl.Params(), case, row_cap, where=("equal", ns))
    assert float(link[2]["q25"]) == float(link[2]["scale"]) == float(link[2]["q75"]) and int(link[2]["flags"]) == sl.SL_OK
    v = np.repeat([0.5, 1.0, 3.0], [ns // 3, ns - 2 * (ns // 3), ns // 3])     # the ranks fall inside runs of equal values
    (*case, row_cap, _), _ = shared_case(ns, values=np.random.default_rng(ns).permutation(v))
    for sp in (sl.Params(), sl.Params(max_rel_spread=5.0, min_scale=1.5), sl.Params(min_shared=ns + 1, max_rel_spread=2.5)):
        check(vislam, ctx, sp, case, row_cap, where=("ties", ns))


@pytest.mark.parametrize("seed", range(5))
def test_hostile_rows_against_the_restatement(vislam, ctx, seed):
    n, row_cap, link_cap, pts_cap = [(9, 40, 37, 41), (17, 64, 70, 66), (5, 8, 30, 30), (33, 65, 64, 64), (6, 300, 1100, 1060)][seed]
    case = random_case(seed, n, row_cap, link_cap, pts_cap, first_prev=sl.KF_CARRIED if seed & 1 else sl.KF_FIRST)
    rng = np.random.default_rng(seed)
    carry = np.where(rng.random(row_cap) < 0.7, rng.uniform(2, 9, row_cap), 0.0)
    carry[:4] = [float("nan"), float("inf"), -2.0, 0.0][:min(4, row_cap)]
    for sp, c in ((sl.Params(), None), (sl.Params(require=0, min_shared=3, max_rel_spread=0.2, min_scale=0.8, max_scale=1.25), carry)):
        depth, link = check(vislam, ctx, sp, case, row_cap, c, where=(seed, c is not None))
        assert np.isfinite(depth).all() and all(np.isfinite(link[f]).all() for f in ("scale", "q25", "q75"))


def test_a_row_of_the_output_is_the_next_calls_carried_row(vislam, ctx):
    """a stream of 12 frames as one call and as two calls of 6, the second given row 5 of the first: the same records but q"""
    import torch
    case = random_case(77, 12, 50, 60, 60, hostile=False)
    prev = np.arange(-1, 11).astype(np.int32)
    prev[0] = sl.KF_FIRST
    case = (prev,) + case[1:]
    _, whole = check(vislam, ctx, sl.Params(min_shared=2), case, 50)
    d1, _ = check(vislam, ctx, sl.Params(min_shared=2), tuple(a[:6] for a in case), 50)
    prev2 = np.arange(-1, 5).astype(np.int32)
    _, second = check(vislam, ctx, sl.Params(min_shared=2), (prev2,) + tuple(a[6:] for a in case[1:]), 50, d1[5])
    a, b = whole[6:].copy(), second.copy()
    a["q"] = b["q"] = 0
    assert a.tobytes() == b.tobytes() and (whole[6:]["n_shared"] > 0).any()
