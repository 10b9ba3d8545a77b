"""CPU: feature tracks as a stream -- the restatement tests/ftrack_ref.py chained launch by launch (link_rows + carry_out) against the
whole-stream dictionary walk of tests/ftrack_stream_cases.py, byte for byte, observations and frame records.

Random streams with every hostile ingredient (duplicates on either side, out-of-range indices, counts beyond their capacities and below zero,
gated and restarting frames) at (n, row_cap, link_cap) = (40, 24, 24), (33, 65, 70) and (9, 8, 8), cut into one launch, launches of one frame,
an uneven cut and a cut one launch of which holds only VIS_KF_NOT_SAVED frames, with and without the mask.

The gated stream of ftrack_stream_cases.py (37 frames, 320 x 240, flat frames, keyframe gate 10) and its plain twin with the lists of the CPU
oracle, cuts A - D, symmetric and good lists, with and without the whole-stream mask; the vacuity guards the GPU module asserts on the
device's lists hold here on the oracle's."""
import numpy as np
import pytest

import ftrack_ref as fr
import ftrack_stream_cases as sc
from test_ftrack_ref import random_stream


@pytest.mark.parametrize("seed,n,row_cap,link_cap", sc.RANDOM_STREAMS)
def test_hostile_random_streams_in_every_cut(seed, n, row_cap, link_cap):
    prev, nkp, links, nlinks, mask = random_stream(seed, n, row_cap, link_cap, hostile=True)
    assert (prev == fr.KF_NOT_SAVED).any() and (nkp > row_cap).any() and (nkp < 0).any() and (nlinks > link_cap).any()
    cuts = sc.cuts_of(prev)
    a = cuts["nothing_saved"][0]
    assert (prev[a:a + cuts["nothing_saved"][1]] == fr.KF_NOT_SAVED).all() and (prev[:a] != fr.KF_NOT_SAVED).any()
    for m_ in (None, mask):
        w_obs, w_fr = sc.walk_link(prev, nkp, links, nlinks, row_cap, m_)
        assert n < 30 or int(w_obs["len"].max()) >= 3               # tracks long enough to cross launches
        for name, cut in cuts.items():
            obs, frames = sc.chain(prev, nkp, links, nlinks, row_cap, cut, m_)
            assert obs.tobytes() == w_obs.tobytes(), (name, m_ is not None, np.argwhere(obs != w_obs)[:5])
            assert frames.tobytes() == w_fr.tobytes(), (name, m_ is not None)
        # the launch that saved nothing carried a row that the launch behind it continues (else the cut shows nothing)
        after = a + cuts["nothing_saved"][1]
        nxt = next((i for i in range(after, n) if 0 <= int(prev[i]) < a), None)
        if m_ is None and n >= 30:
            assert nxt is not None and int(w_fr[nxt]["n_continued"]) > 0, (seed, nxt)


def test_localise_is_the_launch_numbering():
    prev = np.array([fr.KF_FIRST, 0, fr.KF_NOT_SAVED, 1, 3, fr.KF_FIRST, 5], np.int32)
    assert sc.localise(prev, 0, 7).tolist() == prev.tolist()
    assert sc.localise(prev, 3, 4).tolist() == [fr.KF_CARRIED, 0, fr.KF_FIRST, 2]
    assert sc.localise(prev, 2, 1).tolist() == [fr.KF_NOT_SAVED]
    assert sc.globalise(sc.localise(prev, 3, 4), 3, 1) == prev[3:].tolist()
    assert sc.last_saved_of(prev, 3) == 1 and sc.last_saved_of(prev, 0) is None
    assert sc.CUTS["A"] == [8, 1, 4, 8, 3, 8, 5] and all(sum(c) == sc.N for c in sc.CUTS.values()) and sc.FLAT == [3, 9, 10, 11, 12, 20, 21]


@pytest.fixture(scope="module")
def streams(vislam, orc, canvas):
    return {gate: sc.oracle_stream(vislam, orc, canvas, gate) for gate in (True, False)}


@pytest.mark.parametrize("gate", [True, False], ids=["gate_on", "gate_off"])
def test_gated_stream_on_the_oracle_lists(vislam, streams, gate):
    s = streams[gate]
    prev, nkp = s["prev"], s["nkp"]
    R = 256
    saved = prev != fr.KF_NOT_SAVED
    assert [i for i in range(sc.N) if not saved[i]] == (sc.FLAT if gate else [])
    print(f"\ngate {gate}: keypoints {nkp[saved].min()} ... {nkp[saved].max()}")
    assert nkp[saved].min() >= 150 and nkp.max() <= R
    mask_all = sc.stream_mask(R)
    for kind in ("sym", "good"):
        links, nl = sc.as_rows(s[kind], R)
        paired = [len(l) for i, l in enumerate(s[kind]) if prev[i] >= 0]
        whole = {}
        for masked in (False, True):
            m_ = mask_all if masked else None
            w_obs, w_fr = sc.walk_link(prev, nkp, links, nl, R, m_)
            whole[masked] = w_obs
            for name, cut in sc.CUTS.items():
                obs, frames = sc.chain(prev, nkp, links, nl, R, cut, m_)
                assert obs.tobytes() == w_obs.tobytes(), (kind, masked, name)
                assert frames.tobytes() == w_fr.tobytes(), (kind, masked, name)
                got = sc.guards(kind, obs, frames, prev, cut, unmasked=whole[False] if masked else None, gated=gate and name == "A")
                if name == "A":
                    print(f"gate {gate}, {kind}, masked {masked}: lists {min(paired)} ... {max(paired)}, longest track {int(w_obs['len'].max())}, "
                          f"tracks crossing into the launches of cut A {[g[2] for g in got]}")
            assert int(w_obs["len"].max()) >= (4 if masked else 6)
