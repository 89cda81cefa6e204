"""GPU tests of the float forms of the two batched guided calls (include/popsift_hip.h): psx_match_pairs_guided_many (+ _dev)
and psx_match_pairs_guided_graph (+ _dev), and of the whole chain on float descriptors with records that never leave HBM.
The yardstick is the loop of psx_match_pairs_guided_dev -- the single call, on the same device arrays in the same process --,
compared as bytes; the edge lists, scenes and guides are those of tests/graph_chain_cases.py (window, homography, epipolar
band, PSX_GUIDE_NONE on some edges), the descriptors as float32 in the two flavours of tests/match_many_f32_cases.py."""
import ctypes as C

import numpy as np
import pytest
import torch        # before the HIP library is loaded: torch brings a HIP runtime of its own and must initialise first (_dev forms)

from tests import graph_chain_cases as gc
from tests import match_graph_cases as gcs
from tests.match_many_f32_cases import FLAVOURS, flavour
from tests.match_pairs_cases import same_records

pytestmark = pytest.mark.gpu

INF = float("inf")
GUIDED_CASES = {"mixed": (41, gcs.MIXED_LENS, gcs.MIXED_EDGES), "lefts": (42, gcs.LEFTS_LENS, gcs.LEFTS_EDGES)}


class _Views:
    """float32 descriptors and positions of every view as device tensors"""

    def __init__(self, sets, xys, which):
        self.lens = [len(s) for s in sets]
        self.desc = [torch.from_numpy(np.array(flavour(s, which) if len(s) else np.zeros((0, 128), np.float32))).cuda() for s in sets]
        self.xy = [torch.from_numpy(np.array(x, np.float32)).cuda() for x in xys]
        torch.cuda.synchronize()
        self.pdesc = [t.data_ptr() if n else None for t, n in zip(self.desc, self.lens)]
        self.pxy = [t.data_ptr() if n else None for t, n in zip(self.xy, self.lens)]


def _single(capi, dev, a, b, guide, ratio, mutual):
    """psx_match_pairs_guided_dev for one pair of views, read back"""
    cap = dev.lens[a]
    if cap == 0 or dev.lens[b] == 0:
        return np.zeros(0, capi.PAIR_DTYPE)
    dbuf = torch.zeros((cap * 16,), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    n = capi.match_pairs_guided_dev(dev.pdesc[a], dev.pxy[a], dev.lens[a], dev.pdesc[b], dev.pxy[b], dev.lens[b], guide, dbuf.data_ptr(), cap,
                                    ratio, mutual, u8=False)
    return dbuf.cpu().numpy()[:n * 16].view(capi.PAIR_DTYPE).copy()


def _graph_dev(capi, dev, edges, guides, ratio, mutual, cap):
    """psx_match_pairs_guided_graph_dev into a device buffer with a guard band: (per-edge counts, total, the whole buffer)"""
    dbuf = torch.full(((cap + 2) * 16,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    counts, n = capi.match_pairs_guided_graph_dev(dev.pdesc, dev.pxy, dev.lens, edges, guides, dbuf.data_ptr() if cap else 0, cap, ratio, mutual,
                                                  u8=False)
    return counts, n, dbuf.cpu().numpy()


@pytest.mark.parametrize("which", FLAVOURS)
@pytest.mark.parametrize("case", sorted(GUIDED_CASES))
def test_guided_graph_float_equals_the_single_calls(capi, case, which):
    """guides per edge that mix homography, epipolar band and NONE, over views of unequal length (0, 1, 33, 255, 256, 257,
    300, 513, 600 rows among them; empty sides, a self edge, a duplicate, both orders); both flag values, ratios 0.8 and
    inf; a capacity inside an edge and 0 with NULL; counts are always the totals; the guard band stays"""
    seed, lens, edges = GUIDED_CASES[case]
    sets, xys, _ = gc.scene(seed, lens)
    guides = [gc.edge_guide(e, a, b) for e, (a, b) in enumerate(edges)]
    cg = [gc.capi_guide(capi, g) for g in guides]
    assert {g[0] for g in guides} == {gc.NONE, 1, 2}
    room = sum(lens[a] for a, _ in edges)
    dev = _Views(sets, xys, which)
    for mutual in (False, True):
        for ratio in (0.8, INF):
            want = [np.zeros(0, capi.PAIR_DTYPE) if guides[e][0] == gc.NONE else _single(capi, dev, a, b, cg[e], ratio, mutual)
                    for e, (a, b) in enumerate(edges)]
            cat = gc.concat(want, capi.PAIR_DTYPE)
            total = len(cat)
            counts, n, back = _graph_dev(capi, dev, edges, cg, ratio, mutual, room)
            assert n == total and list(counts) == [len(w) for w in want], (case, which, ratio, mutual, list(counts))
            assert back[:total * 16].tobytes() == cat.tobytes() and np.all(back[total * 16:] == 0xA5)
            if ratio == 0.8:
                assert sum(len(w) > 2 for w in want) >= 3 and total > 40, "the planted scene gives pairs under the guides"
                first = next(e for e, w in enumerate(want) if len(w) > 2)
                inside = sum(len(w) for w in want[:first]) + 2                              # a cut inside an edge
                for cap in (inside, 0):
                    c2, n2, b2 = _graph_dev(capi, dev, edges, cg, ratio, mutual, cap)
                    assert n2 == total and np.array_equal(c2, counts), cap
                    assert b2[:cap * 16].tobytes() == cat[:cap].tobytes() and np.all(b2[cap * 16:] == 0xA5), cap
        # the python wrapper on host arrays: the host form of the same call
        fsets = [flavour(s, which) if len(s) else np.zeros((0, 128), np.float32) for s in sets]
        lists, c3 = capi.match_pairs_guided_graph(fsets, xys, edges, cg, 0.8, mutual)
        want = [np.zeros(0, capi.PAIR_DTYPE) if guides[e][0] == gc.NONE else _single(capi, dev, a, b, cg[e], 0.8, mutual) for e, (a, b) in enumerate(edges)]
        assert all(same_records(l, w) for l, w in zip(lists, want)) and list(c3) == [len(w) for w in want]


@pytest.mark.parametrize("which", FLAVOURS)
def test_guided_many_float_equals_the_single_calls(capi, which):
    """the star: view 0 of the LEFTS scene (600 rows) against the five others, set k under its own guide -- homography,
    epipolar band, NONE, a plain window (identity H) that admits few, and a homography so tight that some left rows keep ONE
    admissible partner (a second neighbour of +inf); an empty right set; counts and capacity; the host wrapper"""
    seed, lens = 42, gcs.LEFTS_LENS + (0,)
    sets, xys, _ = gc.scene(seed, lens)
    K = len(lens) - 1
    guides = [gc.edge_guide(k, 0, k + 1) for k in range(K)]
    guides[3] = (1, np.eye(3, dtype=np.float32).reshape(9), 30.0)                         # a search window
    guides[4] = (1, gc.true_h(0, 5), 0.25)                                                # nearly one partner per row
    cg = [gc.capi_guide(capi, g) for g in guides]
    dev = _Views(sets, xys, which)
    nl = lens[0]
    room = nl * K
    for mutual in (False, True):
        for ratio in (0.8, INF):
            want = [np.zeros(0, capi.PAIR_DTYPE) if guides[k][0] == gc.NONE else _single(capi, dev, 0, k + 1, cg[k], ratio, mutual) for k in range(K)]
            cat = gc.concat(want, capi.PAIR_DTYPE)
            total = len(cat)
            for cap in (room, len(want[0]) + 1, 0):
                dbuf = torch.full(((cap + 2) * 16,), 0xA5, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                counts, n = capi.match_pairs_guided_many_dev(dev.pdesc[0], dev.pxy[0], nl, dev.pdesc[1:], dev.pxy[1:], dev.lens[1:], cg,
                                                             dbuf.data_ptr() if cap else 0, cap, ratio, mutual, u8=False)
                back = dbuf.cpu().numpy()
                k = min(cap, total)
                assert n == total and list(counts) == [len(w) for w in want], (which, ratio, mutual, cap, list(counts))
                assert back[:k * 16].tobytes() == cat[:k].tobytes() and np.all(back[k * 16:] == 0xA5), cap
            assert len(want[5]) == 0 and len(want[2]) == 0                                  # the empty set, the skipped set
            if ratio == INF and not mutual:
                assert total > 40 and len(want[4]) > 5 and np.isinf(want[4]["d2"]).any() and not np.isinf(want[4]["d1"]).any()   # one admissible partner
        fsets = [flavour(s, which) if len(s) else np.zeros((0, 128), np.float32) for s in sets]
        lists, c2 = capi.match_pairs_guided_many(fsets[0], xys[0], fsets[1:], xys[1:], cg, 0.8, mutual)
        want = [np.zeros(0, capi.PAIR_DTYPE) if guides[k][0] == gc.NONE else _single(capi, dev, 0, k + 1, cg[k], 0.8, mutual) for k in range(K)]
        assert all(same_records(l, w) for l, w in zip(lists, want)) and list(c2) == [len(w) for w in want]


# ---- the chain ------------------------------------------------------------------------------------------------------------
CHAIN_LENS = (300, 257, 64, 129, 513, 200)
CHAIN_EDGES = [(a, b) for a in range(6) for b in range(6) if a != b]


def test_chain_on_floats_equals_the_chain_of_single_calls(capi):
    """psx_match_pairs_graph_dev -> psx_ransac_homography_graph_dev -> psx_guides_from_ransac ->
    psx_match_pairs_guided_graph_dev -> psx_tracks_graph_dev on six views of one scene (float descriptors, norm 512), all 30
    ordered pairs, nothing downloaded in between (only the per-edge counts and the ransac results, which the calls return on
    the host).  Every stage equals the same chain made of single calls per edge -- psx_match_pairs_dev,
    psx_ransac_homography_dev, psx_match_pairs_guided_dev -- and the tracks equal the host reference on those lists."""
    sets, xys, _ = gc.scene(43, CHAIN_LENS)
    edges, lens = CHAIN_EDGES, list(CHAIN_LENS)
    room = sum(lens[a] for a, _ in edges)
    opts = capi.ransac_opts(gc.TOL, 256, 9, True)
    dev = _Views(sets, xys, "norm512")
    PD = capi.PAIR_DTYPE
    d_pairs, d_inl, d_re = (torch.full((room * 16,), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(3))
    M = sum(lens)
    d_labels = torch.full((M,), -7, dtype=torch.int32, device="cuda")
    d_starts = torch.full((M + 1,), -7, dtype=torch.int32, device="cuda")
    d_members = torch.full((2 * M,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    # ---- the chain: five calls, the records stay where they are ----
    ec, n1 = capi.match_pairs_graph_dev(dev.pdesc, lens, edges, d_pairs.data_ptr(), room, 0.8, True, u8=False)
    path = capi.match_graph_f32_last()["path"]
    g = capi.ransac_homography_graph_dev(d_pairs.data_ptr(), ec, edges, dev.pxy, lens, d_inl.data_ptr(), room, opts)
    guides = capi.guides_from_ransac(g["results"], capi.GUIDE_HOMOGRAPHY, gc.TOL)
    rc, n3 = capi.match_pairs_guided_graph_dev(dev.pdesc, dev.pxy, lens, edges, guides, d_re.data_ptr(), room, 0.8, True, u8=False)
    tr = capi.tracks_graph_dev(d_re.data_ptr(), rc, edges, lens, d_labels.data_ptr(), d_starts.data_ptr(), M, d_members.data_ptr(), M)
    assert path == capi.match_graph_f32_plan(lens, edges, True)["path"] == 1                   # 244 left rows per edge on average: the scan
    # ---- the same chain of single calls ----
    pairs = d_pairs.cpu().numpy()[:n1 * 16].view(PD)
    inl = d_inl.cpu().numpy()[:g["count"] * 16].view(PD)
    re = d_re.cpu().numpy()[:n3 * 16].view(PD)
    p_lists, i_lists, r_lists = capi.split_sets(pairs, ec), capi.split_sets(inl, [r.inliers for r in g["results"]]), capi.split_sets(re, rc)
    assert n1 == int(np.sum(ec)) and n3 == int(np.sum(rc)) and g["count"] == sum(r.inliers for r in g["results"])
    one = torch.zeros((max(lens) * 16,), dtype=torch.uint8, device="cuda")
    one_inl = torch.zeros((max(lens) * 16,), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    verified, singles = 0, []
    for e, (a, b) in enumerate(edges):
        m = capi.match_pairs_dev(dev.pdesc[a], lens[a], dev.pdesc[b], lens[b], one.data_ptr(), lens[a], 0.8, True, u8=False)
        assert one.cpu().numpy()[:m * 16].tobytes() == p_lists[e].tobytes(), e
        s = capi.ransac_homography_dev(one.data_ptr(), m, dev.pxy[a], lens[a], dev.pxy[b], lens[b], one_inl.data_ptr(), lens[a], opts)
        res = g["results"][e]
        assert bytes(res)[:52] == bytes(s["result"])[:52] and s["count"] == res.inliers, e
        assert one_inl.cpu().numpy()[:s["count"] * 16].tobytes() == i_lists[e].tobytes(), e
        if res.best < 0:
            assert guides[e].kind == capi.GUIDE_NONE and rc[e] == 0, e
            singles.append(np.zeros(0, PD))
            continue
        verified += 1
        guide = capi.guides_from_ransac([s["result"]], capi.GUIDE_HOMOGRAPHY, gc.TOL)[0]
        k = capi.match_pairs_guided_dev(dev.pdesc[a], dev.pxy[a], lens[a], dev.pdesc[b], dev.pxy[b], lens[b], guide, one.data_ptr(), lens[a], 0.8, True,
                                        u8=False)
        singles.append(one.cpu().numpy()[:k * 16].view(PD).copy())
        assert same_records(r_lists[e], singles[-1]), e
    assert verified >= 25 and n3 > 100
    ref = capi.tracks_graph_ref(singles, edges, lens)
    assert all(tr[k] == ref[k] for k in tr), (tr, {k: ref[k] for k in tr})
    assert tr["tracks"] > 20
    assert np.array_equal(d_labels.cpu().numpy(), ref["labels"])
    assert np.array_equal(d_starts.cpu().numpy()[:tr["tracks"] + 1], ref["starts"])
    assert d_members.cpu().numpy()[:2 * tr["members"]].tobytes() == ref["member_records"].tobytes()
    assert capi.lib().psx_match_release() == 0
