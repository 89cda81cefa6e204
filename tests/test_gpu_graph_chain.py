"""GPU tests of the two edge-list calls behind psx_match_pairs_graph_u8 (include/popsift_hip.h, "A LIST OF VIEW PAIRS IN ONE
CALL"): psx_ransac_*_graph* for all four models, psx_match_pairs_guided_graph_u8*, the three-call chain on records that never
leave HBM, and FeaturesDev::estimate*Graph / matchPairsGuidedGraph.  Every comparison is as bytes, against the SINGLE device
call on the same device arrays in the same process and against something that is not device code: the host references
psx_ransac_*_graph_ref, and for the guided call the restatement of tests/graph_chain_cases.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch        # before the HIP library is loaded: torch brings a HIP runtime of its own and must initialise first (_dev forms)

from tests import graph_chain_cases as gc
from tests import match_graph_cases as gcs
from tests import ransac_many_cases as mc
from tests.match_pairs_cases import RATIOS
from tests.ransac_cases import PAIR_DTYPE, bits, same_records

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = [(1, mc.CONFIGS[0][1]), (65, mc.CONFIGS[1][1]), (1024, mc.CONFIGS[0][1])]        # N x the seeds of ransac_many_cases
CONFIG_IDS = ["N%d_s%d" % c for c in CONFIGS]
U8 = gcs.PAIR_U8


class _Views:
    """the views' arrays uploaded once: positions, and descriptors where the case has them"""

    def __init__(self, capi, xys, sets=None):
        self.L, self.bufs = capi.lib(), []
        xs = [np.ascontiguousarray(x, np.float32) for x in xys]
        self.lens = [len(x) for x in xs]
        self.pxy = [p.value for p in capi._to_device(self.L, 0, xs, self.bufs)]
        self.pdesc = [p.value for p in capi._to_device(self.L, 0, [np.ascontiguousarray(s, np.uint8) for s in sets], self.bufs)] if sets else None

    def close(self):
        for p in self.bufs:
            self.L.psx_dev_free(0, p)
        self.bufs = []


def _ransac_raw(capi, dev, model, lists, edges, opts, cap, layers=True):
    """psx_ransac_<model>_graph with sentinel-filled outputs: (rc, results, count, out int32 words, models, counts)"""
    E, N = len(edges), opts.hypotheses
    pairs = gc.concat(lists, lists[0].dtype if len(lists) else PAIR_DTYPE)
    ec, ea, la = np.array([len(p) for p in lists], np.int32), np.array(edges, np.int32).reshape(-1, 2), np.array(dev.lens, np.int32)
    pa = (C.c_void_p * max(len(dev.pxy), 1))(*dev.pxy)
    out = np.full((cap + 2) * 4, -7, np.int32)
    models, counts = np.full((E, N, 9), -7, np.float32), np.full((E, N), -7, np.int32)
    res, cnt = (capi.RansacResult * max(E, 1))(), C.c_int(-77)
    C.memset(res, 0x5a, C.sizeof(res))
    ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None
    rv = getattr(dev.L, "psx_ransac_%s_graph" % model)(0, ptr(pairs), ptr(ec), ptr(ea), E, pa, ptr(la), len(la), C.byref(opts), res,
                                                      ptr(out) if cap else None, cap, C.byref(cnt), ptr(models) if layers else None,
                                                      ptr(counts) if layers else None)
    return rv, res, cnt.value, out, models, counts


def _ransac_single(capi, dev, model, a, b, pairs, opts):
    """the single-list device call psx_ransac_<model> for one edge on the same device arrays: the dict of capi._ransac_call"""
    name, kind = capi._ransac_names(model)
    fn = lambda *args: getattr(dev.L, name)(0, *args)
    vp = lambda p: C.c_void_p(p) if p else None
    return capi._ransac_call(fn, name, pairs.ctypes.data_as(C.c_void_p) if pairs.size else None, len(pairs), pairs.dtype, vp(dev.pxy[a]), dev.lens[a],
                             vp(dev.pxy[b]), dev.lens[b], opts, None, True, kind=kind)


@pytest.mark.parametrize("refit", [False, True], ids=["sample", "refit"])
@pytest.mark.parametrize("N,seed", CONFIGS, ids=CONFIG_IDS)
@pytest.mark.parametrize("model", gc.MODELS)
def test_ransac_graph_equals_the_single_calls_and_the_reference(capi, model, N, seed, refit):
    """views of unequal length under the unsorted edge list; lists of 0, min - 1, min, 255, 256, 257, 512 and 513 pairs"""
    c = gc.ransac_case(model)
    opts = capi.ransac_opts(gc.TOL, N, seed, refit)
    ref = getattr(capi, "ransac_%s_graph_ref" % model)(c["lists"], c["edges"], c["xys"], opts, layers=True)
    E, total_pairs = len(c["edges"]), sum(c["counts"])
    dev = _Views(capi, c["xys"])
    try:
        rv, res, cnt, out, models, counts = _ransac_raw(capi, dev, model, c["lists"], c["edges"], opts, total_pairs)
        assert rv == 0
        total = ref["count"]
        assert cnt == total == sum(res[e].inliers for e in range(E))
        got = out[:4 * total].view(PAIR_DTYPE)
        assert same_records(got, ref["records"]) and np.all(out[4 * total:] == -7)            # the concatenation, as bytes
        assert np.array_equal(bits(models), bits(ref["models"])) and np.array_equal(counts, ref["counts"])
        at = 0
        for e, (a, b) in enumerate(c["edges"]):
            n, r = c["counts"][e], res[e]
            assert bytes(r) == bytes(ref["results"][e]), (e, n, r.best, ref["results"][e].best)
            mine = got[at:at + r.inliers]                                                    # starts at the sum of the inliers before it
            at += r.inliers
            one = _ransac_single(capi, dev, model, a, b, c["lists"][e], opts)
            assert bytes(r) == bytes(one["result"]) and same_records(mine, one["inliers"]), (e, n)
            if n >= gc.MIN[model]:
                assert np.array_equal(bits(models[e]), bits(one["models"])) and np.array_equal(counts[e], one["counts"]), (e, n)
            else:
                assert r.best == -1 and r.inliers == 0 and not models[e].any() and not counts[e].any(), (e, n)
        d0, d1 = gc.DUPLICATE
        assert bytes(res[d0]) == bytes(res[d1])                                              # a duplicate edge: the same result twice
        if N >= 65:
            assert sum(res[e].best >= 0 for e in range(E)) >= 6
        # the python wrapper
        g = getattr(capi, "ransac_%s_graph" % model)(c["lists"], c["edges"], c["xys"], opts)
        assert g["count"] == total and same_records(g["records"], ref["records"])
        assert all(bytes(g["results"][e])[:52] == bytes(ref["results"][e])[:52] for e in range(E))
    finally:
        dev.close()


@pytest.mark.parametrize("model", gc.MODELS)
def test_ransac_graph_dev_capacity_byte_records_and_a_bad_index(capi, model):
    """the _dev form on torch buffers: a capacity inside an edge, capacity 0 and the full one report the total and leave the
    bytes behind the capacity alone; records of the byte matcher's dtype carry their payload; ONE left index of the last edge
    that is in range for a longer view but not for its own refuses the call and writes nothing; a good call follows"""
    N, seed = CONFIGS[1]
    c, cu = gc.ransac_case(model), gc.ransac_case(model, u8=True)
    E, total_pairs = len(c["edges"]), sum(c["counts"])
    dev = _Views(capi, c["xys"])
    fn = getattr(capi, "ransac_%s_graph_dev" % model)
    try:
        for refit in (False, True):
            opts = capi.ransac_opts(gc.TOL, N, seed, refit)
            ref = getattr(capi, "ransac_%s_graph_ref" % model)(c["lists"], c["edges"], c["xys"], opts, layers=True)
            cat, total = ref["records"], ref["count"]
            inside = ref["results"][0].inliers + 1
            assert ref["results"][1].inliers > 1 and inside < total
            for lists, dtype in ((c["lists"], PAIR_DTYPE), (cu["lists"], U8)):
                host = np.ascontiguousarray(gc.concat(lists, dtype)).view(np.uint8).copy()
                src = torch.from_numpy(host).cuda()
                for cap in (inside, 0, total_pairs):
                    dbuf = torch.full(((cap + 2) * 16,), 0xA5, dtype=torch.uint8, device="cuda")
                    torch.cuda.synchronize()
                    g = fn(src.data_ptr(), c["counts"], c["edges"], dev.pxy, dev.lens, dbuf.data_ptr() if cap else 0, cap, opts, layers=True)
                    back = dbuf.cpu().numpy()
                    k = min(cap, total)
                    assert g["count"] == total and all(bytes(g["results"][e])[:52] == bytes(ref["results"][e])[:52] for e in range(E)), (cap, dtype)
                    assert np.array_equal(bits(g["models"]), bits(ref["models"])) and np.array_equal(g["counts"], ref["counts"]), cap
                    recs = back[:k * 16].view(dtype)
                    assert np.array_equal(recs["left"], cat["left"][:k]) and np.array_equal(recs["right"], cat["right"][:k]), cap
                    assert np.array_equal(recs["d1"].astype(np.int64), cat["d1"][:k].astype(np.int64))                 # the payload travels
                    assert np.array_equal(recs["d2"].astype(np.int64), cat["d2"][:k].astype(np.int64))
                    assert np.all(back[k * 16:] == 0xA5), cap
                    assert np.array_equal(src.cpu().numpy(), host), cap                                                # the input is only read
        # the bad index: through the one device flag, nothing written
        opts = capi.ransac_opts(gc.TOL, N, seed, True)
        last_left = c["edges"][-1][0]
        lists = [p.copy() for p in c["lists"]]
        lists[-1]["left"][len(lists[-1]) - 1] = c["lens"][last_left]
        assert c["lens"][last_left] < max(c["lens"])
        rv, res, cnt, out, models, counts = _ransac_raw(capi, dev, model, lists, c["edges"], opts, total_pairs)
        assert rv == -1 and cnt == -77 and np.all(out == -7) and np.all(models == -7) and np.all(counts == -7)
        assert bytes(res) == b"\x5a" * C.sizeof(res)
        ref = getattr(capi, "ransac_%s_graph_ref" % model)(c["lists"], c["edges"], c["xys"], opts)
        rv, res, cnt, out, models, counts = _ransac_raw(capi, dev, model, c["lists"], c["edges"], opts, total_pairs)
        assert rv == 0 and cnt == ref["count"] and same_records(out[:4 * cnt].view(PAIR_DTYPE), ref["records"])
    finally:
        dev.close()


# ---- the guided re-match --------------------------------------------------------------------------------------------------
GUIDED_CASES = {"mixed": (41, gcs.MIXED_LENS, gcs.MIXED_EDGES), "lefts": (42, gcs.LEFTS_LENS, gcs.LEFTS_EDGES)}


def _guided_raw(capi, dev, edges, guides, ratio, mutual, cap, pdesc=None, pxy=None):
    """psx_match_pairs_guided_graph_u8 with sentinel-filled outputs: (rc, per-edge counts, count, records int32 words)"""
    E, k = len(edges), len(dev.lens)
    pd = (C.c_void_p * max(k, 1))(*(dev.pdesc if pdesc is None else pdesc))
    px = (C.c_void_p * max(k, 1))(*(dev.pxy if pxy is None else pxy))
    la, ea = np.array(dev.lens, np.int32), np.array(edges, np.int32).reshape(-1, 2)
    ga = (capi.Guide * max(E, 1))(*guides)
    out = np.full((cap + 2) * 4, -7, np.int32)
    sc = np.full(E + 2, -9, np.int32)
    n = C.c_int(-77)
    o = capi.match_opts(ratio, mutual)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    rv = dev.L.psx_match_pairs_guided_graph_u8(0, pd, px, ptr(la), k, ptr(ea), E, ga, C.byref(o), ptr(out) if cap else None, cap, ptr(sc), C.byref(n))
    return rv, sc, n.value, out


def _guided_single(capi, dev, a, b, guide, ratio, mutual):
    """psx_match_pairs_guided_u8_dev for one edge on the same device arrays, read back: PAIR_U8 records"""
    cap = dev.lens[a]
    if cap == 0 or dev.lens[b] == 0:
        return np.zeros(0, U8)
    dbuf = torch.zeros((cap * 16,), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    n = capi.match_pairs_guided_dev(dev.pdesc[a], dev.pxy[a], dev.lens[a], dev.pdesc[b], dev.pxy[b], dev.lens[b], guide, dbuf.data_ptr(), cap,
                                    ratio, mutual, u8=True)
    return dbuf.cpu().numpy()[:n * 16].view(U8).copy()


@pytest.mark.parametrize("mutual", [False, True], ids=["oneway", "mutual"])
@pytest.mark.parametrize("case", sorted(GUIDED_CASES))
def test_guided_graph_equals_the_single_calls_and_the_restatement(capi, case, mutual):
    """guides per edge that mix homography, epipolar and NONE, over views of unequal length (1, 255, 256, 257, 300, 600 rows
    among them); the four ratios; a capacity inside an edge; the sets once as separate allocations and once as slices"""
    seed, lens, edges = GUIDED_CASES[case]
    sets, xys, _ = gc.scene(seed, lens)
    guides = [gc.edge_guide(e, a, b) for e, (a, b) in enumerate(edges)]
    cg = [gc.capi_guide(capi, g) for g in guides]
    assert {g[0] for g in guides} == {gc.NONE, 1, 2}
    room = sum(lens[a] for a, _ in edges)
    dev = _Views(capi, xys, sets)
    try:
        # the same views as slices of ONE descriptor buffer and ONE position buffer
        flat_d = torch.from_numpy(np.concatenate([s.reshape(-1) for s in sets])).cuda()
        flat_x = torch.from_numpy(np.concatenate([x.reshape(-1) for x in xys])).cuda()
        torch.cuda.synchronize()
        offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        sl_d = [flat_d.data_ptr() + 128 * int(offs[v]) if lens[v] else None for v in range(len(lens))]
        sl_x = [flat_x.data_ptr() + 8 * int(offs[v]) if lens[v] else None for v in range(len(lens))]
        for ratio in RATIOS:
            want = [gc.guided_expected(capi, seed, lens, e, a, b, guides[e], ratio, mutual) for e, (a, b) in enumerate(edges)]
            cat = gc.concat(want, U8)
            total = len(cat)
            rv, sc, n, out = _guided_raw(capi, dev, edges, cg, ratio, mutual, room)
            assert rv == 0 and n == total and list(sc[:len(edges)]) == [len(w) for w in want] and list(sc[len(edges):]) == [-9, -9], (ratio, sc)
            assert same_records(out[:4 * total].view(U8), cat) and np.all(out[4 * total:] == -7), ratio
            for e, (a, b) in enumerate(edges):
                if guides[e][0] == gc.NONE:
                    assert sc[e] == 0, e                                                     # a skipped edge leaves its count at 0
                elif ratio == 0.8 or e % 2 == 0:
                    assert same_records(_guided_single(capi, dev, a, b, cg[e], ratio, mutual), want[e]), (e, ratio)
            if ratio == 0.8:
                live = [len(w) for w in want if len(w) > 2]
                assert len(live) >= 3 and total > 40, "the planted scene gives pairs under the guides"
                first = next(e for e, w in enumerate(want) if len(w) > 2)
                inside = sum(len(w) for w in want[:first]) + 2                              # a cut inside an edge
                for cap in (inside, 0):
                    rv, sc2, n2, out2 = _guided_raw(capi, dev, edges, cg, ratio, mutual, cap)
                    assert rv == 0 and n2 == total and np.array_equal(sc2, sc), cap
                    assert same_records(out2[:4 * cap].view(U8), cat[:cap]) and np.all(out2[4 * cap:] == -7), cap
                rv, sc3, n3, out3 = _guided_raw(capi, dev, edges, cg, ratio, mutual, room, pdesc=sl_d, pxy=sl_x)
                assert rv == 0 and n3 == total and np.array_equal(sc3, sc) and np.array_equal(out3, out), "slices of one buffer"
        # the python wrapper on host arrays
        lists, counts = capi.match_pairs_guided_graph_u8(sets, xys, edges, cg, 0.8, mutual)
        want = [gc.guided_expected(capi, seed, lens, e, a, b, guides[e], 0.8, mutual) for e, (a, b) in enumerate(edges)]
        assert all(same_records(l, w) for l, w in zip(lists, want)) and list(counts) == [len(w) for w in want]
    finally:
        dev.close()


# ---- the chain ------------------------------------------------------------------------------------------------------------
CHAIN_LENS = (300, 257, 64, 129, 513, 200)
CHAIN_EDGES = [(a, b) for a in range(6) for b in range(6) if a != b]


def _chain(capi, dev, edges, ransac_opts, d_pairs, d_inl, d_re, room):
    """match -> verify -> guides -> re-match over `edges`, the records staying in the three device buffers"""
    ec, n1 = capi.match_pairs_graph_dev(dev.pdesc, dev.lens, edges, d_pairs.data_ptr(), room, 0.8, True)
    g = capi.ransac_homography_graph_dev(d_pairs.data_ptr(), ec, edges, dev.pxy, dev.lens, d_inl.data_ptr(), room, ransac_opts)
    guides = capi.guides_from_ransac(g["results"], capi.GUIDE_HOMOGRAPHY, gc.TOL)
    rc, n3 = capi.match_pairs_guided_graph_dev(dev.pdesc, dev.pxy, dev.lens, edges, guides, d_re.data_ptr(), room, 0.8, True)
    return ec, n1, g, guides, rc, n3


def test_chain_on_the_device_equals_the_loops_of_single_calls(capi):
    """psx_match_pairs_graph_u8_dev -> psx_ransac_homography_graph_dev -> psx_guides_from_ransac ->
    psx_match_pairs_guided_graph_u8_dev on six views of one scene, all 30 ordered pairs, the records never leaving HBM: every
    stage equals the loop of single calls per edge, and the re-match of a verified edge holds every mutual unguided pair
    that its guide admits"""
    sets, xys, _ = gc.scene(43, CHAIN_LENS)
    edges = CHAIN_EDGES
    assert len(edges) == 30
    room = sum(CHAIN_LENS[a] for a, _ in edges)
    opts = capi.ransac_opts(gc.TOL, 256, 9, True)
    dev = _Views(capi, xys, sets)
    try:
        d_pairs, d_inl, d_re = (torch.full((room * 16,), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(3))
        torch.cuda.synchronize()
        ec, n1, g, guides, rc, n3 = _chain(capi, dev, edges, opts, d_pairs, d_inl, d_re, room)
        pairs = d_pairs.cpu().numpy()[:n1 * 16].view(U8)
        inl = d_inl.cpu().numpy()[:g["count"] * 16].view(U8)
        re = d_re.cpu().numpy()[:n3 * 16].view(U8)
        p_lists, i_lists, r_lists = capi.split_sets(pairs, ec), capi.split_sets(inl, [r.inliers for r in g["results"]]), capi.split_sets(re, rc)
        assert n1 == int(np.sum(ec)) and n3 == int(np.sum(rc)) and g["count"] == sum(r.inliers for r in g["results"])
        ref = capi.ransac_homography_graph_ref(p_lists, edges, xys, opts)
        verified = 0
        for e, (a, b) in enumerate(edges):
            # stage 1 against the single matcher and numpy
            one = capi.match_pairs_u8(sets[a], sets[b], 0.8, True)
            assert same_records(p_lists[e], one), e
            if e % 7 == 0:
                assert same_records(p_lists[e], gcs.numpy_pairs(sets[a], sets[b], 0.8, True)), e
            # stage 2 against the single device call on the same arrays and the host reference
            s = _ransac_single(capi, dev, "homography", a, b, p_lists[e], opts)
            res = g["results"][e]
            assert bytes(res)[:52] == bytes(s["result"])[:52] == bytes(ref["results"][e])[:52], e
            assert same_records(i_lists[e], s["inliers"]) and same_records(i_lists[e], ref["inliers"][e]), e
            # stage 3 against the single guided device call
            if res.best < 0:
                assert guides[e].kind == capi.GUIDE_NONE and rc[e] == 0, e
                continue
            verified += 1
            assert guides[e].kind == capi.GUIDE_HOMOGRAPHY and np.array_equal(bits(np.array(list(guides[e].m), np.float32)), bits(np.array(list(res.m), np.float32)))
            assert same_records(r_lists[e], _guided_single(capi, dev, a, b, guides[e], 0.8, True)), e
            ok = np.diag(capi.guide_allows(guides[e], xys[a][p_lists[e]["left"]], xys[b][p_lists[e]["right"]]))
            have = set(zip(r_lists[e]["left"].tolist(), r_lists[e]["right"].tolist()))
            assert all((int(l), int(r)) in have for l, r in zip(p_lists[e]["left"][ok], p_lists[e]["right"][ok])), e
            assert ok.sum() >= 4, e
        assert verified >= 25
        assert dev.L.psx_match_release() == 0
    finally:
        dev.close()


def test_grouped_by_left_equals_the_one_to_many_calls(capi):
    """with the list grouped by left, each view's slice of both new calls' output is what ransac_*_many_dev and
    match_pairs_guided_many_dev return for that star"""
    sets, xys, _ = gc.scene(43, CHAIN_LENS)
    edges = CHAIN_EDGES                                    # a outer, b inner: grouped by left
    room = sum(CHAIN_LENS[a] for a, _ in edges)
    opts = capi.ransac_opts(gc.TOL, 128, 4, True)
    dev = _Views(capi, xys, sets)
    try:
        d_pairs, d_inl, d_re, d_star = (torch.full((room * 16,), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(4))
        torch.cuda.synchronize()
        for model, kind in (("homography", capi.GUIDE_HOMOGRAPHY), ("fundamental", capi.GUIDE_EPIPOLAR)):
            ec, n1 = capi.match_pairs_graph_dev(dev.pdesc, dev.lens, edges, d_pairs.data_ptr(), room, 0.8, True)
            g = getattr(capi, "ransac_%s_graph_dev" % model)(d_pairs.data_ptr(), ec, edges, dev.pxy, dev.lens, d_inl.data_ptr(), room, opts)
            guides = capi.guides_from_ransac(g["results"], kind, gc.TOL)
            rc, n3 = capi.match_pairs_guided_graph_dev(dev.pdesc, dev.pxy, dev.lens, edges, guides, d_re.data_ptr(), room, 0.8, True)
            inl, re = d_inl.cpu().numpy(), d_re.cpu().numpy()
            p_at = i_at = r_at = 0
            for a in range(6):
                star = [e for e, (l, _) in enumerate(edges) if l == a]
                others = [edges[e][1] for e in star]
                cnts = [int(ec[e]) for e in star]
                m = getattr(capi, "ransac_%s_many_dev" % model)(d_pairs.data_ptr() + 16 * p_at, cnts, dev.pxy[a], dev.lens[a], [dev.pxy[b] for b in others],
                                                              [dev.lens[b] for b in others], d_star.data_ptr(), room, opts)
                assert all(bytes(m["results"][i])[:52] == bytes(g["results"][e])[:52] for i, e in enumerate(star)), (model, a)
                got = d_star.cpu().numpy()[:m["count"] * 16]
                assert np.array_equal(got, inl[16 * i_at:16 * (i_at + m["count"])]), (model, a)
                sc, n = capi.match_pairs_guided_many_dev(dev.pdesc[a], dev.pxy[a], dev.lens[a], [dev.pdesc[b] for b in others], [dev.pxy[b] for b in others],
                                                         [dev.lens[b] for b in others], [guides[e] for e in star], d_star.data_ptr(), room, 0.8, True)
                assert list(sc) == [int(rc[e]) for e in star], (model, a)
                assert np.array_equal(d_star.cpu().numpy()[:n * 16], re[16 * r_at:16 * (r_at + n)]), (model, a)
                p_at, i_at, r_at = p_at + sum(cnts), i_at + m["count"], r_at + n
            assert p_at == n1 and i_at == g["count"] and r_at == n3 > 100
    finally:
        dev.close()


def test_repeated_calls_with_other_edge_lists_equal_fresh_calls(capi):
    """two chains in a row with different edge lists, within the scratch the first one sized, give what each gives as the
    first call after a release of the scratch: nothing leaks from one call into the next"""
    sets, xys, _ = gc.scene(43, CHAIN_LENS)
    big, small = CHAIN_EDGES, [(4, 0), (1, 1), (0, 4), (5, 2), (4, 0)]
    room = sum(CHAIN_LENS[a] for a, _ in big)
    opts = capi.ransac_opts(gc.TOL, 65, 4, True)
    dev = _Views(capi, xys, sets)
    try:
        def run(edges):
            bufs = [torch.full((room * 16,), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(3)]
            torch.cuda.synchronize()
            ec, n1, g, guides, rc, n3 = _chain(capi, dev, edges, opts, bufs[0], bufs[1], bufs[2], room)
            return (list(ec), n1, [bytes(r)[:52] for r in g["results"]], g["count"], list(rc), n3) + tuple(b.cpu().numpy().tobytes() for b in bufs)

        assert dev.L.psx_match_release() == 0
        fresh_big = run(big)
        assert dev.L.psx_match_release() == 0
        fresh_small = run(small)
        again_big = run(big)
        again_small = run(small)                           # within the capacity the big list left
        again_small2 = run(small)
        assert again_big == fresh_big and again_small == fresh_small == again_small2
        assert fresh_small[5] > 0 and fresh_small[4][0] == fresh_small[4][4]
    finally:
        dev.close()


def test_cpp_graph_chain_on_the_gpu(tmp_path):
    """tests/cpp/test_graph_chain_api.cpp with POPSIFT_TEST_EXPECT_GPU: estimate*Graph and matchPairsGuidedGraph equal the
    per-edge member calls field by field"""
    libdir = os.path.join(ROOT, "popsift_amd", "lib")
    exe = str(tmp_path / "test_graph_chain_api")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-pthread", os.path.join(ROOT, "tests", "cpp", "test_graph_chain_api.cpp"), "-o", exe,
                           "-I", os.path.join(ROOT, "popsift_amd", "csrc", "include"), "-I", os.path.join(ROOT, "include"),
                           "-L", libdir, "-lpopsift", "-lpopsift_hip", "-Wl,-rpath," + libdir])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300,
                         env=dict(os.environ, POPSIFT_TEST_EXPECT_GPU="1"))
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout
    assert "estimate*Graph:" in out.stdout and "matchPairsGuidedGraph:" in out.stdout
