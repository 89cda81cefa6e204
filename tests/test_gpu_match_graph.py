"""GPU tests of the pair search over an edge list (include/popsift_hip.h, "a list of view pairs over N descriptor sets"):
psx_match_pairs_graph_u8, its _dev form and FeaturesDev::matchPairsGraph.  The contract is "the concatenation, in the order of
the edge list, of what psx_match_pairs_u8 returns per edge": every slice is compared, as bytes, with that call on the same
device arrays in the same process; for the edges between set 0 and a large set also with the HOST join (capi.pairs_join) of
the oracle's directed results, so the check does not rest on the device code alone.  No tolerances anywhere."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch        # before the HIP library is loaded: torch brings a HIP runtime of its own and must initialise first (_dev form)

from tests.match_graph_cases import (BIG_EDGES, BIG_LENS, BIG_SEED, LEFTS_EDGES, LEFTS_LENS, LEFTS_SEED, MIXED_EDGES, MIXED_LENS,
                                     MIXED_PREMISE, MIXED_SEED, TINY_EDGES, contract, graph_sets, slices, tiny_sets)
from tests.match_pairs_cases import RATIOS, assert_premise, directed, planted, same_records

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Views:
    """N sets uploaded once -- as separate allocations, or as slices of ONE buffer (concat) --; the graph call, the single
    call and the one-to-many call on the same device arrays"""

    def __init__(self, capi, sets, concat=False):
        self.capi, self.L, self.bufs = capi, capi.lib(), []
        self.sets = [np.ascontiguousarray(s, np.uint8).reshape(-1, 128) for s in sets]
        self.lens = [len(s) for s in self.sets]
        if concat:
            (base,) = capi._to_device(self.L, 0, [np.concatenate(self.sets)], self.bufs)
            offs = np.concatenate([[0], np.cumsum(self.lens)]).astype(np.int64) * 128
            self.ptrs = [C.c_void_p((base.value or 0) + int(o)) if n else C.c_void_p() for o, n in zip(offs, self.lens)]
        else:
            self.ptrs = capi._to_device(self.L, 0, self.sets, self.bufs)

    def graph(self, edges, ratio, mutual, capacity=None):
        """(records, per-edge counts, total)"""
        cap = sum(self.lens[a] for a, _ in edges) if capacity is None else capacity
        out = np.zeros((cap,), self.capi.PAIR_U8_DTYPE)
        counts, n = self.capi._graph_call(self.L.psx_match_pairs_graph_u8, "psx_match_pairs_graph_u8", 0, self.ptrs, self.lens, edges,
                                          out.ctypes.data_as(C.c_void_p) if cap else None, cap, ratio, mutual)
        return out[:min(n, cap)], counts, n

    def single(self, a, b, ratio, mutual):
        return self.capi._pairs_call(self.L.psx_match_pairs_u8, "psx_match_pairs_u8", 0, self.ptrs[a], self.lens[a], self.ptrs[b], self.lens[b],
                                     ratio, mutual, self.capi.PAIR_U8_DTYPE, None)[0]

    def many(self, a, bs, ratio, mutual):
        cap = self.lens[a] * len(bs)
        out = np.zeros((cap,), self.capi.PAIR_U8_DTYPE)
        counts, n = self.capi._many_call(self.L.psx_match_pairs_many_u8, "psx_match_pairs_many_u8", 0, self.ptrs[a], self.lens[a],
                                         [self.ptrs[b] for b in bs], [self.lens[b] for b in bs], out.ctypes.data_as(C.c_void_p), cap, ratio, mutual)
        return out[:n], counts, n

    def close(self):
        for p in self.bufs:
            self.L.psx_dev_free(0, p)
        self.bufs = []


def _equal_singles(dev, edges, ratio, mutual, what, other=None):
    """one call against the loop of single calls (on `other`'s arrays when given): every slice, the counts, the total;
    returns the per-edge lists"""
    got, counts, total = dev.graph(edges, ratio, mutual)
    memo = {}
    for e in edges:
        if e not in memo:
            memo[e] = (other or dev).single(e[0], e[1], ratio, mutual)
    per_edge = [memo[e] for e in edges]
    want, wcounts, wtotal = contract(per_edge)
    assert total == wtotal and np.array_equal(counts, wcounts), (what, ratio, mutual, list(counts), list(wcounts))
    for k, (a, b) in enumerate(zip(slices(got, counts), per_edge)):
        assert same_records(a, b), (what, ratio, mutual, edges[k], len(a), len(b))
    assert got.tobytes() == want.tobytes()
    return per_edge


# ---- 1. equals the single calls ---------------------------------------------------------------------------------------------
def test_graph_equals_the_single_calls(oracle, capi):
    """the mixed list -- unsorted, (0,1) and (1,0), a self edge, (3,4) and (4,3), an empty right and an empty left, a one-row
    set both ways, a duplicate -- for every ratio and both flag values: each slice equals psx_match_pairs_u8 on the edge's
    two sets, the counts and the total are equal.  The generator's premise (a pair kept, one dropped by the ratio, one dropped
    by the cross-check alone) is asserted on the oracle's directed results of the edges between set 0 and set 1, and those
    edges are also held to the host join; every other edge with two non-empty sides returns a pair at ratio inf."""
    sets = graph_sets(MIXED_SEED, MIXED_LENS)
    dev = _Views(capi, sets)
    try:
        joins = {}
        for a, b in MIXED_PREMISE:
            fm, fd, bm, bd = directed(oracle, ("graph", MIXED_SEED, a, b), sets[a], sets[b], True)
            assert_premise(fm, fd, bm, len(sets[b]), (a, b))
            joins[(a, b)] = (fm, fd, bm)
        for ratio in RATIOS:
            for mutual in (False, True):
                per_edge = _equal_singles(dev, MIXED_EDGES, ratio, mutual, "mixed")
                for e, p in zip(MIXED_EDGES, per_edge):
                    live = MIXED_LENS[e[0]] > 0 and MIXED_LENS[e[1]] > 0
                    assert live or len(p) == 0, e
                    if e in joins:
                        fm, fd, bm = joins[e]
                        want = capi.pairs_join(fm, fd, bm if mutual else None, MIXED_LENS[e[1]], ratio, mutual)
                        assert same_records(p, want), (e, ratio, mutual, len(p), len(want))
                    elif live and ratio == float("inf"):
                        assert len(p) >= 1, (e, mutual)
                    if e == (0, 0):                              # every row finds itself at distance 0
                        assert len(p) == 300 and np.all(p["left"] == p["right"]) and np.all(p["d1"] == 0), (ratio, mutual)
        got, counts, total = dev.graph(MIXED_EDGES, 0.8, True)
        print("mixed: %s over %s -> %s pairs" % (MIXED_EDGES, list(MIXED_LENS), list(counts)))
        # the python wrapper: per-edge arrays from host arrays
        lists, c2 = capi.match_pairs_graph_u8(sets, MIXED_EDGES, 0.8, True)
        assert np.array_equal(c2, counts) and all(same_records(x, y) for x, y in zip(lists, slices(got, counts)))
    finally:
        dev.close()


# ---- 2. different left lengths in one join ----------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,lens,edges", [(LEFTS_SEED, LEFTS_LENS, LEFTS_EDGES), (BIG_SEED, BIG_LENS, BIG_EDGES)], ids=["1-255-256-257-600", "2500-2300-700"])
def test_left_lengths_differ_within_one_join(capi, seed, lens, edges):
    """left lengths 1, 255, 256, 257 and 600 in one call -- a join workgroup table whose segments differ in length --, and
    (2500, 2300, 700) with all six ordered pairs: several blocks, several chunks and several join workgroups per edge"""
    dev = _Views(capi, graph_sets(seed, lens))
    try:
        if seed == LEFTS_SEED:
            assert {lens[a] for a, _ in edges} == {1, 255, 256, 257, 600}
        for ratio, mutual in ((0.8, True), (0.8, False), (float("inf"), True), (0.6, True)):
            per_edge = _equal_singles(dev, edges, ratio, mutual, lens)
            if ratio == float("inf"):
                assert all(len(p) >= 1 for p in per_edge)
        info = capi.match_graph_plan(lens, edges, True)
        assert info["launches"] == 8 and info["join_workgroups"] == sum(-(-lens[a] // 256) for a, _ in edges) > len(edges)
    finally:
        dev.close()


# ---- 3. a star equals the one-to-many call ----------------------------------------------------------------------------------
def test_a_star_equals_the_one_to_many_call(capi):
    """edges (a, b_0) .. (a, b_{K-1}) return the bytes and counts of psx_match_pairs_many_u8(a, {b_k}); in a list grouped by
    left, each left view's slice of the records and of the counts is that view's one-to-many result"""
    lens = (300, 257, 0, 1, 33, 513, 255)
    dev = _Views(capi, graph_sets(21, lens))
    try:
        for ratio, mutual in ((0.8, True), (0.8, False), (float("inf"), True)):
            bs = [1, 2, 3, 4, 5, 6, 1]
            got, counts, total = dev.graph([(0, b) for b in bs], ratio, mutual)
            want, wcounts, wtotal = dev.many(0, bs, ratio, mutual)
            assert total == wtotal > 0 and np.array_equal(counts, wcounts) and got.tobytes() == want.tobytes(), (ratio, mutual)
            stars = [(0, [1, 5, 6]), (5, [0, 4]), (1, [5, 0, 1])]
            got, counts, total = dev.graph([(a, b) for a, bs in stars for b in bs], ratio, mutual)
            at_rec = at_cnt = 0
            for a, bs in stars:
                want, wcounts, wtotal = dev.many(a, bs, ratio, mutual)
                assert wtotal > 0 and np.array_equal(counts[at_cnt:at_cnt + len(bs)], wcounts), (a, ratio, mutual)
                assert got[at_rec:at_rec + wtotal].tobytes() == want.tobytes(), (a, ratio, mutual)
                at_rec, at_cnt = at_rec + wtotal, at_cnt + len(bs)
            assert at_rec == total
    finally:
        dev.close()


# ---- 4. nothing leaks across a set boundary ---------------------------------------------------------------------------------
@pytest.mark.parametrize("lens", [(33, 40), (255, 256, 257, 40)], ids=["33", "255-256-257"])
def test_no_leak_across_a_set_boundary(capi, lens):
    """The sets are slices of ONE buffer: s_0 .. s_{n-1} of the given lengths, then the 300-row set `left` they are matched
    against.  Every s_k starts with 31 exact copies of rows of `left`, so each s_k is followed by rows that are at distance 0
    from rows of the other side of its edges: a tile, or an outer block, that ran past its set's last row would meet them.
    33 rows: the last tile holds one row of the set and 31 of the next; 255 / 256 / 257: an outer block ends inside a tile,
    at a tile, one past.  Edges run both ways -- every set is outer in one direction and inner in the other -- and between
    neighbouring s_k.  Every slice must equal the stand-alone single call on separate allocations."""
    rng = np.random.default_rng(sum(lens))
    left = rng.integers(0, 64, (300, 128), dtype=np.uint8)
    sets = []
    for k, n in enumerate(lens):
        r = rng.integers(0, 64, (n, 128), dtype=np.uint8)
        r[:31] = left[40 * k:40 * k + 31]                   # exact copies: distance 0 for whoever reads them
        r[31 + k] = left[200 + k] ^ 1                       # and one near-copy of its own, so that no list is trivial
        sets.append(r)
    sets.append(left)                                       # the last set; it follows s_{n-1} in the buffer
    n = len(lens)
    edges = [(n, k) for k in range(n)] + [(k, n) for k in range(n)] + [(k, (k + 1) % n) for k in range(n)]
    cat, alone = _Views(capi, sets, concat=True), _Views(capi, sets)
    try:
        for ratio, mutual in ((0.8, False), (0.8, True), (float("inf"), True), (float("inf"), False)):
            per_edge = _equal_singles(cat, edges, ratio, mutual, lens, other=alone)
            for (a, b), p in zip(edges, per_edge):
                assert len(p) >= 31 or n not in (a, b), (a, b, ratio, mutual, len(p))
                assert len(p) == 0 or (p["right"].max() < len(sets[b]) and p["left"].max() < len(sets[a])), (a, b, ratio, mutual)
    finally:
        cat.close(); alone.close()


# ---- 5. ties ----------------------------------------------------------------------------------------------------------------
def test_ties_keep_the_earlier_index(oracle, capi):
    """the 1100-row case of test_gpu_match_many.py as edges in both directions: rows 500 .. 900 identical, so a left row one
    step away gets best = 500 and d2 == d1 (kept by ratio inf alone), a left row EQUAL to them has 0 / 0 and is never kept;
    in the other direction 401 identical left rows all want the same right row and the cross-check keeps the first.  Also
    all-0 against all-255, both ways.  The directed results are the oracle's."""
    rng = np.random.default_rng(6)
    big = rng.integers(0, 64, (1100, 128), dtype=np.uint8)
    big[500:901] = big[500]
    left = rng.integers(0, 64, (40, 128), dtype=np.uint8)
    left[7] = big[500]
    left[9] = big[500]
    left[9, 3] += 1
    fm, fd, bm, bd = directed(oracle, ("many ties",), left, big, True)
    assert list(fm[9, :2]) == [500, 501] and list(fd[9]) == [1, 1] and list(fm[7, :2]) == [500, 501] and list(fd[7]) == [0, 0]
    zeros, full = np.zeros((3, 128), np.uint8), np.full((2, 128), 255, np.uint8)
    edges = [(1, 0), (0, 1), (2, 3), (3, 2), (1, 1)]
    dev = _Views(capi, [left, big, zeros, full])
    try:
        for ratio in RATIOS:
            for mutual in (False, True):
                per_edge = _equal_singles(dev, edges, ratio, mutual, "ties")
                assert same_records(per_edge[1], capi.pairs_join(fm, fd, bm if mutual else None, 1100, ratio, mutual)), (ratio, mutual)
                assert same_records(per_edge[0], capi.pairs_join(bm, bd, fm if mutual else None, 40, ratio, mutual)), (ratio, mutual)
        got = slices(*dev.graph(edges, float("inf"), False)[:2])
        row = got[1][got[1]["left"] == 9]
        assert len(row) == 1 and row["right"][0] == 500 and row["d1"][0] == row["d2"][0] == 1
        assert 7 not in got[1]["left"] and 9 not in slices(*dev.graph(edges, 1.0, False)[:2])[1]["left"]
        back = got[0][(got[0]["left"] >= 500) & (got[0]["left"] <= 900)]
        assert len(back) == 401 and np.all(back["right"] == 7) and np.all(back["d1"] == 0)
        mut = slices(*dev.graph(edges, float("inf"), True)[:2])
        assert list(mut[0]["left"][(mut[0]["left"] >= 500) & (mut[0]["left"] <= 900)]) == [500]          # the cross-check keeps the earliest
        # all-0 against all-255: two rows give d1 == d2, a quotient of exactly 1
        assert list(got[2]["left"]) == [0, 1, 2] and np.all(got[2]["right"] == 0) and np.all(got[2]["d1"] == 128 * 255 * 255) and np.all(got[2]["d2"] == 128 * 255 * 255)
        assert list(got[3]["left"]) == [0, 1] and np.all(got[3]["right"] == 0)
        assert list(dev.graph(edges, 1.0, False)[1][2:4]) == [0, 0]
        assert list(dev.graph(edges, float("inf"), True)[1][2:4]) == [1, 1]
    finally:
        dev.close()


# ---- 6. capacity ------------------------------------------------------------------------------------------------------------
def test_capacity_and_counts(capi):
    """truncation inside an edge, exactly at an edge boundary, at count - 1 and at 0 with NULL: the totals are still reported,
    the bytes behind the capacity are untouched -- in a host buffer and in a device buffer read back"""
    lens, edges = (257, 64, 1000, 300), [(0, 2), (1, 0), (3, 2), (0, 3)]
    sets = graph_sets(22, lens)
    dev = _Views(capi, sets)
    L = capi.lib()
    try:
        full, counts, total = dev.graph(edges, 0.8, True)
        assert np.all(counts > 4) and total == counts.sum() == len(full)
        ts = [torch.from_numpy(s).cuda() for s in dev.sets]
        for cap in (int(counts[0] + counts[1] // 2), int(counts[0]), int(counts[0] + counts[1]), total - 1, 0, total, total + 3):
            host = np.full(((cap + 2) * 4,), -7, np.int32).view(capi.PAIR_U8_DTYPE)
            c2, n2 = capi._graph_call(L.psx_match_pairs_graph_u8, "psx_match_pairs_graph_u8", 0, dev.ptrs, dev.lens, edges,
                                      host.ctypes.data_as(C.c_void_p) if cap else None, cap, 0.8, True)
            k = min(cap, total)
            assert n2 == total and np.array_equal(c2, counts), cap
            assert same_records(host[:k], full[:k]) and np.all(host[k:].view(np.int32) == -7), cap
            want, _, _ = contract(slices(full, counts), cap)
            assert same_records(host[:k], want)
            dbuf = torch.full(((cap + 2) * 16,), 0xA5, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            c3, n3 = capi.match_pairs_graph_dev([t.data_ptr() for t in ts], dev.lens, edges, dbuf.data_ptr() if cap else 0, cap, 0.8, True)
            back = dbuf.cpu().numpy()
            assert n3 == total and np.array_equal(c3, counts), cap
            assert same_records(back[:k * 16].view(capi.PAIR_U8_DTYPE), full[:k]) and np.all(back[k * 16:] == 0xA5), cap
        # the python wrapper: per-edge arrays, cut as the call cut them
        lists, c4 = capi.match_pairs_graph_u8(sets, edges, 0.8, True, capacity=int(counts[0]) + 2)
        assert np.array_equal(c4, counts) and [len(p) for p in lists] == [counts[0], 2, 0, 0]
        assert same_records(lists[0], full[:counts[0]]) and same_records(lists[1], full[counts[0]:counts[0] + 2])
    finally:
        dev.close()


# ---- 7. 400 edges over 200 tiny sets ----------------------------------------------------------------------------------------
def test_four_hundred_edges_over_tiny_sets(capi):
    """the 200 sets of tiny_many (i % 41 rows, empty ones in between), edge i = (i % 200, (7 i + 3) % 200): hundreds of
    workgroup totals in the scan, edges without any workgroup among them, sets shorter than a tile"""
    sets = tiny_sets()
    dev = _Views(capi, sets, concat=True)
    try:
        for ratio, mutual in ((0.8, True), (float("inf"), True), (float("inf"), False)):
            per_edge = _equal_singles(dev, TINY_EDGES, ratio, mutual, "tiny")
        live = [len(sets[a]) > 0 and len(sets[b]) > 0 for a, b in TINY_EDGES]
        assert [len(p) > 0 for p in per_edge] == live and sum(live) == 380
        assert all(len(p) == len(sets[a]) for p, (a, b), ok in zip(per_edge, TINY_EDGES, live) if ok)   # ratio inf, no cross-check: every left row
    finally:
        dev.close()


# ---- 8. the partials' budget ------------------------------------------------------------------------------------------------
def test_groups_of_edges_above_the_partials_budget(capi):
    """one set of 18 432 rows, the self edge listed 64 times: 64 x 36 chunks x 18 432 rows of partials per direction (340
    MB), above the 256 MiB budget, so both directions run in two groups of whole edges on the stream -- the plan says so.
    Every slice equals the single call."""
    left, _ = planted(18432, 18432, 18432)
    edges = [(0, 0)] * 64
    info = capi.match_graph_plan((18432,), edges, True)
    assert info["fwd_groups"] == 2 and info["bwd_groups"] == 2 and info["launches"] == 12 and info["scratch_bytes"] <= 256 << 20
    dev = _Views(capi, [left])
    try:
        want = dev.single(0, 0, 0.8, True)
        assert len(want) > 1000
        got, counts, total = dev.graph(edges, 0.8, True)
        assert total == 64 * len(want) and np.all(counts == len(want))
        assert got.tobytes() == want.tobytes() * 64
    finally:
        dev.close()


# ---- 9. the scratch ---------------------------------------------------------------------------------------------------------
def test_scratch_beside_the_other_matchers(capi):
    """on one thread's scratch, in sequence: the graph call, psx_match_pairs_many_u8, psx_match_pairs_u8, the graph call again
    (identical bytes), psx_match_release, the graph call once more"""
    dev = _Views(capi, graph_sets(MIXED_SEED, MIXED_LENS))
    try:
        first, counts, total = dev.graph(MIXED_EDGES, 0.8, True)
        assert total > 50
        many, mcounts, mtotal = dev.many(0, [1, 4], 0.8, True)
        one = dev.single(0, 1, 0.8, True)
        assert same_records(one, slices(first, counts)[MIXED_EDGES.index((0, 1))]) and same_records(one, many[:mcounts[0]])
        again, c2, t2 = dev.graph(MIXED_EDGES, 0.8, True)
        assert t2 == total and np.array_equal(c2, counts) and again.tobytes() == first.tobytes()
        assert capi.lib().psx_match_release() == 0
        third, c3, t3 = dev.graph(MIXED_EDGES, 0.8, True)
        assert t3 == total and np.array_equal(c3, counts) and third.tobytes() == first.tobytes()
        assert same_records(dev.single(0, 1, 0.8, True), one)
    finally:
        dev.close()


# ---- 10. C++ ----------------------------------------------------------------------------------------------------------------
def test_cpp_match_pairs_graph_on_the_gpu(tmp_path):
    """tests/cpp/test_match_graph_api.cpp with POPSIFT_TEST_EXPECT_GPU: FeaturesDev::matchPairsGraph equals the loop of
    matchPairs with MatchOptions::bytes, field by field, with and without the cross-check; the throws happen."""
    libdir = os.path.join(ROOT, "popsift_amd", "lib")
    exe = str(tmp_path / "test_match_graph_api")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-pthread", os.path.join(ROOT, "tests", "cpp", "test_match_graph_api.cpp"), "-o", exe,
                           "-I", os.path.join(ROOT, "popsift_amd", "csrc", "include"), "-I", os.path.join(ROOT, "include"),
                           "-L", libdir, "-lpopsift", "-lpopsift_hip", "-Wl,-rpath," + libdir])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300,
                         env=dict(os.environ, POPSIFT_TEST_EXPECT_GPU="1"))
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout
    assert "mutual 0:" in out.stdout and "mutual 1:" in out.stdout
