"""GPU tests of the FLOAT pair search over an edge list (include/popsift_hip.h, "a list of view pairs over N descriptor sets,
float descriptors"): psx_match_pairs_graph and its _dev form.  The contract is "the concatenation, in edge order, of what
psx_match_pairs returns per edge": every slice is compared, as bytes, with that call on the same device arrays in the same
process -- code this call shares nothing with but the scratch --, and for two cases also with the HOST join
(capi.pairs_join) of the oracle's directed results.  psx_match_graph_f32_last says which of the two paths ran, whether the
call fell back, and what it launched and synchronised; every test asserts the path it means to exercise."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch        # before the HIP library is loaded: torch brings a HIP runtime of its own and must initialise first (_dev form)

from tests import match_graph_f32_cases as fc
from tests.match_graph_cases import contract, graph_sets, slices
from tests.match_graph_f32_worker import WORKER_COMBOS, digest
from tests.match_many_cases import TINY_LENS, planted_many
from tests.match_pairs_cases import directed, same_records

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")


class _Graph:
    """float32 sets uploaded once -- as separate allocations, or as adjacent slices of ONE buffer (concat) --; the edge-list
    call and the single call on the same device arrays"""

    def __init__(self, capi, sets, concat=False):
        self.capi, self.L, self.bufs = capi, capi.lib(), []
        self.sets = [np.ascontiguousarray(s, np.float32).reshape(-1, 128) for s in sets]
        self.lens = [len(s) for s in self.sets]
        if concat:
            base, = capi._to_device(self.L, 0, [np.concatenate(self.sets)], self.bufs)
            offs = np.concatenate([[0], np.cumsum(self.lens)]).astype(np.int64) * 512
            self.ptr = [C.c_void_p((base.value or 0) + int(o)) if n else C.c_void_p() for o, n in zip(offs, self.lens)]
        else:
            self.ptr = capi._to_device(self.L, 0, self.sets, self.bufs)
        self._single = {}

    def graph(self, edges, ratio, mutual, capacity=None):
        """(records, per-edge counts, total) through the host form; self.info: the call's"""
        cap = sum(self.lens[a] for a, _ in edges) if capacity is None else capacity
        out = np.zeros((cap,), self.capi.PAIR_DTYPE)
        counts, n = self.capi._graph_call(self.L.psx_match_pairs_graph, "psx_match_pairs_graph", 0, self.ptr, self.lens, edges,
                                          out.ctypes.data_as(C.c_void_p) if cap else None, cap, ratio, mutual)
        self.info = self.capi.match_graph_f32_last()
        return out[:min(n, cap)], counts, n

    def single(self, a, b, ratio, mutual):
        """psx_match_pairs on sets a and b; computed once per (a, b, ratio, mutual)"""
        key = (a, b, ratio, mutual)
        if key not in self._single:
            self._single[key] = self.capi._pairs_call(self.L.psx_match_pairs, "psx_match_pairs", 0, self.ptr[a], self.lens[a], self.ptr[b],
                                                      self.lens[b], ratio, mutual, self.capi.PAIR_DTYPE, None)[0]
        return self._single[key]

    def close(self):
        for p in self.bufs:
            self.L.psx_dev_free(0, p)
        self.bufs = []


def _equal_singles(dev, edges, ratio, mutual, what, path, fell_back=0):
    """one call against the loop of single calls: every slice, the counts, the total, the bytes of the concatenation; the
    path is the one the test means and the plan's, the call fell back (or not) as expected with one synchronisation more
    when it did, and launched what the plan says; returns the per-edge lists"""
    got, counts, total = dev.graph(edges, ratio, mutual)
    info = dev.info
    per_edge = [dev.single(a, b, ratio, mutual) for a, b in edges]
    want, wcounts, wtotal = contract(per_edge)
    assert total == wtotal and np.array_equal(counts, wcounts), (what, ratio, mutual, list(counts), list(wcounts))
    for e, (x, y) in enumerate(zip(slices(got, counts), per_edge)):
        assert same_records(x, y), (what, ratio, mutual, e, edges[e], len(x), len(y))
    assert got.tobytes() == want.tobytes()
    plan = dev.capi.match_graph_f32_plan(dev.lens, edges, mutual)
    assert info["path"] == path == plan["path"] == fc.planned_path(dev.lens, edges), (what, info, plan)
    assert info["fell_back"] == fell_back and info["syncs"] == 1 + fell_back, (what, ratio, mutual, info)
    if not fell_back:
        assert info["launches"] == plan["launches"], (what, info, plan)
    return per_edge


def _oracle_joins(oracle, capi, name, sets, edges):
    """edge -> (fm, fd, bm) of the oracle's directed results, for the distinct live pairs"""
    out = {}
    for a, b in sorted(set(edges)):
        if len(sets[a]) and len(sets[b]):
            fm, fd, bm, bd = directed(oracle, ("graph f32", name, a, b), sets[a], sets[b], False)
            out[(a, b)] = (fm, fd, bm)
    return out


# ---- 1. the scan path: the mixed list --------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", fc.FLAVOURS)
def test_scan_path_on_the_mixed_list(oracle, capi, which):
    """unsorted, both orders, a self edge, empty sides, one row, a duplicate; 2174 right rows: the exact scan.  Both flag
    values at ratios 0.8 and 1.0, against the single calls and the host join of the oracle's directed results"""
    sets = fc.graph_sets_f32(fc.MIXED_SEED, fc.MIXED_LENS, which)
    edges = fc.MIXED_EDGES
    assert sum(fc.MIXED_LENS[b] for a, b in edges if fc.MIXED_LENS[a] and fc.MIXED_LENS[b]) == 2174
    joins = _oracle_joins(oracle, capi, ("mixed", which), sets, edges)
    dev = _Graph(capi, sets)
    try:
        for ratio in (0.8, 1.0):
            for mutual in (False, True):
                per_edge = _equal_singles(dev, edges, ratio, mutual, ("mixed", which), 1)
                for e, (a, b) in enumerate(edges):
                    if (a, b) in joins:
                        fm, fd, bm = joins[(a, b)]
                        want = capi.pairs_join(fm, fd, bm if mutual else None, len(sets[b]), ratio, mutual)
                        assert same_records(per_edge[e], want), (which, e, ratio, mutual, len(per_edge[e]), len(want))
                    else:
                        assert len(per_edge[e]) == 0
                assert same_records(per_edge[1], per_edge[9])                       # the duplicate edge: the same list twice
        got, counts, total = dev.graph(edges, 0.8, True)
        assert dev.info == {"path": 1, "fell_back": 0, "launches": 8, "syncs": 1}
        dev.graph(edges, 0.8, False)
        assert dev.info == {"path": 1, "fell_back": 0, "launches": 6, "syncs": 1}
        assert total > 0 and counts[4] == 0 and counts[7] == 0 and counts[3] > 0
    finally:
        dev.close()


# ---- 2. the prefilter path ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", fc.FLAVOURS)
def test_prefilter_path_on_all_ordered_pairs(oracle, capi, which):
    """2500, 2300 and 700 rows, all six ordered pairs: path 2 without falling back, 9 launches with the cross-check and 7
    without, one synchronisation; against the single calls and the oracle"""
    sets = fc.graph_sets_f32(fc.BIG_SEED, fc.BIG_LENS, which)
    edges = fc.BIG_EDGES
    joins = _oracle_joins(oracle, capi, ("big", which), sets, edges)
    dev = _Graph(capi, sets)
    try:
        for ratio, mutual in ((0.8, True), (0.8, False), (1.0, True), (INF, False)):
            per_edge = _equal_singles(dev, edges, ratio, mutual, ("big", which), 2)
            assert dev.info["launches"] == (9 if mutual else 7)
            for e, (a, b) in enumerate(edges):
                fm, fd, bm = joins[(a, b)]
                want = capi.pairs_join(fm, fd, bm if mutual else None, len(sets[b]), ratio, mutual)
                assert same_records(per_edge[e], want), (which, e, ratio, mutual)
            assert all(len(p) > 0 for p in per_edge)
    finally:
        dev.close()


def test_scan_path_in_a_child_process_gives_the_same_bytes(capi):
    """POPSIFT_MATCH_MFMA=0 in a fresh child process (the switch is read once per thread's scratch): the BIG case takes
    path 1 there and path 2 here, and the SHA-1 of records and counts is the same"""
    env = dict(os.environ, POPSIFT_MATCH_MFMA="0")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "match_graph_f32_worker.py")], stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    child = json.loads(out.stdout.strip().splitlines()[-1])
    assert len(child) == len(fc.FLAVOURS) * len(WORKER_COMBOS)
    for which in fc.FLAVOURS:
        dev = _Graph(capi, fc.graph_sets_f32(fc.BIG_SEED, fc.BIG_LENS, which))
        try:
            for ratio, mutual in WORKER_COMBOS:
                got, counts, total = dev.graph(fc.BIG_EDGES, ratio, mutual)
                path, fell, sha = child["%s/%r/%d" % (which, ratio, mutual)]
                assert (path, fell) == (1, 0) and dev.info["path"] == 2 and dev.info["fell_back"] == 0, (which, dev.info)
                assert total > 0 and sha == digest(got, counts), (which, ratio, mutual)
        finally:
            dev.close()


# ---- 3. the prefilter kernel's edges -----------------------------------------------------------------------------------
@pytest.mark.parametrize("which", fc.FLAVOURS)
def test_prefilter_path_at_the_kernels_edges(capi, which):
    """sets of 1, 31 .. 33, 63 .. 65, 127 .. 129 (the seeding pass), 255 .. 257 (an outer block), 512, 513 and 4097 rows
    (two chunks at any length) as outer and as inner sides of a 3100-row set, which lifts the list over the rule; a self
    edge, a duplicate, both orders of every pair"""
    sets = fc.graph_sets_f32(fc.EDGE_SEED, fc.EDGE_LENS, which)
    edges = fc.EDGE_EDGES
    assert (0, 0) in edges and edges.count((0, 13)) == 2 and all((b, a) in edges for a, b in edges)
    dev = _Graph(capi, sets)
    try:
        for ratio, mutual in ((0.8, True), (INF, False)):
            per_edge = _equal_singles(dev, edges, ratio, mutual, ("edges", which), 2)
            assert all(len(p) > 0 for p in per_edge) if ratio == INF else sum(len(p) > 0 for p in per_edge) > len(edges) // 2
            self_edge = per_edge[edges.index((0, 0))]
            if ratio == INF:
                assert np.array_equal(self_edge["left"], self_edge["right"]) and not self_edge["d1"].any()   # every row finds itself
    finally:
        dev.close()


# ---- 4. nothing leaks across a set boundary ---------------------------------------------------------------------------
def test_no_leak_across_a_set_boundary(capi):
    """The sets are adjacent slices of ONE allocation and every set is followed by a set whose first 31 rows are exact
    copies of rows of set 0: a tile, a staged block or an outer block that ran past its set's last row would meet distance
    0 there.  The results equal those on separate allocations and the single calls'."""
    lens = (300, 33, 255, 256, 257, 40, 3400)
    rng = np.random.default_rng(sum(lens))
    base = [rng.integers(0, 64, (n, 128), dtype=np.uint8) for n in lens]
    for k in range(1, len(lens)):
        base[k][:31] = base[0][40 * (k - 1):40 * (k - 1) + 31]          # exact copies: distance 0 for whoever reads them
        base[k][31 + k] = base[0][250 + k] ^ 1                          # and one near-copy of its own
    edges = [(0, k) for k in range(1, len(lens))] + [(k, 0) for k in range(1, len(lens))] + [(k, k + 1) for k in range(1, len(lens) - 1)]
    for which in fc.FLAVOURS:
        sets = [fc.flavour(s, which) for s in base]
        cat, alone = _Graph(capi, sets, concat=True), _Graph(capi, sets)
        try:
            for ratio, mutual in ((0.8, True), (INF, False)):
                got, counts, total = cat.graph(edges, ratio, mutual)
                assert cat.info["path"] == 2 and cat.info["fell_back"] == 0, cat.info
                sep, scounts, stotal = alone.graph(edges, ratio, mutual)
                assert total == stotal and np.array_equal(counts, scounts) and got.tobytes() == sep.tobytes(), (which, ratio, mutual)
                for e, part in enumerate(slices(got, counts)):
                    a, b = edges[e]
                    want = alone.single(a, b, ratio, mutual)
                    assert same_records(part, want), (which, e, ratio, mutual, len(part), len(want))
                    assert len(part) == 0 or (part["right"].max() < lens[b] and part["left"].max() < lens[a])
                assert all(c >= 31 for c in counts[:6]) or ratio != INF
        finally:
            cat.close(); alone.close()


# ---- 5. ties, the fallback, norms the margin cannot bound ----------------------------------------------------------------
def _tie_sets(run):
    """300 rows in set 0; set 1 of 1100 rows whose rows 500 .. 500 + run - 1 are identical; a 3000-row filler.  Row 7 of
    set 0 EQUALS the run's row (0 / 0: never kept), row 9 is one step away from it"""
    rng = np.random.default_rng(6)
    big = rng.integers(0, 64, (1100, 128), dtype=np.uint8)
    big[500:500 + run] = big[500]
    filler = rng.integers(0, 64, (3000, 128), dtype=np.uint8)
    left = rng.integers(0, 64, (300, 128), dtype=np.uint8)
    left[7] = big[500]
    left[9] = big[500]
    left[9, 3] += 1
    return [left.astype(np.float32), big.astype(np.float32), filler.astype(np.float32)]


@pytest.mark.parametrize("run,fell_back", [(401, 1), (3, 0)], ids=["401-equal-rows", "3-equal-rows"])
def test_ties_and_the_fallback(capi, run, fell_back):
    """401 equal rows in an inner set overflow a candidate segment of 32: the flag comes back up, the scan repeats the call
    (a second synchronisation) and the bytes are still the single calls'; three equal rows fit and nothing falls back; the
    earlier index wins either way"""
    sets = _tie_sets(run)
    edges = [(0, 1), (0, 2), (1, 0)]
    dev = _Graph(capi, sets)
    try:
        for ratio, mutual in ((0.8, True), (0.8, False), (1.0, False), (INF, False)):
            _equal_singles(dev, edges, ratio, mutual, ("ties", run), 2, fell_back=fell_back)
        got = slices(*dev.graph(edges, INF, False)[:2])[0]
        row = got[got["left"] == 9]
        assert len(row) == 1 and row["right"][0] == 500 and row["d1"][0] == row["d2"][0] == 1.0
        assert 7 not in got["left"] and 9 not in slices(*dev.graph(edges, 1.0, False)[:2])[0]["left"]
    finally:
        dev.close()


@pytest.mark.parametrize("what,fell_back", [("nan", 1), ("zero", 0), ("inf", 1)])
def test_norms_the_margin_cannot_bound(capi, what, fell_back):
    """One NaN element / one +inf element in one set: match_scale refuses the norms, the flag is up from the start and the
    scan answers -- a NaN distance never wins, as in the single calls.  An all-zero set of 40 rows is no such case: the
    prefilter answers, every one of its rows ties, and 20 equal candidates per half wave fit a segment."""
    left, rights = planted_many(32, 257, (64, 1000, 300, 2800))
    sets = [left.astype(np.float32)] + [r.astype(np.float32) for r in rights]
    if what == "nan":
        sets[2][17, 5] = np.nan
    elif what == "inf":
        sets[3][3, 100] = np.inf
    else:
        sets.insert(2, np.zeros((40, 128), np.float32))
    edges = [(0, k) for k in range(1, len(sets))] + [(len(sets) - 1, 2)]
    dev = _Graph(capi, sets)
    try:
        for ratio, mutual in ((0.8, True), (0.8, False), (INF, True), (INF, False)):
            _equal_singles(dev, edges, ratio, mutual, what, 2, fell_back=fell_back)
    finally:
        dev.close()


# ---- 6. capacity and counts -----------------------------------------------------------------------------------------------
def test_capacity_and_counts(capi):
    """a cut inside an edge, exactly at an edge boundary, at count - 1 and at 0 with NULL: edge_counts and *count are
    still the totals, the records behind the capacity are untouched -- in a host buffer and in a device buffer with a
    guard band, read back"""
    sets = fc.graph_sets_f32(fc.BIG_SEED, fc.BIG_LENS, "norm512")
    edges = fc.BIG_EDGES
    dev = _Graph(capi, sets)
    L = capi.lib()
    try:
        full, counts, total = dev.graph(edges, 0.8, True)
        assert np.all(counts > 4) and total == counts.sum() == len(full) and dev.info["path"] == 2
        ts = [torch.from_numpy(s.copy()).cuda() for s in dev.sets]
        for cap in (int(counts[0] + counts[1] // 2), int(counts[0]), total - 1, 0, total, total + 3):
            host = np.full(((cap + 2) * 4,), -7, np.int32).view(capi.PAIR_DTYPE)
            c2, n2 = capi._graph_call(L.psx_match_pairs_graph, "psx_match_pairs_graph", 0, dev.ptr, dev.lens, edges,
                                      host.ctypes.data_as(C.c_void_p) if cap else None, cap, 0.8, True)
            k = min(cap, total)
            assert n2 == total and np.array_equal(c2, counts), cap
            assert same_records(host[:k], full[:k]) and np.all(host[k:].view(np.int32) == -7), cap
            want, _, _ = contract(slices(full, counts), cap)
            assert same_records(host[:k], want)
            dbuf = torch.full(((cap + 2) * 16,), 0xA5, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            c3, n3 = capi.match_pairs_graph_dev([t.data_ptr() for t in ts], dev.lens, edges, dbuf.data_ptr() if cap else 0, cap, 0.8, True, u8=False)
            assert capi.match_graph_f32_last()["path"] == 2
            back = dbuf.cpu().numpy()
            assert n3 == total and np.array_equal(c3, counts), cap
            assert same_records(back[:k * 16].view(capi.PAIR_DTYPE), full[:k]) and np.all(back[k * 16:] == 0xA5), cap
        # the python wrapper: per-edge arrays, cut as the call cut them
        lists, c4 = capi.match_pairs_graph(sets, edges, 0.8, True, capacity=int(counts[0]) + 2)
        assert np.array_equal(c4, counts) and [len(p) for p in lists] == [counts[0], 2, 0, 0, 0, 0]
        assert same_records(lists[0], full[:counts[0]]) and same_records(lists[1], full[counts[0]:counts[0] + 2])
    finally:
        dev.close()


# ---- 7. 400 edges over the 200 tiny sets ----------------------------------------------------------------------------------
def test_four_hundred_edges_over_tiny_sets(capi):
    """sets of i % 41 rows in ONE buffer, 400 edges: the exact scan; the launches and synchronisations are those of a
    10-edge list"""
    sets = fc.tiny_sets_f32("norm512")
    assert [len(s) for s in sets] == list(TINY_LENS)
    edges = fc.TINY_EDGES
    dev = _Graph(capi, sets, concat=True)
    try:
        for ratio, mutual in ((0.8, True), (INF, False)):
            per_edge = _equal_singles(dev, edges, ratio, mutual, "tiny400", 1)
            big = dict(dev.info)
            dev.graph(edges[:10], ratio, mutual)
            assert dev.info == big == {"path": 1, "fell_back": 0, "launches": 8 if mutual else 6, "syncs": 1}, (dev.info, big)
            assert ratio != INF or sum(len(p) > 0 for p in per_edge) > 300
    finally:
        dev.close()


# ---- 8. groups ---------------------------------------------------------------------------------------------------------------
def test_groups_of_edges_above_the_budget(capi):
    """duplicate self edges of one 18 432-row set, as many as the plan needs for two forward groups on the prefilter path:
    every edge equals the one single call, and the call still synchronises once"""
    n = fc.GROUP_LEN
    k = 1
    while capi.match_graph_f32_plan((n,), [(0, 0)] * k, True)["fwd_groups"] < 2:
        k += 1
    plan = capi.match_graph_f32_plan((n,), [(0, 0)] * k, True)
    assert k == 12 and plan["path"] == 2 and plan["fwd_groups"] == 2 and plan["bwd_groups"] == 2 and plan["scratch_bytes"] <= 256 << 20
    left, _ = planted_many(77, n, ())
    dev = _Graph(capi, [fc.flavour(left, "norm512")])
    try:
        want = dev.single(0, 0, 0.8, True)
        assert len(want) == n                                                  # every row finds itself, mutually, at distance 0
        got, counts, total = dev.graph([(0, 0)] * k, 0.8, True)
        print("k = %d: %s, %s" % (k, plan, dev.info))
        assert dev.info == {"path": 2, "fell_back": 0, "launches": plan["launches"], "syncs": 1}
        assert total == k * len(want) and np.all(counts == len(want))
        assert got.tobytes() == want.tobytes() * k
    finally:
        dev.close()


# ---- 9. the shared scratch -------------------------------------------------------------------------------------------------
def test_scratch_shared_with_the_other_matchers(capi):
    """on one thread's scratch, in sequence: the float edge list, psx_match_pairs, psx_match_pairs_many (whose buffers this
    call shares), psx_match_pairs_graph_u8, the float edge list again (identical bytes), psx_match_release, and again"""
    sets = fc.graph_sets_f32(fc.BIG_SEED, fc.BIG_LENS, "int")
    u8 = graph_sets(fc.BIG_SEED, fc.BIG_LENS)
    edges = fc.BIG_EDGES
    dev = _Graph(capi, sets)
    try:
        first, counts, total = dev.graph(edges, 0.8, True)
        assert total > 50 and dev.info["path"] == 2
        one = dev.single(0, 1, 0.8, True)
        assert same_records(one, slices(first, counts)[0])
        star, sc = capi.match_pairs_many(sets[0], sets[1:], 0.8, True)
        assert capi.match_many_f32_last()["path"] == 1                        # 3000 right rows: the star takes the scan
        assert same_records(star[0], slices(first, counts)[0]) and same_records(star[1], slices(first, counts)[1])
        lists_u8, counts_u8 = capi.match_pairs_graph_u8(u8, edges, 0.8, True)
        # integer-valued floats: the byte call finds the same pairs
        assert np.array_equal(counts_u8, counts) and all(np.array_equal(a["right"], b["right"]) for a, b in zip(lists_u8, slices(first, counts)))
        again, c2, t2 = dev.graph(edges, 0.8, True)
        assert t2 == total and np.array_equal(c2, counts) and again.tobytes() == first.tobytes()
        small, c5, t5 = dev.graph(edges[:1], 0.8, True)                        # within the capacity the big list left: the scan
        assert dev.info["path"] == 1 and same_records(small, one)
        assert capi.lib().psx_match_release() == 0
        third, c3, t3 = dev.graph(edges, 0.8, True)
        assert t3 == total and np.array_equal(c3, counts) and third.tobytes() == first.tobytes()
    finally:
        dev.close()


# ---- 12. C++ -----------------------------------------------------------------------------------------------------------------
def test_cpp_match_pairs_graph_float_on_the_gpu(tmp_path):
    """tests/cpp/test_match_graph_f32_api.cpp with POPSIFT_TEST_EXPECT_GPU: FeaturesDev::matchPairsGraphFloat,
    matchPairsGuidedManyFloat and matchPairsGuidedGraphFloat equal matchPairs / matchPairsGuided per element, field by
    field; the throws happen."""
    libdir = os.path.join(ROOT, "popsift_amd", "lib")
    exe = str(tmp_path / "test_match_graph_f32_api")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-pthread", os.path.join(ROOT, "tests", "cpp", "test_match_graph_f32_api.cpp"), "-o", exe,
                           "-I", os.path.join(ROOT, "popsift_amd", "csrc", "include"), "-I", os.path.join(ROOT, "include"),
                           "-L", libdir, "-lpopsift", "-lpopsift_hip", "-Wl,-rpath," + libdir])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300,
                         env=dict(os.environ, POPSIFT_TEST_EXPECT_GPU="1"))
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout
    assert "matchPairsGraphFloat:" in out.stdout and "matchPairsGuidedManyFloat:" in out.stdout and "matchPairsGuidedGraphFloat:" in out.stdout
