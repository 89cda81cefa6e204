"""GPU tests of the one-to-many byte pair search (include/popsift_hip.h, "one descriptor set against many"):
psx_match_pairs_many_u8, its _dev form and FeaturesDev::matchPairsMany.  The contract is "the concatenation of what
psx_match_pairs_u8 returns per set": every slice is compared, as bytes, with that call on the same device arrays in the
same process, and for two of the cases also with the HOST join (capi.pairs_join) of the oracle's directed results, so the
check does not rest on the device code alone."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch        # before the HIP library is loaded: torch brings a HIP runtime of its own and must initialise first (_dev form)

from tests.match_many_cases import CASES, CASE_IDS, TINY_LENS, contract, planted_many, slices, tiny_many
from tests.match_pairs_cases import RATIOS, assert_premise, directed, planted, same_records

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Sets:
    """a left set and K right sets uploaded once -- as separate allocations, or as slices of ONE buffer (concat) --;
    the one-to-many call and the single call on the same device arrays"""

    def __init__(self, capi, left, rights, concat=False):
        self.capi, self.L, self.bufs = capi, capi.lib(), []
        self.left = np.ascontiguousarray(left, np.uint8).reshape(-1, 128)
        self.rights = [np.ascontiguousarray(r, np.uint8).reshape(-1, 128) for r in rights]
        self.lens = [len(r) for r in self.rights]
        if concat:
            whole = np.concatenate(self.rights) if self.rights else np.zeros((0, 128), np.uint8)
            self.pl, base = capi._to_device(self.L, 0, [self.left, whole], self.bufs)
            offs = np.concatenate([[0], np.cumsum(self.lens)]).astype(np.int64) * 128
            self.pr = [C.c_void_p((base.value or 0) + int(o)) if n else C.c_void_p() for o, n in zip(offs, self.lens)]
        else:
            ptrs = capi._to_device(self.L, 0, [self.left] + self.rights, self.bufs)
            self.pl, self.pr = ptrs[0], ptrs[1:]

    def many(self, ratio, mutual, capacity=None, order=None):
        """(records, per-set counts, total); order: which sets, in which order (default: all)"""
        order = range(len(self.rights)) if order is None else order
        ptrs, lens = [self.pr[k] for k in order], [self.lens[k] for k in order]
        cap = len(self.left) * len(lens) if capacity is None else capacity
        out = np.zeros((cap,), self.capi.PAIR_U8_DTYPE)
        counts, n = self.capi._many_call(self.L.psx_match_pairs_many_u8, "psx_match_pairs_many_u8", 0, self.pl, len(self.left), ptrs, lens,
                                         out.ctypes.data_as(C.c_void_p) if cap else None, cap, ratio, mutual)
        return out[:min(n, cap)], counts, n

    def single(self, k, ratio, mutual):
        return self.capi._pairs_call(self.L.psx_match_pairs_u8, "psx_match_pairs_u8", 0, self.pl, len(self.left), self.pr[k], self.lens[k],
                                     ratio, mutual, self.capi.PAIR_U8_DTYPE, None)[0]

    def close(self):
        for p in self.bufs:
            self.L.psx_dev_free(0, p)
        self.bufs = []


def _equal_singles(dev, ratio, mutual, what):
    """one call against the loop of single calls: every slice, the counts, the total; returns the per-set lists"""
    got, counts, total = dev.many(ratio, mutual)
    per_set = [dev.single(k, ratio, mutual) for k in range(len(dev.rights))]
    want, wcounts, wtotal = contract(per_set)
    assert total == wtotal and np.array_equal(counts, wcounts), (what, ratio, mutual, list(counts), list(wcounts))
    for k, (a, b) in enumerate(zip(slices(got, counts), per_set)):
        assert same_records(a, b), (what, ratio, mutual, k, len(a), len(b))
    assert got.tobytes() == want.tobytes()
    return per_set


# ---- 1. the four cases ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,nl,lens", CASES, ids=CASE_IDS)
def test_many_equals_the_single_calls(oracle, capi, seed, nl, lens):
    """every ratio and both flag values: each slice equals psx_match_pairs_u8(L, R_k), the counts are equal; seeds 21 and 23
    also against the host join of the oracle's directed results.  The generator's premise (a pair kept, one dropped by the
    ratio, one dropped by the cross-check alone) is asserted for every set with min(nl, nr) >= 64."""
    left, rights = planted_many(seed, nl, lens)
    dev = _Sets(capi, left, rights)
    try:
        joins = {}
        for k, r in enumerate(rights):
            if seed in (21, 23):
                fm, fd, bm, bd = directed(oracle, ("many", seed, k), left, r, True)
                joins[k] = (fm, fd, bm)
            elif min(nl, len(r)) >= 64:
                (fm, fd), (bm, bd) = capi.match_u8(left, r), capi.match_u8(r, left)
            if min(nl, len(r)) >= 64:
                assert_premise(fm, fd, bm, len(r), (seed, k))
        for ratio in RATIOS:
            for mutual in (False, True):
                per_set = _equal_singles(dev, ratio, mutual, seed)
                for k, (fm, fd, bm) in joins.items():
                    want = capi.pairs_join(fm, fd, bm if mutual else None, len(rights[k]), ratio, mutual)
                    assert same_records(per_set[k], want), (seed, k, ratio, mutual, len(per_set[k]), len(want))
        got, counts, total = dev.many(0.8, True)
        print("seed %d: %d x %s -> %s pairs" % (seed, nl, list(lens), list(counts)))
        assert all(c == 0 for c, n in zip(counts, lens) if n == 0)
    finally:
        dev.close()


# ---- 2. one set ------------------------------------------------------------------------------------------------------------
def test_one_set_equals_the_single_call(capi):
    left, rights = planted_many(22, 257, (1000,))
    dev = _Sets(capi, left, rights)
    try:
        for ratio, mutual in ((0.8, False), (0.8, True), (float("inf"), True)):
            got, counts, total = dev.many(ratio, mutual)
            want = dev.single(0, ratio, mutual)
            assert total == len(want) > 0 and list(counts) == [total] and same_records(got, want), (ratio, mutual)
    finally:
        dev.close()


# ---- 3. / 5. where the sets lie ------------------------------------------------------------------------------------------
def test_separate_allocations_and_slices_of_one_buffer(capi):
    """the same sets as separate allocations and as slices of one concatenated buffer: identical bytes"""
    seed, nl, lens = CASES[0]
    left, rights = planted_many(seed, nl, lens)
    a, b = _Sets(capi, left, rights), _Sets(capi, left, rights, concat=True)
    try:
        for ratio, mutual in ((0.8, True), (0.8, False), (float("inf"), True)):
            ra, ca, na = a.many(ratio, mutual)
            rb, cb, nb = b.many(ratio, mutual)
            assert na == nb > 0 and np.array_equal(ca, cb) and ra.tobytes() == rb.tobytes(), (ratio, mutual)
    finally:
        a.close(); b.close()


def test_the_same_pointer_twice(capi):
    """a set given twice (and a third time behind another set) yields the same list each time"""
    left, rights = planted_many(22, 257, (300, 64))
    dev = _Sets(capi, left, rights)
    try:
        for ratio, mutual in ((0.8, True), (float("inf"), False)):
            got, counts, total = dev.many(ratio, mutual, order=(0, 0, 1, 0))
            parts = slices(got, counts)
            one = dev.single(0, ratio, mutual)
            assert len(one) > 0 and counts[0] == counts[1] == counts[3] == len(one)
            assert same_records(parts[0], one) and same_records(parts[1], one) and same_records(parts[3], one)
            assert same_records(parts[2], dev.single(1, ratio, mutual))
    finally:
        dev.close()


# ---- 4. nothing leaks across a set boundary ---------------------------------------------------------------------------
@pytest.mark.parametrize("lens", [(33, 40), (255, 256, 257, 40)], ids=["33", "255-256-257"])
def test_no_leak_across_a_set_boundary(capi, lens):
    """In ONE buffer every set is followed by a set whose first 31 rows are exact copies of left rows: a tile, or an outer
    block, that ran past its set's last row would meet distance 0 there.  33 rows: the forward direction's last tile holds
    one row of the set and 31 of the next; 255 / 256 / 257: a backward outer block ends inside a tile, at a tile, one past.
    Every set's result must equal its stand-alone result (its own allocation, the single call)."""
    rng = np.random.default_rng(sum(lens))
    left = rng.integers(0, 64, (300, 128), dtype=np.uint8)
    rights = []
    for k, n in enumerate(lens):
        r = rng.integers(0, 64, (n, 128), dtype=np.uint8)
        r[:31] = left[40 * k:40 * k + 31]                   # exact copies: distance 0 for whoever reads them
        r[31 + k] = left[200 + k] ^ 1                       # and one near-copy of its own, so that no list is trivial
        rights.append(r)
    cat, alone = _Sets(capi, left, rights, concat=True), _Sets(capi, left, rights)
    try:
        for ratio, mutual in ((0.8, False), (0.8, True), (float("inf"), True), (float("inf"), False)):
            got, counts, total = cat.many(ratio, mutual)
            for k, part in enumerate(slices(got, counts)):
                want = alone.single(k, ratio, mutual)
                assert len(want) >= 31 and same_records(part, want), (lens, k, ratio, mutual, len(part), len(want))
                assert part["right"].max() < lens[k]
    finally:
        cat.close(); alone.close()


# ---- 6. ties ------------------------------------------------------------------------------------------------------------
def test_ties_keep_the_earlier_index(oracle, capi):
    """1100 rows with rows 500 .. 900 identical -- 13 chunks of 32 at 40 left rows, so the run crosses chunk boundaries --:
    a left row one step away from them gets best = 500 and, since the second-best is 501 at the same distance, d2 == d1 (a
    quotient of exactly 1: kept by ratio inf alone); a left row EQUAL to them has 0 / 0 and is never kept.  Also all-0 against
    all-255.  The directed results are the oracle's."""
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
    dev = _Sets(capi, left, [big, full])
    try:
        for ratio in RATIOS:
            for mutual in (False, True):
                per_set = _equal_singles(dev, ratio, mutual, "ties")
                assert same_records(per_set[0], capi.pairs_join(fm, fd, bm if mutual else None, 1100, ratio, mutual)), (ratio, mutual)
        got = slices(*dev.many(float("inf"), False)[:2])[0]
        row = got[got["left"] == 9]
        assert len(row) == 1 and row["right"][0] == 500 and row["d1"][0] == row["d2"][0] == 1
        assert 7 not in got["left"] and 9 not in slices(*dev.many(1.0, False)[:2])[0]["left"]
    finally:
        dev.close()
    dev = _Sets(capi, zeros, [full, full[:1]])
    try:
        # two rows: d1 == d2, a quotient of exactly 1; one row: no second neighbour, a quotient of 0
        assert list(dev.many(1.0, False)[1]) == [0, 3]
        got, counts, total = dev.many(float("inf"), False)
        assert list(counts) == [3, 3] and list(got["left"]) == [0, 1, 2, 0, 1, 2] and np.all(got["right"] == 0)
        assert np.all(got["d1"] == 128 * 255 * 255) and np.all(got["d2"][:3] == 128 * 255 * 255) and np.all(got["d2"][3:] == 2 ** 31 - 1)
        got, counts, total = dev.many(float("inf"), True)
        assert list(counts) == [1, 1] and list(got["left"]) == [0, 0] and list(got["right"]) == [0, 0]
    finally:
        dev.close()


# ---- 7. capacity -----------------------------------------------------------------------------------------------------------
def test_capacity_and_counts(capi):
    """truncation in the middle of a set, exactly at a set boundary, at count - 1 and at 0 with NULL: the totals are still
    reported, the record behind the capacity is untouched -- in a host buffer and in a device buffer read back"""
    seed, nl, lens = CASES[1]
    left, rights = planted_many(seed, nl, lens)
    dev = _Sets(capi, left, rights)
    L = capi.lib()
    try:
        full, counts, total = dev.many(0.8, True)
        assert np.all(counts > 4) and total == counts.sum() == len(full)
        tl = torch.from_numpy(dev.left).cuda()
        tr = [torch.from_numpy(r).cuda() for r in dev.rights]
        for cap in (int(counts[0] + counts[1] // 2), int(counts[0]), total - 1, 0, total, total + 3):
            host = np.full(((cap + 2) * 4,), -7, np.int32).view(capi.PAIR_U8_DTYPE)
            c2, n2 = capi._many_call(L.psx_match_pairs_many_u8, "psx_match_pairs_many_u8", 0, dev.pl, nl, dev.pr, dev.lens,
                                     host.ctypes.data_as(C.c_void_p) if cap else None, cap, 0.8, True)
            k = min(cap, total)
            assert n2 == total and np.array_equal(c2, counts), cap
            assert same_records(host[:k], full[:k]) and np.all(host[k:].view(np.int32) == -7), cap
            want, _, _ = contract(slices(full, counts), cap)
            assert same_records(host[:k], want)
            dbuf = torch.full(((cap + 2) * 16,), 0xA5, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            c3, n3 = capi.match_pairs_many_dev(tl.data_ptr(), nl, [t.data_ptr() for t in tr], dev.lens, dbuf.data_ptr() if cap else 0, cap, 0.8, True)
            back = dbuf.cpu().numpy()
            assert n3 == total and np.array_equal(c3, counts), cap
            assert same_records(back[:k * 16].view(capi.PAIR_U8_DTYPE), full[:k]) and np.all(back[k * 16:] == 0xA5), cap
        # the python wrapper: per-set arrays, cut as the call cut them
        lists, c4 = capi.match_pairs_many_u8(left, rights, 0.8, True, capacity=int(counts[0]) + 2)
        assert np.array_equal(c4, counts) and [len(p) for p in lists] == [counts[0], 2, 0]
        assert same_records(lists[0], full[:counts[0]]) and same_records(lists[1], full[counts[0]:counts[0] + 2])
    finally:
        dev.close()


# ---- 8. many tiny sets -------------------------------------------------------------------------------------------------------
def test_two_hundred_tiny_sets(capi):
    """K = 200 sets of i % 41 rows against 70 left rows: 200 workgroup totals in the scan, empty sets in between, sets
    shorter than a tile; every non-empty set holds an exact copy of a left row, so every one of them yields a pair"""
    left, rights = tiny_many()
    dev = _Sets(capi, left, rights, concat=True)
    try:
        for ratio, mutual in ((0.8, True), (float("inf"), True), (float("inf"), False)):
            _equal_singles(dev, ratio, mutual, "tiny")
        got, counts, total = dev.many(0.8, True)
        assert all((c > 0) == (n > 0) for c, n in zip(counts, TINY_LENS)) and (counts > 0).sum() == 195
        for k, part in enumerate(slices(got, counts)):
            if TINY_LENS[k] > 0:
                assert (k % 70, k % TINY_LENS[k]) in set(zip(part["left"].tolist(), part["right"].tolist())), k
    finally:
        dev.close()


# ---- the partials' budget ----------------------------------------------------------------------------------------------------
def test_groups_of_sets_above_the_partials_budget(capi):
    """18 432 rows against the same 18 432-row set 64 times: 2304 chunks x 18 432 left rows of partials forward (340 MB) and
    36 chunks x 1.18 M right rows backward, both above the 256 MiB budget of match_many.hip, so both directions run in two
    groups of sets on the stream.  Every slice equals the single call."""
    left, right = planted(18432, 18432, 18432)
    dev = _Sets(capi, left, [right])
    try:
        want = dev.single(0, 0.8, True)
        assert len(want) > 1000
        got, counts, total = dev.many(0.8, True, order=(0,) * 64)
        assert total == 64 * len(want) and np.all(counts == len(want))
        assert got.tobytes() == want.tobytes() * 64
    finally:
        dev.close()


# ---- 9. the shared scratch -------------------------------------------------------------------------------------------------
def test_scratch_shared_with_the_other_matchers(capi):
    """on one thread's scratch, in sequence: one-to-many, psx_match_pairs_u8, psx_ransac_homography on a slice's pairs,
    one-to-many again (identical bytes), psx_match_release, one-to-many again"""
    seed, nl, lens = CASES[1]
    left, rights = planted_many(seed, nl, lens)
    dev = _Sets(capi, left, rights)
    try:
        first, counts, total = dev.many(0.8, True)
        assert total > 50
        one = dev.single(1, 0.8, True)
        assert same_records(one, slices(first, counts)[1])
        rng = np.random.default_rng(9)
        lxy, rxy = rng.random((nl, 2), dtype=np.float32) * 640, rng.random((lens[1], 2), dtype=np.float32) * 640
        res = capi.ransac_homography(one, lxy, rxy)
        assert res["count"] >= 0
        again, c2, t2 = dev.many(0.8, True)
        assert t2 == total and np.array_equal(c2, counts) and again.tobytes() == first.tobytes()
        assert capi.lib().psx_match_release() == 0
        third, c3, t3 = dev.many(0.8, True)
        assert t3 == total and np.array_equal(c3, counts) and third.tobytes() == first.tobytes()
        assert same_records(dev.single(1, 0.8, True), one)
    finally:
        dev.close()


# ---- 10. C++ -----------------------------------------------------------------------------------------------------------------
def test_cpp_match_pairs_many_on_the_gpu(tmp_path):
    """tests/cpp/test_match_many_api.cpp with POPSIFT_TEST_EXPECT_GPU: FeaturesDev::matchPairsMany equals the loop of
    matchPairs with MatchOptions::bytes, field by field, with and without the cross-check; the throws happen."""
    libdir = os.path.join(ROOT, "popsift_amd", "lib")
    exe = str(tmp_path / "test_match_many_api")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-pthread", os.path.join(ROOT, "tests", "cpp", "test_match_many_api.cpp"), "-o", exe,
                           "-I", os.path.join(ROOT, "popsift_amd", "csrc", "include"), "-I", os.path.join(ROOT, "include"),
                           "-L", libdir, "-lpopsift", "-lpopsift_hip", "-Wl,-rpath," + libdir])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300,
                         env=dict(os.environ, POPSIFT_TEST_EXPECT_GPU="1"))
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout
    assert "mutual 0:" in out.stdout and "mutual 1:" in out.stdout
