"""GPU tests of the guided re-match of many sets (include/popsift_hip.h, "guided re-match of many sets in one call"):
psx_match_pairs_guided_many_u8, its _dev form, psx_guides_from_ransac in the three-call chain and
FeaturesDev::matchPairsGuidedMany.  The contract is "the concatenation of what psx_match_pairs_guided_u8 returns per set
under that set's own guide": every slice is compared, as bytes, with that call on the same device arrays in the same
process, and in the four cases also with the generator's host expectation (tests/guided_many_cases.py: a numpy
restatement of the rule, int64 distances and the host join), so the check does not rest on the device code alone."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch        # before the HIP library is loaded: torch brings a HIP runtime of its own and must initialise first (_dev form)

from tests.guided_cases import F_EPI, H_ASYM, IDENTITY, _apply_h
from tests.guided_many_cases import (ALL_TOL, CASES, CASE_IDS, NONE, capi_guide, expected, guide_of, positioned_many,
                                     tiny_guided, translated)
from tests.match_many_cases import TINY_LENS, contract, planted_many, slices
from tests.match_pairs_cases import RATIOS, same_records

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Sets:
    """a left set and K right sets with their positions, uploaded once -- as separate allocations, or descriptors AND
    positions as slices of ONE buffer each (concat) --; the one call and the single call on the same device arrays"""

    def __init__(self, capi, left, lxy, rights, rxys, concat=False):
        self.capi, self.L, self.bufs = capi, capi.lib(), []
        self.left = np.ascontiguousarray(left, np.uint8).reshape(-1, 128)
        self.lxy = np.ascontiguousarray(lxy, np.float32).reshape(-1, 2)
        self.rights = [np.ascontiguousarray(r, np.uint8).reshape(-1, 128) for r in rights]
        self.rxys = [np.ascontiguousarray(x, np.float32).reshape(-1, 2) for x in rxys]
        self.lens = [len(r) for r in self.rights]
        assert self.lens == [len(x) for x in self.rxys] and len(self.left) == len(self.lxy)
        if concat:
            whole = np.concatenate(self.rights) if self.rights else np.zeros((0, 128), np.uint8)
            whole_xy = np.concatenate(self.rxys) if self.rxys else np.zeros((0, 2), np.float32)
            self.pl, self.plx, base, base_xy = capi._to_device(self.L, 0, [self.left, self.lxy, whole, whole_xy], self.bufs)
            offs = np.concatenate([[0], np.cumsum(self.lens)]).astype(np.int64)
            self.pr = [C.c_void_p((base.value or 0) + int(o) * 128) if n else C.c_void_p() for o, n in zip(offs, self.lens)]
            self.prx = [C.c_void_p((base_xy.value or 0) + int(o) * 8) if n else C.c_void_p() for o, n in zip(offs, self.lens)]
        else:
            ptrs = capi._to_device(self.L, 0, [self.left, self.lxy] + self.rights + self.rxys, self.bufs)
            k = len(self.rights)
            self.pl, self.plx, self.pr, self.prx = ptrs[0], ptrs[1], ptrs[2:2 + k], ptrs[2 + k:]

    def many(self, guides, ratio, mutual, capacity=None, order=None, null_skipped=False):
        """(records, per-set counts, total); order: which sets, in which order (default: all); guides: one per entry of
        order; null_skipped: the pointers of the sets whose guide is of kind 0 are passed as NULL"""
        order = list(range(len(self.rights)) if order is None else order)
        skip = [null_skipped and g.kind == 0 for g in guides]
        ptrs = [C.c_void_p() if s else self.pr[k] for k, s in zip(order, skip)]
        xptrs = [C.c_void_p() if s else self.prx[k] for k, s in zip(order, skip)]
        lens = [self.lens[k] for k in order]
        cap = len(self.left) * len(lens) if capacity is None else capacity
        out = np.zeros((cap,), self.capi.PAIR_U8_DTYPE)
        counts, n = self.capi._guided_many_call(self.L.psx_match_pairs_guided_many_u8, "psx_match_pairs_guided_many_u8", 0, self.pl, self.plx,
                                                len(self.left), ptrs, xptrs, lens, guides, out.ctypes.data_as(C.c_void_p) if cap else None,
                                                cap, ratio, mutual)
        return out[:min(n, cap)], counts, n

    def single(self, k, guide, ratio, mutual):
        fn = self.capi._guided_fn(self.L.psx_match_pairs_guided_u8, self.plx, self.prx[k], guide)
        return self.capi._pairs_call(fn, "psx_match_pairs_guided_u8", 0, self.pl, len(self.left), self.pr[k], self.lens[k], ratio, mutual,
                                     self.capi.PAIR_U8_DTYPE, None)[0]

    def unguided(self, k, ratio, mutual):
        return self.capi._pairs_call(self.L.psx_match_pairs_u8, "psx_match_pairs_u8", 0, self.pl, len(self.left), self.pr[k], self.lens[k],
                                     ratio, mutual, self.capi.PAIR_U8_DTYPE, None)[0]

    def close(self):
        for p in self.bufs:
            self.L.psx_dev_free(0, p)
        self.bufs = []


def _equal_singles(dev, guides, ratio, mutual, what, order=None, null_skipped=True):
    """one call against the loop of single calls: every slice, the counts, the total; returns the per-set lists"""
    order = list(range(len(dev.rights)) if order is None else order)
    got, counts, total = dev.many(guides, ratio, mutual, order=order, null_skipped=null_skipped)
    per_set = [np.zeros(0, dev.capi.PAIR_U8_DTYPE) if g.kind == 0 else dev.single(k, g, ratio, mutual) for k, g in zip(order, guides)]
    want, wcounts, wtotal = contract(per_set)
    assert total == wtotal and np.array_equal(counts, wcounts), (what, ratio, mutual, list(counts), list(wcounts))
    for k, (a, b) in enumerate(zip(slices(got, counts), per_set)):
        assert same_records(a, b), (what, ratio, mutual, k, len(a), len(b))
    assert got.tobytes() == want.tobytes()
    return per_set


# ---- 1. the four cases ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_many_equals_the_single_calls_and_the_host_expectation(capi, case):
    """every ratio and both flag values, every set under its own guide (homography, epipolar, all-admitting, none in turn):
    each slice equals psx_match_pairs_guided_u8(L, R_k, guide k), the counts are equal, and every slice equals the
    generator's host expectation"""
    seed, nl, lens = case
    left, rights, lxy, rxys = positioned_many(*case)
    guides = [capi_guide(capi, guide_of(k)) for k in range(len(lens))]
    dev = _Sets(capi, left, lxy, rights, rxys)
    try:
        for ratio in RATIOS:
            for mutual in (False, True):
                per_set = _equal_singles(dev, guides, ratio, mutual, seed)
                for k in range(len(lens)):
                    want = expected(capi, case, k, ratio, mutual)
                    assert same_records(per_set[k], want), (seed, k, ratio, mutual, len(per_set[k]), len(want))
        got, counts, total = dev.many(guides, 0.8, True)
        print("seed %d: %d x %s -> %s pairs" % (seed, nl, list(lens), list(counts)))
        assert all(c == 0 for k, (c, n) in enumerate(zip(counts, lens)) if n == 0 or guide_of(k)[0] == NONE)
        if seed in (31, 32):
            assert all(c > 0 for k, (c, n) in enumerate(zip(counts, lens)) if n >= 63 and guide_of(k)[0] != NONE)
    finally:
        dev.close()


# ---- 2. mixed guides in one call -------------------------------------------------------------------------------------------
def test_mixed_guides_in_one_call(capi):
    """homography, epipolar, all-admitting and NONE side by side on seed 32's sets (the long one four times): the
    all-admitting slice equals the UNGUIDED psx_match_pairs_u8 on that set, the NONE slice is empty although its pointers
    are NULL, the others equal their single calls and differ from one another"""
    case = CASES[1]
    left, rights, lxy, rxys = positioned_many(*case)
    dev = _Sets(capi, left, lxy, rights, rxys)
    order = (1, 1, 1, 1, 0, 2)
    guides = [capi.Guide.homography(H_ASYM, 2.0), capi.Guide.epipolar(F_EPI, 2.0), capi.Guide.homography(IDENTITY, ALL_TOL), capi.Guide.none(),
              capi.Guide.none(), capi.Guide.homography(IDENTITY, ALL_TOL)]
    try:
        for ratio, mutual in ((0.8, True), (0.8, False), (float("inf"), True)):
            per_set = _equal_singles(dev, guides, ratio, mutual, "mixed", order=order)
            assert same_records(per_set[2], dev.unguided(1, ratio, mutual)) and len(per_set[2]) > 10
            assert same_records(per_set[5], dev.unguided(2, ratio, mutual)) and len(per_set[5]) > 10
            assert len(per_set[3]) == 0 and len(per_set[4]) == 0
            assert len(per_set[0]) > 0 and len(per_set[1]) > 0
            assert len({p.tobytes() for p in per_set[:3]}) == 3
    finally:
        dev.close()


# ---- 3. nothing leaks across a set boundary ---------------------------------------------------------------------------
@pytest.mark.parametrize("lens", [(63, 64, 65, 129, 40), (255, 256, 257, 40)], ids=["63-64-65-129", "255-256-257"])
def test_no_leak_across_a_set_boundary(capi, lens):
    """Descriptors AND positions of all sets are slices of one buffer each, and every set is followed by a set whose first
    31 rows are exact copies of left rows AT ADMISSIBLE POSITIONS (every guide is a window around the same shift, so the
    copies are admissible under the previous set's guide too): a ballot step, or a backward block, that ran past its set's
    last row would meet distance 0 there.
    63 / 64 / 65 / 129: the 64-wide step ends one before, at, one past the set's end; 255 / 256 / 257: a backward block.
    Every slice must equal its stand-alone result (its own allocation, the single call); `right` stays within the set."""
    rng = np.random.default_rng(sum(lens))
    left = rng.integers(0, 64, (300, 128), dtype=np.uint8)
    lxy = rng.uniform(0.0, 40.0, (300, 2)).astype(np.float32)
    # one shift for all sets, so that a row of the NEXT set is admissible for the wave that wrongly reads it; the guides still
    # differ per set (their tolerances), and the table index is probed by the cases of test 1
    shift = translated(IDENTITY, 1.5, -0.5)
    guides = [capi.Guide.homography(shift, 1.0 + 0.25 * k) for k in range(len(lens))]
    rights, rxys = [], []
    for k, n in enumerate(lens):
        r = rng.integers(0, 64, (n, 128), dtype=np.uint8)
        x = rng.uniform(0.0, 40.0, (n, 2))
        rows = np.arange(40 * k, 40 * k + 31) % 300
        r[:31] = left[rows]                                  # exact copies: distance 0 for whoever reads them
        x[:31] = _apply_h(shift, lxy[rows].astype(np.float64)) + 0.25
        r[31 + k] = left[200 + k] ^ 1                        # and one near-copy of its own, so that no list is trivial
        x[31 + k] = _apply_h(shift, lxy[200 + k][None].astype(np.float64))[0]
        rights.append(r)
        rxys.append(x.astype(np.float32))
    cat, alone = _Sets(capi, left, lxy, rights, rxys, concat=True), _Sets(capi, left, lxy, rights, rxys)
    try:
        for ratio, mutual in ((0.8, False), (0.8, True), (float("inf"), True), (float("inf"), False)):
            got, counts, total = cat.many(guides, ratio, mutual)
            for k, part in enumerate(slices(got, counts)):
                want = alone.single(k, guides[k], ratio, mutual)
                assert len(want) >= 31 and same_records(part, want), (lens, k, ratio, mutual, len(part), len(want))
                assert part["right"].max() < lens[k]
    finally:
        cat.close(); alone.close()


# ---- 4. the same pointer twice under two guides ---------------------------------------------------------------------------
def test_the_same_pointer_twice_under_two_guides(capi):
    case = CASES[1]
    left, rights, lxy, rxys = positioned_many(*case)
    dev = _Sets(capi, left, lxy, rights, rxys)
    ga, gb = capi.Guide.homography(H_ASYM, 2.0), capi.Guide.epipolar(F_EPI, 2.0)
    gc = capi.Guide.homography(H_ASYM, 0.75)
    try:
        for ratio, mutual in ((0.8, True), (float("inf"), False)):
            per_set = _equal_singles(dev, [ga, gb, ga, gc, gb], ratio, mutual, "twice", order=(1, 1, 2, 1, 0))
            assert len(per_set[0]) > 0 and len(per_set[1]) > 0 and len(per_set[3]) > 0
            assert len({per_set[0].tobytes(), per_set[1].tobytes(), per_set[3].tobytes()}) == 3
    finally:
        dev.close()


# ---- 5. capacity -----------------------------------------------------------------------------------------------------------
def test_capacity_and_counts(capi):
    """truncation in the middle of a set, exactly at a set boundary, at count - 1, at 0 with NULL and at count + 3: the
    totals are still reported, the bytes behind the capacity are untouched -- in a host buffer and in a device buffer read
    back"""
    case = CASES[1]
    seed, nl, lens = case
    left, rights, lxy, rxys = positioned_many(*case)
    guides = [capi.Guide.homography(H_ASYM, 2.0), capi.Guide.epipolar(F_EPI, 2.0), capi.Guide.homography(IDENTITY, ALL_TOL)]
    dev = _Sets(capi, left, lxy, rights, rxys)
    L = capi.lib()
    try:
        full, counts, total = dev.many(guides, 0.8, True)
        assert np.all(counts > 4) and total == counts.sum() == len(full)
        tl, tlx = torch.from_numpy(dev.left.copy()).cuda(), torch.from_numpy(dev.lxy.copy()).cuda()      # the generator's arrays are read-only
        tr = [torch.from_numpy(r.copy()).cuda() for r in dev.rights]
        trx = [torch.from_numpy(x.copy()).cuda() for x in dev.rxys]
        for cap in (int(counts[0] + counts[1] // 2), int(counts[0]), total - 1, 0, total, total + 3):
            host = np.full(((cap + 2) * 4,), -7, np.int32).view(capi.PAIR_U8_DTYPE)
            c2, n2 = capi._guided_many_call(L.psx_match_pairs_guided_many_u8, "psx_match_pairs_guided_many_u8", 0, dev.pl, dev.plx, nl, dev.pr,
                                            dev.prx, dev.lens, guides, host.ctypes.data_as(C.c_void_p) if cap else None, cap, 0.8, True)
            k = min(cap, total)
            assert n2 == total and np.array_equal(c2, counts), cap
            assert same_records(host[:k], full[:k]) and np.all(host[k:].view(np.int32) == -7), cap
            want, _, _ = contract(slices(full, counts), cap)
            assert same_records(host[:k], want)
            dbuf = torch.full(((cap + 2) * 16,), 0xA5, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            c3, n3 = capi.match_pairs_guided_many_dev(tl.data_ptr(), tlx.data_ptr(), nl, [t.data_ptr() for t in tr], [t.data_ptr() for t in trx],
                                                      dev.lens, guides, dbuf.data_ptr() if cap else 0, cap, 0.8, True)
            back = dbuf.cpu().numpy()
            assert n3 == total and np.array_equal(c3, counts), cap
            assert same_records(back[:k * 16].view(capi.PAIR_U8_DTYPE), full[:k]) and np.all(back[k * 16:] == 0xA5), cap
        # the python wrapper: per-set arrays, cut as the call cut them
        lists, c4 = capi.match_pairs_guided_many_u8(left, lxy, rights, rxys, guides, 0.8, True, capacity=int(counts[0]) + 2)
        assert np.array_equal(c4, counts) and [len(p) for p in lists] == [counts[0], 2, 0]
        assert same_records(lists[0], full[:counts[0]]) and same_records(lists[1], full[counts[0]:counts[0] + 2])
    finally:
        dev.close()


# ---- 6. two hundred tiny sets ----------------------------------------------------------------------------------------------
def test_two_hundred_tiny_sets(capi):
    """K = 200 sets of i % 41 rows against 70 left rows, every fifth set of kind 0 (its pointers NULL), each other one under a
    guide of its own: 200 workgroup totals in the scan, empty and skipped sets in between; equals the single calls, and
    every set that is neither empty nor skipped yields the pair planted in it"""
    left, rights, lxy, rxys, gs = tiny_guided()
    guides = [capi_guide(capi, g) for g in gs]
    dev = _Sets(capi, left, lxy, rights, rxys, concat=True)
    try:
        for ratio, mutual in ((0.8, True), (float("inf"), True), (float("inf"), False)):
            _equal_singles(dev, guides, ratio, mutual, "tiny")
        got, counts, total = dev.many(guides, float("inf"), False, null_skipped=True)
        for k, part in enumerate(slices(got, counts)):
            if TINY_LENS[k] > 0 and gs[k][0] != NONE:
                assert counts[k] > 0
                row = part[part["left"] == k % 70]
                assert len(row) == 1 and row["d1"][0] == 0, k
            else:
                assert counts[k] == 0
    finally:
        dev.close()


# ---- 7. the shared scratch -------------------------------------------------------------------------------------------------
def test_scratch_shared_with_the_other_many_calls(capi):
    """on one thread's scratch, in sequence: the guided one-to-many call, psx_match_pairs_many_u8, psx_ransac_homography_many
    on its lists, the guided call again (identical bytes), psx_match_release, the guided call again"""
    case = CASES[1]
    seed, nl, lens = case
    left, rights, lxy, rxys = positioned_many(*case)
    guides = [capi_guide(capi, guide_of(k)) for k in range(len(lens))]
    dev = _Sets(capi, left, lxy, rights, rxys)
    try:
        first, counts, total = dev.many(guides, 0.8, True)
        assert total > 50
        lists, c_un = capi.match_pairs_many_u8(left, rights, 0.8, True)
        assert c_un.sum() > 50
        res = capi.ransac_homography_many(lists, lxy, rxys, capi.ransac_opts(2.0, 64, 1))
        assert res["count"] >= 0 and len(res["results"]) == len(lens)
        again, c2, t2 = dev.many(guides, 0.8, True)
        assert t2 == total and np.array_equal(c2, counts) and again.tobytes() == first.tobytes()
        assert capi.lib().psx_match_release() == 0
        third, c3, t3 = dev.many(guides, 0.8, True)
        assert t3 == total and np.array_equal(c3, counts) and third.tobytes() == first.tobytes()
    finally:
        dev.close()


# ---- 8. the chain ----------------------------------------------------------------------------------------------------------
def test_the_three_call_chain_on_device_pointers(capi):
    """match_pairs_many_dev -> ransac_homography_many_dev -> guides_from_ransac -> match_pairs_guided_many_dev, nothing but
    counts, models and guides crossing to the host.  Four planted sets whose right positions follow a known homography of
    their own (partners within 0.4 px of it, every other right point anywhere), and a set of 3 rows that cannot be
    verified: its guide is of kind 0 and its slice empty.  Every other slice equals the single guided call under the same
    guide and contains every pair of the unguided mutual slice that satisfies the rule."""
    nl, lens = 400, (300, 3, 500, 260, 350)
    left, rights = planted_many(41, nl, lens)
    rng = np.random.default_rng(41)
    lxy = rng.uniform(0.0, 600.0, (nl, 2))
    rxys = []
    for k, nr in enumerate(lens):
        h = translated(H_ASYM, 7.0 * k, -4.0 * k)
        x = rng.uniform(0.0, 800.0, (nr, 2))
        # the rows planted_many paired: the same draws
        g = np.random.default_rng([41, k + 1])
        g.integers(0, 64, (nr, 128), dtype=np.uint8)
        m = min(nl, nr) // 2
        if m >= 1:
            src = np.concatenate([[0], 2 + g.permutation(nl - 2)]).astype(np.int64)[:m]
            dst = g.permutation(nr)[:m]
            x[dst] = _apply_h(h, lxy[src]) + rng.uniform(-0.25, 0.25, (m, 2))
        rxys.append(x.astype(np.float32))
    lxy = lxy.astype(np.float32)
    tl, tlx = torch.from_numpy(left).cuda(), torch.from_numpy(lxy).cuda()
    tr = [torch.from_numpy(r).cuda() for r in rights]
    trx = [torch.from_numpy(x).cuda() for x in rxys]
    rp, rxp = [t.data_ptr() for t in tr], [t.data_ptr() for t in trx]
    cap = nl * len(lens)
    pairs = torch.zeros((cap * 16,), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    counts, total = capi.match_pairs_many_dev(tl.data_ptr(), nl, rp, list(lens), pairs.data_ptr(), cap, 0.8, True)
    assert total == counts.sum() and counts[1] < 4 and all(c >= 30 for k, c in enumerate(counts) if k != 1), list(counts)
    tol = 2.0
    res = capi.ransac_homography_many_dev(pairs.data_ptr(), counts, tlx.data_ptr(), nl, rxp, list(lens), 0, 0, capi.ransac_opts(tol, 256, 3))
    assert [r.best < 0 for r in res["results"]] == [False, True, False, False, False]
    guides = capi.guides_from_ransac(res["results"], capi.GUIDE_HOMOGRAPHY, tol)
    assert [g.kind for g in guides] == [1, 0, 1, 1, 1]
    out = torch.zeros((cap * 16,), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rp[1] = rxp[1] = 0                                       # the skipped set's arrays are not needed
    gcounts, gtotal = capi.match_pairs_guided_many_dev(tl.data_ptr(), tlx.data_ptr(), nl, rp, rxp, list(lens), guides, out.data_ptr(), cap,
                                                       0.8, True)
    assert gtotal == gcounts.sum() and gcounts[1] == 0
    unguided = slices(pairs.cpu().numpy()[:total * 16].view(capi.PAIR_U8_DTYPE), counts)
    guided = slices(out.cpu().numpy()[:gtotal * 16].view(capi.PAIR_U8_DTYPE), gcounts)
    for k in (0, 2, 3, 4):
        want = capi.match_pairs_guided_u8(left, lxy, rights[k], rxys[k], guides[k], 0.8, True)
        assert same_records(guided[k], want) and len(want) >= 30, (k, len(guided[k]), len(want))
        # the inclusion: an unguided mutual pair that satisfies the rule is a guided pair
        u = unguided[k]
        ok = capi.guide_allows(guides[k], lxy, rxys[k])[u["left"], u["right"]]
        have = set(zip(guided[k]["left"].tolist(), guided[k]["right"].tolist()))
        assert ok.sum() >= 30 and all((int(a), int(b)) in have for a, b in zip(u["left"][ok], u["right"][ok])), k
    print("chain: unguided %s -> guided %s" % (list(counts), list(gcounts)))


# ---- 9. C++ ------------------------------------------------------------------------------------------------------------------
def test_cpp_match_pairs_guided_many_on_the_gpu(tmp_path):
    """tests/cpp/test_match_guided_many_api.cpp with POPSIFT_TEST_EXPECT_GPU: FeaturesDev::matchPairsGuidedMany equals the loop
    of matchPairsGuided with MatchOptions::bytes, field by field, with and without the cross-check; the throws happen."""
    libdir = os.path.join(ROOT, "popsift_amd", "lib")
    exe = str(tmp_path / "test_match_guided_many_api")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-pthread", os.path.join(ROOT, "tests", "cpp", "test_match_guided_many_api.cpp"), "-o", exe,
                           "-I", os.path.join(ROOT, "popsift_amd", "csrc", "include"), "-I", os.path.join(ROOT, "include"),
                           "-L", libdir, "-lpopsift", "-lpopsift_hip", "-Wl,-rpath," + libdir])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300,
                         env=dict(os.environ, POPSIFT_TEST_EXPECT_GPU="1"))
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout
    assert "mutual 0:" in out.stdout and "mutual 1:" in out.stdout
