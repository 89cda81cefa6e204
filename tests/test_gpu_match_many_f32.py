"""GPU tests of the one-to-many FLOAT pair search (include/popsift_hip.h, "one descriptor set against many, float
descriptors"): psx_match_pairs_many, its _dev form and FeaturesDev::matchPairsManyFloat.  The contract is "the
concatenation of what psx_match_pairs returns per set": every slice is compared, as bytes, with that call on the same
device arrays in the same process, and for two of the cases also with the HOST join (capi.pairs_join) of the oracle's
directed results, so the check does not rest on the device code alone.  psx_match_many_f32_last says which of the two
paths ran, whether the call fell back, and what it launched and synchronised."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch        # before the HIP library is loaded: torch brings a HIP runtime of its own and must initialise first (_dev form)

from tests.match_many_cases import TINY_LENS, contract, planted_many, slices
from tests.match_many_f32_cases import CASES, CASE_IDS, FLAVOURS, ORACLE_SEEDS, flavour, planned_path, planted_many_f32, tiny_many_f32
from tests.match_many_f32_worker import WORKER_COMBOS, digest
from tests.match_pairs_cases import RATIOS, directed, planted, same_records

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")


class _Sets:
    """a left set and K right sets of float32 rows uploaded once -- as separate allocations, or as slices of ONE buffer
    (concat) --; the one-to-many call and the single call on the same device arrays"""

    def __init__(self, capi, left, rights, concat=False):
        self.capi, self.L, self.bufs = capi, capi.lib(), []
        self.left = np.ascontiguousarray(left, np.float32).reshape(-1, 128)
        self.rights = [np.ascontiguousarray(r, np.float32).reshape(-1, 128) for r in rights]
        self.lens = [len(r) for r in self.rights]
        if concat:
            whole = np.concatenate(self.rights) if self.rights else np.zeros((0, 128), np.float32)
            self.pl, base = capi._to_device(self.L, 0, [self.left, whole], self.bufs)
            offs = np.concatenate([[0], np.cumsum(self.lens)]).astype(np.int64) * 512
            self.pr = [C.c_void_p((base.value or 0) + int(o)) if n else C.c_void_p() for o, n in zip(offs, self.lens)]
        else:
            ptrs = capi._to_device(self.L, 0, [self.left] + self.rights, self.bufs)
            self.pl, self.pr = ptrs[0], ptrs[1:]

    def many(self, ratio, mutual, capacity=None, order=None):
        """(records, per-set counts, total); order: which sets, in which order (default: all).  self.info: the call's"""
        order = range(len(self.rights)) if order is None else order
        ptrs, lens = [self.pr[k] for k in order], [self.lens[k] for k in order]
        cap = len(self.left) * len(lens) if capacity is None else capacity
        out = np.zeros((cap,), self.capi.PAIR_DTYPE)
        counts, n = self.capi._many_call(self.L.psx_match_pairs_many, "psx_match_pairs_many", 0, self.pl, len(self.left), ptrs, lens,
                                         out.ctypes.data_as(C.c_void_p) if cap else None, cap, ratio, mutual)
        self.info = self.capi.match_many_f32_last()
        return out[:min(n, cap)], counts, n

    def single(self, k, ratio, mutual):
        return self.capi._pairs_call(self.L.psx_match_pairs, "psx_match_pairs", 0, self.pl, len(self.left), self.pr[k], self.lens[k],
                                     ratio, mutual, self.capi.PAIR_DTYPE, None)[0]

    def close(self):
        for p in self.bufs:
            self.L.psx_dev_free(0, p)
        self.bufs = []


def _equal_singles(dev, ratio, mutual, what, fell_back=0):
    """one call against the loop of single calls: every slice, the counts, the total; the path is the planned one and the
    call fell back (or not) as expected, with one synchronisation more when it did; returns the per-set lists"""
    got, counts, total = dev.many(ratio, mutual)
    info = dev.info
    per_set = [dev.single(k, ratio, mutual) for k in range(len(dev.rights))]
    want, wcounts, wtotal = contract(per_set)
    assert total == wtotal and np.array_equal(counts, wcounts), (what, ratio, mutual, list(counts), list(wcounts))
    for k, (a, b) in enumerate(zip(slices(got, counts), per_set)):
        assert same_records(a, b), (what, ratio, mutual, k, len(a), len(b))
    assert got.tobytes() == want.tobytes()
    path = planned_path(len(dev.left), dev.lens)
    assert info["path"] == path and dev.capi.match_many_f32_plan(len(dev.left), dev.lens, mutual)["path"] == path, (what, info)
    if fell_back is not None:
        assert info["fell_back"] == fell_back and info["syncs"] == 1 + fell_back, (what, ratio, mutual, info)
        if not fell_back:
            assert info["launches"] == dev.capi.match_many_f32_plan(len(dev.left), dev.lens, mutual)["launches"], (what, info)
    return per_set


# ---- 1. the cases -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", FLAVOURS)
@pytest.mark.parametrize("seed,nl,lens", CASES, ids=CASE_IDS)
def test_many_equals_the_single_calls(oracle, capi, seed, nl, lens, which):
    """every ratio and both flag values: each slice equals psx_match_pairs(L, R_k), the counts are equal, the planned
    path ran without falling back and synchronised once; seeds 31 and 34 also against the host join of the oracle's
    directed results (the premise of the planted sets is asserted on the CPU, tests/test_match_many_f32_cpu.py)"""
    left, rights = planted_many_f32(seed, nl, lens, which)
    dev = _Sets(capi, left, rights)
    try:
        joins = {}
        if seed in ORACLE_SEEDS:
            for k, r in enumerate(rights):
                fm, fd, bm, bd = directed(oracle, ("many f32", seed, which, k), left, r, False)
                joins[k] = (fm, fd, bm)
        for ratio in RATIOS:
            for mutual in (False, True):
                per_set = _equal_singles(dev, ratio, mutual, (seed, which))
                for k, (fm, fd, bm) in joins.items():
                    want = capi.pairs_join(fm, fd, bm if mutual else None, len(rights[k]), ratio, mutual)
                    assert same_records(per_set[k], want), (seed, which, k, ratio, mutual, len(per_set[k]), len(want))
        got, counts, total = dev.many(0.8, True)
        print("seed %d %s: %d x %s -> %s pairs, %s" % (seed, which, nl, list(lens), list(counts), dev.info))
        assert all(c == 0 for c, n in zip(counts, lens) if n == 0) and total > 0
    finally:
        dev.close()


# ---- 2. the scan path at the same shapes -----------------------------------------------------------------------------------
def test_scan_path_in_a_child_process_gives_the_same_bytes(capi):
    """POPSIFT_MATCH_MFMA=0 in a fresh child process (the switch is read once per thread's scratch): seeds 31 and 34 take
    path 1 there and path 2 here, and the records' SHA-1 is the same"""
    env = dict(os.environ, POPSIFT_MATCH_MFMA="0")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "match_many_f32_worker.py")] + [str(s) for s in ORACLE_SEEDS],
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    child = json.loads(out.stdout.strip().splitlines()[-1])
    assert len(child) == len(ORACLE_SEEDS) * len(FLAVOURS) * len(WORKER_COMBOS)
    for seed in ORACLE_SEEDS:
        _, nl, lens = [c for c in CASES if c[0] == seed][0]
        for which in FLAVOURS:
            left, rights = planted_many_f32(seed, nl, lens, which)
            dev = _Sets(capi, left, rights)
            try:
                for ratio, mutual in WORKER_COMBOS:
                    got, counts, total = dev.many(ratio, mutual)
                    path, fell, sha = child["%d/%s/%r/%d" % (seed, which, ratio, mutual)]
                    assert (path, fell) == (1, 0) and dev.info["path"] == 2 and dev.info["fell_back"] == 0, (seed, which, dev.info)
                    assert total > 0 and sha == digest(got, counts), (seed, which, ratio, mutual)
            finally:
                dev.close()


# ---- 3. nothing leaks across a set boundary ---------------------------------------------------------------------------
@pytest.mark.parametrize("lens", [(33, 40, 4100), (255, 256, 257, 40, 3400)], ids=["33", "255-256-257"])
def test_no_leak_across_a_set_boundary(capi, lens):
    """In ONE buffer every set is followed by a set whose first 31 rows are exact copies of left rows: a tile, a staged block
    or an outer block that ran past its set's last row would meet distance 0 there.  33 rows: the forward direction's
    last tile holds one row of the set and 31 of the next; 255 / 256 / 257: a backward outer block ends inside a tile, at
    a tile, one past.  Every set's result must equal its stand-alone result (its own allocation, the single call).  The
    last set makes the call large enough for the prefilter; 300 left rows."""
    rng = np.random.default_rng(sum(lens))
    left = rng.integers(0, 64, (300, 128), dtype=np.uint8)
    rights = []
    for k, n in enumerate(lens):
        r = rng.integers(0, 64, (n, 128), dtype=np.uint8)
        r[:31] = left[40 * k:40 * k + 31]                   # exact copies: distance 0 for whoever reads them
        r[31 + k] = left[250 + k] ^ 1                       # and one near-copy of its own, so that no list is trivial
        rights.append(r)
    for which in FLAVOURS:
        fl, fr = flavour(left, which), [flavour(r, which) for r in rights]
        cat, alone = _Sets(capi, fl, fr, concat=True), _Sets(capi, fl, fr)
        try:
            for ratio, mutual in ((0.8, False), (0.8, True), (INF, True), (INF, False)):
                got, counts, total = cat.many(ratio, mutual)
                assert cat.info["path"] == 2 and cat.info["fell_back"] == 0, cat.info
                for k, part in enumerate(slices(got, counts)):
                    want = alone.single(k, ratio, mutual)
                    assert len(want) >= 31 and same_records(part, want), (lens, which, k, ratio, mutual, len(part), len(want))
                    assert part["right"].max() < lens[k]
        finally:
            cat.close(); alone.close()


# ---- 4. ties and the fallback ---------------------------------------------------------------------------------------------
def _tie_sets(run):
    """300 left rows; a 1100-row set whose rows 500 .. 500 + run - 1 are identical, and a 3000-row filler.  left[7] EQUALS
    the run's row (0 / 0: never kept), left[9] is one step away from it (d1 == d2 == 1 when the run has two rows or more)"""
    rng = np.random.default_rng(6)
    big = rng.integers(0, 64, (1100, 128), dtype=np.uint8)
    big[500:500 + run] = big[500]
    filler = rng.integers(0, 64, (3000, 128), dtype=np.uint8)
    left = rng.integers(0, 64, (300, 128), dtype=np.uint8)
    left[7] = big[500]
    left[9] = big[500]
    left[9, 3] += 1
    return left.astype(np.float32), [big.astype(np.float32), filler.astype(np.float32)]


@pytest.mark.parametrize("run,fell_back", [(401, 1), (3, 0)], ids=["401-equal-rows", "3-equal-rows"])
def test_ties_and_the_fallback(oracle, capi, run, fell_back):
    """401 equal neighbours overflow a candidate segment of 32: the flag comes back up, the scan repeats the call (a
    second synchronisation) and the result is still the single calls' and the oracle's; three equal rows fit, nothing falls
    back, and the earlier index wins either way.  A defined path, not a fault."""
    left, rights = _tie_sets(run)
    fm, fd, bm, bd = directed(oracle, ("many f32 ties", run), left, rights[0], False)
    assert list(fm[9, :2]) == [500, 501] and list(fd[9]) == [1, 1] and list(fm[7, :2]) == [500, 501] and list(fd[7]) == [0, 0]
    dev = _Sets(capi, left, rights)
    try:
        for ratio in RATIOS:
            for mutual in (False, True):
                per_set = _equal_singles(dev, ratio, mutual, ("ties", run), fell_back=fell_back)
                assert same_records(per_set[0], capi.pairs_join(fm, fd, bm if mutual else None, 1100, ratio, mutual)), (ratio, mutual)
        got = slices(*dev.many(INF, False)[:2])[0]
        row = got[got["left"] == 9]
        assert len(row) == 1 and row["right"][0] == 500 and row["d1"][0] == row["d2"][0] == 1.0
        assert 7 not in got["left"] and 9 not in slices(*dev.many(1.0, False)[:2])[0]["left"]
    finally:
        dev.close()


# ---- 5. norms the margin cannot bound -------------------------------------------------------------------------------------
@pytest.mark.parametrize("what,fell_back", [("nan", 1), ("zero", 0), ("inf", 1)])
def test_norms_the_margin_cannot_bound(capi, what, fell_back):
    """One NaN row in one set / one +inf element: match_scale refuses the norms, the flag is up from the start and the scan
    answers -- a NaN distance never wins, as in the single calls.  An all-zero set of 40 rows is no such case (the
    largest norms are positive): the prefilter answers, every one of its rows ties, and 20 equal candidates per half
    wave fit a segment."""
    left, rights = planted_many(32, 257, (64, 1000, 300, 2800))
    left, rights = left.astype(np.float32), [r.astype(np.float32) for r in rights]
    if what == "nan":
        rights[1][17, 5] = np.nan
    elif what == "inf":
        rights[2][3, 100] = np.inf
    else:
        rights.insert(1, np.zeros((40, 128), np.float32))
    dev = _Sets(capi, left, rights)
    try:
        for ratio, mutual in ((0.8, True), (0.8, False), (INF, True), (INF, False)):
            _equal_singles(dev, ratio, mutual, what, fell_back=fell_back)
    finally:
        dev.close()


# ---- 6. capacity and counts -----------------------------------------------------------------------------------------------
def test_capacity_and_counts(capi):
    """truncation in the middle of a set, exactly at a set boundary, at count - 1 and at 0 with NULL: the totals are still
    reported, the record behind the capacity is untouched -- in a host buffer and in a device buffer read back"""
    seed, nl, lens = CASES[1]
    left, rights = planted_many_f32(seed, nl, lens, "norm512")
    dev = _Sets(capi, left, rights)
    L = capi.lib()
    try:
        full, counts, total = dev.many(0.8, True)
        assert np.all(counts > 4) and total == counts.sum() == len(full) and dev.info["path"] == 2
        tl = torch.from_numpy(dev.left.copy()).cuda()
        tr = [torch.from_numpy(r.copy()).cuda() for r in dev.rights]
        for cap in (int(counts[0] + counts[1] // 2), int(counts[0]), total - 1, 0, total, total + 3):
            host = np.full(((cap + 2) * 4,), -7, np.int32).view(capi.PAIR_DTYPE)
            c2, n2 = capi._many_call(L.psx_match_pairs_many, "psx_match_pairs_many", 0, dev.pl, nl, dev.pr, dev.lens,
                                     host.ctypes.data_as(C.c_void_p) if cap else None, cap, 0.8, True)
            k = min(cap, total)
            assert n2 == total and np.array_equal(c2, counts), cap
            assert same_records(host[:k], full[:k]) and np.all(host[k:].view(np.int32) == -7), cap
            want, _, _ = contract(slices(full, counts), cap)
            assert same_records(host[:k], want)
            dbuf = torch.full(((cap + 2) * 16,), 0xA5, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            c3, n3 = capi.match_pairs_many_dev(tl.data_ptr(), nl, [t.data_ptr() for t in tr], dev.lens, dbuf.data_ptr() if cap else 0, cap, 0.8, True,
                                               u8=False)
            back = dbuf.cpu().numpy()
            assert n3 == total and np.array_equal(c3, counts), cap
            assert same_records(back[:k * 16].view(capi.PAIR_DTYPE), full[:k]) and np.all(back[k * 16:] == 0xA5), cap
        # the python wrapper: per-set arrays, cut as the call cut them
        lists, c4 = capi.match_pairs_many(left, rights, 0.8, True, capacity=int(counts[0]) + 2)
        assert np.array_equal(c4, counts) and [len(p) for p in lists] == [counts[0], 2, 0, 0]
        assert same_records(lists[0], full[:counts[0]]) and same_records(lists[1], full[counts[0]:counts[0] + 2])
    finally:
        dev.close()


# ---- 7. many tiny sets -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nl,path", [(70, 1), (300, 2)], ids=["70-left-scan", "300-left-prefilter"])
def test_two_hundred_tiny_sets(capi, nl, path):
    """K = 200 sets of i % 41 rows plus a 4100-row filler, in one buffer: 201 workgroup totals in the scan, empty sets in
    between, sets shorter than a tile, a staged block and a chunk; every non-empty tiny set holds an exact copy of a left
    row, so every one of them yields a pair.  70 left rows take the scan, 300 the prefilter."""
    left, rights = tiny_many_f32("norm512", nl)
    filler = flavour(np.random.default_rng(7).integers(0, 64, (4100, 128), dtype=np.uint8), "norm512")
    dev = _Sets(capi, left, rights + [filler], concat=True)
    try:
        for ratio, mutual in ((0.8, True), (INF, True), (INF, False)):
            _equal_singles(dev, ratio, mutual, ("tiny", nl))
            assert dev.info["path"] == path
        got, counts, total = dev.many(0.8, True)
        assert all((c > 0) == (n > 0) for c, n in zip(counts[:200], TINY_LENS)) and (counts[:200] > 0).sum() == 195
        for k, part in enumerate(slices(got, counts)[:200]):
            if TINY_LENS[k] > 0:
                assert (k % nl, k % TINY_LENS[k]) in set(zip(part["left"].tolist(), part["right"].tolist())), k
    finally:
        dev.close()


# ---- 8. groups above the budget -----------------------------------------------------------------------------------------------
def test_groups_of_sets_above_the_budget(capi):
    """1024 rows against the same 1024-row set K times, K the smallest for which the plan reports two groups forward and two
    backward (the candidate segments of all sets exceed 256 MiB either way): every slice equals the one single call, and
    the call still synchronises once."""
    nl = nr = 1024
    k = 1
    while capi.match_many_f32_plan(nl, (nr,) * k, True)["fwd_groups"] < 2:
        k += 1
    while capi.match_many_f32_plan(nl, (nr,) * k, True)["bwd_groups"] < 2:
        k += 1
    plan = capi.match_many_f32_plan(nl, (nr,) * k, True)
    assert plan["path"] == 2 and plan["fwd_groups"] >= 2 and plan["bwd_groups"] >= 2 and plan["scratch_bytes"] <= 256 << 20
    left, right = planted(1024, nl, nr)
    dev = _Sets(capi, flavour(left, "norm512"), [flavour(right, "norm512")])
    try:
        want = dev.single(0, 0.8, True)
        assert len(want) > 100
        got, counts, total = dev.many(0.8, True, order=(0,) * k)
        print("K = %d: %s, %s" % (k, plan, dev.info))
        assert dev.info == {"path": 2, "fell_back": 0, "launches": plan["launches"], "syncs": 1}
        assert total == k * len(want) and np.all(counts == len(want))
        assert got.tobytes() == want.tobytes() * k
    finally:
        dev.close()


# ---- 9. cost does not grow with K ------------------------------------------------------------------------------------------
def test_cost_does_not_grow_with_the_number_of_sets(capi):
    """3 and 40 sets of 1400 rows against 300 left rows: the same launches and synchronisations, with and without the
    cross-check"""
    left, rights = planted_many(39, 300, (1400,) * 40)
    left, rights = flavour(left, "norm512"), [flavour(r, "norm512") for r in rights]
    dev = _Sets(capi, left, rights)
    try:
        for mutual, launches in ((True, 9), (False, 7)):
            dev.many(0.8, mutual, order=range(3))
            a = dict(dev.info)
            got, counts, total = dev.many(0.8, mutual)
            b = dict(dev.info)
            assert a == b == {"path": 2, "fell_back": 0, "launches": launches, "syncs": 1}, (a, b)
            assert np.all(counts > 0)
    finally:
        dev.close()


# ---- 10. where the sets lie ---------------------------------------------------------------------------------------------
def test_separate_allocations_slices_and_the_same_pointer(capi):
    """the same sets as separate allocations and as slices of one concatenated buffer: identical bytes; a set given at
    positions 0, 1 and 3 yields the same list each time"""
    seed, nl, lens = CASES[0]
    left, rights = planted_many_f32(seed, nl, lens, "norm512")
    a, b = _Sets(capi, left, rights), _Sets(capi, left, rights, concat=True)
    try:
        for ratio, mutual in ((0.8, True), (0.8, False), (INF, True)):
            ra, ca, na = a.many(ratio, mutual)
            rb, cb, nb = b.many(ratio, mutual)
            assert na == nb > 0 and np.array_equal(ca, cb) and ra.tobytes() == rb.tobytes(), (ratio, mutual)
        big, other = len(lens) - 1, 9                        # the 3000-row set and the 512-row set
        for ratio, mutual in ((0.8, True), (INF, False)):
            got, counts, total = a.many(ratio, mutual, order=(big, big, other, big))
            parts = slices(got, counts)
            one = a.single(big, ratio, mutual)
            assert a.info["path"] == 2 and len(one) > 0 and counts[0] == counts[1] == counts[3] == len(one)
            assert same_records(parts[0], one) and same_records(parts[1], one) and same_records(parts[3], one)
            assert same_records(parts[2], a.single(other, ratio, mutual))
    finally:
        a.close(); b.close()


# ---- 11. the shared scratch -------------------------------------------------------------------------------------------------
def test_scratch_shared_with_the_other_matchers(capi):
    """on one thread's scratch, in sequence: float one-to-many, psx_match_pairs, psx_match_pairs_many_u8,
    psx_ransac_homography on a slice's pairs, float one-to-many again (identical bytes), psx_match_release, float one-to-many
    again"""
    seed, nl, lens = CASES[1]
    left, rights = planted_many_f32(seed, nl, lens, "int")
    dev = _Sets(capi, left, rights)
    try:
        first, counts, total = dev.many(0.8, True)
        assert total > 50 and dev.info["path"] == 2
        one = dev.single(1, 0.8, True)
        assert same_records(one, slices(first, counts)[1])
        lu, ru = planted_many(seed, nl, lens)
        lists_u8, counts_u8 = capi.match_pairs_many_u8(lu, ru, 0.8, True)
        # integer-valued floats: the byte call finds the same pairs at the same (integer) distances
        assert np.array_equal(counts_u8, counts) and all(np.array_equal(a["right"], b["right"]) for a, b in zip(lists_u8, slices(first, counts)))
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


# ---- 12. real descriptors --------------------------------------------------------------------------------------------------
def test_real_descriptors(capi):
    """A synthetic 640 x 480 frame and five warped copies through Context.extract (float descriptors, the default
    normalisation): the one call equals the loop of single calls, the path is the planned one and the call does not fall
    back -- the condition the segment sizing has to meet on real content."""
    from popsift_amd.synth import synth, warp_homography
    a = synth(640, 480, 4243)
    views = [a]
    for i in range(5):
        H = np.array([[1.0 + 0.01 * i, 0.02 * (i - 2), 3.0 + 2 * i], [-0.015 * (i - 2), 1.0 - 0.005 * i, 2.0 - i], [1e-5 * i, -1e-5 * i, 1.0]])
        views.append(warp_homography(a, H))
    descs = []
    for img in views:
        ctx = capi.Context(capi.default_config(octaves=4))
        ctx.upload(img)
        ctx.extract()
        descs.append(np.ascontiguousarray(ctx.download()[1], np.float32).reshape(-1, 128))
        ctx.close()
    assert all(len(d) > 1000 for d in descs), [len(d) for d in descs]
    dev = _Sets(capi, descs[0], descs[1:])
    try:
        assert planned_path(len(descs[0]), dev.lens) == 2
        for ratio, mutual in ((0.8, True), (0.8, False), (INF, True)):
            per_set = _equal_singles(dev, ratio, mutual, "real", fell_back=0)
        print("real descriptors: %d against %s -> %s mutual pairs at inf, %s" % (len(descs[0]), dev.lens, [len(p) for p in per_set], dev.info))
        assert all(len(p) > 100 for p in _equal_singles(dev, 0.8, True, "real", fell_back=0))
    finally:
        dev.close()


# ---- 13. C++ -----------------------------------------------------------------------------------------------------------------
def test_cpp_match_pairs_many_float_on_the_gpu(tmp_path):
    """tests/cpp/test_match_many_f32_api.cpp with POPSIFT_TEST_EXPECT_GPU: FeaturesDev::matchPairsManyFloat equals the loop
    of matchPairs, field by field, with and without the cross-check; estimateHomographyMany accepts its lists; the throws
    happen."""
    libdir = os.path.join(ROOT, "popsift_amd", "lib")
    exe = str(tmp_path / "test_match_many_f32_api")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-pthread", os.path.join(ROOT, "tests", "cpp", "test_match_many_f32_api.cpp"), "-o", exe,
                           "-I", os.path.join(ROOT, "popsift_amd", "csrc", "include"), "-I", os.path.join(ROOT, "include"),
                           "-L", libdir, "-lpopsift", "-lpopsift_hip", "-Wl,-rpath," + libdir])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300,
                         env=dict(os.environ, POPSIFT_TEST_EXPECT_GPU="1"))
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout
    assert "mutual 0:" in out.stdout and "mutual 1:" in out.stdout and "homographies: 4" in out.stdout
