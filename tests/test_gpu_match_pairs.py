"""GPU tests of the pair search (include/popsift_hip.h, "matches as data"): psx_match_pairs / psx_match_pairs_u8, their
_dev forms, FeaturesDev::matchPairs and popsift-match --pairs.  The expected list is always the HOST join
(capi.pairs_join, pinned to a numpy restatement in tests/test_match_pairs_cpu.py) of directed results both ways -- the
oracle's, or, where the directed matcher is already pinned to the oracle at that size, capi.match's.  Records are compared
bit for bit: indices, and distances as their 32-bit patterns."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch        # before the HIP library is loaded: torch brings a HIP runtime of its own and must initialise first (_dev forms)

from popsift_amd.synth import synth
from tests.match_pairs_cases import (AMPS, INT_MAX, RATIOS, assert_premise, directed, dist_as_int, planted, restate, same_records)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MATCH = os.path.join(ROOT, "popsift_amd", "lib", "popsift-match")


class _OnDevice:
    """two descriptor sets uploaded once; pairs calls with any options on them"""

    def __init__(self, capi, left, right):
        self.capi, self.L, self.bufs = capi, capi.lib(), []
        self.u8 = left.dtype == np.uint8
        self.left, self.right = np.ascontiguousarray(left).reshape(-1, 128), np.ascontiguousarray(right).reshape(-1, 128)
        self.pl, self.pr = capi._to_device(self.L, 0, [self.left, self.right], self.bufs)
        self.fn = self.L.psx_match_pairs_u8 if self.u8 else self.L.psx_match_pairs
        self.dtype = capi.PAIR_U8_DTYPE if self.u8 else capi.PAIR_DTYPE

    def pairs(self, ratio, mutual, capacity=None):
        got = self.capi._pairs_call(self.fn, "pairs", 0, self.pl, len(self.left), self.pr, len(self.right), ratio, mutual,
                                    self.dtype, capacity)
        return got[0] if capacity is None else got

    def close(self):
        for p in self.bufs:
            self.L.psx_dev_free(0, p)
        self.bufs = []


def _check_all(capi, dev, fm, fd, bm, what):
    """every ratio and both flag values against the host join of (fm, fd, bm)"""
    nr = len(dev.right)
    for ratio in RATIOS:
        for mutual in (False, True):
            want = capi.pairs_join(fm, fd, bm if mutual else None, nr, ratio, mutual)
            got = dev.pairs(ratio, mutual)
            assert same_records(got, want), (what, ratio, mutual, len(got), len(want))


def _unit(rng, n):
    v = rng.random((n, 128), dtype=np.float32) ** 4
    return np.sqrt(v / v.sum(1, keepdims=True)).astype(np.float32)


# ---- bytes against the oracle ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("nl,nr,seed", [(300, 257, 1), (257, 513, 2), (33, 31, 8), (2500, 2300, 9), (1, 1, 4), (129, 1, 5), (5, 0, 6), (0, 7, 7)])
def test_pairs_u8_equal_the_join_of_the_oracle(oracle, capi, nl, nr, seed):
    """257 x 513: two chunks of 512 one way; 2500 x 2300: several left blocks, several join workgroups"""
    left, right = planted(seed, nl, nr)
    fm, fd, bm, bd = directed(oracle, ("planted", seed, nl, nr, True), left, right, True)
    if min(nl, nr) >= 64:
        assert_premise(fm, fd, bm, nr, (nl, nr))
    dev = _OnDevice(capi, left, right)
    try:
        _check_all(capi, dev, fm, fd, bm, (nl, nr))
    finally:
        dev.close()


def test_pairs_u8_adversarial(oracle, capi):
    """the construction of test_match_u8_adversarial: ties everywhere, all-0 / all-255, many duplicates"""
    rng = np.random.default_rng(11)
    right = rng.integers(100, 104, size=(1500, 128), dtype=np.uint8)
    right[::7] = 0
    right[3::11] = 255
    right[500:900] = right[100]
    left = np.concatenate([rng.integers(100, 104, size=(300, 128), dtype=np.uint8), np.zeros((5, 128), np.uint8),
                           np.full((5, 128), 255, np.uint8), right[100:110]])
    fm, fd, bm, bd = directed(oracle, ("adversarial",), left, right, True)
    dev = _OnDevice(capi, left, right)
    try:
        _check_all(capi, dev, fm, fd, bm, "adversarial")
    finally:
        dev.close()
    # all-0 against all-255 only: d1 == d2, kept by ratio = inf alone; the cross-check keeps left 0 -> right 0
    dev = _OnDevice(capi, np.zeros((3, 128), np.uint8), np.full((2, 128), 255, np.uint8))
    try:
        assert len(dev.pairs(1.0, False)) == 0
        got = dev.pairs(float("inf"), False)
        assert list(got["left"]) == [0, 1, 2] and np.all(got["right"] == 0) and np.all(got["d1"] == 128 * 255 * 255)
        got = dev.pairs(float("inf"), True)
        assert list(got["left"]) == [0] and list(got["right"]) == [0]
    finally:
        dev.close()


# ---- compaction edges -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_compaction_edges(oracle, capi, n):
    """right = a copy of left: every row pairs with itself at ratio inf, mutual (one wave, a wave boundary, one workgroup,
    a workgroup boundary); a right side without partners gives the empty list at 0.6; capacity count - 1 and 0 report the
    total and leave the record behind the capacity alone -- in the host buffer and in a device buffer read back."""
    rng = np.random.default_rng(100 + n)
    left = rng.integers(0, 64, (n, 128), dtype=np.uint8)
    dev = _OnDevice(capi, left, left.copy())
    L = capi.lib()
    try:
        got = dev.pairs(float("inf"), True)
        assert len(got) == n and np.array_equal(got["left"], np.arange(n)) and np.array_equal(got["right"], np.arange(n))
        assert np.all(got["d1"] == 0)
        fm, fd, bm, bd = directed(oracle, ("self", n), left, left, True)
        assert same_records(got, capi.pairs_join(fm, fd, bm, n, float("inf"), True))
        o = capi.match_opts(float("inf"), True)
        for cap in sorted({max(n - 1, 0), 0}):
            host = np.full(((cap + 2) * 4,), -7, np.int32).view(capi.PAIR_U8_DTYPE)
            cnt = C.c_int(-1)
            rc = L.psx_match_pairs_u8(0, dev.pl, n, dev.pr, n, C.byref(o), host.ctypes.data_as(C.c_void_p) if cap else None, cap, C.byref(cnt))
            assert rc == 0 and cnt.value == n, cap
            assert same_records(host[:cap], got[:cap]) and np.all(host[cap:].view(np.int32) == -7), cap
            dbuf = torch.full(((cap + 2) * 16,), 0xA5, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            cnt = capi.match_pairs_dev(dev.pl.value, n, dev.pr.value, n, dbuf.data_ptr(), cap, float("inf"), True, u8=True)
            back = dbuf.cpu().numpy()
            assert cnt == n, cap
            assert same_records(back[:cap * 16].view(capi.PAIR_U8_DTYPE), got[:cap]) and np.all(back[cap * 16:] == 0xA5), cap
    finally:
        dev.close()
    other = _OnDevice(capi, left, rng.integers(0, 64, (max(n, 40), 128), dtype=np.uint8))
    try:
        for mutual in (False, True):
            part, cnt = other.pairs(0.6, mutual, capacity=4)
            assert cnt == 0 and len(part) == 0
    finally:
        other.close()


def test_compaction_past_256_workgroups(oracle, capi):
    """65 793 = 256 * 257 + 1 left rows against 40 right rows: 258 join workgroups, the smallest size at which the last
    workgroup's sum over the totals of the workgroups before it takes a second trip (it reads totals 0 .. 256 with 256
    threads).  Left rows are noisy copies of right rows (the amplitudes of the planted sets) with a density that differs
    from workgroup to workgroup -- none, 5 %, half, all -- so a wrong prefix moves records, not only the total; the only
    exact copies lie in workgroup 256 and in the last row, so the cross-check keeps rows there and the total depends on
    workgroup 256's count.  Every ratio, with and without the cross-check, host and device form, all records and the count
    against the host join of the oracle's directed results."""
    n, nr = 256 * 257 + 1, 40
    rng = np.random.default_rng(65793)
    right = rng.integers(0, 64, (nr, 128), dtype=np.uint8)
    left = rng.integers(0, 64, (n, 128), dtype=np.uint8)
    density = rng.choice([0.0, 0.05, 0.5, 1.0], 258)
    density[256] = 0.5
    rows = np.nonzero(rng.random(n) < density[np.arange(n) // 256])[0]
    amp = np.array(AMPS)[rows % len(AMPS)]
    noise = np.rint((rng.random((len(rows), 128)) * 2 - 1) * amp[:, None]).astype(np.int64)
    noise[np.arange(len(rows)), rows % 128] += 1                           # never an exact copy
    left[rows] = np.clip(right[rows % nr].astype(np.int64) + noise, 0, 255).astype(np.uint8)
    exact = 65536 + 5 * np.arange(nr - 1)
    left[exact] = right[:nr - 1]
    left[n - 1] = right[nr - 1]
    fm, fd, bm, bd = directed(oracle, ("past 256 workgroups",), left, right, True)
    dev = _OnDevice(capi, left, right)
    try:
        for ratio in RATIOS:
            for mutual in (False, True):
                want = capi.pairs_join(fm, fd, bm if mutual else None, nr, ratio, mutual)
                wg = want["left"] // 256
                assert (wg == 256).any() and want["left"][-1] == n - 1, (ratio, mutual)
                if not mutual and ratio < 1.0:                             # (from 1.0 on nearly every row survives)
                    per_wg = np.bincount(wg, minlength=258)
                    assert (per_wg[:256] == 0).any() and (per_wg[:256] > 100).any(), ratio
                if ratio == float("inf") and not mutual:
                    assert len(want) == n and np.array_equal(want["left"], np.arange(n))
                got = dev.pairs(ratio, mutual)
                assert same_records(got, want), (ratio, mutual, len(got), len(want))
                dbuf = torch.full(((n + 1) * 16,), 0xA5, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                cnt = capi.match_pairs_dev(dev.pl.value, n, dev.pr.value, nr, dbuf.data_ptr(), n, ratio, mutual, u8=True)
                back = dbuf.cpu().numpy()
                assert cnt == len(want), (ratio, mutual, cnt, len(want))
                assert same_records(back[:cnt * 16].view(capi.PAIR_U8_DTYPE), want) and np.all(back[cnt * 16:] == 0xA5), (ratio, mutual)
    finally:
        dev.close()


# ---- floats -------------------------------------------------------------------------------------------------------------
def test_pairs_f32_equal_the_join_of_the_oracle(oracle, capi):
    """the planted sets cast to float32, and unit-norm RootSift-like sets with duplicates below the prefilter's size limit
    (the exact scan both ways), bit for bit"""
    rng = np.random.default_rng(31)
    cases = []
    for nl, nr, seed in ((300, 257, 1), (257, 513, 2), (1, 1, 4), (129, 1, 5)):
        l, r = planted(seed, nl, nr)
        cases.append((("planted", seed, nl, nr, False), l.astype(np.float32), r.astype(np.float32)))
    l, r = _unit(rng, 600), _unit(rng, 3000)
    r[100] = l[5]; r[2000] = l[5]; r[17] = l[9]; r[18] = l[9] + np.float32(1e-4)
    for t in range(40, 240):                                             # near-copies: pairs that pass the ratio test
        r[3 * t] = l[t] + (rng.random(128, dtype=np.float32) - np.float32(0.5)) * np.float32(0.02 * (1 + t % 5))
    l[300] = l[41]
    cases.append((("unit", 31), l, r))
    for key, l, r in cases:
        fm, fd, bm, bd = directed(oracle, key, l, r, False)
        if len(l) >= 300:
            assert_premise(fm, fd, bm, len(r), key)
        dev = _OnDevice(capi, l, r)
        try:
            _check_all(capi, dev, fm, fd, bm, key)
        finally:
            dev.close()
    # empty sides
    for nl, nr in ((5, 0), (0, 7)):
        assert len(capi.match_pairs(np.zeros((nl, 128), np.float32), np.zeros((nr, 128), np.float32), float("inf"), True)) == 0


def test_pairs_f32_prefilter_in_both_directions(capi):
    """4200 x 4300 unit-norm with planted near-copies: both directions take the MFMA prefilter (r_len >= 4096 and l_len >= 256
    seen from either side).  Against the host join of capi.match run both ways: the directed matcher is pinned to the
    oracle at these sizes (test_match_mfma_prefilter_equals_exact_scan)."""
    rng = np.random.default_rng(41)
    l, r = _unit(rng, 4200), _unit(rng, 4300)
    for t in range(0, 2000):
        r[2 * t + 1] = l[t] + (rng.random(128, dtype=np.float32) - np.float32(0.5)) * np.float32(0.01 * (1 + t % 6))
    l[3000] = l[10]; l[3001] = l[11]                                     # many-to-one
    r[4299] = r[21]                                                      # a duplicated right row: d1 == d2
    fm, fd = capi.match(l, r)
    bm, bd = capi.match(r, l)
    assert_premise(fm, fd, bm, len(r), "prefilter")
    dev = _OnDevice(capi, l, r)
    try:
        for ratio, mutual in ((0.8, True), (0.8, False), (float("inf"), True), (0.6, True)):
            want = capi.pairs_join(fm, fd, bm if mutual else None, len(r), ratio, mutual)
            got = dev.pairs(ratio, mutual)
            assert same_records(got, want), (ratio, mutual, len(got), len(want))
    finally:
        dev.close()


def test_pairs_f32_overflow_fallback_inside_a_pairs_call(oracle, capi):
    """The scratch-state sequence of test_match_scratch_state_between_calls with a pairs call in it: thousands of identical
    right rows overflow the candidate segments (the forward direction ends in the exact scan of every pair, the counters are
    not left tidy), then an ordinary capi.match and an ordinary match_pairs at prefilter sizes -- all exact."""
    rng = np.random.default_rng(23)
    lo, ro = _unit(rng, 300), _unit(rng, 9000)
    ro[500:8600] = ro[499]
    ro[8700] = lo[3]; ro[8701] = lo[4] + np.float32(1e-4)
    fm, fd, bm, bd = directed(oracle, ("overflow", 23), lo, ro, False)
    for ratio, mutual in ((0.8, True), (float("inf"), True), (0.8, False)):
        want = capi.pairs_join(fm, fd, bm if mutual else None, len(ro), ratio, mutual)
        assert same_records(capi.match_pairs(lo, ro, ratio, mutual), want), (ratio, mutual)
    lb, rb = _unit(rng, 700), _unit(rng, 4300)
    rb[7] = lb[1]; rb[9] = lb[2] + np.float32(1e-4)
    fm, fd, bm, bd = directed(oracle, ("after overflow", 23), lb, rb, False)
    mg, dg = capi.match(lb, rb)
    assert np.array_equal(mg, fm) and np.array_equal(dg.view(np.uint32), fd.view(np.uint32))
    want = capi.pairs_join(fm, fd, bm, len(rb), 0.8, True)
    assert len(want) >= 2
    assert same_records(capi.match_pairs(lb, rb, 0.8, True), want)
    mg, dg = capi.match(rb, lb)
    assert np.array_equal(mg, bm) and np.array_equal(dg.view(np.uint32), bd.view(np.uint32))


# ---- the existing entry points, in the same process --------------------------------------------------------------------
def test_directed_matchers_unchanged_beside_pairs_calls(oracle, capi):
    left, right = planted(9, 2500, 2300)
    fm, fd, bm, bd = directed(oracle, ("planted", 9, 2500, 2300, True), left, right, True)
    lf, rf = left.astype(np.float32), right.astype(np.float32)
    assert len(capi.match_pairs_u8(left, right, 0.8, True)) > 100
    assert len(capi.match_pairs(lf, rf, 0.8, True)) > 100
    for k in range(2):
        mg, dg = capi.match_u8(left, right)
        assert np.array_equal(mg, fm) and np.array_equal(dg, fd)
        mg, dg = capi.match_u8(right, left)
        assert np.array_equal(mg, bm) and np.array_equal(dg, bd)
        mg, dg = capi.match(lf, rf)
        assert np.array_equal(mg, fm) and np.array_equal(dist_as_int(dg), fd)
        if k == 0:
            assert capi.lib().psx_match_release() == 0
            want = capi.pairs_join(fm, fd, bm, len(right), 0.8, True)
            assert same_records(capi.match_pairs_u8(left, right, 0.8, True), want)


# ---- real descriptors ---------------------------------------------------------------------------------------------------
def test_pairs_on_real_descriptors(oracle, capi):
    """Two views of a synthetic frame shifted by 3 pixels (the construction of test_match_u8_on_quantised_real_descriptors,
    at 640 x 480): the mutual pairs at ratio 0.8 equal the join of the oracle's directed results, for floats and for bytes,
    and at least half of the left descriptors pair (the oracle's own descriptors of these two views give 0.965 for both
    formats)."""
    a = synth(640, 480, 4243)
    df, du = [], []
    for img in (a, np.roll(a, 3, axis=1)):
        ctx = capi.Context(capi.default_config(octaves=4, sift_mode=2, norm_multi=9))
        ctx.set_descriptor_format(capi.DESCFMT_U8)
        ctx.upload(img)
        ctx.extract()
        du.append(ctx.download_u8()[1])
        df.append(ctx.download()[1])
        ctx.close()
    assert len(df[0]) > 1000 and len(df[1]) > 1000
    for u8, (l, r) in ((False, df), (True, du)):
        fm, fd = oracle.match(l.astype(np.float32), r.astype(np.float32))
        bm, bd = oracle.match(r.astype(np.float32), l.astype(np.float32))
        if u8:
            fd = dist_as_int(fd)
        want = capi.pairs_join(fm, fd, bm, len(r), 0.8, True)
        got = capi.match_pairs_u8(l, r, 0.8, True) if u8 else capi.match_pairs(l, r, 0.8, True)
        print("%s: %d of %d left descriptors pair" % ("bytes" if u8 else "float", len(got), len(l)))
        assert same_records(got, want)
        assert len(got) >= 0.5 * len(l)
        assert len(np.unique(got["right"])) == len(got)


# ---- device output ------------------------------------------------------------------------------------------------------
def test_dev_forms_equal_the_host_forms(capi):
    """the list stays in HBM: a torch uint8 tensor viewed with the pair dtype equals the host form's records"""
    left, right = planted(1, 300, 257)
    for u8 in (True, False):
        l = left if u8 else left.astype(np.float32)
        r = right if u8 else right.astype(np.float32)
        dtype = capi.PAIR_U8_DTYPE if u8 else capi.PAIR_DTYPE
        tl, tr = torch.from_numpy(l).cuda(), torch.from_numpy(r).cuda()
        for ratio, mutual in ((0.8, False), (0.8, True), (float("inf"), True)):
            want = capi.match_pairs_u8(l, r, ratio, mutual) if u8 else capi.match_pairs(l, r, ratio, mutual)
            out = torch.zeros((len(l) * 16,), dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            n = capi.match_pairs_dev(tl.data_ptr(), len(l), tr.data_ptr(), len(r), out.data_ptr(), len(l), ratio, mutual, u8=u8)
            got = out.cpu().numpy().view(dtype)
            assert n == len(want) > 0 and same_records(got[:n], want), (u8, ratio, mutual)
            assert not got[n:].view(np.uint8).any()
            # "how many?" with no buffer at all
            assert capi.match_pairs_dev(tl.data_ptr(), len(l), tr.data_ptr(), len(r), 0, 0, ratio, mutual, u8=u8) == n
    dd = capi.DeviceDescriptors(left.astype(np.float32)), capi.DeviceDescriptors(right.astype(np.float32))
    assert same_records(dd[0].match_pairs(dd[1], 0.8, True), capi.match_pairs(left.astype(np.float32), right.astype(np.float32), 0.8, True))
    dd[0].close(); dd[1].close()


# ---- C++ and the command line -------------------------------------------------------------------------------------------
def test_cpp_match_pairs_on_the_gpu(tmp_path):
    """tests/cpp/test_match_pairs_api.cpp with POPSIFT_TEST_EXPECT_GPU: FeaturesDev::matchPairs' descriptor indices and
    distances equal the C-ABI's pairs on the same device arrays, its feature indices are the reverse maps applied to them
    (float and bytes, with and without the cross-check); a refused ratio throws."""
    libdir = os.path.join(ROOT, "popsift_amd", "lib")
    exe = str(tmp_path / "test_match_pairs_api")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-pthread", os.path.join(ROOT, "tests", "cpp", "test_match_pairs_api.cpp"), "-o", exe,
                           "-I", os.path.join(ROOT, "popsift_amd", "csrc", "include"), "-I", os.path.join(ROOT, "include"),
                           "-L", libdir, "-lpopsift", "-lpopsift_hip", "-Wl,-rpath," + libdir])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300,
                         env=dict(os.environ, POPSIFT_TEST_EXPECT_GPU="1"))
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout
    assert "float, mutual 1:" in out.stdout and "bytes, mutual 1:" in out.stdout


def _write_pgm(path, img):
    with open(path, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (img.shape[1], img.shape[0]) + img.tobytes())


def test_match_tool_pairs(capi, tmp_path):
    """popsift-match --pairs FILE writes the pair list (and no accept / reject lines); --ratio, --mutual and
    --uchar-descriptors refine it.  The same two images through a context and match_pairs give the same distances (descriptor
    order is not reproducible between runs: compared as sorted lists of the printed distances) and the same count."""
    base = synth(336, 256, 77)
    a = np.ascontiguousarray(base[8:248, 8:328])
    b = np.ascontiguousarray(base[5:245, 3:323])
    _write_pgm(tmp_path / "l.pgm", a)
    _write_pgm(tmp_path / "r.pgm", b)
    ds = []
    for img in (a, b):
        ctx = capi.Context(capi.default_config(octaves=3, norm_multi=9))      # the byte scale: the quantised form keeps structure
        ctx.upload(img)
        ctx.extract()
        ds.append(ctx.download()[1])
        ctx.close()
    for extra, ratio, mutual, u8 in (([], 0.8, False, False), (["--ratio", "0.7", "--mutual"], 0.7, True, False),
                                     (["--mutual", "--uchar-descriptors", "--ratio=inf"], float("inf"), True, True)):
        out = tmp_path / "pairs.txt"
        p = subprocess.run([MATCH, "-l", "l.pgm", "-r", "r.pgm", "--octaves", "3", "--norm-multi", "9", "--pairs", str(out)] + extra, cwd=str(tmp_path),
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
        assert p.returncode == 0, p.stdout + p.stderr
        assert not any(l.startswith(("accept", "reject")) for l in p.stdout.splitlines())
        rows = [l.split() for l in out.read_text().splitlines()]
        assert "Number of matches: %d" % len(rows) in p.stdout and len(rows) > 20
        assert all(len(r) == 6 for r in rows)
        ld = [int(r[1]) for r in rows]
        assert ld == sorted(set(ld)) and ld[-1] < len(ds[0]) and all(0 <= int(r[3]) < len(ds[1]) for r in rows)
        if mutual:
            assert len({int(r[3]) for r in rows}) == len(rows)
        if u8:
            want = capi.match_pairs_u8(capi.quantize(ds[0]), capi.quantize(ds[1]), ratio, mutual)
            d = np.where(want["d1"] == INT_MAX, np.inf, want["d1"].astype(np.float64)), np.where(want["d2"] == INT_MAX, np.inf, want["d2"].astype(np.float64))
        else:
            want = capi.match_pairs(ds[0], ds[1], ratio, mutual)
            d = want["d1"], want["d2"]
        assert len(rows) == len(want)
        assert sorted((r[4], r[5]) for r in rows) == sorted(("%.3f" % x, "%.3f" % y) for x, y in zip(d[0], d[1]))
    # refinements without --pairs: a usage error; the plain tool still prints its lines
    for extra in (["--ratio", "0.7"], ["--mutual"]):
        p = subprocess.run([MATCH, "-l", "l.pgm", "-r", "r.pgm", "--octaves", "3", "--norm-multi", "9"] + extra, cwd=str(tmp_path),
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
        assert p.returncode != 0 and "--pairs" in p.stderr
    p = subprocess.run([MATCH, "-l", "l.pgm", "-r", "r.pgm", "--octaves", "3", "--norm-multi", "9"], cwd=str(tmp_path),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    lines = [l for l in p.stdout.splitlines() if l.startswith(("accept", "reject"))]
    assert p.returncode == 0 and len(lines) == len(ds[0]) and "Number of matches" not in p.stdout
