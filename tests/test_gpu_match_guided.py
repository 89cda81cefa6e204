"""GPU tests of guided matching (include/popsift_hip.h, "guided matching"): psx_match_guided / psx_match_guided_u8,
psx_match_pairs_guided* and their _dev forms, psx_desc_positions, FeaturesDev::matchPairsGuided and popsift-match's guide
options.  Expected values come from tests/guided_cases.py: the admissible relation from a numpy float32 restatement of
the rule, the directed results from the oracle restricted to each left descriptor's admissible rights, the pair lists from
the HOST join (capi.pairs_join) of the two expected directed results.  Records and distances are compared bit for bit:
indices, and distances as their 32-bit patterns."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch        # before the HIP library is loaded: torch brings a HIP runtime of its own and must initialise first (_dev forms)

from popsift_amd.synth import synth
from tests import guided_cases as gc
from tests.match_pairs_cases import RATIOS, directed, dist_as_int, planted, same_records

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MATCH = os.path.join(ROOT, "popsift_amd", "lib", "popsift-match")


def _bits(d):
    d = np.ascontiguousarray(d)
    return d.view(np.uint32) if d.dtype == np.float32 else d


def _same_directed(got, want):
    return (got[0].dtype == want[0].dtype and got[1].dtype == want[1].dtype and np.array_equal(got[0], want[0])
            and np.array_equal(_bits(got[1]), _bits(want[1])))


class _OnDevice:
    """two descriptor sets and their positions uploaded once; guided calls with any guide and options on them"""

    def __init__(self, capi, left, lxy, right, rxy):
        self.capi, self.L, self.bufs = capi, capi.lib(), []
        self.u8 = left.dtype == np.uint8
        self.left, self.right = np.ascontiguousarray(left).reshape(-1, 128), np.ascontiguousarray(right).reshape(-1, 128)
        self.lxy, self.rxy = np.ascontiguousarray(lxy, np.float32).reshape(-1, 2), np.ascontiguousarray(rxy, np.float32).reshape(-1, 2)
        self.pl, self.plx, self.pr, self.prx = capi._to_device(self.L, 0, [self.left, self.lxy, self.right, self.rxy], self.bufs)
        self.dtype = capi.PAIR_U8_DTYPE if self.u8 else capi.PAIR_DTYPE

    def directed(self, guide):
        fn = self.L.psx_match_guided_u8 if self.u8 else self.L.psx_match_guided
        mm = np.full((len(self.left), 3), -9, np.int32)
        dd = np.full((len(self.left), 2), -9, np.int32 if self.u8 else np.float32)
        rc = fn(0, self.pl, self.plx, len(self.left), self.pr, self.prx, len(self.right), C.byref(guide),
                mm.ctypes.data_as(C.c_void_p), dd.ctypes.data_as(C.c_void_p))
        assert rc == 0
        return mm, dd

    def pairs(self, guide, ratio, mutual, capacity=None):
        fn = self.L.psx_match_pairs_guided_u8 if self.u8 else self.L.psx_match_pairs_guided
        got = self.capi._pairs_call(self.capi._guided_fn(fn, self.plx, self.prx, guide), "guided pairs", 0, self.pl, len(self.left),
                                    self.pr, len(self.right), ratio, mutual, self.dtype, capacity)
        return got[0] if capacity is None else got

    def close(self):
        for p in self.bufs:
            self.L.psx_dev_free(0, p)
        self.bufs = []


def _on_device(capi, c):
    return _OnDevice(capi, c["left"], c["lxy"], c["right"], c["rxy"])


# ---- directed, bytes and floats, both guides ------------------------------------------------------------------------------
@pytest.mark.parametrize("guide", sorted(gc.GUIDES))
@pytest.mark.parametrize("nl,nr,seed", gc.SHAPES, ids=gc.SHAPE_IDS)
def test_directed_guided_equals_the_expectation(oracle, capi, nl, nr, seed, guide):
    """forward: psx_match_guided* against the oracle restricted to the admissible rights; backward (reachable through the
    cross-check only): the mutual list at ratio inf against the host join of the two expected directed results"""
    for u8 in (True, False):
        c = gc.case(oracle, seed, nl, nr, guide, u8)
        g = capi.Guide.make(c["kind"], c["m"], c["tol"])
        dev = _on_device(capi, c)
        try:
            got = dev.directed(g)
            assert _same_directed(got, (c["fm"], c["fd"])), (u8, np.nonzero((got[0] != c["fm"]).any(1))[0][:5])
            for ratio in (float("inf"), 0.8):
                want = capi.pairs_join(c["fm"], c["fd"], c["bm"], nr, ratio, True)
                assert same_records(dev.pairs(g, ratio, True), want), (u8, ratio)
        finally:
            dev.close()
    if nl and nr == 0:
        assert np.all(c["fm"] == 0) and np.all(np.isinf(c["fd"]))


# ---- an all-admitting guide: the unguided matchers ------------------------------------------------------------------------
def test_all_admitting_guide_equals_the_unguided_matchers(capi):
    """identity H with tol 1e30 admits every pair: psx_match_guided* equal psx_match / psx_match_u8 bit for bit and
    psx_match_pairs_guided* equal psx_match_pairs*, on planted(9, 2500, 2300) -- several workgroups, 36 ballot steps; ties
    the new kernels to the oracle-pinned matcher"""
    left, right = planted(9, 2500, 2300)
    rng = np.random.default_rng(77)
    lxy = rng.uniform(0, 2000, (2500, 2)).astype(np.float32)
    rxy = rng.uniform(0, 2000, (2300, 2)).astype(np.float32)
    g = capi.Guide.homography(gc.IDENTITY, 1e30)
    assert gc.restate(gc.HOMOGRAPHY, gc.IDENTITY, 1e30, lxy[:50], rxy).all()
    for u8 in (True, False):
        l, r = (left, right) if u8 else (left.astype(np.float32), right.astype(np.float32))
        dev = _OnDevice(capi, l, lxy, r, rxy)
        try:
            want = capi.match_u8(l, r) if u8 else capi.match(l, r)
            assert _same_directed(dev.directed(g), want), u8
            for ratio, mutual in ((0.8, True), (0.8, False), (float("inf"), True), (0.6, True)):
                want = capi.match_pairs_u8(l, r, ratio, mutual) if u8 else capi.match_pairs(l, r, ratio, mutual)
                got = dev.pairs(g, ratio, mutual)
                assert len(want) > 100 and same_records(got, want), (u8, ratio, mutual, len(got), len(want))
        finally:
            dev.close()


# ---- pairs ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("guide", sorted(gc.GUIDES))
@pytest.mark.parametrize("name", sorted(gc.NAMED))
def test_guided_pairs_equal_the_join_of_the_expectation(oracle, capi, name, guide):
    """every ratio, both flag values, bytes and floats.  With the asymmetric H an implementation that swaps the roles of
    the rule in the backward pass gives another list: the wrong-relation expectation is computed too and must differ."""
    nl, nr, seed = gc.NAMED[name]
    for u8 in (True, False):
        c = gc.case(oracle, seed, nl, nr, guide, u8)
        gc.premises(oracle, c, (name, guide, u8), admissible_counts=(guide == "homography"))
        g = capi.Guide.make(c["kind"], c["m"], c["tol"])
        dev = _on_device(capi, c)
        try:
            for ratio in RATIOS:
                for mutual in (False, True):
                    want = capi.pairs_join(c["fm"], c["fd"], c["bm"] if mutual else None, nr, ratio, mutual)
                    got = dev.pairs(g, ratio, mutual)
                    assert same_records(got, want), (u8, ratio, mutual, len(got), len(want))
            if guide == "homography":
                wm, wd = gc.wrong_backward(oracle, c, u8)
                wrong = capi.pairs_join(c["fm"], c["fd"], wm, nr, float("inf"), True)
                right = capi.pairs_join(c["fm"], c["fd"], c["bm"], nr, float("inf"), True)
                assert not same_records(wrong, right)
                assert same_records(dev.pairs(g, float("inf"), True), right)
        finally:
            dev.close()


def test_capacity_and_dev_forms(oracle, capi):
    """capacity count - 1 and 0 report the total and leave the bytes behind the capacity alone, in the host buffer and in a
    device buffer read back; the _dev forms equal the host forms (one shape: the join is the existing one)"""
    nl, nr, seed = gc.NAMED["300x257"]
    L = capi.lib()
    for u8 in (True, False):
        c = gc.case(oracle, seed, nl, nr, "homography", u8)
        g = capi.Guide.make(c["kind"], c["m"], c["tol"])
        dev = _on_device(capi, c)
        try:
            for ratio, mutual in ((float("inf"), False), (0.8, True)):
                full = dev.pairs(g, ratio, mutual)
                total = len(full)
                assert total > 5 and same_records(full, capi.pairs_join(c["fm"], c["fd"], c["bm"] if mutual else None, nr, ratio, mutual))
                o = capi.match_opts(ratio, mutual)
                host_fn = L.psx_match_pairs_guided_u8 if u8 else L.psx_match_pairs_guided
                for cap in (total - 1, 0, nl):
                    host = np.full(((cap + 2) * 4,), -7, np.int32).view(dev.dtype)
                    cnt = C.c_int(-1)
                    rc = host_fn(0, dev.pl, dev.plx, nl, dev.pr, dev.prx, nr, C.byref(g), C.byref(o),
                                 host.ctypes.data_as(C.c_void_p) if cap else None, cap, C.byref(cnt))
                    k = min(cap, total)
                    assert rc == 0 and cnt.value == total, cap
                    assert same_records(host[:k], full[:k]) and np.all(host[k:].view(np.int32) == -7), cap
                    dbuf = torch.full(((cap + 2) * 16,), 0xA5, dtype=torch.uint8, device="cuda")
                    torch.cuda.synchronize()
                    n = capi.match_pairs_guided_dev(dev.pl.value, dev.plx.value, nl, dev.pr.value, dev.prx.value, nr, g,
                                                    dbuf.data_ptr() if cap else 0, cap, ratio, mutual, u8=u8)
                    back = dbuf.cpu().numpy()
                    assert n == total, cap
                    assert same_records(back[:k * 16].view(dev.dtype), full[:k]) and np.all(back[k * 16:] == 0xA5), cap
                part, n = dev.pairs(g, ratio, mutual, capacity=total - 1)
                assert n == total and same_records(part, full[:total - 1])
        finally:
            dev.close()
    c = gc.case(oracle, seed, nl, nr, "homography", False)
    g = capi.Guide.make(c["kind"], c["m"], c["tol"])
    dd = capi.DeviceDescriptors(c["left"], xy=c["lxy"]), capi.DeviceDescriptors(c["right"], xy=c["rxy"])
    want = capi.match_pairs_guided(c["left"], c["lxy"], c["right"], c["rxy"], g, 0.8, True)
    assert len(want) > 5 and same_records(dd[0].match_pairs_guided(dd[1], g, 0.8, True), want)
    assert same_records(want, capi.pairs_join(c["fm"], c["fd"], c["bm"], nr, 0.8, True))
    dd[0].close(); dd[1].close()
    # the python wrappers of the directed forms
    assert _same_directed(capi.match_guided(c["left"], c["lxy"], c["right"], c["rxy"], g), (c["fm"], c["fd"]))
    cu = gc.case(oracle, seed, nl, nr, "homography", True)
    assert _same_directed(capi.match_guided_u8(cu["left"], cu["lxy"], cu["right"], cu["rxy"], g), (cu["fm"], cu["fd"]))
    assert same_records(capi.match_pairs_guided_u8(cu["left"], cu["lxy"], cu["right"], cu["rxy"], g, 0.8, True),
                        capi.pairs_join(cu["fm"], cu["fd"], cu["bm"], nr, 0.8, True))


# ---- positions --------------------------------------------------------------------------------------------------------------
def _desc_xy(feats, n_desc):
    """position of every descriptor from downloaded psx_feature records (desc_idx of each orientation)"""
    xy = np.full((n_desc, 2), np.nan, np.float32)
    for s in range(feats["desc_idx"].shape[1]):
        sel = feats["num_ori"] > s
        xy[feats["desc_idx"][sel, s]] = np.stack([feats["xpos"][sel], feats["ypos"][sel]], 1)
    assert not np.isnan(xy).any()
    return xy


def test_desc_positions_equal_the_host_gather(capi):
    """psx_desc_positions on a clone's device arrays equals features[reverse_map] of the downloaded clone, on an image whose
    keypoints have several orientations (some features own two or more descriptors)"""
    L = capi.lib()
    L.psx_dev_alloc.argtypes = [C.c_int, C.c_size_t, C.POINTER(C.c_void_p)]
    L.psx_dev_free.argtypes = [C.c_int, C.c_void_p]
    L.psx_dev_read.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]
    L.psx_clone_results.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    ctx = capi.Context(capi.default_config(octaves=4))
    ctx.upload(synth(640, 480, 4243))
    ctx.extract()
    ne, no = ctx.counts()
    feats_h, desc_h = ctx.download()
    assert no > ne > 500 and (feats_h["num_ori"] >= 2).sum() > 10
    ptrs = [C.c_void_p() for _ in range(4)]
    sizes = (ne * capi.FEATURE_DEV_DTYPE.itemsize, no * 512, no * 4, (no + 2) * 8)
    try:
        for p, n in zip(ptrs, sizes):
            assert L.psx_dev_alloc(0, n, C.byref(p)) == 0
        pf, pd, pr, pxy = ptrs
        ctx._chk(L.psx_clone_results(ctx._h, pf, pd, pr))
        sentinel = np.full((no + 2, 2), -77.0, np.float32)
        assert L.psx_dev_write(0, pxy, sentinel.ctypes.data_as(C.c_void_p), sentinel.nbytes) == 0
        capi.desc_positions(pf.value, pr.value, no, pxy.value)
        feats = np.zeros((ne,), capi.FEATURE_DEV_DTYPE)
        rev = np.zeros((no,), np.int32)
        xy = np.zeros((no + 2, 2), np.float32)
        for arr, p in ((feats, pf), (rev, pr), (xy, pxy)):
            assert L.psx_dev_read(0, arr.ctypes.data_as(C.c_void_p), p, arr.nbytes) == 0
    finally:
        for p in ptrs:
            if p:
                L.psx_dev_free(0, p)
        ctx.close()
    want = np.stack([feats["xpos"][rev], feats["ypos"][rev]], 1)
    assert np.array_equal(xy[:no].view(np.uint32), want.view(np.uint32)) and np.all(xy[no:] == -77.0)
    assert len(np.unique(rev)) < no                                       # some features own several descriptors
    assert np.array_equal(want.view(np.uint32), _desc_xy(feats_h, no).view(np.uint32))     # and the psx_feature records agree


# ---- real descriptors -------------------------------------------------------------------------------------------------------
def test_guided_pairs_on_real_descriptors(oracle, capi):
    """The two 640 x 480 views of test_pairs_on_real_descriptors (a shift by 3 px) under the guide "translation by 3, tol
    1.5": the guided mutual pairs equal the expectation; every pair satisfies the restated rule; and every pair of the
    UNGUIDED mutual list that satisfies the rule is in the guided list -- best among all is best among the admissible, and
    the second distance can only grow (the superset property)."""
    a = synth(640, 480, 4243)
    df, du, xy = [], [], []
    for img in (a, np.roll(a, 3, axis=1)):
        ctx = capi.Context(capi.default_config(octaves=4, sift_mode=2, norm_multi=9))
        ctx.set_descriptor_format(capi.DESCFMT_U8)
        ctx.upload(img)
        ctx.extract()
        fu, d8 = ctx.download_u8()
        ff, d32 = ctx.download()
        du.append(d8); df.append(d32)
        xy.append(_desc_xy(ff, len(d32)))
        ctx.close()
    assert len(df[0]) > 1000 and len(df[1]) > 1000
    m = np.array([1, 0, 3, 0, 1, 0, 0, 0, 1], np.float32)
    g = capi.Guide.homography(m, 1.5)
    A = gc.restate(gc.HOMOGRAPHY, m, 1.5, xy[0], xy[1])
    for u8, (l, r) in ((False, df), (True, du)):
        fm, fd = gc.expect_directed(oracle, l, r, A, u8)
        bm, bd = gc.expect_directed(oracle, r, l, A.T, u8)
        want = capi.pairs_join(fm, fd, bm, len(r), 0.8, True)
        fn = capi.match_pairs_guided_u8 if u8 else capi.match_pairs_guided
        got = fn(l, xy[0], r, xy[1], g, 0.8, True)
        plain = capi.match_pairs_u8(l, r, 0.8, True) if u8 else capi.match_pairs(l, r, 0.8, True)
        ok = A[plain["left"], plain["right"]]
        print("%s: %d guided pairs, %d unguided of which %d admissible, %d left descriptors"
              % ("bytes" if u8 else "float", len(got), len(plain), int(ok.sum()), len(l)))
        assert same_records(got, want)
        assert len(got) > 0 and A[got["left"], got["right"]].all()
        have = set(zip(got["left"].tolist(), got["right"].tolist()))
        assert ok.sum() > 100 and all((i, j) in have for i, j in zip(plain["left"][ok].tolist(), plain["right"][ok].tolist()))
        assert len(got) >= ok.sum()


# ---- the existing entry points, in the same process -------------------------------------------------------------------------
def test_existing_matchers_unchanged_beside_guided_calls(oracle, capi):
    """the existing directed matchers and psx_match_pairs before and after guided calls and across psx_match_release: the
    scratch they share with the guided entry points leaves their results as they were"""
    left, right = planted(9, 2500, 2300)
    fm, fd, bm, bd = directed(oracle, ("planted", 9, 2500, 2300, True), left, right, True)
    lf, rf = left.astype(np.float32), right.astype(np.float32)
    c = gc.case(oracle, 1, 300, 257, "homography", True)
    cf = gc.case(oracle, 1, 300, 257, "homography", False)
    g = capi.Guide.make(c["kind"], c["m"], c["tol"])
    want_pairs = capi.pairs_join(fm, fd, bm, len(right), 0.8, True)

    def existing():
        mg, dg = capi.match_u8(left, right)
        assert np.array_equal(mg, fm) and np.array_equal(dg, fd)
        mg, dg = capi.match(lf, rf)
        assert np.array_equal(mg, fm) and np.array_equal(dist_as_int(dg), fd)
        assert same_records(capi.match_pairs_u8(left, right, 0.8, True), want_pairs)
        assert np.array_equal(capi.match_pairs(lf, rf, 0.8, True)["right"], want_pairs["right"])

    def guided():
        assert _same_directed(capi.match_guided_u8(c["left"], c["lxy"], c["right"], c["rxy"], g), (c["fm"], c["fd"]))
        assert same_records(capi.match_pairs_guided(cf["left"], cf["lxy"], cf["right"], cf["rxy"], g, 0.8, True),
                            capi.pairs_join(cf["fm"], cf["fd"], cf["bm"], 257, 0.8, True))

    existing()
    guided()
    existing()
    assert capi.lib().psx_match_release() == 0
    guided()
    assert capi.lib().psx_match_release() == 0
    existing()
    guided()


# ---- C++ and the command line -------------------------------------------------------------------------------------------------
def test_cpp_match_guided_on_the_gpu(tmp_path):
    """tests/cpp/test_match_guided_api.cpp with POPSIFT_TEST_EXPECT_GPU: FeaturesDev::matchPairsGuided equals the C-ABI's
    guided pairs on the same device arrays (float and bytes, with and without the cross-check), every pair lies in the
    window, an invalid guide and a refused ratio throw"""
    libdir = os.path.join(ROOT, "popsift_amd", "lib")
    exe = str(tmp_path / "test_match_guided_api")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-pthread", os.path.join(ROOT, "tests", "cpp", "test_match_guided_api.cpp"), "-o", exe,
                           "-I", os.path.join(ROOT, "popsift_amd", "csrc", "include"), "-I", os.path.join(ROOT, "include"),
                           "-L", libdir, "-lpopsift", "-lpopsift_hip", "-Wl,-rpath," + libdir])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300,
                         env=dict(os.environ, POPSIFT_TEST_EXPECT_GPU="1"))
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout
    assert "float, mutual 1:" in out.stdout and "bytes, mutual 1:" in out.stdout


def _write_pgm(path, img):
    with open(path, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (img.shape[1], img.shape[0]) + img.tobytes())


def test_match_tool_guided_pairs(capi, tmp_path):
    """popsift-match --pairs FILE --homography ... --guide-tol ... (and --fundamental) writes a list whose count and sorted
    distances equal capi.match_pairs_guided on the same two images (descriptor order is not reproducible between runs);
    the usage errors are reported"""
    base = synth(336, 256, 77)
    a = np.ascontiguousarray(base[8:248, 8:328])
    b = np.ascontiguousarray(base[5:245, 3:323])                          # a point of a at (x, y) is at (x + 5, y + 3) in b
    _write_pgm(tmp_path / "l.pgm", a)
    _write_pgm(tmp_path / "r.pgm", b)
    ds, xy = [], []
    for img in (a, b):
        ctx = capi.Context(capi.default_config(octaves=3, norm_multi=9))
        ctx.upload(img)
        ctx.extract()
        f, d = ctx.download()
        ds.append(d); xy.append(_desc_xy(f, len(d)))
        ctx.close()
    hm = [1, 0, 5, 0, 1, 3, 0, 0, 1]
    fmat = [0, 0, 0, 0, 0, -1, 0, 1, 3]                                   # the line y' = y + 3
    text = lambda m: ",".join(str(v) for v in m)
    common = [MATCH, "-l", "l.pgm", "-r", "r.pgm", "--octaves", "3", "--norm-multi", "9"]
    for opts, g, ratio, mutual in ((["--homography", text(hm), "--guide-tol", "1.5", "--mutual"], capi.Guide.homography(hm, 1.5), 0.8, True),
                                   (["--fundamental=" + text(fmat), "--guide-tol=1", "--ratio", "0.7"], capi.Guide.epipolar(fmat, 1.0), 0.7, False)):
        out = tmp_path / "pairs.txt"
        p = subprocess.run(common + ["--pairs", str(out)] + opts, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           text=True, timeout=300)
        assert p.returncode == 0, p.stdout + p.stderr
        rows = [l.split() for l in out.read_text().splitlines()]
        want = capi.match_pairs_guided(ds[0], xy[0], ds[1], xy[1], g, ratio, mutual)
        plain = capi.match_pairs(ds[0], ds[1], ratio, mutual)
        assert "Number of matches: %d" % len(rows) in p.stdout and len(rows) == len(want) > 20
        assert sorted((r[4], r[5]) for r in rows) == sorted(("%.3f" % x, "%.3f" % y) for x, y in zip(want["d1"], want["d2"]))
        assert not same_records(want, plain)                               # the guide changes the list
    for extra, msg in ((["--homography", text(hm), "--guide-tol", "1.5"], "need '--pairs'"),
                       (["--pairs", "p.txt", "--homography", text(hm)], "need '--guide-tol'"),
                       (["--pairs", "p.txt", "--guide-tol", "2"], "needs '--homography' or '--fundamental'"),
                       (["--pairs", "p.txt", "--homography", text(hm), "--fundamental", text(fmat), "--guide-tol", "2"], "at most one")):
        p = subprocess.run(common + extra, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
        assert p.returncode != 0 and msg in p.stderr, (extra, p.stderr)
