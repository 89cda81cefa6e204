"""CPU tests of the guided re-match of many sets (include/popsift_hip.h, "guided re-match of many sets in one call"): the
declarations and bindings; every argument error, before a device is looked at and with the outputs untouched -- an
invalid guide in the LAST set included --; the empty and all-skipped forms; psx_guides_from_ransac; the premises of the
generator the GPU tests run on (tests/guided_many_cases.py); and FeaturesDev::matchPairsGuidedMany's throws."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests.guided_many_cases import CASES, CASE_IDS, NONE, capi_guide, expected, guide_of, positioned_many, premises, tiny_guided
from tests.match_many_cases import TINY_LENS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_MAX = 2 ** 31 - 1
ENTRIES = ("psx_match_pairs_guided_many_u8", "psx_match_pairs_guided_many_u8_dev")
IDENT = (1, 0, 0, 0, 1, 0, 0, 0, 1)


def test_entry_points_declared_and_bound(capi):
    hdr = open(os.path.join(ROOT, "include", "popsift_hip.h")).read()
    for sym in ENTRIES + ("psx_guides_from_ransac",):
        assert "int %s(" % sym in hdr and sym in capi.SYMBOLS and hasattr(capi.lib(), sym), sym
    assert "#define PSX_GUIDE_NONE 0" in hdr and capi.GUIDE_NONE == 0 and capi.Guide.none().kind == 0
    assert hdr.index("typedef struct psx_ransac_result") < hdr.index("int psx_guides_from_ransac(")
    for name in ("match_pairs_guided_many_u8", "match_pairs_guided_many_dev", "guides_from_ransac"):
        assert callable(getattr(capi, name)), name
    from popsift_amd import build
    assert "match_guided_many.hip" in build.HIP_SOURCES
    assert " match_guided_many " in open(os.path.join(ROOT, "CMakeLists.txt")).read()
    hip = os.path.join(ROOT, "popsift_amd", "csrc", "hip")
    src = open(os.path.join(hip, "match_guided_many.hip")).read()
    many = open(os.path.join(hip, "match_many.hip")).read()
    # the segmented join is stated once, in a header its users include
    assert '#include "match_many_join.h"' in many and "void k_many_count(" not in many and "void k_many_write(" not in many
    # the star form is an adapter: no device code and no launch of its own; it hands the star to the edge list's driver
    for piece in ("__global__", "__device__", "__ballot", "atomic", "hipLaunchKernelGGL", "<<<", "match_many_join.h", "match_guided_core.h",
                  "g_match_row"):
        assert piece not in src, piece
    assert "psx_guided_edges_run(" in src and "psx_view_edge{0, k + 1}" in src
    # the wave's search is stated once, in the header the single call and the batched driver include
    graph = open(os.path.join(hip, "match_guided_graph.hip")).read()
    single = open(os.path.join(hip, "match_guided.hip")).read()
    for text in (graph, single):
        assert '#include "match_guided_core.h"' in text
    assert "__ballot" not in single
    for piece in ("g_match_row<unsigned char, int, false>(", "g_match_row<unsigned char, int, true>(", "int psx_guided_edges_run("):
        assert graph.count(piece) == 1, piece
    assert "atomic" not in graph.split("#include")[-1]      # the code: nothing in the ranking depends on arrival order
    fh = open(os.path.join(ROOT, "popsift_amd", "csrc", "include", "popsift", "features.h")).read()
    assert "matchPairsGuidedMany(" in fh and "MatchGuide none()" in fh


def _guides(capi, *gs):
    return (capi.Guide * max(len(gs), 1))(*gs)


def test_argument_errors_touch_nothing(capi):
    """every PSX_ERR_INVALID of the header, with sentinels in every output; the pointers are never dereferenced (they
    are not device memory: this runs without a GPU)"""
    L = capi.lib()
    good = capi.match_opts(0.8, True)
    fake = 0x1000                                            # a non-NULL "device pointer": an error return may not touch it
    win = capi.Guide.homography(IDENT, 2.0)
    epi = capi.Guide.epipolar((0, 0, 0, 0, 0, -1, 0, 1, 0), 1.0)
    nan, inf = float("nan"), float("inf")
    for name in ENTRIES:
        fn = getattr(L, name)

        def call(left=fake, lxy=fake, l_len=4, ptrs=(fake, fake), xys=(fake, fake), lens=(3, 5), n_sets=2, guides=(win, epi), opts=good,
                 out=True, cap=2, counts=True, count=True):
            pa = (C.c_void_p * max(len(ptrs), 1))(*ptrs) if ptrs is not None else None
            xa = (C.c_void_p * max(len(xys), 1))(*xys) if xys is not None else None
            la = np.array(lens, np.int32) if lens is not None else None
            ga = _guides(capi, *guides) if guides is not None else None
            buf = np.full(16, -7, np.int32)
            sc = np.full(8, -9, np.int32)
            n = C.c_int(-5)
            rc = fn(0, left, lxy, l_len, pa, xa, la.ctypes.data_as(C.c_void_p) if la is not None else None, n_sets, ga,
                    C.byref(opts) if opts is not None else None, buf.ctypes.data_as(C.c_void_p) if out else None, cap,
                    sc.ctypes.data_as(C.c_void_p) if counts else None, C.byref(n) if count else None)
            assert np.all(buf == -7) and np.all(sc == -9) and n.value == -5, name
            return rc

        # everything psx_match_pairs_guided_u8 and psx_match_pairs_many_u8 refuse
        for o in (capi.MatchOpts(nan, 0), capi.MatchOpts(0.0, 0), capi.MatchOpts(-0.5, 0), capi.MatchOpts(-inf, 0),
                  capi.MatchOpts(0.8, 2), capi.MatchOpts(0.8, -1)):
            assert call(opts=o) == -1, (name, o.ratio, o.flags)
        assert call(opts=None) == -1
        assert call(count=False) == -1
        assert call(l_len=-1) == -1
        assert call(cap=-1) == -1
        assert call(out=False, cap=2) == -1                  # a capacity without a buffer
        assert call(left=None) == -1                         # NULL left descriptors with a length
        assert call(lxy=None) == -1                          # NULL left positions with a length
        assert call(n_sets=-1) == -1
        assert call(ptrs=None) == -1
        assert call(xys=None) == -1
        assert call(lens=None) == -1
        assert call(guides=None) == -1
        assert call(counts=False) == -1
        assert call(lens=(3, -1)) == -1
        assert call(ptrs=(fake, None)) == -1                 # NULL descriptors of a set that is not skipped and has rows
        assert call(xys=(fake, None)) == -1                  # NULL positions of such a set
        assert call(xys=(None, fake)) == -1
        assert call(l_len=2 ** 30, lens=(3, 5, 1), ptrs=(fake,) * 3, xys=(fake,) * 3, guides=(win,) * 3, n_sets=3) == -1    # n_sets * l_len
        assert call(lens=(INT_MAX, 1)) == -1                 # the sum of r_lens above INT_MAX
        # every guide is checked, the last one too, and also the guide of an EMPTY set
        for bad in (capi.Guide.make(3, IDENT, 2.0), capi.Guide.make(-1, IDENT, 2.0), capi.Guide.homography(IDENT, -1.0),
                    capi.Guide.homography(IDENT, inf), capi.Guide.homography(IDENT, nan), capi.Guide.epipolar((nan,) + IDENT[1:], 2.0),
                    capi.Guide.homography(IDENT[:8] + (inf,), 2.0)):
            assert call(guides=(win, bad)) == -1, (name, bad.kind, bad.tol)
            assert call(guides=(bad, win)) == -1
            assert call(guides=(win, bad), lens=(3, 0), ptrs=(fake, None), xys=(fake, None)) == -1
            assert call(guides=(capi.Guide.none(), bad), ptrs=(None, fake), xys=(None, fake)) == -1
    # the single-set calls keep refusing kind 0
    n = C.c_int(-5)
    for name in ("psx_match_pairs_guided_u8", "psx_match_pairs_guided_u8_dev"):
        none = capi.Guide.none()
        assert getattr(L, name)(0, fake, fake, 4, fake, fake, 3, C.byref(none), C.byref(good), None, 0, C.byref(n)) == -1 and n.value == -5


def test_empty_and_skipped_forms_need_no_device(capi):
    """n_sets = 0, l_len = 0, all sets empty, all sets of kind 0 with NULL arrays: PSX_OK, zero counts, nothing else
    written -- no pair can exist, so no device is touched (this runs without one)"""
    L = capi.lib()
    good = capi.match_opts(0.8, True)
    fake = 0x1000
    win, none = capi.Guide.homography(IDENT, 2.0), capi.Guide.none()
    # a skipped set's guide is not looked at beyond its kind
    odd = capi.Guide.make(0, (float("nan"),) * 9, -3.0)
    for name in ENTRIES:
        fn = getattr(L, name)
        n = C.c_int(-5)
        assert fn(0, None, None, 0, None, None, None, 0, None, C.byref(good), None, 0, None, C.byref(n)) == 0 and n.value == 0, name
        n = C.c_int(-5)
        assert fn(0, fake, fake, 7, None, None, None, 0, None, C.byref(good), None, 0, None, C.byref(n)) == 0 and n.value == 0, name
        for l_ptr, l_len, lens, ptrs, guides in ((None, 0, (3, 5, 0), (fake, fake, None), (win, win, win)),
                                                 (fake, 9, (0, 0, 0), (None, fake, None), (win, none, win)),
                                                 (fake, 9, (4, 1000, 0), (None, None, None), (none, odd, none))):
            pa, xa = (C.c_void_p * 3)(*ptrs), (C.c_void_p * 3)(*ptrs)
            la = np.array(lens, np.int32)
            sc = np.full(5, -9, np.int32)
            buf = np.full(16, -7, np.int32)
            n = C.c_int(-5)
            rc = fn(0, l_ptr, l_ptr, l_len, pa, xa, la.ctypes.data_as(C.c_void_p), 3, _guides(capi, *guides), C.byref(good),
                    buf.ctypes.data_as(C.c_void_p), 4, sc.ctypes.data_as(C.c_void_p), C.byref(n))
            assert rc == 0 and n.value == 0 and list(sc) == [0, 0, 0, -9, -9] and np.all(buf == -7), (name, lens)
    # the python wrapper's form of the same (arrays without rows, or None for a skipped set: nothing to upload)
    e, exy = np.zeros((0, 128), np.uint8), np.zeros((0, 2), np.float32)
    lists, counts = capi.match_pairs_guided_many_u8(e, exy, [e, e], [exy, exy], [win, win])
    assert [len(p) for p in lists] == [0, 0] and list(counts) == [0, 0]
    lists, counts = capi.match_pairs_guided_many_u8(e, exy, [None, None], [None, None], [none, None])
    assert [len(p) for p in lists] == [0, 0] and list(counts) == [0, 0]
    lists, counts = capi.match_pairs_guided_many_u8(e, exy, [], [], [])
    assert lists == [] and len(counts) == 0


def test_guides_from_ransac(capi):
    """best = -1 gives kind 0; the matrix and tol are carried over; the argument errors are reported, nothing written"""
    L = capi.lib()
    m = tuple(float(v) for v in np.arange(1, 10) * 0.5)
    res = [capi.RansacResult((C.c_float * 9)(*m), 17, 40, 42, 1), capi.RansacResult((C.c_float * 9)(*([0.0] * 9)), -1, 0, 0, 0),
           capi.RansacResult((C.c_float * 9)(*m[::-1]), 0, 4, 4, 0)]
    for kind in (capi.GUIDE_HOMOGRAPHY, capi.GUIDE_EPIPOLAR):
        gs = capi.guides_from_ransac(res, kind, 2.5)
        assert [g.kind for g in gs] == [kind, capi.GUIDE_NONE, kind]
        assert tuple(gs[0].m) == m and tuple(gs[2].m) == m[::-1] and tuple(gs[1].m) == (0.0,) * 9
        assert all(g.tol == 2.5 for g in gs)
    assert capi.guides_from_ransac([], capi.GUIDE_HOMOGRAPHY, 0.0) == []
    ra = (capi.RansacResult * 3)(*res)
    for n_sets, r, kind, tol, out in ((-1, True, 1, 2.0, True), (3, False, 1, 2.0, True), (3, True, 1, 2.0, False), (3, True, 0, 2.0, True),
                                      (3, True, 3, 2.0, True), (3, True, 1, -1.0, True), (3, True, 2, float("inf"), True),
                                      (3, True, 2, float("nan"), True)):
        ga = (capi.Guide * 3)(*[capi.Guide.make(7, IDENT, 9.0)] * 3)
        assert L.psx_guides_from_ransac(ra if r else None, n_sets, kind, tol, ga if out else None) == -1, (n_sets, r, kind, tol, out)
        assert all(g.kind == 7 and g.tol == 9.0 for g in ga)
    assert L.psx_guides_from_ransac(None, 0, 1, 2.0, None) == 0


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_generator_premises(capi, case):
    """what the GPU tests rest on: per homography-guided set with min(nl, nr) >= 64 a left row with no and with exactly one
    admissible right, an unguided best that the guide excludes, a pair kept, one dropped by the ratio and one by the
    cross-check alone; set k under a neighbour's guide gives ANOTHER list (a wrong table index cannot pass); roles swapped
    in the backward pass give another list under the asymmetric H"""
    seed, nl, nrs = case
    left, rights, lxy, rxys = positioned_many(*case)
    assert len(left) == len(lxy) == nl and [len(r) for r in rights] == [len(x) for x in rxys] == list(nrs)
    seen = premises(capi, case)
    print("seed %d: %s" % (seed, seen))
    if seed == 31:
        assert seen["homography"] == 3 and seen["backward"] == 3 and seen["swap"] >= 8
    if seed == 32:
        assert seen["homography"] == 1 and seen["swap"] == 4
    for k in range(len(nrs)):
        if guide_of(k)[0] == NONE:
            assert len(expected(capi, case, k, float("inf"), False)) == 0
    # the all-admitting guide admits everything: its expectation is the unguided host join
    if seed == 32:
        from tests.guided_cases import expect_bytes_int64
        every = np.ones((nl, nrs[2]), bool)
        fm, fd = expect_bytes_int64(left, rights[2], every)
        bm, _ = expect_bytes_int64(rights[2], left, every.T)
        want = capi.pairs_join(fm, fd, bm, nrs[2], 0.8, True)
        assert len(want) > 10 and expected(capi, case, 2, 0.8, True).tobytes() == want.tobytes()


def test_tiny_sets_generator(capi):
    left, rights, lxy, rxys, guides = tiny_guided()
    assert [len(r) for r in rights] == [len(x) for x in rxys] == list(TINY_LENS) and len(guides) == 200
    assert sum(g[0] == NONE for g in guides) == 40
    for k, (g, r, x) in enumerate(zip(guides, rights, rxys)):
        if g[0] != NONE and len(r):
            assert capi.guide_allows(capi_guide(capi, g), lxy[k % 70][None], x[k % len(r)][None])[0, 0], k


def test_cpp_match_guided_many_api(tmp_path):
    """tests/cpp/test_match_guided_many_api.cpp against libpopsift.so, built and run the way test_match_many_api.cpp is:
    matchPairsGuidedMany throws for a null entry, an object on another device, float descriptors, a guide count that differs
    and an invalid guide, and returns empty lists for empty objects and skipped sets -- no device is touched."""
    libdir = os.path.join(ROOT, "popsift_amd", "lib")
    if not os.path.exists(os.path.join(libdir, "libpopsift.so")):
        from popsift_amd import build
        build.build_all()
    exe = str(tmp_path / "test_match_guided_many_api")
    cmd = ["g++", "-std=c++14", "-O1", "-pthread", os.path.join(ROOT, "tests", "cpp", "test_match_guided_many_api.cpp"), "-o", exe,
           "-I", os.path.join(ROOT, "popsift_amd", "csrc", "include"), "-I", os.path.join(ROOT, "include"),
           "-L", libdir, "-lpopsift", "-lpopsift_hip", "-Wl,-rpath," + libdir]
    subprocess.check_call(cmd)
    env = {k: v for k, v in os.environ.items() if k != "POPSIFT_TEST_EXPECT_GPU"}
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120, env=env)
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout
