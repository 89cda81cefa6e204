"""CPU tests of guided matching's host side (include/popsift_hip.h, "guided matching"): psx_guide_allows -- the rule the
kernels evaluate, sharing csrc/hip/guide_rule.h with them -- against an independent numpy float32 restatement
(tests/guided_cases.py) on the fixtures and on edge inputs; guide validation and argument errors with nothing touched; the
premises of the fixtures, from the oracle-derived expectation alone; the expectation helper against integer arithmetic;
the declarations and bindings; the C++ layer and popsift-match without a device; and a stand-alone sanitizer build of the
rule.

The premises.  Each named set (guided_cases.NAMED) under the homography guide -- the guide its canvas is sized for -- has a
left descriptor (1) without an admissible right, (2) with exactly one, (3) whose unguided best is inadmissible while the
guided best differs from it, (4) with an exact tie among admissible rights; and at ratio 0.8 with the cross-check (5) a pair
kept, (6) one dropped by the ratio, (7) one dropped by the cross-check alone.  Under the epipolar guide every line crosses
the canvas (it passes through H p), so every left point has tens of admissible rights: 3 to 7 are asserted there, 1 and 2
cannot hold for points that are uniform on the canvas."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import guided_cases as gc
from tests import rule_edge_cases as rc
from tests.match_pairs_cases import INT_MAX, dist_as_int

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _guide(capi, kind, m, tol):
    return capi.Guide.make(kind, m, tol)


@pytest.mark.parametrize("guide", sorted(gc.GUIDES))
@pytest.mark.parametrize("nl,nr,seed", gc.SHAPES, ids=gc.SHAPE_IDS)
def test_guide_allows_equals_the_restatement(capi, nl, nr, seed, guide):
    left, right, lxy, rxy = gc.positioned(seed, nl, nr)
    kind, m, tol = gc.GUIDES[guide]
    want = gc.restate(kind, m, tol, lxy, rxy)
    got = capi.guide_allows(_guide(capi, kind, m, tol), lxy, rxy)
    assert got.shape == want.shape == (nl, nr) and np.array_equal(got, want)
    # the relation is not symmetric in its roles: the backward pass is its transpose, not the rule with the roles swapped
    if guide == "homography" and min(nl, nr) >= 64:
        swapped = capi.guide_allows(_guide(capi, kind, m, tol), rxy, lxy)
        assert np.array_equal(swapped, gc.restate(kind, m, tol, rxy, lxy)) and not np.array_equal(swapped, want.T)


def test_guide_allows_on_edge_inputs(capi):
    lxy, rxy = rc.edge_points()                                           # the lists live in tests/rule_edge_cases.py: the GPU tests use them too
    guides = rc.edge_guides()
    seen = set()
    for kind, m, tol in guides:
        want = gc.restate(kind, m, tol, lxy, rxy)
        got = capi.guide_allows(_guide(capi, kind, m, tol), lxy, rxy)
        assert np.array_equal(got, want), (kind, list(m), tol)
        seen.add((bool(want.any()), bool((~want).any())))
    assert seen == {(True, True), (False, True)} or (True, False) in seen
    # identity H with tol 0 admits exactly the coinciding finite points; a huge tolerance everything finite
    ident0 = gc.restate(gc.HOMOGRAPHY, gc.IDENTITY, 0.0, lxy, rxy)
    assert ident0[10:20, :10].diagonal().all() and ident0.sum() >= 10 and not ident0[20:25].any()
    huge = gc.restate(gc.HOMOGRAPHY, gc.IDENTITY, 1e30, lxy, rxy)
    fin_l, fin_r = np.isfinite(lxy).all(1), np.isfinite(rxy).all(1)
    # (an infinite LEFT coordinate meets a zero of the matrix: NaN; an infinite right one only makes both sides +inf, and
    # inf <= inf holds: the IEEE result is the rule)
    assert huge[np.ix_(fin_l, fin_r)].all() and not huge[~fin_l].any() and not huge[:, np.isnan(rxy).any(1)].any()
    # NaN positions are inadmissible under every guide above
    for kind, m, tol in guides:
        got = capi.guide_allows(_guide(capi, kind, m, tol), lxy, rxy)
        assert not got[20:22].any() and not got[:, 30:32].any()


def test_guide_validation_leaves_everything_untouched(capi):
    L = capi.lib()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    lxy = np.array([[1, 2], [3, 4]], np.float32)
    rxy = np.array([[1, 2], [3, 4], [5, 6]], np.float32)
    nan, inf = float("nan"), float("inf")
    bad = [capi.Guide.make(0, gc.IDENTITY, 2.0), capi.Guide.make(3, gc.IDENTITY, 2.0), capi.Guide.make(-1, gc.IDENTITY, 2.0),
           capi.Guide.make(1, gc.IDENTITY, -1.0), capi.Guide.make(2, gc.IDENTITY, nan), capi.Guide.make(1, gc.IDENTITY, inf),
           capi.Guide.make(1, gc.IDENTITY, -inf)]
    for k in range(9):
        for v in (nan, inf, -inf):
            m = gc.IDENTITY.copy()
            m[k] = v
            bad.append(capi.Guide.make(1 + k % 2, m, 2.0))
    good = capi.Guide.homography(gc.IDENTITY, 0.0)
    out = np.full(6, 7, np.uint8)
    assert L.psx_guide_allows(C.byref(good), vp(lxy), 2, vp(rxy), 3, vp(out)) == 0 and list(out) == [1, 0, 0, 0, 1, 0]
    out[:] = 7
    mm, dd, n = np.full(6, -3, np.int32), np.full(4, -3, np.int32), C.c_int(-5)
    o = capi.match_opts(0.8, True)
    for g in bad + [None]:
        gp = C.byref(g) if g is not None else None
        assert L.psx_guide_allows(gp, vp(lxy), 2, vp(rxy), 3, vp(out)) == -1
        # the device entry points refuse the guide before they touch a device or an argument (the pointers are never read)
        assert L.psx_match_guided(0, vp(lxy), vp(lxy), 2, vp(rxy), vp(rxy), 3, gp, vp(mm), vp(dd)) == -1
        assert L.psx_match_guided_u8(0, vp(lxy), vp(lxy), 2, vp(rxy), vp(rxy), 3, gp, vp(mm), vp(dd)) == -1
        for name in ("psx_match_pairs_guided", "psx_match_pairs_guided_u8", "psx_match_pairs_guided_dev", "psx_match_pairs_guided_u8_dev"):
            assert getattr(L, name)(0, vp(lxy), vp(lxy), 2, vp(rxy), vp(rxy), 3, gp, C.byref(o), vp(mm), 1, C.byref(n)) == -1, name
            assert getattr(L, name)(0, None, None, 0, None, None, 0, gp, C.byref(o), None, 0, C.byref(n)) == -1, name
    # other argument errors of the host rule
    assert L.psx_guide_allows(C.byref(good), None, 2, vp(rxy), 3, vp(out)) == -1
    assert L.psx_guide_allows(C.byref(good), vp(lxy), 2, None, 3, vp(out)) == -1
    assert L.psx_guide_allows(C.byref(good), vp(lxy), 2, vp(rxy), 3, None) == -1
    assert L.psx_guide_allows(C.byref(good), vp(lxy), -1, vp(rxy), 3, vp(out)) == -1
    assert L.psx_guide_allows(C.byref(good), vp(lxy), 2, vp(rxy), -1, vp(out)) == -1
    # a NULL position array with a non-zero length, the other errors of psx_match_pairs, and the valid empty forms
    for name in ("psx_match_pairs_guided", "psx_match_pairs_guided_u8", "psx_match_pairs_guided_dev", "psx_match_pairs_guided_u8_dev"):
        fn = getattr(L, name)
        assert fn(0, vp(lxy), None, 2, vp(rxy), vp(rxy), 3, C.byref(good), C.byref(o), vp(mm), 1, C.byref(n)) == -1, name
        assert fn(0, vp(lxy), vp(lxy), 2, vp(rxy), None, 3, C.byref(good), C.byref(o), vp(mm), 1, C.byref(n)) == -1, name
        assert fn(0, None, vp(lxy), 2, vp(rxy), vp(rxy), 3, C.byref(good), C.byref(o), vp(mm), 1, C.byref(n)) == -1, name
        assert fn(0, None, None, 0, None, None, 0, C.byref(good), None, None, 0, C.byref(n)) == -1, name
        assert fn(0, None, None, 0, None, None, 0, C.byref(good), C.byref(o), None, 0, None) == -1, name
        assert fn(0, None, None, 0, None, None, 0, C.byref(good), C.byref(o), None, 4, C.byref(n)) == -1, name
        assert fn(0, None, None, -1, None, None, 0, C.byref(good), C.byref(o), None, 0, C.byref(n)) == -1, name
        assert fn(0, None, None, 0, None, None, 0, C.byref(good), C.byref(capi.MatchOpts(nan, 0)), None, 0, C.byref(n)) == -1, name
        assert fn(0, None, None, 0, None, None, 0, C.byref(good), C.byref(capi.MatchOpts(0.8, 2)), None, 0, C.byref(n)) == -1, name
        assert n.value == -5
        k = C.c_int(-5)
        assert fn(0, None, None, 0, None, None, 0, C.byref(good), C.byref(o), None, 0, C.byref(k)) == 0 and k.value == 0, name
    for name in ("psx_match_guided", "psx_match_guided_u8"):
        fn = getattr(L, name)
        assert fn(0, vp(lxy), None, 2, vp(rxy), vp(rxy), 3, C.byref(good), vp(mm), vp(dd)) == -1, name
        assert fn(0, vp(lxy), vp(lxy), 2, vp(rxy), None, 3, C.byref(good), vp(mm), vp(dd)) == -1, name
        assert fn(0, vp(lxy), vp(lxy), 2, vp(rxy), vp(rxy), 3, C.byref(good), None, vp(dd)) == -1, name
        assert fn(0, vp(lxy), vp(lxy), -2, vp(rxy), vp(rxy), 3, C.byref(good), vp(mm), vp(dd)) == -1, name
        assert fn(0, None, None, 0, vp(rxy), vp(rxy), 3, C.byref(good), None, None) == 0, name
    assert L.psx_desc_positions(0, None, None, 0, None) == 0 and L.psx_desc_positions(0, None, None, 3, None) == -1
    assert L.psx_desc_positions(0, None, None, -1, None) == -1
    assert np.all(out == 7) and np.all(mm == -3) and np.all(dd == -3) and n.value == -5            # nothing touched
    with pytest.raises(capi.PopSiftError):
        capi.guide_allows(bad[0], lxy, rxy)
    with pytest.raises(ValueError):
        capi.match_pairs_guided(np.zeros((2, 128), np.float32), lxy[:1], np.zeros((3, 128), np.float32), rxy, good)


@pytest.mark.parametrize("guide", sorted(gc.GUIDES))
@pytest.mark.parametrize("name", sorted(gc.NAMED))
def test_named_sets_meet_the_premises(oracle, name, guide):
    nl, nr, seed = gc.NAMED[name]
    for u8 in (True, False):
        c = gc.case(oracle, seed, nl, nr, guide, u8)
        got = gc.premises(oracle, c, (name, guide, u8), admissible_counts=(guide == "homography"))
        print(name, guide, "bytes" if u8 else "float", got)
        if guide == "homography":
            assert 1.0 <= got["mean_admissible"] <= 8.0
            # some planted partners are inadmissible (offset radius 2.5 and 6), others admissible
            assert 0 < got["lost"] < nl
    # the asymmetric H tells a role swap in the backward pass apart: the wrong relation gives another pair list
    c = gc.case(oracle, seed, nl, nr, "homography", True)
    wm, wd = gc.wrong_backward(oracle, c, True)
    assert not np.array_equal(wm[:, 0], c["bm"][:, 0])


@pytest.mark.parametrize("guide", sorted(gc.GUIDES))
@pytest.mark.parametrize("nl,nr,seed", gc.SHAPES, ids=gc.SHAPE_IDS)
def test_expected_bytes_equal_integer_arithmetic(oracle, nl, nr, seed, guide):
    """the oracle-derived expectation for bytes, both directions, against squared distances in numpy int64"""
    c = gc.case(oracle, seed, nl, nr, guide, True)
    for mm, dd, l, r, A in ((c["fm"], c["fd"], c["left"], c["right"], c["A"]), (c["bm"], c["bd"], c["right"], c["left"], c["A"].T)):
        wm, wd = gc.expect_bytes_int64(l, r, A)
        assert np.array_equal(mm, wm) and np.array_equal(dd, wd) and dd.dtype == np.int32
        cnt = A.sum(1)
        assert np.all(dd[cnt == 0] == INT_MAX) and np.all(mm[cnt == 0] == 0)
        assert np.all(dd[cnt == 1, 1] == INT_MAX) and np.all(mm[cnt == 1, 1] == 0) and np.all(mm[cnt == 1, 2] == 1)
        assert np.all(A[np.arange(len(mm))[cnt >= 1], mm[cnt >= 1, 0]]) and np.all(A[np.arange(len(mm))[cnt >= 2], mm[cnt >= 2, 1]])
    # floats of the same (byte-valued) sets: the same indices, the same distances
    f = gc.case(oracle, seed, nl, nr, guide, False)
    assert np.array_equal(f["fm"], c["fm"]) and f["fd"].dtype == np.float32
    assert np.array_equal(dist_as_int(f["fd"]), c["fd"])


def test_entry_points_declared_and_bound(capi):
    hdr = open(os.path.join(ROOT, "include", "popsift_hip.h")).read()
    for sym in ("psx_guide_allows", "psx_desc_positions", "psx_match_guided", "psx_match_guided_u8", "psx_match_pairs_guided",
                "psx_match_pairs_guided_u8", "psx_match_pairs_guided_dev", "psx_match_pairs_guided_u8_dev"):
        assert "int %s(" % sym in hdr and sym in capi.SYMBOLS and hasattr(capi.lib(), sym), sym
    assert "#define PSX_GUIDE_HOMOGRAPHY 1" in hdr and "#define PSX_GUIDE_EPIPOLAR   2" in hdr
    assert "typedef struct psx_guide { int kind; float m[9]; float tol; } psx_guide;" in hdr
    assert capi.GUIDE_HOMOGRAPHY == 1 and capi.GUIDE_EPIPOLAR == 2 and C.sizeof(capi.Guide) == 44
    for name in ("guide_allows", "desc_positions", "match_guided", "match_guided_u8", "match_pairs_guided", "match_pairs_guided_u8",
                 "match_pairs_guided_dev"):
        assert callable(getattr(capi, name)), name
    assert callable(capi.DeviceDescriptors.match_pairs_guided)
    # host and device share one header: the kernel and psx_guide_allows call its predicate; the build knows the new unit
    hip = os.path.join(ROOT, "popsift_amd", "csrc", "hip")
    assert "psx_guide_pair" in open(os.path.join(hip, "guide_rule.h")).read()
    src = open(os.path.join(hip, "match_guided.hip")).read()
    assert all(f in src for f in ("psx_guide_pair(", "psx_guide_left(", "psx_guide_right(")) and '#include "guide_rule.h"' in src and "fmaf" not in open(os.path.join(hip, "guide_rule.h")).read().split("#pragma once")[1]
    from popsift_amd import build
    assert "match_guided.hip" in build.HIP_SOURCES and "-ffp-contract=off" in build.HIP_FLAGS
    assert "match_guided" in open(os.path.join(ROOT, "CMakeLists.txt")).read()
    fh = open(os.path.join(ROOT, "popsift_amd", "csrc", "include", "popsift", "features.h")).read()
    assert "struct MatchGuide" in fh and "matchPairsGuided(" in fh


def test_cpp_match_guided_api(tmp_path):
    """tests/cpp/test_match_guided_api.cpp against libpopsift.so without a device: psx_guide's layout, MatchGuide's kinds,
    matchPairsGuided( nullptr ), objects on two devices and every kind of invalid guide throw; the C-ABI's argument checks"""
    libdir = os.path.join(ROOT, "popsift_amd", "lib")
    exe = str(tmp_path / "test_match_guided_api")
    cmd = ["g++", "-std=c++14", "-O1", "-pthread", os.path.join(ROOT, "tests", "cpp", "test_match_guided_api.cpp"), "-o", exe,
           "-I", os.path.join(ROOT, "popsift_amd", "csrc", "include"), "-I", os.path.join(ROOT, "include"),
           "-L", libdir, "-lpopsift", "-lpopsift_hip", "-Wl,-rpath," + libdir]
    subprocess.check_call(cmd)
    env = {k: v for k, v in os.environ.items() if k != "POPSIFT_TEST_EXPECT_GPU"}
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120, env=env)
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout


def test_match_tool_guide_usage_errors(tmp_path):
    """popsift-match: the guide options are valid only with --pairs, a matrix needs --guide-tol and the tolerance a matrix,
    at most one matrix -- usage errors that name the missing option, before any file or device is looked at"""
    tool = os.path.join(ROOT, "popsift_amd", "lib", "popsift-match")
    ident = "1,0,0,0,1,0,0,0,1"
    pairs = ["--pairs", str(tmp_path / "p.txt")]
    for extra, msg in ((["--homography", ident, "--guide-tol", "2"], "need '--pairs'"),
                       (["--fundamental", ident, "--guide-tol", "2"], "need '--pairs'"),
                       (pairs + ["--guide-tol", "2"], "needs '--homography' or '--fundamental'"),
                       (["--guide-tol", "2"], "needs '--homography' or '--fundamental'"),
                       (pairs + ["--homography", ident], "need '--guide-tol'"),
                       (pairs + ["--fundamental=" + ident], "need '--guide-tol'"),
                       (pairs + ["--homography", ident, "--fundamental", ident, "--guide-tol", "2"], "at most one"),
                       (pairs + ["--homography", "1,0,0,0,1,0,0,0", "--guide-tol", "2"], "nine numbers"),
                       (pairs + ["--homography", "1,0,0,0,1,0,0,0,x", "--guide-tol", "2"], "bad number"),
                       (pairs + ["--homography", ident, "--guide-tol", "-1"], "tolerance must be finite and not negative")):
        p = subprocess.run([tool, "-l", str(tmp_path / "a.pgm"), "-r", str(tmp_path / "b.pgm")] + extra,
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
        assert p.returncode != 0 and msg in p.stderr and "Allowed options" in p.stderr, (extra, p.stderr)
    p = subprocess.run([tool, "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert p.returncode == 0 and all(o in p.stdout for o in ("--homography arg", "--fundamental arg", "--guide-tol arg"))


def test_guide_rule_under_sanitizers(tmp_path):
    """tests/cpp/guide_rule_san.cpp: a stand-alone program (its own main) that includes guide_rule.h and checks the rule on
    2 x 256 pairs against values written out in the program, the edge inputs and the validation -- compiled with
    -ffp-contract=off -fsanitize=address,undefined and run directly."""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed"
    exe = str(tmp_path / "guide_rule_san")
    cmd = [cxx, "-std=c++14", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan",
           os.path.join(ROOT, "tests", "cpp", "guide_rule_san.cpp"), "-o", exe,
           "-I", os.path.join(ROOT, "popsift_amd", "csrc", "hip"), "-I", os.path.join(ROOT, "include")]
    subprocess.check_call(cmd)
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout
