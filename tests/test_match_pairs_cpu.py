"""CPU tests of the pair search's host side (include/popsift_hip.h, "matches as data"): psx_pairs_join / psx_pairs_join_u8
-- the join the device kernels compute, sharing csrc/hip/match_rule.h with them -- on the oracle's directed results both
ways, against an independent numpy restatement of the three conditions (tests/match_pairs_cases.py); counts and capacity;
every argument error; the refusal of out-of-range indices; the declarations and bindings; the C++ layer without a device;
and a stand-alone sanitizer build of the join."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.match_pairs_cases import (INT_MAX, RATIOS, SHAPES, SHAPE_IDS, assert_premise, directed, expect_records, planted,
                                     restate, same_records)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _case(oracle, nl, nr, seed, u8):
    left, right = planted(seed, nl, nr)
    return directed(oracle, ("planted", seed, nl, nr, u8), left, right, u8)


@pytest.mark.parametrize("u8", [True, False], ids=["bytes", "float"])
@pytest.mark.parametrize("nl,nr,seed", SHAPES, ids=SHAPE_IDS)
def test_join_equals_the_restatement(capi, oracle, nl, nr, seed, u8):
    fm, fd, bm, bd = _case(oracle, nl, nr, seed, u8)
    dtype = capi.PAIR_U8_DTYPE if u8 else capi.PAIR_DTYPE
    assert fd.dtype == (np.int32 if u8 else np.float32)
    if min(nl, nr) >= 64:
        assert_premise(fm, fd, bm, nr, (nl, nr))
    for ratio in RATIOS:
        for mutual in (False, True):
            kept, ok_ratio, ok_cross, _ = restate(fm, fd, bm, nr, ratio, mutual)
            want = expect_records(fm, fd, kept, dtype)
            got = capi.pairs_join(fm, fd, bm if mutual else None, nr, ratio, mutual)
            print("%d x %d %s ratio %s mutual %d: %d pairs (ratio passes %d, cross-check passes %d)"
                  % (nl, nr, "u8" if u8 else "f32", ratio, mutual, len(want), int(ok_ratio.sum()), int(ok_cross.sum())))
            assert same_records(got, want), (ratio, mutual)
            assert np.all(np.diff(got["left"]) > 0)                       # ascending left, each once
            if mutual:
                assert len(np.unique(got["right"])) == len(got)           # one-to-one
            if ratio == 0.8 and not mutual:
                assert np.array_equal(got["left"], np.nonzero(fm[:, 2] == 1)[0])      # the oracle's accept rows
    if nl == 0 or nr == 0:
        assert len(capi.pairs_join(fm, fd, bm, nr, float("inf"), True)) == 0


def test_planted_set_has_the_outcome_the_cases_rely_on(oracle):
    """300 x 257: ratio 1.0 keeps fewer rows than inf (the duplicated right row's quotient is exactly 1), 0.6 fewer than
    0.8, and the cross-check drops rows at every ratio"""
    fm, fd, bm, bd = _case(oracle, 300, 257, 1, True)
    n = {(r, m): len(restate(fm, fd, bm, 257, r, m)[0]) for r in RATIOS for m in (False, True)}
    print(n)
    inf = float("inf")
    assert 0 < n[(0.6, False)] < n[(0.8, False)] <= n[(1.0, False)] < n[(inf, False)] == 300
    for r in RATIOS:
        assert 0 < n[(r, True)] < n[(r, False)]
    d = np.where(fd == INT_MAX, np.inf, fd.astype(np.float64))
    assert (d[:, 0] == d[:, 1]).any()


def test_capacity_and_count(capi, oracle):
    fm, fd, bm, bd = _case(oracle, 300, 257, 1, True)
    full = capi.pairs_join(fm, fd, bm, 257, 0.8, True)
    total = len(full)
    assert total > 10
    L = capi.lib()
    o = capi.match_opts(0.8, True)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    for cap in (0, 1, total - 1, total, total + 3):
        buf = np.full((cap + 2,), -7, np.int32).astype(np.int32).repeat(4).view(capi.PAIR_U8_DTYPE)   # sentinels behind the capacity
        n = C.c_int(-1)
        rc = L.psx_pairs_join_u8(vp(fm), vp(fd), 300, vp(bm), 257, C.byref(o), vp(buf) if cap else None, cap, C.byref(n))
        assert rc == 0 and n.value == total, cap
        k = min(cap, total)
        assert same_records(buf[:k], full[:k])
        assert np.all(buf[k:].view(np.int32) == -7), cap
    # the python wrapper's form of the same
    part, n = capi.pairs_join(fm, fd, bm, 257, 0.8, True, capacity=total - 1)
    assert n == total and same_records(part, full[:total - 1])
    none, n = capi.pairs_join(fm, fd, bm, 257, 0.8, True, capacity=0)
    assert n == total and len(none) == 0


def test_argument_errors(capi):
    L = capi.lib()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    fm = np.array([[0, 1, 1], [1, 0, 1]], np.int32)
    bm = np.array([[0, 1, 1], [1, 0, 1]], np.int32)
    sentinel = np.full(8, -3, np.int32)
    for fn, fd in ((L.psx_pairs_join, np.array([[1, 4], [1, 4]], np.float32)), (L.psx_pairs_join_u8, np.array([[1, 4], [1, 4]], np.int32))):
        out = sentinel.copy()
        n = C.c_int(-5)
        good = capi.match_opts(0.8, True)
        assert fn(vp(fm), vp(fd), 2, vp(bm), 2, C.byref(good), vp(out), 2, C.byref(n)) == 0 and n.value == 2
        assert list(out[:8:4]) == [0, 1] and list(out[1:8:4]) == [0, 1]
        out = sentinel.copy()
        n = C.c_int(-5)
        nan, inf = float("nan"), float("inf")
        bad_opts = [capi.MatchOpts(nan, 0), capi.MatchOpts(0.0, 0), capi.MatchOpts(-0.5, 0), capi.MatchOpts(-inf, 0),
                    capi.MatchOpts(0.8, 2), capi.MatchOpts(0.8, 3), capi.MatchOpts(0.8, -1)]
        for o in bad_opts:
            assert fn(vp(fm), vp(fd), 2, vp(bm), 2, C.byref(o), vp(out), 2, C.byref(n)) == -1, (o.ratio, o.flags)
        assert fn(vp(fm), vp(fd), 2, vp(bm), 2, None, vp(out), 2, C.byref(n)) == -1             # opts == NULL
        assert fn(vp(fm), vp(fd), 2, vp(bm), 2, C.byref(good), vp(out), 2, None) == -1          # count == NULL
        assert fn(vp(fm), vp(fd), -1, vp(bm), 2, C.byref(good), vp(out), 2, C.byref(n)) == -1   # negative sizes
        assert fn(vp(fm), vp(fd), 2, vp(bm), -1, C.byref(good), vp(out), 2, C.byref(n)) == -1
        assert fn(vp(fm), vp(fd), 2, vp(bm), 2, C.byref(good), vp(out), -1, C.byref(n)) == -1
        assert fn(None, vp(fd), 2, vp(bm), 2, C.byref(good), vp(out), 2, C.byref(n)) == -1      # NULL data with a size
        assert fn(vp(fm), None, 2, vp(bm), 2, C.byref(good), vp(out), 2, C.byref(n)) == -1
        assert fn(vp(fm), vp(fd), 2, None, 2, C.byref(good), vp(out), 2, C.byref(n)) == -1      # mutual needs the backward side
        assert fn(vp(fm), vp(fd), 2, vp(bm), 2, C.byref(good), None, 2, C.byref(n)) == -1
        assert n.value == -5 and np.array_equal(out, sentinel)                                  # nothing touched
        # valid corner forms: inf as a ratio, no backward side without the flag, "how many?", empty sides
        plain = capi.match_opts(inf, False)
        assert fn(vp(fm), vp(fd), 2, None, 2, C.byref(plain), vp(out), 2, C.byref(n)) == 0 and n.value == 2
        assert fn(vp(fm), vp(fd), 2, None, 2, C.byref(plain), None, 0, C.byref(n)) == 0 and n.value == 2
        n = C.c_int(-5)
        assert fn(None, None, 0, vp(bm), 2, C.byref(good), None, 0, C.byref(n)) == 0 and n.value == 0
        n = C.c_int(-5)
        assert fn(vp(fm), vp(fd), 2, None, 0, C.byref(good), None, 0, C.byref(n)) == 0 and n.value == 0
    o = capi.MatchOpts(0.0, 9)
    assert L.psx_match_opts_default(C.byref(o)) == 0 and o.ratio == np.float32(0.8) and o.flags == 0
    assert L.psx_match_opts_default(None) == -1
    # the device entry points check their arguments before they touch a device
    n = C.c_int(-5)
    good = capi.match_opts()
    for name in ("psx_match_pairs", "psx_match_pairs_u8", "psx_match_pairs_dev", "psx_match_pairs_u8_dev"):
        fn = getattr(L, name)
        assert fn(0, None, 0, None, 0, C.byref(good), None, 0, C.byref(n)) == 0 and n.value == 0, name
        n = C.c_int(-5)
        assert fn(0, None, 0, None, 0, None, None, 0, C.byref(n)) == -1, name
        assert fn(0, None, 0, None, 0, C.byref(good), None, 0, None) == -1, name
        assert fn(0, None, 3, None, 0, C.byref(good), None, 0, C.byref(n)) == -1, name
        assert fn(0, None, 0, None, 3, C.byref(good), None, 0, C.byref(n)) == -1, name
        assert fn(0, None, -1, None, 0, C.byref(good), None, 0, C.byref(n)) == -1, name
        assert fn(0, None, 0, None, 0, C.byref(good), None, 4, C.byref(n)) == -1, name
        assert fn(0, None, 0, None, 0, C.byref(capi.MatchOpts(float("nan"), 0)), None, 0, C.byref(n)) == -1, name
        assert fn(0, None, 0, None, 0, C.byref(capi.MatchOpts(0.8, 4)), None, 0, C.byref(n)) == -1, name
        assert n.value == -5
    with pytest.raises(TypeError):
        capi.pairs_join(fm, np.zeros((2, 2), np.float64), bm, 2)
    with pytest.raises(ValueError):
        capi.pairs_join(fm, np.zeros((3, 2), np.float32), bm, 2)
    with pytest.raises(ValueError):
        capi.pairs_join(fm, np.zeros((2, 2), np.float32), bm, 5, mutual=True)


def test_out_of_range_indices_are_refused(capi):
    """a best index outside [0, r_len), or a backward best outside [0, l_len): PSX_ERR_INVALID, nothing written"""
    fd = np.tile(np.array([1, 4], np.int32), (4, 1))
    for bad in (-1, 3, 2 ** 31 - 1, -2 ** 31):
        fm = np.array([[0, 1, 1], [1, 0, 1], [2, 0, 1], [0, 0, 1]], np.int32)
        bm = np.array([[0, 1, 1], [1, 0, 1], [2, 0, 1]], np.int32)
        fm[2, 0] = bad
        with pytest.raises(capi.PopSiftError):
            capi.pairs_join(fm, fd, None, 3, 0.8, False)
        with pytest.raises(capi.PopSiftError):
            capi.pairs_join(fm, fd.astype(np.float32), bm, 3, 0.8, True)
    for bad in (-1, 4, 2 ** 31 - 1):
        fm = np.array([[0, 1, 1], [1, 0, 1], [2, 0, 1], [0, 0, 1]], np.int32)
        bm = np.array([[0, 1, 1], [1, 0, 1], [bad, 0, 1]], np.int32)
        with pytest.raises(capi.PopSiftError):
            capi.pairs_join(fm, fd, bm, 3, 0.8, True)
        # the backward side is not looked at without the flag
        assert len(capi.pairs_join(fm, fd, bm, 3, 0.8, False)) == 4
    # the SECOND-best index is not part of the rule and is not checked
    fm = np.array([[0, 99, 1], [1, -5, 1]], np.int32)
    assert len(capi.pairs_join(fm, fd[:2], None, 3, 0.8, False)) == 2


def test_entry_points_declared_and_bound(capi):
    hdr = open(os.path.join(ROOT, "include", "popsift_hip.h")).read()
    for sym in ("psx_match_opts_default", "psx_match_pairs", "psx_match_pairs_u8", "psx_match_pairs_dev", "psx_match_pairs_u8_dev",
                "psx_pairs_join", "psx_pairs_join_u8"):
        assert "int %s(" % sym in hdr and sym in capi.SYMBOLS and hasattr(capi.lib(), sym), sym
    assert "#define PSX_PAIRS_MUTUAL 1" in hdr and capi.PAIRS_MUTUAL == 1
    assert capi.PAIR_DTYPE.itemsize == 16 and capi.PAIR_U8_DTYPE.itemsize == 16 and C.sizeof(capi.MatchOpts) == 8
    assert capi.PAIR_DTYPE.names == capi.PAIR_U8_DTYPE.names == ("left", "right", "d1", "d2")
    for name in ("match_pairs", "match_pairs_u8", "pairs_join", "match_pairs_dev"):
        assert callable(getattr(capi, name)), name
    assert callable(capi.DeviceDescriptors.match_pairs)
    # the flat C binding has no FeaturesDev and stays as it is
    assert "pairs" not in open(os.path.join(ROOT, "include", "popsift_c.h")).read().lower()
    # host and device share one header: the join kernels and the host join call its predicate
    hip = os.path.join(ROOT, "popsift_amd", "csrc", "hip")
    assert "psx_match_keep" in open(os.path.join(hip, "match_rule.h")).read()
    assert "psx_match_keep" in open(os.path.join(hip, "match_join.h")).read()
    src = open(os.path.join(hip, "match.hip")).read()
    assert "psx_match_keep" in src and "psx_pairs_join_host" in src
    fh = open(os.path.join(ROOT, "popsift_amd", "csrc", "include", "popsift", "features.h")).read()
    assert "struct MatchOptions" in fh and "struct Match" in fh and "matchPairs(" in fh


def test_cpp_match_pairs_api(tmp_path):
    """tests/cpp/test_match_pairs_api.cpp against libpopsift.so, built and run the way test_mask_api.cpp is: the record
    layouts, MatchOptions' defaults, matchPairs( nullptr ) and objects on two devices throw -- no device is touched."""
    libdir = os.path.join(ROOT, "popsift_amd", "lib")
    if not os.path.exists(os.path.join(libdir, "libpopsift.so")):
        from popsift_amd import build
        build.build_all()
    exe = str(tmp_path / "test_match_pairs_api")
    cmd = ["g++", "-std=c++14", "-O1", "-pthread", os.path.join(ROOT, "tests", "cpp", "test_match_pairs_api.cpp"), "-o", exe,
           "-I", os.path.join(ROOT, "popsift_amd", "csrc", "include"), "-I", os.path.join(ROOT, "include"),
           "-L", libdir, "-lpopsift", "-lpopsift_hip", "-Wl,-rpath," + libdir]
    subprocess.check_call(cmd)
    env = {k: v for k, v in os.environ.items() if k != "POPSIFT_TEST_EXPECT_GPU"}
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120, env=env)
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout


def test_match_tool_refuses_refinements_without_pairs(tmp_path):
    """popsift-match: --ratio / --mutual without --pairs is a usage error, before any file or device is looked at"""
    tool = os.path.join(ROOT, "popsift_amd", "lib", "popsift-match")
    for extra in (["--ratio", "0.7"], ["--mutual"], ["--ratio=0.7", "--mutual"]):
        p = subprocess.run([tool, "-l", str(tmp_path / "a.pgm"), "-r", str(tmp_path / "b.pgm")] + extra,
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
        assert p.returncode != 0 and "need '--pairs'" in p.stderr and "Allowed options" in p.stderr, (extra, p.stderr)
    p = subprocess.run([tool, "-l", "a", "-r", "b", "--pairs", str(tmp_path / "p.txt"), "--ratio", "-1"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert p.returncode != 0 and "ratio must be positive" in p.stderr
    p = subprocess.run([tool, "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert p.returncode == 0 and all(o in p.stdout for o in ("--pairs arg", "--ratio arg", "--mutual"))


def test_host_join_under_sanitizers(tmp_path):
    """tests/cpp/match_join_san.cpp: a stand-alone program (its own main) that includes match_rule.h and drives the host join
    on crafted rows -- NaN, +inf, INT_MAX, ties, every capacity, out-of-range indices -- compiled with
    -fsanitize=address,undefined and run directly."""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed"
    exe = str(tmp_path / "match_join_san")
    # the runtimes linked statically: the program runs as it is, whatever else the environment loads into a process
    cmd = [cxx, "-std=c++14", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           "-static-libasan", "-static-libubsan",
           os.path.join(ROOT, "tests", "cpp", "match_join_san.cpp"), "-o", exe,
           "-I", os.path.join(ROOT, "popsift_amd", "csrc", "hip"), "-I", os.path.join(ROOT, "include")]
    subprocess.check_call(cmd)
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout
