"""CPU tests of the one-to-many FLOAT pair search's host side (include/popsift_hip.h, "one descriptor set against many, float
descriptors"): the declarations and bindings; every argument error, before a device is looked at and with the outputs
untouched; the empty forms; the invariants of the plan (psx_match_many_f32_plan, csrc/hip/match_many_f32_plan.h) on the
cases the GPU tests run; a stand-alone sanitizer build of the plan; the premise of the planted sets in both flavours and the
contract's restatement on the oracle's results, which the GPU tests reuse."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.match_many_cases import TINY_LENS, contract, slices
from tests.match_many_f32_cases import CASES, CASE_IDS, FLAVOURS, ORACLE_SEEDS, planned_path, planted_many_f32
from tests.match_pairs_cases import assert_premise, directed, same_records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_MAX = 2 ** 31 - 1
BUDGET = 256 << 20
ENTRIES = ("psx_match_pairs_many", "psx_match_pairs_many_dev")
PLAN_SHAPES = [(c[1], c[2]) for c in CASES] + [(70, TINY_LENS + (4100,)), (2048, (2048,) * 64), (18432, (18432,))]
PLAN_IDS = CASE_IDS + ["tiny200+4100", "64x2048", "1x18432"]


def test_entry_points_declared_and_bound(capi):
    hdr = open(os.path.join(ROOT, "include", "popsift_hip.h")).read()
    for sym in ENTRIES + ("psx_match_many_f32_plan", "psx_match_many_f32_last"):
        assert "int %s(" % sym in hdr and sym in capi.SYMBOLS and hasattr(capi.lib(), sym), sym
    assert "typedef struct psx_many_f32_info { int path, fell_back, launches, syncs; } psx_many_f32_info;" in hdr
    assert "typedef struct psx_many_f32_plan { int path;" in hdr and "Only the byte form exists. */\nint psx_match_pairs_many_u8" not in hdr
    for name in ("match_pairs_many", "match_pairs_many_dev", "match_many_f32_plan", "match_many_f32_last"):
        assert callable(getattr(capi, name)), name
    from popsift_amd import build
    assert "match_many_f32.hip" in build.HIP_SOURCES
    assert " match_many_f32 " in open(os.path.join(ROOT, "CMakeLists.txt")).read()
    hip = os.path.join(ROOT, "popsift_amd", "csrc", "hip")
    plan = open(os.path.join(hip, "match_many_f32_plan.h")).read()
    assert "hip/hip_runtime.h" not in plan and "__global__" not in plan and "__device__" not in plan      # plain C++
    src = open(os.path.join(hip, "match_many_f32.hip")).read()
    for inc in ("match_many_f32_plan.h", "match_f32_core.h", "match_many_join.h"):
        assert '#include "%s"' % inc in src, inc
    assert "__builtin_amdgcn_mfma_f32_32x32x16_f16" in src
    # the float matcher's shared pieces are stated once
    core = open(os.path.join(hip, "match_f32_core.h")).read()
    old = open(os.path.join(hip, "match.hip")).read()
    for piece in ("struct Top2 {", "void top2_insert(", "void top2_insert_lex(", "int perm_src(", "float l2_tree(", "unsigned short to_f16(",
                  "void match_scale(", "constexpr int MF_SEGCAP", "0.00197f"):
        assert piece in core and piece not in old and piece not in src, piece
    assert '#include "match_f32_core.h"' in old
    # the tuning table has no new row: the call follows POPSIFT_MATCH_MFMA
    assert "MANYF" not in open(os.path.join(hip, "psx_tuning.h")).read()
    fh = open(os.path.join(ROOT, "popsift_amd", "csrc", "include", "popsift", "features.h")).read()
    assert "matchPairsManyFloat(" in fh


def test_last_call_info_starts_at_zero_per_thread(capi):
    """a thread that never called reports zeros"""
    import threading
    got = {}
    t = threading.Thread(target=lambda: got.update(capi.match_many_f32_last()))
    t.start(); t.join()
    assert got == {"path": 0, "fell_back": 0, "launches": 0, "syncs": 0}
    assert capi.lib().psx_match_many_f32_last(None) == -1


def test_argument_errors_touch_nothing(capi):
    """every PSX_ERR_INVALID of the header, with sentinels in every output; the pointers are never dereferenced (they
    are not device memory: this runs without a GPU)"""
    L = capi.lib()
    good = capi.match_opts(0.8, True)
    fake = 0x1000                                            # a non-NULL "device pointer": an error return may not touch it
    for name in ENTRIES:
        fn = getattr(L, name)

        def call(left=fake, l_len=4, ptrs=(fake, fake), lens=(3, 5), n_sets=2, opts=good, out=True, cap=2, counts=True, count=True):
            pa = (C.c_void_p * max(len(ptrs), 1))(*ptrs) if ptrs is not None else None
            la = np.array(lens, np.int32) if lens is not None else None
            buf = np.full(16, -7, np.int32)
            sc = np.full(8, -9, np.int32)
            n = C.c_int(-5)
            rc = fn(0, left, l_len, pa, la.ctypes.data_as(C.c_void_p) if la is not None else None, n_sets,
                    C.byref(opts) if opts is not None else None, buf.ctypes.data_as(C.c_void_p) if out else None, cap,
                    sc.ctypes.data_as(C.c_void_p) if counts else None, C.byref(n) if count else None)
            assert np.all(buf == -7) and np.all(sc == -9) and n.value == -5, name
            return rc

        nan, inf = float("nan"), float("inf")
        # everything psx_match_pairs refuses
        for o in (capi.MatchOpts(nan, 0), capi.MatchOpts(0.0, 0), capi.MatchOpts(-0.5, 0), capi.MatchOpts(-inf, 0),
                  capi.MatchOpts(0.8, 2), capi.MatchOpts(0.8, -1)):
            assert call(opts=o) == -1, (name, o.ratio, o.flags)
        assert call(opts=None) == -1
        assert call(count=False) == -1
        assert call(l_len=-1) == -1
        assert call(cap=-1) == -1
        assert call(out=False, cap=2) == -1                  # a capacity without a buffer
        assert call(left=None) == -1                         # NULL left with a length
        # the sets
        assert call(n_sets=-1) == -1
        assert call(ptrs=None) == -1
        assert call(lens=None) == -1
        assert call(counts=False) == -1
        assert call(lens=(3, -1)) == -1
        assert call(ptrs=(fake, None)) == -1                 # a NULL set with a non-zero length
        assert call(l_len=2 ** 30, lens=(3, 5, 1), ptrs=(fake, fake, fake), n_sets=3) == -1      # n_sets * l_len above INT_MAX
        assert call(lens=(INT_MAX, 1)) == -1                 # the sum of r_lens above INT_MAX
    # the plan refuses the same sets, unknown flag bits, a switch that is neither 0 nor 1, a NULL report
    out = capi.ManyF32Plan(-5, -5, -5, -5, -5)
    for l_len, lens, n_sets, flags, mfma in ((4, (3, -1), 2, 0, 1), (4, (INT_MAX, 1), 2, 0, 1), (2 ** 30, (3, 5, 1), 3, 1, 1), (-1, (3, 5), 2, 0, 1),
                                             (4, (3, 5), -1, 0, 1), (4, (3, 5), 2, 2, 1), (4, (3, 5), 2, 0, 2), (4, (3, 5), 2, 0, -1), (4, None, 2, 0, 1)):
        la = np.array(lens, np.int32) if lens is not None else None
        rc = L.psx_match_many_f32_plan(l_len, la.ctypes.data_as(C.c_void_p) if la is not None else None, n_sets, flags, mfma, C.byref(out))
        assert rc == -1 and (out.path, out.fwd_groups, out.bwd_groups, out.launches, out.scratch_bytes) == (-5,) * 5, (l_len, lens, n_sets, flags, mfma)
    la = np.array((3, 5), np.int32)
    assert L.psx_match_many_f32_plan(4, la.ctypes.data_as(C.c_void_p), 2, 0, 1, None) == -1


def test_empty_forms_need_no_device(capi):
    """n_sets = 0, l_len = 0 and all-empty sets: PSX_OK, zero counts, nothing else written -- no pair can exist, so no
    device is touched (this runs without one); the last-call info then reports path 0 and no launch"""
    L = capi.lib()
    good = capi.match_opts(0.8, True)
    fake = 0x1000
    for name in ENTRIES:
        fn = getattr(L, name)
        n = C.c_int(-5)
        assert fn(0, None, 0, None, None, 0, C.byref(good), None, 0, None, C.byref(n)) == 0 and n.value == 0, name
        n = C.c_int(-5)
        assert fn(0, fake, 7, None, None, 0, C.byref(good), None, 0, None, C.byref(n)) == 0 and n.value == 0, name
        for l_ptr, l_len, lens, ptrs in ((None, 0, (3, 5, 0), (fake, fake, None)), (fake, 9, (0, 0, 0), (None, fake, None))):
            pa = (C.c_void_p * 3)(*ptrs)
            la = np.array(lens, np.int32)
            sc = np.full(5, -9, np.int32)
            buf = np.full(16, -7, np.int32)
            n = C.c_int(-5)
            rc = fn(0, l_ptr, l_len, pa, la.ctypes.data_as(C.c_void_p), 3, C.byref(good), buf.ctypes.data_as(C.c_void_p), 4,
                    sc.ctypes.data_as(C.c_void_p), C.byref(n))
            assert rc == 0 and n.value == 0 and list(sc) == [0, 0, 0, -9, -9] and np.all(buf == -7), (name, lens)
            assert capi.match_many_f32_last() == {"path": 0, "fell_back": 0, "launches": 0, "syncs": 0}
    # the python wrapper's form of the same (arrays without rows: nothing to upload)
    lists, counts = capi.match_pairs_many(np.zeros((0, 128), np.float32), [np.zeros((0, 128), np.float32)] * 2)
    assert [len(p) for p in lists] == [0, 0] and list(counts) == [0, 0]
    lists, counts = capi.match_pairs_many(np.zeros((0, 128), np.float32), [])
    assert lists == [] and len(counts) == 0
    assert capi.match_many_f32_plan(0, (3, 5)) == {"path": 0, "fwd_groups": 0, "bwd_groups": 0, "launches": 0, "scratch_bytes": 0}


@pytest.mark.parametrize("nl,lens", PLAN_SHAPES, ids=PLAN_IDS)
def test_plan_invariants(capi, nl, lens):
    """the path follows the rule, with the switch off too; at least one group per direction that runs; the launch count
    is the fixed kernels plus two per group; a group's share of the growing buffer stays within the budget"""
    for mfma in (True, False):
        for mutual in (False, True):
            p = capi.match_many_f32_plan(nl, lens, mutual, mfma)
            assert p["path"] == planned_path(nl, lens, mfma), (nl, mfma, mutual, p)
            assert p["fwd_groups"] >= 1 and p["bwd_groups"] == (p["bwd_groups"] if mutual else 0) and (not mutual or p["bwd_groups"] >= 1)
            assert p["launches"] == (2 if p["path"] == 2 else 1) + 2 * (p["fwd_groups"] + p["bwd_groups"]) + 3
            assert 0 < p["scratch_bytes"] <= BUDGET
            print("%d x %d sets (%d rows), mfma %d mutual %d: %s" % (nl, len(lens), sum(lens), mfma, mutual, p))
    # the three threshold cases, by name
    assert capi.match_many_f32_plan(255, (4096,))["path"] == 1 and capi.match_many_f32_plan(256, (4095,))["path"] == 1
    assert capi.match_many_f32_plan(256, (4096,))["path"] == 2 and capi.match_many_f32_plan(256, (4096,), mfma_enabled=False)["path"] == 1
    assert capi.match_many_f32_plan(256, (2048, 0, 2048))["path"] == 2            # the threshold is on the call's total


def test_plan_launches_do_not_grow_with_the_sets(capi):
    """3 and 40 sets of equal length, one group each way: the same number of launches, on either path"""
    for nl, n in ((300, 1400), (100, 64)):
        for mfma in (True, False):
            a, b = capi.match_many_f32_plan(nl, (n,) * 3, True, mfma), capi.match_many_f32_plan(nl, (n,) * 40, True, mfma)
            assert a["fwd_groups"] == b["fwd_groups"] == a["bwd_groups"] == b["bwd_groups"] == 1
            assert a["launches"] == b["launches"] == (9 if a["path"] == 2 else 8) and a["path"] == b["path"]
    # and grow by two per further group: the smallest K with two forward groups
    k = 1
    while capi.match_many_f32_plan(4096, (4096,) * k, True)["fwd_groups"] < 2:
        k += 1
    one, two = capi.match_many_f32_plan(4096, (4096,) * (k - 1), True), capi.match_many_f32_plan(4096, (4096,) * k, True)
    assert two["launches"] - one["launches"] == 2 * (two["fwd_groups"] + two["bwd_groups"] - one["fwd_groups"] - one["bwd_groups"])
    assert two["scratch_bytes"] <= BUDGET


def test_plan_under_sanitizers(tmp_path):
    """tests/cpp/match_many_f32_plan_san.cpp: a stand-alone program (its own main) that includes match_many_f32_plan.h
    alone and checks the tables and groups, compiled with -fsanitize=address,undefined and run directly."""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed"
    exe = str(tmp_path / "match_many_f32_plan_san")
    cmd = [cxx, "-std=c++14", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           "-static-libasan", "-static-libubsan",
           os.path.join(ROOT, "tests", "cpp", "match_many_f32_plan_san.cpp"), "-o", exe,
           "-I", os.path.join(ROOT, "popsift_amd", "csrc", "hip"), "-I", os.path.join(ROOT, "include")]
    subprocess.check_call(cmd)
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout


def test_cpp_match_many_f32_api(tmp_path):
    """tests/cpp/test_match_many_f32_api.cpp against libpopsift.so, built and run the way test_match_many_api.cpp is:
    matchPairsManyFloat throws for a null entry, an object on another device and byte descriptors, and returns empty lists
    for empty objects -- no device is touched; matchPairsMany still refuses float descriptors."""
    libdir = os.path.join(ROOT, "popsift_amd", "lib")
    if not os.path.exists(os.path.join(libdir, "libpopsift.so")):
        from popsift_amd import build
        build.build_all()
    exe = str(tmp_path / "test_match_many_f32_api")
    cmd = ["g++", "-std=c++14", "-O1", "-pthread", os.path.join(ROOT, "tests", "cpp", "test_match_many_f32_api.cpp"), "-o", exe,
           "-I", os.path.join(ROOT, "popsift_amd", "csrc", "include"), "-I", os.path.join(ROOT, "include"),
           "-L", libdir, "-lpopsift", "-lpopsift_hip", "-Wl,-rpath," + libdir]
    subprocess.check_call(cmd)
    env = {k: v for k, v in os.environ.items() if k != "POPSIFT_TEST_EXPECT_GPU"}
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120, env=env)
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout


@pytest.mark.parametrize("which", FLAVOURS)
@pytest.mark.parametrize("seed,nl,lens", CASES, ids=CASE_IDS)
def test_premise_of_the_planted_sets(oracle, capi, seed, nl, lens, which):
    """the oracle's directed results of every set with min(nl, nr) >= 64, in both flavours: one pair kept, one dropped by the
    ratio, one dropped by the cross-check alone -- a join that ignores a condition cannot pass on the GPU"""
    left, rights = planted_many_f32(seed, nl, lens, which)
    checked = 0
    for k, r in enumerate(rights):
        if min(nl, len(r)) >= 64:
            fm, fd, bm, bd = directed(oracle, ("many f32", seed, which, k), left, r, False)
            assert fd.dtype == np.float32
            assert_premise(fm, fd, bm, len(r), (seed, which, k))
            checked += 1
    assert checked == sum(1 for n in lens if min(nl, n) >= 64)


@pytest.mark.parametrize("which", FLAVOURS)
@pytest.mark.parametrize("seed", ORACLE_SEEDS)
def test_contract_restatement(capi, oracle, seed, which):
    """contract() / slices() over capi.pairs_join of the oracle's directed results: the expected bytes the GPU tests use
    for seeds 31 and 34 -- the concatenation, `right` local to its set, the counts, the truncation"""
    _, nl, lens = [c for c in CASES if c[0] == seed][0]
    left, rights = planted_many_f32(seed, nl, lens, which)
    per_set = []
    for k, r in enumerate(rights):
        fm, fd, bm, bd = directed(oracle, ("many f32", seed, which, k), left, r, False)
        per_set.append(capi.pairs_join(fm, fd, bm, len(r), 0.8, True))
        assert per_set[-1].dtype == capi.PAIR_DTYPE
    cat, counts, total = contract(per_set)
    assert total == sum(len(p) for p in per_set) == len(cat) and all((c > 0) == (min(nl, n) >= 64) or n < 64 for c, n in zip(counts, lens))
    assert all(same_records(a, b) for a, b in zip(slices(cat, counts), per_set))
    for k, p in enumerate(per_set):
        if len(p):
            assert np.all(np.diff(p["left"]) > 0) and p["right"].max() < lens[k]          # ascending left, right local to the set
    first = int(counts[0])
    assert first > 0 and cat["left"][first] <= cat["left"][first - 1] if total > first else True    # `left` starts again with every set
    for cap in (0, first // 2, first, total - 1, total, total + 5):
        part, c2, t2 = contract(per_set, cap)
        assert t2 == total and np.array_equal(c2, counts) and same_records(part, cat[:cap])
        got = slices(part, counts)
        assert sum(len(g) for g in got) == min(cap, total)
        assert all(same_records(g, p[:len(g)]) for g, p in zip(got, per_set))
        assert all(same_records(a, b) for a, b in zip(capi.split_sets(cat, counts, cap), got))
