"""CPU tests of the one-to-many byte pair search's host side (include/popsift_hip.h, "one descriptor set against many"): the
declarations and bindings; every argument error, before a device is looked at and with the outputs untouched; the empty
forms; the invariants of the plan (psx_match_many_plan, csrc/hip/match_many_plan.h) on the cases the GPU tests run; a
stand-alone sanitizer build of the plan; and the numpy restatement of the contract that the GPU tests reuse."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.match_many_cases import CASES, CASE_IDS, TINY_LENS, contract, planted_many, slices, tiny_many
from tests.match_pairs_cases import assert_premise, directed, same_records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_MAX = 2 ** 31 - 1
ENTRIES = ("psx_match_pairs_many_u8", "psx_match_pairs_many_u8_dev")


def test_entry_points_declared_and_bound(capi):
    hdr = open(os.path.join(ROOT, "include", "popsift_hip.h")).read()
    for sym in ENTRIES + ("psx_match_many_plan",):
        assert "int %s(" % sym in hdr and sym in capi.SYMBOLS and hasattr(capi.lib(), sym), sym
    assert "typedef struct psx_many_chunk { int set, r0, r1; }" in hdr and "typedef struct psx_many_block { int set, row0; }" in hdr
    for name in ("match_pairs_many_u8", "match_pairs_many_dev", "match_many_plan", "split_sets"):
        assert callable(getattr(capi, name)), name
    from popsift_amd import build
    assert "match_many.hip" in build.HIP_SOURCES
    assert " match_many " in open(os.path.join(ROOT, "CMakeLists.txt")).read()
    hip = os.path.join(ROOT, "popsift_amd", "csrc", "hip")
    plan = open(os.path.join(hip, "match_many_plan.h")).read()
    assert "hip/hip_runtime.h" not in plan and "__global__" not in plan and "__device__" not in plan      # plain C++
    src = open(os.path.join(hip, "match_many.hip")).read()
    assert '#include "match_many_plan.h"' in src and '#include "match_u8_core.h"' in src and "psx_match_keep" in src
    assert "atomic" not in src.replace("No atomics", "")                    # nothing in the ranking depends on arrival order
    # the byte matcher's inline pieces are stated once
    core = open(os.path.join(hip, "match_u8_core.h")).read()
    old = open(os.path.join(hip, "match.hip")).read()
    for piece in ("i32x4 u8_frag(", "void key_insert(", "constexpr unsigned U8_NONE"):
        assert piece in core and piece not in old and piece not in src, piece
    fh = open(os.path.join(ROOT, "popsift_amd", "csrc", "include", "popsift", "features.h")).read()
    assert "matchPairsMany(" in fh


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
        # everything psx_match_pairs_u8 refuses
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
    # the plan refuses the same sets
    nc, nb = C.c_int(-5), C.c_int(-5)
    for l_len, lens, n_sets, backward in ((4, (3, -1), 2, 0), (4, (INT_MAX, 1), 2, 0), (2 ** 30, (3, 5, 1), 3, 1), (-1, (3, 5), 2, 0),
                                          (4, (3, 5), -1, 0), (4, (3, 5), 2, 2), (4, None, 2, 0)):
        la = np.array(lens, np.int32) if lens is not None else None
        rc = L.psx_match_many_plan(l_len, la.ctypes.data_as(C.c_void_p) if la is not None else None, n_sets, backward,
                                   None, 0, C.byref(nc), None, 0, C.byref(nb))
        assert rc == -1 and nc.value == -5 and nb.value == -5, (l_len, lens, n_sets, backward)
    la = np.array((3, 5), np.int32)
    assert L.psx_match_many_plan(4, la.ctypes.data_as(C.c_void_p), 2, 0, None, 0, None, None, 0, C.byref(nb)) == -1
    assert L.psx_match_many_plan(4, la.ctypes.data_as(C.c_void_p), 2, 0, None, 3, C.byref(nc), None, 0, C.byref(nb)) == -1


def test_empty_forms_need_no_device(capi):
    """n_sets = 0, l_len = 0 and all-empty sets: PSX_OK, zero counts, nothing else written -- no pair can exist, so no
    device is touched (this runs without one)"""
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
    # the python wrapper's form of the same
    # the python wrapper's form of the same (arrays without rows: nothing to upload)
    lists, counts = capi.match_pairs_many_u8(np.zeros((0, 128), np.uint8), [np.zeros((0, 128), np.uint8)] * 2)
    assert [len(p) for p in lists] == [0, 0] and list(counts) == [0, 0]
    lists, counts = capi.match_pairs_many_u8(np.zeros((0, 128), np.uint8), [])
    assert lists == [] and len(counts) == 0


def _check_tables(lens, chunks, blocks, chunk_side):
    """the invariants of one table over the side it cuts: exact cover, nothing spans two sets, tiles, the key's 9 bits, a
    set's chunks ascending and contiguous, empty sets absent"""
    cover = [np.zeros(n, np.int32) for n in lens]
    if chunk_side:
        assert chunks.shape[1] == 3
        last = -1
        for c, (s, r0, r1) in enumerate(chunks):
            assert 0 <= s < len(lens) and lens[s] > 0
            assert r0 % 32 == 0 and 0 <= r0 < r1 <= lens[s] and r1 - r0 <= 512
            if s != last:
                assert s > last and r0 == 0                  # a set appears once, as one contiguous run, from its first row
                last = s
            else:
                assert r0 == chunks[c - 1][2]
            cover[s][r0:r1] += 1
    else:
        for b, (s, row0) in enumerate(blocks):
            assert 0 <= s < len(lens) and row0 % 256 == 0 and 0 <= row0 < lens[s]
            if b:
                ps, pr = blocks[b - 1]
                assert s > ps or (s == ps and row0 == pr + 256)
            cover[s][row0:row0 + 256] += 1
    for s, c in enumerate(cover):
        assert np.all(c == 1), s


@pytest.mark.parametrize("nl,lens", [(c[1], c[2]) for c in CASES] + [(70, TINY_LENS), (2048, (2048,) * 64), (18432, (18432,))],
                         ids=CASE_IDS + ["tiny200", "64x2048", "1x18432"])
def test_plan_invariants(capi, nl, lens):
    for backward in (False, True):
        chunks, blocks = capi.match_many_plan(nl, lens, backward)
        _check_tables([nl] if backward else list(lens), chunks, blocks, True)
        _check_tables(list(lens) if backward else [nl], chunks, blocks, False)
        print("%d x %d sets, backward %d: %d chunks (longest %d) x %d blocks" %
              (nl, len(lens), backward, len(chunks), int((chunks[:, 2] - chunks[:, 1]).max()), len(blocks)))
    # one set: the chunk length u8_plan (match.hip) chooses for psx_match_pairs_u8
    if len(lens) == 1 and lens[0] == 18432:
        chunks, blocks = capi.match_many_plan(nl, lens, False)
        assert len(blocks) == 72 and len(chunks) == 36 and np.all(chunks[:, 2] - chunks[:, 1] == 512)
    # enough workgroups for the chip where the sets are large enough to give them
    if len(lens) == 64:
        for backward in (False, True):
            chunks, blocks = capi.match_many_plan(nl, lens, backward)
            assert len(chunks) * len(blocks) == 2048


def test_plan_capacity_and_count(capi):
    L = capi.lib()
    lens = np.array(CASES[0][2], np.int32)
    full_c, full_b = capi.match_many_plan(300, lens, False)
    for cap in (0, 1, len(full_c) - 1):
        ch = np.full((cap + 1, 3), -7, np.int32)
        bl = np.full((2, 2), -7, np.int32)
        nc, nb = C.c_int(-1), C.c_int(-1)
        rc = L.psx_match_many_plan(300, lens.ctypes.data_as(C.c_void_p), len(lens), 0, ch.ctypes.data_as(C.c_void_p) if cap else None, cap,
                                   C.byref(nc), bl.ctypes.data_as(C.c_void_p), 1, C.byref(nb))
        assert rc == 0 and nc.value == len(full_c) and nb.value == len(full_b) == 2
        assert np.array_equal(ch[:cap], full_c[:cap]) and np.all(ch[cap:] == -7)
        assert np.array_equal(bl[0], full_b[0]) and np.all(bl[1] == -7)


def test_plan_under_sanitizers(tmp_path):
    """tests/cpp/match_many_plan_san.cpp: a stand-alone program (its own main) that includes match_many_plan.h alone and
    checks the invariants on exact-size heap arrays, compiled with -fsanitize=address,undefined and run directly."""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed"
    exe = str(tmp_path / "match_many_plan_san")
    cmd = [cxx, "-std=c++14", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           "-static-libasan", "-static-libubsan",
           os.path.join(ROOT, "tests", "cpp", "match_many_plan_san.cpp"), "-o", exe,
           "-I", os.path.join(ROOT, "popsift_amd", "csrc", "hip"), "-I", os.path.join(ROOT, "include")]
    subprocess.check_call(cmd)
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout


def test_cpp_match_many_api(tmp_path):
    """tests/cpp/test_match_many_api.cpp against libpopsift.so, built and run the way test_match_pairs_api.cpp is:
    matchPairsMany throws for a null entry, an object on another device and float descriptors, and returns empty lists for
    empty objects -- no device is touched."""
    libdir = os.path.join(ROOT, "popsift_amd", "lib")
    if not os.path.exists(os.path.join(libdir, "libpopsift.so")):
        from popsift_amd import build
        build.build_all()
    exe = str(tmp_path / "test_match_many_api")
    cmd = ["g++", "-std=c++14", "-O1", "-pthread", os.path.join(ROOT, "tests", "cpp", "test_match_many_api.cpp"), "-o", exe,
           "-I", os.path.join(ROOT, "popsift_amd", "csrc", "include"), "-I", os.path.join(ROOT, "include"),
           "-L", libdir, "-lpopsift", "-lpopsift_hip", "-Wl,-rpath," + libdir]
    subprocess.check_call(cmd)
    env = {k: v for k, v in os.environ.items() if k != "POPSIFT_TEST_EXPECT_GPU"}
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120, env=env)
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout


def test_contract_restatement(capi, oracle):
    """contract() / slices() on the host joins of the oracle's directed results of seed 22's three sets: the concatenation,
    `right` local to its set, the counts, and the truncation inside a set, at a set boundary, at total - 1 and at 0; the
    generator's premise holds for every set it is asserted for on the GPU."""
    seed, nl, lens = CASES[1]
    left, rights = planted_many(seed, nl, lens)
    per_set = []
    for k, r in enumerate(rights):
        fm, fd, bm, bd = directed(oracle, ("many", seed, k), left, r, True)
        assert_premise(fm, fd, bm, len(r), (seed, k))
        per_set.append(capi.pairs_join(fm, fd, bm, len(r), 0.8, True))
    cat, counts, total = contract(per_set)
    assert total == sum(len(p) for p in per_set) == len(cat) and np.all(counts > 0)
    assert all(same_records(a, b) for a, b in zip(slices(cat, counts), per_set))
    for k, p in enumerate(per_set):
        assert np.all(np.diff(p["left"]) > 0) and p["right"].max() < lens[k]          # ascending left, right local to the set
    assert cat["left"][counts[0]] <= cat["left"][counts[0] - 1]                       # `left` starts again with every set
    for cap in (0, counts[0] // 2, counts[0], counts[0] + counts[1] // 2, total - 1, total, total + 5):
        part, c2, t2 = contract(per_set, cap)
        assert t2 == total and np.array_equal(c2, counts) and same_records(part, cat[:cap])
        got = slices(part, counts)
        assert sum(len(g) for g in got) == min(cap, total)
        assert all(same_records(g, p[:len(g)]) for g, p in zip(got, per_set))
        assert all(same_records(a, b) for a, b in zip(capi.split_sets(cat, counts, cap), got))
    # the tiny sets: every non-empty one holds an exact copy of a left row
    left, rights = tiny_many()
    assert [len(r) for r in rights] == list(TINY_LENS) and all((r[k % len(r)] == left[k % 70]).all() for k, r in enumerate(rights) if len(r))
