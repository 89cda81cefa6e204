"""CPU tests of the pair search over an edge list (include/popsift_hip.h, "a list of view pairs over N descriptor sets"): the
declarations and bindings; every argument error, before a device is looked at and with the outputs untouched; the empty forms;
the figures of the plan (psx_match_graph_plan, csrc/hip/match_graph_plan.h) on the cases the GPU tests run, against a
restatement of the documented rules; a stand-alone sanitizer build of the plan, which checks the tables themselves; and the
numpy restatement of the contract that the GPU tests reuse."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.match_graph_cases import (MIXED_EDGES, MIXED_LENS, MIXED_PREMISE, MIXED_SEED, PLAN_CASES, contract, graph_sets, nchunks,
                                     numpy_pairs, plan_restated, slices)
from tests.match_pairs_cases import assert_premise, directed, same_records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_MAX = 2 ** 31 - 1
ENTRIES = ("psx_match_pairs_graph_u8", "psx_match_pairs_graph_u8_dev")


def test_entry_points_declared_and_bound(capi):
    hdr = open(os.path.join(ROOT, "include", "popsift_hip.h")).read()
    for sym in ENTRIES + ("psx_match_graph_plan",):
        assert "int %s(" % sym in hdr and sym in capi.SYMBOLS and hasattr(capi.lib(), sym), sym
    assert "typedef struct psx_view_edge { int left, right; } psx_view_edge;" in hdr and "typedef struct psx_graph_plan_info {" in hdr
    for name in ("match_pairs_graph_u8", "match_pairs_graph_dev", "match_graph_plan"):
        assert callable(getattr(capi, name)), name
    assert C.sizeof(capi.GraphPlanInfo) == 48
    from popsift_amd import build
    assert "match_graph.hip" in build.HIP_SOURCES
    assert " match_graph " in open(os.path.join(ROOT, "CMakeLists.txt")).read()
    hip = os.path.join(ROOT, "popsift_amd", "csrc", "hip")
    plan = open(os.path.join(hip, "match_graph_plan.h")).read()
    assert "hip/hip_runtime.h" not in plan and "__global__" not in plan and "__device__" not in plan      # plain C++
    assert '#include "match_many_plan.h"' in plan
    src = open(os.path.join(hip, "match_graph.hip")).read()
    for piece in ('#include "match_graph_plan.h"', '#include "match_u8_core.h"', "psx_match_keep", "wg_scan_totals", "u8_load_cols(",
                  "u8_walk(", "u8_store_keys(", "u8_merge_chunk("):
        assert piece in src, piece
    assert "atomic" not in src                                              # nothing in the ranking depends on arrival order
    # the graph call's buffers are its own: no slot of another feature appears in its source
    scratch = open(os.path.join(hip, "match_scratch.h")).read()
    for slot in ("MS_GRAPH_TABLES", "MS_GRAPH_NORMS", "MS_GRAPH_PARTIAL", "MS_GRAPH_FWD", "MS_GRAPH_BWD", "MS_GRAPH_TOT"):
        assert slot in scratch and slot in src, slot
    assert "MS_MANY_" not in src and "MS_U8_" not in src and "MS_PAIRS_TOT" not in src
    fh = open(os.path.join(ROOT, "popsift_amd", "csrc", "include", "popsift", "features.h")).read()
    assert "matchPairsGraph(" in fh


def test_argument_errors_touch_nothing(capi):
    """every PSX_ERR_INVALID of the header, with sentinels in every output; the pointers are never dereferenced (they are
    not device memory: this runs without a GPU)"""
    L = capi.lib()
    good = capi.match_opts(0.8, True)
    fake = 0x1000                                            # a non-NULL "device pointer": an error return may not touch it
    for name in ENTRIES:
        fn = getattr(L, name)

        def call(ptrs=(fake, fake, fake), lens=(3, 5, 4), n_sets=3, edges=((0, 1), (2, 0)), n_edges=2, opts=good, out=True, cap=2, counts=True,
                 count=True):
            pa = (C.c_void_p * max(len(ptrs), 1))(*ptrs) if ptrs is not None else None
            la = np.array(lens, np.int32) if lens is not None else None
            ea = np.array(edges, np.int32).reshape(-1, 2) if edges is not None else None
            buf = np.full(16, -7, np.int32)
            sc = np.full(8, -9, np.int32)
            n = C.c_int(-5)
            rc = fn(0, pa, la.ctypes.data_as(C.c_void_p) if la is not None else None, n_sets,
                    ea.ctypes.data_as(C.c_void_p) if ea is not None else None, n_edges,
                    C.byref(opts) if opts is not None else None, buf.ctypes.data_as(C.c_void_p) if out else None, cap,
                    sc.ctypes.data_as(C.c_void_p) if counts else None, C.byref(n) if count else None)
            assert np.all(buf == -7) and np.all(sc == -9) and n.value == -5, name
            return rc

        nan, inf = float("nan"), float("inf")
        # everything psx_match_pairs_u8 refuses about opts, output, capacity and count
        for o in (capi.MatchOpts(nan, 0), capi.MatchOpts(0.0, 0), capi.MatchOpts(-0.5, 0), capi.MatchOpts(-inf, 0),
                  capi.MatchOpts(0.8, 2), capi.MatchOpts(0.8, -1)):
            assert call(opts=o) == -1, (name, o.ratio, o.flags)
        assert call(opts=None) == -1
        assert call(count=False) == -1
        assert call(cap=-1) == -1
        assert call(out=False, cap=2) == -1                  # a capacity without a buffer
        # the sets and the edges
        assert call(n_sets=-1) == -1
        assert call(n_edges=-1) == -1
        assert call(ptrs=None) == -1
        assert call(lens=None) == -1
        assert call(edges=None) == -1
        assert call(counts=False) == -1
        assert call(lens=(3, -1, 4)) == -1
        assert call(lens=(3, 5, -4), edges=((0, 1), (0, 1))) == -1           # a negative length, even of a set no edge names
        assert call(ptrs=(fake, None, fake)) == -1           # a NULL set with a non-zero length
        assert call(ptrs=(fake, fake, None), edges=((0, 1), (0, 1))) == -1   # ... even when no edge names it
        for bad in ((0, 3), (3, 0), (-1, 0), (0, -1), (INT_MAX, 0)):
            assert call(edges=((0, 1), bad)) == -1, bad      # every edge is checked, not only the first
        assert call(ptrs=None, lens=None, n_sets=0) == -1    # no sets: no edge is in range
        assert call(lens=(2 ** 30, 5, 4), edges=((0, 1), (0, 2), (0, 0)), n_edges=3) == -1        # the sum of lens[left] above INT_MAX
        assert call(lens=(5, 2 ** 30, 4), edges=((0, 1), (2, 1), (1, 1)), n_edges=3) == -1        # ... of lens[right]
    # the plan refuses the same sets and edges, and unknown flags
    info = capi.GraphPlanInfo()
    info.launches = -5
    for lens, n_sets, edges, n_edges, flags in (((3, -1), 2, ((0, 1),), 1, 0), ((3, 5), -1, ((0, 1),), 1, 0), ((3, 5), 2, ((0, 1),), -1, 0),
                                                ((3, 5), 2, ((0, 2),), 1, 0), ((3, 5), 2, ((-1, 1),), 1, 0), ((3, 5), 2, ((0, 1),), 1, 2),
                                                (None, 2, ((0, 1),), 1, 0), ((3, 5), 2, None, 1, 0), (None, 0, ((0, 0),), 1, 0),
                                                ((2 ** 30, 1), 2, ((0, 1), (0, 1), (0, 0)), 3, 1)):
        la = np.array(lens, np.int32) if lens is not None else None
        ea = np.array(edges, np.int32).reshape(-1, 2) if edges is not None else None
        rc = L.psx_match_graph_plan(la.ctypes.data_as(C.c_void_p) if la is not None else None, n_sets,
                                    ea.ctypes.data_as(C.c_void_p) if ea is not None else None, n_edges, flags, C.byref(info))
        assert rc == -1 and info.launches == -5, (lens, n_sets, edges, n_edges, flags)
    la, ea = np.array((3, 5), np.int32), np.array(((0, 1),), np.int32)
    assert L.psx_match_graph_plan(la.ctypes.data_as(C.c_void_p), 2, ea.ctypes.data_as(C.c_void_p), 1, 0, None) == -1


def test_empty_forms_need_no_device(capi):
    """n_edges = 0, n_sets = 0 and lists whose every edge has an empty side: PSX_OK, zero counts, nothing else written -- no
    pair can exist, so no device is touched (this runs without one)"""
    L = capi.lib()
    good = capi.match_opts(0.8, True)
    fake = 0x1000
    for name in ENTRIES:
        fn = getattr(L, name)
        n = C.c_int(-5)
        assert fn(0, None, None, 0, None, 0, C.byref(good), None, 0, None, C.byref(n)) == 0 and n.value == 0, name
        pa, la = (C.c_void_p * 2)(fake, fake), np.array((7, 9), np.int32)
        n = C.c_int(-5)
        assert fn(0, pa, la.ctypes.data_as(C.c_void_p), 2, None, 0, C.byref(good), None, 0, None, C.byref(n)) == 0 and n.value == 0, name
        for ptrs, lens, edges in (((fake, None, None), (9, 0, 0), ((0, 1), (1, 0), (2, 2), (1, 2))), ((None, None, None), (0, 0, 0), ((0, 0), (1, 2)))):
            pa = (C.c_void_p * 3)(*ptrs)
            la = np.array(lens, np.int32)
            ea = np.array(edges, np.int32)
            sc = np.full(len(edges) + 2, -9, np.int32)
            buf = np.full(16, -7, np.int32)
            n = C.c_int(-5)
            rc = fn(0, pa, la.ctypes.data_as(C.c_void_p), 3, ea.ctypes.data_as(C.c_void_p), len(edges), C.byref(good),
                    buf.ctypes.data_as(C.c_void_p), 4, sc.ctypes.data_as(C.c_void_p), C.byref(n))
            assert rc == 0 and n.value == 0 and list(sc) == [0] * len(edges) + [-9, -9] and np.all(buf == -7), (name, lens)
    # the python wrappers' forms of the same (arrays without rows: nothing to upload)
    z = np.zeros((0, 128), np.uint8)
    lists, counts = capi.match_pairs_graph_u8([z, z], [(0, 1), (1, 1)])
    assert [len(p) for p in lists] == [0, 0] and list(counts) == [0, 0]
    lists, counts = capi.match_pairs_graph_u8([z], [])
    assert lists == [] and len(counts) == 0
    lists, counts = capi.match_pairs_graph_u8([], [])
    assert lists == [] and len(counts) == 0
    for mutual in (False, True):
        info = capi.match_graph_plan((9, 0, 0), [(0, 1), (1, 0), (2, 2)], mutual)
        assert all(v == 0 for v in info.values()), info
        assert all(v == 0 for v in capi.match_graph_plan((), [], mutual).values())


@pytest.mark.parametrize("case", sorted(PLAN_CASES), ids=sorted(PLAN_CASES))
def test_plan_figures(capi, case):
    """what psx_match_graph_plan reports equals what the documented rules give at the chunk length it reports: every
    referenced set cut once (unreferenced ones absent), items = blocks(outer) x chunks(inner) summed over the edges per
    direction, join workgroups = ceil(lens[left] / 256) per edge, launches = 1 + 2 per group + 3.  The tables themselves --
    exact cover, nothing spanning two sets, every (edge, block, chunk) triple once per direction, the per-edge prefix sums
    -- are checked entry by entry by tests/cpp/match_graph_plan_san.cpp on the same cases (test_plan_under_sanitizers)."""
    lens, edges = PLAN_CASES[case]
    for mutual in (False, True):
        info = capi.match_graph_plan(lens, edges, mutual)
        cl = info["chunk_len"]
        assert cl % 32 == 0 and 32 <= cl <= 512
        want = plan_restated(lens, edges, mutual)(cl)
        assert {k: info[k] for k in want} == want, (case, mutual, info, want)
        assert info["fwd_groups"] >= 1 and info["bwd_groups"] == (info["fwd_groups"] if case == "budget" else 1) * mutual
        assert info["launches"] == 1 + 2 * (info["fwd_groups"] + info["bwd_groups"]) + 3
        assert 0 < info["scratch_bytes"]
        if case != "budget":
            assert info["launches"] == (8 if mutual else 6) and info["scratch_bytes"] <= 256 << 20
            # one group: the partials are chunks(inner) x rows(outer) key pairs per edge, the larger direction's sum
            live = [(a, b) for a, b in edges if lens[a] and lens[b]]
            f = sum(nchunks(lens[b], cl) * lens[a] for a, b in live)
            b_ = sum(nchunks(lens[a], cl) * lens[b] for a, b in live) if mutual else 0
            assert info["scratch_bytes"] == 8 * max(f, b_)
        print(case, mutual, info)
    if case == "budget":
        # 64 x (36 chunks x 18 432 rows x 8 bytes) = 340 MB of partials per direction: two groups of whole edges each
        info = capi.match_graph_plan(lens, edges, True)
        assert info["fwd_groups"] == 2 and info["bwd_groups"] == 2 and info["launches"] == 12
        assert info["chunk_len"] == 512 and info["blocks"] == 72 and info["chunks"] == 36 and info["fwd_items"] == 64 * 72 * 36
        assert 64 * 36 * 18432 * 8 > 256 << 20 >= info["scratch_bytes"] > 128 << 20
    if case == "32x2048-all":
        info = capi.match_graph_plan(lens, edges, True)
        assert info["referenced_sets"] == 32 and info["blocks"] == 256 and info["chunks"] == 128 and info["fwd_items"] == 496 * 8 * 4


def test_plan_ignores_what_no_live_edge_names(capi):
    """a set that no edge names, or that only faces an empty set, is absent: the plan is that of the remaining sets"""
    a = capi.match_graph_plan((40, 50, 60, 0), [(1, 1), (0, 3)], True)
    b = capi.match_graph_plan((50,), [(0, 0)], True)
    assert a == b and a["referenced_sets"] == 1 and a["blocks"] == 1
    # the chunk length is one per call and has the whole call in view: one small edge alone gets single tiles, the same edge
    # beside 495 image-sized ones the call's 512
    lens, edges = PLAN_CASES["32x2048-all"]
    assert capi.match_graph_plan((300, 257), [(0, 1)], True)["chunk_len"] == 32
    assert capi.match_graph_plan(lens + (300, 257), edges + [(32, 33)], True)["chunk_len"] == 512


def test_plan_under_sanitizers(tmp_path):
    """tests/cpp/match_graph_plan_san.cpp: a stand-alone program (its own main) that includes match_graph_plan.h alone and
    checks the invariants on exact-size heap arrays, compiled with -fsanitize=address,undefined and run directly."""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed"
    exe = str(tmp_path / "match_graph_plan_san")
    cmd = [cxx, "-std=c++14", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           "-static-libasan", "-static-libubsan",
           os.path.join(ROOT, "tests", "cpp", "match_graph_plan_san.cpp"), "-o", exe,
           "-I", os.path.join(ROOT, "popsift_amd", "csrc", "hip"), "-I", os.path.join(ROOT, "include")]
    subprocess.check_call(cmd)
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout


def test_cpp_match_graph_api(tmp_path):
    """tests/cpp/test_match_graph_api.cpp against libpopsift.so, built and run the way test_match_many_api.cpp is:
    matchPairsGraph throws for an edge out of range, a null referenced entry, views on different devices and float
    descriptors, and returns empty lists for empty objects -- no device is touched."""
    libdir = os.path.join(ROOT, "popsift_amd", "lib")
    if not os.path.exists(os.path.join(libdir, "libpopsift.so")):
        from popsift_amd import build
        build.build_all()
    exe = str(tmp_path / "test_match_graph_api")
    cmd = ["g++", "-std=c++14", "-O1", "-pthread", os.path.join(ROOT, "tests", "cpp", "test_match_graph_api.cpp"), "-o", exe,
           "-I", os.path.join(ROOT, "popsift_amd", "csrc", "include"), "-I", os.path.join(ROOT, "include"),
           "-L", libdir, "-lpopsift", "-lpopsift_hip", "-Wl,-rpath," + libdir]
    subprocess.check_call(cmd)
    env = {k: v for k, v in os.environ.items() if k != "POPSIFT_TEST_EXPECT_GPU"}
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120, env=env)
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout


def test_contract_restatement(capi, oracle):
    """The contract on host data alone, for the mixed list the GPU test runs: per edge the numpy restatement of the single
    call (numpy_pairs), which for the edges between set 0 and a set of >= 64 rows equals the host join (capi.pairs_join) of
    the oracle's directed results; the generator's premise holds for those edges; every other edge with two non-empty sides
    returns at least one pair at ratio inf; and contract() / slices() cut the concatenation inside an edge, at an edge
    boundary, at total - 1 and at 0."""
    sets = graph_sets(MIXED_SEED, MIXED_LENS)
    assert [len(s) for s in sets] == list(MIXED_LENS)
    assert MIXED_EDGES != sorted(MIXED_EDGES) and len(set(MIXED_EDGES)) < len(MIXED_EDGES)          # unsorted, with a duplicate
    for a, b in MIXED_PREMISE:
        fm, fd, bm, bd = directed(oracle, ("graph", MIXED_SEED, a, b), sets[a], sets[b], True)
        assert_premise(fm, fd, bm, len(sets[b]), (a, b))
        for ratio in (0.6, 0.8, float("inf")):
            for mutual in (False, True):
                want = capi.pairs_join(fm, fd, bm if mutual else None, len(sets[b]), ratio, mutual)
                assert same_records(numpy_pairs(sets[a], sets[b], ratio, mutual), want), (a, b, ratio, mutual)
    for a, b in MIXED_EDGES:
        n = len(numpy_pairs(sets[a], sets[b], float("inf"), True))
        assert (n >= 1) == (MIXED_LENS[a] > 0 and MIXED_LENS[b] > 0), (a, b, n)
    self_edge = numpy_pairs(sets[0], sets[0], 0.8, True)
    assert len(self_edge) == 300 and np.all(self_edge["left"] == self_edge["right"]) and np.all(self_edge["d1"] == 0)   # every row finds itself
    per_edge = [numpy_pairs(sets[a], sets[b], 0.8, True) for a, b in MIXED_EDGES]
    cat, counts, total = contract(per_edge)
    assert total == len(cat) and all(c == 0 for c, (a, b) in zip(counts, MIXED_EDGES) if MIXED_LENS[a] == 0 or MIXED_LENS[b] == 0)
    dup = [i for i, e in enumerate(MIXED_EDGES) if e == (0, 1)]
    assert len(dup) == 2 and same_records(per_edge[dup[0]], per_edge[dup[1]]) and counts[dup[0]] > 4
    fwd, rev = per_edge[MIXED_EDGES.index((3, 4))], per_edge[MIXED_EDGES.index((4, 3))]
    assert len(fwd) and len(rev) and fwd["right"].max() < 513 and rev["right"].max() < 33            # (a, b) and (b, a): two lists
    for cap in (0, int(counts[0]) // 2, int(counts[0]), int(counts[0] + counts[1] // 2), total - 1, total, total + 5):
        part, c2, t2 = contract(per_edge, cap)
        assert t2 == total and np.array_equal(c2, counts) and same_records(part, cat[:cap])
        got = slices(part, counts)
        assert sum(len(g) for g in got) == min(cap, total) and all(same_records(g, p[:len(g)]) for g, p in zip(got, per_edge))
        assert all(same_records(x, y) for x, y in zip(capi.split_sets(cat, counts, cap), got))
