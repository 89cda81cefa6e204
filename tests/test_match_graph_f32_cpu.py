"""CPU tests of the float forms of the edge-list calls (include/popsift_hip.h): psx_match_pairs_graph (+ _dev),
psx_match_graph_f32_plan, psx_match_graph_f32_last, psx_match_pairs_guided_many (+ _dev) and psx_match_pairs_guided_graph
(+ _dev).  The declarations and bindings; every argument error, before a device is looked at and with the outputs untouched;
the empty forms; the figures of the plan (csrc/hip/match_graph_f32_plan.h) on the cases the GPU tests run and on the shapes the
measurement uses, against a restatement of the documented rules; the path rule at its edges; a stand-alone sanitizer build of
the plan, which checks the tables themselves; the C++ methods' signatures and throws."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import match_graph_f32_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_MAX = 2 ** 31 - 1
GRAPH = ("psx_match_pairs_graph", "psx_match_pairs_graph_dev")
GUIDED_MANY = ("psx_match_pairs_guided_many", "psx_match_pairs_guided_many_dev")
GUIDED_GRAPH = ("psx_match_pairs_guided_graph", "psx_match_pairs_guided_graph_dev")
HELPERS = ("psx_match_graph_f32_plan", "psx_match_graph_f32_last")


def test_entry_points_declared_and_bound(capi):
    """the six entry points and the two helpers: in the header, in capi.SYMBOLS, in the library; the wrappers; the new unit in
    both build lists; the plan header plain C++ on the two plan headers it builds on; the shared device pieces stated once"""
    hdr = open(os.path.join(ROOT, "include", "popsift_hip.h")).read()
    for sym in GRAPH + GUIDED_MANY + GUIDED_GRAPH + HELPERS:
        assert "int %s(" % sym in hdr and sym in capi.SYMBOLS and hasattr(capi.lib(), sym), sym
    assert "typedef struct psx_graph_f32_plan_info {" in hdr and "There is no float form" not in hdr and "Only the byte form" not in hdr
    for name in ("match_pairs_graph", "match_graph_f32_plan", "match_graph_f32_last", "match_pairs_guided_many", "match_pairs_guided_graph"):
        assert callable(getattr(capi, name)), name
    import inspect
    for name in ("match_pairs_graph_dev", "match_pairs_guided_many_dev", "match_pairs_guided_graph_dev", "match_pairs_many_dev"):
        assert inspect.signature(getattr(capi, name)).parameters["u8"].default is True, name          # the default is the byte call
    assert C.sizeof(capi.GraphF32PlanInfo) == 56
    from popsift_amd import build
    assert "match_graph_f32.hip" in build.HIP_SOURCES
    assert " match_graph_f32 " in open(os.path.join(ROOT, "CMakeLists.txt")).read()
    hip = os.path.join(ROOT, "popsift_amd", "csrc", "hip")
    plan = open(os.path.join(hip, "match_graph_f32_plan.h")).read()
    assert "hip/hip_runtime.h" not in plan and "__global__" not in plan and "__device__" not in plan      # plain C++
    assert '#include "match_graph_plan.h"' in plan and '#include "match_many_f32_plan.h"' in plan
    src = open(os.path.join(hip, "match_graph_f32.hip")).read()
    star = open(os.path.join(hip, "match_many_f32.hip")).read()
    byte = open(os.path.join(hip, "match_graph.hip")).read()
    for piece in ('#include "match_graph_f32_plan.h"', '#include "match_f32_many_core.h"', '#include "match_graph_join.h"', "psx_graph_f32_build(",
                  "fm_prefilter_block(", "fm_exact_row(", "fm_norms_block(", "fm_cvt_block(", "fm_permute_block(", "__launch_bounds__(256, 3)"):
        assert piece in src, piece
    core = open(os.path.join(hip, "match_f32_many_core.h")).read()
    join = open(os.path.join(hip, "match_graph_join.h")).read()
    for piece in ("void fm_walk(", "fm_exact_row(", "fm_prefilter_block(", "__builtin_amdgcn_mfma_f32_32x32x16_f16"):
        assert piece in core and "void fm_walk(" not in star and "void fm_walk(" not in src, piece      # stated once
    assert "__builtin_amdgcn_mfma_f32_32x32x16_f16(a, " in core and "__builtin_amdgcn_mfma_f32_32x32x16_f16(a, " not in src + star
    for k in ("k_graph_count", "k_graph_scan", "k_graph_write"):
        assert "void %s(" % k in join and "void %s(" % k not in byte and "void %s(" % k not in src, k
    assert "psx_graph_join_queue<int>" in byte and "psx_graph_join_queue<float>" in src
    gg = open(os.path.join(hip, "match_guided_graph.hip")).read()
    assert "template int psx_guided_edges_run<unsigned char>(" in gg and "template int psx_guided_edges_run<float>(" in gg
    assert gg.count("g_match_row<float, float, false>(") == 1 and gg.count("g_match_row<float, float, true>(") == 1
    fh = open(os.path.join(ROOT, "popsift_amd", "csrc", "include", "popsift", "features.h")).read()
    for m in ("matchPairsGraphFloat(", "matchPairsGuidedManyFloat(", "matchPairsGuidedGraphFloat("):
        assert m in fh, m


def _arrays(ptrs, lens, edges):
    pa = (C.c_void_p * max(len(ptrs), 1))(*ptrs) if ptrs is not None else None
    la = np.array(lens, np.int32) if lens is not None else None
    ea = np.array(edges, np.int32).reshape(-1, 2) if edges is not None else None
    ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    return pa, la, ea, ptr


def test_argument_errors_touch_nothing(capi):
    """every PSX_ERR_INVALID of the header, with sentinels in every output; the pointers are never dereferenced (they are
    not device memory: this runs without a GPU)"""
    L = capi.lib()
    good = capi.match_opts(0.8, True)
    fake = 0x1000                                            # a non-NULL "device pointer": an error return may not touch it
    nan, inf = float("nan"), float("inf")
    bad_opts = (capi.MatchOpts(nan, 0), capi.MatchOpts(0.0, 0), capi.MatchOpts(-0.5, 0), capi.MatchOpts(-inf, 0), capi.MatchOpts(0.8, 2),
                capi.MatchOpts(0.8, -1))
    window = capi.Guide.make(capi.GUIDE_HOMOGRAPHY, np.eye(3, dtype=np.float32).reshape(9), 2.0)
    broken = capi.Guide.make(capi.GUIDE_HOMOGRAPHY, np.eye(3, dtype=np.float32).reshape(9), 2.0)
    broken.kind = 7
    for name in GRAPH + GUIDED_GRAPH:
        fn = getattr(L, name)
        guided = name in GUIDED_GRAPH

        def call(ptrs=(fake, fake, fake), xys=(fake, fake, fake), lens=(3, 5, 4), n_sets=3, edges=((0, 1), (2, 0)), n_edges=2, opts=good, out=True,
                 cap=2, counts=True, count=True, guides=(window, window)):
            pa, la, ea, ptr = _arrays(ptrs, lens, edges)
            xa = (C.c_void_p * max(len(xys), 1))(*xys) if xys is not None else None
            ga = (capi.Guide * max(len(guides), 1))(*guides) if guides is not None else None
            buf = np.full(16, -7, np.int32)
            sc = np.full(8, -9, np.int32)
            n = C.c_int(-5)
            tail = (C.byref(opts) if opts is not None else None, ptr(buf) if out else None, cap, ptr(sc) if counts else None,
                    C.byref(n) if count else None)
            if guided:
                rc = fn(0, pa, xa, ptr(la), n_sets, ptr(ea), n_edges, ga, *tail)
            else:
                rc = fn(0, pa, ptr(la), n_sets, ptr(ea), n_edges, *tail)
            assert np.all(buf == -7) and np.all(sc == -9) and n.value == -5, name
            return rc

        for o in bad_opts:
            assert call(opts=o) == -1, (name, o.ratio, o.flags)
        assert call(opts=None) == -1
        assert call(count=False) == -1
        assert call(cap=-1) == -1
        assert call(out=False, cap=2) == -1                  # a capacity without a buffer
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
        assert call(ptrs=None, xys=None, lens=None, n_sets=0) == -1          # no sets: no edge is in range
        g3 = (window, window, window)
        assert call(lens=(2 ** 30, 5, 4), edges=((0, 1), (0, 2), (0, 0)), n_edges=3, guides=g3) == -1     # the sum of lens[left] above INT_MAX
        assert call(lens=(5, 2 ** 30, 4), edges=((0, 1), (2, 1), (1, 1)), n_edges=3, guides=g3) == -1     # ... of lens[right]
        if guided:
            assert call(xys=None) == -1
            assert call(xys=(fake, None, fake)) == -1
            assert call(guides=None) == -1
            assert call(guides=(window, broken)) == -1       # every guide is checked
            assert call(guides=(capi.Guide.none(), broken)) == -1
    for name in GUIDED_MANY:
        fn = getattr(L, name)

        def many(left=fake, lxy=fake, l_len=3, ptrs=(fake, fake), xys=(fake, fake), lens=(5, 4), n_sets=2, guides=(window, window), opts=good, out=True,
                 cap=2, counts=True, count=True):
            pa = (C.c_void_p * 2)(*ptrs) if ptrs is not None else None
            xa = (C.c_void_p * 2)(*xys) if xys is not None else None
            la = np.array(lens, np.int32) if lens is not None else None
            ga = (capi.Guide * 2)(*guides) if guides is not None else None
            buf, sc, n = np.full(16, -7, np.int32), np.full(8, -9, np.int32), C.c_int(-5)
            ptr = lambda a: a.ctypes.data_as(C.c_void_p)
            rc = fn(0, left, lxy, l_len, pa, xa, ptr(la) if la is not None else None, n_sets, ga, C.byref(opts) if opts is not None else None,
                    ptr(buf) if out else None, cap, ptr(sc) if counts else None, C.byref(n) if count else None)
            assert np.all(buf == -7) and np.all(sc == -9) and n.value == -5, name
            return rc

        for o in bad_opts:
            assert many(opts=o) == -1, (name, o.ratio, o.flags)
        for kw in (dict(opts=None), dict(count=False), dict(cap=-1), dict(out=False, cap=2), dict(n_sets=-1), dict(l_len=-1), dict(left=None),
                   dict(lxy=None), dict(ptrs=None), dict(xys=None), dict(lens=None), dict(counts=False), dict(guides=None), dict(lens=(5, -4)),
                   dict(ptrs=(fake, None)), dict(xys=(None, fake)), dict(guides=(window, broken)), dict(guides=(capi.Guide.none(), broken)),
                   dict(l_len=2 ** 30, lens=(5, 4))):
            assert many(**kw) == -1, (name, kw)
    # the plan refuses the same sets and edges, unknown flags, an mfma switch that is neither 0 nor 1
    info = capi.GraphF32PlanInfo()
    info.launches = -5
    for lens, n_sets, edges, n_edges, flags, mfma in (((3, -1), 2, ((0, 1),), 1, 0, 1), ((3, 5), -1, ((0, 1),), 1, 0, 1), ((3, 5), 2, ((0, 1),), -1, 0, 1),
                                                      ((3, 5), 2, ((0, 2),), 1, 0, 1), ((3, 5), 2, ((-1, 1),), 1, 0, 1), ((3, 5), 2, ((0, 1),), 1, 2, 1),
                                                      (None, 2, ((0, 1),), 1, 0, 1), ((3, 5), 2, None, 1, 0, 1), (None, 0, ((0, 0),), 1, 0, 1),
                                                      ((3, 5), 2, ((0, 1),), 1, 0, 2), ((3, 5), 2, ((0, 1),), 1, 0, -1),
                                                      ((2 ** 30, 1), 2, ((0, 1), (0, 1), (0, 0)), 3, 1, 1)):
        _, la, ea, ptr = _arrays(None, lens, edges)
        rc = L.psx_match_graph_f32_plan(ptr(la), n_sets, ptr(ea), n_edges, flags, mfma, C.byref(info))
        assert rc == -1 and info.launches == -5, (lens, n_sets, edges, n_edges, flags, mfma)
    _, la, ea, ptr = _arrays(None, (3, 5), ((0, 1),))
    assert L.psx_match_graph_f32_plan(ptr(la), 2, ptr(ea), 1, 0, 1, None) == -1
    assert L.psx_match_graph_f32_last(None) == -1


def test_empty_forms_need_no_device(capi):
    """n_edges = 0, n_sets = 0, lists whose every edge has an empty side, and guided lists whose every edge is skipped:
    PSX_OK, zero counts, nothing else written -- no pair can exist, so no device is touched (this runs without one)"""
    L = capi.lib()
    good = capi.match_opts(0.8, True)
    fake = 0x1000
    window = capi.Guide.make(capi.GUIDE_HOMOGRAPHY, np.eye(3, dtype=np.float32).reshape(9), 2.0)
    for name in GRAPH + GUIDED_GRAPH:
        fn = getattr(L, name)
        guided = name in GUIDED_GRAPH

        def call(ptrs, lens, edges, guides):
            k, E = len(lens), len(edges)
            pa, la, ea, ptr = _arrays(ptrs, lens, edges)
            ga = (capi.Guide * max(E, 1))(*guides)
            sc = np.full(E + 2, -9, np.int32)
            buf = np.full(16, -7, np.int32)
            n = C.c_int(-5)
            head = (0, pa if k else None) + ((pa if k else None,) if guided else ()) + (ptr(la) if k else None, k, ptr(ea) if E else None, E)
            rc = fn(*head, *((ga if E else None,) if guided else ()), C.byref(good), ptr(buf), 4, ptr(sc) if E else None, C.byref(n))
            assert rc == 0 and n.value == 0 and list(sc) == [0] * E + [-9, -9] and np.all(buf == -7), (name, lens, edges)

        call((), (), (), ())
        call((fake, fake), (7, 9), (), ())
        call((fake, None, None), (9, 0, 0), ((0, 1), (1, 0), (2, 2), (1, 2)), (window,) * 4)
        call((None, None, None), (0, 0, 0), ((0, 0), (1, 2)), (window,) * 2)
        if guided:
            call((fake, fake), (7, 9), ((0, 1), (1, 0)), (capi.Guide.none(),) * 2)          # every edge skipped
        else:
            assert capi.match_graph_f32_last() == {"path": 0, "fell_back": 0, "launches": 0, "syncs": 0}
    for name in GUIDED_MANY:
        fn = getattr(L, name)
        for l_len, lens, guides in ((0, (5, 4), (window, window)), (3, (0, 0), (window, window)), (3, (5, 4), (capi.Guide.none(),) * 2), (3, (), ())):
            k = len(lens)
            pa, la, ga = (C.c_void_p * 2)(fake, fake), np.array(lens + (0,), np.int32), (capi.Guide * 2)(*(guides + (window, window))[:2])
            sc, buf, n = np.full(k + 2, -9, np.int32), np.full(16, -7, np.int32), C.c_int(-5)
            ptr = lambda a: a.ctypes.data_as(C.c_void_p)
            rc = fn(0, fake if l_len else None, fake if l_len else None, l_len, pa if k else None, pa if k else None, ptr(la) if k else None, k,
                    ga if k else None, C.byref(good), ptr(buf), 4, ptr(sc) if k else None, C.byref(n))
            assert rc == 0 and n.value == 0 and list(sc) == [0] * k + [-9, -9] and np.all(buf == -7), (name, l_len, lens)
    # the python wrappers' forms of the same (arrays without rows: nothing to upload)
    z, zx = np.zeros((0, 128), np.float32), np.zeros((0, 2), np.float32)
    lists, counts = capi.match_pairs_graph([z, z], [(0, 1), (1, 1)])
    assert [len(p) for p in lists] == [0, 0] and list(counts) == [0, 0] and lists[0].dtype == capi.PAIR_DTYPE
    lists, counts = capi.match_pairs_graph([], [])
    assert lists == [] and len(counts) == 0
    lists, counts = capi.match_pairs_guided_graph([z, z], [zx, zx], [(0, 1)], [window])
    assert [len(p) for p in lists] == [0] and list(counts) == [0]
    lists, counts = capi.match_pairs_guided_many(z, zx, [z, None], [zx, None], [window, None])
    assert [len(p) for p in lists] == [0, 0] and list(counts) == [0, 0]
    for mutual in (False, True):
        info = capi.match_graph_f32_plan((9, 0, 0), [(0, 1), (1, 0), (2, 2)], mutual)
        assert all(v == 0 for v in info.values()), info
        assert all(v == 0 for v in capi.match_graph_f32_plan((), [], mutual).values())


@pytest.mark.parametrize("lens,edges,mfma,path", fc.RULE_CASES, ids=[str(i) for i in range(len(fc.RULE_CASES))])
def test_path_rule_at_its_edges(capi, lens, edges, mfma, path):
    """255 x 4096 and 256 x 4095: the scan; 256 x 4096 and two edges of 256 x 2048: the prefilter; {256 x 4096, 1 x 1}: the
    scan, the mean left side is below 256; the switch off: the scan; no live edge: nothing runs"""
    for mutual in (False, True):
        info = capi.match_graph_f32_plan(lens, edges, mutual, mfma)
        assert info["path"] == path == fc.planned_path(lens, edges, mfma), (lens, edges, mfma, info)
        if path:
            assert info["launches"] == (2 if path == 2 else 1) + 2 * (2 if mutual else 1) + 3
    # for a star the rule is the one-to-many call's
    for nl, rl in ((300, (2000, 0, 2200)), (255, (5000,)), (256, (4000, 95)), (256, (4000, 96))):
        star = capi.match_graph_f32_plan((nl,) + rl, [(0, k + 1) for k in range(len(rl))])
        assert star["path"] == capi.match_many_f32_plan(nl, rl)["path"], (nl, rl)


@pytest.mark.parametrize("case", sorted(fc.PLAN_CASES), ids=sorted(fc.PLAN_CASES))
def test_plan_figures(capi, case):
    """what psx_match_graph_f32_plan reports equals what the documented rules give: the path, every referenced set cut once
    (unreferenced ones absent), the chunk length (the scan's at whatever <= 512 the library chose; the prefilter's the
    restated smallest length), items = blocks(outer) x chunks(inner) summed over the edges per direction, join workgroups,
    groups of whole edges under 256 MiB, launches, the bytes of the largest group.  The tables themselves are checked entry
    by entry by tests/cpp/match_graph_f32_plan_san.cpp on the same cases (test_plan_under_sanitizers)."""
    lens, edges = fc.PLAN_CASES[case]
    for mfma in (True, False):
        path = fc.planned_path(lens, edges, mfma)
        for mutual in (False, True):
            info = capi.match_graph_f32_plan(lens, edges, mutual, mfma)
            cl = info["chunk_len"]
            if path == 2:
                assert cl % 64 == 0 and 512 <= cl <= 4096
            else:
                assert cl % 32 == 0 and 32 <= cl <= 512
            want = fc.plan_restated(lens, edges, mutual, path)(cl)
            assert info == want, (case, mfma, mutual, info, want)
            print(case, "mfma", mfma, "mutual", mutual, info)
    expect = {"mixed": 1, "lefts": 1, "big": 2, "edges": 2, "tiny400": 1, "groups12": 2, "32x2048-all": 2, "16x4096-all": 2, "64x2048-next8": 2,
              "star64": 2, "one-18432": 2}
    assert fc.planned_path(lens, edges) == expect[case]
    info = capi.match_graph_f32_plan(lens, edges, True)
    if case == "groups12":
        assert info["fwd_groups"] == 2 and info["bwd_groups"] == 2 and info["launches"] == 13 and info["scratch_bytes"] == 11 * 5 * 18432 * 264
        assert capi.match_graph_f32_plan(lens, edges[:11], True)["fwd_groups"] == 1
    elif case == "16x4096-all":
        assert info["chunk_len"] == 4096 and info["chunks"] == 16 and info["fwd_items"] == 120 * 16       # one chunk per set
    elif case == "edges":
        assert info["referenced_sets"] == 17 and info["launches"] == 9
    elif case == "32x2048-all":
        assert info["referenced_sets"] == 32 and info["blocks"] == 256 and info["chunks"] == 32 and info["fwd_items"] == 496 * 8


def test_plan_ignores_what_no_live_edge_names(capi):
    """a set that no edge names, or that only faces an empty set, is absent: the plan is that of the remaining sets"""
    a = capi.match_graph_f32_plan((40, 50, 60, 0), [(1, 1), (0, 3)], True)
    b = capi.match_graph_f32_plan((50,), [(0, 0)], True)
    assert a == b and a["referenced_sets"] == 1 and a["blocks"] == 1 and a["path"] == 1
    # ... on the prefilter path too, and the rule counts live edges only: five dead edges do not lower the mean left side
    lens, edges = (300, 4100, 0, 70), [(0, 1), (0, 2), (2, 1), (2, 2), (3, 2), (2, 3)]
    a = capi.match_graph_f32_plan(lens, edges, True)
    b = capi.match_graph_f32_plan((300, 4100), [(0, 1)], True)
    assert a == b and a["path"] == 2 and a["referenced_sets"] == 2


def test_plan_under_sanitizers(tmp_path):
    """tests/cpp/match_graph_f32_plan_san.cpp: a stand-alone program (its own main) that includes match_graph_f32_plan.h
    alone and checks the tables, the groups, the rule and the int overflow refusals on exact-size heap arrays, compiled with
    -fsanitize=address,undefined and run directly."""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed"
    exe = str(tmp_path / "match_graph_f32_plan_san")
    cmd = [cxx, "-std=c++14", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           "-static-libasan", "-static-libubsan",
           os.path.join(ROOT, "tests", "cpp", "match_graph_f32_plan_san.cpp"), "-o", exe,
           "-I", os.path.join(ROOT, "popsift_amd", "csrc", "hip"), "-I", os.path.join(ROOT, "include")]
    subprocess.check_call(cmd)
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout


def test_cpp_match_graph_f32_api(tmp_path):
    """tests/cpp/test_match_graph_f32_api.cpp against libpopsift.so, built and run the way test_match_many_f32_api.cpp is:
    the three methods' signatures (static_assert), their throws and their empty forms -- no device is touched; the byte
    methods still refuse float descriptors."""
    libdir = os.path.join(ROOT, "popsift_amd", "lib")
    if not os.path.exists(os.path.join(libdir, "libpopsift.so")):
        from popsift_amd import build
        build.build_all()
    exe = str(tmp_path / "test_match_graph_f32_api")
    cmd = ["g++", "-std=c++14", "-O1", "-pthread", os.path.join(ROOT, "tests", "cpp", "test_match_graph_f32_api.cpp"), "-o", exe,
           "-I", os.path.join(ROOT, "popsift_amd", "csrc", "include"), "-I", os.path.join(ROOT, "include"),
           "-L", libdir, "-lpopsift", "-lpopsift_hip", "-Wl,-rpath," + libdir]
    subprocess.check_call(cmd)
    env = {k: v for k, v in os.environ.items() if k != "POPSIFT_TEST_EXPECT_GPU"}
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120, env=env)
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout
