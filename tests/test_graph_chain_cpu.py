"""CPU tests of the two edge-list calls behind psx_match_pairs_graph_u8 (include/popsift_hip.h, "A LIST OF VIEW PAIRS IN ONE
CALL"): the declarations and bindings of psx_ransac_*_graph* and psx_match_pairs_guided_graph_u8*; the host references
psx_ransac_*_graph_ref against the loop of the single-list references, all four models; every argument error of both
families, before a device is looked at and with the outputs untouched; the forms that need no device; the block tables
over the edges' counts; a stand-alone sanitizer build of the two plan headers, which checks the guided call's tables
themselves; the C++ API's argument errors."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import graph_chain_cases as gc
from tests import ransac_many_cases as mc
from tests.ransac_cases import bits, same_records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_MAX = 2 ** 31 - 1
RANSAC_DEVICE = tuple("psx_ransac_%s_graph%s" % (m, s) for m in gc.MODELS for s in ("", "_dev"))
RANSAC_REF = tuple("psx_ransac_%s_graph_ref" % m for m in gc.MODELS)
GUIDED = ("psx_match_pairs_guided_graph_u8", "psx_match_pairs_guided_graph_u8_dev")


def test_entry_points_declared_and_bound(capi):
    hdr = open(os.path.join(ROOT, "include", "popsift_hip.h")).read()
    for sym in RANSAC_DEVICE + RANSAC_REF + GUIDED:
        assert "int %s(" % sym in hdr and sym in capi.SYMBOLS and hasattr(capi.lib(), sym), sym
    assert len(RANSAC_DEVICE + RANSAC_REF) == 12
    for m in gc.MODELS:
        for s in ("_graph", "_graph_dev", "_graph_ref"):
            assert callable(getattr(capi, "ransac_%s%s" % (m, s))), (m, s)
    assert callable(capi.match_pairs_guided_graph_u8) and callable(capi.match_pairs_guided_graph_dev)
    from popsift_amd import build
    cm = open(os.path.join(ROOT, "CMakeLists.txt")).read()
    for unit in ("ransac_graph", "match_guided_graph"):
        assert unit + ".hip" in build.HIP_SOURCES and " %s " % unit in cm, unit
    hip = os.path.join(ROOT, "popsift_amd", "csrc", "hip")
    for plan in ("ransac_graph_plan.h", "match_guided_graph_plan.h"):
        text = open(os.path.join(hip, plan)).read()
        assert "hip/hip_runtime.h" not in text and "__global__" not in text and "__device__" not in text, plan      # plain C++
    rsrc = open(os.path.join(hip, "ransac_graph.hip")).read()
    for piece in ('#include "ransac_graph_plan.h"', '#include "ransac_core.h"', "psx_ransac_many_blocks(", "wg_scan_totals(", "r_gather(",
                  "r_sample_fit<KIND>(", "r_score_walk<KIND, ", "r_select(", "r_keep<KIND>(", "r_decide<KIND>("):
        assert piece in rsrc, piece
    for piece in ("psx_homography_fit_rule<4>(", "psx_fundamental_fit_rule<PSX_FUND_MIN>(", "psx_guide_left(", "psx_guide_right("):
        assert piece not in rsrc, piece                      # no rule is restated
    gsrc = open(os.path.join(hip, "match_guided_graph.hip")).read()
    for piece in ('#include "match_guided_graph_plan.h"', '#include "match_guided_core.h"', "g_match_row<unsigned char, int, false>(",
                  "g_match_row<unsigned char, int, true>(", "psx_match_keep", "wg_scan_totals"):
        assert piece in gsrc, piece
    assert "atomic" not in gsrc.split("#include")[-1]        # the code, not the header comment: nothing depends on arrival order
    scratch = open(os.path.join(hip, "match_scratch.h")).read()
    for slot in ("MS_GGRAPH_TABLES", "MS_GGRAPH_LINES", "MS_GGRAPH_FWD", "MS_GGRAPH_BWD", "MS_GGRAPH_TOT"):
        assert slot in scratch and slot in gsrc, slot
    assert "MS_GMANY_" not in gsrc and "MS_GRAPH_" not in gsrc and "MS_GUIDED_" not in gsrc
    assert "MS_RGRAPH_TABLES" in scratch and "MS_RGRAPH_TABLES" in rsrc and "MS_RMANY_TABLES" not in rsrc
    # the star forms run these two drivers: their own scratch slots are gone from every file
    for name in sorted(os.listdir(hip)):
        text = open(os.path.join(hip, name)).read()
        assert "MS_RMANY_TABLES" not in text and "MS_GMANY_" not in text, name
    fh = open(os.path.join(ROOT, "popsift_amd", "csrc", "include", "popsift", "features.h")).read()
    for name in ("estimateHomographyGraph(", "estimateFundamentalGraph(", "estimateAffineGraph(", "estimateSimilarityGraph(", "matchPairsGuidedGraph("):
        assert name in fh, name
    # the docs no longer say the chain stops at a star
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "Verify and re-match a list of view pairs" in doc
    assert "no guided or RANSAC call over an edge list" not in hdr and "a guided or RANSAC call over an edge list" not in doc


def _single_ref(capi, model, pairs, lxy, rxy, opts):
    return capi.ransac_homography_ref(pairs, lxy, rxy, opts, layers=True, model=model)


@pytest.mark.parametrize("refit", [False, True], ids=["sample", "refit"])
@pytest.mark.parametrize("N,seed", mc.CONFIGS, ids=mc.CONFIG_IDS)
@pytest.mark.parametrize("model", gc.MODELS)
def test_graph_ref_equals_the_loop_of_single_references(capi, model, N, seed, refit):
    c = gc.ransac_case(model)
    opts = capi.ransac_opts(gc.TOL, N, seed, refit)
    got = getattr(capi, "ransac_%s_graph_ref" % model)(c["lists"], c["edges"], c["xys"], opts, layers=True)
    E = len(c["edges"])
    assert len(got["results"]) == E == len(got["inliers"]) and got["models"].shape == (E, N, 9) and got["counts"].shape == (E, N)
    loop = [_single_ref(capi, model, c["lists"][e], c["xys"][a], c["xys"][b], opts) for e, (a, b) in enumerate(c["edges"])]
    with_model = 0
    for e, n in enumerate(c["counts"]):
        r, one = got["results"][e], loop[e]
        assert bytes(r) == bytes(one["result"]), (e, n, r.best, one["result"].best)
        assert same_records(got["inliers"][e], one["inliers"]), (e, n)
        if n >= gc.MIN[model]:
            assert np.array_equal(bits(got["models"][e]), bits(one["models"])) and np.array_equal(got["counts"][e], one["counts"]), (e, n)
        else:
            assert r.best == -1 and r.inliers == 0 and not got["models"][e].any() and not got["counts"][e].any(), (e, n)
        with_model += r.best >= 0 and r.inliers >= gc.MIN[model]
    assert with_model >= 6, "the planted edges have models"
    d0, d1 = gc.DUPLICATE
    assert bytes(got["results"][d0]) == bytes(got["results"][d1]) and same_records(got["inliers"][d0], got["inliers"][d1])
    # the edges have different models: no two results of planted edges agree
    planted = [e for e in range(E) if c["counts"][e] >= 255 and e != d0]
    assert len({bytes(got["results"][e]) for e in planted}) == len(planted)
    cat = gc.concat([one["inliers"] for one in loop])
    total = len(cat)
    assert got["count"] == total == sum(r.inliers for r in got["results"]) and same_records(got["records"], cat)
    # capacity inside an edge, 0 with a buffer, 0 with NULL: the total is reported, the prefix written, nothing behind it
    first = got["results"][0].inliers
    assert first > 1 and got["results"][1].inliers > 1
    fn = getattr(capi.lib(), "psx_ransac_%s_graph_ref" % model)
    pairs = gc.concat(c["lists"])
    ec, la, ea = np.array(c["counts"], np.int32), np.array(c["lens"], np.int32), np.array(c["edges"], np.int32)
    ptrs = (C.c_void_p * len(c["xys"]))(*[x.ctypes.data if x.size else None for x in c["xys"]])
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    for cap, with_buf in ((first + 1, True), (0, True), (0, False)):
        out = np.full((cap + 2) * 4, -7, np.int32)
        res, cnt = (capi.RansacResult * E)(), C.c_int(-77)
        rv = fn(ptr(pairs), ptr(ec), ptr(ea), E, ptrs, ptr(la), len(la), C.byref(opts), res, ptr(out) if with_buf else None, cap, C.byref(cnt),
                None, None)
        assert rv == 0 and cnt.value == total, cap
        assert all(bytes(res[e]) == bytes(loop[e]["result"]) for e in range(E))
        assert same_records(out[:4 * cap].view(pairs.dtype), cat[:cap]) and np.all(out[4 * cap:] == -7), cap
    # a bad index in the last edge -- in range for the longest view, outside its own -- refuses the call; nothing is written
    lists = [p.copy() for p in c["lists"]]
    lists[-1]["left"][5] = c["lens"][c["edges"][-1][0]]
    assert lists[-1]["left"][5] < max(c["lens"])
    bad = gc.concat(lists)
    out = np.full(8, -7, np.int32)
    res, cnt = (capi.RansacResult * E)(), C.c_int(-77)
    C.memset(res, 0x5a, C.sizeof(res))
    assert fn(ptr(bad), ptr(ec), ptr(ea), E, ptrs, ptr(la), len(la), C.byref(opts), res, ptr(out), 2, C.byref(cnt), None, None) == -1
    assert cnt.value == -77 and np.all(out == -7) and bytes(res) == b"\x5a" * C.sizeof(res)


def _ransac_call(capi, fn, is_ref, **kw):
    """one call with sentinel-filled outputs and pointers that are never dereferenced on an error return (they are not
    device memory: this runs without a GPU); asserts that nothing was written and returns the return value"""
    fake = 0x1000
    a = dict(pairs=fake, counts=(9, 12), edges=((0, 1), (2, 0)), n_edges=2, ptrs=(fake, fake, fake), lens=(40, 30, 30), n_sets=3,
             opts=capi.ransac_opts(2.0, 16, 0, True), results=True, out=True, cap=4, count=True)
    a.update(kw)
    E = 2 if a["counts"] is None else len(a["counts"])
    pa = (C.c_void_p * max(len(a["ptrs"]), 1))(*a["ptrs"]) if a["ptrs"] is not None else None
    ec = np.array(a["counts"], np.int32) if a["counts"] is not None else None
    ea = np.array(a["edges"], np.int32).reshape(-1, 2) if a["edges"] is not None else None
    la = np.array(a["lens"], np.int32) if a["lens"] is not None else None
    res = (capi.RansacResult * max(E, 1))()
    C.memset(res, 0x5a, C.sizeof(res))
    buf = np.full(32, -7, np.int32)
    models, hc = np.full((max(E, 1), 16, 9), -7, np.float32), np.full((max(E, 1), 16), -7, np.int32)
    n = C.c_int(-77)
    ptr = lambda x: x.ctypes.data_as(C.c_void_p) if x is not None else None
    args = [a["pairs"], ptr(ec), ptr(ea), a["n_edges"], pa, ptr(la), a["n_sets"], C.byref(a["opts"]) if a["opts"] is not None else None,
            res if a["results"] else None, ptr(buf) if a["out"] else None, a["cap"], C.byref(n) if a["count"] else None, ptr(models), ptr(hc)]
    rv = fn(*args) if is_ref else fn(0, *args)
    assert np.all(buf == -7) and np.all(models == -7) and np.all(hc == -7) and n.value == -77 and bytes(res) == b"\x5a" * C.sizeof(res)
    return rv


def test_ransac_argument_errors_touch_nothing(capi):
    """every PSX_ERR_INVALID of the header, with sentinels in every output, for the eight device forms (before any device
    call: this runs without one) and the four host references"""
    L = capi.lib()
    nan, inf = float("nan"), float("inf")
    for name in RANSAC_DEVICE + RANSAC_REF:
        fn, is_ref = getattr(L, name), name in RANSAC_REF
        call = lambda **kw: _ransac_call(capi, fn, is_ref, **kw)
        # everything the batched form refuses
        for o in (capi.RansacOpts(nan, 16, 0, 0), capi.RansacOpts(-1.0, 16, 0, 0), capi.RansacOpts(inf, 16, 0, 0), capi.RansacOpts(2.0, 0, 0, 0),
                  capi.RansacOpts(2.0, 65537, 0, 0), capi.RansacOpts(2.0, 16, 0, 4)):
            assert call(opts=o) == -1, (name, o.tol, o.hypotheses, o.flags)
        assert call(opts=None) == -1, name
        assert call(count=False) == -1 and call(results=False) == -1, name
        assert call(cap=-1) == -1 and call(out=False, cap=4) == -1, name
        assert call(pairs=None) == -1, name
        assert call(n_edges=-1) == -1 and call(counts=None) == -1, name
        assert call(counts=(9, -1)) == -1, name
        assert call(counts=(0x3fffffff, 1)) == -1, name              # the sum of the counts above 0x3fffffff
        assert call(counts=(0,) * 16385, edges=((0, 1),) * 16385, n_edges=16385, opts=capi.ransac_opts(2.0, 65536, 0, True)) == -1, name
        # everything the graph matcher refuses about lens, n_sets, edges and n_edges
        assert call(n_sets=-1) == -1 and call(lens=None) == -1 and call(edges=None) == -1 and call(ptrs=None) == -1, name
        assert call(lens=(40, -1, 30)) == -1, name
        for bad in ((0, 3), (3, 0), (-1, 0), (0, -1), (INT_MAX, 0)):
            assert call(edges=((0, 1), bad)) == -1, (name, bad)      # every edge is checked, not only the first
        assert call(ptrs=None, lens=None, n_sets=0) == -1, name      # no sets: no edge is in range
        assert call(lens=(2 ** 30, 5, 4), edges=((0, 1), (0, 2), (0, 0)), counts=(9, 12, 1), n_edges=3) == -1, name      # sum of lens[left]
        assert call(lens=(5, 2 ** 30, 4), edges=((0, 1), (2, 1), (1, 1)), counts=(9, 12, 1), n_edges=3) == -1, name      # ... of lens[right]
        # the position arrays
        assert call(ptrs=(0x1000, None, 0x1000)) == -1, name         # a NULL array with a length
        assert call(ptrs=(0x1000, None, 0x1000), lens=(40, 0, 30), counts=(1, 12)) == -1, name     # ... under an edge that has pairs
        if not is_ref:
            # an edge with a model to estimate and an empty position array: no index can lie inside it
            assert call(lens=(40, 0, 30)) == -1 and call(lens=(0, 30, 30)) == -1, name


def test_ransac_forms_without_a_model_need_no_device(capi):
    """n_edges = 0 and edges that are all below the minimum: PSX_OK, "no model" results, zero layers, no record -- no device is
    touched (this runs without one)"""
    L = capi.lib()
    fake = 0x1000
    opts = capi.ransac_opts(2.0, 8, 0, True)
    for name in RANSAC_DEVICE:
        fn = getattr(L, name)
        model = name.split("_")[2]
        n = C.c_int(-5)
        assert fn(0, None, None, None, 0, None, None, 0, C.byref(opts), None, None, 0, C.byref(n), None, None) == 0 and n.value == 0, name
        m = gc.MIN[model]
        ec, la, ea = np.array((m - 1, 0, m - 1), np.int32), np.array((5, 0, 5), np.int32), np.array(((0, 2), (1, 1), (2, 0)), np.int32)
        pa = (C.c_void_p * 3)(fake, None, fake)
        res = (capi.RansacResult * 4)()
        C.memset(res, 0x5a, C.sizeof(res))
        buf = np.full(16, -7, np.int32)
        models, hc = np.full((4, 8, 9), -7, np.float32), np.full((4, 8), -7, np.int32)
        n = C.c_int(-5)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)
        rv = fn(0, fake, ptr(ec), ptr(ea), 3, pa, ptr(la), 3, C.byref(opts), res, ptr(buf), 4, C.byref(n), ptr(models), ptr(hc))
        assert rv == 0 and n.value == 0 and np.all(buf == -7), name
        for e in range(3):
            assert res[e].best == -1 and res[e].inliers == 0 and res[e].sample_inliers == 0 and not res[e].matrix().any(), (name, e)
        assert bytes(res[3]) == b"\x5a" * C.sizeof(capi.RansacResult)
        assert not models[:3].any() and not hc[:3].any() and np.all(models[3] == -7) and np.all(hc[3] == -7), name
    got = capi.ransac_fundamental_graph_ref([], [], [])
    assert got["results"] == [] and got["count"] == 0 and got["inliers"] == []


@pytest.mark.parametrize("rows", [512, 256])
@pytest.mark.parametrize("model", gc.MODELS)
def test_blocks_never_cross_an_edge(capi, model, rows):
    """the block tables the edge-list call walks are psx_ransac_many_blocks over the edges' counts: every pair of every edge
    at or above the minimum is covered once, nothing spans two edges, an edge below the minimum has no block"""
    counts = gc.pair_counts(model)
    blocks = capi.ransac_many_plan(counts, gc.MIN[model], rows)
    first = np.concatenate([[0], np.cumsum(np.array(counts, np.int64))])
    cover = np.zeros(int(first[-1]), np.int32)
    for s, p0, p1 in blocks:
        assert counts[s] >= gc.MIN[model] and first[s] <= p0 < p1 <= first[s + 1] and p1 - p0 <= rows
        cover[p0:p1] += 1
    for e, n in enumerate(counts):
        assert np.all(cover[first[e]:first[e + 1]] == (1 if n >= gc.MIN[model] else 0)), e
    assert len(blocks) == sum((n + rows - 1) // rows for n in counts if n >= gc.MIN[model])


def _guided_call(capi, fn, **kw):
    fake = 0x1000
    a = dict(sets=(fake, fake, fake), xys=(fake, fake, fake), lens=(3, 5, 4), n_sets=3, edges=((0, 1), (2, 0)), n_edges=2,
             guides=(capi.Guide.homography(np.eye(3), 2.0), capi.Guide.none()), opts=capi.match_opts(0.8, True), out=True, cap=2, counts=True,
             count=True)
    a.update(kw)
    arr = lambda p: (C.c_void_p * max(len(p), 1))(*p) if p is not None else None
    la = np.array(a["lens"], np.int32) if a["lens"] is not None else None
    ea = np.array(a["edges"], np.int32).reshape(-1, 2) if a["edges"] is not None else None
    ga = (capi.Guide * max(len(a["guides"]), 1))(*a["guides"]) if a["guides"] is not None else None
    buf = np.full(16, -7, np.int32)
    sc = np.full(8, -9, np.int32)
    n = C.c_int(-5)
    ptr = lambda x: x.ctypes.data_as(C.c_void_p) if x is not None else None
    rc = fn(0, arr(a["sets"]), arr(a["xys"]), ptr(la), a["n_sets"], ptr(ea), a["n_edges"], ga, C.byref(a["opts"]) if a["opts"] is not None else None,
            ptr(buf) if a["out"] else None, a["cap"], ptr(sc) if a["counts"] else None, C.byref(n) if a["count"] else None)
    assert np.all(buf == -7) and np.all(sc == -9) and n.value == -5
    return rc


def test_guided_argument_errors_touch_nothing(capi):
    """every PSX_ERR_INVALID of the header, with sentinels in every output; the fake non-NULL "device" pointers are never
    dereferenced (this runs without a GPU)"""
    L = capi.lib()
    fake = 0x1000
    nan, inf = float("nan"), float("inf")
    H = capi.Guide.homography(np.eye(3), 2.0)
    for name in GUIDED:
        fn = getattr(L, name)
        call = lambda **kw: _guided_call(capi, fn, **kw)
        # everything psx_match_pairs_graph_u8 refuses
        for o in (capi.MatchOpts(nan, 0), capi.MatchOpts(0.0, 0), capi.MatchOpts(-0.5, 0), capi.MatchOpts(-inf, 0), capi.MatchOpts(0.8, 2),
                  capi.MatchOpts(0.8, -1)):
            assert call(opts=o) == -1, (name, o.ratio, o.flags)
        assert call(opts=None) == -1 and call(count=False) == -1 and call(cap=-1) == -1 and call(out=False, cap=2) == -1, name
        assert call(n_sets=-1) == -1 and call(n_edges=-1) == -1, name
        assert call(sets=None) == -1 and call(lens=None) == -1 and call(edges=None) == -1 and call(counts=False) == -1, name
        assert call(lens=(3, -1, 4)) == -1, name
        assert call(sets=(fake, None, fake)) == -1, name
        assert call(sets=(fake, fake, None), edges=((0, 1), (0, 1))) == -1, name       # ... even when no edge names it
        for bad in ((0, 3), (3, 0), (-1, 0), (0, -1), (INT_MAX, 0)):
            assert call(edges=((0, 1), bad)) == -1, (name, bad)
        assert call(sets=None, xys=None, lens=None, n_sets=0) == -1, name
        g3 = (H, H, H)
        assert call(lens=(2 ** 30, 5, 4), edges=((0, 1), (0, 2), (0, 0)), n_edges=3, guides=g3) == -1, name       # the sum of lens[left]
        assert call(lens=(5, 2 ** 30, 4), edges=((0, 1), (2, 1), (1, 1)), n_edges=3, guides=g3) == -1, name       # ... of lens[right]
        # the positions and the guides
        assert call(xys=None) == -1 and call(xys=(fake, None, fake)) == -1 and call(guides=None) == -1, name
        for g in (capi.Guide.make(3, np.eye(3).reshape(9), 2.0), capi.Guide.make(-1, np.eye(3).reshape(9), 2.0),
                  capi.Guide.make(1, np.eye(3).reshape(9), -1.0), capi.Guide.make(1, np.eye(3).reshape(9), nan),
                  capi.Guide.make(2, np.eye(3).reshape(9), inf), capi.Guide.make(1, np.full(9, nan), 2.0), capi.Guide.make(2, np.full(9, inf), 2.0)):
            assert call(guides=(H, g)) == -1, (name, g.kind, g.tol)                     # every guide is checked, not only the first
            assert call(guides=(H, g), lens=(3, 5, 0)) == -1, name                      # ... of an edge with an empty side too


def test_guided_empty_and_skipped_forms_need_no_device(capi):
    """n_edges = 0 and lists whose every edge is skipped or has an empty side: PSX_OK and zero counts, nothing else written
    and no device touched (this runs without one); a skipped edge's guide is not looked at"""
    L = capi.lib()
    good = capi.match_opts(0.8, True)
    fake = 0x1000
    H = capi.Guide.homography(np.eye(3), 2.0)
    junk = capi.Guide.make(0, np.full(9, float("nan")), -3.0)          # kind 0: the rest is not looked at
    for name in GUIDED:
        fn = getattr(L, name)
        n = C.c_int(-5)
        assert fn(0, None, None, None, 0, None, 0, None, C.byref(good), None, 0, None, C.byref(n)) == 0 and n.value == 0, name
        for ptrs, lens, edges, guides in (((fake, None, None), (9, 0, 0), ((0, 1), (1, 0), (2, 2), (0, 0)), (H, H, H, junk)),
                                          ((fake, fake, fake), (9, 7, 5), ((0, 1), (1, 2), (2, 0)), (junk, capi.Guide.none(), junk))):
            pa = (C.c_void_p * 3)(*ptrs)
            la, ea = np.array(lens, np.int32), np.array(edges, np.int32)
            ga = (capi.Guide * len(guides))(*guides)
            sc = np.full(len(edges) + 2, -9, np.int32)
            buf = np.full(16, -7, np.int32)
            n = C.c_int(-5)
            rc = fn(0, pa, pa, la.ctypes.data_as(C.c_void_p), 3, ea.ctypes.data_as(C.c_void_p), len(edges), ga, C.byref(good),
                    buf.ctypes.data_as(C.c_void_p), 4, sc.ctypes.data_as(C.c_void_p), C.byref(n))
            assert rc == 0 and n.value == 0 and list(sc) == [0] * len(edges) + [-9, -9] and np.all(buf == -7), (name, lens)
    lists, counts = capi.match_pairs_guided_graph_u8([np.zeros((0, 128), np.uint8)] * 2, [np.zeros((0, 2), np.float32)] * 2, [(0, 1)], [H])
    assert len(lists) == 1 and len(lists[0]) == 0 and list(counts) == [0]


def test_plans_and_host_reference_under_sanitizers(tmp_path):
    """tests/cpp/graph_chain_plan_san.cpp: a stand-alone program (its own main) that includes ransac_graph_plan.h and
    match_guided_graph_plan.h alone and runs the host reference and the table builders on exact-size heap arrays --
    compiled with -ffp-contract=off -fsanitize=address,undefined and run directly"""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed"
    exe = str(tmp_path / "graph_chain_plan_san")
    cmd = [cxx, "-std=c++14", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan",
           os.path.join(ROOT, "tests", "cpp", "graph_chain_plan_san.cpp"), "-o", exe,
           "-I", os.path.join(ROOT, "popsift_amd", "csrc", "hip"), "-I", os.path.join(ROOT, "include")]
    subprocess.check_call(cmd)
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout


def test_cpp_api_argument_errors_without_a_device(tmp_path):
    """tests/cpp/test_graph_chain_api.cpp without POPSIFT_TEST_EXPECT_GPU: the argument checks and the empty forms of
    estimate*Graph and matchPairsGuidedGraph, all before a device is touched"""
    libdir = os.path.join(ROOT, "popsift_amd", "lib")
    exe = str(tmp_path / "test_graph_chain_api")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-pthread", os.path.join(ROOT, "tests", "cpp", "test_graph_chain_api.cpp"), "-o", exe,
                           "-I", os.path.join(ROOT, "popsift_amd", "csrc", "include"), "-I", os.path.join(ROOT, "include"),
                           "-L", libdir, "-lpopsift", "-lpopsift_hip", "-Wl,-rpath," + libdir])
    env = {k: v for k, v in os.environ.items() if k != "POPSIFT_TEST_EXPECT_GPU"}
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120, env=env)
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout
