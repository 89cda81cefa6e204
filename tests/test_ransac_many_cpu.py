"""CPU tests of the batched geometric verification's host side (include/popsift_hip.h, "geometric verification", MANY LISTS
IN ONE CALL): the declarations and bindings; the host references psx_ransac_*_many_ref against the loop of the single-list
references and the restatements of tests/ransac_cases.py / fundamental_cases.py; every argument error of all six entry
points, before a device is looked at and with the outputs untouched; the forms that need no device; the invariants of the
plan (psx_ransac_many_plan, csrc/hip/ransac_many_plan.h) at both block sizes; a stand-alone sanitizer build of the plan and
the host reference; the C++ API's argument errors."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import ransac_many_cases as mc
from tests.ransac_cases import bits, same_records, same_result

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE_ENTRIES = ("psx_ransac_homography_many", "psx_ransac_homography_many_dev", "psx_ransac_fundamental_many", "psx_ransac_fundamental_many_dev")
REF_ENTRIES = ("psx_ransac_homography_many_ref", "psx_ransac_fundamental_many_ref")


def test_entry_points_declared_and_bound(capi):
    hdr = open(os.path.join(ROOT, "include", "popsift_hip.h")).read()
    for sym in DEVICE_ENTRIES + REF_ENTRIES + ("psx_ransac_many_plan",):
        assert "int %s(" % sym in hdr and sym in capi.SYMBOLS and hasattr(capi.lib(), sym), sym
    assert "typedef struct psx_ransac_block { int set, first, end; }" in hdr
    for name in ("ransac_homography_many", "ransac_homography_many_dev", "ransac_homography_many_ref", "ransac_fundamental_many",
                 "ransac_fundamental_many_dev", "ransac_fundamental_many_ref", "ransac_many_plan"):
        assert callable(getattr(capi, name)), name
    from popsift_amd import build
    assert "ransac_many.hip" in build.HIP_SOURCES
    assert " ransac_many " in open(os.path.join(ROOT, "CMakeLists.txt")).read()
    hip = os.path.join(ROOT, "popsift_amd", "csrc", "hip")
    plan = open(os.path.join(hip, "ransac_many_plan.h")).read()
    assert "hip/hip_runtime.h" not in plan and "__global__" not in plan and "__device__" not in plan      # plain C++
    src = open(os.path.join(hip, "ransac_many.hip")).read()
    drv = open(os.path.join(hip, "ransac_graph.hip")).read()     # the one batched driver, for a star and for an edge list
    one = open(os.path.join(hip, "ransac.hip")).read()
    core = open(os.path.join(hip, "ransac_core.h")).read()
    assert '#include "ransac_many_plan.h"' in src and "psx_ransac_lists_run(" in src and "psx_ransac_many_args_ok(" in src
    for piece in ('#include "ransac_graph_plan.h"', '#include "ransac_core.h"', "wg_scan_totals(", "int psx_ransac_lists_run("):
        assert piece in drv, piece
    assert '#include "ransac_many_plan.h"' in open(os.path.join(hip, "ransac_graph_plan.h")).read()
    # the rule headers are used as they are: the device pieces call them, nothing is restated -- and the pieces stand once,
    # in the header that the single call's kernels use too
    assert '#include "ransac_core.h"' in one
    for piece in ("psx_ransac_sample(", "psx_ransac_sample_k<PSX_FUND_MIN>(", "psx_homography_fit_rule<4>(",
                  "psx_fundamental_fit_rule<PSX_FUND_MIN>(", "psx_guide_left(", "psx_guide_right("):
        assert core.count(piece) >= 1, piece
    for piece in ("psx_homography_fit_rule<4>(", "psx_fundamental_fit_rule<PSX_FUND_MIN>(", "psx_guide_left(", "psx_guide_right("):
        assert piece not in src and piece not in drv and piece not in one, piece
    pieces = ("r_gather(", "r_sample_fit<KIND>(", "r_score_walk<KIND, ", "r_select(", "r_keep<KIND>(", "r_decide<KIND>(")
    for piece in pieces:
        assert piece in drv and piece in one, piece
    # the batched sequence is stated once: the star form is an adapter without device code or a launch of its own
    for piece in pieces + ("wg_scan_totals(", "__global__", "__device__", "hipLaunchKernelGGL", "<<<", '#include "ransac_core.h"'):
        assert piece not in src, piece
    # ... and so is the host reference's loop over the single-list rule
    gplan = open(os.path.join(hip, "ransac_graph_plan.h")).read()
    assert plan.count("psx_ransac_many_rule(kind)") == 1 and "psx_ransac_many_rule(" not in gplan
    assert plan.count("inline int psx_ransac_lists_host(") == 1 and "return psx_ransac_lists_host(" in plan and "return psx_ransac_lists_host(" in gplan
    fh = open(os.path.join(ROOT, "popsift_amd", "csrc", "include", "popsift", "features.h")).read()
    assert "estimateHomographyMany(" in fh and "estimateFundamentalMany(" in fh


def _ref_loop(capi, model, c, opts):
    single = capi.ransac_fundamental_ref if model == "fundamental" else capi.ransac_homography_ref
    out = []
    for p, rxy in zip(c["lists"], c["right_xys"]):
        out.append(single(p, c["left_xy"], rxy, opts, layers=True))
    return out


@pytest.mark.parametrize("refit", [False, True], ids=["sample", "refit"])
@pytest.mark.parametrize("N,seed", mc.CONFIGS, ids=mc.CONFIG_IDS)
@pytest.mark.parametrize("model", mc.MODELS)
def test_many_ref_equals_the_loop_and_the_restatement(capi, model, N, seed, refit):
    c = mc.case(model, seed)
    want = mc.expect(model, N, seed, refit)
    if model == "fundamental" and (N, seed) == (65, 4) and refit:
        mc.premise(want, mc.expect(model, N, seed, False), c["sizes"])
    opts = capi.ransac_opts(mc.TOL, N, seed, refit)
    many = getattr(capi, "ransac_%s_many_ref" % model)
    got = many(c["lists"], c["left_xy"], c["right_xys"], opts, layers=True)
    loop = _ref_loop(capi, model, c, opts)
    K = len(c["sizes"])
    assert len(got["results"]) == K == len(got["inliers"]) and got["models"].shape == (K, N, 9) and got["counts"].shape == (K, N)
    for k, n in enumerate(c["sizes"]):
        r, w, one = got["results"][k], want[k], loop[k]
        assert same_result(r, w), (k, n, r.best, r.sample_inliers, r.inliers, w["best"])
        assert bytes(r) == bytes(one["result"]), (k, n)
        assert np.array_equal(bits(got["models"][k]), bits(w["models"])) and np.array_equal(got["counts"][k], w["counts"]), (k, n)
        if n >= mc.MIN[model]:
            assert np.array_equal(bits(got["models"][k]), bits(one["models"])) and np.array_equal(got["counts"][k], one["counts"])
        else:
            assert not got["models"][k].any() and not got["counts"][k].any() and r.best == -1
        assert same_records(got["inliers"][k], w["records"]) and same_records(got["inliers"][k], one["inliers"]), (k, n)
        assert r.guide(1.0).kind == (capi.GUIDE_EPIPOLAR if model == "fundamental" else capi.GUIDE_HOMOGRAPHY)
    cat = mc.concat([w["records"] for w in want])
    total = len(cat)
    assert got["count"] == total == sum(r.inliers for r in got["results"]) and same_records(got["records"], cat)
    starts = np.concatenate([[0], np.cumsum([r.inliers for r in got["results"]])])
    for k in range(K):
        assert same_records(cat[starts[k]:starts[k + 1]], want[k]["records"])
    # capacity total - 1, 0 with a buffer, 0 with NULL: the total is reported, the prefix written, nothing behind it
    L = capi.lib()
    fn = getattr(L, "psx_ransac_%s_many_ref" % model)
    pairs = mc.concat(c["lists"])
    sc = np.array(c["sizes"], np.int32)
    lens = np.array([len(r) for r in c["right_xys"]], np.int32)
    ptrs = (C.c_void_p * K)(*[r.ctypes.data if r.size else None for r in c["right_xys"]])
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    for cap, with_buf in ((total - 1, True), (0, True), (0, False)):
        out = np.full((cap + 2) * 4, -7, np.int32)
        res, cnt = (capi.RansacResult * K)(), C.c_int(-77)
        rv = fn(ptr(pairs), ptr(sc), K, ptr(c["left_xy"]), len(c["left_xy"]), ptrs, ptr(lens), C.byref(opts), res, ptr(out) if with_buf else None,
                cap, C.byref(cnt), None, None)
        assert rv == 0 and cnt.value == total, cap
        assert all(same_result(res[k], want[k]) for k in range(K))
        assert same_records(out[:4 * cap].view(pairs.dtype), cat[:cap]) and np.all(out[4 * cap:] == -7), cap


def _call(capi, fn, is_ref, **kw):
    """one call with sentinel-filled outputs and pointers that are never dereferenced on an error return (they are not
    device memory: this runs without a GPU); asserts that nothing was written and returns the return value"""
    fake = 0x1000
    a = dict(pairs=fake, counts=(9, 12), n_sets=2, left=fake, nl=40, ptrs=(fake, fake), lens=(30, 30), opts=capi.ransac_opts(2.0, 16, 0, True),
             results=True, out=True, cap=4, count=True)
    a.update(kw)
    K = 2 if a["counts"] is None else len(a["counts"])
    pa = (C.c_void_p * max(len(a["ptrs"]), 1))(*a["ptrs"]) if a["ptrs"] is not None else None
    sc = np.array(a["counts"], np.int32) if a["counts"] is not None else None
    la = np.array(a["lens"], np.int32) if a["lens"] is not None else None
    res = (capi.RansacResult * max(K, 1))()
    C.memset(res, 0x5a, C.sizeof(res))
    buf = np.full(32, -7, np.int32)
    models, hc = np.full((max(K, 1), 16, 9), -7, np.float32), np.full((max(K, 1), 16), -7, np.int32)
    n = C.c_int(-77)
    ptr = lambda x: x.ctypes.data_as(C.c_void_p) if x is not None else None
    args = [a["pairs"], ptr(sc), a["n_sets"], a["left"], a["nl"], pa, ptr(la), C.byref(a["opts"]) if a["opts"] is not None else None,
            res if a["results"] else None, ptr(buf) if a["out"] else None, a["cap"], C.byref(n) if a["count"] else None, ptr(models), ptr(hc)]
    rv = fn(*args) if is_ref else fn(0, *args)
    assert np.all(buf == -7) and np.all(models == -7) and np.all(hc == -7) and n.value == -77 and bytes(res) == b"\x5a" * C.sizeof(res)
    return rv


def test_argument_errors_touch_nothing(capi):
    """every PSX_ERR_INVALID of the header, with sentinels in every output, for the four device forms (before any device
    call: this runs without one) and the two host references"""
    L = capi.lib()
    nan, inf = float("nan"), float("inf")
    for name in DEVICE_ENTRIES + REF_ENTRIES:
        fn, is_ref = getattr(L, name), name in REF_ENTRIES
        call = lambda **kw: _call(capi, fn, is_ref, **kw)
        # everything the single call refuses
        for o in (capi.RansacOpts(nan, 16, 0, 0), capi.RansacOpts(-1.0, 16, 0, 0), capi.RansacOpts(inf, 16, 0, 0), capi.RansacOpts(2.0, 0, 0, 0),
                  capi.RansacOpts(2.0, 65537, 0, 0), capi.RansacOpts(2.0, 16, 0, 4)):
            assert call(opts=o) == -1, (name, o.tol, o.hypotheses, o.flags)
        assert call(opts=None) == -1, name
        assert call(count=False) == -1 and call(results=False) == -1, name
        assert call(nl=-1) == -1 and call(cap=-1) == -1, name
        assert call(out=False, cap=4) == -1, name                    # a capacity without a buffer
        assert call(pairs=None) == -1 and call(left=None) == -1, name   # NULL data with a non-zero size
        # the sets
        assert call(n_sets=-1) == -1, name
        assert call(counts=None) == -1 and call(ptrs=None) == -1 and call(lens=None) == -1, name
        assert call(counts=(9, -1)) == -1 and call(lens=(30, -1)) == -1, name
        assert call(ptrs=(0x1000, None)) == -1, name                 # a NULL right array whose set has pairs
        assert call(counts=(0x3fffffff, 1)) == -1, name              # the sum of the counts above 0x3fffffff
        assert call(counts=(0,) * 16385, ptrs=(None,) * 16385, lens=(0,) * 16385, n_sets=16385, opts=capi.ransac_opts(2.0, 65536, 0, True)) == -1, name
        if not is_ref:
            # a set with a model to estimate and an empty position array: no index can lie inside it
            assert call(nl=0, left=None) == -1 and call(lens=(30, 0)) == -1, name
    # the plan
    nb = C.c_int(-5)
    blk = np.full((4, 3), -7, np.int32)
    pb = blk.ctypes.data_as(C.c_void_p)
    for counts, n_sets, min_pairs, rows, tab, cap in (((9, -1), 2, 4, 256, pb, 4), ((0x3fffffff, 1), 2, 4, 256, pb, 4), ((9, 12), -1, 4, 256, pb, 4),
                                                      (None, 2, 4, 256, pb, 4), ((9, 12), 2, 0, 256, pb, 4), ((9, 12), 2, 4, 0, pb, 4),
                                                      ((9, 12), 2, 4, 256, None, 4), ((9, 12), 2, 4, 256, pb, -1)):
        sc = np.array(counts, np.int32) if counts is not None else None
        rv = L.psx_ransac_many_plan(sc.ctypes.data_as(C.c_void_p) if sc is not None else None, n_sets, min_pairs, rows, tab, cap, C.byref(nb))
        assert rv == -1 and nb.value == -5 and np.all(blk == -7), (counts, n_sets, min_pairs, rows, cap)
    sc = np.array((9, 12), np.int32)
    assert L.psx_ransac_many_plan(sc.ctypes.data_as(C.c_void_p), 2, 4, 256, pb, 4, None) == -1 and np.all(blk == -7)


def test_forms_without_a_model_need_no_device(capi):
    """n_sets = 0 and sets that are all below the minimum: PSX_OK, "no model" results, zero layers, no record -- no device
    is touched (this runs without one)"""
    L = capi.lib()
    fake = 0x1000
    opts = capi.ransac_opts(2.0, 8, 0, True)
    for name in DEVICE_ENTRIES:
        fn = getattr(L, name)
        n = C.c_int(-5)
        assert fn(0, None, None, 0, None, 0, None, None, C.byref(opts), None, None, 0, C.byref(n), None, None) == 0 and n.value == 0, name
        small = (3, 0, 2) if "homography" in name else (7, 0, 3)
        sc, lens = np.array(small, np.int32), np.array((5, 0, 5), np.int32)
        pa = (C.c_void_p * 3)(fake, None, fake)
        res = (capi.RansacResult * 4)()
        C.memset(res, 0x5a, C.sizeof(res))
        buf = np.full(16, -7, np.int32)
        models, hc = np.full((4, 8, 9), -7, np.float32), np.full((4, 8), -7, np.int32)
        n = C.c_int(-5)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)
        rv = fn(0, fake, ptr(sc), 3, fake, 9, pa, ptr(lens), C.byref(opts), res, ptr(buf), 4, C.byref(n), ptr(models), ptr(hc))
        assert rv == 0 and n.value == 0 and np.all(buf == -7), name
        for k in range(3):
            assert res[k].best == -1 and res[k].inliers == 0 and res[k].sample_inliers == 0 and not res[k].matrix().any(), (name, k)
        assert bytes(res[3]) == b"\x5a" * C.sizeof(capi.RansacResult)
        assert not models[:3].any() and not hc[:3].any() and np.all(models[3] == -7) and np.all(hc[3] == -7), name
    # the python wrappers' form of the same (no list at all, lists without a model: nothing to verify)
    got = capi.ransac_fundamental_many_ref([], np.zeros((0, 2), np.float32), [])
    assert got["results"] == [] and got["count"] == 0 and got["inliers"] == []


@pytest.mark.parametrize("rows", [512, 256])
@pytest.mark.parametrize("min_pairs", [4, 8])
@pytest.mark.parametrize("counts", [mc.SIZES["fundamental"], mc.SIZES["homography"], (4000,) * 8, (500,) * 64, (1000,) * 16, (0, 0), (3,), ()],
                         ids=["F", "H", "8x4000", "64x500", "16x1000", "empty", "short", "none"])
def test_plan_invariants(capi, counts, min_pairs, rows):
    """every pair of every set at or above the minimum is covered exactly once, nothing spans two sets, the order is
    ascending, smaller sets contribute nothing -- at the score kernel's block size and at the compaction's"""
    blocks = capi.ransac_many_plan(counts, min_pairs, rows)
    first = np.concatenate([[0], np.cumsum(np.array(counts, np.int64))]).astype(np.int64)
    cover = np.zeros(int(first[-1]), np.int32)
    for b, (s, p0, p1) in enumerate(blocks):
        assert 0 <= s < len(counts) and counts[s] >= min_pairs
        assert first[s] <= p0 < p1 <= first[s + 1] and p1 - p0 <= rows
        if b and blocks[b - 1][0] == s:
            assert p0 == blocks[b - 1][2] and blocks[b - 1][2] - blocks[b - 1][1] == rows        # contiguous, only a set's last block is short
        else:
            assert p0 == first[s] and (b == 0 or blocks[b - 1][0] < s)
        cover[p0:p1] += 1
    for s, n in enumerate(counts):
        assert np.all(cover[first[s]:first[s + 1]] == (1 if n >= min_pairs else 0)), s
    assert len(blocks) == sum((n + rows - 1) // rows for n in counts if n >= min_pairs)
    # a smaller capacity: the total is still reported, the prefix is the same, nothing is written past it
    if len(blocks) > 1:
        L = capi.lib()
        sc = np.array(counts, np.int32)
        part = np.full((len(blocks), 3), -7, np.int32)
        nb = C.c_int(-1)
        assert L.psx_ransac_many_plan(sc.ctypes.data_as(C.c_void_p), len(sc), min_pairs, rows, part.ctypes.data_as(C.c_void_p), len(blocks) - 1, C.byref(nb)) == 0
        assert nb.value == len(blocks) and np.array_equal(part[:-1], blocks[:-1]) and np.all(part[-1] == -7)


def test_plan_and_host_reference_under_sanitizers(tmp_path):
    """tests/cpp/ransac_many_plan_san.cpp: a stand-alone program (its own main) that includes ransac_many_plan.h and the host
    rule headers alone and runs the plan and a three-set host reference on exact-size heap arrays -- compiled with
    -ffp-contract=off -fsanitize=address,undefined and run directly."""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed"
    exe = str(tmp_path / "ransac_many_plan_san")
    cmd = [cxx, "-std=c++14", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan",
           os.path.join(ROOT, "tests", "cpp", "ransac_many_plan_san.cpp"), "-o", exe,
           "-I", os.path.join(ROOT, "popsift_amd", "csrc", "hip"), "-I", os.path.join(ROOT, "include")]
    subprocess.check_call(cmd)
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout


def test_cpp_api_argument_errors_without_a_device(tmp_path):
    """tests/cpp/test_ransac_many_api.cpp without POPSIFT_TEST_EXPECT_GPU: estimate*Many's and the C-ABI's argument checks and
    the "no model" forms, all before a device is touched"""
    libdir = os.path.join(ROOT, "popsift_amd", "lib")
    exe = str(tmp_path / "test_ransac_many_api")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-pthread", os.path.join(ROOT, "tests", "cpp", "test_ransac_many_api.cpp"), "-o", exe,
                           "-I", os.path.join(ROOT, "popsift_amd", "csrc", "include"), "-I", os.path.join(ROOT, "include"),
                           "-L", libdir, "-lpopsift", "-lpopsift_hip", "-Wl,-rpath," + libdir])
    env = {k: v for k, v in os.environ.items() if k != "POPSIFT_TEST_EXPECT_GPU"}
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120, env=env)
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout
