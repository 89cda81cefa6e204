"""CPU tests of geometric verification's host side (include/popsift_hip.h, "geometric verification"): psx_ransac_samples,
psx_homography_fit and psx_ransac_homography_ref -- which share csrc/hip/ransac_rule.h with the kernels -- against the
independent restatement of tests/ransac_cases.py, bit for bit; the premises of the planted inputs; argument errors with
nothing written; and a stand-alone sanitizer build of the rule.

The premises (asserted in test_premises_of_the_planted_inputs, from the restatement alone, at tol 2): no hypothesis of any
shape has a non-finite model; (4, 8, 1) has all eight hypotheses tied at 4 inliers and (5, 64, 2) has 17 tied at 4, the
lowest of them h = 1; every other shape has a unique winner; the refit is kept everywhere; and the refit model recovers
(63, 64, 3): 38 of 39 planted pairs, (64, 65, 4): 37 of 39, (65, 64, 5): 39 of 39, (129, 128, 6): 77 of 78, (300, 256, 7): 180
of 180, (2500, 512, 8): 1500 of 1500, (1023, 8, 9): 595 of 615, (1024, 8, 9): 615 of 615, (1025, 8, 32): 590 of 615 and, from
its one hypothesis of 5 inliers, (65, 1, 10): 15 of 39."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import ransac_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (n, N, seed) -> (best, its count, hypotheses at that count, inliers after the refit, planted pairs among them, planted pairs)
PREMISES = {(4, 8, 1): (0, 4, 8, 4, 4, 4), (5, 64, 2): (1, 4, 17, 4, 3, 3), (63, 64, 3): (49, 31, 1, 38, 38, 39),
            (64, 65, 4): (14, 37, 1, 37, 37, 39), (65, 64, 5): (40, 39, 1, 39, 39, 39), (129, 128, 6): (27, 66, 1, 77, 77, 78),
            (300, 256, 7): (229, 170, 1, 180, 180, 180), (2500, 512, 8): (361, 1500, 1, 1500, 1500, 1500),
            (1023, 8, 9): (0, 401, 1, 595, 595, 615), (1024, 8, 9): (7, 538, 1, 615, 615, 615),
            (1025, 8, 32): (1, 268, 1, 590, 590, 615), (65, 1, 10): (0, 5, 1, 15, 15, 39)}


@pytest.mark.parametrize("n,N,seed", rc.SHAPES, ids=rc.SHAPE_IDS)
def test_samples_equal_the_restatement(capi, n, N, seed):
    if n < 4:
        L = capi.lib()
        buf = np.full(4 * N, -7, np.int32)
        assert L.psx_ransac_samples(seed, 0, N, n, buf.ctypes.data_as(C.c_void_p)) == -1 and np.all(buf == -7)
        return
    got = capi.ransac_samples(seed, 0, N, n)
    assert got.tolist() == [rc.samples(seed, h, n) for h in range(N)]


@pytest.mark.parametrize("n", [4, 5, 1000])
def test_samples_are_distinct_and_in_range(capi, n):
    """all 65536 hypotheses; the restatement on every 251st and on the last"""
    got = capi.ransac_samples(1234 + n, 0, 65536, n)
    assert got.min() >= 0 and got.max() < n
    s = np.sort(got, 1)
    assert (s[:, 1:] != s[:, :-1]).all()
    for h in list(range(0, 65536, 251)) + [65535]:
        assert got[h].tolist() == rc.samples(1234 + n, h, n)
    assert np.array_equal(capi.ransac_samples(1234 + n, 65530, 6, n), got[65530:])
    if n == 1000:
        assert len(np.unique(got)) == 1000                                 # every pair is drawn by some hypothesis
    L = capi.lib()
    buf = np.full(8, -7, np.int32)
    for first, count in ((65536, 1), (-1, 1), (0, -1), (65535, 2)):
        assert L.psx_ransac_samples(0, first, count, n, buf.ctypes.data_as(C.c_void_p)) == -1 and np.all(buf == -7)
    assert L.psx_ransac_samples(0, 0, 1, n, None) == -1


@pytest.mark.parametrize("n,N,seed", rc.SHAPES, ids=rc.SHAPE_IDS)
def test_fit_equals_the_restatement(capi, n, N, seed):
    """every hypothesis' four points, and the inlier sets the refit works on"""
    if n < 4:
        return
    pairs, lxy, rxy, _ = rc.planted(n, seed)
    pts = rc.correspondences(pairs, lxy, rxy)
    want = rc.expect(n, N, seed, False)
    for h in range(N):
        idx = rc.samples(seed, h, n)
        got = capi.homography_fit(pts[idx, 0:2], pts[idx, 2:4])
        assert np.array_equal(rc.bits(got), rc.bits(want["models"][h])), h
    sel = rc.passes(want["m"], rc.TOL, pts)
    assert sel.sum() >= 4
    got = capi.homography_fit(pts[sel, 0:2], pts[sel, 2:4])
    assert np.array_equal(rc.bits(got), rc.bits(rc.fit(pts[sel, 0:2], pts[sel, 2:4])))
    assert np.array_equal(rc.bits(got), rc.bits(rc.expect(n, N, seed, True)["m"]))


def test_fit_of_degenerate_inputs_is_not_finite(capi):
    """no special case: four coincident left points, and four collinear points on both sides, run through the same
    arithmetic and leave a non-finite entry -- the same one(s) as the restatement"""
    right = np.array([[10, 20], [200, 30], [40, 300], [250, 260]], np.float32)
    coincident = np.tile(np.array([[7, 9]], np.float32), (4, 1))
    line_l = np.array([[0, 0], [1, 2], [2, 4], [3, 6]], np.float32)
    line_r = np.array([[0, 0], [3, 1], [6, 2], [9, 3]], np.float32)
    for l, r in ((coincident, right), (line_l, line_r)):
        got, want = capi.homography_fit(l, r), rc.fit(l, r)
        assert not np.isfinite(got).all() and not np.isfinite(want).all()
        assert np.array_equal(rc.bits(got), rc.bits(want)), (got, want)
    # and a well-posed input is recovered: the true model from exact correspondences, up to scale
    l = np.array([[10, 20], [600, 30], [40, 400], [500, 460], [300, 200]], np.float32)
    r = rc._apply_h(rc.H_ASYM, l.astype(np.float64)).astype(np.float32)
    m = capi.homography_fit(l, r).astype(np.float64)
    assert np.allclose(m / m[8], rc.H_ASYM.astype(np.float64), rtol=1e-3, atol=1e-6)
    L = capi.lib()
    out = np.full(9, -7, np.float32)
    assert L.psx_homography_fit(l.ctypes.data_as(C.c_void_p), r.ctypes.data_as(C.c_void_p), 3, out.ctypes.data_as(C.c_void_p)) == -1
    assert L.psx_homography_fit(None, r.ctypes.data_as(C.c_void_p), 5, out.ctypes.data_as(C.c_void_p)) == -1 and np.all(out == -7)


@pytest.mark.parametrize("refit", [False, True], ids=["sample", "refit"])
@pytest.mark.parametrize("n,N,seed", rc.SHAPES, ids=rc.SHAPE_IDS)
def test_reference_equals_the_restatement(capi, n, N, seed, refit):
    pairs, lxy, rxy, _ = rc.planted(n, seed)
    want = rc.expect(n, N, seed, refit)
    got = capi.ransac_homography_ref(pairs, lxy, rxy, capi.ransac_opts(rc.TOL, N, seed, refit), layers=True)
    if n >= 4:
        assert np.array_equal(rc.bits(got["models"]), rc.bits(want["models"]))
        assert np.array_equal(got["counts"], want["counts"])
    assert rc.same_result(got["result"], want), (got["result"].best, want["best"])
    assert got["count"] == want["inliers"] and rc.same_records(got["inliers"], want["records"])
    if (n, N, seed) in rc.TIE_SHAPES:
        tied = np.nonzero(want["counts"] == want["counts"].max())[0]
        assert len(tied) > 1 and got["result"].best == tied[0]
    # records of the byte matcher: the same indices give the same result, the payload is copied whole
    pu = rc.planted(n, seed, u8=True)[0]
    gu = capi.ransac_homography_ref(pu, lxy, rxy, capi.ransac_opts(rc.TOL, N, seed, refit))
    assert rc.same_result(gu["result"], want) and np.array_equal(gu["inliers"]["left"], want["records"]["left"])
    assert gu["inliers"].dtype == rc.PAIR_U8_DTYPE and np.array_equal(gu["inliers"]["d2"], 2 * (gu["inliers"]["d1"] - 1) + 7)
    # capacity: the total is reported, the bytes behind the capacity stay
    total = want["inliers"]
    L = capi.lib()
    o = capi.ransac_opts(rc.TOL, N, seed, refit)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None
    for cap in sorted({max(total - 1, 0), 0}):
        buf = np.full((cap + 2) * 4, -7, np.int32)
        res, cnt = capi.RansacResult(), C.c_int(-1)
        rv = L.psx_ransac_homography_ref(ptr(pairs), n, ptr(lxy), n, ptr(rxy), n, C.byref(o), C.byref(res), ptr(buf) if cap else None, cap,
                                         C.byref(cnt), None, None)
        assert rv == 0 and cnt.value == total and rc.same_result(res, want)
        assert rc.same_records(buf[:4 * cap].view(rc.PAIR_DTYPE), want["records"][:cap]) and np.all(buf[4 * cap:] == -7)


def test_premises_of_the_planted_inputs():
    for n, N, seed in rc.SHAPES:
        pairs, lxy, rxy, is_planted = rc.planted(n, seed)
        a, b = rc.expect(n, N, seed, False), rc.expect(n, N, seed, True)
        if n < 4:
            assert a["best"] == b["best"] == -1 and a["inliers"] == 0 and not a["m"].any()
            continue
        assert np.isfinite(a["models"]).all(), (n, "a hypothesis with a non-finite model")
        c = a["counts"]
        planted_ids = set(pairs["d1"][is_planted].tolist())
        got = (a["best"], int(c.max()), int((c == c.max()).sum()), b["inliers"], len(planted_ids & set(b["records"]["d1"].tolist())),
               len(planted_ids))
        assert got == PREMISES[(n, N, seed)], ((n, N, seed), got)
        assert b["refit_kept"] == 1 and b["inliers"] >= a["inliers"] == a["sample_inliers"] == c.max()
        assert ((n, N, seed) in rc.TIE_SHAPES) == (got[2] > 1)
    assert PREMISES[(4, 8, 1)][0] == 0


def test_refit_model_is_accurate_on_exact_pairs(capi):
    """A sanity property with a derived margin: in the 2500-pair case every planted pair of radius 0 -- whose right position
    is H_ASYM of its left one, rounded to float32: exact to 2^-15 px below 1024 -- is an inlier of the refit model at
    tol 0.5.  The refit averages 1500 pairs whose offsets (radius <= 1.5 px, random angle) move the fitted mapping by
    about 1.5 / sqrt(1500) = 0.04 px: 0.5 px is more than ten times that."""
    n, N, seed = 2500, 512, 8
    pairs, lxy, rxy, is_planted = rc.planted(n, seed)
    got = capi.ransac_homography_ref(pairs, lxy, rxy, capi.ransac_opts(rc.TOL, N, seed, True))
    exact = is_planted & (np.arange(n) % 3 == 0)
    assert exact.sum() == 500
    ok = rc.passes(got["result"].matrix(), 0.5, rc.correspondences(pairs, lxy, rxy))
    assert ok[exact].all()
    assert not ok[~is_planted].any()


def test_argument_errors_write_nothing(capi):
    L = capi.lib()
    pairs, lxy, rxy, _ = rc.planted(65, 5)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    ok = capi.ransac_opts(2.0, 16, 0, True)

    def call(p=pairs, n=65, l=lxy, nl=65, r=rxy, nr=65, o=ok, cap=65, with_out=True, with_res=True, with_cnt=True):
        out = np.full(66 * 4, -7, np.int32)
        models, counts = np.full(16 * 9, -7, np.float32), np.full(16, -7, np.int32)
        res = capi.RansacResult()
        C.memset(C.byref(res), 0x5a, C.sizeof(res))
        cnt = C.c_int(-77)
        rv = L.psx_ransac_homography_ref(ptr(p) if p is not None else None, n, ptr(l) if l is not None else None, nl,
                                         ptr(r) if r is not None else None, nr, C.byref(o) if o is not None else None,
                                         C.byref(res) if with_res else None, ptr(out) if with_out else None, cap,
                                         C.byref(cnt) if with_cnt else None, ptr(models), ptr(counts))
        untouched = (np.all(out == -7) and np.all(models == -7) and np.all(counts == -7) and cnt.value == -77 and
                     bytes(res) == b"\x5a" * C.sizeof(res))
        return rv, untouched

    assert call()[0] == 0
    bad_opts = [capi.RansacOpts(float("nan"), 16, 0, 0), capi.RansacOpts(-0.5, 16, 0, 0), capi.RansacOpts(float("inf"), 16, 0, 0),
                capi.RansacOpts(2.0, 0, 0, 0), capi.RansacOpts(2.0, 65537, 0, 0), capi.RansacOpts(2.0, -3, 0, 0),
                capi.RansacOpts(2.0, 16, 0, 2), capi.RansacOpts(2.0, 16, 0, -1)]
    for o in bad_opts:
        assert call(o=o) == (-1, True), (o.tol, o.hypotheses, o.flags)
    for kw in (dict(o=None), dict(n=-1), dict(nl=-1), dict(nr=-1), dict(cap=-1), dict(p=None), dict(l=None), dict(r=None),
               dict(with_out=False), dict(with_res=False), dict(with_cnt=False), dict(nl=64), dict(nr=10)):
        assert call(**kw) == (-1, True), kw
    # an index outside its array is refused even below the minimum n; valid small inputs are "no model"
    bad = pairs[:3].copy()
    bad["left"][1] = -1
    assert call(p=bad, n=3) == (-1, True)
    rv, untouched = call(n=3)
    assert rv == 0 and not untouched
    got = capi.ransac_homography_ref(pairs[:3], lxy, rxy, ok, layers=True)
    assert got["result"].best == -1 and got["count"] == 0 and not got["result"].matrix().any() and got["result"].inliers == 0
    # tol 0 and 65536 hypotheses are valid options
    assert call(o=capi.RansacOpts(0.0, 16, 0, 1))[0] == 0
    d = capi.RansacOpts()
    assert L.psx_ransac_opts_default(C.byref(d)) == 0 and (d.tol, d.hypotheses, d.seed, d.flags) == (2.0, 1024, 0, capi.RANSAC_REFIT)
    assert L.psx_ransac_opts_default(None) == -1


def test_every_hypothesis_degenerate_is_no_model(capi):
    """all left positions coincide: every model has a non-finite entry, every count is 0, the answer is "no model\""""
    pairs, lxy, rxy, _ = rc.planted(65, 5)
    flat = np.tile(np.array([[3, 4]], np.float32), (65, 1))
    for refit in (False, True):
        want = rc.ransac(pairs, flat, rxy, rc.TOL, 32, 9, refit)
        got = capi.ransac_homography_ref(pairs, flat, rxy, capi.ransac_opts(rc.TOL, 32, 9, refit), layers=True)
        assert not np.isfinite(got["models"]).all(1).any() and not got["counts"].any()
        assert np.array_equal(rc.bits(got["models"]), rc.bits(want["models"]))
        assert rc.same_result(got["result"], want) and got["result"].best == -1 and got["count"] == 0


def test_declarations_and_bindings(capi):
    hdr = open(os.path.join(ROOT, "include", "popsift_hip.h")).read()
    for sym in ("psx_ransac_opts_default", "psx_ransac_samples", "psx_homography_fit", "psx_ransac_homography_ref",
                "psx_ransac_homography", "psx_ransac_homography_dev"):
        assert "int %s(" % sym in hdr and sym in capi.SYMBOLS and hasattr(capi.lib(), sym)
    assert C.sizeof(capi.RansacOpts) == 16 and C.sizeof(capi.RansacResult) == 52
    assert "geometric verification" in hdr and "#define PSX_RANSAC_REFIT 1" in hdr


def test_ransac_rule_under_sanitizers(tmp_path):
    """tests/cpp/ransac_rule_san.cpp: a stand-alone program (its own main) that includes ransac_rule.h alone and drives the
    samples, the fit and the whole host rule on exact-size heap arrays -- compiled with -ffp-contract=off
    -fsanitize=address,undefined and run directly."""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed"
    exe = str(tmp_path / "ransac_rule_san")
    cmd = [cxx, "-std=c++14", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan",
           os.path.join(ROOT, "tests", "cpp", "ransac_rule_san.cpp"), "-o", exe,
           "-I", os.path.join(ROOT, "popsift_amd", "csrc", "hip"), "-I", os.path.join(ROOT, "include")]
    subprocess.check_call(cmd)
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout
