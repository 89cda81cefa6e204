"""GPU tests of the fundamental-matrix estimator (include/popsift_hip.h, "geometric verification"): psx_ransac_fundamental
and its _dev form, FeaturesDev::estimateFundamental and popsift-match --verify-fundamental.  Expected values come from
tests/fundamental_cases.py -- an independent restatement of csrc/hip/fundamental_rule.h -- and from the host reference
psx_ransac_fundamental_ref; models are compared as 32-bit patterns, counts, the result struct and the inlier records
exactly."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch        # before the HIP library is loaded: torch brings a HIP runtime of its own and must initialise first (_dev forms)

from popsift_amd.synth import synth
from tests import fundamental_cases as fc
from tests import guided_cases as gc
from tests import ransac_cases as rc
from tests.match_pairs_cases import same_records

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MATCH = os.path.join(ROOT, "popsift_amd", "lib", "popsift-match")


class _Positions:
    """two position arrays uploaded once"""

    def __init__(self, capi, lxy, rxy):
        self.L, self.bufs = capi.lib(), []
        self.nl, self.nr = len(lxy), len(rxy)
        self.plx, self.prx = capi._to_device(self.L, 0, [np.ascontiguousarray(lxy, np.float32), np.ascontiguousarray(rxy, np.float32)], self.bufs)

    def close(self):
        for p in self.bufs:
            self.L.psx_dev_free(0, p)
        self.bufs = []


def _raw(capi, pos, pairs, opts, cap, with_layers=True, fn="psx_ransac_fundamental"):
    """psx_ransac_fundamental with sentinel-filled outputs: (rc, result, count, out int32 words, models, counts)"""
    N = opts.hypotheses
    out = np.full((cap + 2) * 4, -7, np.int32)
    models, counts = np.full((N, 9), -7, np.float32), np.full(N, -7, np.int32)
    res, cnt = capi.RansacResult(), C.c_int(-77)
    C.memset(C.byref(res), 0x5a, C.sizeof(res))
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    rv = getattr(pos.L, fn)(0, ptr(pairs) if len(pairs) else None, len(pairs), pos.plx, pos.nl, pos.prx, pos.nr, C.byref(opts),
                            C.byref(res), ptr(out) if cap else None, cap, C.byref(cnt),
                            ptr(models) if with_layers else None, ptr(counts) if with_layers else None)
    return rv, res, cnt.value, out, models, counts


def _ref_dict(ref):
    r = ref["result"]
    return dict(m=r.matrix(), best=r.best, sample_inliers=r.sample_inliers, inliers=r.inliers, refit_kept=r.refit_kept)


@pytest.mark.parametrize("refit", [False, True], ids=["sample", "refit"])
@pytest.mark.parametrize("kind", fc.KINDS)
@pytest.mark.parametrize("n,N,seed", fc.SHAPES, ids=fc.SHAPE_IDS)
def test_device_equals_reference_and_restatement(capi, n, N, seed, kind, refit):
    pairs, lxy, rxy, _ = fc.planted(n, seed, kind)
    want = fc.expect(n, N, seed, kind, refit)
    opts = capi.ransac_opts(fc.TOL, N, seed, refit)
    ref = capi.ransac_fundamental_ref(pairs, lxy, rxy, opts, layers=True)
    pos = _Positions(capi, lxy, rxy)
    try:
        rv, res, cnt, out, models, counts = _raw(capi, pos, pairs, opts, n)
        assert rv == 0
        if n < 8:
            assert res.best == -1 and cnt == 0 and res.inliers == 0 and not res.matrix().any()
            assert np.all(out == -7) and np.all(models == -7) and np.all(counts == -7)          # buffers untouched
            return
        bad = np.nonzero((fc.bits(models) != fc.bits(want["models"])).any(1))[0]
        assert len(bad) == 0, ("models differ from the restatement at hypotheses", bad[:5], models[bad[:1]], want["models"][bad[:1]])
        assert np.array_equal(fc.bits(models), fc.bits(ref["models"]))
        assert np.array_equal(counts, want["counts"]) and np.array_equal(counts, ref["counts"])
        assert fc.same_result(res, want) and fc.same_result(res, _ref_dict(ref)), (res.best, res.sample_inliers, res.inliers, want["best"])
        assert cnt == want["inliers"] == ref["count"]
        got = out[:4 * cnt].view(fc.PAIR_DTYPE)
        assert fc.same_records(got, want["records"]) and fc.same_records(got, ref["inliers"]) and np.all(out[4 * cnt:] == -7)
        if (n, N, seed) in fc.TIE_SHAPES:
            tied = np.nonzero(want["counts"] == want["counts"].max())[0]
            assert len(tied) > 1 and res.best == tied[0]
        # the python wrapper, and its guide
        g = capi.ransac_fundamental(pairs, lxy, rxy, opts)
        assert fc.same_result(g["result"], want) and fc.same_records(g["inliers"], want["records"])
        gd = g["result"].guide(fc.TOL)
        assert gd.kind == capi.GUIDE_EPIPOLAR and np.array_equal(fc.bits(np.array(list(gd.m), np.float32)), fc.bits(want["m"]))
    finally:
        pos.close()


def test_capacity_dev_form_and_byte_records(capi):
    """capacity count - 1, 0 and the NULL "how many?" form report the total and leave the bytes behind the capacity alone,
    in the host buffer and in a torch device buffer read back; the _dev form equals the host form; records of the byte
    matcher's dtype give the same result as float records with the same indices"""
    n, N, seed, kind = 300, 256, 7, "general"
    pairs, lxy, rxy, _ = fc.planted(n, seed, kind)
    pu = fc.planted(n, seed, kind, u8=True)[0]
    pos = _Positions(capi, lxy, rxy)
    try:
        for refit in (False, True):
            want = fc.expect(n, N, seed, kind, refit)
            total = want["inliers"]
            opts = capi.ransac_opts(fc.TOL, N, seed, refit)
            dpairs = torch.from_numpy(np.ascontiguousarray(pairs).view(np.uint8).copy()).cuda()
            dpu = torch.from_numpy(np.ascontiguousarray(pu).view(np.uint8).copy()).cuda()
            for cap in (total - 1, 0, n):
                rv, res, cnt, out, _, _ = _raw(capi, pos, pairs, opts, cap, with_layers=False)
                k = min(cap, total)
                assert rv == 0 and cnt == total and fc.same_result(res, want), cap
                assert fc.same_records(out[:4 * k].view(fc.PAIR_DTYPE), want["records"][:k]) and np.all(out[4 * k:] == -7), cap
                for src, dtype in ((dpairs, fc.PAIR_DTYPE), (dpu, fc.PAIR_U8_DTYPE)):
                    dbuf = torch.full(((cap + 2) * 16,), 0xA5, dtype=torch.uint8, device="cuda")
                    torch.cuda.synchronize()
                    g = capi.ransac_fundamental_dev(src.data_ptr(), n, pos.plx.value, n, pos.prx.value, n, dbuf.data_ptr() if cap else 0, cap,
                                                    opts, layers=True)
                    back = dbuf.cpu().numpy()
                    assert g["count"] == total and fc.same_result(g["result"], want), cap
                    assert np.array_equal(fc.bits(g["models"]), fc.bits(want["models"])) and np.array_equal(g["counts"], want["counts"])
                    recs = back[:k * 16].view(dtype)
                    assert np.array_equal(recs["left"], want["records"]["left"][:k]) and np.array_equal(recs["right"], want["records"]["right"][:k])
                    assert np.array_equal(recs["d1"].astype(np.int64), want["records"]["d1"][:k].astype(np.int64))       # the payload travels
                    assert np.all(back[k * 16:] == 0xA5), cap
                    assert torch.equal(src.cpu(), torch.from_numpy(np.ascontiguousarray(pairs if dtype == fc.PAIR_DTYPE else pu).view(np.uint8).copy()))
            gu = capi.ransac_fundamental(pu, lxy, rxy, opts)
            assert fc.same_result(gu["result"], want) and gu["inliers"].dtype == fc.PAIR_U8_DTYPE
            part = capi.ransac_fundamental(pairs, lxy, rxy, opts, capacity=total - 1)
            assert part["count"] == total and fc.same_records(part["inliers"], want["records"][:total - 1])
        dd = capi.DeviceDescriptors(np.zeros((n, 128), np.float32), xy=lxy), capi.DeviceDescriptors(np.zeros((n, 128), np.float32), xy=rxy)
        g = dd[0].ransac_fundamental(dd[1], pairs, opts)
        assert fc.same_result(g["result"], want) and fc.same_records(g["inliers"], want["records"])
        assert g["result"].guide(1.0).kind == capi.GUIDE_EPIPOLAR
        dd[0].close(); dd[1].close()
    finally:
        pos.close()


def test_device_argument_errors_write_nothing(capi):
    pairs, lxy, rxy, _ = fc.planted(65, 5, "general")
    pos = _Positions(capi, lxy, rxy)
    try:
        def refused(p=pairs, opts=capi.ransac_opts(2.0, 16, 0, True), cap=65, nl=None, nr=None):
            pos.nl, pos.nr = (65 if nl is None else nl), (65 if nr is None else nr)
            rv, res, cnt, out, models, counts = _raw(capi, pos, p, opts, cap)
            pos.nl = pos.nr = 65
            return (rv == -1 and np.all(out == -7) and np.all(models == -7) and np.all(counts == -7) and cnt == -77 and
                    bytes(res) == b"\x5a" * C.sizeof(res))

        for o in (capi.RansacOpts(float("nan"), 16, 0, 0), capi.RansacOpts(-1.0, 16, 0, 0), capi.RansacOpts(float("inf"), 16, 0, 0),
                  capi.RansacOpts(2.0, 0, 0, 0), capi.RansacOpts(2.0, 65537, 0, 0), capi.RansacOpts(2.0, 16, 0, 4)):
            assert refused(opts=o), (o.tol, o.hypotheses, o.flags)
        assert refused(nl=-1) and refused(nr=-1) and refused(nl=0)
        # a pair index outside its position array: flagged by the gather kernel, nothing is read out of bounds
        bad = pairs.copy()
        bad["right"][40] = 65
        assert refused(p=bad)
        bad = pairs.copy()
        bad["left"][3] = -2
        assert refused(p=bad) and refused(nl=64)
        rv, res, cnt, out, _, _ = _raw(capi, pos, pairs, capi.ransac_opts(2.0, 16, 0, True), 65)
        assert rv == 0 and cnt == res.inliers >= 8
    finally:
        pos.close()


def test_alternating_with_the_homography_on_one_scratch(capi):
    """both estimators use the same scratch slots and the same device state: calls of one between calls of the other,
    with and without the refit, across a release of the scratch, each equal to its own restatement every time"""
    fp, flxy, frxy, _ = fc.planted(300, 7, "general")
    hp, hlxy, hrxy, _ = rc.planted(129, 6)
    fpos, hpos = _Positions(capi, flxy, frxy), _Positions(capi, hlxy, hrxy)
    try:
        for round_ in range(2):
            for refit in (True, False):
                fo, ho = capi.ransac_opts(fc.TOL, 256, 7, refit), capi.ransac_opts(rc.TOL, 128, 6, refit)
                fw, hw = fc.expect(300, 256, 7, "general", refit), rc.expect(129, 128, 6, refit)
                for _ in range(2):
                    rv, res, cnt, out, models, counts = _raw(capi, fpos, fp, fo, 300)
                    assert rv == 0 and fc.same_result(res, fw) and np.array_equal(fc.bits(models), fc.bits(fw["models"]))
                    assert np.array_equal(counts, fw["counts"]) and fc.same_records(out[:4 * cnt].view(fc.PAIR_DTYPE), fw["records"])
                    rv, res, cnt, out, models, counts = _raw(capi, hpos, hp, ho, 129, fn="psx_ransac_homography")
                    assert rv == 0 and rc.same_result(res, hw) and np.array_equal(rc.bits(models), rc.bits(hw["models"]))
                    assert np.array_equal(counts, hw["counts"]) and rc.same_records(out[:4 * cnt].view(rc.PAIR_DTYPE), hw["records"])
            assert capi.lib().psx_match_release() == 0
    finally:
        fpos.close()
        hpos.close()


def test_match_verify_rematch_on_the_device(oracle, capi):
    """the whole chain without the pair list leaving the device: match_pairs_dev -> ransac_fundamental_dev ->
    match_pairs_guided_dev with the returned model as an EPIPOLAR guide, on descriptors planted on the "general" scene
    (fundamental_cases.chain_case).  The RANSAC result equals the restatement on the downloaded list; it drops the
    confident matches at the wrong place; the final list equals the host join of the expectation computed from the restated
    relation under the RETURNED model."""
    left, right, lxy, rxy, is_planted, perm = fc.chain_case()
    n = len(left)
    L = capi.lib()
    bufs = []
    pl, plx, pr, prx = capi._to_device(L, 0, [left, lxy, right, rxy], bufs)
    try:
        for round_ in range(2):
            d_pairs = torch.full((n * 16,), 0xA5, dtype=torch.uint8, device="cuda")
            d_inl = torch.full((n * 16,), 0xA5, dtype=torch.uint8, device="cuda")
            d_final = torch.full((n * 16,), 0xA5, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            n1 = capi.match_pairs_dev(pl.value, n, pr.value, n, d_pairs.data_ptr(), n, 0.8, True)
            opts = capi.ransac_opts(fc.TOL, 256, 11, True)
            g = capi.ransac_fundamental_dev(d_pairs.data_ptr(), n1, plx.value, n, prx.value, n, d_inl.data_ptr(), n, opts)
            res = g["result"]
            guide = res.guide(fc.TOL)
            assert guide.kind == capi.GUIDE_EPIPOLAR
            n3 = capi.match_pairs_guided_dev(pl.value, plx.value, n, pr.value, prx.value, n, guide, d_final.data_ptr(), n, 0.8, True)
            pairs1 = d_pairs.cpu().numpy()[:n1 * 16].view(capi.PAIR_DTYPE)
            assert same_records(pairs1, capi.match_pairs(left, right, 0.8, True))
            planted_pair = is_planted[pairs1["left"]] & (perm[pairs1["left"]] == pairs1["right"])
            wrong_place = ~is_planted[pairs1["left"]] & (perm[pairs1["left"]] == pairs1["right"])
            assert planted_pair.sum() == is_planted.sum() == 120 and wrong_place.sum() == 40
            want = fc.ransac(pairs1, lxy, rxy, fc.TOL, 256, 11, True)
            assert fc.same_result(res, want) and g["count"] == want["inliers"]
            inl = d_inl.cpu().numpy()[:g["count"] * 16].view(capi.PAIR_DTYPE)
            assert fc.same_records(inl, want["records"])
            kept_planted = np.isin(pairs1["left"][planted_pair], inl["left"]).sum()
            kept_wrong = np.isin(pairs1["left"][wrong_place], inl["left"]).sum()
            print("chain: %d pairs, %d inliers: %d of 120 planted, %d of 40 misplaced" % (n1, g["count"], kept_planted, kept_wrong))
            # a uniform outlier lies within 2 px of a given line with probability about 4 * 800 / (640 * 480) = 1 %: at most a few
            assert kept_planted >= 0.85 * 120 and kept_wrong <= 4
            A = gc.restate(gc.EPIPOLAR, res.matrix(), fc.TOL, lxy, rxy)
            efm, efd = gc.expect_directed(oracle, left, right, A, False)
            ebm, ebd = gc.expect_directed(oracle, right, left, A.T, False)
            final = d_final.cpu().numpy()[:n3 * 16].view(capi.PAIR_DTYPE)
            assert same_records(final, capi.pairs_join(efm, efd, ebm, n, 0.8, True)) and n3 >= kept_planted
            assert L.psx_match_release() == 0
    finally:
        for p in bufs:
            L.psx_dev_free(0, p)


def test_cpp_estimate_fundamental_on_the_gpu(tmp_path):
    """tests/cpp/test_fundamental_api.cpp with POPSIFT_TEST_EXPECT_GPU: FeaturesDev::estimateFundamental equals the C-ABI on
    the same device arrays, its guide is an epipolar one accepted by matchPairsGuided, invalid options throw"""
    libdir = os.path.join(ROOT, "popsift_amd", "lib")
    exe = str(tmp_path / "test_fundamental_api")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-pthread", os.path.join(ROOT, "tests", "cpp", "test_fundamental_api.cpp"), "-o", exe,
                           "-I", os.path.join(ROOT, "popsift_amd", "csrc", "include"), "-I", os.path.join(ROOT, "include"),
                           "-L", libdir, "-lpopsift", "-lpopsift_hip", "-Wl,-rpath," + libdir])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300,
                         env=dict(os.environ, POPSIFT_TEST_EXPECT_GPU="1"))
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout
    assert "estimateFundamental:" in out.stdout


def _desc_xy(feats, n_desc):
    xy = np.full((n_desc, 2), np.nan, np.float32)
    for s in range(feats["desc_idx"].shape[1]):
        sel = feats["num_ori"] > s
        xy[feats["desc_idx"][sel, s]] = np.stack([feats["xpos"][sel], feats["ypos"][sel]], 1)
    assert not np.isnan(xy).any()
    return xy


def _crops():
    base = synth(336, 256, 77)
    # a point of a at (x, y) is at (x + 5, y + 3) in b
    return np.ascontiguousarray(base[8:248, 8:328]), np.ascontiguousarray(base[5:245, 3:323])


def _extract(capi, img):
    ctx = capi.Context(capi.default_config(octaves=3, norm_multi=9))
    ctx.upload(img)
    ctx.extract()
    f, d = ctx.download()
    ctx.close()
    return d, _desc_xy(f, len(d))


def _write_pgm(path, img):
    with open(path, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (img.shape[1], img.shape[0]) + img.tobytes())


def _printed_model(stdout):
    line = [l for l in stdout.splitlines() if l.startswith("Fundamental:")][0]
    m = np.array([float(v) for v in line.split()[1:]], np.float32)           # %.9g: float32 round trip
    assert m.shape == (9,)
    return m


def test_match_tool_verify_fundamental(capi, tmp_path):
    """popsift-match --pairs FILE --verify-fundamental 1.5 --ransac-refit prints the nine entries and the inlier count and
    writes only the inliers; --rematch writes the list guided by the epipolar band; the usage errors are reported.
    Descriptor ORDER is not reproducible between runs (so neither are the samples): the rows are compared, as sorted
    distances, with what the restated rule keeps of capi's pairs -- and what capi's guided matcher returns -- under the
    model the tool PRINTED.  The two crops differ by a pure translation, for which every F = [e]x is valid: the count is
    held against the pairs the true motion admits, not against another run's model."""
    a, b = _crops()
    _write_pgm(tmp_path / "l.pgm", a)
    _write_pgm(tmp_path / "r.pgm", b)
    (da, xa), (db, xb) = _extract(capi, a), _extract(capi, b)
    pairs = capi.match_pairs(da, db, 0.8, True)
    pts = rc.correspondences(pairs, xa, xb)
    truth = rc.passes([1, 0, 5, 0, 1, 3, 0, 0, 1], 1.5, pts)
    common = [MATCH, "-l", "l.pgm", "-r", "r.pgm", "--octaves", "3", "--norm-multi", "9"]
    verify = ["--mutual", "--verify-fundamental", "1.5", "--ransac-hypotheses", "500", "--ransac-seed", "7", "--ransac-refit"]
    fmt = lambda recs: sorted(("%.3f" % x, "%.3f" % y) for x, y in zip(recs["d1"], recs["d2"]))
    out = tmp_path / "pairs.txt"
    p = subprocess.run(common + ["--pairs", str(out)] + verify, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    rows = [l.split() for l in out.read_text().splitlines()]
    assert "Fundamental inliers: %d of %d" % (len(rows), len(pairs)) in p.stdout and "Number of matches: %d" % len(rows) in p.stdout
    keep = fc.passes(_printed_model(p.stdout), 1.5, pts)
    assert len(rows) == keep.sum() > 50 and sorted((r[4], r[5]) for r in rows) == fmt(pairs[keep])
    print("tool: %d inliers of %d pairs; the true translation admits %d" % (len(rows), len(pairs), truth.sum()))
    assert 2 * len(rows) >= truth.sum() > 50
    p = subprocess.run(common + ["--pairs", str(out)] + verify + ["--rematch"], cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    rows = [l.split() for l in out.read_text().splitlines()]
    guided = capi.match_pairs_guided(da, xa, db, xb, capi.Guide.epipolar(_printed_model(p.stdout), 1.5), 0.8, True)
    assert "Number of matches: %d" % len(rows) in p.stdout
    assert sorted((r[4], r[5]) for r in rows) == fmt(guided)
    ident = "1,0,0,0,1,0,0,0,1"
    for extra, msg in ((["--verify-fundamental", "1.5"], "'--verify-fundamental' needs '--pairs'"),
                       (["--pairs", "p.txt", "--rematch"], "'--rematch' needs '--verify-homography'"),
                       (["--pairs", "p.txt", "--rematch"], "'--verify-fundamental'"),
                       (["--pairs", "p.txt", "--ransac-refit"], "need '--verify-homography'"),
                       (["--pairs", "p.txt", "--ransac-refit"], "'--verify-fundamental'"),
                       (["--pairs", "p.txt", "--verify-fundamental", "1.5", "--verify-homography", "1.5"], "cannot be combined"),
                       (["--pairs", "p.txt", "--verify-fundamental", "1.5", "--homography", ident, "--guide-tol", "2"], "cannot be combined"),
                       (["--pairs", "p.txt", "--verify-fundamental", "1.5", "--fundamental", ident, "--guide-tol", "2"], "cannot be combined")):
        p = subprocess.run(common + extra, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
        assert p.returncode != 0 and msg in p.stderr, (extra, p.stderr)
