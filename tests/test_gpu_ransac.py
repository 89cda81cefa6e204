"""GPU tests of geometric verification (include/popsift_hip.h, "geometric verification"): psx_ransac_homography and its
_dev form, FeaturesDev::estimateHomography and popsift-match --verify-homography.  Expected values come from
tests/ransac_cases.py -- an independent restatement of csrc/hip/ransac_rule.h -- and from the host reference
psx_ransac_homography_ref; models are compared as 32-bit patterns, counts, the result struct and the inlier records exactly.

Measured on one MI355X (printed by test_ransac_on_real_descriptors): 561 mutual pairs at ratio 0.8 between the two crops, of
which the true translation (+5, +3) admits 557 at tol 1.5; the estimated model keeps 558 (the winning sample's 558; the
refit did not gain and was not kept)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch        # before the HIP library is loaded: torch brings a HIP runtime of its own and must initialise first (_dev forms)

from popsift_amd.synth import synth
from tests import guided_cases as gc
from tests import ransac_cases as rc
from tests.match_pairs_cases import directed, dist_as_int, planted, same_records

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


def _raw(capi, pos, pairs, opts, cap, with_layers=True):
    """psx_ransac_homography with sentinel-filled outputs: (rc, result, count, out int32 words, models, counts)"""
    N = opts.hypotheses
    out = np.full((cap + 2) * 4, -7, np.int32)
    models, counts = np.full((N, 9), -7, np.float32), np.full(N, -7, np.int32)
    res, cnt = capi.RansacResult(), C.c_int(-77)
    C.memset(C.byref(res), 0x5a, C.sizeof(res))
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    rv = pos.L.psx_ransac_homography(0, ptr(pairs) if len(pairs) else None, len(pairs), pos.plx, pos.nl, pos.prx, pos.nr, C.byref(opts),
                                     C.byref(res), ptr(out) if cap else None, cap, C.byref(cnt),
                                     ptr(models) if with_layers else None, ptr(counts) if with_layers else None)
    return rv, res, cnt.value, out, models, counts


@pytest.mark.parametrize("refit", [False, True], ids=["sample", "refit"])
@pytest.mark.parametrize("n,N,seed", rc.SHAPES, ids=rc.SHAPE_IDS)
def test_device_equals_reference_and_restatement(capi, n, N, seed, refit):
    pairs, lxy, rxy, _ = rc.planted(n, seed)
    want = rc.expect(n, N, seed, refit)
    opts = capi.ransac_opts(rc.TOL, N, seed, refit)
    ref = capi.ransac_homography_ref(pairs, lxy, rxy, opts, layers=True)
    pos = _Positions(capi, lxy, rxy)
    try:
        rv, res, cnt, out, models, counts = _raw(capi, pos, pairs, opts, n)
        assert rv == 0
        if n < 4:
            assert res.best == -1 and cnt == 0 and res.inliers == 0 and not res.matrix().any()
            assert np.all(out == -7) and np.all(models == -7) and np.all(counts == -7)          # buffers untouched
            return
        bad = np.nonzero((rc.bits(models) != rc.bits(want["models"])).any(1))[0]
        assert len(bad) == 0, ("models differ from the restatement at hypotheses", bad[:5], models[bad[:1]], want["models"][bad[:1]])
        assert np.array_equal(rc.bits(models), rc.bits(ref["models"]))
        assert np.array_equal(counts, want["counts"]) and np.array_equal(counts, ref["counts"])
        assert rc.same_result(res, want) and rc.same_result(res, rc_dict(ref)), (res.best, res.sample_inliers, res.inliers, want["best"])
        assert cnt == want["inliers"] == ref["count"]
        got = out[:4 * cnt].view(rc.PAIR_DTYPE)
        assert rc.same_records(got, want["records"]) and rc.same_records(got, ref["inliers"]) and np.all(out[4 * cnt:] == -7)
        if (n, N, seed) in rc.TIE_SHAPES:
            tied = np.nonzero(want["counts"] == want["counts"].max())[0]
            assert len(tied) > 1 and res.best == tied[0]
        # the python wrappers
        g = capi.ransac_homography(pairs, lxy, rxy, opts)
        assert rc.same_result(g["result"], want) and rc.same_records(g["inliers"], want["records"])
    finally:
        pos.close()


@pytest.mark.parametrize("refit", [False, True], ids=["sample", "refit"])
def test_inlier_compaction_past_256_workgroups(capi, refit):
    """65 793 = 256 * 257 + 1 planted pairs, 8 hypotheses: 258 compaction workgroups, the smallest size at which the last
    workgroup's sum over the totals of the workgroups before it takes a second trip.  Seed 19: the host reference's
    winning sample keeps 15 793 pairs (36 849 after the refit), 67 (143) of them in workgroup 256 and the last pair in
    workgroup 257, so both the total and the last record's slot depend on that second trip.  The device result equals
    psx_ransac_homography_ref: model bits, best, the three counts, every inlier record.  The pure-Python restatement
    (ransac_cases.expect) is not run at this size: its fit and score are loops in Python."""
    n, N, seed = 256 * 257 + 1, 8, 19
    pairs, lxy, rxy, _ = rc.planted(n, seed)
    opts = capi.ransac_opts(rc.TOL, N, seed, refit)
    ref = capi.ransac_homography_ref(pairs, lxy, rxy, opts, layers=True)
    want = rc_dict(ref)
    assert want["inliers"] == ref["count"] > 5000 and want["refit_kept"] == int(refit)
    at = np.searchsorted(pairs["d1"], ref["inliers"]["d1"])                 # planted: d1 = the record's index + 1, ascending
    assert (at // 256 == 256).any() and at[-1] == n - 1
    pos = _Positions(capi, lxy, rxy)
    try:
        rv, res, cnt, out, models, counts = _raw(capi, pos, pairs, opts, n)
        assert rv == 0
        assert np.array_equal(rc.bits(models), rc.bits(ref["models"])) and np.array_equal(counts, ref["counts"])
        assert rc.same_result(res, want), (res.best, res.sample_inliers, res.inliers, res.refit_kept, want)
        assert cnt == ref["count"]
        assert rc.same_records(out[:4 * cnt].view(rc.PAIR_DTYPE), ref["inliers"]) and np.all(out[4 * cnt:] == -7)
    finally:
        pos.close()


def rc_dict(ref):
    r = ref["result"]
    return dict(m=r.matrix(), best=r.best, sample_inliers=r.sample_inliers, inliers=r.inliers, refit_kept=r.refit_kept)


def test_capacity_dev_form_and_byte_records(capi):
    """capacity count - 1, 0 and the NULL "how many?" form report the total and leave the bytes behind the capacity alone,
    in the host buffer and in a torch device buffer read back; the _dev form equals the host form; records of the byte
    matcher's dtype give the same result as float records with the same indices"""
    n, N, seed = 300, 256, 7
    pairs, lxy, rxy, _ = rc.planted(n, seed)
    pu = rc.planted(n, seed, u8=True)[0]
    pos = _Positions(capi, lxy, rxy)
    try:
        for refit in (False, True):
            want = rc.expect(n, N, seed, refit)
            total = want["inliers"]
            opts = capi.ransac_opts(rc.TOL, N, seed, refit)
            dpairs = torch.from_numpy(np.ascontiguousarray(pairs).view(np.uint8).copy()).cuda()
            dpu = torch.from_numpy(np.ascontiguousarray(pu).view(np.uint8).copy()).cuda()
            for cap in (total - 1, 0, n):
                rv, res, cnt, out, _, _ = _raw(capi, pos, pairs, opts, cap, with_layers=False)
                k = min(cap, total)
                assert rv == 0 and cnt == total and rc.same_result(res, want), cap
                assert rc.same_records(out[:4 * k].view(rc.PAIR_DTYPE), want["records"][:k]) and np.all(out[4 * k:] == -7), cap
                for src, dtype in ((dpairs, rc.PAIR_DTYPE), (dpu, rc.PAIR_U8_DTYPE)):
                    dbuf = torch.full(((cap + 2) * 16,), 0xA5, dtype=torch.uint8, device="cuda")
                    torch.cuda.synchronize()
                    g = capi.ransac_homography_dev(src.data_ptr(), n, pos.plx.value, n, pos.prx.value, n, dbuf.data_ptr() if cap else 0, cap,
                                                   opts, layers=True)
                    back = dbuf.cpu().numpy()
                    assert g["count"] == total and rc.same_result(g["result"], want), cap
                    assert np.array_equal(rc.bits(g["models"]), rc.bits(want["models"])) and np.array_equal(g["counts"], want["counts"])
                    recs = back[:k * 16].view(dtype)
                    assert np.array_equal(recs["left"], want["records"]["left"][:k]) and np.array_equal(recs["right"], want["records"]["right"][:k])
                    assert np.array_equal(recs["d1"].astype(np.int64), want["records"]["d1"][:k].astype(np.int64))       # the payload travels
                    assert np.all(back[k * 16:] == 0xA5), cap
                    assert torch.equal(src.cpu(), torch.from_numpy(np.ascontiguousarray(pairs if dtype == rc.PAIR_DTYPE else pu).view(np.uint8).copy()))
            gu = capi.ransac_homography(pu, lxy, rxy, opts)
            assert rc.same_result(gu["result"], want) and gu["inliers"].dtype == rc.PAIR_U8_DTYPE
            part = capi.ransac_homography(pairs, lxy, rxy, opts, capacity=total - 1)
            assert part["count"] == total and rc.same_records(part["inliers"], want["records"][:total - 1])
        dd = capi.DeviceDescriptors(np.zeros((n, 128), np.float32), xy=lxy), capi.DeviceDescriptors(np.zeros((n, 128), np.float32), xy=rxy)
        g = dd[0].ransac_homography(dd[1], pairs, opts)
        assert rc.same_result(g["result"], want) and rc.same_records(g["inliers"], want["records"])
        dd[0].close(); dd[1].close()
    finally:
        pos.close()


def test_device_argument_errors_write_nothing(capi):
    pairs, lxy, rxy, _ = rc.planted(65, 5)
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
        assert rv == 0 and cnt == res.inliers > 30
    finally:
        pos.close()


def test_match_verify_rematch_on_the_device(oracle, capi):
    """the whole chain without the pair list leaving the device: match_pairs_dev -> ransac_homography_dev ->
    match_pairs_guided_dev with the returned model, on the planted descriptors of guided_cases.  The RANSAC result equals
    the restatement on the downloaded list; the final list equals the host join of the expectation computed from the
    restated relation under the RETURNED model; the existing matchers are unchanged before, after and across a release."""
    nl, nr, seed = gc.NAMED["300x257"]
    c = gc.case(oracle, seed, nl, nr, "homography", False)
    L = capi.lib()
    left, right = planted(9, 2500, 2300)
    fm, fd, bm, bd = directed(oracle, ("planted", 9, 2500, 2300, True), left, right, True)
    want_plain = capi.pairs_join(fm, fd, bm, len(right), 0.8, True)

    def existing():
        mg, dg = capi.match_u8(left, right)
        assert np.array_equal(mg, fm) and np.array_equal(dg, fd)
        assert same_records(capi.match_pairs_u8(left, right, 0.8, True), want_plain)
        got = capi.match_pairs_guided(c["left"], c["lxy"], c["right"], c["rxy"], capi.Guide.make(c["kind"], c["m"], c["tol"]), 0.8, True)
        assert same_records(got, capi.pairs_join(c["fm"], c["fd"], c["bm"], nr, 0.8, True))

    bufs = []
    pl, plx, pr, prx = capi._to_device(L, 0, [c["left"], c["lxy"], c["right"], c["rxy"]], bufs)
    try:
        existing()
        for round_ in range(2):
            d_pairs = torch.full((nl * 16,), 0xA5, dtype=torch.uint8, device="cuda")
            d_inl = torch.full((nl * 16,), 0xA5, dtype=torch.uint8, device="cuda")
            d_final = torch.full((nl * 16,), 0xA5, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            n1 = capi.match_pairs_dev(pl.value, nl, pr.value, nr, d_pairs.data_ptr(), nl, 0.8, True)
            opts = capi.ransac_opts(gc.TOL, 256, 11, True)
            g = capi.ransac_homography_dev(d_pairs.data_ptr(), n1, plx.value, nl, prx.value, nr, d_inl.data_ptr(), nl, opts)
            res = g["result"]
            n3 = capi.match_pairs_guided_dev(pl.value, plx.value, nl, pr.value, prx.value, nr, res.guide(gc.TOL), d_final.data_ptr(), nl, 0.8, True)
            pairs1 = d_pairs.cpu().numpy()[:n1 * 16].view(capi.PAIR_DTYPE)
            assert same_records(pairs1, capi.match_pairs(c["left"], c["right"], 0.8, True)) and n1 > 50
            want = rc.ransac(pairs1, c["lxy"], c["rxy"], gc.TOL, 256, 11, True)
            assert rc.same_result(res, want) and g["count"] == want["inliers"] >= 30
            assert rc.same_records(d_inl.cpu().numpy()[:g["count"] * 16].view(capi.PAIR_DTYPE), want["records"])
            A = gc.restate(gc.HOMOGRAPHY, res.matrix(), gc.TOL, c["lxy"], c["rxy"])
            efm, efd = gc.expect_directed(oracle, c["left"], c["right"], A, False)
            ebm, ebd = gc.expect_directed(oracle, c["right"], c["left"], A.T, False)
            final = d_final.cpu().numpy()[:n3 * 16].view(capi.PAIR_DTYPE)
            assert same_records(final, capi.pairs_join(efm, efd, ebm, nr, 0.8, True)) and n3 >= g["count"]
            existing()
            assert L.psx_match_release() == 0
        existing()
    finally:
        for p in bufs:
            L.psx_dev_free(0, p)


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


def test_ransac_on_real_descriptors(capi):
    """two 320 x 240 crops of one image (true motion (+5, +3)): mutual pairs at ratio 0.8, then RANSAC with tol 1.5, 2000
    hypotheses and the refit.  The result equals the restatement on the same pairs and positions; every returned pair
    satisfies the restated guide rule under the returned model; and the inlier count is at least half of what the true
    translation admits among the same pairs -- a floor against a gross failure, not a quality measurement."""
    (da, xa), (db, xb) = (_extract(capi, img) for img in _crops())
    pairs = capi.match_pairs(da, db, 0.8, True)
    opts = capi.ransac_opts(1.5, 2000, 3, True)
    g = capi.ransac_homography(pairs, xa, xb, opts, layers=True)
    want = rc.ransac(pairs, xa, xb, 1.5, 2000, 3, True)
    assert np.array_equal(rc.bits(g["models"]), rc.bits(want["models"])) and np.array_equal(g["counts"], want["counts"])
    assert rc.same_result(g["result"], want) and rc.same_records(g["inliers"], want["records"])
    A = gc.restate(gc.HOMOGRAPHY, g["result"].matrix(), 1.5, xa, xb)
    assert A[g["inliers"]["left"], g["inliers"]["right"]].all()
    truth = rc.passes([1, 0, 5, 0, 1, 3, 0, 0, 1], 1.5, rc.correspondences(pairs, xa, xb)).sum()
    print("real descriptors: %d pairs, true translation admits %d, estimated model keeps %d (sample %d, refit kept %d)"
          % (len(pairs), truth, g["count"], g["result"].sample_inliers, g["result"].refit_kept))
    assert truth > 50 and 2 * g["count"] >= truth


def test_cpp_estimate_homography_on_the_gpu(tmp_path):
    """tests/cpp/test_ransac_api.cpp with POPSIFT_TEST_EXPECT_GPU: FeaturesDev::estimateHomography equals the C-ABI on the
    same device arrays, its guide is accepted by matchPairsGuided, invalid options throw"""
    libdir = os.path.join(ROOT, "popsift_amd", "lib")
    exe = str(tmp_path / "test_ransac_api")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-pthread", os.path.join(ROOT, "tests", "cpp", "test_ransac_api.cpp"), "-o", exe,
                           "-I", os.path.join(ROOT, "popsift_amd", "csrc", "include"), "-I", os.path.join(ROOT, "include"),
                           "-L", libdir, "-lpopsift", "-lpopsift_hip", "-Wl,-rpath," + libdir])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300,
                         env=dict(os.environ, POPSIFT_TEST_EXPECT_GPU="1"))
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout
    assert "estimateHomography:" in out.stdout


def _write_pgm(path, img):
    with open(path, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (img.shape[1], img.shape[0]) + img.tobytes())


def _printed_model(stdout):
    line = [l for l in stdout.splitlines() if l.startswith("Homography:")][0]
    m = np.array([float(v) for v in line.split()[1:]], np.float32)           # %.9g: float32 round trip
    assert m.shape == (9,)
    return m


def test_match_tool_verify_homography(capi, tmp_path):
    """popsift-match --pairs FILE --verify-homography 1.5 --ransac-refit prints the nine entries and the inlier count and
    writes only the inliers; --rematch writes the guided list; the usage errors are reported.  Descriptor ORDER is not
    reproducible between runs (so neither are the samples): the rows are compared, as sorted distances, with what the
    restated rule keeps of capi's pairs -- and what capi's guided matcher returns -- under the model the tool PRINTED; the
    count is also held against capi.ransac_homography's on the same images."""
    a, b = _crops()
    _write_pgm(tmp_path / "l.pgm", a)
    _write_pgm(tmp_path / "r.pgm", b)
    (da, xa), (db, xb) = _extract(capi, a), _extract(capi, b)
    pairs = capi.match_pairs(da, db, 0.8, True)
    pts = rc.correspondences(pairs, xa, xb)
    want = capi.ransac_homography(pairs, xa, xb, capi.ransac_opts(1.5, 500, 7, True))
    common = [MATCH, "-l", "l.pgm", "-r", "r.pgm", "--octaves", "3", "--norm-multi", "9"]
    verify = ["--mutual", "--verify-homography", "1.5", "--ransac-hypotheses", "500", "--ransac-seed", "7", "--ransac-refit"]
    fmt = lambda recs: sorted(("%.3f" % x, "%.3f" % y) for x, y in zip(recs["d1"], recs["d2"]))
    out = tmp_path / "pairs.txt"
    p = subprocess.run(common + ["--pairs", str(out)] + verify, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    rows = [l.split() for l in out.read_text().splitlines()]
    assert "Homography inliers: %d of %d" % (len(rows), len(pairs)) in p.stdout and "Number of matches: %d" % len(rows) in p.stdout
    keep = rc.passes(_printed_model(p.stdout), 1.5, pts)
    assert len(rows) == keep.sum() > 50 and sorted((r[4], r[5]) for r in rows) == fmt(pairs[keep])
    print("tool: %d inliers; capi.ransac_homography on the same images: %d" % (len(rows), want["count"]))
    assert abs(len(rows) - want["count"]) <= 0.05 * want["count"]
    p = subprocess.run(common + ["--pairs", str(out)] + verify + ["--rematch"], cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    rows = [l.split() for l in out.read_text().splitlines()]
    guided = capi.match_pairs_guided(da, xa, db, xb, capi.Guide.homography(_printed_model(p.stdout), 1.5), 0.8, True)
    assert "Number of matches: %d" % len(rows) in p.stdout and len(rows) >= keep.sum() - 5
    assert sorted((r[4], r[5]) for r in rows) == fmt(guided)
    ident = "1,0,0,0,1,0,0,0,1"
    for extra, msg in ((["--verify-homography", "1.5"], "'--verify-homography' needs '--pairs'"),
                       (["--pairs", "p.txt", "--rematch"], "'--rematch' needs '--verify-homography'"),
                       (["--pairs", "p.txt", "--ransac-refit"], "need '--verify-homography'"),
                       (["--pairs", "p.txt", "--verify-homography", "1.5", "--homography", ident, "--guide-tol", "2"], "cannot be combined"),
                       (["--pairs", "p.txt", "--verify-homography", "1.5", "--fundamental", ident, "--guide-tol", "2"], "cannot be combined")):
        p = subprocess.run(common + extra, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
        assert p.returncode != 0 and msg in p.stderr, (extra, p.stderr)
