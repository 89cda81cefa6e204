"""CPU tests of the affine and similarity estimators' host side (include/popsift_hip.h, "geometric verification"):
psx_ransac_samples_k with k = 2 and 3, psx_affine_fit, psx_similarity_fit, psx_ransac_affine_ref, psx_ransac_similarity_ref
and the batched references -- which share csrc/hip/affine_rule.h with the kernels -- against the independent restatement
of tests/affine_cases.py, bit for bit; the premises of the inputs; properties that do not depend on the rule (the planted
pairs are recovered, the last row is exactly 0 0 1, a similarity is one); accuracy against numpy's least squares; argument
errors with nothing written; and a stand-alone sanitizer build of the rule."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import affine_cases as ac

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = {"affine": "ransac_affine_ref", "similarity": "ransac_similarity_ref"}
FIT = {"affine": "affine_fit", "similarity": "similarity_fit"}


@pytest.mark.parametrize("k", [2, 3])
def test_samples_equal_the_restatement(capi, k):
    model = "similarity" if k == 2 else "affine"
    for n, N, seed in ac.shapes(model):
        if n < k:
            buf = np.full(k * N, -7, np.int32)
            assert capi.lib().psx_ransac_samples_k(seed, 0, N, n, k, buf.ctypes.data_as(C.c_void_p)) == -1 and np.all(buf == -7)
            continue
        got = capi.ransac_samples(seed, 0, N, n, k=k)
        assert got.shape == (N, k) and got.tolist() == [ac.samples(seed, h, n, k) for h in range(N)], (n, N)


@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("n", [4, 5, 1000])
def test_samples_are_the_first_draws_of_four(capi, n, k):
    """all 65536 hypotheses: distinct, in range, the first k columns of the k = 4 draws; the restatement on every 251st and
    on the last; the argument errors of psx_ransac_samples_k"""
    got = capi.ransac_samples(1234 + n, 0, 65536, n, k=k)
    assert got.shape == (65536, k) and got.min() >= 0 and got.max() < n
    s = np.sort(got, 1)
    assert (s[:, 1:] != s[:, :-1]).all()
    assert np.array_equal(got, capi.ransac_samples(1234 + n, 0, 65536, n)[:, :k])
    for h in list(range(0, 65536, 251)) + [65535]:
        assert got[h].tolist() == ac.samples(1234 + n, h, n, k)
    assert np.array_equal(capi.ransac_samples(1234 + n, 65530, 6, n, k=k), got[65530:])
    L = capi.lib()
    buf = np.full(16, -7, np.int32)
    for first, count, kk in ((65536, 1, k), (-1, 1, k), (0, -1, k), (65535, 2, k), (0, 1, 0), (0, 1, 1), (0, 1, 5), (0, 1, 9)):
        assert L.psx_ransac_samples_k(0, first, count, n, kk, buf.ctypes.data_as(C.c_void_p)) == -1 and np.all(buf == -7)
    assert L.psx_ransac_samples_k(0, 0, 1, n, k, None) == -1
    assert L.psx_ransac_samples_k(0, 0, 1, k - 1, k, buf.ctypes.data_as(C.c_void_p)) == -1 and np.all(buf == -7)
    assert L.psx_ransac_samples_k(0, 0, 1, k, k, buf.ctypes.data_as(C.c_void_p)) == 0 and sorted(buf[:k].tolist()) == list(range(k))


@pytest.mark.parametrize("model,kind,n,N,seed", ac.CASES, ids=ac.CASE_IDS)
def test_fit_equals_the_restatement_on_every_minimal_sample(capi, model, kind, n, N, seed):
    """every hypothesis' points -- the degenerate samples of the "shared" scene among them -- and the inlier set the refit
    works on"""
    k = ac.MIN[model]
    if n < k:
        return
    pairs, lxy, rxy, _ = ac.planted(n, seed, kind)
    pts = ac.correspondences(pairs, lxy, rxy)
    want = ac.expect(model, kind, n, N, seed, False)
    fit = getattr(capi, FIT[model])
    for h in range(N):
        idx = ac.samples(seed, h, n, k)
        got = fit(pts[idx, 0:2], pts[idx, 2:4])
        assert np.array_equal(ac.bits(got), ac.bits(want["models"][h])), h
    if want["best"] < 0:
        return
    sel = ac.passes(want["m"], ac.TOL, pts)
    assert sel.sum() >= k
    got = fit(pts[sel, 0:2], pts[sel, 2:4])
    assert np.array_equal(ac.bits(got), ac.bits(ac.fit(model, pts[sel, 0:2], pts[sel, 2:4])))
    assert np.array_equal(ac.bits(got), ac.bits(ac.expect(model, kind, n, N, seed, True)["m"]))


@pytest.mark.parametrize("model", ac.MODELS)
def test_fit_in_order_equals_the_restatement(capi, model):
    for kind in ac.SCENES[model]:
        pts, _ = ac.scene(300, 7, kind)
        k = ac.MIN[model]
        for n in (k, k + 1, 64, 300):
            got, want = getattr(capi, FIT[model])(pts[:n, 0:2], pts[:n, 2:4]), ac.fit(model, pts[:n, 0:2], pts[:n, 2:4])
            assert np.array_equal(ac.bits(got), ac.bits(want)), (kind, n)
            # pairs 0 and 1 of the shared scene have one left position: d = 0 for the similarity, a zero pivot for the affine fit
            assert np.isfinite(want).all() != (kind == "shared" and n == k), (kind, n)


@pytest.mark.parametrize("refit", [False, True], ids=["sample", "refit"])
@pytest.mark.parametrize("model,kind,n,N,seed", ac.CASES, ids=ac.CASE_IDS)
def test_reference_equals_the_restatement(capi, model, kind, n, N, seed, refit):
    pairs, lxy, rxy, _ = ac.planted(n, seed, kind)
    want = ac.expect(model, kind, n, N, seed, refit)
    ref = getattr(capi, REF[model])
    got = ref(pairs, lxy, rxy, capi.ransac_opts(ac.TOL, N, seed, refit), layers=True)
    if n >= ac.MIN[model]:
        assert np.array_equal(ac.bits(got["models"]), ac.bits(want["models"]))
        assert np.array_equal(got["counts"], want["counts"])
    assert ac.same_result(got["result"], want), (got["result"].best, want["best"])
    assert got["count"] == want["inliers"] and ac.same_records(got["inliers"], want["records"])
    assert got["result"].guide(ac.TOL).kind == capi.GUIDE_HOMOGRAPHY
    if want["best"] >= 0:
        assert got["result"].matrix().reshape(9)[6:].tolist() == [0.0, 0.0, 1.0]
    if (n, N, seed) in ac.tie_shapes(model) and want["best"] >= 0:
        tied = np.nonzero(want["counts"] == want["counts"].max())[0]
        assert len(tied) > 1 and got["result"].best == tied[0]
    # records of the byte matcher: the same indices give the same result, the payload is copied whole
    pu = ac.planted(n, seed, kind, u8=True)[0]
    gu = ref(pu, lxy, rxy, capi.ransac_opts(ac.TOL, N, seed, refit))
    assert ac.same_result(gu["result"], want) and np.array_equal(gu["inliers"]["left"], want["records"]["left"])
    assert gu["inliers"].dtype == ac.PAIR_U8_DTYPE and np.array_equal(gu["inliers"]["d2"], 2 * (gu["inliers"]["d1"] - 1) + 7)
    # capacity: the total is reported, the bytes behind the capacity stay
    total = want["inliers"]
    L = capi.lib()
    o = capi.ransac_opts(ac.TOL, N, seed, refit)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None
    for cap in sorted({max(total - 1, 0), 0}):
        buf = np.full((cap + 2) * 4, -7, np.int32)
        res, cnt = capi.RansacResult(), C.c_int(-1)
        rv = getattr(L, "psx_" + REF[model])(ptr(pairs), n, ptr(lxy), n, ptr(rxy), n, C.byref(o), C.byref(res), ptr(buf) if cap else None, cap,
                                             C.byref(cnt), None, None)
        assert rv == 0 and cnt.value == total and ac.same_result(res, want)
        assert ac.same_records(buf[:4 * cap].view(ac.PAIR_DTYPE), want["records"][:cap]) and np.all(buf[4 * cap:] == -7)


def _many_sets(model, kind):
    """the batched reference's input: (0, 1, MIN, 64, 65, 300, 0) pairs against right arrays of their own"""
    k = ac.MIN[model]
    return [ac.planted(n, 40 + i, kind) for i, n in enumerate((0, 1, k, 64, 65, 300, 0))]


@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
@pytest.mark.parametrize("refit", [False, True], ids=["sample", "refit"])
@pytest.mark.parametrize("model", ac.MODELS)
def test_many_reference_equals_the_restatement(capi, model, refit, u8):
    """every set's result, the layers and the concatenated records of psx_ransac_*_many_ref equal the restatement set by
    set; all sets share one left array (each set's left indices are moved behind those of the sets before it)"""
    kind = ac.SCENES[model][0]
    sets = _many_sets(model, kind)
    N, seed = 65, 3
    off = np.cumsum([0] + [len(s[1]) for s in sets])
    lxy = np.concatenate([s[1] for s in sets])
    lists = []
    for i, s in enumerate(sets):
        p = ac.planted(len(s[0]), 40 + i, kind, u8=u8)[0].copy()
        p["left"] += off[i]
        lists.append(p)
    got = getattr(capi, "ransac_%s_many_ref" % model)(lists, lxy, [s[2] for s in sets], capi.ransac_opts(ac.TOL, N, seed, refit), layers=True)
    total = 0
    for i, s in enumerate(sets):
        want = ac.ransac(model, lists[i], lxy, s[2], ac.TOL, N, seed, refit)
        assert ac.same_result(got["results"][i], want), i
        assert ac.same_records(got["inliers"][i], want["records"]), i
        assert np.array_equal(ac.bits(got["models"][i]), ac.bits(want["models"])) and np.array_equal(got["counts"][i], want["counts"])
        assert (want["best"] >= 0) == (len(s[0]) >= ac.MIN[model])
        total += want["inliers"]
    assert got["count"] == total and len(got["records"]) == total
    # every set below the minimum: no model anywhere, nothing written
    few = [l[:ac.MIN[model] - 1] for l in lists]
    got = getattr(capi, "ransac_%s_many_ref" % model)(few, lxy, [s[2] for s in sets], capi.ransac_opts(ac.TOL, N, seed, refit), layers=True)
    assert got["count"] == 0 and all(r.best == -1 and not r.matrix().any() for r in got["results"]) and not got["models"].any()


def test_premises_of_the_inputs():
    """from the restatement alone, at tol 2: below the minimum there is no model; the tie shapes have more than one
    hypothesis at the largest count and best is the lowest of them; the "shared" scene has hypotheses with non-finite
    models, every one of which counts 0 -- at n = 2 all of them, which is "no model" at n >= MIN; where a model is kept
    the refit is kept too and loses no inlier"""
    degenerate = 0
    for (model, kind, n, N, seed) in ac.CASES:
        a, b = ac.expect(model, kind, n, N, seed, False), ac.expect(model, kind, n, N, seed, True)
        if n < ac.MIN[model]:
            assert a["best"] == b["best"] == -1 and a["inliers"] == 0 and not a["m"].any()
            continue
        bad = ~np.isfinite(a["models"]).all(1)
        assert not a["counts"][bad].any()
        if kind != "shared":
            assert not bad.any(), (model, kind, n)
        degenerate += int(bad.sum())
        if (model, kind, n) == ("similarity", "shared", 2):
            assert bad.all() and a["best"] == b["best"] == -1 and not a["m"].any() and a["inliers"] == 0
            continue
        c = a["counts"]
        assert a["best"] == int(np.argmax(c)) and b["refit_kept"] == 1 and b["inliers"] >= a["inliers"] == a["sample_inliers"] == c.max()
        if (n, N, seed) in ac.tie_shapes(model):
            assert (c == c.max()).sum() > 1 and c.max() == n
    assert degenerate >= 40, degenerate


@pytest.mark.parametrize("model,kind", [(m, k) for m in ac.MODELS for k in ac.SCENES[m]])
@pytest.mark.parametrize("n,N,seed", [(300, 256, 7), (2500, 512, 8)], ids=["n300_N256", "n2500_N512"])
def test_every_planted_pair_is_an_inlier(capi, model, kind, n, N, seed):
    """independent of the rule: the planted pairs lie within 1.5 px of the true transform, the tolerance is 2; with the
    refit the kept model admits every one of them, and its last row is exactly (0, 0, 1)"""
    pairs, lxy, rxy, is_planted = ac.planted(n, seed, kind)
    got = getattr(capi, REF[model])(pairs, lxy, rxy, capi.ransac_opts(ac.TOL, N, seed, True))
    planted_ids = set(pairs["d1"][is_planted].tolist())
    found = planted_ids & set(got["inliers"]["d1"].tolist())
    print("%s on %s (%d, %d, %d): %d of %d planted pairs among %d inliers" % (model, kind, n, N, seed, len(found), len(planted_ids), got["count"]))
    assert found == planted_ids
    m = got["result"].matrix().reshape(9)
    assert m[6:].tobytes() == np.array([0, 0, 1], np.float32).tobytes()
    assert np.abs(m[:6] - ac.TRUE[kind][:6]).max() < 0.5


def test_a_similarity_is_one(capi):
    """independent of the rule: on centred input of unit scale (the normalisation of the left side is then the identity: the
    centroid is 0, the mean L1 deviation 1) psx_similarity_fit returns m0 == m4 and m1 == -m3 exactly, whatever the right
    side is -- the model cannot represent a reflection: a mirrored right side gives a fit that misses its own points"""
    left = np.array([[0.5, 0.5], [-0.5, 0.5], [-0.5, -0.5], [0.5, -0.5]], np.float32)          # centroid 0, sum |x| + |y| = 4
    rng = np.random.default_rng(3)
    for trial in range(20):
        right = rng.uniform(-1, 1, (4, 2)).astype(np.float32)
        right -= right.mean(0)
        right = right.astype(np.float32)
        m = capi.similarity_fit(left, right)
        assert np.isfinite(m).all() and m[0] == m[4] and m[1] == -m[3] and m[6:].tolist() == [0.0, 0.0, 1.0], (trial, m)
    # the same through the restatement's normalised rows on any input
    pts, _ = ac.scene(50, 3, "similarity")
    with np.errstate(all="ignore"):
        _, _, _, X, Y = ac._side(*ac._columns(pts[:, 0:2]))
        _, _, _, U, V = ac._side(*ac._columns(pts[:, 2:4]))
        (a, b, c), (d, e, f) = ac.normalised_similarity(X, Y, U, V)
    assert a == e and b == -d and c == 0.0 and f == 0.0
    # a rotation comes back, a reflection does not
    ang = 0.7
    rot = np.array([[np.cos(ang), -np.sin(ang)], [np.sin(ang), np.cos(ang)]])
    m = capi.similarity_fit(left, (left @ rot.T).astype(np.float32))
    assert np.abs(ac.transfer(m, left) - left @ rot.T).max() < 1e-6
    mirror = (left[:3] * np.array([1.5, -1.5]) + np.array([[0.3, 0.0], [0.0, 0.2], [0.0, 0.0]])).astype(np.float32)
    m = capi.similarity_fit(left[:3], mirror)
    assert np.abs(ac.transfer(m, left[:3]) - mirror).max() > 0.5
    m = capi.affine_fit(left[:3], mirror)
    assert np.abs(ac.transfer(m, left[:3]) - mirror).max() < 1e-6


def _lstsq(model, pts):
    """numpy's least squares in float64 on the same float32 positions, without normalisation; rounded to float32"""
    p = np.asarray(pts, np.float64)
    x, y, u, v = p[:, 0], p[:, 1], p[:, 2], p[:, 3]
    one, zero = np.ones(len(p)), np.zeros(len(p))
    if model == "affine":
        A = np.stack([x, y, one], 1)
        r0 = np.linalg.lstsq(A, u, rcond=None)[0]
        r1 = np.linalg.lstsq(A, v, rcond=None)[0]
    else:
        A = np.concatenate([np.stack([x, -y, one, zero], 1), np.stack([y, x, zero, one], 1)])
        a, b, tx, ty = np.linalg.lstsq(A, np.concatenate([u, v]), rcond=None)[0]
        r0, r1 = [a, -b, tx], [b, a, ty]
    return np.array(list(r0) + list(r1) + [0, 0, 1], np.float64).astype(np.float32)


@pytest.mark.parametrize("model", ac.MODELS)
def test_fit_is_as_accurate_as_least_squares(capi, model):
    """Independent of the rule.  Noise-free planted scenes of n = 3, 50 and 300 points (the true transform applied to the
    left positions, both sides rounded to float32).  The quantity compared is the largest distance, over the scene's
    points, between where psx_*_fit's model and where numpy.linalg.lstsq's model (float64 on the same float32 positions,
    rounded to float32) send a left point.  The allowance is four times the largest distance between where lstsq's own
    float32-rounded model and where the planted transform send a left point, measured first: both models are rounded to
    float32, and the rule normalises where lstsq does not.
    Measured (rule against lstsq / lstsq against the truth), px: similarity n = 3: 0 / 4.0e-5, 50: 0 / 3.7e-6, 300: 0 /
    3.1e-6; affine n = 3: 0 / 3.4e-5, 50: 0 / 1.6e-5, 300: 0 / 1.7e-5 -- on noise-free input both least-squares solutions
    round to the same nine float32 values."""
    kind = ac.SCENES[model][0]
    for n in (3, 50, 300):
        pts, _ = ac.scene(n, 21, kind, noise=False)
        left = pts[:, 0:2]
        book = _lstsq(model, pts)
        floor = np.hypot(*(ac.transfer(book, left) - ac.apply(ac.TRUE[kind], left)).T).max()
        ours = getattr(capi, FIT[model])(left, pts[:, 2:4])
        dist = np.hypot(*(ac.transfer(ours, left) - ac.transfer(book, left)).T).max()
        print("%s n = %d: rule against lstsq %.3g px, lstsq against the truth %.3g px" % (model, n, dist, floor))
        assert floor > 0 and dist <= 4 * floor, (model, n, dist, floor)


@pytest.mark.parametrize("model", ac.MODELS)
def test_argument_errors_write_nothing(capi, model):
    L = capi.lib()
    kind = ac.SCENES[model][0]
    pairs, lxy, rxy, _ = ac.planted(65, 5, kind)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    ok = capi.ransac_opts(2.0, 16, 0, True)
    k = ac.MIN[model]

    def call(p=pairs, n=65, l=lxy, nl=65, r=rxy, nr=65, o=ok, cap=65, with_out=True, with_res=True, with_cnt=True):
        out = np.full(66 * 4, -7, np.int32)
        models, counts = np.full(16 * 9, -7, np.float32), np.full(16, -7, np.int32)
        res = capi.RansacResult()
        C.memset(C.byref(res), 0x5a, C.sizeof(res))
        cnt = C.c_int(-77)
        rv = getattr(L, "psx_" + REF[model])(ptr(p) if p is not None else None, n, ptr(l) if l is not None else None, nl,
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
    bad = pairs[:k - 1].copy()
    bad["left"][0] = -1
    assert call(p=bad, n=k - 1) == (-1, True)
    rv, untouched = call(n=k - 1)
    assert rv == 0 and not untouched
    got = getattr(capi, REF[model])(pairs[:k - 1], lxy, rxy, ok, layers=True)
    assert got["result"].best == -1 and got["count"] == 0 and not got["result"].matrix().any() and got["result"].inliers == 0
    assert call(o=capi.RansacOpts(0.0, 16, 0, 1))[0] == 0                  # tol 0 is a valid option
    # the batched reference
    many = getattr(L, "psx_ransac_%s_many_ref" % model)
    sc = np.array([65], np.int32)
    rp = (C.c_void_p * 1)(rxy.ctypes.data)
    lens = np.array([65], np.int32)

    def call_many(o=ok, n_sets=1, counts=sc, rptrs=rp, rl=lens, with_res=True, cap=65):
        out = np.full(66 * 4, -7, np.int32)
        res = capi.RansacResult()
        C.memset(C.byref(res), 0x5a, C.sizeof(res))
        cnt = C.c_int(-77)
        rv = many(ptr(pairs), ptr(counts) if counts is not None else None, n_sets, ptr(lxy), 65, rptrs, ptr(rl) if rl is not None else None,
                  C.byref(o), C.byref(res) if with_res else None, ptr(out), cap, C.byref(cnt), None, None)
        return rv, bool(np.all(out == -7) and cnt.value == -77 and bytes(res) == b"\x5a" * C.sizeof(res))

    assert call_many()[0] == 0
    for kw in (dict(o=bad_opts[0]), dict(n_sets=-1), dict(counts=None), dict(rptrs=None), dict(rl=None), dict(with_res=False), dict(cap=-1),
               dict(counts=np.array([-1], np.int32)), dict(rl=np.array([10], np.int32)), dict(rptrs=(C.c_void_p * 1)(None))):
        assert call_many(**kw) == (-1, True), kw
    # the fit
    out = np.full(9, -7, np.float32)
    fit = getattr(L, "psx_" + FIT[model])
    lk, rk = np.ascontiguousarray(lxy[:k]), np.ascontiguousarray(rxy[:k])
    assert fit(ptr(lk), ptr(rk), k - 1, ptr(out)) == -1
    assert fit(None, ptr(rk), k, ptr(out)) == -1 and fit(ptr(lk), None, k, ptr(out)) == -1
    assert fit(ptr(lk), ptr(rk), k, None) == -1 and np.all(out == -7)
    assert fit(ptr(lk), ptr(rk), k, ptr(out)) == 0 and np.isfinite(out).all()


def test_declarations_and_bindings(capi):
    hdr = open(os.path.join(ROOT, "include", "popsift_hip.h")).read()
    syms = []
    for model in ac.MODELS:
        syms += ["psx_%s_fit" % model] + ["psx_ransac_%s%s" % (model, s) for s in ("_ref", "", "_dev", "_many", "_many_dev", "_many_ref")]
    assert len(syms) == 14
    for sym in syms:
        assert "int %s(" % sym in hdr and sym in capi.SYMBOLS and hasattr(capi.lib(), sym), sym
    for model in ac.MODELS:
        for name in ("%s_fit", "ransac_%s_ref", "ransac_%s", "ransac_%s_dev", "ransac_%s_many_ref", "ransac_%s_many", "ransac_%s_many_dev"):
            assert callable(getattr(capi, name % model))
        assert callable(getattr(capi.DeviceDescriptors, "ransac_%s" % model))
    assert "(0, 0, 1)" in hdr and "cannot represent a reflection" in hdr
    feat = open(os.path.join(ROOT, "popsift_amd", "csrc", "include", "popsift", "features.h")).read()
    for name in ("estimateAffine(", "estimateSimilarity(", "estimateAffineMany(", "estimateSimilarityMany("):
        assert "HomographyEstimate" in feat and name in feat
    rule = open(os.path.join(ROOT, "popsift_amd", "csrc", "hip", "affine_rule.h")).read()
    assert "sqrt" not in rule and "fma" not in rule.replace("fused multiply-add", "")
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "psx_ransac_affine" in text and "psx_ransac_similarity" in text, doc
    assert "estimateSimilarityMany" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


@pytest.mark.parametrize("model", ac.MODELS)
def test_match_tool_usage_errors(model, tmp_path):
    """popsift-match --verify-affine / --verify-similarity: what --verify-homography refuses, refused before a device or a
    file is touched, in messages that name the option"""
    exe = os.path.join(ROOT, "popsift_amd", "lib", "popsift-match")
    opt = "--verify-" + model
    other = "--verify-similarity" if model == "affine" else "--verify-affine"
    ident = "1,0,0,0,1,0,0,0,1"
    common = [exe, "-l", "l.pgm", "-r", "r.pgm"]
    for extra, msg in (([opt, "1.5"], "'%s' needs '--pairs'" % opt),
                       (["--pairs", "p.txt", "--rematch"], "'--rematch' needs '--verify-homography'"),
                       (["--pairs", "p.txt", "--rematch"], "'%s'" % opt),
                       (["--pairs", "p.txt", "--ransac-refit"], "'%s'" % opt),
                       (["--pairs", "p.txt", opt, "1.5", other, "1.5"], "cannot be combined"),
                       (["--pairs", "p.txt", opt, "1.5", "--verify-homography", "1.5"], "cannot be combined"),
                       (["--pairs", "p.txt", opt, "1.5", "--verify-fundamental", "1.5"], "cannot be combined"),
                       (["--pairs", "p.txt", opt, "1.5", "--homography", ident, "--guide-tol", "2"], "cannot be combined"),
                       (["--pairs", "p.txt", opt, "nan"], "tolerance must be finite"),
                       (["--pairs", "p.txt", opt, "1.5", "--ransac-hypotheses", "0"], "1 .. 65536")):
        p = subprocess.run(common + extra, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
        assert p.returncode != 0 and msg in p.stderr, (extra, p.stderr[:300])
    p = subprocess.run([exe, "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert p.returncode == 0 and opt in p.stdout


def test_cpp_api_argument_errors_without_a_device(tmp_path):
    """tests/cpp/test_affine_api.cpp without POPSIFT_TEST_EXPECT_GPU: estimateAffine's, estimateSimilarity's, the batched
    forms' and the C-ABI's argument checks, all before a device is touched"""
    libdir = os.path.join(ROOT, "popsift_amd", "lib")
    exe = str(tmp_path / "test_affine_api")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-pthread", os.path.join(ROOT, "tests", "cpp", "test_affine_api.cpp"), "-o", exe,
                           "-I", os.path.join(ROOT, "popsift_amd", "csrc", "include"), "-I", os.path.join(ROOT, "include"),
                           "-L", libdir, "-lpopsift", "-lpopsift_hip", "-Wl,-rpath," + libdir])
    env = {k: v for k, v in os.environ.items() if k != "POPSIFT_TEST_EXPECT_GPU"}
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120, env=env)
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout


def test_affine_rule_under_sanitizers(tmp_path):
    """tests/cpp/affine_rule_san.cpp: a stand-alone program (its own main) that includes affine_rule.h alone and drives the
    samples, both fits (minimal, dynamic n, a duplicated point, a zero-extent side, collinear points) and the whole host
    rule over the smallest shapes, the degenerate ones included, on exact-size heap arrays -- compiled with
    -ffp-contract=off -fsanitize=address,undefined and run directly."""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed"
    exe = str(tmp_path / "affine_rule_san")
    cmd = [cxx, "-std=c++14", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan",
           os.path.join(ROOT, "tests", "cpp", "affine_rule_san.cpp"), "-o", exe,
           "-I", os.path.join(ROOT, "popsift_amd", "csrc", "hip"), "-I", os.path.join(ROOT, "include")]
    subprocess.check_call(cmd)
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout
