"""GPU tests of the affine and similarity estimators (include/popsift_hip.h, "geometric verification"): psx_ransac_affine,
psx_ransac_similarity, their _dev, _many and _many_dev forms, FeaturesDev::estimateAffine / estimateSimilarity and
popsift-match --verify-affine / --verify-similarity.  The device
is held to the host references psx_ransac_*_ref -- which tests/test_affine_cpu.py holds to the independent restatement of
tests/affine_cases.py -- bit for bit: models as 32-bit patterns, counts, the result struct and the inlier records exactly;
the batched calls to the loop of single calls on the same device arrays."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch        # before the HIP library is loaded: torch brings a HIP runtime of its own and must initialise first (_dev forms)

from popsift_amd.synth import synth
from tests import affine_cases as ac
from tests import guided_cases as gc
from tests.ransac_cases import bits, same_records

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


def _raw(capi, pos, model, pairs, opts, cap, with_layers=True):
    """psx_ransac_<model> with sentinel-filled outputs: (rc, result, count, out int32 words, models, counts)"""
    N = opts.hypotheses
    out = np.full((cap + 2) * 4, -7, np.int32)
    models, counts = np.full((N, 9), -7, np.float32), np.full(N, -7, np.int32)
    res, cnt = capi.RansacResult(), C.c_int(-77)
    C.memset(C.byref(res), 0x5a, C.sizeof(res))
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    rv = getattr(pos.L, "psx_ransac_" + model)(0, ptr(pairs) if len(pairs) else None, len(pairs), pos.plx, pos.nl, pos.prx, pos.nr, C.byref(opts),
                                               C.byref(res), ptr(out) if cap else None, cap, C.byref(cnt),
                                               ptr(models) if with_layers else None, ptr(counts) if with_layers else None)
    return rv, res, cnt.value, out, models, counts


def _ref(capi, model, pairs, lxy, rxy, opts):
    return getattr(capi, "ransac_%s_ref" % model)(pairs, lxy, rxy, opts, layers=True)


@pytest.mark.parametrize("model,kind,n,N,seed", ac.CASES, ids=ac.CASE_IDS)
def test_device_equals_the_reference(capi, model, kind, n, N, seed):
    """host form and _dev form, refit off and on, at capacity n and at capacity total - 1: the models layer, the counts, the
    result struct, the records and *count equal psx_ransac_*_ref; nothing is written behind the capacity"""
    pairs, lxy, rxy, _ = ac.planted(n, seed, kind)
    pos = _Positions(capi, lxy, rxy)
    try:
        dpairs = torch.from_numpy(np.ascontiguousarray(pairs).view(np.uint8).copy()).cuda() if n else None
        for refit in (False, True):
            opts = capi.ransac_opts(ac.TOL, N, seed, refit)
            ref = _ref(capi, model, pairs, lxy, rxy, opts)
            total = ref["count"]
            rv, res, cnt, out, models, counts = _raw(capi, pos, model, pairs, opts, n)
            assert rv == 0
            if n < ac.MIN[model]:
                assert res.best == -1 and cnt == 0 and res.inliers == 0 and not res.matrix().any()
                assert np.all(out == -7) and np.all(models == -7) and np.all(counts == -7)          # buffers untouched
                continue
            bad = np.nonzero((bits(models) != bits(ref["models"])).any(1))[0]
            assert len(bad) == 0, ("models differ from the reference at hypotheses", bad[:5], models[bad[:1]], ref["models"][bad[:1]])
            assert np.array_equal(counts, ref["counts"])
            assert bytes(res) == bytes(ref["result"]), (res.best, res.sample_inliers, res.inliers, ref["result"].best)
            assert cnt == total
            assert same_records(out[:4 * cnt].view(ac.PAIR_DTYPE), ref["inliers"]) and np.all(out[4 * cnt:] == -7)
            if res.best >= 0:
                assert res.matrix().reshape(9)[6:].tolist() == [0.0, 0.0, 1.0]
            if (n, N, seed) in ac.tie_shapes(model) and res.best >= 0:
                tied = np.nonzero(counts == counts.max())[0]
                assert len(tied) > 1 and res.best == tied[0]
            # the capacity cut, host form
            cut = max(total - 1, 0)
            rv, res2, cnt2, out2, _, _ = _raw(capi, pos, model, pairs, opts, cut, with_layers=False)
            assert rv == 0 and cnt2 == total and bytes(res2) == bytes(ref["result"])
            assert same_records(out2[:4 * cut].view(ac.PAIR_DTYPE), ref["inliers"][:cut]) and np.all(out2[4 * cut:] == -7)
            # the _dev form on torch buffers: full capacity and the cut
            for cap in (n, cut):
                dbuf = torch.full(((cap + 2) * 16,), 0xA5, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                g = getattr(capi, "ransac_%s_dev" % model)(dpairs.data_ptr(), n, pos.plx.value, n, pos.prx.value, n, dbuf.data_ptr() if cap else 0,
                                                           cap, opts, layers=True)
                back = dbuf.cpu().numpy()
                k = min(cap, total)
                assert g["count"] == total and bytes(g["result"])[:52] == bytes(ref["result"])[:52], cap
                assert np.array_equal(bits(g["models"]), bits(ref["models"])) and np.array_equal(g["counts"], ref["counts"])
                assert same_records(back[:k * 16].view(ac.PAIR_DTYPE), ref["inliers"][:k]) and np.all(back[k * 16:] == 0xA5), cap
                assert g["result"].guide(ac.TOL).kind == capi.GUIDE_HOMOGRAPHY
    finally:
        pos.close()


@pytest.mark.parametrize("model", ac.MODELS)
def test_byte_records_and_wrappers(capi, model):
    """records of the byte matcher's dtype give the same result as float records with the same indices, the payload
    carried; the python wrappers and DeviceDescriptors.ransac_* agree"""
    kind = ac.SCENES[model][0]
    n, N, seed = 300, 256, 7
    pairs, lxy, rxy, _ = ac.planted(n, seed, kind)
    pu = ac.planted(n, seed, kind, u8=True)[0]
    opts = capi.ransac_opts(ac.TOL, N, seed, True)
    ref = _ref(capi, model, pairs, lxy, rxy, opts)
    g = getattr(capi, "ransac_" + model)(pairs, lxy, rxy, opts)
    assert bytes(g["result"])[:52] == bytes(ref["result"])[:52] and same_records(g["inliers"], ref["inliers"])
    gu = getattr(capi, "ransac_" + model)(pu, lxy, rxy, opts)
    assert bytes(gu["result"])[:52] == bytes(ref["result"])[:52] and gu["inliers"].dtype == ac.PAIR_U8_DTYPE
    assert np.array_equal(gu["inliers"]["left"], ref["inliers"]["left"]) and np.array_equal(gu["inliers"]["d2"], 2 * (gu["inliers"]["d1"] - 1) + 7)
    dd = capi.DeviceDescriptors(np.zeros((n, 128), np.float32), xy=lxy), capi.DeviceDescriptors(np.zeros((n, 128), np.float32), xy=rxy)
    g = getattr(dd[0], "ransac_" + model)(dd[1], pairs, opts)
    assert bytes(g["result"])[:52] == bytes(ref["result"])[:52] and same_records(g["inliers"], ref["inliers"])
    assert g["result"].guide(1.0).kind == capi.GUIDE_HOMOGRAPHY
    dd[0].close(); dd[1].close()


@pytest.mark.parametrize("model", ac.MODELS)
def test_device_argument_errors_write_nothing(capi, model):
    """what the homography call refuses, with the same answer: invalid options, negative or empty position arrays, and a
    pair index outside its position array -- flagged by the gather kernel, nothing is read out of bounds"""
    pairs, lxy, rxy, _ = ac.planted(65, 5, ac.SCENES[model][0])
    pos = _Positions(capi, lxy, rxy)
    try:
        def answer(m, p=pairs, opts=capi.ransac_opts(2.0, 16, 0, True), cap=65, nl=None, nr=None):
            pos.nl, pos.nr = (65 if nl is None else nl), (65 if nr is None else nr)
            rv, res, cnt, out, models, counts = _raw(capi, pos, m, p, opts, cap)
            pos.nl = pos.nr = 65
            return rv, bool(np.all(out == -7) and np.all(models == -7) and np.all(counts == -7) and cnt == -77 and
                            bytes(res) == b"\x5a" * C.sizeof(res))

        def refused(**kw):
            a = answer(model, **kw)
            return a == (-1, True) and a == answer("homography", **kw)

        for o in (capi.RansacOpts(float("nan"), 16, 0, 0), capi.RansacOpts(-1.0, 16, 0, 0), capi.RansacOpts(float("inf"), 16, 0, 0),
                  capi.RansacOpts(2.0, 0, 0, 0), capi.RansacOpts(2.0, 65537, 0, 0), capi.RansacOpts(2.0, 16, 0, 4)):
            assert refused(opts=o), (o.tol, o.hypotheses, o.flags)
        assert refused(nl=-1) and refused(nr=-1) and refused(nl=0)
        bad = pairs.copy()
        bad["right"][40] = 65
        assert refused(p=bad)
        bad = pairs.copy()
        bad["left"][3] = -2
        assert refused(p=bad) and refused(nl=64)
        rv, res, cnt, out, _, _ = _raw(capi, pos, model, pairs, capi.ransac_opts(2.0, 16, 0, True), 65)
        assert rv == 0 and cnt == res.inliers >= ac.MIN[model]
    finally:
        pos.close()


class _Sets:
    """K pair lists against one left array and a right array per set, uploaded once"""

    def __init__(self, capi, model, kind, sizes, u8=False):
        self.L, self.bufs = capi.lib(), []
        sets = [ac.planted(n, 40 + i, kind, u8=u8) for i, n in enumerate(sizes)]
        off = np.cumsum([0] + [len(s[1]) for s in sets])
        self.lxy = np.concatenate([s[1] for s in sets]) if sets else np.zeros((0, 2), np.float32)
        if len(self.lxy) == 0:
            self.lxy = np.zeros((1, 2), np.float32)
        self.rxys = [np.asarray(s[2]) for s in sets]
        self.lists = []
        for i, s in enumerate(sets):
            p = s[0].copy()
            p["left"] += off[i]
            self.lists.append(p)
        self.dtype = ac.PAIR_U8_DTYPE if u8 else ac.PAIR_DTYPE
        ptrs = capi._to_device(self.L, 0, [self.lxy] + [r if len(r) else np.zeros((1, 2), np.float32) for r in self.rxys], self.bufs)
        self.plx, self.nl = ptrs[0], len(self.lxy)
        self.prx, self.lens = [p.value for p in ptrs[1:]], [len(r) for r in self.rxys]

    def close(self):
        for p in self.bufs:
            self.L.psx_dev_free(0, p)
        self.bufs = []


def _single(capi, dev, model, k, opts):
    """psx_ransac_<model> for set k on the same device arrays: the dict of capi._ransac_call"""
    name, kind = capi._ransac_names(model)
    pairs = dev.lists[k]
    fn = lambda *a: getattr(dev.L, name)(0, *a)
    return capi._ransac_call(fn, name, pairs.ctypes.data_as(C.c_void_p) if pairs.size else None, len(pairs), pairs.dtype, dev.plx, dev.nl,
                             C.c_void_p(dev.prx[k]), dev.lens[k], opts, None, True, kind=kind)


def _many_raw(capi, dev, model, opts, cap, dev_form=False):
    """psx_ransac_<model>_many (or _many_dev on torch buffers) with sentinel-filled outputs:
    (rc, results, count, out bytes, models, counts)"""
    K, N = len(dev.lists), opts.hypotheses
    pairs = np.concatenate(dev.lists) if K else np.zeros(0, dev.dtype)
    sc = np.array([len(p) for p in dev.lists], np.int32)
    la = np.array(dev.lens, np.int32)
    pa = (C.c_void_p * max(K, 1))(*dev.prx)
    models, counts = np.full((K, N, 9), -7, np.float32), np.full((K, N), -7, np.int32)
    res, cnt = (capi.RansacResult * max(K, 1))(), C.c_int(-77)
    C.memset(res, 0x5a, C.sizeof(res))
    ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None
    common = (ptr(sc), K, dev.plx, dev.nl, pa if K else None, ptr(la), C.byref(opts), res if K else None)
    if dev_form:
        dp = torch.from_numpy(pairs.view(np.uint8).copy()).cuda() if len(pairs) else None
        dout = torch.full(((cap + 2) * 16,), 0xA5, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        rv = getattr(dev.L, "psx_ransac_%s_many_dev" % model)(0, C.c_void_p(dp.data_ptr()) if dp is not None else None, *common,
                                                              C.c_void_p(dout.data_ptr()) if cap else None, cap, C.byref(cnt), ptr(models), ptr(counts))
        out = dout.cpu().numpy()
    else:
        out = np.full((cap + 2) * 16, 0xA5, np.uint8)
        rv = getattr(dev.L, "psx_ransac_%s_many" % model)(0, ptr(pairs), *common, ptr(out) if cap else None, cap, C.byref(cnt), ptr(models),
                                                          ptr(counts))
    return rv, res, cnt.value, out, models, counts


@pytest.mark.parametrize("refit", [False, True], ids=["sample", "refit"])
@pytest.mark.parametrize("model", ac.MODELS)
def test_many_equals_the_loop_of_single_calls(capi, model, refit):
    """K = 0, K = 1, K = 7 with per-set counts (0, 1, MIN, 64, 65, 300, 0), and a call in which every set is below MIN; host
    and _dev forms: every set's result and layers, the concatenated inlier list and *count equal the loop of single
    device calls and the host reference; sets without a model report best = -1; a capacity cut leaves the bytes behind it"""
    k = ac.MIN[model]
    kind = ac.SCENES[model][0]
    N, seed = 65, 3
    opts = capi.ransac_opts(ac.TOL, N, seed, refit)
    for sizes in ((), (300,), (0, 1, k, 64, 65, 300, 0), (k - 1, 0, k - 1)):
        dev = _Sets(capi, model, kind, sizes, u8=len(sizes) == 7)
        try:
            K = len(sizes)
            singles = [_single(capi, dev, model, i, opts) for i in range(K)]
            cat = np.concatenate([s["inliers"] for s in singles]) if K else np.zeros(0, dev.dtype)
            total = len(cat)
            ref = getattr(capi, "ransac_%s_many_ref" % model)(dev.lists, dev.lxy, dev.rxys, opts, layers=True)
            assert ref["count"] == total
            for dev_form in (False, True):
                for cap in sorted({sum(sizes), max(total - 1, 0)}, reverse=True):
                    rv, res, cnt, out, models, counts = _many_raw(capi, dev, model, opts, cap, dev_form)
                    w = min(cap, total)
                    assert rv == 0 and cnt == total, (sizes, dev_form, cap)
                    assert same_records(out[:16 * w].view(dev.dtype), cat[:w]) and np.all(out[16 * w:] == 0xA5), (sizes, dev_form, cap)
                    for i, n in enumerate(sizes):
                        assert bytes(res[i]) == bytes(singles[i]["result"])[:52] == bytes(ref["results"][i])[:52], (sizes, i)
                        if n >= k:
                            assert res[i].best >= 0 and res[i].matrix().reshape(9)[6:].tolist() == [0.0, 0.0, 1.0]
                            assert np.array_equal(bits(models[i]), bits(singles[i]["models"])) and np.array_equal(counts[i], singles[i]["counts"])
                        else:
                            assert res[i].best == -1 and res[i].inliers == 0 and not res[i].matrix().any()
                            assert not models[i].any() and not counts[i].any()
        finally:
            dev.close()


def test_match_verify_rematch_of_many_sets(capi):
    """the chain on planted byte descriptors at 300 x 257 (guided_cases.positioned): psx_match_pairs_many_u8_dev ->
    psx_ransac_similarity_many_dev on its output buffer and its set_counts -> psx_guides_from_ransac(HOMOGRAPHY) ->
    psx_match_pairs_guided_many_u8, against three right sets: the planted one, its rows reversed, and unrelated
    descriptors, which leave fewer than 2 pairs -- that set gets no model and is skipped through PSX_GUIDE_NONE.  Every
    set's verification equals the host reference on the downloaded slice, and the re-match equals the per-set single guided
    calls under the same guides."""
    left, right, lxy, rxy = gc.positioned(1, 300, 257)
    lq, rq = capi.quantize_rule(left), capi.quantize_rule(right)
    rng = np.random.default_rng(77)
    rights = [rq, np.ascontiguousarray(rq[::-1]), rng.integers(128, 255, (40, 128), dtype=np.uint8)]
    rxys = [np.asarray(rxy), np.ascontiguousarray(rxy[::-1]), rng.uniform(0, 30, (40, 2)).astype(np.float32)]
    L = capi.lib()
    bufs = []
    nl = len(lq)
    ptrs = capi._to_device(L, 0, [lq, np.asarray(lxy)] + rights + rxys, bufs)
    pl, plx, pr, prx = ptrs[0], ptrs[1], ptrs[2:5], ptrs[5:8]
    r_lens = [len(r) for r in rights]
    N, seed = 96, 11
    try:
        d_pairs = torch.full((3 * nl * 16,), 0xA5, dtype=torch.uint8, device="cuda")
        d_inl = torch.full((3 * nl * 16,), 0xA5, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        set_counts, n1 = capi.match_pairs_many_dev(pl.value, nl, [p.value for p in pr], r_lens, d_pairs.data_ptr(), 3 * nl, 0.8, True)
        assert n1 == int(np.sum(set_counts)) and int(set_counts[0]) >= 50 and int(set_counts[1]) >= 50 and int(set_counts[2]) < 2, set_counts
        opts = capi.ransac_opts(ac.TOL, N, seed, True)
        g = capi.ransac_similarity_many_dev(d_pairs.data_ptr(), set_counts, plx.value, nl, [p.value for p in prx], r_lens, d_inl.data_ptr(), 3 * nl,
                                            opts)
        pairs = d_pairs.cpu().numpy()[:n1 * 16].view(capi.PAIR_U8_DTYPE)
        inl = d_inl.cpu().numpy()
        lists = capi.split_sets(pairs, set_counts)
        at = 0
        for k in range(3):
            ref = capi.ransac_similarity_ref(lists[k], lxy, rxys[k], opts)
            res = g["results"][k]
            assert bytes(res)[:52] == bytes(ref["result"])[:52], (k, res.best, res.inliers, ref["result"].best)
            assert same_records(inl[at * 16:(at + res.inliers) * 16].view(capi.PAIR_U8_DTYPE), ref["inliers"])
            at += res.inliers
        assert at == g["count"] and np.all(inl[at * 16:] == 0xA5)
        assert g["results"][0].best >= 0 and g["results"][1].best >= 0 and g["results"][2].best == -1
        assert g["results"][0].inliers >= 30, g["results"][0].inliers
        guides = capi.guides_from_ransac(g["results"], capi.GUIDE_HOMOGRAPHY, ac.TOL)
        assert [gd.kind for gd in guides] == [capi.GUIDE_HOMOGRAPHY, capi.GUIDE_HOMOGRAPHY, capi.GUIDE_NONE]
        again, counts = capi.match_pairs_guided_many_u8(lq, lxy, rights, rxys, guides, 0.8, True)
        assert len(again[2]) == 0 and int(counts[2]) == 0
        for k in range(2):
            one = capi.match_pairs_guided_u8(lq, lxy, rights[k], rxys[k], guides[k], 0.8, True)
            assert same_records(again[k], one) and int(counts[k]) == len(one) > 0, k
            have = set(zip(one["left"].tolist(), one["right"].tolist()))
            mine = capi.ransac_similarity_ref(lists[k], lxy, rxys[k], opts)["inliers"]
            assert all((int(a), int(b)) in have for a, b in zip(mine["left"], mine["right"])), k
        assert L.psx_match_release() == 0
    finally:
        for p in bufs:
            L.psx_dev_free(0, p)


def test_three_pairs_are_enough(capi):
    """the case the feature exists for: a list of exactly 3 pairs, all planted.  The homography and fundamental calls
    return best = -1; the affine and similarity calls return a model that admits all three."""
    pts, _ = ac.scene(3, 5, "similarity")
    pairs = np.zeros(3, ac.PAIR_DTYPE)
    pairs["left"] = pairs["right"] = np.arange(3)
    lxy, rxy = np.ascontiguousarray(pts[:, 0:2]), np.ascontiguousarray(pts[:, 2:4])
    opts = capi.ransac_opts(ac.TOL, 16, 0, True)
    for model in ("homography", "fundamental"):
        g = getattr(capi, "ransac_" + model)(pairs, lxy, rxy, opts)
        assert g["result"].best == -1 and g["count"] == 0 and not g["result"].matrix().any(), model
        g = getattr(capi, "ransac_%s_many" % model)([pairs], lxy, [rxy], opts)
        assert g["results"][0].best == -1 and g["count"] == 0, model
    for model in ac.MODELS:
        g = getattr(capi, "ransac_" + model)(pairs, lxy, rxy, opts)
        assert g["result"].best >= 0 and g["count"] == 3 and same_records(g["inliers"], pairs), model
        m = g["result"].matrix().reshape(9)
        assert m[6:].tolist() == [0.0, 0.0, 1.0] and np.hypot(*(ac.transfer(m, lxy) - rxy).T).max() <= ac.TOL
        assert gc.restate(gc.HOMOGRAPHY, m, ac.TOL, lxy, rxy).diagonal().all()
        gm = getattr(capi, "ransac_%s_many" % model)([pairs], lxy, [rxy], opts)
        assert bytes(gm["results"][0])[:52] == bytes(g["result"])[:52] and gm["count"] == 3, model
        # the model guides a re-match
        guide = capi.guides_from_ransac([g["result"]], capi.GUIDE_HOMOGRAPHY, ac.TOL)[0]
        assert guide.kind == capi.GUIDE_HOMOGRAPHY and capi.guide_allows(guide, lxy, rxy).diagonal().all()


def test_cpp_estimate_affine_and_similarity_on_the_gpu(tmp_path):
    """tests/cpp/test_affine_api.cpp with POPSIFT_TEST_EXPECT_GPU: FeaturesDev::estimateAffine / estimateSimilarity and their
    Many forms equal the C-ABI on the same device arrays, the guide is a homography accepted by matchPairsGuided, three
    matches give a model where estimateHomography has none, invalid options throw"""
    libdir = os.path.join(ROOT, "popsift_amd", "lib")
    exe = str(tmp_path / "test_affine_api")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-pthread", os.path.join(ROOT, "tests", "cpp", "test_affine_api.cpp"), "-o", exe,
                           "-I", os.path.join(ROOT, "popsift_amd", "csrc", "include"), "-I", os.path.join(ROOT, "include"),
                           "-L", libdir, "-lpopsift", "-lpopsift_hip", "-Wl,-rpath," + libdir])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300,
                         env=dict(os.environ, POPSIFT_TEST_EXPECT_GPU="1"))
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout
    assert "estimateAffine:" in out.stdout and "estimateSimilarity:" in out.stdout


def _desc_xy(feats, n_desc):
    xy = np.full((n_desc, 2), np.nan, np.float32)
    for s in range(feats["desc_idx"].shape[1]):
        sel = feats["num_ori"] > s
        xy[feats["desc_idx"][sel, s]] = np.stack([feats["xpos"][sel], feats["ypos"][sel]], 1)
    assert not np.isnan(xy).any()
    return xy


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


@pytest.mark.parametrize("model", ac.MODELS)
def test_match_tool_verify(capi, tmp_path, model):
    """popsift-match --pairs FILE --verify-affine / --verify-similarity 1.5 --ransac-refit prints the nine entries (the
    last three 0 0 1) and the inlier count and writes only the inliers; --rematch writes the list guided by the model.
    Descriptor ORDER is not reproducible between runs (so neither are the samples): the rows are compared, as sorted
    distances, with what the restated rule keeps of capi's pairs -- and what capi's guided matcher returns -- under the
    model the tool PRINTED.  The two crops differ by the translation (5, 3), which both models can represent."""
    base = synth(336, 256, 77)
    a, b = np.ascontiguousarray(base[8:248, 8:328]), np.ascontiguousarray(base[5:245, 3:323])     # (x, y) of a is (x + 5, y + 3) in b
    _write_pgm(tmp_path / "l.pgm", a)
    _write_pgm(tmp_path / "r.pgm", b)
    (da, xa), (db, xb) = _extract(capi, a), _extract(capi, b)
    pairs = capi.match_pairs(da, db, 0.8, True)
    pts = ac.correspondences(pairs, xa, xb)
    truth = ac.passes([1, 0, 5, 0, 1, 3, 0, 0, 1], 1.5, pts)
    name = model.capitalize()
    common = [MATCH, "-l", "l.pgm", "-r", "r.pgm", "--octaves", "3", "--norm-multi", "9"]
    verify = ["--mutual", "--verify-" + model, "1.5", "--ransac-hypotheses", "200", "--ransac-seed", "7", "--ransac-refit"]
    fmt = lambda recs: sorted(("%.3f" % x, "%.3f" % y) for x, y in zip(recs["d1"], recs["d2"]))

    def printed(stdout):
        line = [l for l in stdout.splitlines() if l.startswith(name + ":")][0]
        m = np.array([float(v) for v in line.split()[1:]], np.float32)       # %.9g: float32 round trip
        assert m.shape == (9,) and m[6:].tolist() == [0.0, 0.0, 1.0]
        return m

    out = tmp_path / "pairs.txt"
    p = subprocess.run(common + ["--pairs", str(out)] + verify, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    rows = [l.split() for l in out.read_text().splitlines()]
    assert "%s inliers: %d of %d" % (name, len(rows), len(pairs)) in p.stdout and "Number of matches: %d" % len(rows) in p.stdout
    m = printed(p.stdout)
    keep = ac.passes(m, 1.5, pts)
    assert len(rows) == keep.sum() > 50 and sorted((r[4], r[5]) for r in rows) == fmt(pairs[keep])
    print("tool --verify-%s: %d inliers of %d pairs; the true translation admits %d; model %s" % (model, len(rows), len(pairs), truth.sum(), m[:6]))
    assert len(rows) >= 0.9 * truth.sum() > 50
    # a pair that both the model and the true translation admit lies within 1.5 px of each: there the two are within 3 px
    both = pts[keep & truth]
    assert len(both) > 50 and np.hypot(*(ac.transfer(m, both[:, 0:2]) - (both[:, 0:2] + np.float32([5, 3]))).T).max() <= 3.0
    p = subprocess.run(common + ["--pairs", str(out)] + verify + ["--rematch"], cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    rows = [l.split() for l in out.read_text().splitlines()]
    guided = capi.match_pairs_guided(da, xa, db, xb, capi.Guide.homography(printed(p.stdout), 1.5), 0.8, True)
    assert "Number of matches: %d" % len(rows) in p.stdout
    assert sorted((r[4], r[5]) for r in rows) == fmt(guided)
