"""GPU tests of the batched geometric verification (include/popsift_hip.h, "geometric verification", MANY LISTS IN ONE CALL):
psx_ransac_homography_many / psx_ransac_fundamental_many and their _dev forms, FeaturesDev::estimate*Many.  Expected values
come from tests/ransac_many_cases.py -- the single-list restatements of ransac_cases.py / fundamental_cases.py per set --,
from the host references psx_ransac_*_many_ref and from the single-list device calls on the same device arrays in the same
process; models are compared as 32-bit patterns, counts, the result structs and the inlier records exactly."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch        # before the HIP library is loaded: torch brings a HIP runtime of its own and must initialise first (_dev forms)

from tests import fundamental_cases as fc
from tests import ransac_cases as rc
from tests import ransac_many_cases as mc
from tests.ransac_cases import bits, same_records, same_result

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Dev:
    """the position arrays of a case uploaded once: one left array, one right array per set"""

    def __init__(self, capi, c):
        self.L, self.bufs = capi.lib(), []
        arrays = [np.ascontiguousarray(c["left_xy"], np.float32)] + [np.ascontiguousarray(r, np.float32) for r in c["right_xys"]]
        ptrs = capi._to_device(self.L, 0, arrays, self.bufs)
        self.plx, self.nl = ptrs[0], len(c["left_xy"])
        self.prx, self.lens = [p.value for p in ptrs[1:]], [len(r) for r in c["right_xys"]]

    def close(self):
        for p in self.bufs:
            self.L.psx_dev_free(0, p)
        self.bufs = []


def _raw(capi, dev, model, lists, opts, cap, order=None, prx=None, lens=None, layers=True, nl=None):
    """psx_ransac_<model>_many with sentinel-filled outputs: (rc, results, count, out int32 words, models, counts)"""
    order = list(range(len(lists))) if order is None else list(order)
    prx = dev.prx if prx is None else prx
    lens = dev.lens if lens is None else lens
    K, N = len(order), opts.hypotheses
    pairs = mc.concat([lists[k] for k in order], lists[0].dtype if len(lists) else rc.PAIR_DTYPE)
    sc = np.array([len(lists[k]) for k in order], np.int32)
    la = np.array([lens[k] for k in order], np.int32)
    pa = (C.c_void_p * max(K, 1))(*[prx[k] for k in order])
    out = np.full((cap + 2) * 4, -7, np.int32)
    models, counts = np.full((K, N, 9), -7, np.float32), np.full((K, N), -7, np.int32)
    res, cnt = (capi.RansacResult * max(K, 1))(), C.c_int(-77)
    C.memset(res, 0x5a, C.sizeof(res))
    ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None
    rv = getattr(dev.L, "psx_ransac_%s_many" % model)(0, ptr(pairs), ptr(sc), K, dev.plx, dev.nl if nl is None else nl, pa, ptr(la), C.byref(opts), res,
                                                     ptr(out) if cap else None, cap, C.byref(cnt), ptr(models) if layers else None,
                                                     ptr(counts) if layers else None)
    return rv, res, cnt.value, out, models, counts


def _single(capi, dev, model, k, pairs, opts):
    """the single-list device call psx_ransac_<model> for set k on the same device arrays: the dict of capi._ransac_call"""
    name, kind = capi._ransac_names(model)
    fn = lambda *a: getattr(dev.L, name)(0, *a)
    return capi._ransac_call(fn, name, pairs.ctypes.data_as(C.c_void_p) if pairs.size else None, len(pairs), pairs.dtype, dev.plx, dev.nl,
                             C.c_void_p(dev.prx[k]) if dev.prx[k] else None, dev.lens[k], opts, None, True, kind=kind)


def _untouched(res, cnt, out, models, counts):
    return cnt == -77 and np.all(out == -7) and np.all(models == -7) and np.all(counts == -7) and bytes(res) == b"\x5a" * C.sizeof(res)


@pytest.mark.parametrize("refit", [False, True], ids=["sample", "refit"])
@pytest.mark.parametrize("N,seed", mc.CONFIGS, ids=mc.CONFIG_IDS)
@pytest.mark.parametrize("model", mc.MODELS)
def test_host_form_equals_restatement_reference_and_single_calls(capi, model, N, seed, refit):
    c = mc.case(model, seed)
    want = mc.expect(model, N, seed, refit)
    if model == "fundamental" and (N, seed) == (65, 4) and refit:
        mc.premise(want, mc.expect(model, N, seed, False), c["sizes"])
    opts = capi.ransac_opts(mc.TOL, N, seed, refit)
    ref = getattr(capi, "ransac_%s_many_ref" % model)(c["lists"], c["left_xy"], c["right_xys"], opts, layers=True)
    K = len(c["sizes"])
    total_pairs = sum(c["sizes"])
    dev = _Dev(capi, c)
    try:
        rv, res, cnt, out, models, counts = _raw(capi, dev, model, c["lists"], opts, total_pairs)
        assert rv == 0
        cat = mc.concat([w["records"] for w in want])
        total = len(cat)
        assert cnt == total == ref["count"] == sum(res[k].inliers for k in range(K))
        got = out[:4 * total].view(rc.PAIR_DTYPE)
        assert same_records(got, cat) and same_records(got, ref["records"]) and np.all(out[4 * total:] == -7)         # the concatenation, as bytes
        at = 0
        for k, n in enumerate(c["sizes"]):
            w, r = want[k], res[k]
            bad = np.nonzero((bits(models[k]) != bits(w["models"])).any(1))[0]
            assert len(bad) == 0, ("set", k, n, "models differ from the restatement at hypotheses", bad[:5])
            assert np.array_equal(bits(models[k]), bits(ref["models"][k]))
            assert np.array_equal(counts[k], w["counts"]) and np.array_equal(counts[k], ref["counts"][k]), (k, n)
            assert same_result(r, w), (k, n, r.best, r.sample_inliers, r.inliers, r.refit_kept, w["best"], w["sample_inliers"], w["inliers"])
            assert bytes(r) == bytes(ref["results"][k]), (k, n)
            mine = got[at:at + r.inliers]
            assert same_records(mine, w["records"]) and same_records(mine, ref["inliers"][k]), (k, n)
            at += r.inliers
            one = _single(capi, dev, model, k, c["lists"][k], opts)
            assert bytes(r) == bytes(one["result"]) and same_records(mine, one["inliers"]), (k, n)
            if n >= mc.MIN[model]:
                assert np.array_equal(bits(models[k]), bits(one["models"])) and np.array_equal(counts[k], one["counts"]), (k, n)
            else:
                assert r.best == -1 and r.inliers == 0 and not models[k].any() and not counts[k].any(), (k, n)
        # the python wrapper, and its guides
        g = getattr(capi, "ransac_%s_many" % model)(c["lists"], c["left_xy"], c["right_xys"], opts)
        assert g["count"] == total and same_records(g["records"], cat)
        for k in range(K):
            assert same_result(g["results"][k], want[k]) and same_records(g["inliers"][k], want[k]["records"])
            assert g["results"][k].guide(mc.TOL).kind == (capi.GUIDE_EPIPOLAR if model == "fundamental" else capi.GUIDE_HOMOGRAPHY)
    finally:
        dev.close()


@pytest.mark.parametrize("model", mc.MODELS)
def test_dev_form_capacity_and_byte_records(capi, model):
    """the _dev form on torch buffers: capacities total - 1, 0 and full report the total and leave the bytes behind the capacity
    alone; the input list is unchanged; records of the byte matcher's dtype give the same result with the payload carried"""
    N, seed = mc.CONFIGS[1]
    c, cu = mc.case(model, seed), mc.case(model, seed, u8=True)
    K = len(c["sizes"])
    total_pairs = sum(c["sizes"])
    dev = _Dev(capi, c)
    fn = getattr(capi, "ransac_%s_many_dev" % model)
    try:
        for refit in (False, True):
            want = mc.expect(model, N, seed, refit)
            cat = mc.concat([w["records"] for w in want])
            total = len(cat)
            opts = capi.ransac_opts(mc.TOL, N, seed, refit)
            for lists, dtype in ((c["lists"], rc.PAIR_DTYPE), (cu["lists"], rc.PAIR_U8_DTYPE)):
                host = np.ascontiguousarray(mc.concat(lists, dtype)).view(np.uint8).copy()
                src = torch.from_numpy(host).cuda()
                for cap in (total - 1, 0, total_pairs):
                    dbuf = torch.full(((cap + 2) * 16,), 0xA5, dtype=torch.uint8, device="cuda")
                    torch.cuda.synchronize()
                    g = fn(src.data_ptr(), c["sizes"], dev.plx.value, dev.nl, dev.prx, dev.lens, dbuf.data_ptr() if cap else 0, cap, opts, layers=True)
                    back = dbuf.cpu().numpy()
                    k = min(cap, total)
                    assert g["count"] == total and all(same_result(g["results"][i], want[i]) for i in range(K)), (cap, dtype)
                    assert all(np.array_equal(bits(g["models"][i]), bits(want[i]["models"])) and np.array_equal(g["counts"][i], want[i]["counts"])
                               for i in range(K)), cap
                    recs = back[:k * 16].view(dtype)
                    assert np.array_equal(recs["left"], cat["left"][:k]) and np.array_equal(recs["right"], cat["right"][:k]), cap
                    assert np.array_equal(recs["d1"].astype(np.int64), cat["d1"][:k].astype(np.int64))                 # the payload travels
                    assert np.array_equal(recs["d2"].astype(np.int64), cat["d2"][:k].astype(np.int64))
                    assert np.all(back[k * 16:] == 0xA5), cap
                    assert np.array_equal(src.cpu().numpy(), host), cap                                                # the input is only read
    finally:
        dev.close()


def test_set_handling(capi):
    """one set alone equals the single call; a permutation of the sets permutes the results and reorders the slices; the
    same right pointer twice; right arrays as slices of one allocation"""
    model = "fundamental"
    N, seed = mc.CONFIGS[1]
    c = mc.case(model, seed)
    want = mc.expect(model, N, seed, True)
    opts = capi.ransac_opts(mc.TOL, N, seed, True)
    K = len(c["sizes"])
    total_pairs = sum(c["sizes"])
    dev = _Dev(capi, c)
    try:
        def check(order, prx=None, what=""):
            rv, res, cnt, out, models, counts = _raw(capi, dev, model, c["lists"], opts, total_pairs, order=order, prx=prx)
            cat = mc.concat([want[k]["records"] for k in order])
            assert rv == 0 and cnt == len(cat), what
            assert same_records(out[:4 * cnt].view(rc.PAIR_DTYPE), cat) and np.all(out[4 * cnt:] == -7), what
            for i, k in enumerate(order):
                assert same_result(res[i], want[k]), (what, i, k)
                assert np.array_equal(bits(models[i]), bits(want[k]["models"])) and np.array_equal(counts[i], want[k]["counts"]), (what, i, k)
            return res

        for k in (3, 11, 13):                                   # n = 9, 1023, 1025 alone
            res = check([k], what="alone")
            one = _single(capi, dev, model, k, c["lists"][k], opts)
            assert bytes(res[0]) == bytes(one["result"])
        perm = [13, 0, 4, 12, 7, 3, 11, 1, 14, 5, 10, 2, 9, 6, 8]
        assert sorted(perm) == list(range(K))
        check(perm, what="permuted")
        check([12, 12, 5, 12], what="the same set and right pointer more than once")
        # all right arrays in ONE allocation, every set a slice of it (8-byte aligned: whole positions)
        flat = np.concatenate([np.ascontiguousarray(r, np.float32).reshape(-1) for r in c["right_xys"]])
        buf = torch.from_numpy(flat).cuda()
        torch.cuda.synchronize()
        offs = np.concatenate([[0], np.cumsum([2 * len(r) for r in c["right_xys"]])])
        slices = [buf.data_ptr() + 4 * int(offs[k]) if len(c["right_xys"][k]) else None for k in range(K)]
        check(list(range(K)), prx=slices, what="slices of one allocation")
        check(perm, prx=slices, what="slices, permuted")
    finally:
        dev.close()


@pytest.mark.parametrize("model", mc.MODELS)
def test_errors_write_nothing_and_a_good_call_follows(capi, model):
    N, seed = 16, mc.CONFIGS[0][1]
    sizes = (65, 0, 257, 64)
    c = mc.case(model, seed, sizes=sizes)
    K = len(sizes)
    total_pairs = sum(sizes)
    good = capi.ransac_opts(mc.TOL, N, seed, True)
    dev = _Dev(capi, c)
    try:
        def refused(lists=c["lists"], opts=good, cap=total_pairs, **kw):
            rv, res, cnt, out, models, counts = _raw(capi, dev, model, lists, opts, cap, **kw)
            return rv == -1 and _untouched(res, cnt, out, models, counts)

        for o in (capi.RansacOpts(float("nan"), N, 0, 0), capi.RansacOpts(-1.0, N, 0, 0), capi.RansacOpts(float("inf"), N, 0, 0),
                  capi.RansacOpts(2.0, 0, 0, 0), capi.RansacOpts(2.0, 65537, 0, 0), capi.RansacOpts(2.0, N, 0, 4)):
            assert refused(opts=o), (o.tol, o.hypotheses, o.flags)
        assert refused(nl=-1) and refused(nl=0)
        assert refused(lens=[65, 0, -1, 64]) and refused(lens=[65, 0, 0, 64])
        assert refused(prx=[dev.prx[0], None, None, dev.prx[3]])
        # a pair index outside its position array, in the middle set: one flag for the whole call, no record is written
        for field, k, at, value in (("right", 2, 40, sizes[2]), ("left", 2, 3, -2), ("left", 3, 63, total_pairs), ("right", 0, 64, -1)):
            lists = [p.copy() for p in c["lists"]]
            lists[k][field][at] = value
            assert refused(lists=lists), (field, k, at, value)
        # a set shorter than its pairs' indices (the last position of set 2 is referenced by its permutation)
        assert refused(lens=[65, 0, sizes[2] - 1, 64])
        # afterwards a good call succeeds, and equals the reference
        rv, res, cnt, out, models, counts = _raw(capi, dev, model, c["lists"], good, total_pairs)
        ref = getattr(capi, "ransac_%s_many_ref" % model)(c["lists"], c["left_xy"], c["right_xys"], good, layers=True)
        assert rv == 0 and cnt == ref["count"] > 3 * mc.MIN[model] and same_records(out[:4 * cnt].view(rc.PAIR_DTYPE), ref["records"])
        assert all(bytes(res[k]) == bytes(ref["results"][k]) for k in range(K)) and res[1].best == -1
        assert np.array_equal(bits(models), bits(ref["models"])) and np.array_equal(counts, ref["counts"])
    finally:
        dev.close()


def test_alternating_with_the_single_calls_on_one_scratch(capi):
    """many-H, single-F, many-F and single-H share the calling thread's scratch (slots of their own, one stream, one pinned
    buffer): in turn, with and without the refit, across a release of the scratch, each equal to its expectation"""
    N, seed = mc.CONFIGS[0]
    ch, cf = mc.case("homography", seed), mc.case("fundamental", seed)
    fp, flxy, frxy, _ = fc.planted(300, 7, "general")
    hp, hlxy, hrxy, _ = rc.planted(129, 6)
    dh, df = _Dev(capi, ch), _Dev(capi, cf)
    sf, sh = _Dev(capi, dict(left_xy=flxy, right_xys=[frxy])), _Dev(capi, dict(left_xy=hlxy, right_xys=[hrxy]))
    try:
        for round_ in range(2):
            for refit in (True, False):
                om = capi.ransac_opts(mc.TOL, N, seed, refit)
                fo, ho = capi.ransac_opts(fc.TOL, 256, 7, refit), capi.ransac_opts(rc.TOL, 128, 6, refit)
                fw, hw = fc.expect(300, 256, 7, "general", refit), rc.expect(129, 128, 6, refit)
                for model, c, dev in (("homography", ch, dh), ("fundamental", cf, df)):
                    want = mc.expect(model, N, seed, refit)
                    rv, res, cnt, out, models, counts = _raw(capi, dev, model, c["lists"], om, sum(c["sizes"]))
                    cat = mc.concat([w["records"] for w in want])
                    assert rv == 0 and cnt == len(cat) and same_records(out[:4 * cnt].view(rc.PAIR_DTYPE), cat), (model, refit, round_)
                    assert all(same_result(res[k], want[k]) and np.array_equal(counts[k], want[k]["counts"]) for k in range(len(want)))
                    # the other model's single call in between
                    other, sd, p, o, w = (("fundamental", sf, fp, fo, fw) if model == "homography" else ("homography", sh, hp, ho, hw))
                    one = _single(capi, sd, other, 0, p, o)
                    assert same_result(one["result"], w) and same_records(one["inliers"], w["records"]), (other, refit, round_)
                    assert np.array_equal(bits(one["models"]), bits(w["models"])) and np.array_equal(one["counts"], w["counts"])
            assert capi.lib().psx_match_release() == 0
    finally:
        for d in (dh, df, sf, sh):
            d.close()


def test_match_many_then_verify_many_on_the_device(capi):
    """the chain on the device: match_pairs_many_dev -> ransac_fundamental_many_dev directly on its output buffer and its
    set_counts, no download in between, on fundamental_cases.chain_case() descriptors quantised to bytes against three
    right sets (the planted one, its rows reversed, its first 150 rows).  Each set's result equals the restatement on the
    downloaded slice; the returned guides are accepted by match_pairs_guided_u8, whose list holds every inlier."""
    left, right, lxy, rxy, is_planted, perm = fc.chain_case()
    n = len(left)
    lq, rq = capi.quantize_rule(left), capi.quantize_rule(right)
    rights = [rq, np.ascontiguousarray(rq[::-1]), np.ascontiguousarray(rq[:150])]
    rxys = [rxy, np.ascontiguousarray(rxy[::-1]), np.ascontiguousarray(rxy[:150])]
    L = capi.lib()
    bufs = []
    ptrs = capi._to_device(L, 0, [lq, lxy] + rights + rxys, bufs)
    pl, plx, pr, prx = ptrs[0], ptrs[1], ptrs[2:5], ptrs[5:8]
    r_lens = [len(r) for r in rights]
    N, seed = 96, 11
    try:
        d_pairs = torch.full((3 * n * 16,), 0xA5, dtype=torch.uint8, device="cuda")
        d_inl = torch.full((3 * n * 16,), 0xA5, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        set_counts, n1 = capi.match_pairs_many_dev(pl.value, n, [p.value for p in pr], r_lens, d_pairs.data_ptr(), 3 * n, 0.8, True)
        opts = capi.ransac_opts(fc.TOL, N, seed, True)
        g = capi.ransac_fundamental_many_dev(d_pairs.data_ptr(), set_counts, plx.value, n, [p.value for p in prx], r_lens, d_inl.data_ptr(), 3 * n, opts)
        pairs = d_pairs.cpu().numpy()[:n1 * 16].view(capi.PAIR_U8_DTYPE)
        inl = d_inl.cpu().numpy()
        assert n1 == int(np.sum(set_counts)) and all(int(s) >= 100 for s in set_counts[:2]) and int(set_counts[2]) >= 60, set_counts
        lists = capi.split_sets(pairs, set_counts)
        at = 0
        for k in range(3):
            want = fc.ransac(lists[k], lxy, rxys[k], fc.TOL, N, seed, True)
            res = g["results"][k]
            assert fc.same_result(res, want), (k, res.best, res.sample_inliers, res.inliers, want["best"], want["inliers"])
            mine = inl[at * 16:(at + res.inliers) * 16].view(capi.PAIR_U8_DTYPE)
            assert fc.same_records(mine, want["records"]) and res.best >= 0 and res.inliers >= 8, (k, res.inliers)
            at += res.inliers
            guide = res.guide(fc.TOL)
            assert guide.kind == capi.GUIDE_EPIPOLAR
            guided = capi.match_pairs_guided_u8(lq, lxy, rights[k], rxys[k], guide, 0.8, True)
            have = set(zip(guided["left"].tolist(), guided["right"].tolist()))
            assert all((int(a), int(b)) in have for a, b in zip(mine["left"], mine["right"])), k
        assert at == g["count"] and np.all(inl[at * 16:] == 0xA5)
        assert L.psx_match_release() == 0
    finally:
        for p in bufs:
            L.psx_dev_free(0, p)


def test_cpp_estimate_many_on_the_gpu(tmp_path):
    """tests/cpp/test_ransac_many_api.cpp with POPSIFT_TEST_EXPECT_GPU: estimateHomographyMany / estimateFundamentalMany equal the
    C-ABI on the same objects and the loop of the single estimates; a size mismatch and invalid options throw"""
    libdir = os.path.join(ROOT, "popsift_amd", "lib")
    exe = str(tmp_path / "test_ransac_many_api")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-pthread", os.path.join(ROOT, "tests", "cpp", "test_ransac_many_api.cpp"), "-o", exe,
                           "-I", os.path.join(ROOT, "popsift_amd", "csrc", "include"), "-I", os.path.join(ROOT, "include"),
                           "-L", libdir, "-lpopsift", "-lpopsift_hip", "-Wl,-rpath," + libdir])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300,
                         env=dict(os.environ, POPSIFT_TEST_EXPECT_GPU="1"))
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout
    assert "estimateHomographyMany:" in out.stdout and "estimateFundamentalMany:" in out.stdout
