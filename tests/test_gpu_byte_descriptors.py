"""GPU tests of byte descriptors: the quantisation rule (psx_quantize_desc), the exact integer 2-NN matcher
(psx_match_u8) and byte mode of a context (psx_set_descriptor_format, psx_download_u8, psx_attach_export_u8)."""
import ctypes as C
import time

import numpy as np
import pytest

from popsift_amd.synth import synth

pytestmark = pytest.mark.gpu

INT_MAX = 2 ** 31 - 1


def _oracle_u8(oracle, left, right):
    """oracle.match on the float-cast bytes; distances as integers (INT_MAX where the oracle reports +inf)."""
    mo, do_ = oracle.match(left.astype(np.float32), right.astype(np.float32))
    return mo, _as_int(do_)


def _as_int(d):
    """float distances as int64, +inf -> INT_MAX (what psx_match_u8 reports for a missing neighbour)"""
    d = np.asarray(d, np.float64)
    assert np.all(np.isinf(d) | (d == np.round(d)))                 # exact integers
    return np.where(np.isinf(d), INT_MAX, np.where(np.isinf(d), 0, d)).astype(np.int64)


def _random_u8(rng, n, lo=0, hi=256):
    return rng.integers(lo, hi, size=(n, 128), dtype=np.uint8)


def test_quantize_crafted_values(capi):
    vals = np.array([0.0, 0.49999997, 0.5, 1.5, 2.5, 254.5, 255.49, 255.5, 600.0, -0.0, -0.5, -3.0, 127.5, 0.5000001],
                    np.float32)
    want = np.array([0, 0, 1, 2, 3, 255, 255, 255, 255, 0, 0, 0, 128, 1], np.uint8)
    d = np.zeros((3, 128), np.float32)
    d[0, :len(vals)] = vals
    d[1] = np.linspace(-2.0, 300.0, 128, dtype=np.float32)
    d[2] = np.arange(128, dtype=np.float32) + np.float32(0.5)           # every exact .5: half away from zero
    q = capi.quantize(d)
    assert np.array_equal(q[0, :len(vals)], want)
    assert np.array_equal(q, capi.quantize_rule(d))
    assert np.array_equal(q[2], np.arange(1, 129, dtype=np.uint8))


@pytest.mark.parametrize("nl,nr,seed", [(300, 257, 1), (64, 1000, 2), (1, 1, 3), (5, 0, 4), (129, 1, 5), (0, 7, 6),
                                        (33, 31, 7), (257, 513, 8), (2500, 2300, 9)])
def test_match_u8_equals_oracle(oracle, capi, nl, nr, seed):
    rng = np.random.default_rng(seed)
    left, right = _random_u8(rng, nl), _random_u8(rng, nr)
    if nr > 10 and nl > 3:
        right[7] = left[0]; right[3] = left[0]                  # exact duplicates: ties keep the earlier index
        right[9] = left[2]; right[9, 5] ^= 1
        right[nr - 1] = right[3]                                 # a third copy at the far end (another chunk)
    mo, do_ = _oracle_u8(oracle, left, right)
    mg, dg = capi.match_u8(left, right)
    assert np.array_equal(mo, mg)
    assert np.array_equal(do_, dg.astype(np.int64))
    # the float matcher on the same byte-valued inputs agrees too
    mf, df = capi.match(left.astype(np.float32), right.astype(np.float32))
    assert np.array_equal(mf, mg)
    assert np.array_equal(_as_int(df), dg.astype(np.int64))


def test_match_u8_adversarial(oracle, capi):
    """Equal distances everywhere: constant descriptors, all-0 / all-255, many duplicates, a narrow value range."""
    rng = np.random.default_rng(11)
    right = _random_u8(rng, 1500, 100, 104)                       # few distinct distances: ties everywhere
    right[::7] = 0
    right[3::11] = 255
    right[500:900] = right[100]
    left = np.concatenate([_random_u8(rng, 300, 100, 104), np.zeros((5, 128), np.uint8),
                           np.full((5, 128), 255, np.uint8), right[100:110]])
    mo, do_ = _oracle_u8(oracle, left, right)
    mg, dg = capi.match_u8(left, right)
    assert np.array_equal(mo, mg) and np.array_equal(do_, dg.astype(np.int64))
    # extreme distance: all-0 against all-255 only
    l0, r0 = np.zeros((3, 128), np.uint8), np.full((2, 128), 255, np.uint8)
    mg, dg = capi.match_u8(l0, r0)
    assert np.all(dg == 128 * 255 * 255) and np.all(mg[:, :2] == [0, 1]) and np.all(mg[:, 2] == 0)


def test_match_u8_scratch_grow_shrink_grow(oracle, capi):
    """One thread, calls whose sizes grow, shrink and grow again: the same results as fresh calls."""
    rng = np.random.default_rng(21)
    sets = [(_random_u8(rng, n), _random_u8(rng, m)) for n, m in ((3000, 2900), (40, 70), (1, 600), (4100, 3300))]
    first = [capi.match_u8(l, r) for l, r in sets]
    capi.lib().psx_match_release()
    for (l, r), (m1, d1) in zip(sets, first):
        capi.lib().psx_match_release()
        m2, d2 = capi.match_u8(l, r)
        assert np.array_equal(m1, m2) and np.array_equal(d1, d2)
    mo, do_ = _oracle_u8(oracle, *sets[3])
    assert np.array_equal(first[3][0], mo) and np.array_equal(first[3][1].astype(np.int64), do_)


def _extract(capi, cfg, img, fmt, export=False, float_img=False):
    ctx = capi.Context(cfg)
    ctx.set_descriptor_format(fmt)
    if float_img:
        ctx.upload(img.astype(np.float32) / np.float32(255.0))
    else:
        ctx.upload(img)
    bufs = None
    if export:
        fb = np.zeros(60000 * capi.FEATURE_DTYPE.itemsize, np.uint8)
        db = np.zeros((60000, 128), np.uint8)
        ctx.attach_export_u8(fb, db)
        bufs = (fb, db)
    ctx.extract()
    return ctx, bufs


def test_download_u8_is_rule_of_floats(capi):
    img = synth(640, 480, 5)
    cfg = capi.default_config(octaves=4, sift_mode=2, norm_multi=9, norm_mode=1)
    ctx, _ = _extract(capi, cfg, img, capi.DESCFMT_U8)
    fq, dq = ctx.download_u8()
    ff, df = ctx.download()
    assert len(dq) > 100
    assert np.array_equal(fq.view(np.uint8), ff.view(np.uint8))
    assert np.array_equal(dq, capi.quantize_rule(df))
    assert np.array_equal(dq, capi.quantize(df))
    # the same frame in float mode: the floats are unchanged by byte mode; download_u8 refuses float mode
    ctx2, _ = _extract(capi, cfg, img, capi.DESCFMT_F32)
    f2, d2 = ctx2.download()
    # (record order follows atomic arrival: compare as sets of rows)
    assert len(f2) == len(ff) and len(d2) == len(df)
    assert sorted(map(bytes, d2.view(np.uint32))) == sorted(map(bytes, df.view(np.uint32)))
    with pytest.raises(capi.PopSiftError):
        ctx2.download_u8()
    with pytest.raises(capi.PopSiftError):
        ctx2.set_descriptor_format(2)
    ctx.close(); ctx2.close()


@pytest.mark.parametrize("desc_mode", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("norm", ["rootsift9", "rootsift10", "classic9"])
def test_export_u8_every_desc_mode(capi, desc_mode, norm):
    img = synth(320, 240, 31 + desc_mode)
    kw = dict(octaves=3, desc_mode=desc_mode)
    kw.update({"rootsift9": dict(norm_mode=0, norm_multi=9), "rootsift10": dict(norm_mode=0, norm_multi=10),
               "classic9": dict(norm_mode=1, norm_multi=9)}[norm])
    cfg = capi.default_config(**kw)
    ctx, _ = _extract(capi, cfg, img, capi.DESCFMT_U8, export=True)
    fe, de = ctx.exported()
    de = de.copy()
    ff, df = ctx.download()
    assert len(de) > 20
    assert np.array_equal(fe.view(np.uint8), ff.view(np.uint8))
    assert np.array_equal(de, capi.quantize_rule(df))
    assert de.max() > 100              # the multiplier reached the bytes
    if norm == "rootsift10":
        # RootSift x 1024 (up to 1024): many bins above 255.5, the epilogue's saturation at 255 is exercised (x 512 can reach
        # 512 only for a bin with a quarter of the descriptor's L1 mass, which these images do not produce)
        sat = df > 255.5
        assert sat.sum() > 100 and np.all(de[sat] == 255)
    ctx.close()


@pytest.mark.parametrize("variant", ["float_image", "grid_filter"])
def test_export_and_download_u8_variants(capi, variant):
    img = synth(400, 300, 77)
    if variant == "grid_filter":
        cfg = capi.default_config(octaves=3, filter_max_extrema=150, filter_grid_size=3, grid_filter_mode=1)
    else:
        cfg = capi.default_config(octaves=3, sift_mode=2, norm_mode=1, norm_multi=9)
    ctx, _ = _extract(capi, cfg, img, capi.DESCFMT_U8, export=True, float_img=(variant == "float_image"))
    fe, de = ctx.exported()
    fe, de = fe.copy(), de.copy()
    ff, df = ctx.download()
    assert np.array_equal(de, capi.quantize_rule(df)) and np.array_equal(fe.view(np.uint8), ff.view(np.uint8))
    # a second frame through psx_download_u8 after detaching
    ctx.attach_export_u8(None, None)
    ctx.extract()
    fq, dq = ctx.download_u8()
    ff, df = ctx.download()
    assert np.array_equal(dq, capi.quantize_rule(df)) and np.array_equal(fq.view(np.uint8), ff.view(np.uint8))
    ctx.close()


def test_match_u8_on_quantised_real_descriptors(oracle, capi):
    """Quantised descriptors of two views of a 1080p frame (RootSift, norm_multi 9: the caller profile)."""
    a = synth(1920, 1080, 4243)
    ds = []
    for img in (a, np.roll(a, 3, axis=1)):
        ctx = capi.Context(capi.default_config(octaves=5, sift_mode=2, norm_multi=9))
        ctx.set_descriptor_format(capi.DESCFMT_U8)
        ctx.upload(img)
        ctx.extract()
        ds.append(ctx.download_u8()[1])
        ctx.close()
    assert len(ds[0]) > 4096 and len(ds[1]) > 4096
    mo, do_ = _oracle_u8(oracle, ds[0], ds[1])
    mg, dg = capi.match_u8(ds[0], ds[1])
    assert np.array_equal(mo, mg) and np.array_equal(do_, dg.astype(np.int64))
    assert mg[:, 2].mean() > 0.5


def test_match_u8_18432_equals_oracle_and_float_matcher(oracle, capi):
    """18432 x 18432 against the oracle and against psx_match on the same byte-valued inputs (timings printed only:
    tools/byte_desc_ab.py measures them)."""
    rng = np.random.default_rng(18432)
    left, right = _random_u8(rng, 18432, 0, 64), _random_u8(rng, 18432, 0, 64)
    right[5000:5010] = left[:10]
    mo, do_ = _oracle_u8(oracle, left, right)
    L = capi.lib()
    L.psx_match_u8.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.psx_match.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    bufs = []
    try:
        pl, pr, plf, prf = capi._to_device(L, 0, [left, right, left.astype(np.float32), right.astype(np.float32)], bufs)
        mm = np.zeros((len(left), 3), np.int32)
        dd = np.zeros((len(left), 2), np.int32)
        mf = np.zeros((len(left), 3), np.int32)
        df = np.zeros((len(left), 2), np.float32)
        t_u8, t_f = [], []
        for _ in range(4):
            t0 = time.perf_counter()
            assert L.psx_match_u8(0, pl, len(left), pr, len(right), mm.ctypes.data, dd.ctypes.data) == 0
            t_u8.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            assert L.psx_match(0, plf, len(left), prf, len(right), mf.ctypes.data, df.ctypes.data) == 0
            t_f.append(time.perf_counter() - t0)
    finally:
        for p in bufs:
            L.psx_dev_free(0, p)
    assert np.array_equal(mo, mm) and np.array_equal(do_, dd.astype(np.int64))
    assert np.array_equal(mf, mm) and np.array_equal(_as_int(df), dd.astype(np.int64))
    print("psx_match_u8 %.3f ms, psx_match %.3f ms (best of 4, 18432 x 18432)" % (1e3 * min(t_u8), 1e3 * min(t_f)))
