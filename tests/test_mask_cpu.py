"""CPU tests of the detection mask (include/popsift_hip.h, "detection mask"): the rule on the host (psx_mask_keep -- the
function the extrema kernels share through csrc/hip/mask_rule.h) against a numpy float32 restatement, on random
positions, on the corners of the rounding and the clamp, and on the CPU oracle's features of five configurations; the
argument errors; the declarations and bindings; the flat C binding's NULL handling; the C++ overloads.

One corner is stated here as the rule gives it, not as one might expect: x = 0.49999997 (the float32 below 0.5) lands
on pixel 1, not 0.  The rule adds 0.5f in float32, and 0.49999997f + 0.5f is a tie that rounds to 1.0f; the restatement
floor(float32(x) + float32(0.5)) says the same, and the device evaluates exactly this expression."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from popsift_amd.synth import synth
from tests.mask_cases import CONFIGS, CONFIG_IDS, MASKS, assert_premise, make_mask, pixel, restate_keep

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mask_keep_equals_the_restatement_on_random_positions(capi):
    w, h = 173, 97
    rng = np.random.default_rng(21)
    mask = rng.integers(0, 3, (h, w), dtype=np.uint8)
    n = 100000
    x = rng.uniform(-4, w + 4, n).astype(np.float32)
    y = rng.uniform(-4, h + 4, n).astype(np.float32)
    # a share of the positions on and next to the half-pixel boundaries, where the rounding decides
    k = n // 4
    x[:k] = np.nextafter(np.floor(x[:k]) + np.float32(0.5), rng.choice([-np.inf, np.inf], k).astype(np.float32))
    y[k:2 * k] = np.floor(y[k:2 * k]) + np.float32(0.5)
    got = capi.mask_keep(mask, x, y)
    want = restate_keep(mask, x, y)
    assert got.dtype == bool and np.array_equal(got, want)
    assert want.sum() > 10000 and (~want).sum() > 10000
    # a bool mask is taken as it is
    assert np.array_equal(capi.mask_keep(mask != 0, x, y), want)


def test_mask_keep_corners(capi):
    """The clamp (w - 0.5 and w + 3 land on w - 1, negative positions on 0) and the rounding (0.5 lands on pixel 1, and
    so does the float32 just below it -- module docstring), for x and for y; NaN lands on 0, +inf on the last pixel."""
    w, h = 9, 7
    f32 = np.float32
    below_half = np.nextafter(f32(0.5), f32(0))
    assert float(below_half) == float(f32(0.49999997))
    cases = [(f32(w - 0.5), w - 1), (f32(w + 3), w - 1), (below_half, 1), (f32(0.5), 1), (f32(0.49), 0), (f32(-0.5), 0), (f32(-7), 0),
             (f32(1.5), 2), (np.nextafter(f32(1.5), f32(0)), 1), (f32(w - 1), w - 1), (f32(np.nan), 0), (f32(np.inf), w - 1), (f32(-np.inf), 0)]
    for axis, n in (("x", w), ("y", h)):
        for v, want_px in cases:
            want_px = min(want_px, n - 1) if want_px >= w - 1 else want_px
            assert int(pixel(v, n)) == want_px, (axis, v)
            # a mask with exactly that one row / column set: kept iff the position lands on it
            for px in range(n):
                mask = np.zeros((h, w), np.uint8)
                if axis == "x":
                    mask[:, px] = 1
                    got = capi.mask_keep(mask, [v], [f32(3)])
                else:
                    mask[px, :] = 1
                    got = capi.mask_keep(mask, [f32(3)], [v])
                assert bool(got[0]) == (px == want_px), (axis, float(v), px, want_px)


_ORACLE = {}


def oracle_features(oracle, i):
    if i not in _ORACLE:
        kw, size, seed = CONFIGS[i]
        ref = oracle.run(oracle.default_config(**kw), synth(size[0], size[1], seed))
        _ORACLE[i] = ref.features()
    return _ORACLE[i]


@pytest.mark.parametrize("i", range(len(CONFIGS)), ids=CONFIG_IDS)
def test_oracle_features_filtered_by_both(capi, oracle, i):
    """The oracle's features, filtered with mask_keep and with the restatement, select the same rows; every mask keeps
    more than 300 and rejects more than 300 of them (the premise of the GPU tests; mask_cases.assert_premise says where
    blocks16 cannot and what holds there instead)."""
    kw, (w, h), seed = CONFIGS[i]
    F = oracle_features(oracle, i)
    for name in MASKS:
        mask = make_mask(name, w, h)
        got = capi.mask_keep(mask, F["xpos"], F["ypos"])
        want = restate_keep(mask, F["xpos"], F["ypos"])
        print("%s %s: keeps %d of %d" % (CONFIG_IDS[i], name, int(want.sum()), len(F)))
        assert np.array_equal(got, want), name
        assert_premise(name, int(want.sum()), len(F), CONFIG_IDS[i])
    assert capi.mask_keep(make_mask("ones", w, h), F["xpos"], F["ypos"]).all()
    assert not capi.mask_keep(make_mask("zeros", w, h), F["xpos"], F["ypos"]).any()


def test_mask_keep_argument_errors(capi):
    L = capi.lib()
    m = np.ones((4, 5), np.uint8)
    x = np.zeros(3, np.float32)
    k = np.zeros(3, np.uint8)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.psx_mask_keep(vp(m), 5, 4, vp(x), vp(x), 3, vp(k)) == 0 and k.all()
    assert L.psx_mask_keep(None, 5, 4, vp(x), vp(x), 3, vp(k)) == -1
    assert L.psx_mask_keep(vp(m), 0, 4, vp(x), vp(x), 3, vp(k)) == -1
    assert L.psx_mask_keep(vp(m), 5, -1, vp(x), vp(x), 3, vp(k)) == -1
    assert L.psx_mask_keep(vp(m), 5, 4, vp(x), vp(x), -1, vp(k)) == -1
    assert L.psx_mask_keep(vp(m), 5, 4, None, vp(x), 3, vp(k)) == -1
    assert L.psx_mask_keep(vp(m), 5, 4, vp(x), None, 3, vp(k)) == -1
    assert L.psx_mask_keep(vp(m), 5, 4, vp(x), vp(x), 3, None) == -1
    assert L.psx_mask_keep(vp(m), 5, 4, None, None, 0, None) == 0           # nothing to do
    with pytest.raises(TypeError):
        capi.mask_keep(np.ones((4, 5), np.float32), x, x)
    with pytest.raises(TypeError):
        capi.mask_keep(np.ones(20, np.uint8), x, x)
    with pytest.raises(ValueError):
        capi.mask_keep(m, x, x[:2])
    # the context entry points refuse a NULL context
    assert L.psx_set_mask(None, vp(m), 5, 4) == -1 and L.psx_set_mask_dev(None, vp(m), 5, 4) == -1


def test_entry_points_declared_and_bound(capi):
    hdr = open(os.path.join(ROOT, "include", "popsift_hip.h")).read()
    for sym in ("psx_set_mask", "psx_set_mask_dev", "psx_mask_keep"):
        assert "int %s(" % sym in hdr and sym in capi.SYMBOLS and hasattr(capi.lib(), sym), sym
    chdr = open(os.path.join(ROOT, "include", "popsift_c.h")).read()
    for sym in ("popsift_c_enqueue_u8_mask", "popsift_c_enqueue_f32_mask"):
        assert "popsift_c_job* %s(" % sym in chdr and sym in capi.HOST_SYMBOLS and hasattr(capi.host_lib(), sym), sym
    for name in ("set_mask", "set_mask_tensor"):
        assert callable(getattr(capi.Context, name))
    assert "mask" in capi.PopSift.enqueue.__code__.co_varnames
    # host and device share one header, and the kernel's last test calls its function
    hip = os.path.join(ROOT, "popsift_amd", "csrc", "hip")
    assert "psx_mask_allows" in open(os.path.join(hip, "mask_rule.h")).read()
    assert "psx_mask_allows" in open(os.path.join(hip, "extrema.hip")).read()
    assert "psx_mask_allows" in open(os.path.join(hip, "api.hip")).read()


def test_c_binding_null_handle(capi):
    H = capi.host_lib()
    img = np.zeros((8, 8), np.uint8)
    fimg = np.zeros((8, 8), np.float32)
    m = np.ones((8, 8), np.uint8)
    assert not H.popsift_c_enqueue_u8_mask(None, 8, 8, img.ctypes.data, m.ctypes.data, 8, 8)
    assert not H.popsift_c_enqueue_f32_mask(None, 8, 8, fimg.ctypes.data, m.ctypes.data, 8, 8)
    assert b"NULL handle" in H.popsift_c_last_error()


def test_popsift_enqueue_refuses_a_mask_of_another_size(capi):
    """capi.PopSift.enqueue(img, mask=...): refused at enqueue, before a device is touched, with both sizes named"""
    ps = capi.PopSift(capi.default_config(octaves=3))
    img = np.zeros((48, 64), np.uint8)
    with pytest.raises(capi.PopSiftError) as e:
        ps.enqueue(img, mask=np.ones((48, 63), np.uint8))
    assert "63 x 48" in str(e.value) and "64 x 48" in str(e.value)
    with pytest.raises(ValueError):
        ps.enqueue(img, keypoints=np.zeros(0, capi.KEYPOINT_DTYPE), mask=np.ones((48, 64), np.uint8))
    with pytest.raises(TypeError):
        ps.enqueue(img, mask=np.ones((48, 64), np.float32))
    ps.close()


def test_cpp_mask_overloads(tmp_path):
    """tests/cpp/test_mask_api.cpp against libpopsift.so, built and run the way test_keypoints_api.cpp is: the overloads
    compile and are unambiguous, the job owns a copy of the plane, a mask of another size is refused before a device is
    touched, every job is fulfilled."""
    libdir = os.path.join(ROOT, "popsift_amd", "lib")
    if not os.path.exists(os.path.join(libdir, "libpopsift.so")):
        from popsift_amd import build
        build.build_all()
    exe = str(tmp_path / "test_mask_api")
    cmd = ["g++", "-std=c++14", "-O1", "-pthread", os.path.join(ROOT, "tests", "cpp", "test_mask_api.cpp"), "-o", exe,
           "-I", os.path.join(ROOT, "popsift_amd", "csrc", "include"), "-I", os.path.join(ROOT, "include"),
           "-L", libdir, "-lpopsift", "-lpopsift_hip", "-Wl,-rpath," + libdir]
    subprocess.check_call(cmd)
    env = {k: v for k, v in os.environ.items() if k != "POPSIFT_TEST_EXPECT_GPU"}
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120, env=env)
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout
