"""CPU tests of byte descriptors: the C-ABI surface (symbols, argument checks that come before any device is touched),
the host statement of the quantisation rule, and the exactness argument of the integer matcher (psx_match_u8): on
byte-valued inputs the reference's float matcher (the oracle's osift_match) equals an int64 brute-force top-2 in the
(squared distance, index) order."""
import ctypes as C
import re
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["psx_set_descriptor_format", "psx_download_u8", "psx_attach_export_u8", "psx_attach_export_mapped_u8",
       "psx_quantize_desc", "psx_match_u8"]


def test_new_symbols_declared_exported_and_listed(capi):
    hdr = open(os.path.join(ROOT, "include", "popsift_hip.h")).read()
    declared = set(re.findall(r"\b(psx_[a-z0-9_]+)\s*\(", hdr))
    L = capi.lib()
    for s in NEW:
        assert s in declared and s in capi.SYMBOLS and hasattr(L, s), s
    assert "#define PSX_DESCFMT_F32 0" in hdr and "#define PSX_DESCFMT_U8  1" in hdr
    assert capi.DESCFMT_F32 == 0 and capi.DESCFMT_U8 == 1


def test_invalid_arguments_refused_before_any_device(capi):
    L = capi.lib()
    L.psx_set_descriptor_format.argtypes = [C.c_void_p, C.c_int]
    for fmt in (-1, 2, 7):
        assert L.psx_set_descriptor_format(None, fmt) == -1
    assert L.psx_set_descriptor_format(None, 1) == -1             # no context
    L.psx_download_u8.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    assert L.psx_download_u8(None, None, 0, None, 0) == -1
    L.psx_attach_export_u8.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    assert L.psx_attach_export_u8(None, None, 0, None, 0) == -1
    L.psx_quantize_desc.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    assert L.psx_quantize_desc(0, None, -1, None) == -1
    assert L.psx_quantize_desc(0, None, 3, None) == -1
    assert L.psx_quantize_desc(0, None, 0, None) == 0              # nothing to do
    L.psx_match_u8.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    assert L.psx_match_u8(0, None, -1, None, 0, None, None) == -1
    assert L.psx_match_u8(0, None, 4, None, 4, None, None) == -1
    assert L.psx_match_u8(0, None, 0, None, 0, None, None) == 0    # l_len 0: as psx_match
    # r_len 0: what psx_match returns (no neighbour, indices 0, rejected) without a device
    mm = np.full((3, 3), 9, np.int32)
    dd = np.zeros((3, 2), np.int32)
    assert L.psx_match_u8(0, C.c_void_p(16), 3, None, 0, mm.ctypes.data, dd.ctypes.data) == 0
    assert np.all(mm == 0) and np.all(dd == 2 ** 31 - 1)


def test_quantize_rule_on_the_host(capi):
    d = np.array([0.0, 0.49999997, 0.5, 1.5, 2.5, 254.5, 255.49, 255.5, 600.0, -0.0, -0.5, -7.0, np.nan, 511.9],
                 np.float32)
    want = np.array([0, 0, 1, 2, 3, 255, 255, 255, 255, 0, 0, 0, 0, 255], np.uint8)
    assert np.array_equal(capi.quantize_rule(d), want)
    # roundf, not rint: every exact .5 goes up
    h = np.arange(255, dtype=np.float32) + np.float32(0.5)
    assert np.array_equal(capi.quantize_rule(h), np.arange(1, 256).astype(np.uint8))
    assert not np.array_equal(np.rint(h).astype(np.uint8), capi.quantize_rule(h))


def _int_top2(left, right):
    """int64 brute force: the two smallest (squared distance, index) per left row; missing -> (inf, 0) as the reference"""
    l = left.astype(np.int64)
    r = right.astype(np.int64)
    d = (l * l).sum(1)[:, None] + (r * r).sum(1)[None, :] - 2 * l @ r.T
    n = len(left)
    mm = np.zeros((n, 3), np.int32)
    dd = np.full((n, 2), np.inf)
    if len(right) == 0:
        return mm, dd
    order = np.lexsort((np.broadcast_to(np.arange(len(right)), d.shape), d), axis=1)
    mm[:, 0] = order[:, 0]
    dd[:, 0] = d[np.arange(n), order[:, 0]]
    if len(right) > 1:
        mm[:, 1] = order[:, 1]
        dd[:, 1] = d[np.arange(n), order[:, 1]]
    with np.errstate(invalid="ignore", divide="ignore"):
        mm[:, 2] = (dd[:, 0].astype(np.float32) / dd[:, 1].astype(np.float32) < np.float32(0.8))
    return mm, dd


@pytest.mark.parametrize("case", ["random", "narrow", "duplicates", "extremes", "tiny"])
def test_reference_float_matcher_is_exact_on_bytes(oracle, case):
    rng = np.random.default_rng(["random", "narrow", "duplicates", "extremes", "tiny"].index(case) + 101)
    if case == "random":
        left = rng.integers(0, 256, (200, 128), dtype=np.uint8); right = rng.integers(0, 256, (300, 128), dtype=np.uint8)
    elif case == "narrow":                 # few distinct distances: ties everywhere
        left = rng.integers(10, 12, (150, 128), dtype=np.uint8); right = rng.integers(10, 12, (400, 128), dtype=np.uint8)
    elif case == "duplicates":
        left = rng.integers(0, 256, (60, 128), dtype=np.uint8); right = rng.integers(0, 256, (250, 128), dtype=np.uint8)
        right[10:40] = left[5]; right[200] = left[5]; right[3] = left[7]; right[100] = left[7]
    elif case == "extremes":               # all-0 and all-255 rows: the largest distance 128 * 255^2
        left = np.concatenate([np.zeros((4, 128), np.uint8), np.full((4, 128), 255, np.uint8)])
        right = np.concatenate([np.full((3, 128), 255, np.uint8), np.zeros((2, 128), np.uint8), np.full((3, 128), 255, np.uint8)])
    else:
        left = rng.integers(0, 256, (5, 128), dtype=np.uint8); right = rng.integers(0, 256, (1, 128), dtype=np.uint8)
    mo, do_ = oracle.match(left.astype(np.float32), right.astype(np.float32))
    mi, di = _int_top2(left, right)
    assert np.array_equal(mo, mi)
    assert np.array_equal(do_.astype(np.float64), di)
    assert 128 * 255 * 255 < 2 ** 23                              # 9 index bits remain in a 32-bit key


def _host_libs():
    import subprocess
    libdir = os.path.join(ROOT, "popsift_amd", "lib")
    if not os.path.exists(os.path.join(libdir, "libpopsift.so")):
        subprocess.check_call([__import__("sys").executable, "-m", "popsift_amd.build"], cwd=ROOT)
    return libdir


def test_cpp_config_and_byte_mode_without_gpu(tmp_path):
    """tests/cpp/test_byte_descriptors.cpp against libpopsift.so: DescriptorFormat default and setter, no byte view on a
    float FeaturesHost, Feature::print with a null descriptor, and a byte-mode PopSift that fails loudly without a GPU."""
    import subprocess
    libdir = _host_libs()
    exe = str(tmp_path / "test_byte_descriptors")
    cmd = ["g++", "-std=c++14", "-O1", "-pthread", os.path.join(ROOT, "tests", "cpp", "test_byte_descriptors.cpp"), "-o", exe,
           "-I", os.path.join(ROOT, "popsift_amd", "csrc", "include"), "-I", os.path.join(ROOT, "include"),
           "-L", libdir, "-lpopsift", "-lpopsift_hip", "-Wl,-rpath," + libdir]
    subprocess.check_call(cmd)
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout


def test_flat_c_byte_entries(capi):
    H = capi.host_lib()
    for s in ("popsift_c_create_fmt", "popsift_c_descriptor_format", "popsift_c_copy_u8", "popsift_c_descriptor_bytes"):
        assert s in capi.HOST_SYMBOLS and hasattr(H, s), s
    hdr = open(os.path.join(ROOT, "include", "popsift_c.h")).read()
    declared = set(re.findall(r"\b(popsift_c_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(capi.HOST_SYMBOLS)
    # an invalid format is refused before a PopSift (and a device) exists
    cfg = capi.default_config()
    for fmt in (-1, 2, 9):
        assert not H.popsift_c_create_fmt(C.byref(cfg), 0, 0, fmt)
        assert b"descriptor format" in H.popsift_c_last_error()
    # NULL results
    assert H.popsift_c_descriptor_format(None) == -1 and H.popsift_c_copy_u8(None, None, None) == -1
    assert H.popsift_c_descriptor_bytes(None) is None
