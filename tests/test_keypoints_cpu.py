"""CPU tests of caller-supplied keypoints (include/popsift_hip.h, "caller-supplied keypoints"): the record layout, the
bounds table, the placement and acceptance rule on the host (psx_place_keypoints -- the function the device kernel
shares through csrc/hip/kp_place.h) against a numpy restatement that reads the table and only compares, every rejection
rule, the round trip detector -> image-unit records -> automatic placement on the CPU oracle, and the C++ overloads."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from popsift_amd.synth import synth
from tests.rule_edge_cases import boundary_records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the four configurations of the round trip (keyword arguments of default_config, image size, synth seed)
ROUND_TRIP = [
    (dict(), (640, 480), 3),
    (dict(sift_mode=2), (640, 480), 5),
    (dict(upscale_factor=0.0, levels=4, sigma=1.4), (480, 360), 8),
    (dict(sift_mode=1, upscale_factor=-1.0), (800, 600), 2),
]


def octave_dims(cfg, w, h, num_octaves):
    """psx_resize's octave sizes: ceil(w * 2^up), then ceil halves"""
    scale = 2.0 ** cfg.upscale_factor
    ow, oh = int(math.ceil(w * scale)), int(math.ceil(h * scale))
    dims = []
    for _ in range(num_octaves):
        dims.append((ow, oh))
        ow, oh = int(math.ceil(ow / 2.0)), int(math.ceil(oh / 2.0))
    return dims


def restate(capi, cfg, w, h, kps, num_octaves):
    """The rule of INTEGRATION.md in numpy float32: the bounds come from psx_keypoint_bounds, the code only compares."""
    f32 = np.float32
    b = capi.keypoint_bounds(cfg)
    levels = len(b) - 1
    L = levels + 3
    up = int(cfg.upscale_factor)
    dims = octave_dims(cfg, w, h, num_octaves)
    smin = f32(cfg.sigma)
    smax = f32(np.float64(f32(cfg.sigma)) * 2.0 ** ((L - 1) / levels))
    octave = np.full(len(kps), -1, np.int32)
    lpos = np.full(len(kps), -1, np.int32)
    for i, k in enumerate(kps):
        x, y, sg = f32(k["xpos"]), f32(k["ypos"]), f32(k["sigma"])
        if not (np.isfinite(x) and np.isfinite(y) and np.isfinite(sg)) or not sg > 0:
            continue
        n = int(k["num_ori"])
        if n < 0 or n > 4 or not np.isfinite(k["orientation"][:n]).all():
            continue
        if k["octave"] == capi.KP_AUTO:
            s, o = f32(sg * f32(2.0 ** up)), 0
            while o < num_octaves - 1 and s >= b[levels]:
                s, o = f32(s * f32(0.5)), o + 1
            lp = 0 if s < b[0] else 1 + int((b[1:levels] <= s).sum())
        else:
            o, lp = int(k["octave"]), int(k["lpos"])
            if o < 0 or o >= num_octaves:
                continue
        if lp < 0 or lp > L - 1:
            continue
        unit = f32(2.0 ** (o - up))
        with np.errstate(over="ignore"):
            xo, yo, so = f32(x / unit), f32(y / unit), f32(sg / unit)
        if xo < 0 or xo > f32(dims[o][0]) - f32(1) or yo < 0 or yo > f32(dims[o][1]) - f32(1):
            continue
        if so < smin or so > smax:
            continue
        octave[i], lpos[i] = o, lp
    return octave, lpos


def test_record_layout(capi):
    assert C.sizeof(capi.Keypoint) == 40 and capi.KEYPOINT_DTYPE.itemsize == 40
    assert [n for n, _ in capi.Keypoint._fields_] == list(capi.KEYPOINT_DTYPE.names)
    for (name, _), off in zip(capi.Keypoint._fields_, (0, 4, 8, 12, 16, 20, 24)):
        assert getattr(capi.Keypoint, name).offset == off == capi.KEYPOINT_DTYPE.fields[name][1]
    hdr = open(os.path.join(ROOT, "include", "popsift_hip.h")).read()
    assert "#define PSX_KP_AUTO (-1)" in hdr and "#define PSX_DESCRIBE_REUSE_PYRAMID 1" in hdr
    assert capi.KP_AUTO == -1 and capi.DESCRIBE_REUSE_PYRAMID == 1
    k = capi.Keypoint(1.5, 2.5, 3.0, capi.KP_AUTO, 0, 1, (C.c_float * 4)(0.25, 0, 0, 0))
    a = capi.keypoints_array([k])
    assert a.dtype == capi.KEYPOINT_DTYPE and a[0]["sigma"] == 3.0 and a[0]["orientation"][0] == 0.25
    assert len(capi.keypoints_array(None)) == 0


@pytest.mark.parametrize("kw", [dict(), dict(levels=4, sigma=1.4), dict(levels=2, sigma=2.0), dict(levels=5, sigma=1.2)])
def test_bounds_table(capi, kw):
    """b_l = (float)(sigma * 2^((l + 0.5) / levels)), double arithmetic rounded once; [b_0, b_levels) is a factor of 2."""
    cfg = capi.default_config(**kw)
    b = capi.keypoint_bounds(cfg)
    assert b.dtype == np.float32 and len(b) == cfg.levels + 1
    want = [np.float32(float(np.float32(cfg.sigma)) * 2.0 ** ((l + 0.5) / cfg.levels)) for l in range(cfg.levels + 1)]
    assert np.array_equal(b, np.array(want, np.float32))
    assert (np.diff(b) > 0).all() and abs(float(b[-1]) / float(b[0]) - 2.0) < 1e-6
    small = (C.c_float * 2)()
    assert capi.lib().psx_keypoint_bounds(C.byref(cfg), small, 2, None) == -1           # capacity too small


@pytest.mark.parametrize("kw,size", [(dict(octaves=5), (640, 480)), (dict(octaves=4, upscale_factor=0.0, levels=4, sigma=1.4), (480, 360)),
                                     (dict(octaves=3, upscale_factor=-1.0, levels=2), (801, 603)), (dict(octaves=1), (97, 61))])
def test_placement_equals_the_restatement(capi, kw, size):
    """Automatic and explicit placement on seeded random records whose sigmas include, for every octave, every bound
    itself and its two float neighbours (and the two ends of the accepted sigma range with theirs)."""
    w, h = size
    cfg = capi.default_config(**kw)
    kps, explicit = boundary_records(capi, cfg, w, h)                    # tests/rule_edge_cases.py: the GPU tests use them too
    for recs in (kps, explicit):
        o_lib, l_lib = capi.place_keypoints(cfg, w, h, recs)
        o_np, l_np = restate(capi, cfg, w, h, recs, cfg.octaves)
        assert np.array_equal(o_lib, o_np) and np.array_equal(l_lib, l_np)
        assert (o_lib >= 0).sum() > 100 and (o_lib < 0).sum() > 50      # both outcomes are exercised
        assert (l_lib[o_lib < 0] == -1).all()


def test_every_rejection_rule(capi):
    cfg = capi.default_config(octaves=4)
    w, h = 320, 240
    L = cfg.levels + 3
    base = np.zeros(1, capi.KEYPOINT_DTYPE)
    base["xpos"], base["ypos"], base["sigma"], base["octave"] = 100.0, 80.0, 3.0, capi.KP_AUTO

    def placed(**kw):
        k = base.copy()
        for name, v in kw.items():
            k[name] = v
        o, l = capi.place_keypoints(cfg, w, h, k)
        return int(o[0]), int(l[0])

    assert placed() == (1, 3)                              # s = 6 -> 3.0 in octave 1; b_2 = 2.851 <= 3.0 < b_3 = 3.592
    assert placed(octave=2, lpos=1, sigma=4.0) == (2, 1)   # explicit placement is taken as given (sigma 2.0 in octave 2)
    assert placed(octave=2, lpos=1)[0] == -1               # ... and held to the sigma range: 3.0 / 2 = 1.5 < sigma0
    for bad in (np.nan, np.inf, -np.inf):
        assert placed(xpos=bad)[0] == -1 and placed(ypos=bad)[0] == -1 and placed(sigma=bad)[0] == -1
    assert placed(sigma=0.0)[0] == -1 and placed(sigma=-2.0)[0] == -1
    assert placed(octave=4, lpos=1)[0] == -1 and placed(octave=-2, lpos=1)[0] == -1 and placed(octave=19, lpos=1)[0] == -1
    assert placed(octave=1, lpos=-1)[0] == -1 and placed(octave=1, lpos=L)[0] == -1
    assert placed(octave=1, lpos=L - 1) == (1, L - 1) and placed(octave=1, lpos=0) == (1, 0)
    # position: octave 1 is the image itself here (upscale 1), [0, 319] x [0, 239]
    assert placed(xpos=-0.001)[0] == -1 and placed(xpos=319.001)[0] == -1 and placed(ypos=239.5)[0] == -1
    assert placed(xpos=0.0)[0] == 1 and placed(xpos=319.0)[0] == 1 and placed(ypos=239.0)[0] == 1
    # octave 3 is 80 x 60 in octave units = 4 image pixels per texel: x up to 79 * 4
    assert placed(octave=3, lpos=1, sigma=8.0, xpos=316.0)[0] == 3 and placed(octave=3, lpos=1, sigma=8.0, xpos=316.5)[0] == -1
    # sigma range in octave units: [1.6, 1.6 * 2^(5/3) = 5.0797]
    assert placed(octave=1, lpos=1, sigma=1.59)[0] == -1 and placed(octave=1, lpos=1, sigma=1.6)[0] == 1
    assert placed(octave=1, lpos=1, sigma=5.07)[0] == 1 and placed(octave=1, lpos=1, sigma=5.09)[0] == -1
    assert placed(sigma=0.5)[0] == -1                       # automatic: below the first octave's range
    assert placed(sigma=60.0)[0] == -1                      # automatic: above the last octave's range
    assert placed(num_ori=-1)[0] == -1 and placed(num_ori=5)[0] == -1 and placed(num_ori=4)[0] == 1
    ori = np.zeros(4, np.float32)
    ori[1] = np.nan
    assert placed(num_ori=2, orientation=ori)[0] == -1      # a GIVEN orientation that is not finite
    assert placed(num_ori=1, orientation=ori)[0] == 1       # entries beyond num_ori are not looked at
    # argument errors
    one = np.zeros(1, np.int32)
    L_ = capi.lib()
    assert L_.psx_place_keypoints(C.byref(cfg), 0, 10, base.ctypes.data, 1, one.ctypes.data, one.ctypes.data) == -1
    assert L_.psx_place_keypoints(C.byref(cfg), 10, 10, None, 1, one.ctypes.data, one.ctypes.data) == -1
    assert L_.psx_place_keypoints(C.byref(cfg), 10, 10, None, 0, None, None) == 0


@pytest.mark.parametrize("kw,size,seed", ROUND_TRIP)
def test_round_trip_with_the_detector(capi, oracle, kw, size, seed):
    """Detector keypoints of the CPU oracle, as image-unit records with PSX_KP_AUTO: every keypoint of level 1 .. levels
    lands at the detector's own (octave, lpos) -- zero exceptions; the others (level 0 or levels + 1) are accepted too,
    in a neighbouring octave or their own."""
    w, h = size
    img = synth(w, h, seed)
    ref = oracle.run(oracle.default_config(**kw), img)
    cfg = capi.default_config(**kw)
    ext, feat = ref.extrema(), ref.features()
    assert len(ext) == len(feat) > 500
    kps = np.zeros(len(feat), capi.KEYPOINT_DTYPE)
    for name in ("xpos", "ypos", "sigma"):
        kps[name] = feat[name]
    kps["octave"] = capi.KP_AUTO
    octave, lpos = capi.place_keypoints(cfg, w, h, kps)
    assert octave_dims(cfg, w, h, ref.num_octaves) == ref.dims           # the host rule sees the oracle's pyramid
    inner = (ext["lpos"] >= 1) & (ext["lpos"] <= cfg.levels)
    wrong = inner & ((octave != ext["octave"]) | (lpos != ext["lpos"]))
    print("%s: %d misplaced of %d (%d more at level 0 or levels + 1)" % (kw, int(wrong.sum()), int(inner.sum()), int((~inner).sum())))
    assert inner.sum() > 500 and wrong.sum() == 0, np.flatnonzero(wrong)[:10]
    # units: mapping the records back to octave units reproduces the detector's extrema bit for bit
    unit = np.exp2(ext["octave"].astype(np.float64) - int(cfg.upscale_factor)).astype(np.float32)
    for name in ("xpos", "ypos", "sigma"):
        assert np.array_equal((feat[name] / unit).view(np.uint32), ext[name].view(np.uint32)), name
    # explicit records from the detector's own (octave, lpos): all accepted as given
    kps["octave"], kps["lpos"] = ext["octave"], ext["lpos"]
    octave, lpos = capi.place_keypoints(cfg, w, h, kps)
    assert np.array_equal(octave, ext["octave"]) and np.array_equal(lpos, ext["lpos"])


def test_cpp_keypoint_overloads(tmp_path):
    """tests/cpp/test_keypoints_api.cpp against libpopsift.so, built and run the way test_host_api.cpp is: the
    overloads compile, the job owns a copy of the list, the image-mode check holds, every job is fulfilled."""
    libdir = os.path.join(ROOT, "popsift_amd", "lib")
    if not os.path.exists(os.path.join(libdir, "libpopsift.so")):
        from popsift_amd import build
        build.build_all()
    exe = str(tmp_path / "test_keypoints_api")
    cmd = ["g++", "-std=c++14", "-O1", "-pthread", os.path.join(ROOT, "tests", "cpp", "test_keypoints_api.cpp"), "-o", exe,
           "-I", os.path.join(ROOT, "popsift_amd", "csrc", "include"), "-I", os.path.join(ROOT, "include"),
           "-L", libdir, "-lpopsift", "-lpopsift_hip", "-Wl,-rpath," + libdir]
    subprocess.check_call(cmd)
    env = {k: v for k, v in os.environ.items() if k != "POPSIFT_TEST_EXPECT_GPU"}
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120, env=env)
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout
