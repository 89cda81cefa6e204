"""GPU tests of caller-supplied keypoints: psx_set_keypoints / psx_describe / psx_keypoint_map through capi.Context, and
PopSift::enqueue(..., keypoints) through the flat C binding (a worker process, tests/keypoints_popsift_worker.py).

The reference for library-assigned orientations is psx_extract itself (same kernels behind the injection: the results
must be BIT-equal) and, independently, the CPU oracle within parity.budget; for given orientations it is the oracle's
descriptor stage on caller-supplied oriented extrema (pyoracle.Result.describe).

Every test runs under a watchdog of its own (faulthandler: the process is ended, nothing more is started on the GPU,
when a step does not come back); the PopSift path runs in a worker process with a timeout.  The order in which
psx_extract emits the features of an octave is the arrival order of its atomics and not a contract (tests/parity.py),
so two EXTRACTIONS are compared bit for bit in canonical order; the order of a describe call is a function of its
input and is compared as it is."""
import faulthandler
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from popsift_amd.synth import synth, synth_float
from tests.parity import assert_descriptor_rows, assert_parity, budget, match_features
from tests.test_keypoints_cpu import ROUND_TRIP

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("xpos", "ypos", "sigma", "num_ori", "orientation")
FULL_HD = (dict(sift_mode=2), (1920, 1080), 1000)
STEP_TIMEOUT = 420          # seconds per test: the slowest one runs the CPU oracle on a 1080p frame


@pytest.fixture(autouse=True)
def watchdog():
    faulthandler.dump_traceback_later(STEP_TIMEOUT, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8).tobytes()


def same_records(fa, fb, what=""):
    assert len(fa) == len(fb), (what, len(fa), len(fb))
    for name in FIELDS + ("debug_octave",):
        assert bits(fa[name]) == bits(fb[name]), (what, name, int((fa[name] != fb[name]).sum()))


def desc_rows(feats, desc):
    """(keypoint, orientation) -> descriptor row, -1 rows (beyond the descriptor capacity) excluded by assertion"""
    on = np.arange(4)[None, :] < feats["num_ori"][:, None]
    idx = feats["desc_idx"][on]
    assert (idx >= 0).all() and (idx < len(desc)).all()
    return desc[idx]


def canonical(feats, desc):
    """records and descriptor rows of an extraction in an order that does not depend on atomic arrival"""
    on = np.arange(4)[None, :] < feats["num_ori"][:, None]
    kp, k = np.nonzero(on)
    rows = desc[feats["desc_idx"][kp, k]]
    key = np.stack([feats["debug_octave"][kp].astype(np.float64), feats["xpos"][kp], feats["ypos"][kp], feats["sigma"][kp],
                    feats["orientation"][kp, k]], 1)
    order = np.lexsort(key.T[::-1])
    return bits(key[order]), bits(rows[order])


def detect(capi, kw, img):
    """psx_extract: context (left open), features, descriptors, level and octave of every feature (from dump_iext)"""
    ctx = capi.Context(capi.default_config(**kw))
    ctx.upload(img)
    ctx.extract()
    F, D = ctx.download()
    iext = [ctx.dump_iext(o) for o in range(ctx.num_octaves)]
    lpos = np.concatenate([e["lpos"] for e in iext]) if iext else np.zeros(0, np.int32)
    octave = np.concatenate([np.full(len(e), o, np.int32) for o, e in enumerate(iext)])
    assert len(lpos) == len(F) and np.array_equal(octave, F["debug_octave"])
    # features are the initial extrema in buffer order, in image units (an exact power-of-two scale)
    unit = np.exp2(octave.astype(np.float64) - int(ctx.cfg.upscale_factor)).astype(np.float32)
    assert bits(np.concatenate([e["xpos"] for e in iext]) * unit) == bits(F["xpos"])
    return ctx, F, D, octave, lpos


def records(capi, F, octave=None, lpos=None, ori=False):
    k = np.zeros(len(F), capi.KEYPOINT_DTYPE)
    for name in ("xpos", "ypos", "sigma"):
        k[name] = F[name]
    k["octave"] = capi.KP_AUTO if octave is None else octave
    if lpos is not None:
        k["lpos"] = lpos
    if ori:
        k["num_ori"], k["orientation"] = F["num_ori"], F["orientation"]
    return k


def describe(ctx, recs, reuse=False):
    ctx.set_keypoints(recs)
    ctx.describe(reuse_pyramid=reuse)
    F, D = ctx.download()
    src = ctx.keypoint_map()
    assert len(src) == len(F)
    return F, D, src


def check_against_detector(ctx, F, D, F2, D2, orig, what):
    """output feature i of a describe call came from detector feature orig[i]: every field and (loop mode: integer
    histogram sums, the order cannot matter) every descriptor bit-equal"""
    same_records(F[orig], F2, what)
    if ctx.cfg.desc_mode == 0:
        assert bits(desc_rows(F[orig], D)) == bits(desc_rows(F2, D2)), what


def in_caller_order(src, octaves):
    """octave-major, caller order inside an octave"""
    assert (np.diff(octaves) >= 0).all()
    for o in np.unique(octaves):
        assert (np.diff(src[octaves == o]) > 0).all(), o


@pytest.mark.parametrize("kw,size,seed", ROUND_TRIP + [FULL_HD])
def test_library_assigned_orientations(capi, oracle, kw, size, seed):
    """1. The detector's own keypoints as explicit records (octave, lpos from dump_iext; num_ori = 0) in a seeded random
    permutation: after undoing the permutation through keypoint_map every psx_feature field and every descriptor is
    bit-equal to psx_extract's; independently the result is within budget(n) of the oracle."""
    img = synth(size[0], size[1], seed)
    ctx, F, D, octave, lpos = detect(capi, kw, img)
    n = len(F)
    assert n > 500
    perm = np.random.default_rng(seed).permutation(n)
    recs = records(capi, F, octave, lpos)[perm]
    F2, D2, src = describe(ctx, recs)
    assert len(F2) == n and len(D2) == len(D)
    in_caller_order(src, F2["debug_octave"])
    check_against_detector(ctx, F, D, F2, D2, perm[src], str(kw))
    ref = oracle.run(oracle.default_config(**kw), img)
    m = match_features(ref.features(), ref.descriptors(), F2, D2)
    print(kw, size, {k: v for k, v in m.items() if k != "misses"})
    assert_parity(m, what=str(kw), **budget(n))
    ctx.close()


@pytest.mark.parametrize("desc_mode", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("norm", [dict(), dict(norm_mode=1, norm_multi=9)])
def test_given_orientations(capi, oracle, desc_mode, norm):
    """2. The oracle's oriented extrema as explicit records with their orientations given: adopted verbatim, and row
    idx_ori + k of the oracle's descriptor stage on the same records matches within budget; the same upright
    (num_ori = 1, orientation = 0)."""
    img = synth(480, 360, 8)
    kw = dict(octaves=4, desc_mode=desc_mode, **norm)
    scale = float(2 ** norm.get("norm_multi", 0))
    ref = oracle.run(oracle.default_config(**kw), img)
    ext = ref.extrema()
    ext = ext[ext["num_ori"] >= 1]                       # num_ori = 0 in a record means "the library assigns"
    n = len(ext)
    assert n > 500
    ctx = capi.Context(capi.default_config(**kw))
    ctx.upload(img)
    unit = np.exp2(ext["octave"].astype(np.float64) - int(ctx.cfg.upscale_factor)).astype(np.float32)
    recs = np.zeros(n, capi.KEYPOINT_DTYPE)
    for name in ("xpos", "ypos", "sigma"):
        recs[name] = ext[name] * unit
    recs["octave"], recs["lpos"] = ext["octave"], ext["lpos"]
    for upright in (False, True):
        e = ext.copy()
        if upright:
            e["num_ori"], e["orientation"] = 1, 0.0
        e["idx_ori"] = np.cumsum(e["num_ori"]) - e["num_ori"]
        recs["num_ori"], recs["orientation"] = e["num_ori"], e["orientation"]
        F2, D2, src = describe(ctx, recs, reuse=upright)
        assert len(F2) == n and np.array_equal(src, np.arange(n))
        assert np.array_equal(F2["num_ori"], e["num_ori"])
        on = np.arange(4)[None, :] < e["num_ori"][:, None]
        assert bits(np.where(on, e["orientation"], 0).astype(np.float32)) == bits(F2["orientation"])
        assert np.array_equal(F2["desc_idx"][on], (e["idx_ori"][:, None] + np.arange(4)[None, :])[on])
        dumped = ctx.dump_extrema()
        for name in ("xpos", "ypos", "sigma", "lpos", "octave", "num_ori", "idx_ori"):
            assert bits(dumped[name]) == bits(e[name]), name
        nd = int(e["num_ori"].sum())
        assert len(D2) == nd
        worst = assert_descriptor_rows(ref.describe(e, nd), D2, n, what="desc_mode %d upright %d" % (desc_mode, upright), norm_scale=scale)
        print("desc_mode %d %s upright %d: %d descriptors, max L2 %.3g" % (desc_mode, norm, upright, nd, worst))
    ctx.close()


@pytest.mark.parametrize("kw,size,seed", ROUND_TRIP)
def test_automatic_placement_end_to_end(capi, oracle, kw, size, seed):
    """3. Image-unit records with PSX_KP_AUTO for the detector keypoints of level 1 .. levels: the device places them
    where the detector found them; expectations as in test 1."""
    img = synth(size[0], size[1], seed)
    ctx, F, D, octave, lpos = detect(capi, kw, img)
    inner = np.flatnonzero((lpos >= 1) & (lpos <= ctx.cfg.levels))
    assert len(inner) > 500
    perm = np.random.default_rng(seed + 1).permutation(len(inner))
    recs = records(capi, F[inner])[perm]
    ho, hl = capi.place_keypoints(ctx.cfg, size[0], size[1], recs)
    assert np.array_equal(ho, octave[inner][perm]) and np.array_equal(hl, lpos[inner][perm])
    F2, D2, src = describe(ctx, recs)
    assert len(F2) == len(inner)
    in_caller_order(src, F2["debug_octave"])
    orig = inner[perm[src]]
    check_against_detector(ctx, F, D, F2, D2, orig, str(kw))
    assert np.array_equal(ctx.dump_extrema()["lpos"], lpos[orig])
    ref = oracle.run(oracle.default_config(**kw), img)
    m = match_features(F2, D2, ref.features(), ref.descriptors())
    assert_parity(m, what=str(kw), **budget(len(F2)))
    ctx.close()


def plane_digests(capi, ctx):
    return [hashlib.sha1(ctx.dump_plane(capi.PLANE_GAUSS, o, l).tobytes()).hexdigest()
            for o in range(ctx.num_octaves) for l in range(ctx.num_levels)]


def test_detect_filter_redescribe(capi):
    """4. PSX_DESCRIBE_REUSE_PYRAMID on every second detector keypoint: rows bit-equal to the detector's, the planes
    untouched, and a following psx_extract on the same context gives what it gave before."""
    kw, size, seed = ROUND_TRIP[0]
    img = synth(size[0], size[1], seed)
    ctx, F, D, octave, lpos = detect(capi, kw, img)
    before = plane_digests(capi, ctx)
    keep = np.arange(0, len(F), 2)
    F2, D2, src = describe(ctx, records(capi, F[keep], octave[keep], lpos[keep]), reuse=True)
    assert np.array_equal(src, np.arange(len(keep)))
    check_against_detector(ctx, F, D, F2, D2, keep, "reuse")
    assert plane_digests(capi, ctx) == before
    # the stage timers work on a describe call: [0] nothing (reused pyramid), [1] injection, [2] orientation, [3] descriptors
    ctx.enable_timers(True)
    ctx.describe(reuse_pyramid=True)
    ms = ctx.stage_times()
    print("stage times of describe(reuse_pyramid=True): %s ms" % ms)
    assert all(np.isfinite(ms)) and min(ms) >= 0 and ms[2] > 0 and ms[3] > 0, ms
    ctx.enable_timers(False)
    ctx.extract()
    F3, D3 = ctx.download()
    assert canonical(F3, D3) == canonical(F, D)
    with pytest.raises(capi.PopSiftError):
        ctx.keypoint_map()                                   # the last results are the detector's
    ctx.describe(reuse_pyramid=True)                         # the list is still set; the pyramid is the extraction's
    F4, D4 = ctx.download()
    same_records(F2, F4, "after extract")
    assert bits(D2) == bits(D4)
    # a new image invalidates the pyramid the context holds
    ctx.upload(synth(size[0], size[1], seed + 1))
    with pytest.raises(capi.PopSiftError):
        ctx.describe(reuse_pyramid=True)
    ctx.close()


def test_mixed_and_hostile_input(capi):
    """5. Rejected records of every kind interleaved with good ones, duplicates, explicit and automatic placement mixed,
    more than max_extrema records in one octave, several chunks of 256: counts, order and keypoint_map are exactly what
    the rule says (octave-major, caller order, the first max_extrema accepted records per octave)."""
    w, h = 320, 240
    cap = 150
    kw = dict(octaves=3, max_extrema=cap)
    img = synth(w, h, 4)
    ctx = capi.Context(capi.default_config(**kw))
    ctx.upload(img)
    rng = np.random.default_rng(5)
    n = 1500
    recs = np.zeros(n, capi.KEYPOINT_DTYPE)
    recs["xpos"] = rng.uniform(8, w - 8, n).astype(np.float32)
    recs["ypos"] = rng.uniform(8, h - 8, n).astype(np.float32)
    recs["sigma"] = np.exp2(rng.uniform(0.0, 3.2, n)).astype(np.float32)
    recs["octave"] = capi.KP_AUTO
    ex = rng.random(n) < 0.3                                  # explicit placement, sigma made to fit the octave
    recs["octave"][ex] = rng.integers(0, 3, int(ex.sum()))
    recs["lpos"][ex] = rng.integers(0, 6, int(ex.sum()))
    recs["sigma"][ex] = (np.float32(2.0) * np.exp2(recs["octave"][ex].astype(np.float32) - 1)).astype(np.float32)
    given = rng.random(n) < 0.4
    recs["num_ori"][given] = rng.integers(1, 5, int(given.sum()))
    recs["orientation"] = rng.uniform(-3.1, 3.1, (n, 4)).astype(np.float32)
    recs[100:140] = recs[60:100]                              # duplicates
    given = recs["num_ori"] > 0
    hostile = [("xpos", np.nan), ("ypos", np.inf), ("sigma", -1.0), ("sigma", 0.0), ("sigma", np.nan), ("xpos", -3.0),
               ("ypos", 1e9), ("sigma", 1e-3), ("sigma", 1e6), ("num_ori", 5), ("num_ori", -1), ("octave", 3), ("octave", -7),
               ("lpos", -1), ("lpos", 6)]
    bad = rng.choice(n, 20 * len(hostile), replace=False)
    for j, i in enumerate(bad):
        name, v = hostile[j % len(hostile)]
        if name == "lpos":
            recs["octave"][i] = 1
            recs["sigma"][i] = 2.0
        recs[name][i] = v
    nan_ori = rng.choice(np.flatnonzero(given), 15, replace=False)
    recs["orientation"][nan_ori, 0] = np.nan
    ho, hl = capi.place_keypoints(ctx.cfg, w, h, recs)
    assert (ho[nan_ori] == -1).all() and (ho[bad] == -1).all()
    want = np.concatenate([np.flatnonzero(ho == o)[:cap] for o in range(3)])
    assert max(int((ho == o).sum()) for o in range(3)) > cap          # the cap bites in at least one octave
    assert min(int((ho == o).sum()) for o in range(3)) > 10
    F2, D2, src = describe(ctx, recs)
    ne, no = ctx.counts()
    assert ne == len(want) and np.array_equal(src, want)
    assert np.array_equal(F2["debug_octave"], ho[want])
    for name in ("xpos", "ypos", "sigma"):
        assert bits(F2[name]) == bits(recs[name][want]), name
    ext = ctx.dump_extrema()
    assert np.array_equal(ext["lpos"], hl[want]) and np.array_equal(ext["octave"], ho[want])
    for o in range(3):
        assert len(ctx.dump_iext(o)) == min(cap, int((ho == o).sum()))
    g = recs["num_ori"][want] > 0                             # given orientations adopted, the others assigned
    assert np.array_equal(F2["num_ori"][g], recs["num_ori"][want][g]) and (F2["num_ori"][~g] >= 1).all()
    on = np.arange(4)[None, :] < F2["num_ori"][:, None]
    assert bits(F2["orientation"][g][on[g]]) == bits(recs["orientation"][want][g][on[g]])
    assert no == int(F2["num_ori"].sum()) == len(D2) and np.isfinite(D2).all()
    # duplicates give identical rows
    d0, d1 = np.flatnonzero(np.isin(want, np.arange(60, 100))), np.flatnonzero(np.isin(want, np.arange(100, 140)))
    pairs = [(a, b) for a in d0 for b in d1 if want[b] == want[a] + 40]
    assert len(pairs) > 5
    for a, b in pairs:
        assert bits(desc_rows(F2[a:a + 1], D2)) == bits(desc_rows(F2[b:b + 1], D2))
    # an empty list: zero features, an empty map, everything downstream still works
    for empty in (None, recs[:0]):
        ctx.set_keypoints(empty)
        ctx.describe(reuse_pyramid=True)
        assert ctx.counts() == (0, 0) and len(ctx.keypoint_map()) == 0 and len(ctx.download()[0]) == 0
    # a list of rejected records only
    ctx.set_keypoints(recs[bad])
    ctx.describe()
    assert ctx.counts() == (0, 0)
    ctx.close()


def test_calls_out_of_sequence(capi):
    ctx = capi.Context(capi.default_config(octaves=3))
    recs = np.zeros(1, capi.KEYPOINT_DTYPE)
    with pytest.raises(capi.PopSiftError):
        ctx.set_keypoints(recs)                              # no input image yet
    ctx.upload(synth(160, 120, 1))
    with pytest.raises(capi.PopSiftError):
        ctx.describe()                                       # no keypoints set
    ctx.set_keypoints(recs)
    with pytest.raises(capi.PopSiftError):
        ctx.describe(reuse_pyramid=True)                     # no pyramid of this input
    assert capi.lib().psx_describe(ctx._h, 6) == -1          # unknown flag
    ctx.describe()
    assert ctx.counts() == (0, 0)                            # sigma 0: dropped
    ctx.close()


def test_device_pointer_bytes_and_clone(capi):
    """6. Records in a torch tensor on the device (no copy) give the host list's result; byte format gives
    quantize_rule of the floats; psx_clone_results (what MatchingMode hands out) holds the same descriptors."""
    import torch
    kw, size, seed = ROUND_TRIP[1]
    img = synth(size[0], size[1], seed)
    ctx, F, D, octave, lpos = detect(capi, kw, img)
    recs = records(capi, F, octave, lpos)[::-1].copy()
    F2, D2, src = describe(ctx, recs)
    t = torch.from_numpy(recs.view(np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    ctx.set_keypoints(t)
    ctx.describe(reuse_pyramid=True)
    F3, D3 = ctx.download()
    same_records(F2, F3, "device pointer")
    assert bits(D2) == bits(D3) and np.array_equal(ctx.keypoint_map(), src)
    cf, cd, rev, base = ctx.clone_results()
    assert bits(cd) == bits(D2) and len(cf) == len(F2)
    for name in FIELDS:
        assert bits(cf[name]) == bits(F2[name]), name
    on = np.arange(4)[None, :] < F2["num_ori"][:, None]
    assert np.array_equal((cf["desc"][on] - base) // 512, F2["desc_idx"][on])
    assert np.array_equal(rev[F2["desc_idx"][on]], np.nonzero(on)[0])
    ctx.set_descriptor_format(capi.DESCFMT_U8)
    ctx.describe(reuse_pyramid=True)
    F4, B4 = ctx.download_u8()
    same_records(F2, F4, "byte mode")
    assert B4.dtype == np.uint8 and np.array_equal(B4, capi.quantize_rule(D2))
    assert bits(ctx.download()[1]) == bits(D2)
    ctx.close()


def test_popsift_enqueue_with_keypoints(capi, tmp_path):
    """6. capi.PopSift.enqueue(img, keypoints=...) through popsift_c, byte and float images, float and byte descriptors:
    the features, descriptors and source indices of the Context path; an empty list gives an empty result; the detector
    jobs of the same PopSift are what they are without keypoint jobs in between."""
    out = str(tmp_path / "kp.npz")
    subprocess.run([sys.executable, "-m", "tests.keypoints_popsift_worker", out], cwd=ROOT, check=True, timeout=STEP_TIMEOUT)
    z = np.load(out)
    for tag in ("u8", "f32"):
        cf, cd, cs = z[tag + "_ctx_feat"], z[tag + "_ctx_desc"], z[tag + "_ctx_src"]
        assert len(cf) > 300
        for k in range(3):                                   # several jobs in flight over the worker contexts
            pf, pd, ps = z["%s_ps_feat_%d" % (tag, k)], z["%s_ps_desc_%d" % (tag, k)], z["%s_ps_src_%d" % (tag, k)]
            same_records(cf, pf, tag)
            assert bits(desc_rows(cf, cd)) == bits(desc_rows(pf, pd)) and np.array_equal(cs, ps)
        assert len(z[tag + "_ps_empty_feat"]) == 0 and len(z[tag + "_ps_empty_src"]) == 0
        assert len(z[tag + "_ps_det_src"]) == 0
        assert canonical(z[tag + "_ps_det_feat"], z[tag + "_ps_det_desc"]) == canonical(z[tag + "_ctx_det_feat"], z[tag + "_ctx_det_desc"])
    bf, bd = z["u8_ps_bytes_feat"], z["u8_ps_bytes_desc"]
    same_records(z["u8_ctx_feat"], bf, "byte descriptors")
    assert bd.dtype == np.uint8 and np.array_equal(desc_rows(bf, bd), capi.quantize_rule(desc_rows(z["u8_ctx_feat"], z["u8_ctx_desc"])))


def test_cpp_keypoint_overloads_on_the_gpu(tmp_path):
    """tests/cpp/test_keypoints_api.cpp with POPSIFT_TEST_EXPECT_GPU: null and zero-length lists yield empty results,
    a real list its survivors in caller order with their source indices, ExtractingMode and MatchingMode."""
    libdir = os.path.join(ROOT, "popsift_amd", "lib")
    exe = str(tmp_path / "test_keypoints_api")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-pthread", os.path.join(ROOT, "tests", "cpp", "test_keypoints_api.cpp"), "-o", exe,
                           "-I", os.path.join(ROOT, "popsift_amd", "csrc", "include"), "-I", os.path.join(ROOT, "include"),
                           "-L", libdir, "-lpopsift", "-lpopsift_hip", "-Wl,-rpath," + libdir])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300,
                       env=dict(os.environ, POPSIFT_TEST_EXPECT_GPU="1", POPSIFT_PIPE_DEPTH="2"))
    assert p.returncode == 0 and "ALL OK" in p.stdout, p.stdout
