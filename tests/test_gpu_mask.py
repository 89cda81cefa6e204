"""GPU tests of the detection mask: psx_set_mask / psx_set_mask_dev through capi.Context, PopSift::enqueue(..., mask)
through the flat C binding (a worker process, tests/mask_popsift_worker.py), the C++ overloads and popsift-demo --mask.

The reference for a masked extraction is the UNMASKED extraction of the same context, filtered on the host by the rule
on the reported positions (capi.mask_keep, and independently its numpy restatement): the masked result must hold
exactly those rows, bit for bit.  Independently the CPU oracle's features, filtered the same way, must match within
parity.budget.  The order in which psx_extract emits the features of an octave is the arrival order of its atomics and
not a contract (tests/parity.py), so extractions are compared in canonical order.

Every test runs under a watchdog of its own (faulthandler: the process is ended, nothing more is started on the GPU,
when a step does not come back); the PopSift path runs in a worker process with a timeout."""
import faulthandler
import os
import subprocess
import sys

import numpy as np
import pytest
import torch        # before the HIP library is loaded: torch brings a HIP runtime of its own and must initialise first (test 7)

from popsift_amd.synth import synth
from tests.mask_cases import CONFIGS, CONFIG_IDS, FULL_HD, MASKS, assert_premise, make_mask, restate_keep
from tests.parity import assert_parity, budget, match_features, sort_iext

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(ROOT, "popsift_amd", "lib", "popsift-demo")
FIELDS = ("debug_octave", "xpos", "ypos", "sigma", "num_ori", "orientation")
STEP_TIMEOUT = 420          # seconds per test: the slowest one runs the CPU oracle on a 1080p frame


@pytest.fixture(autouse=True)
def watchdog():
    faulthandler.dump_traceback_later(STEP_TIMEOUT, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8).tobytes()


def canonical(feats, desc):
    """Every record field and every descriptor row of an extraction in an order that does not depend on atomic arrival:
    the records sorted by (octave, x, y, sigma, orientations), then per (record, orientation) the descriptor row."""
    key = np.stack([feats["debug_octave"].astype(np.float64), feats["xpos"], feats["ypos"], feats["sigma"], feats["num_ori"]]
                   + [feats["orientation"][:, k] for k in range(4)], 1)
    order = np.lexsort(key.T[::-1])
    f = feats[order]
    on = np.arange(4)[None, :] < f["num_ori"][:, None]
    idx = f["desc_idx"][on]
    assert (idx >= 0).all() and (idx < len(desc)).all()
    return tuple(bits(f[name]) for name in FIELDS), bits(desc[idx])


def assert_same_extraction(got, want, what):
    (gf, gd), (wf, wd) = got, want
    for name, a, b in zip(FIELDS, gf, wf):
        assert a == b, (what, name)
    assert gd == wd, (what, "descriptors")


def octave_counts(ctx):
    return [len(ctx.dump_iext(o)) for o in range(ctx.num_octaves)]


def extract(ctx):
    ctx.extract()
    F, D = ctx.download()
    return F, D


def keep_of(capi, mask, F):
    keep = capi.mask_keep(mask, F["xpos"], F["ypos"])
    assert np.array_equal(keep, restate_keep(mask, F["xpos"], F["ypos"]))
    return keep


def iext_image_units(ctx, o):
    e = ctx.dump_iext(o)
    unit = np.float32(2.0 ** (o - int(ctx.cfg.upscale_factor)))
    return e, e["xpos"] * unit, e["ypos"] * unit


_RUNS = {}


def runs(capi, i):
    """Config i: the unmasked extraction and the masked one for every mask, on one context (shared by tests 1 and 2)"""
    if i in _RUNS:
        return _RUNS[i]
    kw, (w, h), seed = CONFIGS[i]
    img = synth(w, h, seed)
    ctx = capi.Context(capi.default_config(**kw))
    ctx.upload(img)
    F0, D0 = extract(ctx)
    assert ctx.cfg.desc_mode == capi.DESC_LOOP            # integer histogram sums: descriptor bits are comparable
    iext0 = [iext_image_units(ctx, o) for o in range(ctx.num_octaves)]
    assert max(len(e[0]) for e in iext0) < ctx.cfg.max_extrema
    out = dict(img=img, F0=F0, D0=D0, masked={})
    for name in MASKS:
        m = make_mask(name, w, h)
        ctx.set_mask(m)
        F, D = extract(ctx)
        counts = octave_counts(ctx)
        assert max(counts) < ctx.cfg.max_extrema
        out["masked"][name] = (m, F, D)
        # dump_iext of the masked run holds exactly the survivors
        for o, (e0, x0, y0) in enumerate(iext0):
            ko = restate_keep(m, x0, y0)
            assert bits(sort_iext(ctx.dump_iext(o))) == bits(sort_iext(e0[ko])), (CONFIG_IDS[i], name, o)
    ctx.set_mask(None)
    F1, D1 = extract(ctx)
    assert_same_extraction(canonical(F1, D1), canonical(F0, D0), "mask cleared")
    ctx.close()
    _RUNS[i] = out
    return out


@pytest.mark.parametrize("i", range(len(CONFIGS)), ids=CONFIG_IDS)
def test_masked_equals_filtered(capi, i):
    """1. psx_extract without a mask, then with each mask, on the same context: the masked result is the unmasked
    result's rows selected by the rule on their reported positions, in every record field and every descriptor bit;
    both runs stay below max_extrema in every octave; dump_iext holds exactly the survivors (in runs())."""
    r = runs(capi, i)
    F0, D0 = r["F0"], r["D0"]
    for name in MASKS:
        m, F, D = r["masked"][name]
        keep = keep_of(capi, m, F0)
        print("%s %s: %d of %d kept" % (CONFIG_IDS[i], name, len(F), len(F0)))
        assert_premise(name, int(keep.sum()), len(F0), CONFIG_IDS[i])
        assert len(F) == int(keep.sum()) and len(D) == int(F0["num_ori"][keep].sum())
        assert len(np.unique(F["debug_octave"])) >= 3                     # several octaves
        assert_same_extraction(canonical(F, D), canonical(F0[keep], D0), "%s %s" % (CONFIG_IDS[i], name))
        assert restate_keep(m, F["xpos"], F["ypos"]).all()


@pytest.mark.parametrize("i", range(len(CONFIGS)), ids=CONFIG_IDS)
def test_masked_against_the_oracle(capi, oracle, i):
    """2. The oracle's features filtered by the rule against the masked GPU result: within budget(n), which allows no
    keypoint mismatch (positions are bit-equal by construction), and the same number of keypoints."""
    kw, (w, h), seed = CONFIGS[i]
    r = runs(capi, i)
    ref = oracle.run(oracle.default_config(**kw), r["img"])
    fa, da = ref.features(), ref.descriptors()
    for name in MASKS:
        m, F, D = r["masked"][name]
        keep = keep_of(capi, m, fa)
        assert_premise(name, int(keep.sum()), len(fa), CONFIG_IDS[i])
        assert len(F) == int(keep.sum()), (name, len(F), int(keep.sum()))
        res = match_features(fa[keep], da, F, D)
        print(CONFIG_IDS[i], name, {k: v for k, v in res.items() if k != "misses"})
        assert_parity(res, what="%s %s" % (CONFIG_IDS[i], name), **budget(len(F)))


def test_ones_and_zeros(capi):
    """3. An all-ones mask is bit-equal to no mask; an all-zero mask gives counts 0 / 0, empty downloads and no error;
    clearing the mask afterwards restores the unmasked result."""
    kw, (w, h), seed = CONFIGS[0]
    ctx = capi.Context(capi.default_config(**kw))
    ctx.upload(synth(w, h, seed))
    base = canonical(*extract(ctx))
    ctx.set_mask(make_mask("ones", w, h))
    assert_same_extraction(canonical(*extract(ctx)), base, "ones")
    ctx.set_mask(make_mask("zeros", w, h))
    ctx.extract()
    assert ctx.counts() == (0, 0)
    F, D = ctx.download()
    assert len(F) == 0 and len(D) == 0 and octave_counts(ctx) == [0] * ctx.num_octaves and len(ctx.dump_extrema()) == 0
    ctx.extract()                                             # sticky: still in force
    assert ctx.counts() == (0, 0)
    ctx.set_mask(None)
    assert_same_extraction(canonical(*extract(ctx)), base, "cleared")
    ctx.close()


def test_masked_out_points_take_no_slot(capi):
    """4. max_extrema = 200 and `half` on the 1080p frame: every octave's count is min(200, the survivors of that octave
    in the uncapped masked run) -- a masked-out point does not count toward max_extrema -- and every feature lies
    inside the mask."""
    kw, (w, h), seed = FULL_HD
    img = synth(w, h, seed)
    m = make_mask("half", w, h)
    ctx = capi.Context(capi.default_config(**kw))
    ctx.upload(img)
    ctx.set_mask(m)
    ctx.extract()
    survivors = octave_counts(ctx)
    ctx.set_mask(None)
    ctx.extract()
    unmasked = octave_counts(ctx)
    ctx.close()
    cap = 200
    # the cap bites, and in at least one octave the masked-out points alone would fill it: if they took slots, that
    # octave would hold fewer than min(cap, survivors)
    assert max(survivors) > 4 * cap and max(u - s for u, s in zip(unmasked, survivors)) > cap
    ctx = capi.Context(capi.default_config(max_extrema=cap, **kw))
    ctx.upload(img)
    ctx.set_mask(m)
    F, D = extract(ctx)
    counts = octave_counts(ctx)
    print("survivors %s unmasked %s capped %s" % (survivors, unmasked, counts))
    assert counts == [min(cap, s) for s in survivors]
    assert len(F) == sum(counts) and restate_keep(m, F["xpos"], F["ypos"]).all()
    ctx.close()


def test_mask_before_grid_filter(capi):
    """5. 640 x 480 default with filter_max_extrema = 1500 and `half`: unmasked the grid filter runs (more than 1650
    extrema), masked it must not (fewer than 1650 survivors) -- masked-out points do not count toward its test -- so
    the masked, filtered result is the masked result of a context with the filter off.  With filter_max_extrema = 400
    the filter does run on the survivors: every feature inside the mask, no more than the filter allows."""
    kw, (w, h), seed = CONFIGS[0]
    img = synth(w, h, seed)
    m = make_mask("half", w, h)
    fmax = 1500
    off = capi.Context(capi.default_config(**kw))
    off.upload(img)
    off.extract()
    n_unmasked = sum(octave_counts(off))
    off.set_mask(m)
    Fm, Dm = extract(off)
    n_masked = sum(octave_counts(off))
    off.close()
    assert n_unmasked > int(fmax * 1.1) > n_masked > 300, (n_unmasked, n_masked)      # both premises
    on = capi.Context(capi.default_config(filter_max_extrema=fmax, **kw))
    on.upload(img)
    F, D = extract(on)
    assert len(F) < n_unmasked                                # unmasked, the filter runs
    on.set_mask(m)
    F, D = extract(on)
    assert_same_extraction(canonical(F, D), canonical(Fm, Dm), "masked, filter not triggered")
    on.close()
    small = capi.Context(capi.default_config(filter_max_extrema=400, **kw))
    small.upload(img)
    small.set_mask(m)
    F, D = extract(small)
    print("filter_max_extrema 400 on %d survivors: %d features" % (n_masked, len(F)))
    assert 0 < len(F) < n_masked and restate_keep(m, F["xpos"], F["ypos"]).all()
    # what the filter allows (gridfilter.hip, s_filtergrid.cu:219-262): the ct fullest cells are cut to
    # newlimit = ceil(tail / ct - floor((total - fmax) / ct)); ct * newlimit < tail - (total - fmax) + 2 ct, the other
    # cells keep what they have, so at most fmax + 2 ct <= fmax + 2 * grid^2 extrema stay
    assert len(F) <= 400 + 2 * small.cfg.filter_grid_size ** 2
    small.close()


def test_candidate_list_overflow_path(capi):
    """6. The content and configuration of test_max_extrema_cap_and_candidate_overflow (a tiny max_extrema makes the
    candidate sub-lists of k_extrema overflow: most survivors are refined in place, in k_extrema itself) with checker1.
    With the cap biting, WHICH survivors take the slots is arrival order, so the comparison with the filtered unmasked
    result is: every feature is a row of the uncapped unmasked result that the rule keeps (bit-equal record and
    descriptors), no row twice, and every octave holds min(cap, its survivors)."""
    w, h = 640, 480
    img = synth(w, h, 808)
    m = make_mask("checker1", w, h)
    cap = 40
    full = capi.Context(capi.default_config(octaves=4))
    full.upload(img)
    F0, D0 = extract(full)
    full.set_mask(m)
    full.extract()
    survivors = octave_counts(full)
    full.close()
    assert max(survivors) > 5 * cap                           # more survivors alone than list entries (4 * cap per octave)
    keep = keep_of(capi, m, F0)
    ctx = capi.Context(capi.default_config(octaves=4, max_extrema=cap))
    ctx.upload(img)
    ctx.set_mask(m)
    F, D = extract(ctx)
    assert octave_counts(ctx) == [min(cap, s) for s in survivors]
    assert len(F) == sum(min(cap, s) for s in survivors) and len(D) == int(F["num_ori"].sum())
    assert restate_keep(m, F["xpos"], F["ypos"]).all()
    rec = lambda A: [bits(np.array([a[n] for n in FIELDS[:4]], np.float64)) + bits(a["orientation"]) + bytes([int(a["num_ori"])]) for a in A]
    allowed = {}
    for a, r in zip(F0[keep], rec(F0[keep])):
        allowed.setdefault(r, []).append(a)
    seen = {}
    for a, r in zip(F, rec(F)):
        assert r in allowed, "a feature that is no kept row of the unmasked result"
        seen[r] = seen.get(r, 0) + 1
        assert seen[r] <= len(allowed[r])
        b = allowed[r][0]
        for k in range(int(a["num_ori"])):
            assert bits(D[a["desc_idx"][k]]) == bits(D0[b["desc_idx"][k]])
    ctx.close()


def test_device_mask(capi):
    """7. set_mask_tensor with a torch.uint8 and a torch.bool tensor gives the result of set_mask with the same values;
    a tensor written on another torch stream needs no more than stream order against the context's stream."""
    kw, (w, h), seed = CONFIGS[1]
    m = make_mask("blocks16", w, h)
    ctx = capi.Context(capi.default_config(**kw))
    ctx.upload(synth(w, h, seed))
    ctx.set_mask(m)
    want = canonical(*extract(ctx))
    unmasked_n = None
    for t in (torch.from_numpy(m).cuda(), torch.from_numpy(m != 0).cuda()):
        torch.cuda.synchronize()
        ctx.set_mask_tensor(t)
        assert_same_extraction(canonical(*extract(ctx)), want, str(t.dtype))
    # written on a side stream behind other work, ordered by an event wait of the context's stream only
    side = torch.cuda.Stream()
    t = torch.zeros((h, w), dtype=torch.uint8, device="cuda")
    src = torch.from_numpy(m).cuda()
    torch.cuda.synchronize()
    ctx.set_mask_tensor(t)
    with torch.cuda.stream(side):
        a = torch.randn(2048, 2048, device="cuda")
        for _ in range(8):
            a = a @ a * 1e-3                                   # keeps the side stream busy in front of the write
        t.copy_(src)
    torch.cuda.ExternalStream(ctx.stream).wait_stream(side)
    ctx.extract()
    got = canonical(*ctx.download())
    assert_same_extraction(got, want, "side stream")
    ctx.set_mask(None)
    ctx.extract()
    unmasked_n = ctx.counts()[0]
    assert unmasked_n > len(want[0][0]) // 4                   # the mask had an effect (record bytes / 4 per int32 field)
    ctx.close()


def test_state_and_describe(capi):
    """8. A mask of another size: PSX_ERR_STATE from extract and find_extrema, the message names both sizes, nothing is
    dropped silently; a correct upload or a clear makes the context work again; bad arguments leave the context as it
    was; describe ignores the mask."""
    kw, (w, h), seed = CONFIGS[0]
    img = synth(w, h, seed)
    ctx = capi.Context(capi.default_config(**kw))
    ctx.upload(img)
    base = canonical(*extract(ctx))
    m = make_mask("disc", w, h)
    ctx.set_mask(m)
    masked = canonical(*extract(ctx))
    assert masked != base
    # bad arguments: PSX_ERR_INVALID, the mask in force stays
    L = capi.lib()
    assert L.psx_set_mask(ctx._h, None, w, h) == -1 and L.psx_set_mask(ctx._h, m.ctypes.data, 0, h) == -1
    assert L.psx_set_mask(ctx._h, m.ctypes.data, w, -3) == -1 and L.psx_set_mask_dev(ctx._h, None, 1, 0) == -1
    assert_same_extraction(canonical(*extract(ctx)), masked, "after refused calls")
    ctx.set_mask(make_mask("disc", w - 16, h))
    for call in (ctx.extract, ctx.find_extrema):
        with pytest.raises(capi.PopSiftError) as e:
            call()
        assert "(-4)" in str(e.value) and "%d x %d" % (w - 16, h) in str(e.value) and "%d x %d" % (w, h) in str(e.value), str(e.value)
    ctx.set_mask(m)                                            # a correct upload
    assert_same_extraction(canonical(*extract(ctx)), masked, "after a correct upload")
    ctx.set_mask(make_mask("disc", w, h + 2))
    with pytest.raises(capi.PopSiftError):
        ctx.extract()
    ctx.set_mask(None)                                         # a clear
    assert_same_extraction(canonical(*extract(ctx)), base, "after a clear")
    # an image of another size under a sticky mask: refused until the mask fits again
    ctx.set_mask(m)
    small = synth(w - 64, h, seed)
    ctx.upload(small)
    with pytest.raises(capi.PopSiftError):
        ctx.extract()
    ctx.upload(img)
    assert_same_extraction(canonical(*extract(ctx)), masked, "image size restored")
    # describe ignores the mask: the caller chose those points
    ctx.set_mask(None)
    F0, D0 = extract(ctx)
    recs = np.zeros(len(F0), capi.KEYPOINT_DTYPE)
    for name in ("xpos", "ypos", "sigma"):
        recs[name] = F0[name]
    recs["octave"] = capi.KP_AUTO
    ctx.set_keypoints(recs)
    ctx.describe()
    Fa, Da = ctx.download()
    for mm in (make_mask("zeros", w, h), make_mask("disc", w + 8, h)):       # not even its size is looked at
        ctx.set_mask(mm)
        ctx.describe()
        Fb, Db = ctx.download()
        assert len(Fb) == len(Fa) > 300 and bits(Fa) == bits(Fb) and bits(Da) == bits(Db)
    ctx.close()


def test_popsift_enqueue_with_masks(capi, tmp_path):
    """9. 48 jobs alternating masked and unmasked, two different masks, from 4 caller threads (two rounds): every result
    equals the single-context result for its (image, mask) -- a mask that leaked from one job to the next on a reused
    context would show --, the pinned pool's allocation and free counters do not move after the warm-up (the worker
    says what the warm-up is and why a plain round is none), and byte-descriptor mode with a mask gives the quantised
    rows of the float result."""
    from tests.mask_popsift_worker import NJOBS, job_spec
    out = str(tmp_path / "mask.npz")
    subprocess.run([sys.executable, "-m", "tests.mask_popsift_worker", out], cwd=ROOT, check=True, timeout=STEP_TIMEOUT)
    z = np.load(out)
    assert len(z["errors"]) == 0, z["errors"]
    sizes = set()
    for i in range(NJOBS):
        k, name = job_spec(i)
        want = canonical(z["ctx_feat_%d_%s" % (k, name)], z["ctx_desc_%d_%s" % (k, name)])
        assert_same_extraction(canonical(z["ps_feat_%d" % i], z["ps_desc_%d" % i]), want, "job %d (image %d, mask %s)" % (i, k, name))
        sizes.add((k, name, len(z["ps_feat_%d" % i])))
    for k in range(3):                                        # the masks did something, and not the same thing
        n = {name: cnt for kk, name, cnt in sizes if kk == k}
        assert n[None] > n["checker1"] > 300 and n[None] > n["disc"] > 300 and n["checker1"] != n["disc"], n
    print("pool allocs / frees after warm-up %s, at the end %s" % (z["pool_warm"], z["pool_end"]))
    assert np.array_equal(z["pool_warm"], z["pool_end"])
    bf, bd = z["bytes_feat"], z["bytes_desc"]
    cf, cd = z["ctx_feat_0_disc"], z["ctx_desc_0_disc"]
    assert bd.dtype == np.uint8
    assert_same_extraction(canonical(bf, bd), canonical(cf, capi.quantize_rule(cd)), "byte descriptors")


def test_cpp_mask_overloads_on_the_gpu(tmp_path):
    """tests/cpp/test_mask_api.cpp with POPSIFT_TEST_EXPECT_GPU on ONE worker context: an all-ones mask gives the
    unmasked counts, an all-zero mask an empty result (ExtractingMode and MatchingMode), and the unmasked job behind a
    masked one on the same context is unmasked."""
    libdir = os.path.join(ROOT, "popsift_amd", "lib")
    exe = str(tmp_path / "test_mask_api")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-pthread", os.path.join(ROOT, "tests", "cpp", "test_mask_api.cpp"), "-o", exe,
                           "-I", os.path.join(ROOT, "popsift_amd", "csrc", "include"), "-I", os.path.join(ROOT, "include"),
                           "-L", libdir, "-lpopsift", "-lpopsift_hip", "-Wl,-rpath," + libdir])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300,
                       env=dict(os.environ, POPSIFT_TEST_EXPECT_GPU="1", POPSIFT_PIPE_DEPTH="1"))
    assert p.returncode == 0 and "ALL OK" in p.stdout, p.stdout


def test_demo_mask_option(capi, tmp_path):
    """10. popsift-demo --mask on a written PGM pair gives the features of test 1: the rows of the masked context
    result, in the tool's text format."""
    kw, (w, h), seed = CONFIGS[0]
    img = synth(w, h, seed)
    with open(str(tmp_path / "in.pgm"), "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (w, h) + img.tobytes())
    ctx = capi.Context(capi.default_config(**kw))
    ctx.upload(img)
    for name in ("checker1", "half"):
        m = make_mask(name, w, h)
        with open(str(tmp_path / "mask.pgm"), "wb") as f:
            f.write(b"P5\n# %s\n%d %d\n255\n" % (name.encode(), w, h) + m.tobytes())
        ctx.set_mask(m)
        F, D = extract(ctx)
        p = subprocess.run([DEMO, "-i", "in.pgm", "--mask", "mask.pgm"], cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           text=True, timeout=300)
        assert p.returncode == 0, p.stdout + p.stderr
        assert "Number of feature points: %d number of feature descriptors: %d" % (len(F), len(D)) in p.stderr, p.stderr
        rows = []
        for a in F:
            s = np.float32(1.0) / (a["sigma"] * a["sigma"])
            for k in range(a["num_ori"]):
                rows.append(np.concatenate([[a["xpos"], a["ypos"], s, 0.0, s], D[a["desc_idx"][k]]]))
        exp = np.array(rows)
        srt = lambda r: r[np.lexsort((r[:, 5], r[:, 2], r[:, 1], r[:, 0]))]
        got = srt(np.loadtxt(str(tmp_path / "output-features.txt"), ndmin=2))
        exp = srt(np.array([[float("%g" % v) for v in r[:5]] + [float("%.3g" % v) for v in r[5:]] for r in exp]))
        assert got.shape == exp.shape == (len(D), 133)
        assert np.allclose(got, exp, rtol=1e-6, atol=0), name       # the same numbers through the same text format
        assert restate_keep(m, got[:, 0].astype(np.float32), got[:, 1].astype(np.float32)).mean() > 0.99
    ctx.close()
