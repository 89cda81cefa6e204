"""The two ways through the frame's launch plan (csrc/hip/pyramid_plan.h) that psx_extract alone does not take: the stages
called one by one, where psx_find_extrema issues the plan's scan steps, and the blur probe on a context whose tile schedule
would take octave 0, where psx_build_pyramid falls back to the diagonal plan.  Both must give what psx_extract gives, bit for
bit.  The order in which an octave's features are emitted is the arrival order of its atomics and not a contract
(tests/parity.py), so extractions are compared in canonical order."""
import numpy as np
import pytest

from popsift_amd.synth import synth
from tests.parity import sort_iext

pytestmark = pytest.mark.gpu

FIELDS = ("debug_octave", "xpos", "ypos", "sigma", "num_ori", "orientation")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8).tobytes()


def canonical(feats, desc):
    """every record field, and per (record, orientation) the descriptor row, sorted by (octave, x, y, sigma, orientations)"""
    key = np.stack([feats["debug_octave"].astype(np.float64), feats["xpos"], feats["ypos"], feats["sigma"], feats["num_ori"]]
                   + [feats["orientation"][:, k] for k in range(4)], 1)
    f = feats[np.lexsort(key.T[::-1])]
    idx = f["desc_idx"][np.arange(4)[None, :] < f["num_ori"][:, None]]
    assert (idx >= 0).all() and (idx < len(desc)).all()
    return [bits(f[name]) for name in FIELDS] + [bits(desc[idx])]


def snapshot(capi, ctx):
    """planes, initial extrema per octave and the canonical extraction of the context's last frame"""
    planes = [bits(ctx.dump_plane(capi.PLANE_GAUSS, o, l)) for o in range(ctx.num_octaves) for l in range(ctx.num_levels)]
    iext = [bits(sort_iext(ctx.dump_iext(o))) for o in range(ctx.num_octaves)]
    feats, desc = ctx.download()
    assert len(feats) > 50 and len(desc) >= len(feats)
    return planes, iext, canonical(feats, desc)


def assert_same(got, want, what):
    for name, a, b in zip(("planes", "initial extrema", "features and descriptors"), got, want):
        assert len(a) == len(b) and all(x == y for x, y in zip(a, b)), (what, name)


@pytest.fixture(scope="module")
def image():
    return synth(300, 200, 77)


def test_stages_called_one_by_one_give_the_extraction(capi, image):
    whole = capi.Context(capi.default_config())
    whole.upload(image)
    whole.extract()
    want = snapshot(capi, whole)
    whole.close()
    ctx = capi.Context(capi.default_config())
    ctx.upload(image)
    for _ in range(2):                                   # a second frame: psx_find_extrema left no scan state behind
        ctx.build_pyramid()
        ctx.find_extrema()
        ctx.orientation()
        ctx.descriptors()
        assert_same(snapshot(capi, ctx), want, "stages apart")
    ctx.close()


def test_blur_probe_beside_a_tile_schedule_falls_back_to_the_diagonal_plan(capi, image, monkeypatch):
    monkeypatch.setenv("POPSIFT_TILE", "1")              # read at psx_create: every octave of this frame is tiled, octave 0 included
    plain, probed = capi.Context(capi.default_config()), capi.Context(capi.default_config())
    plain.upload(image)
    plain.extract()
    want = snapshot(capi, plain)
    plain.close()
    probed.upload(image)
    # the premise: this frame's tile plan starts with a tile launch, so the probe (octave 0 level by level) cannot use it
    spans = capi.gauss_tables(capi.default_config())["inc_span"]
    w0, h0 = probed.octave_dims(0)
    tile_plan = capi.pyramid_plan(w0, h0, probed.num_octaves, probed.num_levels - 3, spans, schedule=capi.PLAN_TILE)
    assert tile_plan is not None and tile_plan[0][0] == capi.STEP_TILE
    probed.enable_blur_probe(True)
    probed.extract()
    ms, nbytes = probed.blur_probe_times()
    assert len(ms) == probed.num_levels - 1 and all(m > 0.0 for m in ms), ms
    assert nbytes >= 8.0 * w0 * h0
    assert_same(snapshot(capi, probed), want, "probe on")
    probed.close()
