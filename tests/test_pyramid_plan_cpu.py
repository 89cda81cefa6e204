"""The frame's launch plan (csrc/hip/pyramid_plan.h, psx_pyramid_plan), checked without a device: the default diagonal
schedule against a restatement of the rule in Python, step for step, and the ordering invariants of every plan -- diagonal,
tile and flow.  The plan is what psx_build_pyramid issues behind the level-0 launch of octave 0, so the step count is the
launch count."""
import ctypes as C
import math

import numpy as np
import pytest

from tests.test_gpu_schedule import CASES

RESIDENT = [1024, 64, 1 << 20]       # an MI355X; only the tiniest planes pair; every pair fits and every scan is deferred


@pytest.fixture(autouse=True)
def default_tuning(monkeypatch):
    for name in ("POPSIFT_BATCH_OCTAVES", "POPSIFT_BLUR_STEPS", "POPSIFT_BLUR_ONESTEP", "POPSIFT_TILE_TY", "POPSIFT_TILE_NT",
                 "POPSIFT_TILE_MAXPX", "POPSIFT_TILE_SMALL"):
        monkeypatch.delenv(name, raising=False)


def octave_sizes(capi, w, h, kw):
    """(w, h) of every octave as psx_resize derives them (octaves = -1: from the smaller side)"""
    cfg = capi.default_config(**kw)
    scale = 2.0 ** cfg.upscale_factor
    n = cfg.octaves
    if n < 0:
        n = max(int((min(w, h).bit_length() - 1) - 3 + scale), 1)
        # the library's own count (kp_place.h): a keypoint of 3 sigma0 in units of octave n-1 is placed there automatically
        # only when that is the last octave -- with more octaves it moves on, with fewer it is out of range and dropped
        kp = np.zeros((1,), capi.KEYPOINT_DTYPE)
        kp[0] = (0.0, 0.0, 3.0 * cfg.sigma * 2.0 ** (n - 1) / scale, capi.KP_AUTO, 0, 1, (0.0,) * capi.ORI_MAX)
        assert capi.place_keypoints(cfg, w, h, kp)[0][0] == n - 1
    n = min(max(n, 1), capi.MAX_OCTAVES)
    ow, oh = math.ceil(w * scale), math.ceil(h * scale)
    sizes = []
    for _ in range(n):
        sizes.append((ow, oh))
        ow, oh = (ow + 1) // 2, (oh + 1) // 2
    return cfg, sizes


def restate_diagonal(capi, sizes, L, spans, resident):
    """The diagonal schedule as the parent's psx_build_pyramid walked it: start slots per octave, then launches per slot.
    Returns the steps and how often a slot paired two planes / refused a pair / left a third plane alone."""
    n, D = len(sizes), L - 3
    pair_ok = lambda o, o2, span: capi.blur_grid(*sizes[o], span) + capi.blur_grid(*sizes[o2], span) <= resident
    tiles = lambda o: -(-sizes[o][0] // 64) * -(-sizes[o][1] // 16)
    t0 = [0]
    for o in range(n - 1):
        t0.append(t0[o] + (D if pair_ok(o, o + 1, spans[L - 1]) else L - 1))
    steps, deferred, seen = [], [], dict(pair=0, refused=0, odd=0)
    for t in range(1, t0[-1] + L):
        jo = [o for o in range(n) if 1 <= t - t0[o] <= L - 1][:4]
        for q in range(0, len(jo), 2):
            o, l = jo[q], t - t0[jo[q]]
            if q + 1 == len(jo):
                steps.append((capi.STEP_BLUR, 0, o, l, 0, 0))
                seen["odd"] += len(jo) > 1
                continue
            o2, l2 = jo[q + 1], t - t0[jo[q + 1]]
            if pair_ok(o, o2, max(spans[l], spans[l2])):
                steps.append((capi.STEP_BLUR2, 0, o, l, o2, l2))
                seen["pair"] += 1
            else:
                steps += [(capi.STEP_BLUR, 0, o, l, 0, 0), (capi.STEP_BLUR, 0, o2, l2, 0, 0)]
                seen["refused"] += 1
        for o in jo:
            if t - t0[o] == L - 1:
                if tiles(o) >= resident:
                    steps.append((capi.STEP_SCAN, 0, o, 0, 0, 0))
                else:
                    deferred.append(o)
    for i in range(0, len(deferred), capi.EXT_BATCH):
        part = deferred[i:i + capi.EXT_BATCH]
        steps.append((capi.STEP_SCAN_SET, len(part)) + tuple(part + [0] * (capi.EXT_BATCH - len(part))))
    return steps, seen


def check_invariants(capi, steps, n, L, block_first=None):
    """Every level 1..L-1 of every octave produced exactly once, behind level l-1 of its octave; level 1 of octave o+1 behind
    level L-3 of octave o (whose launch writes level 0 of o+1); every octave scanned exactly once, behind its level L-1; a
    batched scan holds 1..PSX_EXT_BATCH octaves.  block_first: the TILE steps (as one block, at the last one's position:
    psx_tile_selfcheck orders its inside) or the FLOW step produce every level of the octaves from there on."""
    made, scanned = {}, {}
    block = max([i for i, s in enumerate(steps) if s[0] in (capi.STEP_TILE, capi.STEP_FLOW)], default=None)
    assert (block is None) == (block_first is None)
    if block is not None:
        made = {(o, l): block for o in range(block_first, n) for l in range(1, L)}
    for i, (kind, cnt, a, b, c, d) in enumerate(steps):
        planes = {capi.STEP_BLUR: [(a, b)], capi.STEP_BLUR2: [(a, b), (c, d)]}.get(kind, [])
        for p in planes:
            assert p not in made and 0 <= p[0] < n and 1 <= p[1] < L, (i, p)
            made[p] = i
        octs = [a] if kind == capi.STEP_SCAN else [a, b, c, d][:cnt] if kind == capi.STEP_SCAN_SET else []
        if kind == capi.STEP_SCAN_SET:
            assert 1 <= cnt <= capi.EXT_BATCH, (i, cnt)
        for o in octs:
            assert o not in scanned and 0 <= o < n, (i, o)
            scanned[o] = i
    assert sorted(made) == [(o, l) for o in range(n) for l in range(1, L)] and sorted(scanned) == list(range(n))
    behind = lambda later, earlier: made[later] > made[earlier] or (made[later] == made[earlier] == block and later[0] >= block_first and earlier[0] >= block_first)
    for o in range(n):
        assert all(behind((o, l), (o, l - 1)) for l in range(2, L)), o
        assert o + 1 == n or behind((o + 1, 1), (o, L - 3)), o
        assert scanned[o] > made[(o, L - 1)], o


def diagonal_cases(capi):
    out = [(w, h, kw) for w, h, kw in CASES]
    out.append((300, 200, dict(octaves=4, levels=1)))    # L = 4: three octaves active in one slot, the third launches alone
    out.append((1920, 1080, dict(octaves=5, levels=1)))
    # octaves 0 and 1 fit one round at the last level's span, so they overlap, and not at another: a slot refuses its pair
    out.append((1170, 877, dict(octaves=4, levels=1, upscale_factor=0.0)))
    return out


def test_diagonal_plan_is_the_restated_schedule(capi):
    seen_all = dict(pair=0, refused=0, odd=0)
    for w, h, kw in diagonal_cases(capi):
        cfg, sizes = octave_sizes(capi, w, h, kw)
        L = cfg.levels + 3
        spans = [int(v) for v in capi.gauss_tables(cfg)["inc_span"]]
        for resident in RESIDENT:
            want, seen = restate_diagonal(capi, sizes, L, spans, resident)
            got = capi.pyramid_plan(sizes[0][0], sizes[0][1], len(sizes), cfg.levels, spans, resident)
            assert [tuple(int(v) for v in s) for s in got] == want, (w, h, kw, resident)
            check_invariants(capi, want, len(sizes), L)
            # the launch count: one launch per step
            blurs = sum(1 for s in want if s[0] in (capi.STEP_BLUR, capi.STEP_BLUR2))
            assert blurs == len(sizes) * (L - 1) - seen["pair"]
            if resident == 1 << 20:
                assert seen["refused"] == 0 and not any(s[0] == capi.STEP_SCAN for s in want)
                assert sum(s[1] for s in want if s[0] == capi.STEP_SCAN_SET) == len(sizes)
            for k in seen:
                seen_all[k] += seen[k]
    # every branch of the slot walk was taken by some case: a shared launch, a refused pair (two launches), and a plane
    # that launches alone beside others
    assert seen_all["pair"] > 0 and seen_all["refused"] > 0 and seen_all["odd"] > 0, seen_all


def test_default_1080p_plan_counts(capi):
    """1080p, default configuration, MI355X: 19 blur launches instead of 25, octaves 0 and 1 scanned by
    launches of their own, the other three in one."""
    cfg, sizes = octave_sizes(capi, 1920, 1080, dict(octaves=5))
    spans = [int(v) for v in capi.gauss_tables(cfg)["inc_span"]]
    got = capi.pyramid_plan(sizes[0][0], sizes[0][1], 5, 3, spans)
    kinds = [int(s[0]) for s in got]
    assert kinds.count(capi.STEP_BLUR) + kinds.count(capi.STEP_BLUR2) == 19 and kinds.count(capi.STEP_BLUR2) == 6
    assert [tuple(int(v) for v in s) for s in got if s[0] in (capi.STEP_SCAN, capi.STEP_SCAN_SET)] == [
        (capi.STEP_SCAN, 0, 0, 0, 0, 0), (capi.STEP_SCAN, 0, 1, 0, 0, 0), (capi.STEP_SCAN_SET, 3, 2, 3, 4, 0)]


FLOW_SHAPES = [(3840, 2160, 5, 0), (3840, 2160, 5, 1), (8192, 8192, 6, 0), (1280, 960, 5, 0), (640, 480, 4, 0), (150, 122, 3, 0),
               (64, 64, 2, 0), (4097, 33, 3, 0), (9, 3000, 4, 0), (2, 2, 1, 0), (1, 128, 2, 0), (667, 503, 4, 1)]
TILE_SHAPES = [(3840, 2160, 5, 3), (8192, 8192, 6, 3), (1280, 960, 5, 3), (640, 480, 4, 3), (150, 122, 3, 3), (64, 64, 2, 3),
               (4097, 33, 3, 3), (9, 3000, 4, 3), (2, 2, 1, 3), (1, 128, 2, 3), (667, 503, 4, 2), (667, 503, 4, 4), (1280, 960, 5, 5)]


@pytest.mark.parametrize("resident", RESIDENT)
def test_flow_plans_keep_the_order(capi, resident):
    """tests/test_capi_cpu.py's flow shapes: octave 0 by launches when the work list starts at octave 1, ONE flow step, then
    the scans of every octave in order (psx_find_extrema issues them)."""
    spans = [int(v) for v in capi.gauss_tables(capi.default_config())["inc_span"]]
    for w0, h0, n, first in FLOW_SHAPES:
        got = [tuple(int(v) for v in s) for s in capi.pyramid_plan(w0, h0, n, 3, spans, resident, capi.PLAN_FLOW, first)]
        check_invariants(capi, got, n, 6, block_first=first)
        head = [(capi.STEP_BLUR, 0, 0, l, 0, 0) for l in range(1, 6)] if first else []
        assert got[:len(head) + 1] == head + [(capi.STEP_FLOW, 0, 0, 0, 0, 0)]
        assert all(s[0] in (capi.STEP_SCAN, capi.STEP_SCAN_SET) for s in got[len(head) + 1:])
        order = [o for s in got if s[0] == capi.STEP_SCAN for o in [s[2]]] + [o for s in got if s[0] == capi.STEP_SCAN_SET for o in s[2:2 + s[1]]]
        tiles = lambda o: -(-((w0 + (1 << o) - 1) >> o) // 64) * -(-((h0 + (1 << o) - 1) >> o) // 16)
        assert order == [o for o in range(n) if tiles(o) >= resident] + [o for o in range(n) if tiles(o) < resident]


@pytest.mark.parametrize("resident", RESIDENT)
def test_tile_plans_keep_the_order(capi, resident):
    """tests/test_capi_cpu.py's tile shapes under the default tile tuning: the octaves in front of the first tiled one level
    by level, each followed by its scan or deferral, then one TILE step per launch of the schedule, then the other scans."""
    L_ = capi.lib()
    L_.psx_tile_selfcheck.argtypes = [C.c_int] * 4 + [C.POINTER(C.c_int)] + [C.c_int] * 2 + [C.c_longlong, C.POINTER(C.c_int)]
    tiled = 0
    for w0, h0, n, levels in TILE_SHAPES:
        spans = [int(v) for v in capi.gauss_tables(capi.default_config(levels=levels))["inc_span"]]
        stats = (C.c_int * 4)()
        njobs = L_.psx_tile_selfcheck(w0, h0, n, levels, (C.c_int * capi.GAUSS_LEVELS)(*spans), 64, 1024, 3 << 20, stats)
        got = capi.pyramid_plan(w0, h0, n, levels, spans, resident, capi.PLAN_TILE)
        assert (got is None) == (njobs == 0), (w0, h0, n, levels)
        if got is None:
            continue
        tiled += 1
        got = [tuple(int(v) for v in s) for s in got]
        first, launches = stats[0], stats[1]
        check_invariants(capi, got, n, levels + 3, block_first=first)
        assert [s[2] for s in got if s[0] == capi.STEP_TILE] == list(range(launches))
        at = [i for i, s in enumerate(got) if s[0] == capi.STEP_TILE]
        assert at == list(range(at[0], at[0] + launches))
        assert [s[2:4] for s in got[:at[0]] if s[0] == capi.STEP_BLUR] == [(o, l) for o in range(first) for l in range(1, levels + 3)]
        assert not any(s[0] in (capi.STEP_BLUR2, capi.STEP_FLOW) for s in got)
        assert all(s[0] in (capi.STEP_SCAN, capi.STEP_SCAN_SET) for s in got[at[-1] + 1:])
    assert tiled >= 8


def test_plan_entry_checks_its_arguments(capi):
    L_ = capi.lib()
    spans = (C.c_int * capi.GAUSS_LEVELS)(*[int(v) for v in capi.gauss_tables(capi.default_config())["inc_span"]])
    n = C.c_int(-7)
    buf = np.full((4, 6), -7, np.int32)                                                     # room for three steps is offered
    call = lambda *a: L_.psx_pyramid_plan(*a)
    ok = (640, 480, 4, 3, spans, 1024, capi.PLAN_DIAGONAL, 0)
    assert call(*ok, buf.ctypes.data_as(C.c_void_p), 3, C.byref(n)) == 0 and n.value > 4      # the total; three steps written
    assert np.all(buf[:3, 0] == capi.STEP_BLUR) and np.all(buf[:3, 3] == [1, 2, 3]) and np.all(buf[3] == -7)
    for bad in [(0, 480, 4, 3, spans, 1024, 0, 0), (640, 480, 0, 3, spans, 1024, 0, 0), (640, 480, capi.MAX_OCTAVES + 1, 3, spans, 1024, 0, 0),
                (640, 480, 4, 0, spans, 1024, 0, 0), (640, 480, 4, capi.GAUSS_LEVELS - 2, spans, 1024, 0, 0), (640, 480, 4, 3, None, 1024, 0, 0),
                (640, 480, 4, 3, spans, 0, 0, 0), (640, 480, 4, 3, spans, 1024, 3, 0), (640, 480, 4, 3, spans, 1024, capi.PLAN_FLOW, 2),
                (640, 480, 1, 3, spans, 1024, capi.PLAN_FLOW, 1)]:
        assert call(*bad, None, 0, C.byref(n)) == -1, bad[:4] + bad[5:]
    assert call(*ok, None, 4, C.byref(n)) == -1 and call(*ok, None, -1, C.byref(n)) == -1 and call(*ok, None, 0, None) == -1
    assert L_.psx_blur_grid_of(0, 4, 6) == -1 and L_.psx_blur_grid_of(64, 64, 0) == -1 and capi.blur_grid(64, 64, 6) >= 1
