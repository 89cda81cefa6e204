"""CPU tests of tests/rule_edge_cases.py: the PREMISES of its constructions -- conditions on the inputs, from the numpy
restatements alone -- and the host copies of the shared rules (psx_guide_allows, psx_pairs_join, psx_place_keypoints) on
them.  tests/test_gpu_rule_edges.py holds the device copies to the same expectations, bit for bit."""
import numpy as np
import pytest

from tests import guided_cases as gc
from tests import rule_edge_cases as rc
from tests.match_pairs_cases import INT_MAX, dist_as_int, same_records
from tests.test_keypoints_cpu import octave_dims, restate as kp_restate

INF = float("inf")


# ---- 1. probe sets ----------------------------------------------------------------------------------------------------------
def _probe_entries(s):
    i = np.repeat(s["prim"], 2)
    return i, s["probe"].reshape(-1), s["fall"].reshape(-1)


@pytest.mark.parametrize("guide", sorted(gc.GUIDES))
def test_probe_sets_sit_on_the_comparison(capi, guide):
    """(a) 35 % .. 65 % of the probes are admitted; (b) the contracted restatement decides at least 2 % of them
    differently, and so does '<' in place of '<=' somewhere; (d) psx_guide_allows equals the restatement on the whole set;
    every fallback firmly admits its probe"""
    s = rc.probe_set(guide)
    i, j, f = _probe_entries(s)
    adm = s["A"][i, j]
    frac = adm.mean()
    con = rc.restate_contracted(s["kind"], s["m"], s["tol"], s["lxy"], s["rxy"])
    flips = (con[i, j] != adm).mean()
    print("%s: %d probes, %.1f %% admitted, %.1f %% decided differently under contraction" % (guide, len(i), 100 * frac, 100 * flips))
    assert len(i) == 2 * rc.PROBE_N and 0.35 <= frac <= 0.65
    assert flips >= 0.02
    assert s["A"][f, j].all() and con[f, j].all()
    got = capi.guide_allows(capi.Guide.make(s["kind"], s["m"], s["tol"]), s["lxy"], s["rxy"])
    assert np.array_equal(got, s["A"])


@pytest.mark.parametrize("guide", sorted(gc.GUIDES))
def test_probe_decisions_are_visible(oracle, capi, guide):
    """(c) for every probe entry, flipping that one entry of the relation changes the expected forward directed row, the
    expected mutual pair list, and the list again when only the backward pass sees the flip; and the descriptor premises:
    the probes are the two nearest rights of their primary at small distinct distances, the bytes' expectation equals
    integer arithmetic"""
    s = rc.probe_set(guide)
    left, right, A = s["left"], s["right"], s["A"]
    nr = len(right)
    ex = rc.expected(oracle, ("probe", guide), left, right, A)
    fm, fd, bm, bd = ex[True]
    wm, wd = gc.expect_bytes_int64(left, right, A)
    assert np.array_equal(fm, wm) and np.array_equal(fd, wd)
    wm, wd = gc.expect_bytes_int64(right, left, A.T)
    assert np.array_equal(bm, wm) and np.array_equal(bd, wd)
    assert np.array_equal(rc.top2(rc.int_distances(left, right), A, True)[0], fm)
    um, ud = gc.expect_bytes_int64(left[s["prim"]], right, np.ones((len(s["prim"]), nr), bool))
    assert np.array_equal(um[:, :2], s["probe"]) and np.array_equal(ud, np.stack([s["da"], s["db"]], 1))
    assert (s["da"] < s["db"]).all() and s["db"].max() < 20
    base = capi.pairs_join(fm, fd, bm, nr, INF, True)
    i, j, f = _probe_entries(s)
    assert np.array_equal(fm[f, 0], j)                                     # a fallback's best is its probe
    for a, b in zip(i, j):
        row = A[a].copy()
        row[b] = not row[b]
        col = A[:, b].copy()
        col[a] = not col[a]
        m1, d1 = gc.expect_directed(oracle, left[a:a + 1], right, row[None, :], True)
        m2, _ = gc.expect_directed(oracle, right[b:b + 1], left, col[None, :], True)
        assert not (np.array_equal(m1[0], fm[a]) and np.array_equal(d1[0], fd[a])), (a, b)
        fm2, fd2, bm2 = fm.copy(), fd.copy(), bm.copy()
        fm2[a], fd2[a], bm2[b] = m1[0], d1[0], m2[0]
        assert not same_records(capi.pairs_join(fm2, fd2, bm2, nr, INF, True), base), (a, b)
        assert not same_records(capi.pairs_join(fm, fd, bm2, nr, INF, True), base), (a, b, "backward alone")


# ---- 1. special values ------------------------------------------------------------------------------------------------------
def test_special_guides_on_the_host(capi):
    lxy, rxy = rc.special_points()
    assert lxy.shape == (33, 2) and rxy.shape == (44, 2)
    flushed_differs = 0
    for kind, m, tol in rc.special_guides():
        g = capi.Guide.make(kind, m, tol)
        want = gc.restate(kind, m, tol, lxy, rxy)
        assert np.array_equal(capi.guide_allows(g, lxy, rxy), want), (kind, list(m), tol)
    for kind, m, tol in rc.SUBNORMAL_GUIDES:
        assert any(0 < abs(float(np.float32(v))) < 1.1754944e-38 for v in m) or kind == gc.HOMOGRAPHY
        want = gc.restate(kind, m, tol, lxy, rxy)
        # what flushing subnormal inputs and results to zero would give: the guide's entries and c
        ftz = lambda v: np.where(np.abs(v) < np.float32(1.1754944e-38), np.float32(0), v).astype(np.float32)
        mz = ftz(np.asarray(m, np.float32))
        flushed = gc.restate(kind, mz, tol, ftz(lxy), ftz(rxy))
        flushed_differs += int(not np.array_equal(flushed, want))
        assert want.any() and not want.all()
    assert flushed_differs >= 3                                            # flushed denormals would show
    # c is subnormal for the appended left points under the 2^-110 guides
    m = np.asarray(rc.SUBNORMAL_GUIDES[2][1], np.float32)
    c = (m[6] * rc.SUBNORMAL_LEFTS[:, 0] + m[7] * rc.SUBNORMAL_LEFTS[:, 1]) + m[8]
    assert (np.abs(c[:3]) > 0).all() and (np.abs(c[:3]) < np.float32(1.1754944e-38)).all() and c[3] == 0


def test_special_value_constructions(oracle, capi):
    """forward slices: the four outcomes of a two-row slice are told apart; the diagonal set: top2 equals
    guided_cases.expect_directed, every pair whose column some left admits is decided by the list"""
    A2 = np.array([[0, 0], [1, 0], [0, 1], [1, 1]], bool)
    mm, dd = rc.slice_expect(A2, True)
    assert mm.tolist() == [[0, 0, 0], [0, 0, 1], [1, 0, 1], [0, 1, 1]]
    assert dd.tolist() == [[INT_MAX, INT_MAX], [1, INT_MAX], [2, INT_MAX], [1, 2]]
    rows = rc.slice_rows(44)
    em, ed = gc.expect_directed(oracle, np.tile(rc.SLICE_BASE, (4, 1)), rows[6:8], A2, True)
    assert np.array_equal(em, mm) and np.array_equal(ed, dd)
    seen_diag = seen_fall = 0
    for kind, m, tol in (rc.special_guides()[3], rc.special_guides()[7], rc.SUBNORMAL_GUIDES[2]):
        d = rc.diagonal_set(kind, m, tol)
        n = len(d["right"])
        assert d["left"].shape == (2 * n, 128) and n == 33 * 44
        fm, fd = rc.top2(d["D"], d["A"], True)
        bm, bd = rc.top2(d["D"].T, d["A"].T, True)
        sel = np.random.default_rng(1).choice(2 * n, 150, replace=False)
        em, ed = gc.expect_directed(oracle, d["left"][sel], d["right"], d["A"][sel], True)
        assert np.array_equal(em, fm[sel]) and np.array_equal(ed, fd[sel])
        sel = sel[sel < n]
        em, ed = gc.expect_directed(oracle, d["right"][sel], d["left"], d["A"].T[sel], True)
        assert np.array_equal(em, bm[sel]) and np.array_equal(ed, bd[sel])
        pairs = capi.pairs_join(fm, fd, bm, n, INF, True)
        kept = set(zip(pairs["left"].tolist(), pairs["right"].tolist()))
        a0 = d["A0"][d["ii"], d["jj"]]
        for k in range(n):
            has_other = d["fb"][k] != d["ii"][k]
            assert ((k, k) in kept) == bool(a0[k]), k
            if has_other:
                assert ((n + k, k) in kept) == (not a0[k]), k              # the backward decision of a REJECTED pair shows too
        seen_diag += int(a0.sum())
        seen_fall += int(sum((n + k, k) in kept for k in range(n)))
    assert seen_diag > 100 and seen_fall > 100


# ---- 2. the walk ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i_len", rc.WALK_LENGTHS)
def test_walk_patterns_are_what_the_rule_admits(capi, i_len):
    counts, lanes = set(), set()
    for c in rc.walk_calls(i_len):
        want = c["pattern"]
        assert np.array_equal(gc.restate(gc.HOMOGRAPHY, gc.IDENTITY, rc.WALK_TOL, c["oxy"], c["ixy"]), want)
        assert np.array_equal(gc.restate(gc.HOMOGRAPHY, gc.IDENTITY, rc.WALK_TOL, c["ixy"], c["oxy"]), want.T)
        assert np.array_equal(capi.guide_allows(capi.Guide.homography(gc.IDENTITY, rc.WALK_TOL), c["oxy"], c["ixy"]), want)
        assert c["inner"].shape == (i_len, 128) and want.any(1).all()
        for row in want:
            for s in range(0, i_len, 64):
                counts.add(int(row[s:s + 64].sum()))
            lanes |= set((np.flatnonzero(row) % 64).tolist())
    assert counts >= set(range(1, min(9, i_len) + 1)) and (i_len < 64 or {63, 64} <= counts) and (i_len < 63 or 63 in counts)
    assert i_len < 64 or {0, 31, 32, 63} <= lanes
    assert any(c["pattern"][:, i_len - 1].any() for c in rc.walk_calls(i_len))     # a set bit in the last valid lane
    if i_len == 129:
        steps = [set((np.flatnonzero(row) // 64).tolist()) for c in rc.walk_calls(i_len) for row in c["pattern"]]
        assert {0} in steps and {1} in steps and {2} in steps and {0, 1} in steps and {0, 2} in steps


def test_tie_and_nonfinite_cases(oracle, capi):
    c = rc.tie_call()
    assert np.array_equal(gc.restate(gc.HOMOGRAPHY, gc.IDENTITY, rc.WALK_TOL, c["oxy"], c["ixy"]), c["pattern"])
    fm, fd = gc.expect_directed(oracle, c["outer"], c["inner"], c["pattern"], True)
    for t, (ranks, scen) in enumerate(rc.TIE_CASES):
        members = np.flatnonzero(c["pattern"][t])
        assert len(members) == 8 and len(set(members // 64)) == 2
        copies = np.array([members[6] if r is None else members[r] for r in ranks])
        assert (c["inner"][copies] == c["inner"][copies[0]]).all()         # identical rows
        if scen == "best":
            assert fm[t, :2].tolist() == sorted(copies)[:2] and fd[t].tolist() == [4, 4]
        elif scen == "all":
            assert fm[t, :2].tolist() == sorted(copies)[:2] and fd[t].tolist() == [4, 4] and len(copies) == 3
        else:
            assert fm[t, 1] == copies.min() and fd[t].tolist() == [1, 4] and fm[t, 0] not in copies
    # float only: the oracle's strict '<' scan skips a NaN distance and a +inf distance
    for rows, b, s, d1, d2 in rc.nonfinite_calls():
        inner = np.stack(rows).astype(np.float32)
        outer = np.full((1, 128), 50, np.float32)
        with np.errstate(all="ignore"):
            m, d = oracle.match(outer, inner)
        assert (m[0, 0], m[0, 1]) == (b, s) and d[0].tolist() == [d1, d2], (m, d)
        if len(inner) >= 2:
            em, ed = gc.expect_directed(oracle, outer, inner, np.ones((1, len(inner)), bool), False)
            assert em[0, :2].tolist() == [b, s] and ed[0].tolist() == [d1, d2]
        dist = ((inner.astype(np.float64) - 50.0) ** 2).sum(1)
        assert np.isnan(dist).any() or (dist > 3.5e38).any()


# ---- 3. the ratio rule ------------------------------------------------------------------------------------------------------
def _ratio_expect(s):
    fm, fd = gc.expect_bytes_int64(s["left"], s["right"], np.ones((len(s["left"]), len(s["right"])), bool))
    bm, bd = gc.expect_bytes_int64(s["right"], s["left"], np.ones((len(s["right"]), len(s["left"])), bool))
    return fm, fd, bm


def test_ratio_sets_and_the_host_join(oracle, capi):
    s = rc.ratio_set()
    n = len(s["left"])
    fm, fd, bm = _ratio_expect(s)
    assert n > 200 and np.array_equal(fd, np.stack([s["d1"], s["d2"]], 1))               # exactly the planted distances
    assert np.array_equal(np.sort(fm[:, :2], 1), np.stack([2 * np.arange(n), 2 * np.arange(n) + 1], 1))
    om, od = oracle.match(s["left"].astype(np.float32), s["right"].astype(np.float32))
    assert np.array_equal(om[:, :2], fm[:, :2]) and np.array_equal(dist_as_int(od), fd)
    q = rc.quotients(fd[:, 0], fd[:, 1])
    ratios = rc.ratios_around(q)
    assert len(ratios) > 60 and np.isnan(q).sum() == 1 and (q == 1).sum() >= 3 and (q == 0).sum() >= 2
    assert (q == np.float32(0.8)).sum() == 9                                # 4 k / 5 k rounds to exactly 0.8f: rejected
    k45 = np.flatnonzero(s["d1"] * 5 == s["d2"] * 4)[:9]
    assert (fm[k45, 2] == 0).all()
    # the premise: on each finite quotient the three ratios give reject / reject / keep
    f1, f2 = fd[:, 0].astype(np.float32), fd[:, 1].astype(np.float32)
    mutated = 0
    for v in np.unique(q[np.isfinite(q)]):
        rows = q == v
        lo, hi = np.nextafter(v, np.float32(0)), np.nextafter(v, np.float32(INF))
        assert not (q[rows] < lo).any() and not (q[rows] < v).any() and (q[rows] < hi).all()
        for r in (lo, v, hi):                                              # a product in place of the quotient decides otherwise
            mutated += int(((f1[rows] < np.float32(r) * f2[rows]) != (q[rows] < np.float32(r))).sum())
    assert mutated >= 10
    for u8 in (True, False):
        d = fd if u8 else np.where(fd == INT_MAX, np.inf, fd).astype(np.float32)
        dtype = capi.PAIR_U8_DTYPE if u8 else capi.PAIR_DTYPE
        for ratio in ratios:
            for mutual in (False, True):
                want = rc.keep_reference(fm, d, bm, ratio, mutual, dtype)
                assert same_records(capi.pairs_join(fm, d, bm if mutual else None, 2 * n, ratio, mutual), want), (u8, ratio, mutual)
    # one neighbour only: d2 = +inf, the quotient is 0, kept at every ratio
    one = rc.keep_reference(np.zeros((n, 3), np.int32), np.stack([fd[:, 0], np.full(n, INT_MAX)], 1).astype(np.int32), None,
                            float(np.nextafter(np.float32(0), np.float32(1))), False, capi.PAIR_U8_DTYPE)
    assert len(one) == n


# ---- 4. keypoints -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("up", [1.0, 0.0])
def test_position_edge_records_on_the_host(capi, up):
    w, h = 320, 240
    cfg = capi.default_config(octaves=3, upscale_factor=up)
    dims = octave_dims(cfg, w, h, 3)
    recs = rc.position_edge_records(capi, cfg, dims)
    o_lib, l_lib = capi.place_keypoints(cfg, w, h, recs)
    o_np, l_np = kp_restate(capi, cfg, w, h, recs, 3)
    assert np.array_equal(o_lib, o_np) and np.array_equal(l_lib, l_np)
    assert (o_lib >= 0).sum() > 100 and (o_lib < 0).sum() > 30
    # one float32 step decides: the record ON w_o - 1 is accepted, its upper neighbour is not
    unit = np.float32(2.0 ** (0 - int(up)))
    on = np.flatnonzero((recs["octave"] == 0) & (recs["xpos"] == np.float32(dims[0][0] - 1) * unit))
    above = np.flatnonzero((recs["octave"] == 0) & (recs["xpos"] == np.nextafter(np.float32(dims[0][0] - 1), np.float32(INF)) * unit))
    assert len(on) and len(above) and (o_lib[on] == 0).all() and (o_lib[above] == -1).all()
    # sigma ON the octave hand-over b[levels] goes to the next octave, its lower neighbour stays
    b = capi.keypoint_bounds(cfg)
    auto = recs["octave"] == capi.KP_AUTO
    s0 = np.float32(b[-1]) * unit
    assert (o_lib[auto & (recs["sigma"] == s0)] == 1).all() and (o_lib[auto & (recs["sigma"] == np.nextafter(s0, np.float32(0)))] == 0).all()
