"""GPU tests of the DEVICE copies of the rules host and device share (csrc/hip/guide_rule.h, match_rule.h, kp_place.h) and of
the walk around the guide rule (k_match_guided, both formats, both directions), on the inputs of tests/rule_edge_cases.py:
probes one to six float32 steps from the guide's comparison, special values and subnormals with the whole relation
observed, ballot steps whose set bits are chosen one by one, exact ties, quotients on the ratio, keypoint records on the
placement tables.  The premises of those inputs are asserted in tests/test_rule_edges_cpu.py.  Every comparison is bit for
bit: indices, and distances as their 32-bit patterns; there is no tolerance anywhere in this module."""
import ctypes as C
import faulthandler

import numpy as np
import pytest

from popsift_amd.synth import synth
from tests import guided_cases as gc
from tests import rule_edge_cases as rc
from tests.match_pairs_cases import INT_MAX, same_records
from tests.test_keypoints_cpu import octave_dims

pytestmark = pytest.mark.gpu

INF = float("inf")


@pytest.fixture(autouse=True)
def watchdog():
    """a step that does not come back ends the process: nothing more is started on the GPU"""
    faulthandler.dump_traceback_later(300, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _bits(d):
    d = np.ascontiguousarray(d)
    return d.view(np.uint32) if d.dtype == np.float32 else d


def _same_directed(got, want):
    return (got[0].dtype == want[0].dtype and got[1].dtype == want[1].dtype and np.array_equal(got[0], want[0])
            and np.array_equal(_bits(got[1]), _bits(want[1])))


def _where(got, want):
    bad = np.flatnonzero((got[0] != want[0]).any(1) | (_bits(got[1]) != _bits(want[1])).any(1))
    return len(bad), [(int(i), got[0][i].tolist(), got[1][i].tolist(), want[0][i].tolist(), want[1][i].tolist()) for i in bad[:4]]


class _Dev:
    """two descriptor sets and their positions uploaded once; guided and unguided calls on them, or on row ranges of them"""

    def __init__(self, capi, left, lxy, right, rxy):
        self.capi, self.L, self.bufs = capi, capi.lib(), []
        self.u8 = left.dtype == np.uint8
        assert right.dtype == left.dtype and left.dtype in (np.uint8, np.float32)
        self.left, self.right = np.ascontiguousarray(left).reshape(-1, 128), np.ascontiguousarray(right).reshape(-1, 128)
        self.lxy, self.rxy = np.ascontiguousarray(lxy, np.float32).reshape(-1, 2), np.ascontiguousarray(rxy, np.float32).reshape(-1, 2)
        assert len(self.lxy) == len(self.left) and len(self.rxy) == len(self.right)
        self.pl, self.plx, self.pr, self.prx = capi._to_device(self.L, 0, [self.left, self.lxy, self.right, self.rxy], self.bufs)
        self.dtype = capi.PAIR_U8_DTYPE if self.u8 else capi.PAIR_DTYPE
        self.row = 128 * self.left.itemsize

    def _side(self, p, px, n, rng):
        if rng is None:
            return p, px, n
        a, b = rng
        assert 0 <= a <= b <= n
        return C.c_void_p(p.value + a * self.row), C.c_void_p(px.value + a * 8), b - a

    def directed(self, guide, lrange=None, rrange=None):
        pl, plx, nl = self._side(self.pl, self.plx, len(self.left), lrange)
        pr, prx, nr = self._side(self.pr, self.prx, len(self.right), rrange)
        fn = self.L.psx_match_guided_u8 if self.u8 else self.L.psx_match_guided
        mm = np.full((nl, 3), -9, np.int32)
        dd = np.full((nl, 2), -9, np.int32 if self.u8 else np.float32)
        rc_ = fn(0, pl, plx, nl, pr, prx, nr, C.byref(guide), mm.ctypes.data_as(C.c_void_p), dd.ctypes.data_as(C.c_void_p))
        assert rc_ == 0
        return mm, dd

    def unguided(self):
        fn = self.L.psx_match_u8 if self.u8 else self.L.psx_match
        fn.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        mm = np.full((len(self.left), 3), -9, np.int32)
        dd = np.full((len(self.left), 2), -9, np.int32 if self.u8 else np.float32)
        assert fn(0, self.pl, len(self.left), self.pr, len(self.right), mm.ctypes.data_as(C.c_void_p), dd.ctypes.data_as(C.c_void_p)) == 0
        return mm, dd

    def pairs(self, guide, ratio, mutual):
        """guide None: psx_match_pairs / _u8"""
        if guide is None:
            fn = self.L.psx_match_pairs_u8 if self.u8 else self.L.psx_match_pairs
            name = "pairs"
        else:
            fn = self.capi._guided_fn(self.L.psx_match_pairs_guided_u8 if self.u8 else self.L.psx_match_pairs_guided, self.plx, self.prx, guide)
            name = "guided pairs"
        return self.capi._pairs_call(fn, name, 0, self.pl, len(self.left), self.pr, len(self.right), ratio, mutual, self.dtype, None)[0]

    def close(self):
        for p in self.bufs:
            self.L.psx_dev_free(0, p)
        self.bufs = []


# ---- 1. the guide rule at its comparison ------------------------------------------------------------------------------------
@pytest.mark.parametrize("u8", [True, False], ids=["bytes", "float"])
@pytest.mark.parametrize("guide", sorted(gc.GUIDES))
def test_probes_on_the_comparison(oracle, capi, guide, u8):
    """2048 probe rights one to six float32 steps from the boundary of their left point's admissible set (about half on
    either side; a contracted multiply-add decides several per cent of them differently): the forward directed result
    shows both probe decisions of every primary left, the mutual list at ratio inf every backward decision -- (i, probe) is
    kept iff both passes admit it, (fallback, probe) iff the backward pass rejects it."""
    s = rc.probe_set(guide)
    fm, fd, bm, bd = rc.expected(oracle, ("probe", guide), s["left"], s["right"], s["A"])[u8]
    if u8:
        wm, wd = gc.expect_bytes_int64(s["left"], s["right"], s["A"])
        assert np.array_equal(wm, fm) and np.array_equal(wd, fd)
    g = capi.Guide.make(s["kind"], s["m"], s["tol"])
    dev = _Dev(capi, rc.as_format(s["left"], u8), s["lxy"], rc.as_format(s["right"], u8), s["rxy"])
    try:
        got = dev.directed(g)
        assert _same_directed(got, (fm, fd)), _where(got, (fm, fd))
        for ratio in (INF, 0.8):
            for mutual in (True, False):
                want = capi.pairs_join(fm, fd, bm if mutual else None, len(s["right"]), ratio, mutual)
                got = dev.pairs(g, ratio, mutual)
                assert len(want) > 500 and same_records(got, want), (ratio, mutual, len(got), len(want))
    finally:
        dev.close()
    wrap = capi.match_guided_u8 if u8 else capi.match_guided
    sel = slice(0, 64)
    got = wrap(rc.as_format(s["left"][sel], u8), s["lxy"][sel], rc.as_format(s["right"], u8), s["rxy"], g)
    assert _same_directed(got, (fm[sel], fd[sel]))


@pytest.mark.parametrize("u8", [True, False], ids=["bytes", "float"])
def test_special_values_forward(capi, u8):
    """NaN, +-inf, overflow, c <= 0, degenerate lines, subnormal matrix entries and subnormal c: the device's WHOLE forward
    relation on 33 x 44 points -- the right side cut into slices of two rows at distances 1 and 2 from every left row, so
    indices and +inf distances say exactly which of the two were admitted -- equals the restatement, entry for entry"""
    lxy, rxy = rc.special_points()
    nl, nr = len(lxy), len(rxy)
    left = rc.as_format(np.tile(rc.SLICE_BASE, (nl, 1)), u8)
    right = rc.as_format(rc.slice_rows(nr), u8)
    dev = _Dev(capi, left, lxy, right, rxy)
    outcomes = set()
    try:
        for kind, m, tol in rc.special_guides():
            A = gc.restate(kind, m, tol, lxy, rxy)
            g = capi.Guide.make(kind, m, tol)
            seen = np.zeros_like(A)
            for s in range(0, nr, 2):
                got = dev.directed(g, rrange=(s, s + 2))
                want = rc.slice_expect(A[:, s:s + 2], u8)
                assert _same_directed(got, want), (kind, list(m), tol, s, _where(got, want))
                # the relation itself, read off the result
                one = 1 if u8 else np.float32(1)
                seen[:, s] = got[1][:, 0] == one
                seen[:, s + 1] = (got[1][:, 0] == 2 * one) | (got[1][:, 1] == 2 * one)
            assert np.array_equal(seen, A), (kind, list(m), tol)
            outcomes.add((bool(A.any()), bool((~A).any())))
    finally:
        dev.close()
    assert (True, True) in outcomes and (False, True) in outcomes


@pytest.mark.parametrize("u8", [True, False], ids=["bytes", "float"])
def test_special_values_backward(capi, u8):
    """the same guides through the BACKWARD pass (k_guide_lines, then k_match_guided with the loops exchanged): one mutual
    call per guide on the diagonal set -- pair k of the 33 x 44 is kept iff both passes admit it, its fallback iff the backward
    pass rejects it (tests/rule_edge_cases.diagonal_set)"""
    total = 0
    for kind, m, tol in rc.special_guides():
        d = rc.diagonal_set(kind, m, tol)
        n = len(d["right"])
        fm, fd = rc.top2(d["D"], d["A"], u8)
        bm, _ = rc.top2(d["D"].T, d["A"].T, u8)
        want = capi.pairs_join(fm, fd, bm, n, INF, True)
        fn = capi.match_pairs_guided_u8 if u8 else capi.match_pairs_guided
        got = fn(rc.as_format(d["left"], u8), d["lxy"], rc.as_format(d["right"], u8), d["rxy"], capi.Guide.make(kind, m, tol), INF, True)
        assert same_records(got, want), (kind, list(m), tol, len(got), len(want))
        total += len(want)
    assert total > 5000


# ---- 2. the walk around the rule --------------------------------------------------------------------------------------------
def _walk_check(oracle, capi, c, u8, what):
    g = capi.Guide.homography(gc.IDENTITY, rc.WALK_TOL)
    outer, inner, P = rc.as_format(c["outer"], u8), rc.as_format(c["inner"], u8), c["pattern"]
    fm, fd, bm, bd = rc.expected(oracle, what, c["outer"], c["inner"], P)[u8]
    if u8:
        wm, wd = gc.expect_bytes_int64(c["outer"], c["inner"], P)
        assert np.array_equal(wm, fm) and np.array_equal(wd, fd)
    # forward: the outer descriptors are the left side
    dev = _Dev(capi, outer, c["oxy"], inner, c["ixy"])
    try:
        got = dev.directed(g)
        assert _same_directed(got, (fm, fd)), (what, _where(got, (fm, fd)))
        assert same_records(dev.pairs(g, INF, True), capi.pairs_join(fm, fd, bm, len(inner), INF, True)), what
    finally:
        dev.close()
    # backward: the loops exchanged -- the outer descriptors are the RIGHT side of a mutual call, the walk runs over lefts
    dev = _Dev(capi, inner, c["ixy"], outer, c["oxy"])
    try:
        want = capi.pairs_join(bm, bd, fm, len(outer), INF, True)
        assert len(want) >= 1 and same_records(dev.pairs(g, INF, True), want), what
        got = dev.directed(g)
        assert _same_directed(got, (bm, bd)), (what, _where(got, (bm, bd)))
    finally:
        dev.close()


@pytest.mark.parametrize("u8", [True, False], ids=["bytes", "float"])
@pytest.mark.parametrize("i_len", rc.WALK_LENGTHS)
def test_walk_set_bits(oracle, capi, i_len, u8):
    """1 .. 9, 63 and 64 set bits per 64-point step, at lanes 0 / 31 / 32 / 63, as runs straddling lane 32, in the first, a
    middle or the last (partial) step alone, a set bit in the last valid lane: every set bit is the nearest of some outer
    descriptor and a row outside the pattern would win if it were taken"""
    for k, c in enumerate(rc.walk_calls(i_len)):
        _walk_check(oracle, capi, c, u8, ("walk", i_len, k))


@pytest.mark.parametrize("u8", [True, False], ids=["bytes", "float"])
def test_walk_exact_ties(oracle, capi, u8):
    """two and three identical rows admissible for one descriptor -- in one round and half, one round and both halves, two
    rounds of a step, two steps; best tied, second tied, all three tied: the smaller index wins, then the next smaller;
    forward (tie among rights) and with the loops exchanged (tie among lefts)"""
    _walk_check(oracle, capi, rc.tie_call(), u8, ("ties",))


def test_walk_skips_nan_and_overflowing_rows(oracle, capi):
    """float only: an admissible inner row that holds a NaN, or whose distance overflows to +inf, is never a neighbour (the
    reference's strict '<' scan: oracle.match on the admissible subset)"""
    g = capi.Guide.homography(gc.IDENTITY, rc.WALK_TOL)
    for rows, b, s, d1, d2 in rc.nonfinite_calls():
        inner = np.stack(rows).astype(np.float32)
        outer = np.full((1, 128), 50, np.float32)
        with np.errstate(all="ignore"):
            om, od = oracle.match(outer, inner)
        assert om[0, :2].tolist() == [b, s]
        mm, dd = capi.match_guided(outer, np.zeros((1, 2), np.float32), inner, np.zeros((len(inner), 2), np.float32), g)
        assert np.array_equal(mm, om) and np.array_equal(_bits(dd), _bits(od)), (mm, dd, om, od)
        assert dd[0].tolist() == [d1, d2]
        # the loops exchanged: the rows are lefts, ranked by the one right row
        left_xy = np.zeros((len(inner), 2), np.float32)
        got = capi.match_pairs_guided(inner, left_xy, outer, np.zeros((1, 2), np.float32), g, INF, True)
        if np.isfinite(d1):
            assert got["left"].tolist() == [b] and got["right"].tolist() == [0] and got["d1"].tolist() == [d1]
        else:
            assert len(got) == 0


# ---- 3. the ratio rule at its quotient --------------------------------------------------------------------------------------
@pytest.mark.parametrize("u8", [True, False], ids=["bytes", "float"])
def test_ratio_on_the_quotient(capi, u8):
    """left rows with exactly known integer (d1, d2); every ratio on a quotient and one float32 step either side of it, 0.8f
    and inf; psx_match_pairs* and psx_match_pairs_guided* under an all-admitting guide, with and without the cross-check,
    against numpy float32 division and '<'; the accept flag of the four directed matchers (4 k / 5 k is exactly 0.8f:
    rejected)"""
    s = rc.ratio_set()
    n = len(s["left"])
    all_ok = np.ones((n, 2 * n), bool)
    fm, fd = gc.expect_bytes_int64(s["left"], s["right"], all_ok)
    bm, _ = gc.expect_bytes_int64(s["right"], s["left"], all_ok.T)
    assert np.array_equal(fd, np.stack([s["d1"], s["d2"]], 1))
    if not u8:
        fd = np.where(fd == INT_MAX, np.inf, fd).astype(np.float32)
    ratios = rc.ratios_around(rc.quotients(s["d1"], s["d2"]))
    rng = np.random.default_rng(3)
    lxy, rxy = rng.uniform(0, 500, (n, 2)).astype(np.float32), rng.uniform(0, 500, (2 * n, 2)).astype(np.float32)
    g = capi.Guide.homography(gc.IDENTITY, 1e30)
    assert gc.restate(gc.HOMOGRAPHY, gc.IDENTITY, 1e30, lxy, rxy).all()
    dev = _Dev(capi, rc.as_format(s["left"], u8), lxy, rc.as_format(s["right"], u8), rxy)
    try:
        for got in (dev.unguided(), dev.directed(g)):
            assert _same_directed(got, (fm, fd)), _where(got, (fm, fd))
        k45 = np.flatnonzero((s["d1"] * 5 == s["d2"] * 4) & (s["d1"] > 0))
        assert len(k45) >= 9 and (fm[k45, 2] == 0).all()
        for ratio in ratios:
            for mutual in (False, True):
                want = rc.keep_reference(fm, fd, bm, ratio, mutual, dev.dtype)
                for guide in (None, g):
                    got = dev.pairs(guide, ratio, mutual)
                    assert same_records(got, want), (ratio, mutual, guide is not None, len(got), len(want))
        # one neighbour only: d2 = +inf, the quotient is 0 and passes every ratio
        tiny = float(np.nextafter(np.float32(0), np.float32(1)))
        mm, dd = dev.directed(g, rrange=(0, 1))
        assert (mm[:, 2] == 1).all() and (mm[:, :2] == 0).all() and (dd[:, 1] == (INT_MAX if u8 else np.float32(np.inf))).all()
        one = _Dev(capi, dev.left, lxy, dev.right[:1], rxy[:1])
        try:
            for guide in (None, g):
                for ratio in (tiny, 0.8, INF):
                    got = one.pairs(guide, ratio, False)
                    assert len(got) == n and (got["right"] == 0).all() and np.array_equal(got["left"], np.arange(n))
                    assert (got["d2"] == (INT_MAX if u8 else np.float32(np.inf))).all()
            assert (one.unguided()[0][:, 2] == 1).all()
        finally:
            one.close()
    finally:
        dev.close()


# ---- 4. keypoint placement at its tables ------------------------------------------------------------------------------------
@pytest.mark.parametrize("up", [1.0, 0.0], ids=["upscale1", "upscale0"])
def test_keypoint_placement_on_the_tables(capi, up):
    """sigma on every b_l, on sigma_min / sigma_max in octave units and on the octave hand-over, positions on 0, w_o - 1 and
    h_o - 1, each with its float32 neighbours, automatic and explicit: k_kp_classify / k_kp_scatter accept, reject and place
    record for record as psx_place_keypoints does"""
    w, h, cap = 320, 240, 16384
    cfg = capi.default_config(octaves=3, upscale_factor=up, max_extrema=cap)
    ctx = capi.Context(cfg)
    try:
        ctx.upload(synth(w, h, 4))
        auto, explicit = rc.boundary_records(capi, cfg, w, h)
        dims = octave_dims(cfg, w, h, 3)
        lists = [auto, explicit, rc.position_edge_records(capi, cfg, dims)]
        for k, recs in enumerate(lists):
            ho, hl = capi.place_keypoints(cfg, w, h, recs)
            want = np.concatenate([np.flatnonzero(ho == o) for o in range(3)])
            assert max(int((ho == o).sum()) for o in range(3)) <= cap
            ctx.set_keypoints(recs)
            ctx.describe()
            assert ctx.num_octaves == 3 and [ctx.octave_dims(o) for o in range(3)] == dims
            F, D = ctx.download()
            src = ctx.keypoint_map()
            ne, no = ctx.counts()
            print("upscale %g, list %d: %d records, %d accepted, %d rejected" % (up, k, len(recs), ne, len(recs) - ne))
            assert ne == len(want) == len(F) and len(recs) - ne == int((ho < 0).sum())
            assert np.array_equal(src, want)
            assert np.array_equal(F["debug_octave"], ho[want])
            ext = ctx.dump_extrema()
            assert np.array_equal(ext["lpos"], hl[want]) and np.array_equal(ext["octave"], ho[want])
            for name in ("xpos", "ypos", "sigma"):                          # reported in image units: the record's own bits
                v = recs[name][want]                                         # (a subnormal does not survive the change of units)
                ok = (v == 0) | (np.abs(v) > 1e-30)
                assert F[name][ok].tobytes() == v[ok].tobytes(), name
            assert len(want) > 100 and (ho < 0).sum() > 30
    finally:
        ctx.close()
