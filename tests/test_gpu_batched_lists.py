"""GPU tests that a STAR is an edge list: the one-to-many forms (psx_ransac_*_many, psx_match_pairs_guided_many_u8) and the
edge-list forms (psx_ransac_*_graph, psx_match_pairs_guided_graph_u8) run ONE batched driver each, so the star call and the
graph call on the same star -- sets [left, rights...], edges (0, k + 1) -- must return the same bytes: records, per-list
counts, total, psx_ransac_results and both layers.  Each is also held to something that is not device code (the host
reference psx_ransac_*_many_ref, the restatement of tests/guided_many_cases.py), so the pair cannot agree on a wrong answer.

Shapes, the smallest that can still go wrong: RANSAC lists of 0, min - 1, min, 256, 257 and 513 pairs (the gather's and the
compaction's 256-pair block and the score kernel's 512-pair block, each crossed by one), 65 hypotheses (one past a
64-hypothesis block), with and without the refit, a capacity inside the concatenation, and K = 1; the guided re-match with 257
left rows (one past a 256-row block) against right sets of 300, 0, 1 and 63 rows under a homography, an epipolar band (on
the empty set), PSX_GUIDE_NONE and an epipolar band, with and without the cross-check, a capacity inside the concatenation,
and K = 1."""
import numpy as np
import pytest
import torch        # noqa: F401  before the HIP library is loaded: torch brings a HIP runtime of its own and must initialise first

from tests import graph_chain_cases as gc
from tests import guided_many_cases as gm
from tests import ransac_many_cases as mc
from tests.guided_cases import EPIPOLAR, HOMOGRAPHY
from tests.ransac_cases import bits, same_records

pytestmark = pytest.mark.gpu

N, SEED = mc.CONFIGS[1]                                   # 65 hypotheses
assert N == 65


def _star_graph(n_rights):
    return [(0, k + 1) for k in range(n_rights)]


def _same_ransac(a, b, what):
    assert a["count"] == b["count"], what
    assert [bytes(r) for r in a["results"]] == [bytes(r) for r in b["results"]], what
    assert a["records"].tobytes() == b["records"].tobytes(), what
    assert np.array_equal(bits(a["models"]), bits(b["models"])) and np.array_equal(a["counts"], b["counts"]), what


@pytest.mark.parametrize("refit", [False, True], ids=["sample", "refit"])
@pytest.mark.parametrize("model", gc.MODELS)
def test_ransac_star_call_equals_graph_call_on_the_star(capi, model, refit):
    m = gc.MIN[model]
    sizes = (0, m - 1, m, 256, 257, 513)
    c = mc.case("fundamental" if model == "fundamental" else "homography", SEED, sizes=sizes)
    opts = capi.ransac_opts(gc.TOL, N, SEED, refit)
    many, graph, ref = (getattr(capi, "ransac_%s_%s" % (model, form)) for form in ("many", "graph", "many_ref"))
    xys, edges = [c["left_xy"]] + list(c["right_xys"]), _star_graph(len(sizes))
    want = ref(c["lists"], c["left_xy"], c["right_xys"], opts, layers=True)
    star = many(c["lists"], c["left_xy"], c["right_xys"], opts, layers=True)
    over = graph(c["lists"], edges, xys, opts, layers=True)
    _same_ransac(star, over, "star / graph")
    _same_ransac(star, want, "star / host reference")
    total = star["count"]
    assert total == sum(r.inliers for r in star["results"]) and all(r.inliers >= 40 for r in want["results"][3:])   # the plant is found
    assert [r.best >= 0 for r in star["results"]] == [n >= m for n in sizes]
    assert star["models"].shape == (len(sizes), N, 9) and not star["models"][:2].any() and not star["counts"][:2].any()
    # a capacity inside the concatenation: the total is reported, the prefix written
    cap = total - star["results"][-1].inliers // 2
    cut_s = many(c["lists"], c["left_xy"], c["right_xys"], opts, capacity=cap, layers=True)
    cut_g = graph(c["lists"], edges, xys, opts, capacity=cap, layers=True)
    _same_ransac(cut_s, cut_g, "star / graph, truncated")
    assert cut_s["count"] == total and len(cut_s["records"]) == cap and same_records(cut_s["records"], star["records"][:cap])
    assert [bytes(r) for r in cut_s["results"]] == [bytes(r) for r in star["results"]]
    # K = 1
    one_s = many(c["lists"][4:5], c["left_xy"], c["right_xys"][4:5], opts, layers=True)
    one_g = graph(c["lists"][4:5], [(0, 1)], [c["left_xy"], c["right_xys"][4]], opts, layers=True)
    _same_ransac(one_s, one_g, "K = 1")
    assert bytes(one_s["results"][0]) == bytes(star["results"][4]) and one_s["count"] == star["results"][4].inliers > 0


# the guided star: 257 left rows against right sets of 300, 0, 1 and 63 rows -- the longest first, because the canvas of
# guided_many_cases.positioned_many is sized by set 0 (about 2.5 admissible right points per left point under its homography).
# Set 0 takes its own homography; the empty set has a valid guide and the one-row set is skipped though it has a row; set 3's
# positions follow H_ASYM, and it takes the epipolar band through H_ASYM p
GUIDED_CASE = (36, 257, (300, 0, 1, 63))
GUIDES = [gm.guide_of(0), gm.guide_of(1), (gm.NONE, np.zeros(9, np.float32), 0.0), gm.guide_of(1)]
LONG, BAND = 0, 3


def _guided_expected(capi, ratio, mutual):
    seed, nl, nrs = GUIDED_CASE
    left, rights, lxy, rxys = gm.positioned_many(*GUIDED_CASE)
    out = []
    for k, nr in enumerate(nrs):
        if GUIDES[k][0] == gm.NONE or nr == 0:
            out.append(np.zeros(0, capi.PAIR_U8_DTYPE))
            continue
        A, fm, fd, bm = gm.directed(("star", seed, k), left, lxy, rights[k], rxys[k], GUIDES[k])
        out.append(capi.pairs_join(fm, fd, bm if mutual else None, nr, ratio, mutual))
    return out


def _bytes(lists):
    return b"".join(np.ascontiguousarray(l).tobytes() for l in lists)


@pytest.mark.parametrize("mutual", [False, True], ids=["oneway", "mutual"])
def test_guided_star_call_equals_graph_call_on_the_star(capi, mutual):
    left, rights, lxy, rxys = gm.positioned_many(*GUIDED_CASE)
    guides = [gm.capi_guide(capi, g) for g in GUIDES]
    assert [g[0] for g in GUIDES] == [HOMOGRAPHY, EPIPOLAR, gm.NONE, EPIPOLAR]
    want = _guided_expected(capi, 0.8, mutual)

    def both(ks, capacity=None):
        """the star call and the graph call on sets ks of the star; asserts that they agree, returns the star's"""
        r, x, g = [rights[k] for k in ks], [rxys[k] for k in ks], [guides[k] for k in ks]
        s_lists, s_counts = capi.match_pairs_guided_many_u8(left, lxy, r, x, g, 0.8, mutual, capacity=capacity)
        g_lists, g_counts = capi.match_pairs_guided_graph_u8([left] + r, [lxy] + x, _star_graph(len(ks)), g, 0.8, mutual, capacity=capacity)
        assert list(s_counts) == list(g_counts) and len(s_lists) == len(g_lists) == len(ks), ks
        assert [l.tobytes() for l in s_lists] == [l.tobytes() for l in g_lists], ks
        return s_lists, list(s_counts)

    lists, counts = both(range(4))
    assert counts == [len(w) for w in want] and all(same_records(l, w) for l, w in zip(lists, want))
    assert counts[1] == 0 and counts[2] == 0 and counts[LONG] >= 30 and counts[BAND] >= 3, counts
    # a capacity inside the last set: the counts are still the totals, the prefix is written
    cap = sum(counts) - counts[BAND] // 2
    cut, cut_counts = both(range(4), capacity=cap)
    assert cut_counts == counts and _bytes(cut) == _bytes(lists)[:16 * cap]
    # K = 1
    one, one_counts = both([LONG])
    assert one_counts == [counts[LONG]] and one[0].tobytes() == lists[LONG].tobytes()
