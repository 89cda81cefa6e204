"""Shared by the CPU and GPU tests of the batched geometric verification (psx_ransac_homography_many*,
psx_ransac_fundamental_many*; include/popsift_hip.h, "geometric verification"): K planted pair lists behind one another.

Set k is fundamental_cases.planted(n_k, seed, kind_k) for the fundamental matrix (kinds alternating general / rectified) and
ransac_cases.planted(n_k, seed) for the homography.  The sets' left position arrays are concatenated into the call's ONE
left array and each set's `left` indices are shifted by its offset; the right arrays stay per set.  The restatements
fc.expect / rc.expect therefore give each set's expected result unchanged -- only the records' `left` is shifted.

The sizes sit on the kernels' edges and no larger: the minimum (8 / 4) and its neighbours, the ballot (64), the
compaction's and the gather's workgroup (256), the score kernel's block (512, crossed by 1023 / 1024 / 1025 together
with the next one), and empty sets first, in the middle and last.  (N, seed) = (64, 3) and (65, 4): one and two blocks of
hypotheses."""
import numpy as np

from tests import fundamental_cases as fc
from tests import ransac_cases as rc

CONFIGS = [(64, 3), (65, 4)]
CONFIG_IDS = ["N%d_s%d" % c for c in CONFIGS]
MODELS = ("homography", "fundamental")
MIN = {"homography": 4, "fundamental": 8}
SIZES = {"fundamental": (0, 7, 8, 9, 63, 64, 65, 0, 255, 256, 257, 1023, 1024, 1025, 0),
         "homography": (0, 3, 4, 5, 63, 64, 65, 0, 255, 256, 257, 1023, 1024, 1025, 0)}
TOL = 2.0
assert rc.TOL == fc.TOL == TOL


def kind_of(k):
    return fc.KINDS[k % 2]


def planted_set(model, k, n, seed, u8=False):
    """(pairs, left_xy, right_xy) of set k, as the single-list tests use it"""
    return (fc.planted(n, seed, kind_of(k), u8) if model == "fundamental" else rc.planted(n, seed, u8))[:3]


def expect_set(model, k, n, N, seed, refit):
    return fc.expect(n, N, seed, kind_of(k), refit) if model == "fundamental" else rc.expect(n, N, seed, refit)


_CASES = {}


def case(model, seed, u8=False, sizes=None):
    """dict: sizes, lists (per-set records, `left` shifted into the concatenated left array), left_xy, right_xys, offsets
    (of every set's left positions); read-only arrays, computed once"""
    sizes = SIZES[model] if sizes is None else tuple(sizes)
    key = (model, seed, u8, sizes)
    if key not in _CASES:
        lists, lxys, rxys, offsets, off = [], [], [], [], 0
        for k, n in enumerate(sizes):
            pairs, lxy, rxy = planted_set(model, k, n, seed, u8)
            p = pairs.copy()
            p["left"] += off
            p.setflags(write=False)
            lists.append(p)
            lxys.append(lxy)
            rxys.append(rxy)
            offsets.append(off)
            off += n
        left_xy = np.concatenate(lxys).astype(np.float32).reshape(-1, 2)
        left_xy.setflags(write=False)
        _CASES[key] = dict(sizes=sizes, lists=lists, left_xy=left_xy, right_xys=rxys, offsets=offsets)
    return _CASES[key]


def shifted(records, off):
    r = records.copy()
    r["left"] += off
    return r


_EXPECT = {}


def expect(model, N, seed, refit, sizes=None):
    """per set: the single-list restatement's dict, its records' `left` shifted as case() shifts them"""
    sizes = SIZES[model] if sizes is None else tuple(sizes)
    key = (model, N, seed, refit, sizes)
    if key not in _EXPECT:
        c = case(model, seed, sizes=sizes)
        out = []
        for k, n in enumerate(sizes):
            e = dict(expect_set(model, k, n, N, seed, refit))
            e["records"] = shifted(e["records"], c["offsets"][k])
            out.append(e)
        _EXPECT[key] = out
    return _EXPECT[key]


def concat(lists, dtype=rc.PAIR_DTYPE):
    lists = list(lists)
    return np.concatenate(lists) if lists else np.zeros(0, dtype)


def premise(want_refit, want_sample, sizes):
    """What the restatement gives for the fundamental matrix at (N, seed) = (65, 4), asserted so that a later change of the
    generator cannot quietly stop covering these cases: no-model sets, ties resolved to the lowest index, a refit tried
    and rejected, a refit not tried, refits kept."""
    by_n = {}
    for n, e in zip(sizes, want_refit):
        by_n.setdefault(n, e)
    for n in (0, 7):
        assert by_n[n]["best"] == -1 and by_n[n]["inliers"] == 0 and not by_n[n]["m"].any(), n
    c8, c9 = by_n[8]["counts"], by_n[9]["counts"]
    assert (c8 == c8.max()).sum() == 65 and by_n[8]["best"] == 0, "n = 8: all 65 hypotheses tie"
    assert (c9 == c9.max()).sum() == 4 and by_n[9]["best"] == int(np.argmax(c9)), "n = 9: 4 tie"
    assert by_n[63]["sample_inliers"] == 8 and by_n[63]["refit_kept"] == 0, "n = 63: a refit tried and rejected"
    assert by_n[9]["sample_inliers"] == 4 and by_n[9]["refit_kept"] == 0, "n = 9: a refit not tried"
    for n in sizes:
        if n >= 64:
            assert by_n[n]["refit_kept"] == 1 and by_n[n]["inliers"] >= by_n[n]["sample_inliers"] >= 8, n
    # without the refit the sample model is the result
    for a, b in zip(want_refit, want_sample):
        assert b["refit_kept"] == 0 and a["best"] == b["best"] and a["sample_inliers"] == b["sample_inliers"]
