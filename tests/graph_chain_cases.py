"""Shared by the CPU and GPU tests of the two edge-list calls behind psx_match_pairs_graph_u8 (psx_ransac_*_graph*,
psx_match_pairs_guided_graph_u8*; include/popsift_hip.h, "A LIST OF VIEW PAIRS IN ONE CALL").

1. ransac_case(model): views of UNEQUAL length with positions -- match_graph_cases.MIXED_LENS = (300, 257, 0, 33, 513, 1)
   under MIXED_EDGES, the unsorted list with a duplicate, both orders, a self edge and empty sides -- and one pair list per
   edge of 0, min - 1, min, 255, 256, 257, 512 and 513 pairs (512 is the score kernel's block, 256 the gather's and the
   compaction's), every edge planted under a model of its OWN.
   How the positions are made.  A view's rows are cut into a LOW part, of which every edge that has the view on its right
   owns a segment, and a HIGH part, the view's free pool, which no edge writes.  Edge e = (a, b) with n pairs pairs slot j
   of its segment of b with a row l_j drawn from the free pool of a, and puts the right position of that slot at
   M_e (P_a[l_j] + depth_j (1, 0)) + t_e plus a jitter of radius 0, 0.5 or 1.5 px, M_e a rotation and scale and t_e a
   translation of the edge's own; two slots in five are outliers anywhere.  depth_j is 0 except for the fundamental
   matrix, where it is a per-point disparity: a scene with depth.  Pair i of the edge is slot i modulo the segment's
   length, so a list longer than its segment repeats correspondences.  The edges are laid in list order and a free pool is
   never written, so every plant stays true.  Because the free pool is the HIGH part, a left index of one view is out of
   range for every shorter view: a kernel that reads the wrong left array or the wrong length trips the range flag or
   changes the result.  The duplicate edge carries the same list as its first occurrence.

2. scene(seed, lens): byte descriptor sets WITH positions that share one scene, for the guided call and for the chain.  A
   pool of scene points, each a random descriptor and a place on a canvas; view v sees lens[v] of them in an order of its
   own, the descriptor with noise of the amplitudes of match_pairs_cases.AMPS, the place through the view's own similarity
   plus a jitter of radius 0, 0.5, 1.5 or 6 px (the last is inadmissible at tol 2).  true_h(a, b) is the homography from
   view a to view b.
   edge_guide(e, a, b): the guide of edge e -- e % 3 == 0 the edge's true homography at tol 2, == 1 the epipolar band
   through it ([epipole]_x H), == 2 PSX_GUIDE_NONE.
   guided_expected(...): the list the call owes for one edge from guided_cases.restate / expect_bytes_int64 and
   capi.pairs_join: no device code."""
import numpy as np

from tests import match_graph_cases as gcs
from tests.guided_cases import EPIPOLAR, HOMOGRAPHY, expect_bytes_int64, restate
from tests.match_pairs_cases import AMPS
from tests.ransac_cases import PAIR_DTYPE

NONE = 0
TOL = 2.0
MODELS = ("homography", "fundamental", "affine", "similarity")
MIN = {"homography": 4, "fundamental": 8, "affine": 3, "similarity": 2}
LENS = gcs.MIXED_LENS
EDGES = gcs.MIXED_EDGES
DUPLICATE = (9, 1)                       # edge 9 repeats edge 1: (0, 1)
# first row of every view's free pool (the rows below it are the right segments)
POOL = (200, 200, 0, 20, 400, 0)


def pair_counts(model):
    """pairs per edge of EDGES: 0 where a side is empty; min - 1 and min where a side has one row"""
    m = MIN[model]
    return (257, 513, m - 1, 256, 0, 512, m, 0, 255, 513)


def _segments():
    """edge -> (first row, rows) of its segment in its right view: the low part of a view split evenly among the edges that
    have it on the right (a duplicate shares its original's)"""
    seg = {}
    for v in range(len(LENS)):
        owners = [e for e, (a, b) in enumerate(EDGES) if b == v and e != DUPLICATE[0] and LENS[a] > 0 and LENS[b] > 0]
        low = POOL[v] if POOL[v] > 0 else LENS[v]
        for i, e in enumerate(owners):
            n = low // len(owners)
            seg[e] = (i * n, n)
    seg[DUPLICATE[0]] = seg[DUPLICATE[1]]
    return seg


def edge_model(e):
    """(2 x 2 matrix, translation) of edge e: a rotation by 0.1 (e + 1) rad, a scale of 1 + 0.03 e, its own shift"""
    th, s = 0.1 * (e + 1), 1.0 + 0.03 * e
    return s * np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]]), np.array([12.0 * e - 40.0, 25.0 - 7.0 * e])


_RANSAC = {}


def ransac_case(model, u8=False):
    """dict: lens, edges, xys (one float32 (n, 2) array per view), lists (one record array per edge), counts; read-only,
    computed once"""
    key = (model, u8)
    if key in _RANSAC:
        return _RANSAC[key]
    rng = np.random.default_rng(7100 + MODELS.index(model))
    xys = [rng.uniform([0.0, 0.0], [640.0, 480.0], (n, 2)) for n in LENS]
    seg = _segments()
    counts = pair_counts(model)
    lists = []
    for e, (a, b) in enumerate(EDGES):
        n = counts[e]
        p = np.zeros(n, gcs.PAIR_U8 if u8 else PAIR_DTYPE)
        if e == DUPLICATE[0]:
            p = lists[DUPLICATE[1]].copy()
        elif n:
            s0, slots = seg[e]
            lj = rng.integers(POOL[a], LENS[a], slots)
            mat, t = edge_model(e)
            depth = rng.uniform(-40.0, 40.0, slots) if model == "fundamental" else np.zeros(slots)
            ang = rng.uniform(0.0, 2 * np.pi, slots)
            rad = np.array([(0.0, 0.5, 1.5)[j % 3] for j in range(slots)])
            right = (xys[a][lj] + np.stack([depth, np.zeros(slots)], 1)) @ mat.T + t + np.stack([rad * np.cos(ang), rad * np.sin(ang)], 1)
            outlier = (np.arange(slots) % 5) >= 3 if slots > 4 else np.zeros(slots, bool)
            right[outlier] = rng.uniform([0.0, 0.0], [640.0, 480.0], (int(outlier.sum()), 2))
            xys[b][s0:s0 + slots] = right
            i = np.arange(n)
            p["left"], p["right"] = lj[i % slots], s0 + i % slots
            p["d1"], p["d2"] = i + 1, 2 * i + 7                     # a payload that must travel with the record
        p.setflags(write=False)
        lists.append(p)
    xys = [x.astype(np.float32) for x in xys]
    for x in xys:
        x.setflags(write=False)
    for e, (a, b) in enumerate(EDGES):
        assert len(lists[e]) == 0 or (lists[e]["left"].max() < LENS[a] and lists[e]["right"].max() < LENS[b])
    _RANSAC[key] = dict(lens=LENS, edges=EDGES, xys=xys, lists=lists, counts=counts)
    return _RANSAC[key]


# ---- 2. views that share a scene -----------------------------------------------------------------------------------------
CANVAS = 400.0
RADII = (0.0, 0.5, 1.5, 6.0)


def view_transform(v):
    """the 3 x 3 similarity that places the canvas in view v"""
    th, s = 0.07 * v - 0.1, 1.0 + 0.05 * v
    return np.array([[s * np.cos(th), -s * np.sin(th), 15.0 * v], [s * np.sin(th), s * np.cos(th), 40.0 - 9.0 * v], [0.0, 0.0, 1.0]])


def true_h(a, b):
    """the homography from view a to view b, float32 row major"""
    return (view_transform(b) @ np.linalg.inv(view_transform(a))).astype(np.float32).reshape(9)


_SCENES = {}


def scene(seed, lens):
    """(sets, xys, ids): per view the uint8 (n, 128) descriptors, the float32 (n, 2) positions and the scene point behind
    every row; read-only, computed once"""
    key = (seed, tuple(lens))
    if key in _SCENES:
        return _SCENES[key]
    rng = np.random.default_rng([9000, seed])
    pool = max(lens) + max(lens) // 4 + 8
    base = rng.integers(0, 64, (pool, 128), dtype=np.uint8)
    world = rng.uniform(0.0, CANVAS, (pool, 2))
    sets, xys, ids = [], [], []
    for v, n in enumerate(lens):
        pick = rng.permutation(pool)[:n]
        amp = np.array([AMPS[t % len(AMPS)] for t in range(n)])[:, None]
        noise = np.rint(rng.uniform(-1.0, 1.0, (n, 128)) * amp).astype(np.int64)
        desc = np.clip(base[pick].astype(np.int64) + noise, 0, 255).astype(np.uint8)
        q = np.concatenate([world[pick], np.ones((n, 1))], 1) @ view_transform(v).T
        ang = rng.uniform(0.0, 2 * np.pi, n)
        rad = np.array([RADII[t % len(RADII)] for t in range(n)])
        xy = (q[:, :2] + np.stack([rad * np.cos(ang), rad * np.sin(ang)], 1)).astype(np.float32)
        for a in (desc, xy, pick):
            a.setflags(write=False)
        sets.append(desc)
        xys.append(xy)
        ids.append(pick)
    _SCENES[key] = (sets, xys, ids)
    return _SCENES[key]


def edge_guide(e, a, b):
    """(kind, m, tol) of edge e = (a, b)"""
    h = true_h(a, b)
    if e % 3 == 0:
        return HOMOGRAPHY, h, TOL
    if e % 3 == 1:
        ep = np.array([[0.0, -1.0, 310.0], [1.0, 0.0, 900.0], [-310.0, -900.0, 0.0]])          # [epipole]_x, epipole (-900, 310, 1)
        f = ep @ h.astype(np.float64).reshape(3, 3)
        return EPIPOLAR, (f / np.abs(f).max()).astype(np.float32).reshape(9), TOL
    return NONE, np.zeros(9, np.float32), 0.0


def capi_guide(capi, guide):
    kind, m, tol = guide
    return capi.Guide.none() if kind == NONE else capi.Guide.make(kind, m, tol)


_DIRECTED = {}


def guided_expected(capi, seed, lens, e, a, b, guide, ratio, mutual):
    """PAIR_U8_DTYPE records: what psx_match_pairs_guided_u8 owes for views a, b of scene(seed, lens) under `guide`"""
    sets, xys, _ = scene(seed, lens)
    kind, m, tol = guide
    if kind == NONE or lens[a] == 0 or lens[b] == 0:
        return np.zeros(0, capi.PAIR_U8_DTYPE)
    key = (seed, tuple(lens), e, a, b)
    if key not in _DIRECTED:
        A = restate(kind, m, tol, xys[a], xys[b])
        fm, fd = expect_bytes_int64(sets[a], sets[b], A)
        bm, _ = expect_bytes_int64(sets[b], sets[a], A.T)
        _DIRECTED[key] = (fm, fd, bm)
    fm, fd, bm = _DIRECTED[key]
    return capi.pairs_join(fm, fd, bm if mutual else None, lens[b], ratio, mutual)


def concat(lists, dtype=PAIR_DTYPE):
    lists = list(lists)
    return np.concatenate(lists) if lists else np.zeros(0, dtype)
