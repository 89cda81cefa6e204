"""Shared by the CPU and GPU tests of the pair search over an edge list (psx_match_pairs_graph_u8): descriptor sets and edge
lists with a known, non-trivial outcome per edge, a numpy restatement of the single call, and of what the graph call owes its
caller -- the concatenation of the per-edge lists in the order of the edge list, the per-edge counts, the total, the
truncation at a capacity (contract / slices of tests/match_many_cases.py: the concatenation rule is the same).

The sets come from planted_many (tests/match_many_cases.py, imported, not edited): set 0 is its left set, sets 1 .. its right
sets.  Every right set holds noisy copies of left rows, so edges AMONG the right sets find pairs too."""
import numpy as np

from tests.match_many_cases import contract, planted_many, slices, tiny_many      # noqa: F401  (re-exported to the tests)
from tests.match_pairs_cases import INT_MAX, restate

PAIR_U8 = np.dtype([("left", "<i4"), ("right", "<i4"), ("d1", "<i4"), ("d2", "<i4")])

# ---- 1. the mixed list: unsorted; both orders; a self edge; an empty right and an empty left; one row; a duplicate ----------
MIXED_SEED = 31
MIXED_LENS = (300, 257, 0, 33, 513, 1)
MIXED_EDGES = [(3, 4), (0, 1), (4, 5), (0, 0), (0, 2), (1, 0), (5, 4), (2, 0), (4, 3), (0, 1)]
MIXED_PREMISE = [(0, 1), (1, 0)]            # the edges between set 0 and a set of >= 64 rows: assert_premise holds for them

# ---- 2. different left lengths in one join: 1, 255, 256, 257 and 600 left rows; several blocks / chunks / join workgroups ---
LEFTS_SEED = 32
LEFTS_LENS = (600, 1, 255, 256, 257, 300)
LEFTS_EDGES = [(1, 0), (2, 5), (3, 0), (4, 5), (0, 5), (4, 0), (0, 3)]
BIG_SEED = 24
BIG_LENS = (2500, 2300, 700)
BIG_EDGES = [(a, b) for a in range(3) for b in range(3) if a != b]

# ---- 7. 400 edges over the 200 tiny sets ----------------------------------------------------------------------------------
TINY_EDGES = [(i % 200, (7 * i + 3) % 200) for i in range(400)]

# what the plan is checked on without a GPU (the GPU cases, and the shapes the measurement uses)
PLAN_CASES = {
    "mixed": (MIXED_LENS, MIXED_EDGES),
    "lefts": (LEFTS_LENS, LEFTS_EDGES),
    "big": (BIG_LENS, BIG_EDGES),
    "tiny400": (tuple(i % 41 for i in range(200)), TINY_EDGES),
    "32x2048-all": ((2048,) * 32, [(a, b) for a in range(32) for b in range(a + 1, 32)]),
    "budget": ((18432,), [(0, 0)] * 64),
}


def graph_sets(seed, lens):
    """[set 0, set 1, ...] uint8 descriptor sets of the given lengths: planted_many's left set, then its right sets"""
    left, rights = planted_many(seed, lens[0], lens[1:])
    return [left] + rights


def tiny_sets():
    """the 200 right sets of tiny_many (lengths i % 41)"""
    return tiny_many()[1]


def numpy_pairs(left, right, ratio, mutual):
    """psx_match_pairs_u8 restated in numpy, independent of the library: the two smallest right rows under the (squared
    distance, index) order, the ratio test as a float32 division, the cross-check; PAIR_U8 records in ascending left"""
    nl, nr = len(left), len(right)
    if nl == 0 or nr == 0:
        return np.zeros(0, PAIR_U8)

    def directed(a, b):
        a64, b64 = a.astype(np.int64), b.astype(np.int64)
        d = (a64 * a64).sum(1)[:, None] + (b64 * b64).sum(1)[None, :] - 2 * (a64 @ b64.T)
        order = np.argsort(d, axis=1, kind="stable")[:, :2]
        m = np.zeros((len(a), 3), np.int32)
        dist = np.full((len(a), 2), INT_MAX, np.int32)
        m[:, 0] = order[:, 0]
        dist[:, 0] = d[np.arange(len(a)), order[:, 0]]
        if len(b) > 1:
            m[:, 1] = order[:, 1]
            dist[:, 1] = d[np.arange(len(a)), order[:, 1]]
        return m, dist

    fm, fd = directed(left, right)
    bm, _ = directed(right, left)
    kept, _, _, _ = restate(fm, fd, bm, nr, ratio, mutual)
    out = np.zeros(len(kept), PAIR_U8)
    out["left"], out["right"], out["d1"], out["d2"] = kept, fm[kept, 0], fd[kept, 0], fd[kept, 1]
    return out


def nchunks(n, chunk_len):
    """chunks of a set of n >= 1 rows at a chunk length: ceil(n / chunk_len) pieces of equal length, rounded up to whole tiles"""
    pieces = -(-n // chunk_len)
    step = -(-(-(-n // pieces)) // 32) * 32
    return -(-n // step)


def plan_restated(lens, edges, mutual):
    """The figures of psx_match_graph_plan derived from the documented rules alone (blocks of 256, ONE chunk length for the
    call, items = blocks x chunks per edge, join workgroups = ceil(lens[left] / 256) per edge), for any chunk length the
    library reports: returns a function chunk_len -> dict of the counts that follow from it"""
    lens = list(lens)
    live = [(a, b) for a, b in edges if lens[a] > 0 and lens[b] > 0]
    ref = sorted({s for e in live for s in e})

    def at(chunk_len):
        nb = {s: -(-lens[s] // 256) for s in ref}
        nc = {s: nchunks(lens[s], chunk_len) for s in ref}
        return {"referenced_sets": len(ref), "blocks": sum(nb.values()), "chunks": sum(nc.values()),
                "fwd_items": sum(nb[a] * nc[b] for a, b in live), "bwd_items": sum(nb[b] * nc[a] for a, b in live) if mutual else 0,
                "join_workgroups": sum(nb[a] for a, _ in live)}
    return at
