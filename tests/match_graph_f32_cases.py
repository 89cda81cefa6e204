"""Shared by the CPU and GPU tests of the FLOAT pair search over an edge list (psx_match_pairs_graph): the sets and edge
lists of tests/match_graph_cases.py as float32 in the two flavours of tests/match_many_f32_cases.py ("int": the bytes as
floats, every distance an exact integer; "norm512": every row scaled to norm 512, so that sums and norms ROUND), the list
that names the prefilter kernel's edges, the path rule and the plan restated from the documented rules alone.

The sizes: a tile of 32, a staged block of 64, the seeding pass' 128 rows, an outer block of 256, a prefilter chunk (512 at
least, 4096 at most) and the path thresholds (4096 right rows over the live edges, 256 left rows per live edge on
average)."""
import numpy as np

from tests import match_graph_cases as gcs
from tests.match_many_f32_cases import FLAVOURS, flavour                    # noqa: F401  (re-exported to the tests)

MIXED_SEED, MIXED_LENS, MIXED_EDGES = gcs.MIXED_SEED, gcs.MIXED_LENS, gcs.MIXED_EDGES
BIG_SEED, BIG_LENS, BIG_EDGES = gcs.BIG_SEED, gcs.BIG_LENS, gcs.BIG_EDGES
TINY_EDGES = gcs.TINY_EDGES
ORACLE_CASES = ("mixed", "big")               # also checked against the host join of the oracle's directed results

# ---- 3. the prefilter kernel's edges: set 0 (3100 rows) lifts the totals over the rule; every other set meets it as the
# outer and as the inner side; a self edge, a duplicate, and so both orders of every pair --------------------------------------
EDGE_SEED = 52
EDGE_LENS = (3100, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 512, 513, 4097)
EDGE_EDGES = ([(s, 0) for s in range(1, len(EDGE_LENS))] + [(0, 0)] + [(0, s) for s in range(1, len(EDGE_LENS))] +
              [(13, 16), (0, 13), (16, 13)])          # 257 x 4097 and back (two chunks on the inner side), a duplicate of (0, 13)

# ---- 8. the smallest list of duplicate self edges of one 18 432-row set that the plan cuts into two forward groups ------------
GROUP_LEN = 18432

# the shapes tools/match_graph_f32_ms.py measures
MEASURED = {
    "32x2048-all": ((2048,) * 32, [(a, b) for a in range(32) for b in range(a + 1, 32)]),
    "16x4096-all": ((4096,) * 16, [(a, b) for a in range(16) for b in range(a + 1, 16)]),
    "64x2048-next8": ((2048,) * 64, [(a, b) for a in range(64) for b in range(a + 1, min(a + 9, 64))]),
    "star64": ((2048,) * 65, [(0, b) for b in range(1, 65)]),
    "one-18432": ((18432, 18432), [(0, 1)]),
}

# what the plan is checked on without a GPU: the GPU cases and the measured shapes
PLAN_CASES = dict({
    "mixed": (MIXED_LENS, MIXED_EDGES),
    "lefts": (gcs.LEFTS_LENS, gcs.LEFTS_EDGES),
    "big": (BIG_LENS, BIG_EDGES),
    "edges": (EDGE_LENS, EDGE_EDGES),
    "tiny400": (tuple(i % 41 for i in range(200)), TINY_EDGES),
    "groups12": ((GROUP_LEN,), [(0, 0)] * 12),
}, **MEASURED)

# the rule at its edges: (lens, edges, mfma, path)
RULE_CASES = [
    ((255, 4096), [(0, 1)], True, 1),
    ((256, 4095), [(0, 1)], True, 1),
    ((256, 4096), [(0, 1)], True, 2),
    ((256, 2048), [(0, 1), (0, 1)], True, 2),
    ((256, 4096, 1), [(0, 1), (2, 2)], True, 1),          # the mean left side is 128.5
    ((256, 4096), [(0, 1)], False, 1),
    ((256, 4096, 0), [(0, 2), (2, 1)], True, 0),          # no live edge
]

_SETS = {}


def graph_sets_f32(seed, lens, which):
    """[set 0, set 1, ...] float32 in one of FLAVOURS: graph_sets of tests/match_graph_cases.py; computed once, read-only"""
    key = (seed, tuple(lens), which)
    if key not in _SETS:
        out = [flavour(s, which) for s in gcs.graph_sets(seed, lens)]
        for s in out:
            s.setflags(write=False)
        _SETS[key] = out
    return _SETS[key]


def tiny_sets_f32(which="norm512"):
    """the 200 tiny sets (lengths i % 41) as float32"""
    return [flavour(s, which) for s in gcs.tiny_sets()]


def planned_path(lens, edges, mfma=True):
    """the rule of the header, restated: over the live edges as listed, the prefilter iff the switch is on, the right rows
    sum to 4096 at least and the left rows to 256 per live edge at least"""
    live = [(a, b) for a, b in edges if lens[a] > 0 and lens[b] > 0]
    if not live:
        return 0
    return 2 if (mfma and sum(lens[b] for _, b in live) >= 4096 and sum(lens[a] for a, _ in live) >= 256 * len(live)) else 1


def nchunks(n, chunk_len, step):
    """chunks of a set of n >= 1 rows at a chunk length: ceil(n / chunk_len) equal pieces, rounded up to whole `step` rows"""
    pieces = -(-n // chunk_len)
    size = -(-(-(-n // pieces)) // step) * step
    return -(-n // size)


def plan_restated(lens, edges, mutual, path):
    """The figures of psx_match_graph_f32_plan derived from the documented rules alone: referenced sets, blocks of 256, the
    call's ONE chunk length (scan: whatever <= 512 in whole tiles the library reports; prefilter: the smallest multiple of
    64 in [512, 4096] at which the direction with fewer items has at most 768 of them, 4096 if none), items = blocks x
    chunks per edge, join workgroups, groups of whole edges under 256 MiB of 16 (scan) or 264 (prefilter) bytes per (chunk,
    outer row), launches.  Returns a function chunk_len -> dict; for the prefilter the dict holds the chunk length itself."""
    lens = list(lens)
    live = [(a, b) for a, b in edges if lens[a] > 0 and lens[b] > 0]
    ref = sorted({s for e in live for s in e})
    step, unit = (64, 264) if path == 2 else (32, 16)
    nb = {s: -(-lens[s] // 256) for s in ref}

    def items(chunk_len):
        nc = {s: nchunks(lens[s], chunk_len, step) for s in ref}
        return nc, sum(nb[a] * nc[b] for a, b in live), sum(nb[b] * nc[a] for a, b in live)

    def groups(nc, backward):
        n, cur = 0, 0
        big = 0
        for a, b in live:
            o, i = (b, a) if backward else (a, b)
            en = nc[i] * lens[o]
            if cur > 0 and unit * (cur + en) > 256 << 20:
                n, big, cur = n + 1, max(big, cur), 0
            cur += en
        if cur > 0:
            n, big = n + 1, max(big, cur)
        return n, big

    def at(chunk_len):
        nc, fi, bi = items(chunk_len)
        fg, fbig = groups(nc, False)
        bg, bbig = groups(nc, True) if mutual else (0, 0)
        return {"path": path, "referenced_sets": len(ref), "blocks": sum(nb.values()), "chunks": sum(nc.values()), "chunk_len": chunk_len,
                "fwd_items": fi, "bwd_items": bi if mutual else 0, "fwd_groups": fg, "bwd_groups": bg,
                "join_workgroups": sum(nb[a] for a, _ in live), "launches": (2 if path == 2 else 1) + 2 * (fg + bg) + 3,
                "scratch_bytes": unit * max(fbig, bbig)}

    if path != 2:
        return at
    want = 4096
    for cl in range(512, 4096, 64):
        _, fi, bi = items(cl)
        if (min(fi, bi) if mutual else fi) <= 768:
            want = cl
            break
    return lambda chunk_len=None: at(want)
