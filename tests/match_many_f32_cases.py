"""Shared by the CPU and GPU tests of the one-to-many FLOAT pair search (psx_match_pairs_many): the planted sets of
tests/match_many_cases.py as float32 in two flavours, the cases whose sizes name the edges of both paths, and the rule
that says which path a call takes.

Flavours: "int" -- the bytes as float32, every distance an exact integer --, and "norm512" -- every row L2-normalised and
scaled to norm 512 in float32, so that products, sums and norms ROUND and the operation tree's order shows.

The sizes: a tile of 32, a staged block of 64, a prefilter chunk (512 at least), an outer block of 256 and the path
threshold (256 left rows, 4096 right rows in all sets)."""
import numpy as np

from tests.match_many_cases import TINY_LENS, planted_many, tiny_many

FLAVOURS = ("int", "norm512")

# (seed, nl, right set lengths)
CASES = [(31, 300, (257, 0, 1, 31, 32, 33, 63, 64, 65, 512, 513, 255, 256, 3000)),     # sum 5082: prefilter
         (32, 257, (64, 1000, 300, 2800)),                                             # sum 4164: prefilter
         (33, 1, (1, 2, 40)),                                                          # scan
         (34, 2500, (2300, 700, 1200)),                                                # sum 4200: prefilter, several outer blocks
         (35, 255, (4096,)),                                                           # one left row short: scan
         (36, 256, (4095,)),                                                           # one right row short: scan
         (37, 256, (4096,))]                                                           # both thresholds met: prefilter
CASE_IDS = ["seed%d" % c[0] for c in CASES]
ORACLE_SEEDS = (31, 34)                       # also checked against the host join of the oracle's directed results


def planned_path(nl, lens, mfma=True):
    """the rule of the issue, restated: the prefilter iff the switch is on, nl >= 256 and sum(lens) >= 4096"""
    if nl == 0 or sum(lens) == 0:
        return 0
    return 2 if (mfma and nl >= 256 and sum(lens) >= 4096) else 1


def flavour(a, which):
    """a uint8 (n, 128) set as float32 in one of FLAVOURS"""
    f = np.ascontiguousarray(a, np.float32).reshape(-1, 128)
    if which == "int":
        return f
    assert which == "norm512"
    n = np.sqrt((f * f).sum(axis=1, dtype=np.float32)).astype(np.float32)
    assert np.all(n > 0)
    return np.ascontiguousarray(f / n[:, None] * np.float32(512.0), np.float32)


_SETS = {}


def planted_many_f32(seed, nl, lens, which):
    """(left, [right_k]) float32, computed once per (seed, flavour) and read-only"""
    key = (seed, nl, tuple(lens), which)
    if key not in _SETS:
        left, rights = planted_many(seed, nl, lens)
        out = (flavour(left, which), [flavour(r, which) for r in rights])
        out[0].setflags(write=False)
        for r in out[1]:
            r.setflags(write=False)
        _SETS[key] = out
    return _SETS[key]


def tiny_many_f32(which="norm512", nl=70):
    """tiny_many (nl left rows, the 200 sets of TINY_LENS) as float32"""
    left, rights = tiny_many(nl=nl)
    return flavour(left, which), [flavour(r, which) for r in rights]
