"""dev tool (GPU box): what one call over an edge list costs beside the two loops it replaces, on one MI355X.
Device-resident byte descriptors, ratio 0.8 with PSX_PAIRS_MUTUAL, records into device buffers (the _dev forms):
  graph  psx_match_pairs_graph_u8_dev( sets, edges )                           one call
  stars  psx_match_pairs_many_u8_dev( L, {R ...} ) per left view of the list   one call per left view  } code this change does
  edges  psx_match_pairs_u8_dev( L, R ) per edge                               one call per edge       } not touch: the baselines
run ALTERNATELY in one process (graph, stars, edges, graph, ...): best of 5 after 2 warm-up rounds, host wall ms for the
whole edge list, the worst of the 5 in brackets, and the best as microseconds per edge.  The edge lists are grouped by left,
so the per-edge counts of the three must agree entry by entry: the tool asserts it.  Planted content as tools/match_many_ms.py
plants it: every view holds noisy copies of half of a common base set's rows, so any two views share matches.
Shapes: 32 views x 2048 rows, all pairs a < b (496 edges); 16 x 4096, all pairs (120); 64 x 2048, each view against the 8
that follow (476); the star 2048 x (64 x 2048), where `stars` is ONE one-to-many call; one edge 18 432 x 18 432, where
`stars` and `edges` are one call each.
usage: python tools/match_graph_ms.py [out.txt]      (default profiles/match_graph_ms.txt)"""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from popsift_amd import capi

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "match_graph_ms.txt")
REPS, WARM = 5, 2
AMPS = np.array([2, 8, 16, 24, 32, 40])


def views(seed, n, rows, base_rows):
    """the base set and n views of `rows` rows, half of them noisy copies of base rows"""
    base = np.random.default_rng(seed).integers(0, 64, (base_rows, 128), dtype=np.uint8)
    out = []
    for s in range(n):
        rng = np.random.default_rng([seed, s + 1])
        v = rng.integers(0, 64, (rows, 128), dtype=np.uint8)
        m = min(base_rows, rows) // 2
        src, dst = rng.permutation(base_rows)[:m], rng.permutation(rows)[:m]
        amp = AMPS[np.arange(m) % 6][:, None]
        noise = (rng.random((m, 128)) * (2 * amp + 1)).astype(np.int64) - amp
        v[dst] = np.clip(base[src].astype(np.int64) + noise, 0, 255).astype(np.uint8)
        out.append(v)
    return base, out


def alternate(calls):
    """calls: name -> function; every round runs each once, in order; (best, worst) of the REPS rounds after WARM"""
    ts = {n: [] for n in calls}
    for r in range(WARM + REPS):
        for n, f in calls.items():
            t0 = time.perf_counter()
            f()
            if r >= WARM:
                ts[n].append((time.perf_counter() - t0) * 1e3)
    return {n: (min(v), max(v)) for n, v in ts.items()}


def shapes():
    _, v = views(32, 32, 2048, 2048)
    yield "32 x 2048, all pairs", v, [(a, b) for a in range(32) for b in range(a + 1, 32)]
    _, v = views(16, 16, 4096, 4096)
    yield "16 x 4096, all pairs", v, [(a, b) for a in range(16) for b in range(a + 1, 16)]
    _, v = views(64, 64, 2048, 2048)
    yield "64 x 2048, window 8", v, [(a, b) for a in range(64) for b in range(a + 1, min(a + 9, 64))]
    base, v = views(2048 + 64, 64, 2048, 2048)
    yield "star 2048 x (64 x 2048)", [base] + v, [(0, b) for b in range(1, 65)]
    base, v = views(18432 + 1, 1, 18432, 18432)
    yield "one edge 18432 x 18432", [base] + v, [(0, 1)]


L = capi.lib()
o = capi.match_opts(0.8, True)
lines = ["match_graph_ms: psx_match_pairs_graph_u8_dev beside the loop of psx_match_pairs_many_u8_dev per left view and the loop of",
         "psx_match_pairs_u8_dev per edge, ratio 0.8, mutual, device in / device out; alternating in one process, best of %d after %d" % (REPS, WARM),
         "warm-up rounds [worst of the %d], host wall ms for the whole edge list; us/edge from the best" % REPS, "",
         "%-24s %6s %6s %20s %20s %20s %8s %8s %8s %9s" % ("shape", "edges", "lefts", "graph: one call", "stars: call per left", "edges: call per edge",
                                                            "graph", "stars", "edges", "pairs"),
         "%-24s %6s %6s %20s %20s %20s %8s %8s %8s" % ("", "", "", "ms", "ms", "ms", "us/edge", "us/edge", "us/edge")]
for name, sets, edges in shapes():
    bufs = []
    ptrs = capi._to_device(L, 0, sets, bufs)
    lens = np.array([len(s) for s in sets], np.int32)
    ne = len(edges)
    cap = int(sum(lens[a] for a, _ in edges))
    out = capi._to_device(L, 0, [np.zeros((cap, 4), np.int32)], bufs)[0]
    pa = (C.c_void_p * len(sets))(*[p.value for p in ptrs])
    ea = np.ascontiguousarray(edges, np.int32)
    g_counts, s_counts, e_counts = np.zeros(ne, np.int32), np.zeros(ne, np.int32), np.zeros(ne, np.int32)
    n = C.c_int()
    # the list grouped by left: (left, first edge, its rights as a pointer array, their lengths)
    stars, at = [], 0
    while at < ne:
        a, end = edges[at][0], at
        while end < ne and edges[end][0] == a:
            end += 1
        bs = [b for _, b in edges[at:end]]
        stars.append((a, at, (C.c_void_p * len(bs))(*[ptrs[b].value for b in bs]), np.array([lens[b] for b in bs], np.int32)))
        at = end

    def graph():
        assert L.psx_match_pairs_graph_u8_dev(0, pa, lens.ctypes.data, len(sets), ea.ctypes.data, ne, C.byref(o), out, cap, g_counts.ctypes.data, C.byref(n)) == 0

    def per_left():
        c = C.c_int()
        for a, at, rp, rl in stars:
            k = len(rl)
            assert L.psx_match_pairs_many_u8_dev(0, ptrs[a], int(lens[a]), rp, rl.ctypes.data, k, C.byref(o), out, k * int(lens[a]),
                                                 s_counts[at:].ctypes.data, C.byref(c)) == 0

    def per_edge():
        c = C.c_int()
        for e, (a, b) in enumerate(edges):
            assert L.psx_match_pairs_u8_dev(0, ptrs[a], int(lens[a]), ptrs[b], int(lens[b]), C.byref(o), out, int(lens[a]), C.byref(c)) == 0
            e_counts[e] = c.value

    t = alternate({"graph": graph, "stars": per_left, "edges": per_edge})
    assert np.array_equal(g_counts, s_counts) and np.array_equal(g_counts, e_counts) and n.value == g_counts.sum() > 0
    lines.append("%-24s %6d %6d %11.3f [%6.3f] %11.3f [%6.3f] %11.3f [%6.3f] %8.2f %8.2f %8.2f %9d" %
                 (name, ne, len(stars), t["graph"][0], t["graph"][1], t["stars"][0], t["stars"][1], t["edges"][0], t["edges"][1],
                  1e3 * t["graph"][0] / ne, 1e3 * t["stars"][0] / ne, 1e3 * t["edges"][0] / ne, n.value))
    for p in bufs:
        L.psx_dev_free(0, p)
text = "\n".join(lines) + "\n"
print(text)
with open(OUT, "w") as f:
    f.write(text)
