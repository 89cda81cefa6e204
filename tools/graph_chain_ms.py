"""dev tool (GPU box): what the two edge-list calls behind the graph matcher cost beside the two loops each replaces, on
one MI355X.  Device-resident planted views with positions, records in device buffers (the _dev forms):
  graph  psx_ransac_<model>_graph_dev / psx_match_pairs_guided_graph_u8_dev( views, edges )   one call
  stars  psx_ransac_<model>_many_dev / psx_match_pairs_guided_many_u8_dev per left view       one call per left view } code this
  edges  psx_ransac_<model>_dev / psx_match_pairs_guided_u8_dev per edge                      one call per edge      } change does
                                                                                                                       not touch
run ALTERNATELY in one process (graph, stars, edges, graph, ...): best of 5 after 2 warm-up rounds, host wall ms for the
whole edge list, the worst of the 5 in brackets, and the best as microseconds per edge.  The edge lists are grouped by left,
so the three must agree result by result and count by count: the tool asserts it.
RANSAC: homography and fundamental matrix, 1024 hypotheses, refit on, tol 2, on the lists psx_match_pairs_graph_u8_dev
(ratio 0.8, mutual) left in HBM.  Guided: ratio 0.8, mutual, ONE guide for all edges, as tools/match_guided_many_ms.py has
them: window = identity H with the radius that gives a left point about 2.5 admissible right points; band = the epipolar
band of a horizontal motion, tol 2.  chain: psx_match_pairs_graph_u8_dev -> psx_ransac_homography_graph_dev ->
psx_guides_from_ransac -> psx_match_pairs_guided_graph_u8_dev beside the same three steps per left view and per edge.
Scene: points uniform in 1920 x 1080 with a depth in [1, 2]; view s is a camera moved 0.25 s px sideways, so a point's
disparity between two views is at most 16 px and its row is the same; every view holds noisy copies of half of the base
set's rows.
Shapes: 32 views x 2048 rows, all pairs a < b (496 edges); 64 x 2048, each view against the 8 that follow (476); the star
2048 x (64 x 2048), where `stars` is ONE call; one edge 2048 x 2048, where `stars` and `edges` are one call each.
usage: python tools/graph_chain_ms.py [out.txt]      (default profiles/graph_chain_ms.txt)"""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from popsift_amd import capi

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "graph_chain_ms.txt")
REPS, WARM = 5, 2
W, H = 1920.0, 1080.0
AMPS = np.array([2, 8, 16, 24, 32, 40])
IDENT = (1, 0, 0, 0, 1, 0, 0, 0, 1)
F_ROWS = (0, 0, 0, 0, 0, -1, 0, 1, 0)
RES_B, GUIDE_B = C.sizeof(capi.RansacResult), C.sizeof(capi.Guide)


def views(seed, n, rows, first_is_base=False):
    """n views of `rows` rows with positions: half of a view's rows are noisy copies of base rows, seen from its camera"""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 64, (rows, 128), dtype=np.uint8)
    bxy = rng.uniform((0, 0), (W, H), (rows, 2))
    depth = rng.uniform(1.0, 2.0, rows)
    sets, xys = ([base], [bxy.astype(np.float32)]) if first_is_base else ([], [])
    for s in range(len(sets), n):
        rng = np.random.default_rng([seed, s + 1])
        v = rng.integers(0, 64, (rows, 128), dtype=np.uint8)
        xy = rng.uniform((0, 0), (W, H), (rows, 2))
        m = rows // 2
        src, dst = rng.permutation(rows)[:m], rng.permutation(rows)[:m]
        amp = AMPS[np.arange(m) % 6][:, None]
        noise = (rng.random((m, 128)) * (2 * amp + 1)).astype(np.int64) - amp
        v[dst] = np.clip(base[src].astype(np.int64) + noise, 0, 255).astype(np.uint8)
        xy[dst] = bxy[src] + np.stack([0.25 * s / depth[src], np.zeros(m)], 1) + rng.uniform(-0.5, 0.5, (m, 2))
        sets.append(v)
        xys.append(xy.astype(np.float32))
    return sets, xys


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
    s, x = views(32, 32, 2048)
    yield "32 x 2048, all pairs", s, x, [(a, b) for a in range(32) for b in range(a + 1, 32)], True
    s, x = views(64, 64, 2048)
    yield "64 x 2048, window 8", s, x, [(a, b) for a in range(64) for b in range(a + 1, min(a + 9, 64))], True
    s, x = views(65, 65, 2048, first_is_base=True)
    yield "star 2048 x (64 x 2048)", s, x, [(0, b) for b in range(1, 65)], False
    s, x = views(2, 2, 2048, first_is_base=True)
    yield "one edge 2048 x 2048", s, x, [(0, 1)], False


L = capi.lib()
mo = capi.match_opts(0.8, True)
ro = capi.ransac_opts(2.0, 1024, 1, True)
head = "%-24s %-14s %6s %6s %20s %20s %20s %8s %8s %8s %9s"
row = "%-24s %-14s %6d %6d %11.3f [%6.3f] %11.3f [%6.3f] %11.3f [%6.3f] %8.2f %8.2f %8.2f %9d"
lines = ["graph_chain_ms: the edge-list calls beside the loop of the one-to-many calls per left view and the loop of the single calls per",
         "edge; device in / device out; alternating in one process, best of %d after %d warm-up rounds [worst of the %d], host wall ms for" % (REPS, WARM, REPS),
         "the whole edge list; us/edge from the best.  RANSAC: 1024 hypotheses, refit, tol 2; guided and chain: ratio 0.8, mutual", "",
         head % ("shape", "step", "edges", "lefts", "graph: one call", "stars: call per left", "edges: call per edge", "graph", "stars", "edges", "records"),
         head % ("", "", "", "", "ms", "ms", "ms", "us/edge", "us/edge", "us/edge", "")]
for name, sets, xys, edges, with_chain in shapes():
    bufs = []
    ns, ne = len(sets), len(edges)
    ptrs = [p.value for p in capi._to_device(L, 0, sets, bufs)]
    xptrs = [p.value for p in capi._to_device(L, 0, xys, bufs)]
    lens = np.array([len(s) for s in sets], np.int32)
    cap = int(sum(lens[a] for a, _ in edges))
    d_pairs, d_inl, d_re, d_tmp = [p.value for p in capi._to_device(L, 0, [np.zeros((cap, 4), np.int32)] * 4, bufs)]
    pa, xa = (C.c_void_p * ns)(*ptrs), (C.c_void_p * ns)(*xptrs)
    ea = np.ascontiguousarray(edges, np.int32)
    ec = np.zeros(ne, np.int32)
    n = C.c_int()
    # the list grouped by left: (left, first edge, its rights' descriptor and position pointer arrays, their lengths)
    stars, at = [], 0
    while at < ne:
        a, end = edges[at][0], at
        while end < ne and edges[end][0] == a:
            end += 1
        bs = [b for _, b in edges[at:end]]
        stars.append((a, at, (C.c_void_p * len(bs))(*[ptrs[b] for b in bs]), (C.c_void_p * len(bs))(*[xptrs[b] for b in bs]),
                      np.array([lens[b] for b in bs], np.int32)))
        at = end
    assert L.psx_match_pairs_graph_u8_dev(0, pa, lens.ctypes.data, ns, ea.ctypes.data, ne, C.byref(mo), d_pairs, cap, ec.ctypes.data, C.byref(n)) == 0
    first = np.concatenate([[0], np.cumsum(ec)]).astype(np.int64)          # an edge's first record

    def report(step, t, records):
        lines.append(row % (name, step, ne, len(stars), t["graph"][0], t["graph"][1], t["stars"][0], t["stars"][1], t["edges"][0], t["edges"][1],
                            1e3 * t["graph"][0] / ne, 1e3 * t["stars"][0] / ne, 1e3 * t["edges"][0] / ne, records))

    # ---- RANSAC on the matcher's lists ----
    for model in ("homography", "fundamental"):
        f_graph, f_many, f_one = (getattr(L, "psx_ransac_%s%s" % (model, s)) for s in ("_graph_dev", "_many_dev", "_dev"))
        rg, rs, re_ = ((capi.RansacResult * ne)() for _ in range(3))
        cg = C.c_int()

        def graph():
            assert f_graph(0, d_pairs, ec.ctypes.data, ea.ctypes.data, ne, xa, lens.ctypes.data, ns, C.byref(ro), rg, d_inl, cap, C.byref(cg), None, None) == 0

        def per_left():
            c = C.c_int()
            for a, at, _, rxp, rl in stars:
                assert f_many(0, d_pairs + 16 * int(first[at]), ec[at:].ctypes.data, len(rl), xptrs[a], int(lens[a]), rxp, rl.ctypes.data, C.byref(ro),
                              C.byref(rs, at * RES_B), d_tmp, cap, C.byref(c), None, None) == 0

        def per_edge():
            c = C.c_int()
            for e, (a, b) in enumerate(edges):
                assert f_one(0, d_pairs + 16 * int(first[e]), int(ec[e]), xptrs[a], int(lens[a]), xptrs[b], int(lens[b]), C.byref(ro),
                             C.byref(re_[e]), d_tmp, cap, C.byref(c), None, None) == 0

        t = alternate({"graph": graph, "stars": per_left, "edges": per_edge})
        assert bytes(rg) == bytes(rs) == bytes(re_) and cg.value == sum(r.inliers for r in rg)
        report("ransac " + model[:4], t, cg.value)

    # ---- the guided re-match under one guide for all edges ----
    radius = float(np.sqrt(2.5 * W * H / (np.pi * 2048)))
    for gname, guide in (("window", capi.Guide.homography(IDENT, radius)), ("band", capi.Guide.epipolar(F_ROWS, 2.0))):
        ga = (capi.Guide * ne)(*[guide] * ne)
        gc_, sc_, ec_ = np.zeros(ne, np.int32), np.zeros(ne, np.int32), np.zeros(ne, np.int32)
        ng = C.c_int()

        def graph():
            assert L.psx_match_pairs_guided_graph_u8_dev(0, pa, xa, lens.ctypes.data, ns, ea.ctypes.data, ne, ga, C.byref(mo), d_re, cap,
                                                         gc_.ctypes.data, C.byref(ng)) == 0

        def per_left():
            c = C.c_int()
            for a, at, rp, rxp, rl in stars:
                k = len(rl)
                assert L.psx_match_pairs_guided_many_u8_dev(0, ptrs[a], xptrs[a], int(lens[a]), rp, rxp, rl.ctypes.data, k, C.byref(ga, at * GUIDE_B),
                                                            C.byref(mo), d_tmp, k * int(lens[a]), sc_[at:].ctypes.data, C.byref(c)) == 0

        def per_edge():
            c = C.c_int()
            for e, (a, b) in enumerate(edges):
                assert L.psx_match_pairs_guided_u8_dev(0, ptrs[a], xptrs[a], int(lens[a]), ptrs[b], xptrs[b], int(lens[b]), C.byref(guide), C.byref(mo),
                                                       d_tmp, int(lens[a]), C.byref(c)) == 0
                ec_[e] = c.value

        t = alternate({"graph": graph, "stars": per_left, "edges": per_edge})
        assert np.array_equal(gc_, sc_) and np.array_equal(gc_, ec_) and ng.value == gc_.sum() > 0
        report("guided " + gname, t, ng.value)

    # ---- the whole chain: match -> verify (homography) -> guides -> re-match ----
    if with_chain:
        rg, rs, re_ = ((capi.RansacResult * ne)() for _ in range(3))
        gg, gs = (capi.Guide * ne)(), (capi.Guide * ne)()
        c1, c3, s1, s3, e3 = (np.zeros(ne, np.int32) for _ in range(5))
        tot = C.c_int()

        def graph():
            c = C.c_int()
            assert L.psx_match_pairs_graph_u8_dev(0, pa, lens.ctypes.data, ns, ea.ctypes.data, ne, C.byref(mo), d_pairs, cap, c1.ctypes.data, C.byref(c)) == 0
            assert L.psx_ransac_homography_graph_dev(0, d_pairs, c1.ctypes.data, ea.ctypes.data, ne, xa, lens.ctypes.data, ns, C.byref(ro), rg, d_inl, cap,
                                                     C.byref(c), None, None) == 0
            assert L.psx_guides_from_ransac(rg, ne, capi.GUIDE_HOMOGRAPHY, 2.0, gg) == 0
            assert L.psx_match_pairs_guided_graph_u8_dev(0, pa, xa, lens.ctypes.data, ns, ea.ctypes.data, ne, gg, C.byref(mo), d_re, cap, c3.ctypes.data,
                                                         C.byref(tot)) == 0

        def per_left():
            c = C.c_int()
            for a, at, rp, rxp, rl in stars:
                k, nl = len(rl), int(lens[a])
                assert L.psx_match_pairs_many_u8_dev(0, ptrs[a], nl, rp, rl.ctypes.data, k, C.byref(mo), d_tmp, k * nl, s1[at:].ctypes.data, C.byref(c)) == 0
                assert L.psx_ransac_homography_many_dev(0, d_tmp, s1[at:].ctypes.data, k, xptrs[a], nl, rxp, rl.ctypes.data, C.byref(ro),
                                                        C.byref(rs, at * RES_B), d_inl, cap, C.byref(c), None, None) == 0
                assert L.psx_guides_from_ransac(C.byref(rs, at * RES_B), k, capi.GUIDE_HOMOGRAPHY, 2.0, C.byref(gs, at * GUIDE_B)) == 0
                assert L.psx_match_pairs_guided_many_u8_dev(0, ptrs[a], xptrs[a], nl, rp, rxp, rl.ctypes.data, k, C.byref(gs, at * GUIDE_B), C.byref(mo),
                                                            d_re, k * nl, s3[at:].ctypes.data, C.byref(c)) == 0

        def per_edge():
            c = C.c_int()
            for e, (a, b) in enumerate(edges):
                nl, nr = int(lens[a]), int(lens[b])
                assert L.psx_match_pairs_u8_dev(0, ptrs[a], nl, ptrs[b], nr, C.byref(mo), d_tmp, nl, C.byref(c)) == 0
                assert L.psx_ransac_homography_dev(0, d_tmp, c.value, xptrs[a], nl, xptrs[b], nr, C.byref(ro), C.byref(re_[e]), d_inl, cap,
                                                   C.byref(c), None, None) == 0
                e3[e] = 0
                if re_[e].best >= 0:
                    g = capi.Guide.homography(list(re_[e].m), 2.0)
                    assert L.psx_match_pairs_guided_u8_dev(0, ptrs[a], xptrs[a], nl, ptrs[b], xptrs[b], nr, C.byref(g), C.byref(mo), d_re, nl, C.byref(c)) == 0
                    e3[e] = c.value

        t = alternate({"graph": graph, "stars": per_left, "edges": per_edge})
        assert bytes(rg) == bytes(rs) == bytes(re_) and np.array_equal(c1, s1) and np.array_equal(c3, s3) and np.array_equal(c3, e3)
        assert tot.value == c3.sum() > 0
        report("chain", t, tot.value)
    for p in bufs:
        L.psx_dev_free(0, p)
text = "\n".join(lines) + "\n"
print(text)
with open(OUT, "w") as f:
    f.write(text)
