"""dev tool (GPU box): what the float edge-list calls cost beside the loops they replace, on one MI355X; the protocol of
tools/match_graph_ms.py.  Device-resident planted float descriptors, rows normalised to 512, ratio 0.8 with PSX_PAIRS_MUTUAL,
records into device buffers (the _dev forms):
  graph  psx_match_pairs_graph_dev( sets, edges )                           one call
  stars  psx_match_pairs_many_dev( L, {R ...} ) per left view of the list   one call per left view  } code this change does not
  edges  psx_match_pairs_dev( L, R ) per edge                               one call per edge       } add: the baselines
run ALTERNATELY in one process (graph, stars, edges, graph, ...): best of 5 after 2 warm-up rounds, host wall ms for the
whole edge list, the worst of the 5 in brackets.  The edge lists are grouped by left, so the per-edge counts of the three must
agree entry by entry: the tool asserts it.  Per shape also: the one call with POPSIFT_MATCH_MFMA=0 (the exact scan; a child
process, the switch is read once per thread's scratch), and from a child with POPSIFT_MATCH_STATS set what the prefilter
prints -- the chunk length, the candidates per (left, edge), the fullest segment of 32 slots, whether the call fell back.
Shapes: 32 views x 2048 rows, all pairs a < b (496 edges); 16 x 4096, all pairs (120); 64 x 2048, each view against the 8
that follow (476); the star 2048 x (64 x 2048), where `stars` is ONE one-to-many call; one edge 18 432 x 18 432, where
`stars` and `edges` are one call each.
Then the guided float forms at 32 x 2048 all pairs and at the star, every edge under a window guide, beside the loop of
psx_match_pairs_guided_dev per edge.
With --parent LIB (a libpopsift_hip.so built from the parent commit): the three existing calls whose kernels' text moved
into headers, alternating that library and this one in one process -- psx_match_pairs_many_dev at 2048 x (64 x 2048),
psx_match_pairs_graph_u8_dev and psx_match_pairs_guided_graph_u8_dev at 32 x 2048 all pairs.
usage: python tools/match_graph_f32_ms.py [out.txt] [--parent LIB]      (default profiles/match_graph_f32_ms.txt)"""
import ctypes as C
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from popsift_amd import capi

ARGS = [a for a in sys.argv[1:]]
PARENT = ARGS[ARGS.index("--parent") + 1] if "--parent" in ARGS else None
CHILD = ARGS[ARGS.index("--child") + 1] if "--child" in ARGS else None
for flag in ("--parent", "--child"):
    if flag in ARGS:
        i = ARGS.index(flag)
        del ARGS[i:i + 2]
OUT = ARGS[0] if ARGS else os.path.join(ROOT, "profiles", "match_graph_f32_ms.txt")
REPS, WARM = 5, 2
AMPS = np.array([2, 8, 16, 24, 32, 40])


def views(seed, n, rows, base_rows):
    """the base set and n views of `rows` rows, half of them noisy copies of base rows (uint8), with positions: a copy
    lies within a pixel of its base row's place, every other row anywhere on a 640 x 480 canvas"""
    r0 = np.random.default_rng(seed)
    base = r0.integers(0, 64, (base_rows, 128), dtype=np.uint8)
    base_xy = r0.uniform([0.0, 0.0], [640.0, 480.0], (base_rows, 2))
    out, xys = [], []
    for s in range(n):
        rng = np.random.default_rng([seed, s + 1])
        v = rng.integers(0, 64, (rows, 128), dtype=np.uint8)
        xy = rng.uniform([0.0, 0.0], [640.0, 480.0], (rows, 2))
        m = min(base_rows, rows) // 2
        src, dst = rng.permutation(base_rows)[:m], rng.permutation(rows)[:m]
        amp = AMPS[np.arange(m) % 6][:, None]
        noise = (rng.random((m, 128)) * (2 * amp + 1)).astype(np.int64) - amp
        v[dst] = np.clip(base[src].astype(np.int64) + noise, 0, 255).astype(np.uint8)
        xy[dst] = base_xy[src] + rng.uniform(-0.7, 0.7, (m, 2))
        out.append(v)
        xys.append(xy.astype(np.float32))
    return base, base_xy.astype(np.float32), out, xys


def norm512(a):
    f = np.ascontiguousarray(a, np.float32)
    n = np.sqrt((f * f).sum(axis=1, dtype=np.float32)).astype(np.float32)
    return np.ascontiguousarray(f / n[:, None] * np.float32(512.0), np.float32)


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


def shapes(which=None):
    """(name, byte sets, positions, edges)"""
    if which in (None, 0):
        _, _, v, x = views(32, 32, 2048, 2048)
        yield "32 x 2048, all pairs", v, x, [(a, b) for a in range(32) for b in range(a + 1, 32)]
    if which in (None, 1):
        _, _, v, x = views(16, 16, 4096, 4096)
        yield "16 x 4096, all pairs", v, x, [(a, b) for a in range(16) for b in range(a + 1, 16)]
    if which in (None, 2):
        _, _, v, x = views(64, 64, 2048, 2048)
        yield "64 x 2048, window 8", v, x, [(a, b) for a in range(64) for b in range(a + 1, min(a + 9, 64))]
    if which in (None, 3):
        base, bx, v, x = views(2048 + 64, 64, 2048, 2048)
        yield "star 2048 x (64 x 2048)", [base] + v, [bx] + x, [(0, b) for b in range(1, 65)]
    if which in (None, 4):
        base, bx, v, x = views(18432 + 1, 1, 18432, 18432)
        yield "one edge 18432 x 18432", [base] + v, [bx] + x, [(0, 1)]


def grouped(edges, ptrs, lens):
    """the list grouped by left: (left, first edge, its rights as a pointer array, their lengths)"""
    stars, at, ne = [], 0, len(edges)
    while at < ne:
        a, end = edges[at][0], at
        while end < ne and edges[end][0] == a:
            end += 1
        bs = [b for _, b in edges[at:end]]
        stars.append((a, at, (C.c_void_p * len(bs))(*[ptrs[b].value for b in bs]), np.array([lens[b] for b in bs], np.int32), bs))
        at = end
    return stars


L = capi.lib()
o = capi.match_opts(0.8, True)


def upload(sets, edges, bufs):
    ptrs = capi._to_device(L, 0, sets, bufs)
    lens = np.array([len(s) for s in sets], np.int32)
    cap = int(sum(lens[a] for a, _ in edges))
    out = capi._to_device(L, 0, [np.zeros((cap, 4), np.int32)], bufs)[0]
    pa = (C.c_void_p * len(sets))(*[p.value for p in ptrs])
    return ptrs, lens, cap, out, pa


def child_main():
    """--child mfma0: {shape: [best, worst, path]} of the one call; --child stats: the one call once per shape"""
    res = {}
    for name, sets, _, edges in shapes():
        bufs = []
        ptrs, lens, cap, out, pa = upload([norm512(s) for s in sets], edges, bufs)
        ea = np.ascontiguousarray(edges, np.int32)
        counts, n = np.zeros(len(edges), np.int32), C.c_int()

        def graph():
            assert L.psx_match_pairs_graph_dev(0, pa, lens.ctypes.data, len(sets), ea.ctypes.data, len(edges), C.byref(o), out, cap,
                                               counts.ctypes.data, C.byref(n)) == 0
        if CHILD == "stats":
            sys.stderr.write("shape: %s\n" % name)
            sys.stderr.flush()
            graph()
            res[name] = capi.match_graph_f32_last()
        else:
            t = alternate({"graph": graph})
            res[name] = [t["graph"][0], t["graph"][1], capi.match_graph_f32_last()["path"], int(n.value)]
        for p in bufs:
            L.psx_dev_free(0, p)
    print(json.dumps(res))


def run_child(mode, env_add):
    env = dict(os.environ, **env_add)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env)
    if p.returncode != 0:
        raise SystemExit("child %s failed (%d):\n%s" % (mode, p.returncode, p.stderr[-3000:]))
    return json.loads(p.stdout.strip().splitlines()[-1]), p.stderr


def main():
    mfma0, _ = run_child("mfma0", {"POPSIFT_MATCH_MFMA": "0"})
    stats, err = run_child("stats", {"POPSIFT_MATCH_STATS": "1"})
    seen, cur = {}, None
    for line in err.splitlines():
        if line.startswith("shape: "):
            cur = line[7:]
        m = re.search(r"chunk length (\d+), candidates per \(left, edge\): mean ([0-9.]+), max (\d+); fullest segment (\d+) of (\d+)(.*)", line)
        if m and cur:
            seen[cur] = (int(m.group(1)), float(m.group(2)), int(m.group(3)), int(m.group(4)), "yes" if "exact scan" in m.group(6) else "no")
    lines = ["match_graph_f32_ms: psx_match_pairs_graph_dev beside the loop of psx_match_pairs_many_dev per left view and the loop of",
             "psx_match_pairs_dev per edge; float descriptors, rows of norm 512, ratio 0.8, mutual, device in / device out; alternating in one",
             "process, best of %d after %d warm-up rounds [worst of the %d], host wall ms for the whole edge list; `scan`: the one call with" % (REPS, WARM, REPS),
             "POPSIFT_MATCH_MFMA=0 in a process of its own; candidates: per (left row, edge) over the forward direction, from POPSIFT_MATCH_STATS", "",
             "%-24s %5s %5s %4s %19s %19s %19s %19s %7s %6s %5s %5s %5s %8s" % ("shape", "edges", "lefts", "path", "graph: one call", "stars: per left",
                                                                                  "edges: per edge", "scan: one call", "chunk", "cand", "cand", "full", "fell", "pairs"),
             "%-24s %5s %5s %4s %19s %19s %19s %19s %7s %6s %5s %5s %5s" % ("", "", "", "", "ms", "ms", "ms", "ms", "rows", "mean", "max", "seg", "back")]
    guided = []
    for idx, (name, sets, xys, edges) in enumerate(shapes()):
        bufs = []
        fsets = [norm512(s) for s in sets]
        ptrs, lens, cap, out, pa = upload(fsets, edges, bufs)
        ne = len(edges)
        ea = np.ascontiguousarray(edges, np.int32)
        g_counts, s_counts, e_counts = np.zeros(ne, np.int32), np.zeros(ne, np.int32), np.zeros(ne, np.int32)
        n = C.c_int()
        stars = grouped(edges, ptrs, lens)

        def graph():
            assert L.psx_match_pairs_graph_dev(0, pa, lens.ctypes.data, len(sets), ea.ctypes.data, ne, C.byref(o), out, cap, g_counts.ctypes.data, C.byref(n)) == 0

        def per_left():
            c = C.c_int()
            for a, at, rp, rl, _ in stars:
                k = len(rl)
                assert L.psx_match_pairs_many_dev(0, ptrs[a], int(lens[a]), rp, rl.ctypes.data, k, C.byref(o), out, k * int(lens[a]),
                                                  s_counts[at:].ctypes.data, C.byref(c)) == 0

        def per_edge():
            c = C.c_int()
            for e, (a, b) in enumerate(edges):
                assert L.psx_match_pairs_dev(0, ptrs[a], int(lens[a]), ptrs[b], int(lens[b]), C.byref(o), out, int(lens[a]), C.byref(c)) == 0
                e_counts[e] = c.value

        t = alternate({"graph": graph, "stars": per_left, "edges": per_edge})
        info = capi.match_graph_f32_last()
        assert np.array_equal(g_counts, s_counts) and np.array_equal(g_counts, e_counts) and n.value == g_counts.sum() > 0
        assert info["fell_back"] == 0 or seen.get(name, (0, 0, 0, 0, "no"))[4] == "yes"
        sc = mfma0[name]
        assert sc[2] == 1 and sc[3] == n.value
        st = seen.get(name, (0, 0.0, 0, 0, "-"))
        lines.append("%-24s %5d %5d %4d %10.3f [%6.3f] %10.3f [%6.3f] %10.3f [%6.3f] %10.3f [%6.3f] %7d %6.1f %5d %5d %5s %8d" %
                     (name, ne, len(stars), info["path"], t["graph"][0], t["graph"][1], t["stars"][0], t["stars"][1], t["edges"][0], t["edges"][1],
                      sc[0], sc[1], st[0], st[1], st[2], st[3], "yes" if info["fell_back"] else st[4], n.value))
        if idx in (0, 3):
            # the guided float forms: every edge under a window of 2 px (identity H), the positions of views()
            xp = capi._to_device(L, 0, [np.ascontiguousarray(x, np.float32) for x in xys], bufs)
            xa = (C.c_void_p * len(sets))(*[p.value for p in xp])
            win = capi.Guide.make(capi.GUIDE_HOMOGRAPHY, np.eye(3, dtype=np.float32).reshape(9), 2.0)
            ga = (capi.Guide * ne)(*([win] * ne))
            gg_counts, ge_counts, gs_counts = np.zeros(ne, np.int32), np.zeros(ne, np.int32), np.zeros(ne, np.int32)
            gn = C.c_int()

            def g_graph():
                assert L.psx_match_pairs_guided_graph_dev(0, pa, xa, lens.ctypes.data, len(sets), ea.ctypes.data, ne, ga, C.byref(o), out, cap,
                                                          gg_counts.ctypes.data, C.byref(gn)) == 0

            def g_left():
                c = C.c_int()
                for a, at, rp, rl, bs in stars:
                    k = len(rl)
                    xr = (C.c_void_p * k)(*[xp[b].value for b in bs])
                    assert L.psx_match_pairs_guided_many_dev(0, ptrs[a], xp[a], int(lens[a]), rp, xr, rl.ctypes.data, k, ga, C.byref(o), out,
                                                             k * int(lens[a]), gs_counts[at:].ctypes.data, C.byref(c)) == 0

            def g_edge():
                c = C.c_int()
                for e, (a, b) in enumerate(edges):
                    assert L.psx_match_pairs_guided_dev(0, ptrs[a], xp[a], int(lens[a]), ptrs[b], xp[b], int(lens[b]), C.byref(win), C.byref(o), out,
                                                        int(lens[a]), C.byref(c)) == 0
                    ge_counts[e] = c.value

            tg = alternate({"graph": g_graph, "stars": g_left, "edges": g_edge})
            assert np.array_equal(gg_counts, ge_counts) and np.array_equal(gg_counts, gs_counts) and gn.value == gg_counts.sum() > 0
            guided.append("%-24s %5d %5d %10.3f [%6.3f] %10.3f [%6.3f] %10.3f [%6.3f] %8d" %
                          (name, ne, len(stars), tg["graph"][0], tg["graph"][1], tg["stars"][0], tg["stars"][1], tg["edges"][0], tg["edges"][1], gn.value))
        for p in bufs:
            L.psx_dev_free(0, p)
    lines += ["", "the guided float forms, every edge under a window guide (identity H, 2 px): psx_match_pairs_guided_graph_dev beside the loop of",
              "psx_match_pairs_guided_many_dev per left view and the loop of psx_match_pairs_guided_dev per edge; same protocol", "",
              "%-24s %5s %5s %19s %19s %19s %8s" % ("shape", "edges", "lefts", "graph: one call", "stars: per left", "edges: per edge", "pairs")] + guided
    if PARENT:
        lines += [""] + moved_calls()
    text = "\n".join(lines) + "\n"
    print(text)
    with open(OUT, "w") as f:
        f.write(text)


def moved_calls():
    """the existing calls whose kernels' text moved into headers: the parent commit's library and this one, alternating"""
    P = C.CDLL(PARENT)
    names = ("psx_match_pairs_many_dev", "psx_match_pairs_graph_u8_dev", "psx_match_pairs_guided_graph_u8_dev")
    for nm in names:
        getattr(P, nm).argtypes = getattr(L, nm).argtypes
    rows = ["existing calls whose device code moved into shared headers: the parent commit's library and this one, alternating in one process,",
            "best of %d after %d warm-up rounds [worst], host wall ms; the new best is to lie within the parent's best-to-worst spread" % (REPS, WARM), "",
            "%-58s %19s %19s %8s" % ("call", "parent", "this", "within")]
    # psx_match_pairs_many_dev at 2048 x (64 x 2048), float
    base, _, v, _ = views(2048 + 64, 64, 2048, 2048)
    bufs = []
    ptrs = capi._to_device(L, 0, [norm512(base)] + [norm512(s) for s in v], bufs)
    out = capi._to_device(L, 0, [np.zeros((64 * 2048, 4), np.int32)], bufs)[0]
    rp = (C.c_void_p * 64)(*[p.value for p in ptrs[1:]])
    rl = np.full(64, 2048, np.int32)
    cnt = {k: np.zeros(64, np.int32) for k in "pt"}
    c = C.c_int()

    def many(lib, key):
        return lambda: lib.psx_match_pairs_many_dev(0, ptrs[0], 2048, rp, rl.ctypes.data, 64, C.byref(o), out, 64 * 2048, cnt[key].ctypes.data, C.byref(c))
    t = alternate({"parent": many(P, "p"), "this": many(L, "t")})
    assert np.array_equal(cnt["p"], cnt["t"]) and cnt["t"].sum() > 0
    rows.append(fmt_moved("psx_match_pairs_many_dev, 2048 x (64 x 2048), float", t))
    for p in bufs:
        L.psx_dev_free(0, p)
    # the byte edge-list calls at 32 x 2048, all pairs
    _, _, v, x = views(32, 32, 2048, 2048)
    edges = [(a, b) for a in range(32) for b in range(a + 1, 32)]
    bufs = []
    ptrs, lens, cap, out, pa = upload(v, edges, bufs)
    xp = capi._to_device(L, 0, x, bufs)
    xa = (C.c_void_p * 32)(*[p.value for p in xp])
    ea = np.ascontiguousarray(edges, np.int32)
    ne = len(edges)
    win = capi.Guide.make(capi.GUIDE_HOMOGRAPHY, np.eye(3, dtype=np.float32).reshape(9), 2.0)
    ga = (capi.Guide * ne)(*([win] * ne))
    cnt = {k: np.zeros(ne, np.int32) for k in "pt"}

    def graph(lib, key):
        return lambda: lib.psx_match_pairs_graph_u8_dev(0, pa, lens.ctypes.data, 32, ea.ctypes.data, ne, C.byref(o), out, cap, cnt[key].ctypes.data, C.byref(c))

    def gguided(lib, key):
        return lambda: lib.psx_match_pairs_guided_graph_u8_dev(0, pa, xa, lens.ctypes.data, 32, ea.ctypes.data, ne, ga, C.byref(o), out, cap,
                                                               cnt[key].ctypes.data, C.byref(c))
    t = alternate({"parent": graph(P, "p"), "this": graph(L, "t")})
    assert np.array_equal(cnt["p"], cnt["t"]) and cnt["t"].sum() > 0
    rows.append(fmt_moved("psx_match_pairs_graph_u8_dev, 32 x 2048 all pairs", t))
    t = alternate({"parent": gguided(P, "p"), "this": gguided(L, "t")})
    assert np.array_equal(cnt["p"], cnt["t"]) and cnt["t"].sum() > 0
    rows.append(fmt_moved("psx_match_pairs_guided_graph_u8_dev, 32 x 2048 all pairs", t))
    for p in bufs:
        L.psx_dev_free(0, p)
    return rows


def fmt_moved(name, t):
    return "%-58s %10.3f [%6.3f] %10.3f [%6.3f] %8s" % (name, t["parent"][0], t["parent"][1], t["this"][0], t["this"][1],
                                                       "yes" if t["this"][0] <= t["parent"][1] else "NO")


if __name__ == "__main__":
    child_main() if CHILD else main()
