"""dev tool (GPU box): what the tracks call costs beside what a caller had to do without it, on one MI355X.
Device-resident inlier lists, left in HBM by psx_match_pairs_graph_u8_dev (ratio 0.8, mutual) ->
psx_ransac_homography_graph_dev (1024 hypotheses, refit, tol 2) on the planted views of tools/graph_chain_ms.py:
  device    psx_tracks_graph_dev( inlier buffer, results[e].inliers as counts ), labels / starts / members left in HBM  one call
  download  the inlier records to the host with the device-to-host copy the library always had (psx_dev_read)         } without
  host      that download, then a union-find on the host that gives the same labels, starts and members: a small C      } the call
            helper compiled from THIS file's source -- not psx_tracks_graph_ref, and no numpy or Python in the loop
run ALTERNATELY in one process (device, download, host, device, ...): best of 5 after 2 warm-up rounds, host wall ms, the
worst of the 5 in brackets.  min_views 2, conflicts dropped.  The tool asserts that the helper and the device call agree on
labels, starts and members, byte for byte.
Shapes: 32 views x 2048 rows, all pairs a < b (496 edges); 64 x 2048, each view against the 8 that follow (476); the star
2048 x (64 x 2048); one edge 2048 x 2048.
usage: python tools/tracks_ms.py [out.txt]      (default profiles/tracks_ms.txt)"""
import ctypes as C
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from popsift_amd import capi

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "tracks_ms.txt")
REPS, WARM = 5, 2
W, H = 1920.0, 1080.0
AMPS = np.array([2, 8, 16, 24, 32, 40])

# what a caller writes for themselves: union-find with path halving, the larger root under the smaller, then the tracks of
# at least two views without two members in one view, as labels and CSR
HELPER = r"""
#include <stdlib.h>
static int find(int* p, int x) { while (p[x] != x) { p[x] = p[p[x]]; x = p[x]; } return x; }
int host_tracks(const int* rec, const int* counts, const int* edges, int E, const int* off, int n_views, int* labels, int* starts, int* members,
                int* out_tracks, int* out_members)
{
    const int M = off[n_views];
    int* p = (int*)malloc(sizeof(int) * 5 * (size_t)(M > 0 ? M : 1));
    if (!p) return -1;
    int *size = p + M, *views = size + M, *last = views + M, *slot = last + M;
    for (int g = 0; g < M; g++) { p[g] = g; size[g] = 0; views[g] = 0; last[g] = -1; }
    long at = 0;
    for (int e = 0; e < E; e++)
        for (int i = 0; i < counts[e]; i++, at++) {
            int a = find(p, off[edges[2 * e]] + rec[4 * at]), b = find(p, off[edges[2 * e + 1]] + rec[4 * at + 1]);
            if (a == b) continue;
            if (a < b) p[b] = a; else p[a] = b;
        }
    int v = 0;
    for (int g = 0; g < M; g++) {
        while (off[v + 1] <= g) v++;
        const int r = find(p, g);
        size[r]++;
        if (last[r] == v) views[r] = -M; else { views[r]++; last[r] = v; }
    }
    int t = 0, m = 0;
    for (int r = 0; r < M; r++) {
        slot[r] = -1;
        if (p[r] != r || size[r] < 2 || views[r] < 2) continue;
        starts[t] = m; last[r] = t++; slot[r] = m; m += size[r];
    }
    starts[t] = m;
    v = 0;
    for (int g = 0; g < M; g++) {
        while (off[v + 1] <= g) v++;
        const int r = p[g] == g ? g : find(p, g);
        if (slot[r] < 0) { labels[g] = -1; continue; }
        labels[g] = last[r];
        members[2 * slot[r]] = v; members[2 * slot[r] + 1] = g - off[v]; slot[r]++;
    }
    *out_tracks = t; *out_members = m;
    free(p);
    return 0;
}
"""


def build_helper():
    d = tempfile.mkdtemp(prefix="tracks_ms_")
    src, so = os.path.join(d, "host_tracks.c"), os.path.join(d, "host_tracks.so")
    with open(src, "w") as f:
        f.write(HELPER)
    subprocess.check_call(["gcc", "-O2", "-shared", "-fPIC", src, "-o", so])
    lib = C.CDLL(so)
    lib.host_tracks.argtypes = [C.c_void_p] * 3 + [C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 5
    return lib.host_tracks


def views(seed, n, rows, first_is_base=False):
    """the planted views of tools/graph_chain_ms.py: half of a view's rows are noisy copies of base rows, seen from its camera"""
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
    yield "32 x 2048, all pairs", s, x, [(a, b) for a in range(32) for b in range(a + 1, 32)]
    s, x = views(64, 64, 2048)
    yield "64 x 2048, window 8", s, x, [(a, b) for a in range(64) for b in range(a + 1, min(a + 9, 64))]
    s, x = views(65, 65, 2048, first_is_base=True)
    yield "star 2048 x (64 x 2048)", s, x, [(0, b) for b in range(1, 65)]
    s, x = views(2, 2, 2048, first_is_base=True)
    yield "one edge 2048 x 2048", s, x, [(0, 1)]


def main():
    L = capi.lib()
    L.psx_dev_read.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]
    host_tracks = build_helper()
    mo = capi.match_opts(0.8, True)
    ro = capi.ransac_opts(2.0, 1024, 1, True)
    to = capi.track_opts(2, False)
    head = "%-24s %6s %8s %9s %20s %20s %20s %8s %8s %9s"
    row = "%-24s %6d %8d %9d %11.3f [%6.3f] %11.3f [%6.3f] %11.3f [%6.3f] %8d %8d %9d"
    lines = ["tracks_ms: psx_tracks_graph_dev on device-resident inlier lists (outputs left in HBM) beside what a caller does without it:",
             "the download of the records (psx_dev_read) and a host union-find in C that gives the same labels, starts and members;",
             "alternating in one process, best of %d after %d warm-up rounds [worst of the %d], host wall ms; min_views 2, conflicts dropped" % (REPS, WARM, REPS),
             "", head % ("shape", "edges", "nodes", "records", "device: one call", "download alone", "download + host", "tracks", "members", "conflicts"),
             head % ("", "", "", "", "ms", "ms", "ms", "", "", "")]
    for name, sets, xys, edges in shapes():
        bufs = []
        ns, ne = len(sets), len(edges)
        ptrs = [p.value for p in capi._to_device(L, 0, sets, bufs)]
        xptrs = [p.value for p in capi._to_device(L, 0, xys, bufs)]
        lens = np.array([len(s) for s in sets], np.int32)
        M = int(lens.sum())
        cap = int(sum(lens[a] for a, _ in edges))
        d_pairs, d_inl = [p.value for p in capi._to_device(L, 0, [np.zeros((cap, 4), np.int32)] * 2, bufs)]
        d_lab, d_st, d_mem = [p.value for p in capi._to_device(L, 0, [np.zeros(M, np.int32), np.zeros(M // 2 + 1, np.int32), np.zeros(2 * M, np.int32)], bufs)]
        pa, xa = (C.c_void_p * ns)(*ptrs), (C.c_void_p * ns)(*xptrs)
        ea = np.ascontiguousarray(edges, np.int32)
        ec = np.zeros(ne, np.int32)
        n = C.c_int()
        res = (capi.RansacResult * ne)()
        assert L.psx_match_pairs_graph_u8_dev(0, pa, lens.ctypes.data, ns, ea.ctypes.data, ne, C.byref(mo), d_pairs, cap, ec.ctypes.data, C.byref(n)) == 0
        assert L.psx_ransac_homography_graph_dev(0, d_pairs, ec.ctypes.data, ea.ctypes.data, ne, xa, lens.ctypes.data, ns, C.byref(ro), res, d_inl, cap,
                                                 C.byref(n), None, None) == 0
        ic = np.array([r.inliers for r in res], np.int32)
        total = int(ic.sum())
        assert total == n.value > 0
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        info = capi.TracksInfo()
        rec = np.zeros((total, 4), np.int32)
        h_lab, h_st, h_mem = np.zeros(M, np.int32), np.zeros(M // 2 + 1, np.int32), np.zeros(2 * M, np.int32)
        ht, hm = C.c_int(), C.c_int()

        def device():
            assert L.psx_tracks_graph_dev(0, d_inl, ic.ctypes.data, ea.ctypes.data, ne, lens.ctypes.data, ns, C.byref(to), d_lab, d_st, M // 2, d_mem, M,
                                          C.byref(info)) == 0

        def download():
            assert L.psx_dev_read(0, rec.ctypes.data, d_inl, 16 * total) == 0

        def host():
            download()
            assert host_tracks(rec.ctypes.data, ic.ctypes.data, ea.ctypes.data, ne, off.ctypes.data, ns, h_lab.ctypes.data, h_st.ctypes.data,
                               h_mem.ctypes.data, C.byref(ht), C.byref(hm)) == 0

        t = alternate({"device": device, "download": download, "host": host})
        # the two agree, byte for byte
        g_lab, g_st, g_mem = np.zeros(M, np.int32), np.zeros(info.tracks + 1, np.int32), np.zeros(2 * info.members, np.int32)
        for arr, p in ((g_lab, d_lab), (g_st, d_st), (g_mem, d_mem)):
            assert L.psx_dev_read(0, arr.ctypes.data, p, arr.nbytes) == 0
        assert (ht.value, hm.value) == (info.tracks, info.members) and info.tracks > 0
        assert np.array_equal(g_lab, h_lab) and np.array_equal(g_st, h_st[:info.tracks + 1]) and np.array_equal(g_mem, h_mem[:2 * info.members])
        lines.append(row % (name, ne, M, total, t["device"][0], t["device"][1], t["download"][0], t["download"][1], t["host"][0], t["host"][1],
                            info.tracks, info.members, info.conflicts))
        for p in bufs:
            L.psx_dev_free(0, p)
    text = "\n".join(lines) + "\n"
    print(text)
    with open(OUT, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
