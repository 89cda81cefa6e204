"""dev tool (GPU box): what the view shortlist costs beside what a caller has without it, on one MI355X.
Device-resident byte descriptor sets, W = 4096 words, 4 training iterations, k = 8:
  train / bags / lists   psx_vocab_train_u8_dev, psx_bow_u8_dev, psx_shortlist_views_dev: vocabulary, histogram, lists and
                         edges left in HBM
  shortlist + match      psx_shortlist_views_dev, the download of the edges, psx_match_pairs_graph_u8_dev on them
  all pairs              psx_match_pairs_graph_u8_dev on every pair a < b of the same views (ratio 0.8, mutual), what a caller
                         without a shortlist runs; measured for the two smaller shapes, for the larger ones extrapolated from
                         the measured time per edge of the shortlisted edges of the same shape and marked with '~'
run ALTERNATELY in one process: best of 5 after 2 warm-up rounds, host wall ms, the worst of the 5 in brackets.
  host reference         psx_*_ref on the host after the download of the descriptors (psx_dev_read), ONCE and for the smallest
                         shape only: the sequential definition takes seconds there and minutes on the larger shapes
The vocabulary is trained once per run on the views themselves and then applied; a caller with a fixed vocabulary pays
bags + lists per batch of views.
Shapes: 32 x 2048 rows, 64 x 2048, 512 x 2048, 2048 x 512; views in groups of 8 that see the same scene.
usage: python tools/shortlist_ms.py [out.txt]      (default profiles/shortlist_ms.txt)"""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from popsift_amd import capi

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "shortlist_ms.txt")
REPS, WARM = 5, 2
WORDS, ITERATIONS, K = 4096, 4, 8
SHAPES = ((32, 2048, True), (64, 2048, True), (512, 2048, False), (2048, 512, False))      # views, rows, all pairs measured


def views(seed, n, rows, group=8):
    """groups of `group` views: three quarters of a view's rows are noisy copies of its group's scene, the rest random"""
    rng = np.random.default_rng(seed)
    sets = []
    for g in range(0, n, group):
        scene = rng.integers(0, 256, (rows, 128), dtype=np.int16)
        for _ in range(min(group, n - g)):
            v = scene[rng.permutation(rows)] + rng.integers(-4, 5, (rows, 128), dtype=np.int16)
            v[rows * 3 // 4:] = rng.integers(0, 256, (rows - rows * 3 // 4, 128), dtype=np.int16)
            sets.append(np.clip(v, 0, 255).astype(np.uint8))
    return sets


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


def main():
    L = capi.lib()
    L.psx_dev_read.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]
    mo = capi.match_opts(0.8, True)
    vo = capi.VocabOpts(WORDS, ITERATIONS)
    so = capi.shortlist_opts(K)
    cell = lambda t: "%10.3f [%9.3f]" % t
    lines = ["shortlist_ms: the three calls of the view shortlist on device-resident byte sets (W = %d, T = %d, k = %d), everything left in HBM," % (WORDS, ITERATIONS, K),
             "beside psx_match_pairs_graph_u8_dev (ratio 0.8, mutual) on ALL pairs of the same views and on the shortlisted edges;",
             "alternating in one process, best of %d after %d warm-up rounds [worst of the %d], host wall ms; '~': extrapolated from the" % (REPS, WARM, REPS),
             "measured time per edge of the shortlisted edges of the same shape", ""]
    ref_lines = []
    for n, rows, measure_all in SHAPES:
        sets = views(n, n, rows)
        bufs = []
        ptrs = [p.value for p in capi._to_device(L, 0, sets, bufs)]
        lens = np.full((n,), rows, np.int32)
        M = n * rows
        all_edges = np.array([(a, b) for a in range(n) for b in range(a + 1, n)], np.int32)
        cap = (len(all_edges) if measure_all else n * K) * rows
        d_vocab, d_hist, d_nb, d_sc, d_edges, d_pairs = [p.value for p in capi._to_device(
            L, 0, [np.zeros(WORDS * 128, np.uint8), np.zeros(n * WORDS, np.uint32), np.zeros(n * K, np.int32), np.zeros(n * K, np.uint32),
                   np.zeros(2 * n * K, np.int32), np.zeros((cap, 4), np.int32)], bufs)]
        pa = (C.c_void_p * n)(*ptrs)
        info = capi.VocabInfo()
        count, total = C.c_int(), C.c_int()
        edges = np.zeros((n * K, 2), np.int32)
        ec = np.zeros(max(len(all_edges), n * K), np.int32)

        def train():
            assert L.psx_vocab_train_u8_dev(0, pa, lens.ctypes.data, n, C.byref(vo), d_vocab, C.byref(info)) == 0

        def bags():
            assert L.psx_bow_u8_dev(0, d_vocab, WORDS, pa, lens.ctypes.data, n, d_hist, None) == 0

        def lists():
            assert L.psx_shortlist_views_dev(0, d_hist, n, WORDS, C.byref(so), d_nb, d_sc, d_edges, n * K, C.byref(count)) == 0

        def match(ea, ne):
            assert L.psx_match_pairs_graph_u8_dev(0, pa, lens.ctypes.data, n, ea.ctypes.data, ne, C.byref(mo), d_pairs, cap, ec.ctypes.data,
                                                  C.byref(total)) == 0

        def lists_and_match():
            lists()
            assert L.psx_dev_read(0, edges.ctypes.data, d_edges, 8 * count.value) == 0
            match(edges, count.value)

        calls = {"train": train, "bags": bags, "lists": lists, "short": lists_and_match}
        if measure_all:
            calls["all"] = lambda: match(all_edges, len(all_edges))
        t = alternate(calls)
        ne = count.value
        nb = np.zeros((n, K), np.int32)
        assert L.psx_dev_read(0, nb.ctypes.data, d_nb, nb.nbytes) == 0
        mates = float(np.mean([np.sum(nb[i] // 8 == i // 8) for i in range(n)]))
        per_edge = (t["short"][0] - t["lists"][0]) / max(ne, 1)
        all_ms = cell(t["all"]) if measure_all else "~%9.1f %11s" % (per_edge * len(all_edges), "")
        lines += ["%d views x %d rows (%d rows, %d pairs in all, %d shortlisted, %.2f of a view's %d neighbours in its own group of 8):" % (
                      n, rows, M, len(all_edges), ne, mates, K),
                  "    psx_vocab_train_u8_dev   %s   (%d iterations ran)" % (cell(t["train"]), info.iterations),
                  "    psx_bow_u8_dev           %s" % cell(t["bags"]),
                  "    psx_shortlist_views_dev  %s" % cell(t["lists"]),
                  "    shortlist + match        %s   (%.2f us per matched edge)" % (cell(t["short"]), 1e3 * per_edge),
                  "    match ALL pairs          %s" % all_ms,
                  "    bags + shortlist + match %10.3f   against all pairs %s" % (t["bags"][0] + t["short"][0],
                                                                                 ("%.3f" % t["all"][0]) if measure_all else "~%.1f" % (per_edge * len(all_edges))), ""]
        if (n, rows) == SHAPES[0][:2]:
            # the host references, once: download, then the sequential definition
            host = [np.zeros_like(s) for s in sets]
            t0 = time.perf_counter()
            for h, p in zip(host, ptrs):
                assert L.psx_dev_read(0, h.ctypes.data, p, h.nbytes) == 0
            t_down = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            vocab, rinfo = capi.vocab_train_u8_ref(host, WORDS, ITERATIONS)
            t_train = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            hist = capi.bow_u8_ref(vocab, host)
            t_bags = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            ref = capi.shortlist_views_ref(hist, K)
            t_lists = (time.perf_counter() - t0) * 1e3
            g_vocab, g_hist = np.zeros_like(vocab), np.zeros_like(hist)
            assert L.psx_dev_read(0, g_vocab.ctypes.data, d_vocab, g_vocab.nbytes) == 0 and L.psx_dev_read(0, g_hist.ctypes.data, d_hist, g_hist.nbytes) == 0
            assert np.array_equal(g_vocab, vocab) and np.array_equal(g_hist, hist) and np.array_equal(nb, ref["neighbours"]) and ne == ref["count"]
            ref_lines = ["host references at %d x %d, run ONCE (the device results above equal them byte for byte): download of the descriptors %.1f ms," % (
                             n, rows, t_down),
                         "psx_vocab_train_u8_ref %.0f ms (%d iterations), psx_bow_u8_ref %.0f ms, psx_shortlist_views_ref %.1f ms" % (
                             t_train, rinfo["iterations"], t_bags, t_lists)]
        for p in bufs:
            L.psx_dev_free(0, p)
    text = "\n".join(lines + ref_lines) + "\n"
    print(text)
    with open(OUT, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
