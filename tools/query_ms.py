"""dev tool (GPU box): what ranking a few arriving views against a database of stored ones costs, beside what a caller has
without it, on one MI355X.  W = 4096 words, k = 8; 4096 views of 256 rows from the planted generator of tools/shortlist_ms.py
(groups of 8 that see the same scene), one vocabulary trained on them (4 iterations), their bags left in HBM.  For n_db in
{512, 2048, 4032} stored views and Q in {1, 8, 64} arriving ones, run ALTERNATELY in one process, best of 5 after 2 warm-up
rounds, host wall ms, the worst of the 5 in brackets:
  query        psx_shortlist_query_dev: the Q rows behind the first n_db rows of q against those n_db, neighbours, scores and
               edges left in HBM; the weights are psx_bow_weights of the n_db stored views' df
  quantise Q   psx_bow_quantize_dev of the Q arriving histograms alone (no df): with `query`, what an arrival costs
  all pairs    what a caller does without the query: psx_shortlist_views_dev over the n_db + Q histograms.  That call's code
               is untouched since the commit before the query was added, so this IS that commit's call
and once per n_db: psx_bow_quantize_dev of the n_db stored rows with df (what building the database costs, once).
Also n_db = 65 536: the 4096 quantised rows repeated 16 times (512 MB of q).  psx_shortlist_views_dev refuses that size, so
there is no baseline.
usage: python tools/query_ms.py [out.txt]      (default profiles/query_ms.txt)"""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from popsift_amd import capi
from tools.shortlist_ms import alternate, views, REPS, WARM

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "query_ms.txt")
WORDS, ITERATIONS, K = 4096, 4, 8
VIEWS, ROWS = 4096, 256
N_DB, QUERIES = (512, 2048, 4032), (1, 8, 64)
BIG, BIG_COPIES = 65536, 16


def main():
    L = capi.lib()
    L.psx_dev_read.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]
    L.psx_dev_write.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]
    cell = lambda t: "%10.3f [%9.3f]" % t
    sets = views(VIEWS, VIEWS, ROWS)
    bufs = []
    ptrs = [p.value for p in capi._to_device(L, 0, sets, bufs)]
    lens = np.full((VIEWS,), ROWS, np.int32)
    d_vocab, d_hist, d_q, d_qq, d_nb, d_sc, d_edges = [p.value for p in capi._to_device(
        L, 0, [np.zeros(WORDS * 128, np.uint8), np.zeros(VIEWS * WORDS, np.uint32), np.zeros(VIEWS * WORDS, np.uint16),
               np.zeros(max(QUERIES) * WORDS, np.uint16), np.zeros(VIEWS * K, np.int32), np.zeros(VIEWS * K, np.uint32),
               np.zeros(2 * VIEWS * K, np.int32)], bufs)]
    info = capi.vocab_train_u8_dev(ptrs, lens, WORDS, ITERATIONS, d_vocab)
    capi.bow_u8_dev(d_vocab, WORDS, ptrs, lens, d_hist)
    capi.bow_quantize_dev(d_hist, VIEWS, WORDS, d_q)
    so = capi.shortlist_opts(K)
    count = C.c_int()
    lines = ["query_ms: psx_shortlist_query_dev (W = %d, k = %d) of Q arriving views against n_db stored ones, everything in HBM, beside" % (WORDS, K),
             "psx_shortlist_views_dev over the n_db + Q histograms (all pairs again: what a caller without the query runs; that call's code is",
             "unchanged, so it is the previous commit's); %d planted views x %d rows, vocabulary trained in %d iterations;" % (VIEWS, ROWS, info["iterations"]),
             "alternating in one process, best of %d after %d warm-up rounds [worst of the %d], host wall ms" % (REPS, WARM, REPS), ""]
    weights = None
    for n_db in N_DB:
        df = np.zeros((WORDS,), np.int32)
        capi.bow_quantize_dev(d_hist, n_db, WORDS, d_q, df)
        weights = capi.bow_weights(df, n_db)
        wp = weights.ctypes.data_as(C.c_void_p)
        scratch_df = np.zeros((WORDS,), np.int32)
        calls = {"build": lambda: capi.bow_quantize_dev(d_hist, n_db, WORDS, d_q, scratch_df)}
        for Q in QUERIES:
            o = capi.query_opts(K, edge_base=n_db)

            def query(Q=Q, o=o):
                assert L.psx_shortlist_query_dev(0, d_q, n_db, d_q + 2 * n_db * WORDS, Q, WORDS, wp, None, C.byref(o), d_nb, d_sc, d_edges, Q * K,
                                                 C.byref(count)) == 0

            def quantise(Q=Q):
                assert L.psx_bow_quantize_dev(0, d_hist + 4 * n_db * WORDS, Q, WORDS, d_qq, None) == 0

            def all_pairs(Q=Q):
                assert L.psx_shortlist_views_dev(0, d_hist, n_db + Q, WORDS, C.byref(so), d_nb, d_sc, d_edges, (n_db + Q) * K, C.byref(count)) == 0

            calls.update({"query%d" % Q: query, "quant%d" % Q: quantise, "all%d" % Q: all_pairs})
        t = alternate(calls)
        plan = capi.shortlist_query_plan(n_db, 64, WORDS, K)
        lines += ["n_db = %d stored views (psx_bow_quantize_dev of the %d rows with df: %s; at Q = 64: %d blocks, %d keys between the kernels):" % (
                      n_db, n_db, cell(t["build"]).strip(), plan["blocks"], plan["partial_keys"]),
                  "      Q   psx_shortlist_query_dev   psx_bow_quantize_dev (Q)   psx_shortlist_views_dev (n_db + Q)   all pairs / (quantise + query)"]
        for Q in QUERIES:
            a, b, c = t["query%d" % Q], t["quant%d" % Q], t["all%d" % Q]
            lines.append("   %4d   %s   %s   %s   %6.1f" % (Q, cell(a), cell(b), cell(c), c[0] / (a[0] + b[0])))
        lines.append("")
    # 65 536 stored views: the 4096 quantised rows, repeated
    block = np.zeros((VIEWS * WORDS,), np.uint16)
    assert L.psx_dev_read(0, block.ctypes.data, d_q, block.nbytes) == 0
    big = C.c_void_p()
    assert L.psx_dev_alloc(0, BIG * WORDS * 2, C.byref(big)) == 0
    bufs.append(big)
    for c in range(BIG_COPIES):
        assert L.psx_dev_write(0, big.value + c * block.nbytes, block.ctypes.data, block.nbytes) == 0
    wp = weights.ctypes.data_as(C.c_void_p)
    calls = {}
    for Q in QUERIES:
        o = capi.query_opts(K, edge_base=BIG)

        def query(Q=Q, o=o):
            assert L.psx_shortlist_query_dev(0, big, BIG, d_q + 2 * N_DB[-1] * WORDS, Q, WORDS, wp, None, C.byref(o), d_nb, d_sc, d_edges, Q * K,
                                             C.byref(count)) == 0

        calls["query%d" % Q] = query
    t = alternate(calls)
    plan = capi.shortlist_query_plan(BIG, 64, WORDS, K)
    lines += ["n_db = %d stored views (the %d quantised rows repeated %d times, %d MB of q; at Q = 64: %d blocks, %d keys between the kernels);" % (
                  BIG, VIEWS, BIG_COPIES, BIG * WORDS * 2 >> 20, plan["blocks"], plan["partial_keys"]),
              "no baseline: psx_shortlist_views_dev refuses more than 4096 views",
              "      Q   psx_shortlist_query_dev"]
    lines += ["   %4d   %s" % (Q, cell(t["query%d" % Q])) for Q in QUERIES]
    for p in bufs:
        L.psx_dev_free(0, p)
    text = "\n".join(lines) + "\n"
    print(text)
    with open(OUT, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
