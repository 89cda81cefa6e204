"""Cases of the view shortlist (include/popsift_hip.h, "WHICH PAIRS TO MATCH") and a plain-numpy restatement of its three
rules: integer k-means, bags of words, idf-weighted histogram intersection with top-k lists and the edge list.  Seeded
generators only.  The restatement takes its weights from psx_bow_weights, as the library and its reference do;
tests/test_shortlist_cpu.py holds that function to numpy on its own."""
import ctypes as C

import numpy as np

EDGE = np.dtype([("left", "<i4"), ("right", "<i4")])

# wave and workgroup edges, an empty view, view boundaries inside a workgroup
LENS = (1, 63, 64, 65, 0, 257, 300)
# the tile of 32 and the chunk of 512
WORDS = (2, 33, 511, 512, 513, 1025)


# ---- generators -------------------------------------------------------------------------------------------------------

def clustered(seed, lens, centres=12, spread=6):
    """views whose rows scatter around a few centres, with duplicate rows, an all-0 and an all-255 row"""
    rng = np.random.default_rng(seed)
    c = rng.integers(0, 256, (centres, 128))
    sets = []
    for n in lens:
        x = c[rng.integers(0, centres, n)] + rng.integers(-spread, spread + 1, (n, 128))
        sets.append(np.clip(x, 0, 255).astype(np.uint8))
    rows = [(v, r) for v, n in enumerate(lens) for r in range(n)]
    if len(rows) >= 8:
        pick = [rows[i] for i in rng.choice(len(rows), 8, replace=False)]
        sets[pick[0][0]][pick[0][1]] = 0
        sets[pick[1][0]][pick[1][1]] = 255
        for a, b in ((2, 3), (4, 5), (6, 7)):                       # duplicate rows: ties between equal distances
            sets[pick[a][0]][pick[a][1]] = sets[pick[b][0]][pick[b][1]]
    return sets


def vocabulary(seed, words):
    """random words with duplicates (ties go to the lower one), an all-0 and an all-255 word"""
    rng = np.random.default_rng(seed)
    v = rng.integers(0, 256, (words, 128)).astype(np.uint8)
    if words >= 2:
        v[0], v[words - 1] = 0, 255
    if words >= 6:
        v[words // 2] = v[1]
        v[words - 2] = v[2]
    return v


def bow_case(words):
    """(vocabulary, sets): some rows ARE words, so a duplicated word is an exact tie at distance 0"""
    sets = clustered(100 + words, LENS)
    v = vocabulary(200 + words, words)
    sets[5][3] = v[1]
    sets[6][299] = v[min(2, words - 1)]
    sets[1][0] = 255
    sets[3][64] = 0
    return v, sets


# name -> (lens, words, iterations); M = W exactly in the last two
TRAIN = {("w%d_t%d" % (w, t)): (LENS, w, t) for w in WORDS[:5] for t in (1, 40)}
TRAIN.update({"m_equals_w_t1": ((1000, 0, 25), 1025, 1), "m_equals_w_t40": ((40, 0, 25), 65, 40)})


def train_case(name):
    lens, words, iterations = TRAIN[name]
    return clustered(300 + words, lens), words, iterations


def hists(seed, n_views, words):
    """sparse random histograms with: two identical views, a view without rows, a pair of views with no common word"""
    rng = np.random.default_rng(seed)
    h = (rng.integers(0, 9, (n_views, words)) * (rng.random((n_views, words)) < 0.35)).astype(np.uint32)
    if n_views >= 2:
        h[1] = h[0]                                               # identical: equal scores against every third view
    if n_views >= 8:
        h[3] = 0                                                  # no rows
        h[5], h[6] = 0, 0                                         # disjoint supports: score 0
        h[5, :words // 2] = 3
        h[6, words // 2:] = 2
        h[7] = h[0]
    return h


# name -> (n_views, words, k, mutual)
SHORTLIST = {}
for _n, _w in ((1, 7), (2, 40), (33, 100), (65, 40)):
    for _k in (1, _n + 2):
        for _m in (False, True):
            SHORTLIST["n%d_k%d%s" % (_n, _k, "_mutual" if _m else "")] = (_n, _w, _k, _m)
SHORTLIST["n8_disjoint"] = (8, 10, 3, False)


def shortlist_case(name):
    n, w, k, mutual = SHORTLIST[name]
    return hists(400 + n, n, w), k, mutual


PLANTED = dict(groups=4, per_group=6, scene=400, seen=240, clutter=60, noise=3, words=256, iterations=8, k=5)


def planted(seed=7):
    """24 views in 4 groups of 6: most rows of a view are noisy copies of its group's scene descriptors, the rest random"""
    p = PLANTED
    rng = np.random.default_rng(seed)
    sets = []
    for g in range(p["groups"]):
        scene = rng.integers(0, 256, (p["scene"], 128))
        for _ in range(p["per_group"]):
            seen = scene[rng.choice(p["scene"], p["seen"], replace=False)] + rng.integers(-p["noise"], p["noise"] + 1, (p["seen"], 128))
            rows = np.concatenate([seen, rng.integers(0, 256, (p["clutter"], 128))])
            sets.append(np.clip(rows[rng.permutation(len(rows))], 0, 255).astype(np.uint8))
    return sets


def planted_mates(i):
    g = i // PLANTED["per_group"] * PLANTED["per_group"]
    return [j for j in range(g, g + PLANTED["per_group"]) if j != i]


# ---- the rules in numpy -----------------------------------------------------------------------------------------------

def assign(rows, vocab):
    """(word, distance) per row: the smallest (d, w); np.argmin returns the first minimum"""
    x, c = rows.astype(np.int64), vocab.astype(np.int64)
    d = (x * x).sum(1)[:, None] + (c * c).sum(1)[None, :] - 2 * (x @ c.T)
    a = np.argmin(d, axis=1)
    return a.astype(np.int32), d[np.arange(len(x)), a]


def train(sets, words, iterations):
    rows = np.concatenate([s.reshape(-1, 128) for s in sets])
    M = len(rows)
    vocab = rows[[w * M // words for w in range(words)]].copy()
    prev = np.full((M,), -1, np.int32)
    info = {}
    for it in range(1, iterations + 1):
        a, d = assign(rows, vocab)
        cnt = np.bincount(a, minlength=words).astype(np.int64)
        total = np.zeros((words, 128), np.int64)
        np.add.at(total, a, rows.astype(np.int64))
        info = dict(iterations=it, changed=int((a != prev).sum()), empty_words=int((cnt == 0).sum()), inertia=int(d.sum()))
        has = cnt > 0
        vocab[has] = ((2 * total[has] + cnt[has, None]) // (2 * cnt[has, None])).astype(np.uint8)
        prev = a
        if info["changed"] == 0:
            break
    return vocab, info


def bow(vocab, sets):
    hist = np.zeros((len(sets), len(vocab)), np.uint32)
    words = []
    for v, s in enumerate(sets):
        if len(s):
            a, _ = assign(s.reshape(-1, 128), vocab)
            hist[v] = np.bincount(a, minlength=len(vocab))
            words.append(a)
    return hist, (np.concatenate(words) if words else np.zeros((0,), np.int32))


def shortlist(capi, hist, k, mutual):
    """dict neighbours / scores / edges / count under the rule; the weights come from psx_bow_weights"""
    h = hist.astype(np.int64)
    N, W = h.shape
    nb = np.full((N, k), -1, np.int32)
    sc = np.zeros((N, k), np.uint32)
    if N == 0:
        return dict(neighbours=nb, scores=sc, edges=np.zeros((0,), EDGE), count=0)
    weight = capi.bow_weights((h > 0).sum(0), N).astype(np.int64)
    n = h.sum(1)
    q = np.where(n[:, None] > 0, h * 65535 // np.maximum(n, 1)[:, None], 0)
    listed = np.zeros((N, N), bool)
    for i in range(N):
        s = (weight[None, :] * np.minimum(q[i][None, :], q)).sum(1)
        cand = sorted((-int(s[j]), j) for j in range(N) if j != i and s[j] > 0)[:k]
        for r, (neg, j) in enumerate(cand):
            nb[i, r], sc[i, r], listed[i, j] = j, -neg, True
    keep = (listed & listed.T) if mutual else (listed | listed.T)
    edges = np.array([(a, b) for a in range(N) for b in range(a + 1, N) if keep[a, b]], EDGE).reshape(-1)
    return dict(neighbours=nb, scores=sc, edges=edges, count=len(edges))


# ---- raw calls on sentinel-filled host arrays (the _ref and the host forms) ---------------------------------------------

def ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None


def set_table(addresses, lens):
    k = len(lens)
    arr = (C.c_void_p * max(k, 1))(*addresses)
    la = np.ascontiguousarray(lens, dtype=np.int32)
    return (arr if k else None), la


def raw_train(capi, fn, addresses, lens, words, iterations, slack=64):
    """fn(sets, lens, n, opts, vocab, info) -> (rc, info bytes, vocabulary bytes with slack)"""
    arr, la = set_table(addresses, lens)
    vocab = np.full((max(words, 0) * 128 + slack,), 0xA5, np.uint8)
    info = capi.VocabInfo(-77, -77, -77, -77, 77)
    o = capi.VocabOpts(words, iterations)
    rc = fn(arr, ptr(la), len(lens), C.byref(o), ptr(vocab), C.byref(info))
    return rc, bytes(info), vocab


def raw_bow(capi, fn, vocab, addresses, lens, row_words=True, slack=5):
    """fn(vocab, words, sets, lens, n, hist, words_out) -> (rc, hist with slack, row words with slack)"""
    arr, la = set_table(addresses, lens)
    hist = np.full((len(lens) * len(vocab) + slack,), 0xA5A5A5A5, np.uint32)
    rw = np.full((int(sum(lens)) + slack,), -7, np.int32)
    rc = fn(ptr(vocab), len(vocab), arr, ptr(la), len(lens), ptr(hist), ptr(rw) if row_words else None)
    return rc, hist, rw


def raw_shortlist(capi, fn, hist, k, mutual, capacity, lists=True, slack=3):
    """fn(hist, n, words, opts, neighbours, scores, edges, capacity, count) on arrays filled with sentinels; capacity None:
    NULL with 0 -> (rc, count, neighbours, scores, edge words)"""
    N, W = hist.shape
    nb = np.full((N * k + slack,), -7, np.int32)
    sc = np.full((N * k + slack,), 0xA5A5A5A5, np.uint32)
    ed = np.full((2 * ((capacity or 0) + slack),), -7, np.int32)
    n = C.c_int(-77)
    o = capi.shortlist_opts(k, mutual)
    rc = fn(ptr(hist), N, W, C.byref(o), ptr(nb) if lists else None, ptr(sc) if lists else None, ptr(ed) if capacity is not None else None,
            capacity or 0, C.byref(n))
    return rc, n.value, nb, sc, ed


def addresses_of(sets):
    return [s.ctypes.data for s in sets]
