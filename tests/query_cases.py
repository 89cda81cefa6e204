"""Cases of the database query (include/popsift_hip.h, "QUERY A DATABASE OF VIEWS") and a plain-numpy restatement of its two
rules: the quantisation of a histogram row by its own sum, and the k best stored views per query with limits, a self index, a
least score and the edge list in list order.  Seeded generators only; the histograms come from tests/shortlist_cases.py."""
import ctypes as C
import itertools

import numpy as np

from tests import shortlist_cases as sc

EDGE = sc.EDGE
MAX_VIEWS = 1 << 20
TILE = 64

# the tile of 64 on either side, the 32-word step, k below, at and above the 64 keys of a block list
N_DB = (1, 63, 64, 65, 130)
N_QUERIES = (1, 5, 65)
WORDS = (1, 31, 33, 100)
KS = (1, 3, 70)


# ---- the rules in numpy -----------------------------------------------------------------------------------------------

def quantize(hist):
    """(q uint16, df int64): every row by its own sum, 0 for an empty row"""
    h = np.asarray(hist).astype(np.int64)
    n = h.sum(1)
    q = np.where(n[:, None] > 0, h * 65535 // np.maximum(n, 1)[:, None], 0)
    return q.astype(np.uint16), (h > 0).sum(0)


def scores_of(db, query_row, weights):
    """unsigned 32-bit sums, as every form adds them"""
    s = (np.asarray(weights, np.int64)[None, :] * np.minimum(query_row.astype(np.int64)[None, :], db.astype(np.int64))).sum(1)
    return s & 0xffffffff


def query(db, qq, weights, k, db_limit=None, self_base=-1, edge_base=0, min_score=0):
    """dict neighbours / scores / edges / count under the rule"""
    n_db, nq = len(db), len(qq)
    nb = np.full((nq, k), -1, np.int32)
    scr = np.zeros((nq, k), np.uint32)
    edges = []
    j = np.arange(n_db)
    for i in range(nq):
        limit = n_db if db_limit is None else int(db_limit[i])
        s = scores_of(db, qq[i], weights) if n_db else np.zeros((0,), np.int64)
        cand = (j < limit) & (s > 0) & (s >= min_score)
        if self_base >= 0:
            cand &= j != self_base + i
        c = j[cand]
        order = c[np.lexsort((c, -s[c]))][:k]                     # score descending, index ascending
        nb[i, :len(order)] = order
        scr[i, :len(order)] = s[order]
        edges += [(edge_base + i, int(v)) for v in order]
    return dict(neighbours=nb, scores=scr, edges=np.array(edges, EDGE).reshape(-1), count=len(edges))


def plan(n_db, nq, words, k):
    """the formula of psx_shortlist_query_plan"""
    if n_db == 0 or nq == 0:
        return dict(blocks=0, keys_per_block=0, partial_keys=0, scratch_bytes=0)
    pad16 = lambda b: (b + 15) // 16 * 16
    blocks, kpb = (n_db + TILE - 1) // TILE, min(k, TILE)
    partial = nq * blocks * kpb
    return dict(blocks=blocks, keys_per_block=kpb, partial_keys=partial,
                scratch_bytes=pad16(4 * words) + pad16(4 * nq) + 8 * partial + 4 * (2 * ((nq * k + 255) // 256) + 2))


# ---- generators -------------------------------------------------------------------------------------------------------

def rows(seed, n_db, nq, words):
    """(db q, query q, weights): sparse random histograms, quantised.  Database views 2 and 66 are identical (a tie across two
    blocks), view 3 and query 1 have no rows, view 5 and query 2 share no word (score 0), query 0 IS view 0 (the top score)."""
    rng = np.random.default_rng(seed)
    make = lambda n: (rng.integers(0, 9, (n, words)) * (rng.random((n, words)) < 0.4)).astype(np.uint32)
    db, qq = make(n_db), make(nq)
    if n_db >= 8:
        db[3] = 0
        db[5] = 0
        db[5, :max(words // 2, 1)] = 3
    if n_db >= 67:
        db[66] = db[2]
    if n_db and nq:
        qq[0] = db[0]
    if nq >= 5:
        qq[1] = 0
        qq[2] = 0
        qq[2, max(words // 2, 1):] = 2
    dbq, df = quantize(db)
    weights = np.where(df > 0, 1 + rng.integers(0, 190, words), 0).astype(np.int32)
    return dbq, quantize(qq)[0], weights


def _case(n_db, nq, words, k, **kw):
    d = dict(n_db=n_db, nq=nq, words=words, k=k, db_limit=None, self_base=-1, edge_base=0, min_score=0)
    d.update(kw)
    return d


# name -> the sizes and options of a call
CASES = {}
for _d, _q, _w, _k in itertools.product(N_DB, N_QUERIES, WORDS, KS):
    CASES["db%d_q%d_w%d_k%d" % (_d, _q, _w, _k)] = _case(_d, _q, _w, _k, edge_base=_d)
CASES["k_above_db"] = _case(130, 5, 33, 200, edge_base=7)
CASES["limits"] = _case(130, 5, 33, 70, db_limit=(0, 65, 130, 64, 1))
CASES["limits_k3"] = _case(130, 65, 31, 3, db_limit=tuple([0, 65, 130] + [i * 2 for i in range(62)]))
CASES["self_inside"] = _case(130, 65, 33, 3, self_base=60, edge_base=60)
CASES["self_earlier_only"] = _case(130, 65, 100, 70, self_base=65, edge_base=65, db_limit=tuple(65 + i for i in range(65)))
CASES["min_score"] = _case(130, 5, 100, 70, min_score="median")
CASES["min_score_k3"] = _case(65, 65, 33, 3, min_score="upper")
CASES["empty_db"] = _case(0, 5, 7, 3)
CASES["no_queries"] = _case(130, 0, 7, 3)
CASES["heavy_word"] = _case(8, 1, 4, 3)
CASES["million"] = _case(MAX_VIEWS, 1, 2, 3)

SMALL = sorted(n for n in CASES if n != "million")


def case(name):
    """(db q, query q, weights, options dict) of a case; the options are what query() and the raw calls take"""
    c = dict(CASES[name])
    n_db, nq, words = c.pop("n_db"), c.pop("nq"), c.pop("words")
    if name == "million":
        # 4 MB of database: every row {100, 65435} scores 35635 against the query; three rows score more, the best LAST
        db = np.empty((n_db, 2), np.uint16)
        db[:] = (100, 65435)
        db[n_db - 1], db[0], db[n_db // 2] = (30000, 35535), (29999, 35535), (29998, 35535)
        return db, np.array([[30000, 35535]], np.uint16), np.array([1, 1], np.int32), c
    if name == "heavy_word":
        # one word of the largest weight, a query and a view concentrated on it: 65535 * 1023 > 2^24
        db, qq, weights = rows(5, n_db, nq, words)
        weights[:] = (1023, 1, 1, 1)
        db[4], qq[0] = (65535, 0, 0, 0), (65535, 0, 0, 0)
        return db, qq, weights, c
    seed = 1000 + sorted(CASES).index(name)
    if c["self_base"] >= 0:                                        # the queries ARE stored views
        db, _, weights = rows(seed, n_db, 1, words)
        qq = db[c["self_base"]:c["self_base"] + nq].copy()
    else:
        db, qq, weights = rows(seed, n_db, nq, words)
    if c["min_score"] in ("median", "upper"):                      # between two scores that occur: the middle ones, or high
        s = np.concatenate([scores_of(db, r, weights) for r in qq])    # enough to cut lists of three
        s = np.unique(s[s > 0])
        assert len(s) >= 20, name
        at = len(s) // 2 if c["min_score"] == "median" else len(s) * 19 // 20
        c["min_score"] = int(s[at - 1]) + 1
        assert s[at - 1] < c["min_score"] <= s[at]
    return db, qq, weights, c


# ---- raw calls on sentinel-filled host arrays (the _ref and the host forms) ---------------------------------------------

ptr = sc.ptr


def raw_query(capi, fn, db_ptr, n_db, q_ptr, nq, words, weights, opt, capacity, lists=True, slack=3):
    """fn(db, n_db, queries, nq, words, weights, limits, opts, neighbours, scores, edges, capacity, count) on arrays filled with
    sentinels; capacity None: NULL with 0 -> (rc, count, neighbours, scores, edge words)"""
    k = opt["k"]
    nb = np.full((nq * k + slack,), -7, np.int32)
    scr = np.full((nq * k + slack,), 0xA5A5A5A5, np.uint32)
    ed = np.full((2 * ((capacity or 0) + slack),), -7, np.int32)
    n = C.c_int(-77)
    o = capi.QueryOpts(k, opt.get("flags", 0), opt["self_base"], opt["edge_base"], opt["min_score"], opt.get("reserved", 0))
    w = np.ascontiguousarray(weights, np.int32)
    lim = None if opt["db_limit"] is None else np.ascontiguousarray(opt["db_limit"], np.int32)
    rc = fn(db_ptr, n_db, q_ptr, nq, words, ptr(w), ptr(lim), C.byref(o), ptr(nb) if lists else None, ptr(scr) if lists else None,
            ptr(ed) if capacity is not None else None, capacity or 0, C.byref(n))
    return rc, n.value, nb, scr, ed


def raw_query_ref(capi, db, qq, weights, opt, capacity, lists=True):
    return raw_query(capi, capi.lib().psx_shortlist_query_ref, ptr(db), len(db), ptr(qq), len(qq), db.shape[1], weights, opt, capacity, lists)
