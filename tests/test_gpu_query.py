"""GPU tests of the database query (include/popsift_hip.h, "QUERY A DATABASE OF VIEWS"): psx_bow_quantize_dev and
psx_shortlist_query in its _dev and host-output forms on the smallest shapes at which the kernels can go wrong -- the tile of
64 on either side, the 32-word step, k below and above the 64 keys of a block list, ties across blocks, limits, a self index, a
least score, scores above 2^24, a million stored views -- the tie to psx_shortlist_views_dev, the chain into
psx_match_pairs_graph_u8_dev, the python wrappers and popsift::ViewDatabase.  Every comparison is as bytes against the host
references, called with the same capacities on arrays filled with the same sentinels: whole buffers are compared, so nothing
may be written past the range the rule names.  Out-of-range inputs are refused on the host before any launch."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest
import torch        # before the HIP library is loaded: torch brings a HIP runtime of its own and must initialise first (_dev forms)

from tests import query_cases as qc
from tests import shortlist_cases as sc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda() if a.size else None


def _vp(t, offset=0):
    return C.c_void_p(t.data_ptr() + offset) if t is not None else None


def _query_dev(capi, ddb, dqq, db, qq, weights, opt, capacity, lists=True, slack=3, misalign=()):
    """psx_shortlist_query_dev on sentinel-filled device arrays -> what qc.raw_query returns"""
    k, nq = opt["k"], len(qq)
    nb = torch.full((nq * k + slack,), -7, dtype=torch.int32, device="cuda")
    scr = torch.full((nq * k + slack,), -0x5A5A5A5B, dtype=torch.int32, device="cuda")      # 0xA5A5A5A5
    ed = torch.full((2 * ((capacity or 0) + slack),), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    n = C.c_int(-77)
    o = capi.QueryOpts(k, 0, opt["self_base"], opt["edge_base"], opt["min_score"], 0)
    w = np.ascontiguousarray(weights, np.int32)
    lim = None if opt["db_limit"] is None else np.ascontiguousarray(opt["db_limit"], np.int32)
    off = lambda what, by: by if what in misalign else 0
    rc = capi.lib().psx_shortlist_query_dev(0, _vp(ddb, off("db", 1)), len(db), _vp(dqq, off("queries", 1)), nq, db.shape[1], qc.ptr(w), qc.ptr(lim),
                                            C.byref(o), _vp(nb, off("neighbours", 2)) if lists else None, _vp(scr, off("scores", 2)) if lists else None,
                                            _vp(ed, off("edges", 4)) if capacity is not None else None, capacity or 0, C.byref(n))
    return rc, n.value, nb.cpu().numpy(), scr.cpu().numpy().view(np.uint32), ed.cpu().numpy()


def _query_host_form(capi, ddb, dqq, db, qq, weights, opt, capacity, lists=True):
    fn = lambda *a: capi.lib().psx_shortlist_query(0, *a)
    return qc.raw_query(capi, fn, _vp(ddb), len(db), _vp(dqq), len(qq), db.shape[1], weights, opt, capacity, lists)


def _same(got, want, what):
    assert got[0] == want[0] == 0, (what, got[0], want[0])
    for g, w in zip(got[1:], want[1:]):
        assert (g == w) if isinstance(w, int) else np.array_equal(g, w), (what, g, w)


def _both_forms(capi, name, capacities=("total",)):
    """the _dev and the host form of a case against the reference; returns the reference's tuple at the exact capacity"""
    db, qq, weights, opt = qc.case(name)
    ddb, dqq = _cuda(db), _cuda(qq)
    total = qc.raw_query_ref(capi, db, qq, weights, opt, None, False)[1]
    exact = None
    for cap, lists in capacities:
        cap = {"total": total, "short": total - 1, "half": total // 2, "more": total + 2}.get(cap, cap)
        want = qc.raw_query_ref(capi, db, qq, weights, opt, cap, lists)
        assert want[0] == 0 and want[1] == total
        _same(_query_dev(capi, ddb, dqq, db, qq, weights, opt, cap, lists), want, (name, "dev", cap, lists))
        _same(_query_host_form(capi, ddb, dqq, db, qq, weights, opt, cap, lists), want, (name, "host form", cap, lists))
        exact = want if cap == total and lists else exact
    if ddb is not None:
        assert np.array_equal(ddb.cpu().numpy(), db.view(np.uint8).reshape(-1)), "the database is only read"
    return exact


@pytest.mark.parametrize("n_db", qc.N_DB)
def test_tile_edges(capi, n_db):
    """n_db in {1, 63, 64, 65, 130} x n_queries in {1, 5, 65} x words in {1, 31, 33, 100} x k in {1, 3, 70}: one, two and three
    database blocks, two query blocks, words off the 32-word step, partial lists of 64 keys merged across blocks"""
    for nq, words, k in itertools.product(qc.N_QUERIES, qc.WORDS, qc.KS):
        _both_forms(capi, "db%d_q%d_w%d_k%d" % (n_db, nq, words, k), (("total", True),))


@pytest.mark.parametrize("name", ["k_above_db", "limits", "limits_k3", "self_inside", "self_earlier_only", "min_score", "min_score_k3",
                                  "heavy_word"])
def test_lists_limits_and_range(capi, name):
    """k above n_db; limits of 0, 65 and n_db, and blocks that leave early; queries inside the database without themselves, and
    against the earlier views alone; a least score between two that occur; a score of 65535 * 1023 > 2^24"""
    want = _both_forms(capi, name, (("total", True),))
    if name == "heavy_word":
        assert want[2][0] == 4 and want[3][0] == 65535 * 1023


def test_ties_across_blocks(capi):
    """database views 2 and 66 are identical and lie in different blocks: every query that lists 66 lists 2 directly before it"""
    db, qq, weights, opt = qc.case("db130_q65_w100_k70")
    got = _query_dev(capi, _cuda(db), _cuda(qq), db, qq, weights, opt, 0)
    assert got[0] == 0
    rows = got[2][:-3].reshape(len(qq), opt["k"]).tolist()
    seen = 0
    for i, row in enumerate(rows):
        if 66 in row:
            assert row.index(2) + 1 == row.index(66), i
            seen += 1
    want = qc.query(db, qq, weights, **opt)["neighbours"].tolist()
    assert seen == sum(66 in row for row in want) >= 10


def test_million_stored_views(capi):
    """n_db = 1 048 576, words = 2, one query, k = 3: the winners at the last, the first and a middle index -- 20 index bits
    from the key through the merge over 16384 block lists"""
    want = _both_forms(capi, "million", (("total", True),))
    assert want[1] == 3 and list(want[2][:3]) == [qc.MAX_VIEWS - 1, 0, qc.MAX_VIEWS // 2] and list(want[3][:3]) == [65535, 65534, 65533]


@pytest.mark.parametrize("name", ["db130_q5_w33_k70", "self_inside"])
def test_edge_capacities(capi, name):
    """0 / NULL, below the total, the total and more; with and without the list arrays"""
    _both_forms(capi, name, (("total", False), ("short", True), ("half", True), ("more", True), (0, True), (None, True), (None, False)))


def test_empty_forms(capi):
    db, qq, weights, opt = qc.case("no_queries")
    got = _query_dev(capi, _cuda(db), None, db, qq, weights, opt, 0)
    assert got[0] == 0 and got[1] == 0 and np.all(got[2] == -7) and np.all(got[4] == -7)
    # an empty database: the _dev form still writes every entry as unused
    _both_forms(capi, "empty_db", (("total", True), (None, False)))
    db, qq, weights, opt = qc.case("empty_db")
    got = _query_dev(capi, None, _cuda(qq), db, qq, weights, opt, 0)
    assert list(got[2]) == [-1] * 15 + [-7] * 3 and list(got[3][:15]) == [0] * 15


def test_refusals_before_any_launch(capi):
    """misaligned device pointers and out-of-range arguments: PSX_ERR_INVALID, every device array as it was"""
    db, qq, weights, opt = qc.case("db65_q5_w33_k3")
    ddb, dqq = _cuda(db), _cuda(qq)
    for what in ("db", "queries", "neighbours", "scores", "edges"):
        rc, n, nb, scr, ed = _query_dev(capi, ddb, dqq, db, qq, weights, opt, 4, misalign=(what,))
        assert rc == -1 and n == -77 and np.all(nb == -7) and np.all(scr == 0xA5A5A5A5) and np.all(ed == -7), what
    heavy = weights.copy()
    heavy[0] = 1024
    for w, o in ((heavy, opt), (weights, dict(opt, db_limit=(0, 0, 66, 0, 0))), (weights, dict(opt, self_base=61))):
        rc, n, nb, scr, ed = _query_dev(capi, ddb, dqq, db, qq, w, o, 4)
        assert rc == -1 and n == -77 and np.all(nb == -7) and np.all(scr == 0xA5A5A5A5) and np.all(ed == -7)
    n = C.c_int(-77)
    w = np.ascontiguousarray(weights, np.int32)
    for o in (capi.QueryOpts(0, 0, -1, 0, 0, 0), capi.QueryOpts(3, 1, -1, 0, 0, 0), capi.QueryOpts(3, 0, -1, 0, 0, 1)):
        assert capi.lib().psx_shortlist_query_dev(0, _vp(ddb), 65, _vp(dqq), 5, 33, qc.ptr(w), None, C.byref(o), None, None, None, 0, C.byref(n)) == -1
        assert n.value == -77
    hist = torch.zeros((8 * 10,), dtype=torch.int32, device="cuda")
    q = torch.full((8 * 10 * 2,), 0x5A, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    L = capi.lib()
    assert L.psx_bow_quantize_dev(0, _vp(hist, 2), 8, 10, _vp(q), None) == -1
    assert L.psx_bow_quantize_dev(0, _vp(hist), 8, 10, _vp(q, 1), None) == -1
    assert L.psx_bow_quantize_dev(0, _vp(hist), 8, 0, _vp(q), None) == -1
    assert L.psx_bow_quantize_dev(0, None, 8, 10, _vp(q), None) == -1
    assert np.all(q.cpu().numpy() == 0x5A)


@pytest.mark.parametrize("name", ["n8_disjoint", "n65_k67"])
def test_device_quantisation_equals_the_reference(capi, name):
    """q and df as bytes; df is ADDED; a database grows by quantising new rows behind the old ones; without df nothing comes down"""
    hist, _, _ = sc.shortlist_case(name)
    N, W = hist.shape
    want_q = np.full((N * W + 3,), 0xA5A5, np.uint16)
    want_df = np.full((W,), 5, np.int32)
    assert capi.lib().psx_bow_quantize_ref(sc.ptr(hist), N, W, sc.ptr(want_q), sc.ptr(want_df)) == 0
    dh = _cuda(hist)
    dq = _cuda(np.full((N * W + 3,), 0xA5A5, np.uint16))
    df = np.full((W,), 5, np.int32)
    torch.cuda.synchronize()
    half = N // 2
    capi.bow_quantize_dev(dh.data_ptr(), half, W, dq.data_ptr(), df)
    capi.bow_quantize_dev(dh.data_ptr() + 4 * half * W, N - half, W, dq.data_ptr() + 2 * half * W, df)
    assert np.array_equal(dq.cpu().numpy().view(np.uint16), want_q) and np.array_equal(df, want_df)
    dq2 = _cuda(np.full((N * W + 3,), 0xA5A5, np.uint16))
    torch.cuda.synchronize()
    capi.bow_quantize_dev(dh.data_ptr(), N, W, dq2.data_ptr())
    assert np.array_equal(dq2.cpu().numpy().view(np.uint16), want_q)
    assert np.array_equal(dh.cpu().numpy(), hist.view(np.uint8).reshape(-1)), "the histogram is only read"


def test_tie_to_the_symmetric_call_on_the_device(capi):
    """n65_k67: quantise on the device, weigh, query the database with itself and self_base = 0 -- neighbours and scores of
    psx_shortlist_views_dev as bytes, its edge list as the set of unordered pairs"""
    hist, k, _ = sc.shortlist_case("n65_k67")
    N, W = hist.shape
    dh = _cuda(hist)
    dq = torch.zeros((N * W * 2,), dtype=torch.uint8, device="cuda")
    out = [torch.full((N * k,), -7, dtype=torch.int32, device="cuda") for _ in range(4)]
    ed = [torch.full((2 * N * k,), -7, dtype=torch.int32, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    df = np.zeros((W,), np.int32)
    capi.bow_quantize_dev(dh.data_ptr(), N, W, dq.data_ptr(), df)
    weights = capi.bow_weights(df, N)
    n_query = capi.shortlist_query_dev(dq.data_ptr(), N, dq.data_ptr(), N, W, weights, k, out[0].data_ptr(), out[1].data_ptr(), ed[0].data_ptr(), N * k,
                                       self_base=0)
    n_views = capi.shortlist_views_dev(dh.data_ptr(), N, W, k, out[2].data_ptr(), out[3].data_ptr(), ed[1].data_ptr(), N * k)
    assert torch.equal(out[0], out[2]) and torch.equal(out[1], out[3])
    assert n_query == int((out[0] >= 0).sum())
    mine = ed[0].cpu().numpy()[:2 * n_query].reshape(-1, 2)
    theirs = ed[1].cpu().numpy()[:2 * n_views].reshape(-1, 2)
    assert {(min(a, b), max(a, b)) for a, b in mine.tolist()} == {tuple(e) for e in theirs.tolist()}


def test_the_chain_with_two_arriving_views(capi):
    """the planted views: 22 are stored, views 5 and 23 arrive.  train -> bags -> quantise -> query on the device, then
    psx_match_pairs_graph_u8_dev on the returned edges over the stored sets with the arriving ones behind them: each arriving
    view's first neighbour is a view of its own group, and the per-edge counts are those of the same edges written by hand"""
    p = sc.PLANTED
    sets = sc.planted()
    arriving = (5, 23)
    order = [i for i in range(len(sets)) if i not in arriving] + list(arriving)
    sets = [sets[i] for i in order]
    lens = [len(s) for s in sets]
    n_db, nq, W, k = len(sets) - 2, 2, p["words"], p["k"]
    keep = [_cuda(s) for s in sets]
    adr = [t.data_ptr() for t in keep]
    vocab = torch.zeros((W * 128,), dtype=torch.uint8, device="cuda")
    hist = torch.zeros((len(sets) * W,), dtype=torch.int32, device="cuda")
    q = torch.zeros((len(sets) * W * 2,), dtype=torch.uint8, device="cuda")
    nb = torch.full((nq * k,), -7, dtype=torch.int32, device="cuda")
    edges = torch.full((2 * nq * k,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    capi.vocab_train_u8_dev(adr[:n_db], lens[:n_db], W, p["iterations"], vocab.data_ptr())
    capi.bow_u8_dev(vocab.data_ptr(), W, adr, lens, hist.data_ptr())
    df = np.zeros((W,), np.int32)
    capi.bow_quantize_dev(hist.data_ptr(), n_db, W, q.data_ptr(), df)
    capi.bow_quantize_dev(hist.data_ptr() + 4 * n_db * W, nq, W, q.data_ptr() + 2 * n_db * W)
    weights = capi.bow_weights(df, n_db)
    count = capi.shortlist_query_dev(q.data_ptr(), n_db, q.data_ptr() + 2 * n_db * W, nq, W, weights, k, nb.data_ptr(), 0, edges.data_ptr(), nq * k,
                                     edge_base=n_db)
    rows = nb.cpu().numpy().reshape(nq, k)
    assert count == nq * k and np.all(rows >= 0)
    for i, view in enumerate(arriving):
        assert order[rows[i, 0]] // p["per_group"] == view // p["per_group"], (view, rows[i])
        assert sorted(order[j] for j in rows[i]) == sc.planted_mates(view), (view, rows[i])
    returned = edges.cpu().numpy().reshape(-1, 2)
    by_hand = [(n_db + i, int(j)) for i in range(nq) for j in rows[i]]
    assert returned.tolist() == [list(e) for e in by_hand]
    room = int(sum(lens[a] for a, _ in by_hand))
    pairs = torch.zeros((room * 16,), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    got_counts, got_n = capi.match_pairs_graph_dev(adr, lens, returned, pairs.data_ptr(), room, 0.8, True)
    want_counts, want_n = capi.match_pairs_graph_dev(adr, lens, by_hand, pairs.data_ptr(), room, 0.8, True)
    assert np.array_equal(got_counts, want_counts) and got_n == want_n == int(got_counts.sum()) and np.all(got_counts > 0)
    # the reference on what came down: the same lists
    want = capi.shortlist_query_ref(q.cpu().numpy().view(np.uint16).reshape(-1, W)[:n_db], q.cpu().numpy().view(np.uint16).reshape(-1, W)[n_db:],
                                    weights, k, edge_base=n_db)
    assert np.array_equal(want["neighbours"], rows) and want["edges"].tolist() == by_hand
    assert keep


def test_python_wrappers(capi):
    """capi.shortlist_query (which asks "how many?" first) and shortlist_query_plan against the _ref wrapper"""
    db, qq, weights, opt = qc.case("limits")
    ddb, dqq = _cuda(db), _cuda(qq)
    kw = dict(db_limit=opt["db_limit"], self_base=opt["self_base"], edge_base=opt["edge_base"], min_score=opt["min_score"])
    got = capi.shortlist_query(ddb.data_ptr(), len(db), dqq.data_ptr(), len(qq), db.shape[1], weights, opt["k"], **kw)
    want = capi.shortlist_query_ref(db, qq, weights, opt["k"], **kw)
    assert got["count"] == want["count"] > 0 and all(np.array_equal(got[f], want[f]) for f in ("neighbours", "scores", "edges"))
    assert got["edges"].tolist() == qc.query(db, qq, weights, **opt)["edges"].tolist()
    assert capi.shortlist_query_plan(len(db), len(qq), db.shape[1], opt["k"]) == qc.plan(len(db), len(qq), db.shape[1], opt["k"])
    assert capi.lib().psx_match_release() == 0


def test_cpp_view_database_on_the_gpu(tmp_path):
    """tests/cpp/test_view_database_api.cpp with POPSIFT_TEST_EXPECT_GPU: popsift::ViewDatabase and the vocabulary file end to end"""
    libdir = os.path.join(ROOT, "popsift_amd", "lib")
    exe = str(tmp_path / "test_view_database_api")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-pthread", os.path.join(ROOT, "tests", "cpp", "test_view_database_api.cpp"), "-o", exe,
                           "-I", os.path.join(ROOT, "popsift_amd", "csrc", "include"), "-I", os.path.join(ROOT, "include"),
                           "-L", libdir, "-lpopsift", "-lpopsift_hip", "-Wl,-rpath," + libdir])
    out = subprocess.run([exe, str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300,
                         env=dict(os.environ, POPSIFT_TEST_EXPECT_GPU="1"))
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout
    assert "view database:" in out.stdout
