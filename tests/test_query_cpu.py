"""The database query without a GPU (include/popsift_hip.h, "QUERY A DATABASE OF VIEWS"): psx_bow_quantize_ref and
psx_shortlist_query_ref against the numpy restatement of tests/query_cases.py on every case the GPU tests run, arrays filled
with sentinels and compared whole; the refusals (outputs untouched); the capacity rule; psx_shortlist_query_plan against its
formula; the tie to psx_shortlist_views_ref; and tests/cpp/query_san.cpp: the references, the checks and the vocabulary file
reader and writer as a stand-alone program under -fsanitize=address,undefined."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import query_cases as qc
from tests import shortlist_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _whole(got, want, k, capacity):
    """(rc, count, neighbours, scores, edge words) against the restatement, slack and all"""
    rc, n, nb, scr, ed = got
    assert rc == 0 and n == want["count"]
    assert np.array_equal(nb[:-3], want["neighbours"].reshape(-1)) and np.all(nb[-3:] == -7)
    assert np.array_equal(scr[:-3], want["scores"].reshape(-1)) and np.all(scr[-3:] == 0xA5A5A5A5)
    kept = min(n, capacity or 0)
    assert np.array_equal(ed[:2 * kept], want["edges"].view(np.int32).reshape(-1)[:2 * kept]) and np.all(ed[2 * kept:] == -7)


@pytest.mark.parametrize("name", qc.SMALL)
def test_query_reference_equals_numpy(capi, name):
    db, qq, weights, opt = qc.case(name)
    want = qc.query(db, qq, weights, **opt)
    _whole(qc.raw_query_ref(capi, db, qq, weights, opt, want["count"]), want, opt["k"], want["count"])
    nb = want["neighbours"]
    if len(db) >= 67 and opt["db_limit"] is None and opt["k"] >= 3:
        for i, row in enumerate(nb.tolist()):                      # views 2 and 66 are identical: the lower one directly before
            if 66 in row:
                assert row.index(2) + 1 == row.index(66), (name, i)
    if len(db) >= 8:
        assert 3 not in nb, "a view without rows is nobody's candidate"
    if len(qq) >= 5 and len(db) and opt["self_base"] < 0:
        assert np.all(nb[1] == -1), "a query without rows has no candidate"
        assert 5 not in nb[2], "no common word: score 0"
    if opt["self_base"] >= 0:
        assert all(opt["self_base"] + i not in row for i, row in enumerate(nb.tolist()))
    if opt["db_limit"] is not None:
        assert all(v < lim for row, lim in zip(nb.tolist(), opt["db_limit"]) for v in row)
    if opt["min_score"] > 0:
        plain = qc.query(db, qq, weights, **dict(opt, min_score=0))
        assert 0 < want["count"] < plain["count"] and want["scores"][want["scores"] > 0].min() >= opt["min_score"]


def test_what_the_cases_hold():
    """the properties the issue names are in the cases: k above the 64 keys of a block and above n_db, three blocks, limits of
    0, 65 and n_db, a score above 2^24"""
    assert qc.CASES["k_above_db"]["k"] > qc.CASES["k_above_db"]["n_db"] == 130
    assert set((0, 65, 130)) <= set(qc.CASES["limits"]["db_limit"])
    db, qq, weights, opt = qc.case("heavy_word")
    want = qc.query(db, qq, weights, **opt)
    assert want["neighbours"][0, 0] == 4 and want["scores"][0, 0] == 65535 * 1023 > 1 << 24
    db, qq, weights, opt = qc.case("db130_q5_w100_k70")
    want = qc.query(db, qq, weights, **opt)
    assert (want["neighbours"][0] >= 0).sum() > 64, "a list longer than one block's 64 keys"


def test_million_views_reference(capi):
    """n_db = 2^20: the 20 index bits end to end -- the winners at the last, the first and a middle index, in that order"""
    db, qq, weights, opt = qc.case("million")
    want = qc.query(db, qq, weights, **opt)
    assert want["neighbours"].tolist() == [[qc.MAX_VIEWS - 1, 0, qc.MAX_VIEWS // 2]] and want["scores"].tolist() == [[65535, 65534, 65533]]
    _whole(qc.raw_query_ref(capi, db, qq, weights, opt, 3), want, 3, 3)


@pytest.mark.parametrize("name", ["n1_k1", "n8_disjoint", "n33_k35", "n65_k67"])
def test_quantize_reference_equals_numpy(capi, name):
    hist, _, _ = sc.shortlist_case(name)
    want_q, want_df = qc.quantize(hist)
    N, W = hist.shape
    q = np.full((N * W + 3,), 0xA5A5, np.uint16)
    df = np.full((W + 2,), 5, np.int32)
    assert capi.lib().psx_bow_quantize_ref(sc.ptr(hist), N, W, sc.ptr(q), sc.ptr(df)) == 0
    assert np.array_equal(q[:-3], want_q.reshape(-1)) and np.all(q[-3:] == 0xA5A5)
    assert np.array_equal(df[:W], 5 + want_df) and np.all(df[W:] == 5), "df is ADDED to what was there"
    # a database grows by quantising new rows behind the old ones
    half = N // 2
    df2 = np.zeros((W,), np.int32)
    parts = [capi.bow_quantize_ref(hist[:half], df2), capi.bow_quantize_ref(hist[half:], df2)]
    assert np.array_equal(np.concatenate(parts), want_q) and np.array_equal(df2, want_df)
    assert np.array_equal(capi.bow_quantize_ref(hist), want_q)


@pytest.mark.parametrize("name", sorted(sc.SHORTLIST))
def test_tie_to_the_symmetric_call(capi, name):
    """quantise, weigh, query the database with itself and self_base = 0: neighbours and scores of psx_shortlist_views_ref bit
    for bit, and its non-mutual edge list as the set of unordered pairs"""
    n, w, k, _ = sc.SHORTLIST[name]
    hist = sc.hists(400 + n, n, w)
    df = np.zeros((w,), np.int32)
    q = capi.bow_quantize_ref(hist, df)
    weights = capi.bow_weights(df, n)
    got = capi.shortlist_query_ref(q, q, weights, k, self_base=0)
    want = capi.shortlist_views_ref(hist, k, mutual=False)
    assert np.array_equal(got["neighbours"], want["neighbours"]) and np.array_equal(got["scores"], want["scores"])
    assert {(min(a, b), max(a, b)) for a, b in got["edges"].tolist()} == set(want["edges"].tolist())
    assert got["count"] == int((got["neighbours"] >= 0).sum())


def _refused(capi, db, qq, weights, opt, n_db=None, nq=None, words=None, capacity=0, edges=True, db_ptr=True, q_ptr=True, w_ptr=True):
    """the call returns PSX_ERR_INVALID and writes nothing"""
    k = max(opt["k"], 1)
    rows = max(len(qq) if nq is None else nq, 1)
    nb = np.full((min(rows * k, 1 << 16),), -7, np.int32)
    scr = np.full((len(nb),), 0xA5A5A5A5, np.uint32)
    ed = np.full((16,), -7, np.int32)
    n = C.c_int(-77)
    o = capi.QueryOpts(opt["k"], opt.get("flags", 0), opt["self_base"], opt["edge_base"], opt["min_score"], opt.get("reserved", 0))
    w = np.ascontiguousarray(weights, np.int32)
    lim = None if opt["db_limit"] is None else np.ascontiguousarray(opt["db_limit"], np.int32)
    rc = capi.lib().psx_shortlist_query_ref(sc.ptr(db) if db_ptr else None, len(db) if n_db is None else n_db, sc.ptr(qq) if q_ptr else None,
                                            len(qq) if nq is None else nq, db.shape[1] if words is None else words, sc.ptr(w) if w_ptr else None,
                                            sc.ptr(lim), C.byref(o), sc.ptr(nb), sc.ptr(scr), sc.ptr(ed) if edges else None, capacity, C.byref(n))
    assert rc == -1 and n.value == -77 and np.all(nb == -7) and np.all(scr == 0xA5A5A5A5) and np.all(ed == -7)


def test_refusals_leave_the_outputs_untouched(capi):
    db, qq, weights, opt = qc.case("db65_q5_w33_k3")
    _refused(capi, db, qq, weights, opt, n_db=-1)
    _refused(capi, db, qq, weights, opt, nq=-1)
    _refused(capi, db, qq, weights, opt, db_ptr=False)
    _refused(capi, db, qq, weights, opt, q_ptr=False)
    _refused(capi, db, qq, weights, opt, w_ptr=False)
    _refused(capi, db, qq, weights, opt, words=0)
    _refused(capi, db, qq, weights, opt, words=65537)
    _refused(capi, db, qq, weights, opt, n_db=qc.MAX_VIEWS + 1)
    _refused(capi, db, qq, weights, opt, nq=4097)
    _refused(capi, db, qq, weights, dict(opt, k=0))
    _refused(capi, db, qq, weights, dict(opt, k=-3))
    _refused(capi, db, qq, weights, dict(opt, k=(1 << 31) // 5 + 1))                     # n_queries * k above INT_MAX
    _refused(capi, db, qq, weights, dict(opt, flags=1))
    _refused(capi, db, qq, weights, dict(opt, reserved=1))
    _refused(capi, db, qq, weights, dict(opt, self_base=-2))
    _refused(capi, db, qq, weights, dict(opt, self_base=61))                             # 61 + 5 > 65
    for bad in (-1, 1024):
        w = weights.copy()
        w[7] = bad
        _refused(capi, db, qq, w, opt)
    _refused(capi, db, qq, weights, dict(opt, db_limit=(0, 1, 2, 66, 3)))
    _refused(capi, db, qq, weights, dict(opt, db_limit=(0, 1, -1, 6, 3)))
    _refused(capi, db, qq, weights, opt, capacity=-1)
    _refused(capi, db, qq, weights, opt, capacity=2, edges=False)
    # the block lists: 4096 queries x 16384 blocks x 64 keys are far above 2^27
    _refused(capi, db, qq, weights, dict(opt, k=64), n_db=qc.MAX_VIEWS, nq=4096)
    L = capi.lib()
    o = capi.query_opts(3)
    w = np.ascontiguousarray(weights, np.int32)
    assert L.psx_shortlist_query_ref(sc.ptr(db), 65, sc.ptr(qq), 5, 33, sc.ptr(w), None, None, None, None, None, 0, C.byref(C.c_int())) == -1
    assert L.psx_shortlist_query_ref(sc.ptr(db), 65, sc.ptr(qq), 5, 33, sc.ptr(w), None, C.byref(o), None, None, None, 0, None) == -1
    # self_base + n_queries = n_db exactly, and the largest weight, are fine
    w[:] = np.minimum(w * 1023, 1023)
    n = C.c_int(-77)
    o = capi.query_opts(3, self_base=60)
    assert L.psx_shortlist_query_ref(sc.ptr(db), 65, sc.ptr(db[60:]), 5, 33, sc.ptr(w), None, C.byref(o), None, None, None, 0, C.byref(n)) == 0
    assert n.value > 0
    # psx_bow_quantize_ref
    hist = sc.hists(3, 8, 10)
    q = np.full((80,), 0xA5A5, np.uint16)
    df = np.full((10,), 5, np.int32)
    for h, nv, words, qp in ((None, 8, 10, sc.ptr(q)), (sc.ptr(hist), 8, 10, None), (sc.ptr(hist), -1, 10, sc.ptr(q)), (sc.ptr(hist), 8, 0, sc.ptr(q)),
                             (sc.ptr(hist), 8, 65537, sc.ptr(q)), (sc.ptr(hist), qc.MAX_VIEWS + 1, 10, sc.ptr(q))):
        assert L.psx_bow_quantize_ref(h, nv, words, qp, sc.ptr(df)) == -1 and np.all(q == 0xA5A5) and np.all(df == 5)
    assert L.psx_bow_quantize_ref(None, 0, 10, None, sc.ptr(df)) == 0 and np.all(df == 5)


@pytest.mark.parametrize("name", ["db130_q5_w33_k70", "self_inside", "limits"])
def test_capacities(capi, name):
    """the exact capacity, one short, a cut in the middle, more than needed, 0 and NULL; with and without the list arrays: the
    count is always the total and nothing at or past the capacity is touched"""
    db, qq, weights, opt = qc.case(name)
    want = qc.query(db, qq, weights, **opt)
    total = want["count"]
    assert total >= 3
    words = want["edges"].view(np.int32).reshape(-1)
    for cap, lists in ((total, True), (total - 1, True), (total // 2, False), (total + 2, False), (0, True), (None, True), (None, False)):
        rc, n, nb, scr, ed = qc.raw_query_ref(capi, db, qq, weights, opt, cap, lists)
        kept = min(total, cap or 0)
        assert rc == 0 and n == total
        assert np.array_equal(ed[:2 * kept], words[:2 * kept]) and np.all(ed[2 * kept:] == -7), cap
        assert np.array_equal(nb[:-3], want["neighbours"].reshape(-1)) if lists else np.all(nb == -7)
        assert np.array_equal(scr[:-3], want["scores"].reshape(-1)) if lists else np.all(scr == 0xA5A5A5A5)


def test_empty_forms(capi):
    db, qq, weights, opt = qc.case("no_queries")
    rc, n, nb, scr, ed = qc.raw_query_ref(capi, db, qq, weights, opt, 0)
    assert rc == 0 and n == 0 and np.all(nb == -7) and np.all(ed == -7)
    db, qq, weights, opt = qc.case("empty_db")
    rc, n, nb, scr, ed = qc.raw_query_ref(capi, db, qq, weights, opt, 0)
    assert rc == 0 and n == 0 and list(nb) == [-1] * 15 + [-7] * 3 and list(scr[:15]) == [0] * 15 and np.all(ed == -7)


def test_plan_equals_the_formula(capi):
    for n_db, nq, words, k in ((1, 1, 1, 1), (64, 5, 33, 3), (65, 65, 100, 70), (130, 4096, 4096, 64), (qc.MAX_VIEWS, 1, 2, 3), (65536, 64, 4096, 8),
                               (0, 5, 7, 3), (130, 0, 7, 3), (qc.MAX_VIEWS, 128, 65536, 1)):
        assert capi.shortlist_query_plan(n_db, nq, words, k) == qc.plan(n_db, nq, words, k), (n_db, nq, words, k)
    assert capi.shortlist_query_plan(qc.MAX_VIEWS, 128, 8, 64)["partial_keys"] == 1 << 27
    L = capi.lib()
    out = capi.QueryPlan(-7, -7, -7, -7)
    for n_db, nq, words, k in ((-1, 1, 1, 1), (1, -1, 1, 1), (qc.MAX_VIEWS + 1, 1, 1, 1), (1, 4097, 1, 1), (1, 1, 0, 1), (1, 1, 65537, 1), (1, 1, 1, 0),
                               (64, 4096, 8, 1 << 20), (qc.MAX_VIEWS, 129, 8, 64)):
        assert L.psx_shortlist_query_plan(n_db, nq, words, k, C.byref(out)) == -1 and out.blocks == -7 and out.scratch_bytes == -7
    assert L.psx_shortlist_query_plan(1, 1, 1, 1, None) == -1


def test_symbols_and_constants(capi):
    hdr = open(os.path.join(ROOT, "include", "popsift_hip.h")).read()
    for sym in ("psx_bow_quantize_dev", "psx_bow_quantize_ref", "psx_shortlist_query", "psx_shortlist_query_dev", "psx_shortlist_query_ref",
                "psx_shortlist_query_plan"):
        assert "int %s(" % sym in hdr and sym in capi.SYMBOLS and hasattr(capi.lib(), sym), sym
    assert "QUERY A DATABASE OF VIEWS" in hdr
    assert C.sizeof(capi.QueryOpts) == 24 and C.sizeof(capi.QueryPlan) == 24
    rule = open(os.path.join(ROOT, "popsift_amd", "csrc", "hip", "bow_rule.h")).read()
    assert "PSX_QUERY_MAX_VIEWS = 1 << 20" in rule and "PSX_QUERY_MAX_WEIGHT = 1023" in rule
    assert capi.QUERY_MAX_VIEWS == 1 << 20 and capi.QUERY_MAX_WEIGHT == 1023
    for unit in ("build.py", ):
        assert "bow_query.hip" in open(os.path.join(ROOT, "popsift_amd", unit)).read()
    assert "bow_query" in open(os.path.join(ROOT, "CMakeLists.txt")).read()
    text = open(os.path.join(ROOT, "popsift_amd", "csrc", "include", "popsift", "vocabulary_file.h")).read()
    assert "#include <hip" not in text and "psx_" not in text, "the file format header stands alone"


def test_reference_program_under_sanitizers(tmp_path):
    """tests/cpp/query_san.cpp: the query references and checks of bow_plan.h and the vocabulary file reader and writer,
    compiled by g++ with -fsanitize=address,undefined: a round trip and each malformed file"""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed"
    exe = str(tmp_path / "query_san")
    subprocess.check_call([cxx, "-std=c++14", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           "-static-libasan", "-static-libubsan", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "query_san.cpp"),
                           "-o", exe, "-I", os.path.join(ROOT, "popsift_amd", "csrc", "hip"), "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "popsift_amd", "csrc", "include")])
    out = subprocess.run([exe, str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout


def test_cpp_view_database_argument_errors(tmp_path):
    """tests/cpp/test_view_database_api.cpp without a GPU: the vocabulary file through popsift::Vocabulary, and what
    popsift::ViewDatabase refuses before any device call"""
    libdir = os.path.join(ROOT, "popsift_amd", "lib")
    exe = str(tmp_path / "test_view_database_api")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-pthread", os.path.join(ROOT, "tests", "cpp", "test_view_database_api.cpp"), "-o", exe,
                           "-I", os.path.join(ROOT, "popsift_amd", "csrc", "include"), "-I", os.path.join(ROOT, "include"),
                           "-L", libdir, "-lpopsift", "-lpopsift_hip", "-Wl,-rpath," + libdir])
    env = {k: v for k, v in os.environ.items() if k != "POPSIFT_TEST_EXPECT_GPU"}
    out = subprocess.run([exe, str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120, env=env)
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout
