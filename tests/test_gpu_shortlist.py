"""GPU tests of the view shortlist (include/popsift_hip.h, "WHICH PAIRS TO MATCH"): psx_vocab_train_u8, psx_bow_u8 and
psx_shortlist_views in their _dev and host-output forms on the smallest shapes at which the kernels can go wrong, the planted
views, the chain into psx_match_pairs_graph_u8_dev, the python wrappers and popsift::Vocabulary.  Every comparison is as
bytes against the host references, called with the same capacities on arrays filled with the same sentinels: whole buffers
are compared, so nothing may be written past the range the rule names."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch        # before the HIP library is loaded: torch brings a HIP runtime of its own and must initialise first (_dev forms)

from tests import shortlist_cases as sc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_REF = {}


def _once(key, make):
    """a reference result, computed once and never changed"""
    if key not in _REF:
        _REF[key] = make()
    return _REF[key]


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def _device_sets(sets):
    """(tensors, addresses): an empty view has no buffer"""
    t = [_cuda(s) if len(s) else None for s in sets]
    return t, [x.data_ptr() if x is not None else 0 for x in t]


def _vp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _train_dev(capi, adr, lens, words, iterations, slack=64):
    arr, la = sc.set_table(adr, lens)
    vocab = torch.full((words * 128 + slack,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    info = capi.VocabInfo(-77, -77, -77, -77, 77)
    o = capi.VocabOpts(words, iterations)
    rc = capi.lib().psx_vocab_train_u8_dev(0, arr, sc.ptr(la), len(lens), C.byref(o), _vp(vocab), C.byref(info))
    return rc, bytes(info), vocab.cpu().numpy()


def _bow_dev(capi, vocab, adr, lens, row_words=True, slack=5):
    arr, la = sc.set_table(adr, lens)
    dv = _cuda(vocab)
    hist = torch.full((len(lens) * len(vocab) + slack,), -0x5A5A5A5B, dtype=torch.int32, device="cuda")      # 0xA5A5A5A5
    rw = torch.full((int(sum(lens)) + slack,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rc = capi.lib().psx_bow_u8_dev(0, _vp(dv), len(vocab), arr, sc.ptr(la), len(lens), _vp(hist), _vp(rw) if row_words else None)
    assert np.array_equal(dv.cpu().numpy(), vocab.reshape(-1)), "the vocabulary is only read"
    return rc, hist.cpu().numpy().view(np.uint32), rw.cpu().numpy()


def _shortlist_dev(capi, hist, k, mutual, capacity, lists=True, slack=3):
    N, W = hist.shape
    dh = _cuda(hist) if hist.size else None
    nb = torch.full((N * k + slack,), -7, dtype=torch.int32, device="cuda")
    scores = torch.full((N * k + slack,), -0x5A5A5A5B, dtype=torch.int32, device="cuda")
    ed = torch.full((2 * ((capacity or 0) + slack),), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    n = C.c_int(-77)
    o = capi.shortlist_opts(k, mutual)
    rc = capi.lib().psx_shortlist_views_dev(0, _vp(dh), N, W, C.byref(o), _vp(nb) if lists else None, _vp(scores) if lists else None,
                                            _vp(ed) if capacity is not None else None, capacity or 0, C.byref(n))
    return rc, n.value, nb.cpu().numpy(), scores.cpu().numpy().view(np.uint32), ed.cpu().numpy()


def _same(got, want, what):
    assert got[0] == want[0] == 0, (what, got[0], want[0])
    for g, w in zip(got[1:], want[1:]):
        assert (g == w) if isinstance(w, (bytes, int)) else np.array_equal(g, w), (what, g, w)


@pytest.mark.parametrize("name", sorted(sc.TRAIN))
def test_device_training_equals_the_reference(capi, name):
    """W around the tile of 32 and the chunk of 512, views across wave and workgroup edges, an empty view, M = W exactly,
    duplicate rows, all-0 and all-255 rows; T = 1 and a T at which the early stop triggers: vocabulary and info as bytes"""
    sets, words, iterations = sc.train_case(name)
    lens = [len(s) for s in sets]
    L = capi.lib()
    want = _once(("train", name), lambda: sc.raw_train(capi, L.psx_vocab_train_u8_ref, sc.addresses_of(sets), lens, words, iterations))
    keep, adr = _device_sets(sets)
    _same(_train_dev(capi, adr, lens, words, iterations), want, "dev")
    _same(sc.raw_train(capi, lambda *a: L.psx_vocab_train_u8(0, *a), adr, lens, words, iterations), want, "host form")
    info = capi.VocabInfo.from_buffer_copy(want[1])
    assert info.iterations == 1 if iterations == 1 else (info.changed == 0 and 1 < info.iterations < iterations)
    for t, s in zip(keep, sets):
        assert t is None or np.array_equal(t.cpu().numpy(), s.reshape(-1)), "the sets are only read"


def test_two_training_calls_give_the_same_bytes(capi):
    """hundreds of lanes add to the same word's sums: two calls in one process are equal as bytes"""
    sets, words, iterations = sc.train_case("w2_t40")
    lens = [len(s) for s in sets]
    keep, adr = _device_sets(sets)
    first = _train_dev(capi, adr, lens, words, iterations)
    second = _train_dev(capi, adr, lens, words, iterations)
    _same(first, second, "run to run")
    assert keep


@pytest.mark.parametrize("words", sc.WORDS)
def test_device_bags_equal_the_reference(capi, words):
    """duplicate words and rows that ARE words (exact ties), all-0 and all-255 on both sides; with and without the rows' words"""
    vocab, sets = sc.bow_case(words)
    lens = [len(s) for s in sets]
    L = capi.lib()
    keep, adr = _device_sets(sets)
    for row_words in (True, False):
        want = _once(("bow", words, row_words), lambda: sc.raw_bow(capi, L.psx_bow_u8_ref, vocab, sc.addresses_of(sets), lens, row_words))
        _same(_bow_dev(capi, vocab, adr, lens, row_words), want, ("dev", row_words))
        _same(sc.raw_bow(capi, lambda *a: L.psx_bow_u8(0, *a), vocab, adr, lens, row_words), want, ("host form", row_words))
    assert keep


def test_empty_forms_touch_nothing(capi):
    vocab = sc.vocabulary(2, 4)
    rc, hist, rw = _bow_dev(capi, vocab, [0, 0], [0, 0])
    assert rc == 0 and np.all(hist == 0xA5A5A5A5) and np.all(rw == -7)                     # the _dev form writes nothing
    rc, hist, rw = sc.raw_bow(capi, lambda *a: capi.lib().psx_bow_u8(0, *a), vocab, [0, 0], [0, 0])
    assert rc == 0 and np.all(hist[:8] == 0) and np.all(hist[8:] == 0xA5A5A5A5)
    rc, n, nb, scores, ed = _shortlist_dev(capi, np.zeros((0, 4), np.uint32), 2, False, 0)
    assert rc == 0 and n == 0 and np.all(nb == -7) and np.all(ed == -7)


@pytest.mark.parametrize("name", sorted(sc.SHORTLIST))
def test_device_shortlist_equals_the_reference(capi, name):
    """N in {1, 2, 33, 65}, k = 1 and k > N - 1, identical views, a view without rows, a pair with score 0, mutual or not:
    lists, scores and edges at the exact capacity"""
    hist, k, mutual = sc.shortlist_case(name)
    L = capi.lib()
    total = _once(("total", name), lambda: sc.raw_shortlist(capi, L.psx_shortlist_views_ref, hist, k, mutual, None, False))[1]
    want = _once(("shortlist", name, total, True), lambda: sc.raw_shortlist(capi, L.psx_shortlist_views_ref, hist, k, mutual, total))
    _same(_shortlist_dev(capi, hist, k, mutual, total), want, "dev")
    _same(sc.raw_shortlist(capi, lambda *a: L.psx_shortlist_views(0, *a), hist, k, mutual, total), want, "host form")


@pytest.mark.parametrize("name", ["n33_k35", "n65_k1_mutual"])
def test_edge_capacities(capi, name):
    """the exact capacity, one short, more than needed, 0 and NULL; with and without the list arrays"""
    hist, k, mutual = sc.shortlist_case(name)
    L = capi.lib()
    total = _once(("total", name), lambda: sc.raw_shortlist(capi, L.psx_shortlist_views_ref, hist, k, mutual, None, False))[1]
    assert total >= 3
    for cap, lists in ((total, False), (total - 1, True), (total + 2, True), (0, True), (None, True), (None, False)):
        want = _once(("shortlist", name, cap, lists), lambda: sc.raw_shortlist(capi, L.psx_shortlist_views_ref, hist, k, mutual, cap, lists))
        _same(_shortlist_dev(capi, hist, k, mutual, cap, lists), want, ("dev", cap, lists))
        _same(sc.raw_shortlist(capi, lambda *a: L.psx_shortlist_views(0, *a), hist, k, mutual, cap, lists), want, ("host form", cap, lists))


def test_planted_views_and_the_chain(capi):
    """24 planted views: psx_vocab_train_u8_dev -> psx_bow_u8_dev -> psx_shortlist_views_dev with the vocabulary and the
    histogram never leaving HBM; every output equals the reference bytewise, every list is the view's five group mates, and
    the edge list goes into psx_match_pairs_graph_u8_dev unchanged"""
    p = sc.PLANTED
    sets = sc.planted()
    lens = [len(s) for s in sets]
    N, W, k = len(sets), p["words"], p["k"]
    L = capi.lib()
    keep, adr = _device_sets(sets)
    vocab = torch.full((W * 128,), 0xA5, dtype=torch.uint8, device="cuda")
    hist = torch.full((N * W,), -7, dtype=torch.int32, device="cuda")
    nb = torch.full((N * k,), -7, dtype=torch.int32, device="cuda")
    scores = torch.full((N * k,), -7, dtype=torch.int32, device="cuda")
    edges = torch.full((2 * N * k,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    info = capi.vocab_train_u8_dev(adr, lens, W, p["iterations"], vocab.data_ptr())
    capi.bow_u8_dev(vocab.data_ptr(), W, adr, lens, hist.data_ptr())
    count = capi.shortlist_views_dev(hist.data_ptr(), N, W, k, nb.data_ptr(), scores.data_ptr(), edges.data_ptr(), N * k)
    # only now: the downloads and the reference
    want_vocab, want_info = capi.vocab_train_u8_ref(sets, W, p["iterations"])
    want_hist = capi.bow_u8_ref(want_vocab, sets)
    want = capi.shortlist_views_ref(want_hist, k)
    assert info == want_info and np.array_equal(vocab.cpu().numpy(), want_vocab.reshape(-1))
    assert np.array_equal(hist.cpu().numpy().view(np.uint32), want_hist.reshape(-1))
    assert np.array_equal(nb.cpu().numpy(), want["neighbours"].reshape(-1))
    assert np.array_equal(scores.cpu().numpy().view(np.uint32), want["scores"].reshape(-1))
    assert count == want["count"] == 60
    got_edges = edges.cpu().numpy()
    assert np.array_equal(got_edges[:2 * count], want["edges"].view(np.int32).reshape(-1)) and np.all(got_edges[2 * count:] == -7)
    for i in range(N):
        assert sorted(want["neighbours"][i]) == sc.planted_mates(i), i
    # the fifth call: the list as it came out
    edge_list = got_edges[:2 * count].reshape(-1, 2)
    room = int(sum(lens[a] for a, _ in edge_list))
    pairs = torch.full((room * 16,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    edge_counts, n = capi.match_pairs_graph_dev(adr, lens, edge_list, pairs.data_ptr(), room, 0.8, True)
    assert len(edge_counts) == count and n == int(edge_counts.sum()) and np.all(edge_counts >= 0) and np.any(edge_counts > 0)
    assert keep


def test_python_wrappers(capi):
    """capi.vocab_train_u8, bow_u8 and shortlist_views (which asks "how many?" first) against their _ref wrappers"""
    sets, words, iterations = sc.train_case("w33_t40")
    vocab, info = capi.vocab_train_u8(sets, words, iterations)
    want_vocab, want_info = capi.vocab_train_u8_ref(sets, words, iterations)
    assert info == want_info and np.array_equal(vocab, want_vocab)
    hist, rw = capi.bow_u8(vocab, sets, row_words=True)
    want_hist, want_rw = capi.bow_u8_ref(vocab, sets, row_words=True)
    assert np.array_equal(hist, want_hist) and np.array_equal(rw, want_rw)
    assert np.array_equal(capi.bow_u8(vocab, sets), want_hist)
    for k, mutual in ((2, False), (3, True)):
        got, want = capi.shortlist_views(hist, k, mutual), capi.shortlist_views_ref(hist, k, mutual)
        assert got["count"] == want["count"] and all(np.array_equal(got[f], want[f]) for f in ("neighbours", "scores", "edges"))
        assert got["edges"].tolist() == sc.shortlist(capi, hist, k, mutual)["edges"].tolist()
    assert capi.lib().psx_match_release() == 0


def test_cpp_vocabulary_on_the_gpu(tmp_path):
    """tests/cpp/test_shortlist_api.cpp with POPSIFT_TEST_EXPECT_GPU: popsift::Vocabulary end to end"""
    libdir = os.path.join(ROOT, "popsift_amd", "lib")
    exe = str(tmp_path / "test_shortlist_api")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-pthread", os.path.join(ROOT, "tests", "cpp", "test_shortlist_api.cpp"), "-o", exe,
                           "-I", os.path.join(ROOT, "popsift_amd", "csrc", "include"), "-I", os.path.join(ROOT, "include"),
                           "-L", libdir, "-lpopsift", "-lpopsift_hip", "-Wl,-rpath," + libdir])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300,
                         env=dict(os.environ, POPSIFT_TEST_EXPECT_GPU="1"))
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout
    assert "shortlist:" in out.stdout
