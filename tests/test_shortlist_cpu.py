"""The view shortlist without a GPU (include/popsift_hip.h, "WHICH PAIRS TO MATCH"): the host references
psx_vocab_train_u8_ref, psx_bow_u8_ref and psx_shortlist_views_ref against the numpy restatement of tests/shortlist_cases.py
on every case the GPU tests run, psx_bow_weights against numpy, the argument errors (outputs untouched), the capacity rules
on sentinel-filled arrays compared whole, a hand example, the planted views, and tests/cpp/shortlist_san.cpp: the same
reference code as a stand-alone program under -fsanitize=address,undefined."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import shortlist_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INFO_UNTOUCHED = (-77, -77, -77, -77, 77)


def _info(capi, raw):
    t = capi.VocabInfo.from_buffer_copy(raw)
    assert t.reserved == 0
    return dict(iterations=t.iterations, changed=t.changed, empty_words=t.empty_words, inertia=t.inertia)


@pytest.mark.parametrize("name", sorted(sc.TRAIN))
def test_training_reference_equals_numpy(capi, name):
    sets, words, iterations = sc.train_case(name)
    rc, info, vocab = sc.raw_train(capi, capi.lib().psx_vocab_train_u8_ref, sc.addresses_of(sets), [len(s) for s in sets], words, iterations)
    want, want_info = sc.train(sets, words, iterations)
    assert rc == 0 and _info(capi, info) == want_info
    assert np.array_equal(vocab[:words * 128], want.reshape(-1)) and np.all(vocab[words * 128:] == 0xA5)
    if iterations > 1:
        assert want_info["changed"] == 0 and 1 < want_info["iterations"] < iterations, "the early stop triggers"
        # stopping early gives the same words as running on
        again, _ = sc.train(sets, words, want_info["iterations"] - 1)
        assert np.array_equal(again, want)


@pytest.mark.parametrize("words", sc.WORDS)
def test_bow_reference_equals_numpy(capi, words):
    vocab, sets = sc.bow_case(words)
    lens = [len(s) for s in sets]
    rc, hist, rw = sc.raw_bow(capi, capi.lib().psx_bow_u8_ref, vocab, sc.addresses_of(sets), lens)
    want_hist, want_words = sc.bow(vocab, sets)
    assert rc == 0
    assert np.array_equal(hist[:-5], want_hist.reshape(-1)) and np.all(hist[-5:] == 0xA5A5A5A5)
    assert np.array_equal(rw[:-5], want_words) and np.all(rw[-5:] == -7)
    assert np.all(want_hist[4] == 0) and want_hist.sum() == sum(lens)                  # the empty view: a zero row
    if words >= 6:
        assert want_hist[:, words // 2].sum() == 0 and want_hist[:, 1].sum() >= 1      # a duplicated word loses every tie
    rc, hist2, rw2 = sc.raw_bow(capi, capi.lib().psx_bow_u8_ref, vocab, sc.addresses_of(sets), lens, row_words=False)
    assert rc == 0 and np.array_equal(hist2, hist) and np.all(rw2 == -7)


@pytest.mark.parametrize("name", sorted(sc.SHORTLIST))
def test_shortlist_reference_equals_numpy(capi, name):
    hist, k, mutual = sc.shortlist_case(name)
    want = sc.shortlist(capi, hist, k, mutual)
    rc, n, nb, scores, ed = sc.raw_shortlist(capi, capi.lib().psx_shortlist_views_ref, hist, k, mutual, want["count"])
    assert rc == 0 and n == want["count"]
    assert np.array_equal(nb[:-3], want["neighbours"].reshape(-1)) and np.all(nb[-3:] == -7)
    assert np.array_equal(scores[:-3], want["scores"].reshape(-1)) and np.all(scores[-3:] == 0xA5A5A5A5)
    assert np.array_equal(ed[:2 * n], want["edges"].view(np.int32).reshape(-1)) and np.all(ed[2 * n:] == -7)
    N = len(hist)
    if N >= 8:
        assert 3 not in want["neighbours"] and np.all(want["neighbours"][3] == -1)    # the view without rows
        assert 6 not in want["neighbours"][5] and 5 not in want["neighbours"][6]      # score 0: excluded even with k > N - 1
        assert want["neighbours"][0, 0] == 1 and want["neighbours"][1, 0] == 0        # identical views find each other first
        for i in range(8, N):                                                          # views 0 and 1 are identical: equal scores,
            row = list(want["neighbours"][i])                                          # the lower view first
            if 1 in row:
                assert row.index(0) + 1 == row.index(1), i
    if k > N - 1 and N >= 2:
        assert np.all(want["neighbours"][:, N - 1:] == -1) and np.all(want["scores"][:, N - 1:] == 0)
    if mutual:
        plain = sc.shortlist(capi, hist, k, False)
        assert set(want["edges"].tolist()) <= set(plain["edges"].tolist())
    assert want["edges"].tolist() == sorted(set(want["edges"].tolist()))


def test_weights_equal_numpy(capi):
    """1 + floor(16 log2(N / df) + 0.5) on every (N, df) whose fraction is more than 1e-9 away from the rounding boundary"""
    checked = 0
    for N in list(range(1, 70)) + [100, 1000, 4095, 4096]:
        df = np.arange(0, N + 1)
        x = 16.0 * np.log2(N / np.maximum(df, 1).astype(np.float64)) + 0.5
        clear = np.abs(x - np.round(x)) > 1e-9
        want = np.where(df > 0, 1 + np.floor(x).astype(np.int64), 0)
        got = capi.bow_weights(df, N)
        assert np.array_equal(got[clear], want[clear]), N
        checked += int(clear.sum())
        assert got[0] == 0 and got[N] == 1 and got.max() <= 193
    assert checked > 9000
    assert capi.lib().psx_bow_weights(None, 0, 1, None) == 0
    df = np.array([0, 2], np.int32)
    out = np.full((2,), -7, np.int32)
    for bad_df, n_views in (([0, 3], 2), ([-1, 1], 2), ([0, 0], 0)):
        df[:] = bad_df
        assert capi.lib().psx_bow_weights(sc.ptr(df), 2, n_views, sc.ptr(out)) == -1 and np.all(out == -7)


def test_argument_errors_leave_the_outputs_untouched(capi):
    L = capi.lib()
    sets = sc.clustered(1, (5, 0, 4))
    adr, lens = sc.addresses_of(sets), [5, 0, 4]
    untouched = bytes(capi.VocabInfo(*INFO_UNTOUCHED))
    for a, l, words, iterations in ((adr, lens, 1, 3), (adr, lens, 65537, 3), (adr, lens, 10, 3), (adr, lens, 3, 0), (adr, [5, -1, 4], 3, 3),
                                    ([adr[0], adr[1], 0], lens, 3, 3)):
        rc, info, vocab = sc.raw_train(capi, L.psx_vocab_train_u8_ref, a, l, words, iterations)
        assert rc == -1 and info == untouched and np.all(vocab == 0xA5), (words, iterations, l)
    o = capi.VocabOpts(3, 3)
    arr, la = sc.set_table(adr, lens)
    vocab = np.zeros((3 * 128,), np.uint8)
    info = capi.VocabInfo()
    assert L.psx_vocab_train_u8_ref(arr, sc.ptr(la), 3, None, sc.ptr(vocab), C.byref(info)) == -1
    assert L.psx_vocab_train_u8_ref(arr, sc.ptr(la), 3, C.byref(o), None, C.byref(info)) == -1
    assert L.psx_vocab_train_u8_ref(arr, sc.ptr(la), 3, C.byref(o), sc.ptr(vocab), None) == -1
    assert L.psx_vocab_train_u8_ref(None, sc.ptr(la), 3, C.byref(o), sc.ptr(vocab), C.byref(info)) == -1
    # an empty view with a NULL set is fine
    rc, info, _ = sc.raw_train(capi, L.psx_vocab_train_u8_ref, [adr[0], 0, adr[2]], lens, 3, 3)
    assert rc == 0 and info != untouched

    v = sc.vocabulary(2, 4)
    for vocab_arg, a, l in ((v[:0], adr, lens), (v, [0, 0, adr[2]], lens), (v, adr, [5, 0, -4])):
        rc, hist, rw = sc.raw_bow(capi, L.psx_bow_u8_ref, vocab_arg, a, l)
        assert rc == -1 and np.all(hist == 0xA5A5A5A5) and np.all(rw == -7)
    assert L.psx_bow_u8_ref(sc.ptr(v), 4, arr, sc.ptr(la), 3, None, None) == -1           # no histogram
    assert L.psx_bow_u8_ref(sc.ptr(v), 65537, arr, sc.ptr(la), 3, sc.ptr(np.zeros(12, np.uint32)), None) == -1

    hist = sc.hists(3, 8, 10)
    for k, flags in ((0, 0), (-1, 0), (2, 2), (2, 4)):
        n = C.c_int(-77)
        o = capi.ShortlistOpts(k, flags)
        nb = np.full((8 * 2,), -7, np.int32)
        assert L.psx_shortlist_views_ref(sc.ptr(hist), 8, 10, C.byref(o), sc.ptr(nb), None, None, 0, C.byref(n)) == -1
        assert n.value == -77 and np.all(nb == -7)
    o, n = capi.shortlist_opts(2), C.c_int(-77)
    big = np.zeros((4097, 1), np.uint32)
    assert L.psx_shortlist_views_ref(sc.ptr(big), 4097, 1, C.byref(o), None, None, None, 0, C.byref(n)) == -1
    assert L.psx_shortlist_views_ref(None, 8, 10, C.byref(o), None, None, None, 0, C.byref(n)) == -1
    assert L.psx_shortlist_views_ref(sc.ptr(hist), 8, 10, None, None, None, None, 0, C.byref(n)) == -1
    assert L.psx_shortlist_views_ref(sc.ptr(hist), 8, 10, C.byref(o), None, None, None, 0, None) == -1
    assert L.psx_shortlist_views_ref(sc.ptr(hist), 8, 10, C.byref(o), None, None, None, 1, C.byref(n)) == -1     # a capacity without an array
    assert L.psx_shortlist_views_ref(sc.ptr(hist), 8, 10, C.byref(o), None, None, None, -1, C.byref(n)) == -1
    assert L.psx_shortlist_views_ref(sc.ptr(hist), 8, 0, C.byref(o), None, None, None, 0, C.byref(n)) == -1
    assert n.value == -77
    assert L.psx_shortlist_views_ref(sc.ptr(big), 4096, 1, C.byref(o), None, None, None, 0, C.byref(n)) == 0 and n.value == 0


def test_empty_forms(capi):
    L = capi.lib()
    v = sc.vocabulary(2, 4)
    rc, hist, rw = sc.raw_bow(capi, L.psx_bow_u8_ref, v, [0, 0], [0, 0])
    assert rc == 0 and np.all(hist[:8] == 0) and np.all(hist[8:] == 0xA5A5A5A5) and np.all(rw == -7)
    rc, hist, rw = sc.raw_bow(capi, L.psx_bow_u8_ref, v, [], [])
    assert rc == 0 and np.all(hist == 0xA5A5A5A5)
    rc, n, nb, scores, ed = sc.raw_shortlist(capi, L.psx_shortlist_views_ref, np.zeros((0, 4), np.uint32), 2, False, 0)
    assert rc == 0 and n == 0 and np.all(nb == -7) and np.all(ed == -7)
    rc, n, nb, scores, ed = sc.raw_shortlist(capi, L.psx_shortlist_views_ref, np.ones((1, 4), np.uint32), 2, False, 0)
    assert rc == 0 and n == 0 and list(nb) == [-1, -1, -7, -7, -7] and list(scores[:2]) == [0, 0]


@pytest.mark.parametrize("name", ["n33_k35", "n65_k1_mutual", "n8_disjoint"])
def test_capacities(capi, name):
    """the exact capacity, one short, a cut in the middle, more than needed, 0 and NULL; with and without the list arrays: the
    count is always the total and nothing at or past the capacity is touched"""
    hist, k, mutual = sc.shortlist_case(name)
    want = sc.shortlist(capi, hist, k, mutual)
    total = want["count"]
    assert total >= 3
    words = want["edges"].view(np.int32).reshape(-1)
    for cap, lists in ((total, True), (total - 1, True), (total // 2, False), (total + 2, False), (0, True), (None, True), (None, False)):
        rc, n, nb, scores, ed = sc.raw_shortlist(capi, capi.lib().psx_shortlist_views_ref, hist, k, mutual, cap, lists)
        kept = min(total, cap or 0)
        assert rc == 0 and n == total
        assert np.array_equal(ed[:2 * kept], words[:2 * kept]) and np.all(ed[2 * kept:] == -7), cap
        assert np.array_equal(nb[:-3], want["neighbours"].reshape(-1)) if lists else np.all(nb == -7)


def _rows(first_bytes):
    r = np.zeros((len(first_bytes), 128), np.uint8)
    r[:, 0] = first_bytes
    return r


def test_hand_example(capi):
    """two views, six rows that differ in their first byte: 10 13 10 11 | 100 101, three words from rows 0, 2 and 4.
    Iteration 1: words 0 and 1 are the same row, every tie goes to word 0, word 1 stays empty and keeps its bytes; word 0
    becomes 44 / 4 = 11 and word 2 becomes 100.5, rounded UP to 101.  Iteration 2: the rows at 10 move to word 1, word 0
    becomes 12.  Iteration 3: row 3 (11) is as far from word 0 (12) as from word 1 (10) and stays with the lower; nothing moves."""
    sets = [_rows([10, 13, 10, 11]), _rows([100, 101])]
    vocab, info = capi.vocab_train_u8_ref(sets, 3, 1)
    assert list(vocab[:, 0]) == [11, 10, 101] and not vocab[:, 1:].any()
    assert info == dict(iterations=1, changed=6, empty_words=1, inertia=11)
    vocab, info = capi.vocab_train_u8_ref(sets, 3, 10)
    assert list(vocab[:, 0]) == [12, 10, 101] and info == dict(iterations=3, changed=0, empty_words=0, inertia=3)
    assert capi.vocab_train_u8_ref(sets, 3, 2)[1] == dict(iterations=2, changed=2, empty_words=0, inertia=5)
    hist, words = capi.bow_u8_ref(vocab, sets, row_words=True)
    assert hist.tolist() == [[2, 2, 0], [0, 0, 2]] and list(words) == [1, 0, 1, 0, 2, 2]
    # three views over two words: df = (3, 2), weights (1, 10), q = (32767, 32767) twice and (65535, 0)
    h = np.array([[1, 1], [1, 1], [2, 0]], np.uint32)
    assert list(capi.bow_weights([3, 2], 3)) == [1, 10]
    got = capi.shortlist_views_ref(h, 1)
    assert got["neighbours"].tolist() == [[1], [0], [0]] and got["scores"].tolist() == [[360437], [360437], [32767]]
    assert got["edges"].tolist() == [(0, 1), (0, 2)] and got["count"] == 2
    assert capi.shortlist_views_ref(h, 1, mutual=True)["edges"].tolist() == [(0, 1)]
    got = capi.shortlist_views_ref(h, 4)
    assert got["neighbours"].tolist() == [[1, 2, -1, -1], [0, 2, -1, -1], [0, 1, -1, -1]]
    assert got["edges"].tolist() == [(0, 1), (0, 2), (1, 2)]
    assert capi.shortlist_views_ref(h, 4, capacity=2)["edges"].tolist() == [(0, 1), (0, 2)]


def test_planted_views_shortlist_their_group_mates(capi):
    """the usefulness condition, on the REFERENCE: 24 views in 4 groups of 6, W = 256, T = 8, k = 5 -- every view's list is
    exactly its five group mates"""
    p = sc.PLANTED
    sets = sc.planted()
    assert len(sets) == 24 and all(len(s) == 300 for s in sets)
    vocab, info = capi.vocab_train_u8_ref(sets, p["words"], p["iterations"])
    hist = capi.bow_u8_ref(vocab, sets)
    got = capi.shortlist_views_ref(hist, p["k"])
    for i in range(24):
        assert sorted(got["neighbours"][i]) == sc.planted_mates(i), i
    assert got["count"] == 4 * 15 and got["edges"].tolist() == [(a, b) for a in range(24) for b in sc.planted_mates(a) if b > a]
    assert capi.shortlist_views_ref(hist, p["k"], mutual=True)["count"] == 60


def test_reference_program_under_sanitizers(tmp_path):
    """tests/cpp/shortlist_san.cpp: bow_rule.h and bow_plan.h -- the code behind the _ref entry points -- compiled by g++
    with -fsanitize=address,undefined, on the hand example and the capacity cuts"""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed"
    exe = str(tmp_path / "shortlist_san")
    subprocess.check_call([cxx, "-std=c++14", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           "-static-libasan", "-static-libubsan", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "shortlist_san.cpp"),
                           "-o", exe, "-I", os.path.join(ROOT, "popsift_amd", "csrc", "hip"), "-I", os.path.join(ROOT, "include")])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout


def test_rule_header_is_host_clean():
    """bow_rule.h and bow_plan.h name no HIP header: g++ compiles them alone"""
    for f in ("bow_rule.h", "bow_plan.h"):
        text = open(os.path.join(ROOT, "popsift_amd", "csrc", "hip", f)).read()
        assert "hip_runtime" not in text and "psx_internal" not in text, f


def test_cpp_vocabulary_argument_errors(tmp_path):
    """tests/cpp/test_shortlist_api.cpp without a GPU: popsift::Vocabulary refuses bad arguments before any device call"""
    libdir = os.path.join(ROOT, "popsift_amd", "lib")
    exe = str(tmp_path / "test_shortlist_api")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-pthread", os.path.join(ROOT, "tests", "cpp", "test_shortlist_api.cpp"), "-o", exe,
                           "-I", os.path.join(ROOT, "popsift_amd", "csrc", "include"), "-I", os.path.join(ROOT, "include"),
                           "-L", libdir, "-lpopsift", "-lpopsift_hip", "-Wl,-rpath," + libdir])
    env = {k: v for k, v in os.environ.items() if k != "POPSIFT_TEST_EXPECT_GPU"}
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120, env=env)
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout
