"""GPU tests of tracks over an edge list (include/popsift_hip.h, "TRACKS FROM A LIST OF VIEW PAIRS"): psx_tracks_graph_dev and
psx_tracks_graph on the smallest shapes at which the kernels can go wrong, the four-call chain on records that never leave
HBM, the python wrapper and FeaturesDev::buildTracks.  Every comparison is as bytes against the host reference
psx_tracks_graph_ref, called with the same capacities on arrays filled with the same sentinels: whole buffers are compared,
so nothing may be written past the range the rule names."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch        # before the HIP library is loaded: torch brings a HIP runtime of its own and must initialise first (_dev forms)

from tests import graph_chain_cases as gc
from tests import tracks_cases as tc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_REF = {}


def _ref(capi, name, option, tcap, mcap, with_labels=True):
    """psx_tracks_graph_ref on sentinel-filled arrays, computed once per (case, options, capacities) and never changed"""
    key = (name, option, tcap, mcap, with_labels)
    if key not in _REF:
        _REF[key] = tc.raw_call(capi, capi.lib().psx_tracks_graph_ref, tc.CASES[name](), capi.track_opts(*option), tcap, mcap, with_labels)
    return _REF[key]


def _totals(capi, name, option):
    rc, info, _, _, _ = _ref(capi, name, option, None, None, False)
    assert rc == 0
    t = capi.TracksInfo.from_buffer_copy(info)
    return t.tracks, t.members


def _dev(capi, case, option, tcap, mcap, with_labels=True, slack=3):
    """psx_tracks_graph_dev on torch buffers filled with the sentinel -7: (rc, info bytes, labels, starts, members words)"""
    pairs = tc.concat(case["lists"])
    src = torch.from_numpy(pairs.view(np.uint8).copy()).cuda() if len(pairs) else None
    M = int(sum(case["lens"]))
    labels = torch.full((M + slack,), -7, dtype=torch.int32, device="cuda")
    starts = torch.full(((tcap or 0) + 1 + slack,), -7, dtype=torch.int32, device="cuda")
    members = torch.full((2 * ((mcap or 0) + slack),), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    vp = lambda t: C.c_void_p(t.data_ptr())
    ec = np.array([len(p) for p in case["lists"]], np.int32)
    ea = np.array(case["edges"], np.int32).reshape(-1, 2)
    la = np.array(case["lens"], np.int32)
    info = capi.TracksInfo(-77, -77, -77, -77, -77, -77)
    o = capi.track_opts(*option)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None
    rc = capi.lib().psx_tracks_graph_dev(0, vp(src) if src is not None else None, ptr(ec), ptr(ea), len(ea), ptr(la), len(la), C.byref(o),
                                         vp(labels) if with_labels else None, vp(starts) if tcap is not None else None, tcap or 0,
                                         vp(members) if mcap is not None else None, mcap or 0, C.byref(info))
    if src is not None:
        assert np.array_equal(src.cpu().numpy(), pairs.view(np.uint8)), "the input is only read"
    return rc, bytes(info), labels.cpu().numpy(), starts.cpu().numpy(), members.cpu().numpy()


def _same(got, want, what):
    assert got[0] == want[0] == 0, what
    assert got[1] == want[1], (what, np.frombuffer(got[1], np.int32), np.frombuffer(want[1], np.int32))
    for k, part in ((2, "labels"), (3, "starts"), (4, "members")):
        assert np.array_equal(got[k], want[k]), (what, part)


@pytest.mark.parametrize("option", tc.OPTIONS, ids=tc.OPTION_IDS)
@pytest.mark.parametrize("name", sorted(tc.CASES))
def test_device_tracks_equal_the_reference(capi, name, option):
    """the deep chain in reversed and shuffled order, the contention case, the block edges, duplicate / reversed / self edges,
    the hand example and a scattered graph; min_views 2 and 3, both flag values; device and host form at the exact capacity"""
    tracks, members = _totals(capi, name, option)
    case = tc.CASES[name]()
    want = _ref(capi, name, option, tracks, members)
    _same(_dev(capi, case, option, tracks, members), want, "dev")
    L = capi.lib()
    _same(tc.raw_call(capi, lambda *a: L.psx_tracks_graph(0, *a), case, capi.track_opts(*option), tracks, members), want, "host form")
    if name == "contention":
        t = capi.TracksInfo.from_buffer_copy(want[1])
        assert (t.tracks, t.members, t.conflicts, t.components) == ((1, 900, 1, 1) if option[1] else (0, 0, 1, 1))
    if name.startswith("chain"):
        assert capi.TracksInfo.from_buffer_copy(want[1]).members == 70


@pytest.mark.parametrize("name,option", [("scattered", (2, False)), ("contention", (2, True)), ("block_edges", (2, True))])
def test_capacities(capi, name, option):
    """the exact capacity, one member short (a cut inside the last track), one track short, a cut in the middle, and 0 / NULL;
    labels NULL and non-NULL: the totals are always reported and nothing at or past a capacity is touched"""
    tracks, members = _totals(capi, name, option)
    assert tracks >= 1 and members >= 2
    case = tc.CASES[name]()
    for tcap, mcap, with_labels in ((tracks, members, False), (tracks, members - 1, True), (tracks - 1, members, True),
                                    (tracks // 2, members // 2 + 1, True), (0, 0, False), (None, None, True), (None, None, False),
                                    (tracks + 2, None, False), (None, members + 2, False)):
        _same(_dev(capi, case, option, tcap, mcap, with_labels), _ref(capi, name, option, tcap, mcap, with_labels), (tcap, mcap, with_labels))


def test_out_of_range_record_refuses_the_call_and_a_good_call_follows(capi):
    """ONE record whose right row equals its own edge's right length -- in range for a longer view -- gives PSX_ERR_INVALID
    through the device flag, info and the host outputs untouched; the next valid call on the same device succeeds"""
    name, option = "dup_rev_self", (2, False)
    good = tc.CASES[name]()
    bad = dict(good, lists=[p.copy() for p in good["lists"]])
    bad["lists"][0]["right"][7] = bad["lens"][bad["edges"][0][1]]  # edge (0, 1): right == lens[1] = 37 < lens[0] = 40
    assert bad["lens"][bad["edges"][0][1]] < max(bad["lens"])
    assert tc.restate(bad["lists"], bad["edges"], bad["lens"]) is None
    L = capi.lib()
    tracks, members = _totals(capi, name, option)
    rc, info, labels, starts, mem = tc.raw_call(capi, lambda *a: L.psx_tracks_graph(0, *a), bad, capi.track_opts(*option), tracks, members)
    assert rc == -1 and info == bytes(capi.TracksInfo(-77, -77, -77, -77, -77, -77))
    assert np.all(labels == -7) and np.all(starts == -7) and np.all(mem == -7)
    rc, info, _, _, _ = _dev(capi, bad, option, tracks, members)
    assert rc == -1 and info == bytes(capi.TracksInfo(-77, -77, -77, -77, -77, -77))
    assert tc.raw_call(capi, L.psx_tracks_graph_ref, bad, capi.track_opts(*option), tracks, members)[0] == -1
    _same(_dev(capi, good, option, tracks, members), _ref(capi, name, option, tracks, members), "the call after the refused one")


def test_two_calls_give_the_same_bytes(capi):
    """the contention case twice in one process: hundreds of lanes race for one root, the outputs are equal as bytes"""
    case = tc.CASES["contention"]()
    first = _dev(capi, case, (2, True), 1, 900)
    second = _dev(capi, case, (2, True), 1, 900)
    _same(first, second, "run to run")
    _same(first, _ref(capi, "contention", (2, True), 1, 900), "against the reference")


CHAIN_LENS = (300, 257, 64, 129, 513, 200)
CHAIN_EDGES = [(a, b) for a in range(6) for b in range(6) if a != b]


def test_chain_on_the_device(capi):
    """psx_match_pairs_graph_u8_dev -> psx_ransac_homography_graph_dev -> psx_tracks_graph_dev on the inlier buffer with
    results[e].inliers as counts, on six planted views and all 30 ordered pairs; nothing is downloaded between the calls.
    The inliers are downloaded once afterwards: the device tracks equal psx_tracks_graph_ref of them.  The same on the
    matcher's psx_match_pair_u8 records directly."""
    sets, xys, _ = gc.scene(43, CHAIN_LENS)
    edges, lens = CHAIN_EDGES, list(CHAIN_LENS)
    room = sum(CHAIN_LENS[a] for a, _ in edges)
    M = sum(lens)
    L, bufs = capi.lib(), []
    try:
        pxy = [p.value for p in capi._to_device(L, 0, [np.ascontiguousarray(x, np.float32) for x in xys], bufs)]
        pdesc = [p.value for p in capi._to_device(L, 0, [np.ascontiguousarray(s, np.uint8) for s in sets], bufs)]
        d_pairs, d_inl = (torch.full((room * 16,), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(2))
        outs = {}
        for which in ("inliers", "pairs"):
            outs[which] = (torch.full((M + 3,), -7, dtype=torch.int32, device="cuda"), torch.full((M // 2 + 1 + 3,), -7, dtype=torch.int32, device="cuda"),
                           torch.full((2 * (M + 3),), -7, dtype=torch.int32, device="cuda"))
        torch.cuda.synchronize()
        ec, n1 = capi.match_pairs_graph_dev(pdesc, lens, edges, d_pairs.data_ptr(), room, 0.8, True)
        g = capi.ransac_homography_graph_dev(d_pairs.data_ptr(), ec, edges, pxy, lens, d_inl.data_ptr(), room, capi.ransac_opts(gc.TOL, 256, 9, True))
        ic = [r.inliers for r in g["results"]]
        info = {}
        for which, buf, counts in (("inliers", d_inl, ic), ("pairs", d_pairs, ec)):
            lab, st, mem = outs[which]
            info[which] = capi.tracks_graph_dev(buf.data_ptr(), counts, edges, lens, lab.data_ptr(), st.data_ptr(), M // 2, mem.data_ptr(), M)
        # only now: the downloads
        for which, buf, counts, n in (("inliers", d_inl, ic, g["count"]), ("pairs", d_pairs, list(ec), n1)):
            recs = buf.cpu().numpy()[:n * 16].view(tc.PAIR_U8)
            case = dict(lens=lens, edges=edges, lists=capi.split_sets(recs, counts))
            want = tc.raw_call(capi, L.psx_tracks_graph_ref, case, capi.track_opts(), M // 2, M)
            t = capi.TracksInfo.from_buffer_copy(want[1])
            assert want[0] == 0 and {k: getattr(t, k) for k in tc.TOTALS} == info[which], which
            lab, st, mem = (x.cpu().numpy() for x in outs[which])
            assert np.array_equal(lab, want[2]) and np.array_equal(st, want[3]) and np.array_equal(mem, want[4]), which
            assert t.tracks > 50 and t.members >= 2 * t.tracks, (which, t.tracks)
        assert sum(ic) == g["count"] > 100
    finally:
        for p in bufs:
            L.psx_dev_free(0, p)


def test_python_wrapper(capi):
    """capi.tracks_graph asks "how many?" and then fills arrays of that size: the dict of capi.tracks_graph_ref"""
    for name in ("scattered", "hand"):
        case = tc.CASES[name]()
        for option in tc.OPTIONS[:2]:
            got = capi.tracks_graph(case["lists"], case["edges"], case["lens"], capi.track_opts(*option))
            assert tc.same(got, capi.tracks_graph_ref(case["lists"], case["edges"], case["lens"], capi.track_opts(*option))) is None, (name, option)
            assert tc.same(got, tc.restate(case["lists"], case["edges"], case["lens"], *option)) is None, (name, option)
    assert capi.lib().psx_match_release() == 0


def test_cpp_build_tracks_on_the_gpu(tmp_path):
    """tests/cpp/test_tracks_api.cpp with POPSIFT_TEST_EXPECT_GPU: FeaturesDev::buildTracks equals a union-find looped over
    `matches` on the host"""
    libdir = os.path.join(ROOT, "popsift_amd", "lib")
    exe = str(tmp_path / "test_tracks_api")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-pthread", os.path.join(ROOT, "tests", "cpp", "test_tracks_api.cpp"), "-o", exe,
                           "-I", os.path.join(ROOT, "popsift_amd", "csrc", "include"), "-I", os.path.join(ROOT, "include"),
                           "-L", libdir, "-lpopsift", "-lpopsift_hip", "-Wl,-rpath," + libdir])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300,
                         env=dict(os.environ, POPSIFT_TEST_EXPECT_GPU="1"))
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout
    assert "buildTracks:" in out.stdout
