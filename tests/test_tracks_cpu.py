"""CPU tests of tracks over an edge list (include/popsift_hip.h, "TRACKS FROM A LIST OF VIEW PAIRS"): the declarations and
bindings of psx_tracks_graph, _dev, _ref and psx_tracks_plan; the host reference against the independent restatement of
tests/tracks_cases.py and against one example written out by hand; every argument error, before a device is looked at and
with the outputs untouched; the forms that need no device; the capacity rule; the plan against figures computed by hand; a
stand-alone sanitizer build of tracks_plan.h; the C++ API's argument errors."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import tracks_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_MAX = 2 ** 31 - 1
DEVICE = ("psx_tracks_graph", "psx_tracks_graph_dev")
ALL = DEVICE + ("psx_tracks_graph_ref", "psx_tracks_plan")


def test_entry_points_declared_and_bound(capi):
    hdr = open(os.path.join(ROOT, "include", "popsift_hip.h")).read()
    for sym in ALL:
        assert "int %s(" % sym in hdr and sym in capi.SYMBOLS and hasattr(capi.lib(), sym), sym
    for name in ("tracks_graph", "tracks_graph_dev", "tracks_graph_ref", "tracks_plan"):
        assert callable(getattr(capi, name)), name
    for text in ("#define PSX_TRACKS_KEEP_CONFLICTS 1", "typedef struct psx_track_opts", "typedef struct psx_track_member",
                 "typedef struct psx_tracks_info", "typedef struct psx_tracks_plan_info"):
        assert text in hdr, text
    assert hdr.index("TRACKS FROM A LIST OF VIEW PAIRS") > hdr.index("A LIST OF VIEW PAIRS IN ONE CALL")
    assert C.sizeof(capi.TracksInfo) == 24 and C.sizeof(capi.TrackOpts) == 8 and tc.MEMBER.itemsize == 8 == capi.TRACK_MEMBER_DTYPE.itemsize
    from popsift_amd import build
    cm = open(os.path.join(ROOT, "CMakeLists.txt")).read()
    assert "tracks.hip" in build.HIP_SOURCES and " tracks " in cm
    hip = os.path.join(ROOT, "popsift_amd", "csrc", "hip")
    for plain in ("tracks_plan.h", "tracks_rule.h"):
        text = open(os.path.join(hip, plain)).read()
        assert "hip/hip_runtime.h" not in text and "__global__" not in text and "rocprim" not in text, plain
    assert "__device__" not in open(os.path.join(hip, "tracks_plan.h")).read()                # plain C++
    src = open(os.path.join(hip, "tracks.hip")).read()
    for piece in ('#include "tracks_plan.h"', "psx_track_keep(", "psx_track_link(", "psx_track_record_ok(", "wg_scan_totals(",
                  "rocprim::radix_sort_pairs(", "__HIP_MEMORY_SCOPE_AGENT", "psx_tracks_args_ok("):
        assert piece in src, piece
    assert src.count("hipStreamSynchronize(") == 1                                            # one synchronisation per call
    scratch = open(os.path.join(hip, "match_scratch.h")).read()
    for slot in ("MS_TRACKS_TABLES", "MS_TRACKS_PAIRS", "MS_TRACKS_NODES", "MS_TRACKS_SORT", "MS_TRACKS_TOT", "MS_TRACKS_STATE", "MS_TRACKS_OUT"):
        assert slot in scratch and slot in src, slot
    assert "MS_RANSAC_" not in src and "MS_RGRAPH_" not in src and "MS_GRAPH_" not in src
    fh = open(os.path.join(ROOT, "popsift_amd", "csrc", "include", "popsift", "features.h")).read()
    assert "buildTracks(" in fh and "struct Tracks" in fh and "struct TrackOptions" in fh
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "Tracks from a list of view pairs" in doc
    assert doc.index("Tracks from a list of view pairs") > doc.index("Verify and re-match a list of view pairs")


@pytest.mark.parametrize("option", tc.OPTIONS, ids=tc.OPTION_IDS)
@pytest.mark.parametrize("name", sorted(tc.CASES))
def test_reference_equals_the_restatement(capi, name, option):
    case = tc.CASES[name]()
    want = tc.restate(case["lists"], case["edges"], case["lens"], *option)
    got = capi.tracks_graph_ref(case["lists"], case["edges"], case["lens"], capi.track_opts(*option))
    assert tc.same(got, want) is None, tc.same(got, want)
    assert got["starts"][0] == 0 and got["starts"][-1] == got["members"] and len(got["starts"]) == got["tracks"] + 1
    assert np.all(np.diff(got["starts"]) >= 2)
    # records of the float matcher's dtype are the same 16 bytes
    if name == "scattered":
        f32 = np.dtype([("left", "<i4"), ("right", "<i4"), ("d1", "<f4"), ("d2", "<f4")])
        again = capi.tracks_graph_ref([p.view(f32) for p in case["lists"]], case["edges"], case["lens"], capi.track_opts(*option))
        assert tc.same(again, got) is None


def test_cases_cover_what_they_claim(capi):
    """the shapes the GPU tests lean on are what their names say"""
    c = tc.CASES["chain_reversed"]()
    assert len(c["lens"]) == 70 and set(c["lens"]) == {1, 2, 3} and c["edges"][0] == (68, 69) and c["edges"][-1] == (0, 1)
    s = tc.CASES["chain_shuffled"]()
    assert sorted(s["edges"]) == sorted(c["edges"]) and s["edges"] != c["edges"] and s["edges"] != c["edges"][::-1]
    for case in (c, s):
        r = tc.restate(case["lists"], case["edges"], case["lens"])
        assert (r["tracks"], r["members"], r["components"], r["conflicts"]) == (1, 70, 1, 0)
    k = tc.CASES["contention"]()
    assert k["lens"] == (300, 300, 300) and sum(len(p) for p in k["lists"]) == 900
    r0, r1 = tc.restate(k["lists"], k["edges"], k["lens"]), tc.restate(k["lists"], k["edges"], k["lens"], 2, True)
    assert (r0["tracks"], r0["conflicts"], r0["components"]) == (0, 1, 1) and (r1["tracks"], r1["members"]) == (1, 900)
    b = tc.CASES["block_edges"]()
    assert {0, 1, 255, 256, 257, 513} <= {len(p) for p in b["lists"]} and {0, 1, 63, 64, 65, 257} <= set(b["lens"])
    assert any(len(p) == 0 and 0 in (b["lens"][l], b["lens"][r]) for p, (l, r) in zip(b["lists"], b["edges"]))
    rb = tc.restate(b["lists"], b["edges"], b["lens"])
    assert rb["tracks"] >= 60 and rb["conflicts"] >= 1 and rb["too_few_views"] >= 1
    d = tc.CASES["dup_rev_self"]()
    e = d["edges"]
    assert e.count((0, 1)) == 2 and (1, 0) in e and (2, 2) in e and (1, 2) in e and (2, 1) in e
    loops = d["lists"][e.index((2, 2))]
    assert np.sum(loops["left"] == loops["right"]) == 3 and np.sum(loops["left"] != loops["right"]) == 1


@pytest.mark.parametrize("option", sorted(tc.HAND_EXPECTED), ids=lambda o: "v%d%s" % (o[0], "_keep" if o[1] else ""))
def test_reference_equals_the_example_written_out_by_hand(capi, option):
    """4 views, 5 edges: a duplicate edge, a reversed edge, a self edge with a self-loop and one conflict, one conflict
    component across views, two two-view tracks, one node alone"""
    want = tc.HAND_EXPECTED[option]
    got = capi.tracks_graph_ref(tc.HAND["lists"], tc.HAND["edges"], tc.HAND["lens"], capi.track_opts(*option))
    for k in tc.TOTALS:
        assert got[k] == want[k], k
    assert got["starts"].tolist() == want["starts"] and got["labels"].tolist() == want["labels"]
    assert [tuple(m) for m in got["member_records"].tolist()] == want["member_records"]


def _call(capi, fn, is_ref, **kw):
    """one call with sentinel-filled outputs and pointers that are never dereferenced on an error return (they are not
    device memory: this runs without a GPU); asserts that nothing was written and returns the return value"""
    fake = 0x1000
    a = dict(pairs=fake, counts=(9, 12), edges=((0, 1), (2, 0)), n_edges=2, lens=(40, 30, 30), n_sets=3, opts=capi.track_opts(), labels=True,
             starts=True, tcap=4, members=True, mcap=6, info=True)
    a.update(kw)
    ec = np.array(a["counts"], np.int32) if a["counts"] is not None else None
    ea = np.array(a["edges"], np.int32).reshape(-1, 2) if a["edges"] is not None else None
    la = np.array(a["lens"], np.int32) if a["lens"] is not None else None
    labels, starts, members = np.full(128, -7, np.int32), np.full(16, -7, np.int32), np.full(32, -7, np.int32)
    info = capi.TracksInfo(-77, -77, -77, -77, -77, -77)
    ptr = lambda x: x.ctypes.data_as(C.c_void_p) if x is not None else None
    pick = lambda arr, want: (want if isinstance(want, int) and not isinstance(want, bool) else ptr(arr)) if want else None
    args = [a["pairs"], ptr(ec), ptr(ea), a["n_edges"], ptr(la), a["n_sets"], C.byref(a["opts"]) if a["opts"] is not None else None,
            pick(labels, a["labels"]), pick(starts, a["starts"]), a["tcap"], pick(members, a["members"]), a["mcap"],
            C.byref(info) if a["info"] else None]
    rv = fn(*args) if is_ref else fn(0, *args)
    assert np.all(labels == -7) and np.all(starts == -7) and np.all(members == -7) and bytes(info) == bytes(capi.TracksInfo(*[-77] * 6))
    return rv


def test_argument_errors_touch_nothing(capi):
    """every PSX_ERR_INVALID of the header, with sentinels in every output, for the two device forms (before any device call:
    this runs without one) and the host reference"""
    L = capi.lib()
    for name in DEVICE + ("psx_tracks_graph_ref",):
        fn, is_ref = getattr(L, name), name.endswith("_ref")
        call = lambda **kw: _call(capi, fn, is_ref, **kw)
        for o in (capi.TrackOpts(1, 0), capi.TrackOpts(0, 0), capi.TrackOpts(-3, 1), capi.TrackOpts(2, 2), capi.TrackOpts(2, -1), capi.TrackOpts(2, 3)):
            assert call(opts=o) == -1, (name, o.min_views, o.flags)
        assert call(opts=None) == -1 and call(info=False) == -1, name
        assert call(tcap=-1) == -1 and call(mcap=-1) == -1, name
        assert call(starts=False, tcap=4) == -1 and call(members=False, mcap=6) == -1, name
        assert call(pairs=None) == -1, name
        # what the graph RANSAC call refuses about edge_counts, edges, n_edges, lens, n_sets
        assert call(n_edges=-1) == -1 and call(counts=None) == -1 and call(edges=None) == -1, name
        assert call(counts=(9, -1)) == -1, name
        assert call(counts=(0x3fffffff, 1)) == -1, name                                       # the sum of the counts above 0x3fffffff
        assert call(n_sets=-1) == -1 and call(lens=None) == -1, name
        assert call(lens=(40, -1, 30)) == -1, name
        for bad in ((0, 3), (3, 0), (-1, 0), (0, -1), (INT_MAX, 0)):
            assert call(edges=((0, 1), bad)) == -1, (name, bad)                               # every edge is checked, not only the first
        assert call(lens=None, n_sets=0) == -1, name                                          # no sets: no edge is in range
        assert call(lens=(0x3fffffff, 1, 30), counts=(0, 0)) == -1, name                      # M above 0x3fffffff
        assert call(lens=(2 ** 30, 5, 4), edges=((0, 1), (0, 2), (0, 0)), counts=(0, 0, 0), n_edges=3) == -1, name      # sum of lens[left]
        # records on an edge with an empty side: no row can lie inside it
        assert call(lens=(40, 0, 30)) == -1 and call(lens=(0, 30, 30)) == -1, name
        if not is_ref:
            # misaligned device pointers: records 16 bytes, members 8, ints 4
            if name.endswith("_dev"):
                assert call(pairs=0x1008) == -1 and call(members=0x1004) == -1 and call(starts=0x1002) == -1 and call(labels=0x1001) == -1, name
    # a record outside its own edge's views, in range for a longer one: the reference refuses the whole call, nothing written
    case = tc.CASES["dup_rev_self"]()
    bad = dict(case, lists=[p.copy() for p in case["lists"]])
    bad["lists"][0]["right"][7] = case["lens"][1]
    assert case["lens"][1] < max(case["lens"])
    rc, info, labels, starts, members = tc.raw_call(capi, L.psx_tracks_graph_ref, bad, capi.track_opts(), 40, 100)
    assert rc == -1 and info == bytes(capi.TracksInfo(*[-77] * 6)) and np.all(labels == -7) and np.all(starts == -7) and np.all(members == -7)
    bad["lists"][0]["right"][7] = -1
    assert tc.raw_call(capi, L.psx_tracks_graph_ref, bad, capi.track_opts(), 40, 100)[0] == -1


def test_forms_without_a_join_need_no_device(capi):
    """n_edges = 0, all counts zero, M = 0: zero totals and PSX_OK without a device (this runs without one); labels all -1 and
    track_starts[0] = 0 where a host array is given; the _dev form writes nothing (its pointers are fake here)"""
    L = capi.lib()
    zero = bytes(capi.TracksInfo(0, 0, 0, 0, 0, 0))
    empty = [dict(lens=(5, 0, 7), edges=[], lists=[]),
             dict(lens=(5, 0, 7), edges=[(0, 2), (1, 1), (2, 0)], lists=[tc.records([], [])] * 3),
             dict(lens=(0, 0), edges=[(0, 1), (1, 1)], lists=[tc.records([], [])] * 2),
             dict(lens=(), edges=[], lists=[])]
    for case in empty:
        M = sum(case["lens"])
        for fn in (L.psx_tracks_graph_ref, lambda *a: L.psx_tracks_graph(0, *a)):
            rc, info, labels, starts, members = tc.raw_call(capi, fn, case, capi.track_opts(), 2, 3, pairs_ptr=0x1000)
            assert rc == 0 and info == zero and np.all(labels[:M] == -1) and np.all(labels[M:] == -7), case["lens"]
            assert starts[0] == 0 and np.all(starts[1:] == -7) and np.all(members == -7)
            rc, info, labels, starts, members = tc.raw_call(capi, fn, case, capi.track_opts(3, True), None, None, with_labels=False)
            assert rc == 0 and info == zero and np.all(labels == -7) and np.all(starts == -7) and np.all(members == -7)
        ec = np.array([len(p) for p in case["lists"]], np.int32)
        ea, la = np.array(case["edges"], np.int32).reshape(-1, 2), np.array(case["lens"], np.int32)
        info = capi.TracksInfo(*[-77] * 6)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None
        o = capi.track_opts()
        assert L.psx_tracks_graph_dev(0, 0x1000, ptr(ec), ptr(ea), len(ea), ptr(la), len(la), C.byref(o), 0x2000, 0x3000, 2, 0x4000, 3, C.byref(info)) == 0
        assert bytes(info) == zero
    got = capi.tracks_graph_ref([], [], [5, 3])
    assert got["tracks"] == 0 and got["starts"].tolist() == [0] and len(got["member_records"]) == 0 and got["labels"].tolist() == [-1] * 8


@pytest.mark.parametrize("name,option", [("scattered", (2, False)), ("block_edges", (2, True)), ("hand", (2, True))])
def test_capacity_rule(capi, name, option):
    """the exact capacity, one short of each -- the member cut falls inside the last track --, a cut in the middle, 0 with
    buffers, and 0 with NULL ("how many?"): the totals are always reported, the prefix is the full result's, nothing at or
    past a capacity is touched"""
    case = tc.CASES[name]()
    full = tc.restate(case["lists"], case["edges"], case["lens"], *option)
    T, N = full["tracks"], full["members"]
    assert T >= 2 and full["starts"][-1] - full["starts"][-2] >= 2
    L = capi.lib()
    for tcap, mcap, with_labels in ((T, N, True), (T, N - 1, True), (T - 1, N, False), (T // 2, N // 2 + 1, True), (0, 0, True), (None, None, False),
                                    (None, None, True), (T + 3, N + 3, True)):
        rc, info, labels, starts, members = tc.raw_call(capi, L.psx_tracks_graph_ref, case, capi.track_opts(*option), tcap, mcap, with_labels)
        t = capi.TracksInfo.from_buffer_copy(info)
        assert rc == 0 and all(getattr(t, k) == full[k] for k in tc.TOTALS), (tcap, mcap)
        M = sum(case["lens"])
        assert np.array_equal(labels[:M], full["labels"]) if with_labels else np.all(labels == -7)
        assert np.all(labels[M:] == -7)
        if tcap is None:
            assert np.all(starts == -7) and np.all(members == -7)
            continue
        ns, nm = min(T, tcap) + 1, min(N, mcap)
        assert np.array_equal(starts[:ns], full["starts"][:ns]) and np.all(starts[ns:] == -7), (tcap, mcap)
        assert members[:2 * nm].tobytes() == full["member_records"][:nm].tobytes() and np.all(members[2 * nm:] == -7), (tcap, mcap)


def test_plan_matches_figures_computed_by_hand(capi):
    # the hand example: 10 nodes, 8 records in 5 edges -> 5 blocks; 2^3 < 10 <= 2^4
    p = capi.tracks_plan(tc.HAND["lens"], [len(x) for x in tc.HAND["lists"]])
    assert p == dict(nodes=10, records=8, record_blocks=5, sort_bits=4, launches=7,
                     # tables 16 * 5 + 16 * 5 + pad16(4 * 5); nodes 6 * 4 * 10; sort 4 * 4 * 10; totals 4 * (4 * 1 + 2); state 32
                     scratch_bytes=(80 + 80 + 32) + 240 + 160 + 24 + 32)
    # the block edges: 513 -> 3 blocks, 255 -> 1, 0 -> 0, 256 -> 1, 1 -> 1, 257 -> 2, 64 -> 1, 0 -> 0, 64 -> 1; 514 nodes in 3 workgroups
    p = capi.tracks_plan(tc.BLOCK_LENS, tc.BLOCK_COUNTS)
    assert p == dict(nodes=514, records=1410, record_blocks=10, sort_bits=10, launches=7,
                     scratch_bytes=(16 * 9 + 16 * 10 + 32) + 6 * 4 * 514 + 4 * 4 * 514 + 4 * (4 * 3 + 2) + 32)
    # launches do not grow with the sizes
    big = capi.tracks_plan([2048] * 64, [1500] * 496)
    assert big["launches"] == 7 and big["nodes"] == 131072 and big["sort_bits"] == 17 and big["record_blocks"] == 496 * 6
    # nothing to join: nothing planned
    assert capi.tracks_plan([5, 7], [0, 0]) == dict(nodes=12, records=0, record_blocks=0, sort_bits=4, launches=0, scratch_bytes=0)
    assert capi.tracks_plan([], [3])["nodes"] == 0
    L = capi.lib()
    out = capi.TracksPlanInfo()
    la, ec = np.array([5, -1], np.int32), np.array([3], np.int32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.psx_tracks_plan(ptr(la), 2, ptr(ec), 1, C.byref(out)) == -1 and L.psx_tracks_plan(ptr(ec), 1, ptr(la), 2, C.byref(out)) == -1
    assert L.psx_tracks_plan(ptr(ec), 1, ptr(ec), 1, None) == -1 and L.psx_tracks_plan(None, 1, ptr(ec), 1, C.byref(out)) == -1


def test_plan_and_host_reference_under_sanitizers(tmp_path):
    """tests/cpp/tracks_plan_san.cpp: a stand-alone program (its own main) that includes tracks_plan.h alone and runs the plan
    and the host reference on exact-size heap arrays -- compiled with -fsanitize=address,undefined and run directly"""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed"
    exe = str(tmp_path / "tracks_plan_san")
    cmd = [cxx, "-std=c++14", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan",
           os.path.join(ROOT, "tests", "cpp", "tracks_plan_san.cpp"), "-o", exe,
           "-I", os.path.join(ROOT, "popsift_amd", "csrc", "hip"), "-I", os.path.join(ROOT, "include")]
    subprocess.check_call(cmd)
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout


def test_cpp_api_argument_errors_without_a_device(tmp_path):
    """tests/cpp/test_tracks_api.cpp without POPSIFT_TEST_EXPECT_GPU: the argument checks and the empty forms of
    FeaturesDev::buildTracks, all before a device is touched"""
    libdir = os.path.join(ROOT, "popsift_amd", "lib")
    exe = str(tmp_path / "test_tracks_api")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-pthread", os.path.join(ROOT, "tests", "cpp", "test_tracks_api.cpp"), "-o", exe,
                           "-I", os.path.join(ROOT, "popsift_amd", "csrc", "include"), "-I", os.path.join(ROOT, "include"),
                           "-L", libdir, "-lpopsift", "-lpopsift_hip", "-Wl,-rpath," + libdir])
    env = {k: v for k, v in os.environ.items() if k != "POPSIFT_TEST_EXPECT_GPU"}
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120, env=env)
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout
