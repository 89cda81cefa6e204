"""tests/switch_matrix_cases.py against the table of popsift_amd/csrc/hip/psx_tuning.h, without a GPU (the tuning shim of
tests/test_tuning_cpu.py, built with the host compiler): every row of the table is in exactly one of MATRIX,
COVERED_ELSEWHERE and EXEMPT -- a row added to the table without an entry fails here --, a covering test really names its
switch, and every value the matrix sets is taken by the parser and is not the default (a typo must not test the default).
With the oracle's Gauss tables and the launch code's chunking formulas: an entry of a switch that only chooses among chunk
lengths changes some chunk on one of its frames; the matcher's overflow set really overflows a candidate list."""
import os
import re

import pytest

from tests import switch_matrix_cases as sc
from tests.test_tuning_cpu import ROOT, get, rows, shim  # noqa: F401  (shim: the module-scoped fixture)

FAMILIES = ("pyramid", "orient_desc", "orient_desc_export", "match")


def test_every_table_row_is_in_exactly_one_list(shim):  # noqa: F811
    table = sorted(n for n, _, _ in rows(shim))
    assert len(set(table)) == len(table)
    where = {n: [] for n in table}
    for tag, names in (("MATRIX", sc.matrix_names()), ("COVERED_ELSEWHERE", sc.COVERED_ELSEWHERE), ("EXEMPT", sc.EXEMPT)):
        for n in names:
            assert n in where, "%s names %s, which is no row of the table" % (tag, n)
            where[n].append(tag)
    missing = [n for n in table if not where[n]]
    assert not missing, "rows of psx_tuning.h with no matrix, covered or exempt entry: %s" % missing
    twice = {n: w for n, w in where.items() if len(w) > 1}
    assert not twice, "rows in more than one list: %s" % twice


def test_exempt_is_the_agreed_list():
    assert sorted(sc.EXEMPT) == sorted(["PSX_NULL_DEVICE_WORK", "POPSIFT_FLOW_DEBUG", "POPSIFT_BLUR_DBG", "POPSIFT_BLUR_LDS_PAD",
                                        "POPSIFT_CU_PARTITIONS", "POPSIFT_CU_PARTITION_MODE", "POPSIFT_WAIT_SLEEP_US"])
    for n, why in sc.EXEMPT.items():
        assert why.strip().endswith(".") and len(why.split()) >= 6, n


def test_covering_tests_exist_and_name_their_switch():
    for n, node in sc.COVERED_ELSEWHERE.items():
        path, _, func = node.partition("::")
        assert re.fullmatch(r"tests/test_gpu_\w+\.py", path) and func, node
        text = open(os.path.join(ROOT, path)).read()
        assert re.search(r"^def %s\(" % re.escape(func), text, re.M), "%s: no such test" % node
        assert re.search(r"\b%s\b" % n, text), "%s does not name %s" % (path, n)


def test_matrix_is_well_formed():
    ids = [e[0] for e in sc.MATRIX]
    assert len(set(ids)) == len(ids)
    for name, env, family, frames in sc.MATRIX:
        assert family in FAMILIES, name
        assert env, name
        if family == "match":
            assert frames in sc.MATCH_SEQUENCES, name
            assert all(n.startswith("POPSIFT_MATCH_") for n in env), name
        else:
            assert frames and all(f in sc.FRAMES for f in frames), name
            assert not any(n.startswith("POPSIFT_MATCH_") for n in env), name
        assert sc.timeout_of((name, env, family, frames)) in (120, 300)
    # the issue's rows, by what they set
    have = {tuple(sorted(env.items())) for _, env, _, _ in sc.MATRIX}
    for want in (dict(POPSIFT_BATCH_OCTAVES="0"), dict(POPSIFT_BLUR_ONESTEP="1"), dict(POPSIFT_BLUR_STEPS="2"),
                 dict(POPSIFT_BLUR_STEPS="64"), dict(POPSIFT_BLUR_DMA="1"), dict(POPSIFT_BLUR_DMA="2", POPSIFT_BLUR_DMA_STEPS="2"),
                 dict(POPSIFT_BLUR_DMA="2", POPSIFT_BLUR_DMA_STEPS="9"), dict(POPSIFT_INTERP_MINWG="1"),
                 dict(POPSIFT_TILE="1", POPSIFT_TILE_SMALL="0"), dict(POPSIFT_FLOW="1", POPSIFT_FLOW_ORDER="1"),
                 dict(POPSIFT_FLOW="1", POPSIFT_FLOW_ORDER="2"), dict(POPSIFT_FLOW="1", POPSIFT_FLOW_GRID="8"),
                 dict(POPSIFT_ORI_WPB="1"), dict(POPSIFT_DESC_WGS="1"), dict(POPSIFT_DESC_WPB="1", POPSIFT_DESC_WGS="1"),
                 dict(POPSIFT_DESC_WPB="2", POPSIFT_DESC_WGS="1"), dict(POPSIFT_DESC_WPB="4", POPSIFT_DESC_WGS="1"),
                 dict(POPSIFT_ALT_WGS="1"), dict(POPSIFT_ALT_WGS="64"), dict(POPSIFT_DESC_WPB="1"), dict(POPSIFT_DESC_WPB="2"),
                 dict(POPSIFT_DESC_OCC="5"), dict(POPSIFT_MATCH_WGS_PER_CU="1"),
                 dict(POPSIFT_MATCH_WGS_PER_CU="1", POPSIFT_MATCH_ROUNDS="2"), dict(POPSIFT_MATCH_MFMA="0"),
                 dict(POPSIFT_MATCH_STATS="1")):
        assert tuple(sorted(want.items())) in have, want
    export = {tuple(sorted(env.items())) for _, env, family, _ in sc.MATRIX if family == "orient_desc_export"}
    for want in (dict(POPSIFT_DESC_WPB="1"), dict(POPSIFT_DESC_WPB="2"), dict(POPSIFT_DESC_OCC="5"), dict(POPSIFT_DESC_WGS="1")):
        assert tuple(sorted(want.items())) in export, want
    # the slow persistent grid stays on the smallest frames
    for _, env, _, frames in sc.MATRIX:
        if "POPSIFT_FLOW_GRID" in env:
            assert all(sc.FRAMES[f][0] <= 333 and sc.FRAMES[f][1] <= 251 for f in frames)


@pytest.mark.parametrize("entry", sc.MATRIX, ids=[e[0] for e in sc.MATRIX])
def test_matrix_values_are_accepted_and_not_the_default(shim, monkeypatch, entry):  # noqa: F811
    name, env, _, _ = entry
    table = {n: (kind, default) for n, kind, default in rows(shim)}
    for n in table:
        monkeypatch.delenv(n, raising=False)
    defaults = {n: get(shim, n) for n in env}
    for n, v in env.items():
        monkeypatch.setenv(n, v)
    for n, v in env.items():
        value, err = get(shim, n)
        assert err == "", (name, n, err)
        assert value != defaults[n][0], "%s: %s=%s leaves the default %r" % (name, n, v, value)
        if table[n][0] in ("INT", "LL", "DIGIT", "STRICT"):
            assert str(value) == v, "%s: %s=%s was read as %r" % (name, n, v, value)
    # and nothing else moved
    for n, (kind, default) in table.items():
        if n not in env:
            assert str(get(shim, n)[0]) == default, (name, n)


def test_match_plan_reaches_the_paths_the_entries_are_for():
    """On a whole MI355X (256 CUs) the matrix reaches the two paths no default run does: fewer seeding chunks than MF_SEEDCH
    and the uncapped chunk count with a short last chunk.  The default (3 workgroups per CU) reaches neither at these sizes;
    a 32-CU partition does at ordinary sizes."""
    p = sc.match_plan(8448, 4300, 256, 1)
    assert (p["nseed"], p["mchunks"]) == (7, 7) and p["nseed"] < sc.MF_SEEDCH
    p = sc.match_plan(8448, 4300, 256, 1, rounds=2)
    assert (p["mchunks"], p["mlen"], p["last"]) == (15, 288, 268)
    p = sc.match_plan(33024, 4200, 256, 1)
    assert (p["nseed"], p["mchunks"]) == (1, 1)
    assert sc.match_plan(8448, 4300, 256, 3)["nseed"] == sc.MF_SEEDCH
    assert sc.match_plan(3073, 4300, 32, 3)["nseed"] < sc.MF_SEEDCH <= sc.match_plan(3072, 4300, 32, 3)["nseed"]
    assert sc.match_plan(255, 4095, 256, 1)["path"] == "exact scan"
    assert sc.match_plan(700, 4531, 256, 3, mfma=False)["path"] == "exact scan"


def test_match_sets_put_ties_across_every_tile_boundary():
    import numpy as np
    l, r = sc.match_sets("ties", 700, 4531)
    l2, r2 = sc.match_sets("ties", 700, 4531)
    assert np.array_equal(l, l2) and np.array_equal(r, r2)              # the child and the test draw the same sets
    ks = range(1, (4531 - 2) // 32 + 1)
    assert len(ks) > 100
    for k in ks:
        j = (k * 61) % 700
        assert np.array_equal(r[32 * k - 1], l[j]) and np.array_equal(r[32 * k], l[j])
        assert not np.array_equal(r[32 * k + 1], l[j]) and np.abs(r[32 * k + 1] - l[j]).max() < 2e-4
    _, ro = sc.match_sets("overflow", 300, 9000)
    assert (ro[500:8600] == ro[499]).all()


def test_chunking_entries_move_a_chunk_seam_on_their_frames(oracle):
    """POPSIFT_BLUR_STEPS, POPSIFT_BLUR_ONESTEP and POPSIFT_INTERP_MINWG only choose among chunk lengths, and on a small plane
    every value ends at the same two steps: an entry of them must change the rows per chunk of some plane of one of its
    frames (the launch code's formulas, tests/switch_matrix_cases.chunk_rows), or it tests the default.  The other pyramid
    entries select another kernel or schedule outright."""
    checked = []
    for name, env, family, frames in sc.MATRIX:
        if family != "pyramid" or not set(env) <= set(sc.CHUNKING_SWITCHES):
            continue
        changed = {}
        for frame in frames:
            kw = sc.FRAMES[frame][3]
            relative = kw.get("gauss_mode", 0) == 1
            if any(n.startswith("POPSIFT_INTERP_") for n in env) != relative:
                continue                                             # the switch is not read for this frame's mode
            tables = oracle.gauss_tables(oracle.default_config(**kw))
            a, b = sc.chunk_rows(frame, {}, tables), sc.chunk_rows(frame, env, tables)
            assert a.keys() == b.keys() and a
            changed[frame] = sorted(k for k in a if a[k] != b[k])
        print(name, changed)
        assert any(changed.values()), "%s %s changes no chunk on %s" % (name, env, list(frames))
        checked.append(name)
    assert {"blur_onestep1", "blur_steps2", "blur_steps64", "interp_minwg1", "interp_minwg_large"} <= set(checked)
    # what the frames' comments claim
    t = oracle.gauss_tables(oracle.default_config(octaves=4))
    assert all(v == sc.chunk_rows("640x480", {}, t)[k] for k, v in sc.chunk_rows("640x480", {"POPSIFT_BLUR_STEPS": "64"}, t).items())
    t = oracle.gauss_tables(oracle.default_config(octaves=4, gauss_mode=1))
    assert sc.chunk_rows("640x480_relative", {}, t) == sc.chunk_rows("640x480_relative", {"POPSIFT_INTERP_MINWG": "100000"}, t)


def test_level0_of_the_frame_without_upsampling_can_take_the_dma_kernel(oracle):
    """k_blur_dma<R, LEVEL0> runs for level 0 only when no x2 kernel takes it (octave 0 is not the input upsampled x2) and the
    radius is at most 8: the frame the POPSIFT_BLUR_DMA=2 / 3 entries add for it."""
    frame = "tile_257x190_up0"
    kw = sc.FRAMES[frame][3]
    assert kw["upscale_factor"] == 0.0
    t = oracle.gauss_tables(oracle.default_config(**kw))
    assert max(int(t["dd_span"][0]), int(t["inc_span"][0])) - 1 <= 8
    for name, env, _, frames in sc.MATRIX:
        if env.get("POPSIFT_BLUR_DMA") in ("2", "3") and "POPSIFT_BLUR_DMA_STEPS" in env and env["POPSIFT_BLUR_DMA_STEPS"] == "2":
            assert frame in frames, name


def test_overflow_set_overflows_the_candidate_lists(oracle):
    """The repeated right descriptor is the nearest or second nearest of some left descriptor: all of its copies tie there,
    every one of them is a candidate, and they are more than the MF_SEGS x 32 slots of a left descriptor's list."""
    import numpy as np
    for _, kind, l_len, r_len in {c for calls in sc.MATCH_SEQUENCES.values() for c in calls if c[1] == "overflow"}:
        l, r = sc.match_sets(kind, l_len, r_len)
        copies = int((r == r[499]).all(1).sum())
        assert copies == r_len - 900 + 1 and copies > sc.MF_SEGS * 32
        mo, do_ = oracle.match(l, r)
        tied = np.flatnonzero((mo[:, 0] == 499) & (mo[:, 1] == 500) & (do_[:, 0] == do_[:, 1]))
        second = np.flatnonzero((mo[:, 1] == 499) & (mo[:, 0] < 499))
        assert len(tied) + len(second) >= 1, "no left descriptor has the repeated one among its two nearest"
