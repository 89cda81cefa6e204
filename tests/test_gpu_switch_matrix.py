"""Every result-preserving switch of psx_tuning.h that no other GPU test sets, held to the CPU oracle on the device
(tests/switch_matrix_cases.py lists them; tests/test_switch_matrix_cpu.py keeps that list a partition of the table).

A switch chooses a kernel instantiation, a chunking or a launch schedule, and INTEGRATION.md promises the same results for
it: here the kernel it selects runs, on the smallest frame at which its launches differ from the default's, and is compared
    pyramid            : every Gaussian plane bit for bit, the extrema as sets, the features within tests.parity.budget
    orient_desc*       : features and descriptors within the budget AND the sorted (feature record, descriptor) rows bit
                         for bit with those of a child that sets no switch (the histogram bins are integer fixed point: a
                         variant may not change a bit); that child's rows are held to the oracle in the same test
    match              : indices, accept flags and the bits of the distances against the oracle's sequential scan
Every entry runs in a fresh child (tests/switch_matrix_worker.py) with every POPSIFT_* removed from its environment and
then the entry's own switches, under a time limit sized to its frames.  The children run one after another; once one ends
abnormally (a HIP error, a fault, a time limit) no further child is started.  One oracle run per frame and one oracle scan
per descriptor pair serve every entry."""
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from tests import switch_matrix_cases as sc
from tests.parity import assert_descriptor_rows, assert_parity, budget, match_features, sort_iext

pytestmark = pytest.mark.gpu

_HERE = os.path.dirname(os.path.abspath(__file__))
_ORACLE = {}            # frame -> the oracle's Result and what was derived from it
_SCAN = {}              # (kind, l_len, r_len) -> the oracle's (match, dist)
_BASELINE = {}          # (frames, family) -> directory of the no-switch child's output
_STOPPED = []           # a child that ended abnormally: no more GPU work in this module


def _child_env(switches):
    # the library choice (POPSIFT_HIP_LIB, POPSIFT_HOST_LIB) is not a switch: the child tests the library the parent loaded
    keep = ("POPSIFT_HIP_LIB", "POPSIFT_HOST_LIB")
    env = {k: v for k, v in os.environ.items() if not (k.startswith("POPSIFT_") or k.startswith("PSX_")) or k in keep}
    env.update(switches)
    return env


def _run_child(name, switches, spec, out_dir, timeout):
    """One worker process; returns its standard output.  Fails the test -- and stops the module -- when it ends abnormally."""
    if _STOPPED:
        pytest.fail("not started: an earlier child of this module ended abnormally (%s)" % _STOPPED[0])
    os.makedirs(out_dir, exist_ok=True)
    spec_path = os.path.join(out_dir, "spec.json")
    with open(spec_path, "w") as f:
        json.dump(spec, f)
    t0 = time.perf_counter()
    try:
        p = subprocess.run([sys.executable, os.path.join(_HERE, "switch_matrix_worker.py"), spec_path, out_dir],
                           capture_output=True, text=True, env=_child_env(switches), timeout=timeout)
    except subprocess.TimeoutExpired:
        _STOPPED.append("%s: time limit of %d s" % (name, timeout))
        raise
    wall = time.perf_counter() - t0
    print("switch matrix child %s %s: %.1f s\n%s" % (name, switches, wall, p.stdout))
    if p.returncode != 0:
        _STOPPED.append("%s: exit status %d" % (name, p.returncode))
    assert p.returncode == 0, "%s %s: exit status %d\n%s\n%s" % (name, switches, p.returncode, p.stdout[-1500:], p.stderr[-3000:])
    return p.stdout, p.stderr


def _oracle(oracle, frame):
    if frame not in _ORACLE:
        kw = sc.FRAMES[frame][3]
        ref = oracle.run(oracle.default_config(**kw), sc.image(frame))
        _ORACLE[frame] = dict(ref=ref, planes={}, features=ref.features(), descriptors=ref.descriptors(),
                              iext=[sort_iext(ref.iext(o)) for o in range(ref.num_octaves)])
    return _ORACLE[frame]


def _oracle_plane(s, o, l):
    from tests import full_size_cases as fc
    if (o, l) not in s["planes"]:
        s["planes"][o, l] = fc.plane_digests(s["ref"].gauss(o, l))
    return s["planes"][o, l]


def _first(idx, n=6):
    return "%s%s" % (idx[:n].tolist(), " .." if len(idx) > n else "")


def _compare_geometry(where, s, got):
    ref = s["ref"]
    no, nl = int(got["num_octaves"]), int(got["num_levels"])
    dims = [tuple(int(v) for v in d) for d in got["dims"]]
    assert (no, nl, dims) == (ref.num_octaves, ref.num_levels, [tuple(d) for d in ref.dims]), where


def _compare_planes(where, s, got):
    errs = []
    for o in range(s["ref"].num_octaves):
        for l in range(s["ref"].num_levels):
            sha, rows, cols = _oracle_plane(s, o, l)
            g_rows, g_cols = got["rows_%d_%d" % (o, l)], got["cols_%d_%d" % (o, l)]
            if str(got["sha_%d_%d" % (o, l)]) != sha or not np.array_equal(g_rows, rows) or not np.array_equal(g_cols, cols):
                br, bc = np.flatnonzero(g_rows != rows), np.flatnonzero(g_cols != cols)
                errs.append("%s: Gaussian plane (octave %d, level %d) differs from the oracle in %d rows %s and %d columns %s"
                            % (where, o, l, len(br), _first(br), len(bc), _first(bc)))
    return errs


def _compare_extrema(where, s, got):
    errs = []
    for o in range(s["ref"].num_octaves):
        a = s["iext"][o]
        b = np.zeros(len(got["iext_lpos_%d" % o]), dtype=[("xpos", "<f4"), ("ypos", "<f4"), ("lpos", "<i4")])
        for f in ("xpos", "ypos", "lpos"):
            b[f] = got["iext_%s_%d" % (f, o)]
        b = sort_iext(b)
        if len(a) != len(b) or any(not np.array_equal(a[f], b[f]) for f in ("xpos", "ypos", "lpos")):
            errs.append("%s: initial extrema of octave %d differ (%d, oracle %d)" % (where, o, len(b), len(a)))
    return errs


def _compare_features(where, s, got, grid=False):
    """Features and descriptors against the oracle within tests.parity.budget.  grid (desc_mode Grid): the sample points are
    snapped to pixels, decided by the last bits of sin / cos of the orientation, so end to end a share of the descriptors is
    knife-edge (tests/test_gpu_modes.py::test_grid_descriptor_mode); keypoints and orientations are held end to end, the
    descriptors at stage level -- the oracle redoes them for the device's own oriented extrema -- with the same budget, and end
    to end with that test's bound."""
    fb, db = got["features"], got["descriptors"]
    ref = s["ref"]
    if len(fb) != ref.ext_total:
        return ["%s: %d features, oracle %d" % (where, len(fb), ref.ext_total)]
    if abs(len(db) - ref.ori_total) > budget(len(fb))["ori"]:
        return ["%s: %d descriptors, oracle %d" % (where, len(db), ref.ori_total)]
    try:
        m = match_features(s["features"], s["descriptors"], fb, db)
        if grid:
            assert_parity(m, what=where, **dict(budget(len(fb)), desc=m["desc_compared"]))
            # end to end the bound of test_grid_descriptor_mode: a small share of knife-edge descriptors, none far off
            assert m["desc_miss"] <= 0.06 * m["desc_compared"] and m["max_desc_dist"] < 0.05, \
                "%s: %d of %d descriptors beyond 1e-3 end to end, max %.3g" % (where, m["desc_miss"], m["desc_compared"], m["max_desc_dist"])
            ext = got["extrema"]
            assert len(ext) == len(fb), "%s: %d oriented extrema, %d features" % (where, len(ext), len(fb))
            assert_descriptor_rows(ref.describe(ext, len(db)), db, len(fb), what=where + " descriptor stage")
        else:
            assert_parity(m, what=where, **budget(len(fb)))
    except AssertionError as e:
        return [str(e)]
    return []


def _is_grid(frame):
    return sc.FRAMES[frame][3].get("desc_mode", 0) == 2


def _row_digest(f, d):
    """(number of descriptors, SHA-1 over the (xpos, ypos, sigma, orientation, 128 values) rows sorted by the record), as
    tests/desc_walk_worker.py hashes them: the order of the extrema list is not deterministic, its content is."""
    f, d = np.asarray(f), np.asarray(d, np.float32).reshape(-1, 128)
    k = np.arange(f["orientation"].shape[1])[None, :]
    di = f["desc_idx"].astype(np.int64)
    sel = (k < f["num_ori"][:, None]) & (di >= 0)
    assert (di[sel] < len(d)).all(), "a feature record points past the descriptor array"
    i, kk = np.nonzero(sel)
    rows = np.concatenate([np.stack([f["xpos"][i], f["ypos"][i], f["sigma"][i], f["orientation"][i, kk]], 1).astype(np.float32),
                           d[di[i, kk]]], axis=1).astype(np.float32).reshape(-1, 132)
    order = np.lexsort(rows.T[::-1])
    return len(rows), hashlib.sha1(np.ascontiguousarray(rows[order]).tobytes()).hexdigest(), rows[order]


def _check_yield(frame, n_kp, n_desc, what):
    assert n_desc >= sc.MIN_DESCRIPTORS.get(frame, 0), "%s: %s has %d descriptors, the wave loop does not wrap" % (what, frame, n_desc)
    assert n_kp >= sc.MIN_KEYPOINTS.get(frame, 0), "%s: %s has %d keypoints, the wave loop does not wrap" % (what, frame, n_kp)


def _baseline(oracle, tmp_path_factory, frames, family):
    """The child that sets no switch, once per (frames, family); every frame of it held to the oracle."""
    key = (frames, family)
    if key not in _BASELINE:
        out = str(tmp_path_factory.mktemp("switch_matrix_baseline"))
        limit = sc.timeout_of(("baseline", {}, family, frames))
        _run_child("no switch [%s]" % family, {}, {"family": family, "frames": list(frames)}, out, limit)
        errs = []
        for frame in frames:
            with np.load(os.path.join(out, frame + ".npz")) as got:
                errs += _compare_features("%s [no switch, %s]" % (frame, family), _oracle(oracle, frame), got, _is_grid(frame))
        assert not errs, "\n".join(errs)
        _BASELINE[key] = out
    return _BASELINE[key]


_FRAME_ENTRIES = [e for e in sc.MATRIX if e[2] != "match"]
_MATCH_ENTRIES = [e for e in sc.MATRIX if e[2] == "match"]


@pytest.mark.parametrize("entry", _FRAME_ENTRIES, ids=[e[0] for e in _FRAME_ENTRIES])
def test_switch_keeps_results(oracle, capi, tmp_path, tmp_path_factory, entry):
    name, switches, family, frames = entry
    base = _baseline(oracle, tmp_path_factory, frames, family) if family != "pyramid" else None
    _run_child(name, switches, {"family": family, "frames": list(frames)}, str(tmp_path), sc.timeout_of(entry))
    errs = []
    for frame in frames:
        where = "%s [%s]" % (frame, name)
        s = _oracle(oracle, frame)
        _check_yield(frame, s["ref"].ext_total, s["ref"].ori_total, "oracle")
        with np.load(str(tmp_path / (frame + ".npz"))) as got:
            _compare_geometry(where, s, got)
            _check_yield(frame, len(got["features"]), len(got["descriptors"]), "device")
            if family == "pyramid":
                errs += _compare_planes(where, s, got)
                errs += _compare_extrema(where, s, got)
                errs += _compare_features(where, s, got, _is_grid(frame))
                continue
            errs += _compare_features(where, s, got, _is_grid(frame))
            n, sha, rows = _row_digest(got["features"], got["descriptors"])
        with np.load(os.path.join(base, frame + ".npz")) as plain:
            n0, sha0, rows0 = _row_digest(plain["features"], plain["descriptors"])
        print("%s: %d rows %s, no switch: %d rows %s" % (where, n, sha, n0, sha0))
        if (n, sha) != (n0, sha0):
            bad = np.flatnonzero((rows.view(np.uint32) != rows0.view(np.uint32)).any(1)) if n == n0 else np.zeros(0, np.int64)
            errs.append("%s: the sorted (record, descriptor) rows differ from the run with no switch: %d rows against %d, "
                        "%d rows with other bits %s" % (where, n, n0, len(bad), _first(bad)))
    assert not errs, "\n".join(errs)


@pytest.mark.parametrize("entry", _MATCH_ENTRIES, ids=[e[0] for e in _MATCH_ENTRIES])
def test_match_switch_keeps_results(oracle, capi, tmp_path, entry):
    name, switches, _, sequence = entry
    _, stderr = _run_child(name, switches, {"family": "match", "sequence": sequence}, str(tmp_path), sc.timeout_of(entry))
    calls = sc.MATCH_SEQUENCES[sequence]
    if "POPSIFT_MATCH_STATS" in switches:
        # one line per call that took the prefilter; it says when the call then went through the exact scan of every pair
        said = [ln for ln in stderr.splitlines() if ln.startswith("psx_match prefilter:")]
        print("\n".join(said))
        assert len(said) == len(calls), stderr[-2000:]
        for ln, (label, kind, l_len, r_len) in zip(said, calls):
            assert ("%d x %d" % (l_len, r_len)) in ln, ln
            assert ln.endswith("-> exact scan of every pair") == (kind == "overflow"), "%s: %s" % (label, ln)
        if len({c[1:] for c in calls}) == 1:
            assert len({ln.split(":", 1)[1] for ln in said}) == 1, "a repeated call counted other candidates: stale counters"
    errs = []
    with np.load(str(tmp_path / "match.npz")) as got:
        for i, (label, kind, l_len, r_len) in enumerate(calls):
            if (kind, l_len, r_len) not in _SCAN:
                _SCAN[kind, l_len, r_len] = oracle.match(*sc.match_sets(kind, l_len, r_len))
            mo, do_ = _SCAN[kind, l_len, r_len]
            mg, dg = got["match_%d" % i], got["dist_%d" % i]
            where = "%s, call %d (%s, %d x %d)" % (name, i, label, l_len, r_len)
            bad = np.flatnonzero((mo != mg).any(1))
            if len(bad):
                j = bad[0]
                errs.append("%s: (best, second, accept) differ for %d left descriptors %s; first: %s, oracle %s, distances %s, "
                            "oracle %s" % (where, len(bad), _first(bad), mg[j].tolist(), mo[j].tolist(), dg[j].tolist(), do_[j].tolist()))
            bad = np.flatnonzero((do_.view(np.uint32) != dg.view(np.uint32)).any(1))
            if len(bad):
                errs.append("%s: the distances of %d left descriptors %s have other bits" % (where, len(bad), _first(bad)))
            if kind == "ties":
                # the sets are what they are meant to be: a left descriptor with copies at 32k - 1 and 32k keeps the earlier one
                k = np.arange(1, (r_len - 2) // 32 + 1)
                j = (k * 61) % l_len
                last = {int(jj): int(kk) for jj, kk in zip(j[::-1], k[::-1])}          # the first k of every left index
                for jj, kk in last.items():
                    assert mo[jj, 0] == 32 * kk - 1 and do_[jj, 0] == 0.0, (where, jj, kk, mo[jj].tolist())
    assert not errs, "\n".join(errs)
