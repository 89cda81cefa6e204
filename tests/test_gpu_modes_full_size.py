"""Fixed9 / Fixed15 / VLFeat_Relative / VLFeat_Relative_All held to the CPU oracle at full size (tests/full_size_cases.py): 1080p
frames, planes across the 2048 / 4096 / 8192 binades, the Fixed-mode size bound and the pair counts beyond the fused
kernels.  The small-size tests of tests/test_gpu_modes.py never reach the long-march chunking, the pairing rule at 1080p or
the columns where the relative mode's weights vary; test_fused_mode_kernels_equal_per_level_kernels compares HIP with HIP.

The chunking and schedule switches are read once per context (psx_create); every setting runs in a fresh child
(tests/full_size_modes_worker.py) with a clean environment: every POPSIFT_* removed, then the setting's own values.  A
setting runs the cases its switches can change; the defaults run every case and also compare features and descriptors.
Planes are compared through digests (whole plane, every row, every column): a failure names the case, the setting, the
octave and level and the first rows and columns that differ -- a chunk seam is a band of rows, a binade a band of columns.
One oracle run per case serves every setting.  The children run one after another; once one ends abnormally (a fault, an
abort, a time limit) no further child is started."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import full_size_cases as fc
from tests.parity import assert_parity, budget, match_features, sort_iext

pytestmark = pytest.mark.gpu

ALL = ("fixed", "relative", "relative_all")
# (name, switches, families of the cases the switches can change)
SETTINGS = [
    ("defaults", {}, ALL),
    # one chunk per strip: the whole plane in one march | short chunks, no one-step branch
    ("fixed_one_chunk+interp_steps2", dict(POPSIFT_FIXED_WGS="1", POPSIFT_INTERP_STEPS="2", POPSIFT_INTERP_ONESTEP="0"),
     ("fixed", "relative")),
    # the smallest chunks, seams every step | long chunks
    ("fixed_minsteps1+interp_steps64", dict(POPSIFT_FIXED_WGS="100000", POPSIFT_FIXED_MINSTEPS="1", POPSIFT_INTERP_STEPS="64"),
     ("fixed", "relative")),
    # seams every third step | large planes share launches
    ("fixed_minsteps3+interp_pair_rounds", dict(POPSIFT_FIXED_WGS="100000", POPSIFT_FIXED_MINSTEPS="3",
                                                 POPSIFT_INTERP_PAIR_ROUNDS="1000"), ("fixed", "relative")),
    # every weight computed per element
    ("interp_literal", dict(POPSIFT_INTERP_LITERAL="1"), ("relative",)),
    # the diagonal schedule off: one launch per level
    ("interp_no_diagonal", dict(POPSIFT_INTERP_DIAGONAL="0"), ("relative",)),
    # the per-level kernels of pyramid_alt.hip
    ("per_level", dict(POPSIFT_FIXED_FUSED="0", POPSIFT_INTERP_FUSED="0"), ("fixed", "relative")),
]

_ORACLE = {}            # case name -> what the comparison needs of the oracle's run
_STOPPED = []           # a child that ended abnormally: no more GPU work in this module


def _oracle(oracle, case):
    if case.name not in _ORACLE:
        ref = oracle.run(oracle.default_config(**fc.config(case)), fc.image(case))
        s = dict(num_octaves=ref.num_octaves, num_levels=ref.num_levels, dims=[tuple(d) for d in ref.dims],
                 planes={}, iext={}, ext_total=ref.ext_total, features=ref.features(), descriptors=ref.descriptors())
        for o in range(ref.num_octaves):
            for l in range(ref.num_levels):
                s["planes"][o, l] = fc.plane_digests(ref.gauss(o, l))
            s["iext"][o] = sort_iext(ref.iext(o))
        ref.close()
        _ORACLE[case.name] = s
    return _ORACLE[case.name]


def _first(idx, n=6):
    return "%s%s" % (idx[:n].tolist(), " .." if len(idx) > n else "")


def _compare(case, setting, ref, got, features):
    """Every difference of one case under one setting, as messages."""
    where = "%s [%s]" % (case.name, setting)
    no, nl = int(got["num_octaves"]), int(got["num_levels"])
    dims = [tuple(int(v) for v in d) for d in got["dims"]]
    if (no, nl, dims) != (ref["num_octaves"], ref["num_levels"], ref["dims"]):
        return ["%s: %d octaves x %d levels %s, oracle %d x %d %s" % (where, no, nl, dims, ref["num_octaves"], ref["num_levels"],
                                                                     ref["dims"])]
    errs = []
    for o in range(no):
        for l in range(nl):
            sha, rows, cols = ref["planes"][o, l]
            g_rows, g_cols = got["rows_%d_%d" % (o, l)], got["cols_%d_%d" % (o, l)]
            if str(got["sha_%d_%d" % (o, l)]) != sha or not np.array_equal(g_rows, rows) or not np.array_equal(g_cols, cols):
                br, bc = np.flatnonzero(g_rows != rows), np.flatnonzero(g_cols != cols)
                errs.append("%s: Gaussian plane (octave %d, level %d) of %d x %d differs from the oracle in %d rows %s and "
                            "%d columns %s" % (where, o, l, dims[o][0], dims[o][1], len(br), _first(br), len(bc), _first(bc)))
        a = ref["iext"][o]
        b = np.zeros(len(got["iext_lpos_%d" % o]), dtype=[("xpos", "<f4"), ("ypos", "<f4"), ("lpos", "<i4")])
        for f in ("xpos", "ypos", "lpos"):
            b[f] = got["iext_%s_%d" % (f, o)]
        b = sort_iext(b)
        if len(a) != len(b) or any(not np.array_equal(a[f], b[f]) for f in ("xpos", "ypos", "lpos")):
            errs.append("%s: initial extrema of octave %d differ (%d, oracle %d)" % (where, o, len(b), len(a)))
    if features:
        fb, db = got["features"], got["descriptors"]
        if len(fb) != ref["ext_total"]:
            errs.append("%s: %d features, oracle %d" % (where, len(fb), ref["ext_total"]))
        else:
            try:
                assert_parity(match_features(ref["features"], ref["descriptors"], fb, db), what=where, **budget(len(fb)))
            except AssertionError as e:
                errs.append(str(e))
    return errs


def _child_env(switches):
    # the library choice (POPSIFT_HIP_LIB, POPSIFT_HOST_LIB) is not a switch: the child tests the library the parent loaded
    keep = ("POPSIFT_HIP_LIB", "POPSIFT_HOST_LIB")
    env = {k: v for k, v in os.environ.items() if not k.startswith("POPSIFT_") or k in keep}
    env.update(switches)
    return env


@pytest.mark.parametrize("setting,switches,families", SETTINGS, ids=[s[0] for s in SETTINGS])
def test_full_size_modes_match_oracle(oracle, capi, tmp_path, setting, switches, families):
    if _STOPPED:
        pytest.fail("not started: an earlier child of this module ended abnormally (%s)" % _STOPPED[0])
    cases = [c for c in fc.CASES if fc.family(c) in families]
    features = setting == "defaults"
    spec = tmp_path / "spec.json"
    spec.write_text(json.dumps({"cases": [c.name for c in cases], "features": features}))
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "full_size_modes_worker.py")
    try:
        p = subprocess.run([sys.executable, worker, str(spec), str(tmp_path)], capture_output=True, text=True,
                           env=_child_env(switches), timeout=300)
    except subprocess.TimeoutExpired:
        _STOPPED.append("%s: time limit" % setting)
        raise
    if p.returncode != 0:
        _STOPPED.append("%s: exit status %d" % (setting, p.returncode))
    assert p.returncode == 0, "%s: exit status %d\n%s" % (setting, p.returncode, p.stderr[-3000:])
    assert json.loads(p.stdout.strip().splitlines()[-1]) == [c.name for c in cases]
    errs = []
    for c in cases:
        with np.load(str(tmp_path / (c.name + ".npz"))) as got:
            errs += _compare(c, setting, _oracle(oracle, c), got, features)
    print("%s: %d cases compared" % (setting, len(cases)))
    assert not errs, "\n".join(errs)
