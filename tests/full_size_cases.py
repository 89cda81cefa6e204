"""Full-size cases of the alternative Gauss modes' own kernels (tests/test_gpu_modes_full_size.py), importable without a GPU.

Fixed9 / Fixed15 run k_fixed_octave (pyramid_fixed.hip), VLFeat_Relative k_blur_interp / k_blur_interp2 (pyramid_interp.hip)
and, at level 0 of a x2 octave 0, k_level0_x2<.., VNP> (pyramid.hip); VLFeat_Relative_All every level of octave 0 through
the level-0 kernels.  What decides their chunking, pairing and weight survey is the plane size (and the CU count), so these
cases are 1080p frames and planes that cross the 2048 / 4096 / 8192 column binades and the Fixed-mode size bound.
tests/test_full_size_cases_cpu.py holds the list to the coverage it was written for.

Also the plane digests both sides of the comparison compute: a SHA-1 of the whole plane (equality) and a 64-bit hash per row
and per column (where it differs: a chunk seam is a band of rows, a binade a band of columns)."""
import hashlib
from collections import namedtuple

import numpy as np

Case = namedtuple("Case", "name config size is_float")

FIXED9, FIXED15, RELATIVE, RELATIVE_ALL = 4, 5, 1, 2
BASE = dict(octaves=5)

CASES = [
    # ---- Fixed9 / Fixed15 (levels = 3: the only level count the fixed-span modes take) ----
    Case("fixed9_1080p", dict(gauss_mode=FIXED9), (1920, 1080), False),
    Case("fixed15_1080p", dict(gauss_mode=FIXED15), (1920, 1080), False),
    Case("fixed9_1080p_float", dict(gauss_mode=FIXED9), (1920, 1080), True),
    Case("fixed15_odd_float", dict(gauss_mode=FIXED15), (1171, 653), True),
    # W = 8192: columns past 2048, 4096 and 8192 texels of the upsampled plane, the largest image octave 0 fuses
    Case("fixed9_w4096", dict(gauss_mode=FIXED9), (4096, 200), False),
    # the same bound on the rows
    Case("fixed15_h4096_float", dict(gauss_mode=FIXED15), (200, 4096), True),
    # just past the bound: octave 0 on the per-level literal kernels, octaves >= 1 on the fused one
    Case("fixed9_w4097", dict(gauss_mode=FIXED9), (4097, 200), False),
    Case("fixed9_direct_1080p", dict(gauss_mode=FIXED9, scaling_mode=0), (1920, 1080), False),
    Case("fixed15_up0_1080p", dict(gauss_mode=FIXED15, upscale_factor=0.0), (1920, 1080), False),
    Case("fixed9_opencv_1080p", dict(gauss_mode=FIXED9, sift_mode=1), (1920, 1080), False),
    # ---- VLFeat_Relative ----
    # sampling shift 1.0 (VLFeat) and 0.5 (OpenCV): the two s1 variants of k_level0_x2
    Case("relative_vlfeat_1080p", dict(gauss_mode=RELATIVE, sift_mode=2), (1920, 1080), False),
    Case("relative_opencv_1080p", dict(gauss_mode=RELATIVE, sift_mode=1), (1920, 1080), False),
    # 4200 x 2600 planes: c -+ off changes its binade at the columns 2048 / 4096 and the rows 2048
    Case("relative_float_wide", dict(gauss_mode=RELATIVE), (2100, 1300), True),
    # pairs 4, 3, 4, 4, 5, 6, 7: VNP 4 at level 0, NP 6, the paired kernel at 6 and 7
    Case("relative_levels4_sigma2", dict(gauss_mode=RELATIVE, levels=4, sigma=2.0), (1920, 1080), False),
    # pairs 4, 4, 6, 8, 12: NP 8 on the single-level kernel, k_alt_interp beyond 8 pairs, the per-level loop
    Case("relative_levels2_sigma2", dict(gauss_mode=RELATIVE, levels=2, sigma=2.0), (1920, 1080), False),
    # pairs 3, 4, 5, 7, 10: another level beyond 8 pairs
    Case("relative_levels2", dict(gauss_mode=RELATIVE, levels=2), (1280, 720), False),
    Case("relative_direct_1080p", dict(gauss_mode=RELATIVE, scaling_mode=0), (1920, 1080), False),
    Case("relative_up0_1080p", dict(gauss_mode=RELATIVE, upscale_factor=0.0), (1920, 1080), False),
    # W = 3906 = 61 * 64 + 2: a last strip of two columns
    Case("relative_w1953", dict(gauss_mode=RELATIVE), (1953, 1099), False),
    # ---- VLFeat_Relative_All ----
    Case("relative_all_1080p", dict(gauss_mode=RELATIVE_ALL), (1920, 1080), False),
    Case("relative_all_1080p_float", dict(gauss_mode=RELATIVE_ALL), (1920, 1080), True),
]

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES), "case names must be unique"

SEED = 5


def config(case):
    """The case's configuration keywords (both capi.default_config and the oracle's default_config take them)."""
    return dict(BASE, **case.config)


def image(case):
    from popsift_amd.synth import synth, synth_float
    w, h = case.size
    return synth_float(w, h, SEED) if case.is_float else synth(w, h, SEED)


def family(case):
    """"fixed", "relative" or "relative_all": which environment switches can change the case's path."""
    gm = case.config["gauss_mode"]
    return {FIXED9: "fixed", FIXED15: "fixed", RELATIVE: "relative", RELATIVE_ALL: "relative_all"}[gm]


def is_x2(case):
    """Octave 0 is the input upsampled x2 (the default scaling with upscale_factor 1)."""
    return case.config.get("scaling_mode", 1) != 0 and case.config.get("upscale_factor", 1.0) == 1.0


def num_levels(case):
    return case.config.get("levels", 3) + 3


def interp_pairs(case, gauss_tables):
    """Tap pairs of every level of a relative case, from its interpolated table: (ispan - 1) / 2 (the reference loops over
    offset = 1, 3, .. < ispan).  gauss_tables: oracle.pyoracle.gauss_tables."""
    from oracle import pyoracle as po
    t = gauss_tables(po.default_config(**config(case)))
    return [int(s - 1) // 2 for s in t["inc_ispan"][:num_levels(case)]]


_KEYS = {}


def _keys(n):
    """Fixed odd 64-bit multipliers: any change of a single word changes the row / column hash."""
    if n not in _KEYS:
        k = np.random.default_rng(12345 + n).integers(0, 2 ** 63, size=n, dtype=np.uint64)
        _KEYS[n] = k * np.uint64(2) + np.uint64(1)
    return _KEYS[n]


def plane_digests(plane):
    """(SHA-1 hex of the plane's bytes, uint64 hash of every row, uint64 hash of every column) of a float32 plane."""
    p = np.ascontiguousarray(plane, dtype=np.float32)
    h, w = p.shape
    u = p.view(np.uint32).astype(np.uint64)
    with np.errstate(over="ignore"):
        rows = (u * _keys(w)[None, :]).sum(axis=1, dtype=np.uint64)
        cols = (u * _keys(h)[:, None]).sum(axis=0, dtype=np.uint64)
    return hashlib.sha1(p.tobytes()).hexdigest(), rows, cols
