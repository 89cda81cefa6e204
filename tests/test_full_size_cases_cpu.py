"""The case list of tests/test_gpu_modes_full_size.py keeps the coverage it was written for.  Only facts of the tables
(oracle.gauss_tables) and of the case sizes are checked here, not the C++ dispatch rules: pair counts per level, the
instantiation that count needs (3 .. 8 pairs: the smallest of 3 .. 8 that holds it), both Fixed shifts with byte and float
input, the Fixed size bound, planes across the relative mode's binades."""
from tests import full_size_cases as fc


def _relative_levels(oracle):
    """(case, level, pairs) of every VLFeat_Relative level."""
    out = []
    for c in fc.CASES:
        if fc.family(c) == "relative":
            out += [(c, l, n) for l, n in enumerate(fc.interp_pairs(c, oracle.gauss_tables))]
    return out


def test_full_size_cases_are_well_formed():
    assert len(fc.CASES) >= 20
    for c in fc.CASES:
        assert set(c.config) <= {"gauss_mode", "levels", "sigma", "scaling_mode", "upscale_factor", "sift_mode"}, c
        if fc.family(c) == "fixed":
            assert fc.num_levels(c) == 6, "%s: the fixed-span modes take levels = 3 only" % c.name
        w, h = c.size
        assert 4 <= w <= 8192 and 4 <= h <= 8192, c


def test_full_size_cases_cover_every_relative_instantiation(oracle):
    levels = _relative_levels(oracle)
    # levels >= 1: the per-level kernel k_blur_interp<NP> / the paired k_blur_interp2<NP>, NP = max(3, pairs) up to 8
    fused = {max(3, n) for c, l, n in levels if l >= 1 and n <= 8}
    missing = sorted(set(range(3, 9)) - fused)
    assert not missing, "no full-size case has a relative level with NP %s on the fused kernel" % missing
    beyond = [(c.name, l, n) for c, l, n in levels if l >= 1 and n > 8]
    assert beyond, "no full-size relative case has a level with more than 8 pairs (the k_alt_interp fallback)"
    # level 0 of a x2 octave 0: k_level0_x2<.., VNP> with VNP 3 (up to 3 pairs) or 4
    vnp = {3 if n <= 3 else 4 for c, l, n in levels if l == 0 and fc.is_x2(c) and n <= 4}
    assert vnp >= {3, 4}, "level 0 of the x2 relative cases reaches VNP %s only" % sorted(vnp)


def test_full_size_cases_cover_the_fixed_shifts_and_bounds():
    fixed = [c for c in fc.CASES if fc.family(c) == "fixed"]
    x2 = [c for c in fixed if fc.is_x2(c)]
    have = {(c.config["gauss_mode"], c.is_float) for c in x2}
    for gm in (fc.FIXED9, fc.FIXED15):
        for is_float in (False, True):
            assert (gm, is_float) in have, "no x2 Fixed case with gauss_mode %d and %s input" % (gm, "float" if is_float else "u8")
    assert any(c.size[0] == 4096 for c in x2), "no x2 Fixed case at w == 4096"
    assert any(c.size[1] == 4096 for c in x2), "no x2 Fixed case at h == 4096"
    assert any(c.size[0] == 4097 for c in x2), "no x2 Fixed case at w == 4097 (just past the fused kernel's bound)"
    assert any(c.size[0] >= 1920 and c.size[1] >= 1080 and not fc.is_x2(c) for c in fixed), "no full-size Fixed case off x2"
    assert any(c.config.get("scaling_mode") == 0 for c in fixed) and any(c.config.get("upscale_factor") == 0.0 for c in fixed)
    assert any(c.config.get("sift_mode") == 1 for c in fixed)


def test_full_size_cases_cross_the_relative_binades():
    rel = [c for c in fc.CASES if fc.family(c) == "relative" and fc.is_x2(c)]
    assert any(2 * c.size[0] > 4096 and 2 * c.size[1] > 2048 for c in rel), \
        "no x2 relative case whose planes exceed 4096 columns and 2048 rows"
    assert any((2 * c.size[0]) % 64 in (1, 2) for c in rel), "no relative case whose last strip has 1-2 columns"
    assert {c.config.get("sift_mode", 0) for c in rel if c.size == (1920, 1080)} >= {1, 2}
    other = [c for c in fc.CASES if fc.family(c) == "relative" and not fc.is_x2(c)]
    assert any(c.config.get("scaling_mode") == 0 for c in other) and any(c.config.get("upscale_factor") == 0.0 for c in other)
    assert {c.is_float for c in fc.CASES if fc.family(c) == "relative_all"} == {False, True}


def test_plane_digests_localise_a_difference():
    import numpy as np
    rng = np.random.default_rng(3)
    a = rng.random((37, 70), dtype=np.float32)
    b = a.copy()
    b[11, 65] = np.nextafter(b[11, 65], np.float32(2.0))
    sa, ra, ca = fc.plane_digests(a)
    sb, rb, cb = fc.plane_digests(b)
    assert sa != sb
    assert np.flatnonzero(ra != rb).tolist() == [11] and np.flatnonzero(ca != cb).tolist() == [65]
    assert fc.plane_digests(a.copy())[0] == sa
