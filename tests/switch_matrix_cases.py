"""The result-preserving switches of popsift_amd/csrc/hip/psx_tuning.h and where the suite holds each of them to the oracle,
importable without a GPU.  tests/test_switch_matrix_cpu.py keeps the three lists below a partition of the table;
tests/test_gpu_switch_matrix.py runs every MATRIX entry in a fresh child (tests/switch_matrix_worker.py).

MATRIX             (id, env, family, frames): the switches of one child process and what is compared
                   family "pyramid"          : every Gaussian plane bit-equal to the oracle, equal extrema, features in budget
                   family "orient_desc"      : features and descriptors in budget against the oracle AND the sorted
                                               (feature record, descriptor) rows bit-identical to a run with no switch set
                   family "orient_desc_export": the same on the buffers of the zero-copy export
                   family "match"            : frames = one name of MATCH_SEQUENCES; indices, accept flags and the bits of
                                               the distances equal to the oracle's sequential scan
COVERED_ELSEWHERE  name -> node id of the GPU test that already sets it (not repeated here)
EXEMPT             name -> why no result can be compared (the row says the results are wrong or stale, or it touches no
                   device code)

The frames are the smallest at which the variant's launches differ from the default's (the launch code decides by plane
size and CU count; the numbers in the comments are for 256 CUs)."""
import numpy as np

# ---- frames: name -> (width, height, seed, configuration keywords of capi.default_config / the oracle's) -------------------
FRAMES = {
    # every octave pair shares its launches: POPSIFT_BATCH_OCTAVES=0 changes every launch
    "300x200": (300, 200, 9, dict(octaves=-1)),
    # octave 0 stays at two-step chunks (20 strips x 18 chunks = 360 workgroups >= 256), octaves >= 1 fall to two steps with
    # fewer than 256 workgroups: POPSIFT_BLUR_ONESTEP=1 cuts their levels of radius bucket <= 10 into one-step chunks of
    # 22 / 18 / 16 / 12 rows and leaves the level of bucket 13.  2 694 descriptors (oracle): 1 024 descriptor waves wrap
    "640x480": (640, 480, 9, dict(octaves=4)),
    "333x251": (333, 251, 5, dict(octaves=3, sift_mode=1)),
    # 4 183 descriptors (oracle): with the zero-copy export attached POPSIFT_DESC_OCC=5 launches 3 workgroups of four waves per
    # CU, 3 072 waves, the largest grid of the export entries -- they wrap too
    "800x600": (800, 600, 9, dict(octaves=4)),
    # planes of 3840 x 2160: five-step chunks by default, so POPSIFT_BLUR_STEPS moves the chunk seams (on the smaller frames
    # every plane is at two steps whatever the switch says); 15 228 keypoints (oracle): k_orientation<1>'s 8 192 waves wrap
    "1080p": (1920, 1080, 9, dict(octaves=5)),
    # GaussMode VLFeat_Relative: the fused interpolated kernels, whose chunking POPSIFT_INTERP_MINWG decides
    # every plane of it is at two-step (or one-step) chunks by default: POPSIFT_INTERP_MINWG=1 lengthens them
    "640x480_relative": (640, 480, 9, dict(octaves=4, gauss_mode=1)),
    # planes of 3840 x 2160 and 1920 x 1080 take five- and three-step chunks by default: a large POPSIFT_INTERP_MINWG shortens
    # them to two steps (on the 640 x 480 frame it would change nothing)
    "1080p_relative": (1920, 1080, 9, dict(octaves=5, gauss_mode=1)),
    # the frames of test_gpu_parity.py::test_tile_kernel_bit_exact of at most 640 x 480
    "tile_640x480_opencv": (640, 480, 1001, dict(octaves=5, sift_mode=1, gauss_mode=3)),
    "tile_333x251": (333, 251, 7, dict(octaves=4)),
    "tile_257x190_up0": (257, 190, 3, dict(octaves=3, upscale_factor=0.0)),
    "tile_65x65": (65, 65, 9, dict(octaves=3)),
    "tile_200x150_up2": (200, 150, 21, dict(octaves=4, upscale_factor=2.0)),
    "tile_320x240_levels2": (320, 240, 11, dict(octaves=3, levels=2)),
    "tile_320x240_levels4": (320, 240, 12, dict(octaves=3, levels=4)),
    "tile_31x17": (31, 17, 13, dict(octaves=2)),
    # k_descriptors_alt, desc_mode ILoop / Grid / IGrid / NoTile
    "640x480_iloop": (640, 480, 9, dict(octaves=4, desc_mode=1)),
    "640x480_grid": (640, 480, 9, dict(octaves=4, desc_mode=2)),
    "640x480_igrid": (640, 480, 9, dict(octaves=4, desc_mode=3)),
    "640x480_notile": (640, 480, 9, dict(octaves=4, desc_mode=4)),
}

SMALL = ("300x200", "640x480", "333x251")
TILE_FRAMES = ("tile_640x480_opencv", "tile_333x251", "tile_257x190_up0", "tile_65x65", "tile_200x150_up2",
               "tile_320x240_levels2", "tile_320x240_levels4", "tile_31x17")
ALT_FRAMES = ("640x480_iloop", "640x480_grid", "640x480_igrid", "640x480_notile")

# frames whose child gets the long time limit
LARGE_FRAMES = ("1080p", "1080p_relative")
TIMEOUT_SMALL, TIMEOUT_LARGE = 120, 300

# what a frame must yield for its entries to mean anything (asserted on the oracle's counts and on the device's)
MIN_DESCRIPTORS = {"640x480": 1025, "800x600": 3073, "640x480_iloop": 257, "640x480_grid": 257, "640x480_igrid": 257, "640x480_notile": 257}
MIN_KEYPOINTS = {"1080p": 8193}


def _e(**kw):
    return {"POPSIFT_" + k: str(v) for k, v in kw.items()}


MATRIX = [
    # ---- pyramid ----
    ("batch_octaves0", _e(BATCH_OCTAVES=0), "pyramid", SMALL),
    ("blur_onestep1", _e(BLUR_ONESTEP=1), "pyramid", SMALL),
    ("blur_steps2", _e(BLUR_STEPS=2), "pyramid", ("1080p",)),
    ("blur_steps64", _e(BLUR_STEPS=64), "pyramid", ("1080p",)),
    ("blur_dma1", _e(BLUR_DMA=1), "pyramid", SMALL),
    # the frame without upsampling: its level 0 is no x2 kernel's, it runs k_upscale + k_blur_dma<R, LEVEL0> under 2 and 3
    ("blur_dma2_steps2", _e(BLUR_DMA=2, BLUR_DMA_STEPS=2), "pyramid", SMALL + ("tile_257x190_up0",)),
    ("blur_dma2_steps9", _e(BLUR_DMA=2, BLUR_DMA_STEPS=9), "pyramid", SMALL),
    # the paired launches of the diagonal schedule never take k_blur_dma: without them every level does
    ("blur_dma1_unbatched", _e(BLUR_DMA=1, BATCH_OCTAVES=0), "pyramid", SMALL),
    ("blur_dma3_steps2_unbatched", _e(BLUR_DMA=3, BLUR_DMA_STEPS=2, BATCH_OCTAVES=0), "pyramid", SMALL + ("tile_257x190_up0",)),
    ("interp_minwg1", _e(INTERP_MINWG=1), "pyramid", ("640x480_relative",)),
    ("interp_minwg_large", _e(INTERP_MINWG=100000), "pyramid", ("1080p_relative",)),
    ("tile1_small0", _e(TILE=1, TILE_SMALL=0), "pyramid", TILE_FRAMES),
    ("flow1_order1", _e(FLOW=1, FLOW_ORDER=1), "pyramid", SMALL),
    ("flow1_order2", _e(FLOW=1, FLOW_ORDER=2), "pyramid", SMALL),
    # 8 persistent workgroups are slow on purpose: the two smallest frames only
    ("flow1_grid8", _e(FLOW=1, FLOW_GRID=8), "pyramid", ("300x200", "333x251")),
    # ---- orientation, descriptors ----
    ("ori_wpb1", _e(ORI_WPB=1), "orient_desc", ("1080p",)),
    ("desc_wgs1", _e(DESC_WGS=1), "orient_desc", ("640x480",)),
    ("desc_wgs64", _e(DESC_WGS=64), "orient_desc", ("640x480",)),
    ("desc_wpb1_wgs1", _e(DESC_WPB=1, DESC_WGS=1), "orient_desc", ("640x480",)),
    ("desc_wpb2_wgs1", _e(DESC_WPB=2, DESC_WGS=1), "orient_desc", ("640x480",)),
    ("desc_wpb4_wgs1", _e(DESC_WPB=4, DESC_WGS=1), "orient_desc", ("640x480",)),
    ("alt_wgs1", _e(ALT_WGS=1), "orient_desc", ALT_FRAMES),
    ("alt_wgs64", _e(ALT_WGS=64), "orient_desc", ALT_FRAMES),
    # ---- the same with the zero-copy export attached: another grid and another default instantiation ----
    ("export_desc_wpb1", _e(DESC_WPB=1), "orient_desc_export", ("800x600",)),
    ("export_desc_wpb2", _e(DESC_WPB=2), "orient_desc_export", ("800x600",)),
    ("export_desc_occ5", _e(DESC_OCC=5), "orient_desc_export", ("800x600",)),
    ("export_desc_wgs1", _e(DESC_WGS=1), "orient_desc_export", ("800x600",)),
    # ---- psx_match ----
    ("match_wgs1", _e(MATCH_WGS_PER_CU=1), "match", "wgs1_sequence"),
    ("match_wgs1_rounds2", _e(MATCH_WGS_PER_CU=1, MATCH_ROUNDS=2), "match", "chunked_twice"),
    ("match_wgs1_long_left", _e(MATCH_WGS_PER_CU=1), "match", "long_left"),
    ("match_mfma0", _e(MATCH_MFMA=0), "match", "prefilter_size"),
    ("match_stats1", _e(MATCH_STATS=1), "match", "prefilter_size_twice"),
    # the statistics line says how a call ended: the overflow set has to end in the exact scan of every pair
    ("match_stats1_overflow", _e(MATCH_STATS=1, MATCH_WGS_PER_CU=1), "match", "overflow_then_ordinary"),
]

COVERED_ELSEWHERE = {
    "POPSIFT_HIP_GRAPH": "tests/test_gpu_parity.py::test_hipgraph_replay_matches_stream_launches",
    "POPSIFT_TILE_TY": "tests/test_gpu_parity.py::test_tile_kernel_bit_exact",
    "POPSIFT_TILE_NT": "tests/test_gpu_parity.py::test_tile_kernel_bit_exact",
    "POPSIFT_TILE_MAXPX": "tests/test_gpu_parity.py::test_tile_kernel_bit_exact",
    "POPSIFT_FLOW_LD": "tests/test_gpu_parity.py::test_pyramid_flow_kernel_bit_exact",
    "POPSIFT_FLOW_STEPS": "tests/test_gpu_parity.py::test_pyramid_flow_kernel_bit_exact",
    "POPSIFT_BLUR_DEFER": "tests/test_gpu_api.py::test_documented_fallback_switches_keep_parity",
    "POPSIFT_LEVEL0_FUSED": "tests/test_gpu_api.py::test_documented_fallback_switches_keep_parity",
    "POPSIFT_LEVEL0_X2": "tests/test_gpu_api.py::test_documented_fallback_switches_keep_parity",
    "POPSIFT_DESC_DENORM": "tests/test_gpu_api.py::test_documented_fallback_switches_keep_parity",
    "POPSIFT_INTERP_FUSED": "tests/test_gpu_modes_full_size.py::test_full_size_modes_match_oracle",
    "POPSIFT_INTERP_LITERAL": "tests/test_gpu_modes_full_size.py::test_full_size_modes_match_oracle",
    "POPSIFT_INTERP_STEPS": "tests/test_gpu_modes_full_size.py::test_full_size_modes_match_oracle",
    "POPSIFT_INTERP_ONESTEP": "tests/test_gpu_modes_full_size.py::test_full_size_modes_match_oracle",
    "POPSIFT_INTERP_PAIR_ROUNDS": "tests/test_gpu_modes_full_size.py::test_full_size_modes_match_oracle",
    "POPSIFT_INTERP_DIAGONAL": "tests/test_gpu_modes_full_size.py::test_full_size_modes_match_oracle",
    "POPSIFT_FIXED_FUSED": "tests/test_gpu_modes_full_size.py::test_full_size_modes_match_oracle",
    "POPSIFT_FIXED_WGS": "tests/test_gpu_modes_full_size.py::test_full_size_modes_match_oracle",
    "POPSIFT_FIXED_MINSTEPS": "tests/test_gpu_modes_full_size.py::test_full_size_modes_match_oracle",
    "POPSIFT_ALT_WINDOW": "tests/test_gpu_modes.py::test_alt_descriptor_window_equals_plane",
}

EXEMPT = {
    "PSX_NULL_DEVICE_WORK": "Measurement: the kernels (and DMAs) after a context's first frame are left out, the results are stale.",
    "POPSIFT_FLOW_DEBUG": "Measurement: the row itself says the results are wrong (no dependency waits, no arithmetic).",
    "POPSIFT_BLUR_DBG": "Read by the phase-timing builds only, where k_blur stops after the named phase: no complete plane.",
    "POPSIFT_BLUR_LDS_PAD": "Measurement: extra dynamic LDS per workgroup changes residency only, no kernel reads the value.",
    "POPSIFT_CU_PARTITIONS": "Measurement: CU masks of the contexts' streams decide where kernels run, not what they compute.",
    "POPSIFT_CU_PARTITION_MODE": "The shape of those CU masks: without effect unless POPSIFT_CU_PARTITIONS is set.",
    "POPSIFT_WAIT_SLEEP_US": "Host only: how long the blocking wait sleeps between two event queries.",
}


def matrix_names():
    """Every environment name a MATRIX entry sets."""
    return sorted({n for _, env, _, _ in MATRIX for n in env})


def timeout_of(entry):
    _, _, family, frames = entry
    if family == "match":
        return TIMEOUT_SMALL
    return TIMEOUT_LARGE if any(f in LARGE_FRAMES for f in frames) else TIMEOUT_SMALL


def image(frame):
    from popsift_amd.synth import synth
    w, h, seed, _ = FRAMES[frame]
    return synth(w, h, seed)


# ---- the chunking of the marching kernels, as the launch code derives it ------------------------------------------------------
TW, BR = 64, 32                                      # pyramid.hip, pyramid_interp.hip: strip width, rows per marching step
BLUR_RADII = (5, 7, 8, 10, 13, 16, 22, 30)           # the radii k_blur is instantiated for (psx_launch_blur)
# the switches that only move chunk seams, with their defaults: whether an entry of these changes anything depends on the frame
CHUNKING_SWITCHES = {"POPSIFT_BLUR_STEPS": 5, "POPSIFT_BLUR_ONESTEP": 0, "POPSIFT_INTERP_MINWG": 384}


def _wgs(W, H, cr):
    return ((W + TW - 1) // TW) * ((H + cr - 1) // cr)


def blur_chunk_rows(W, H, span, steps=5, onestep=False):
    """Rows per chunk of a k_blur / k_blur2 launch: chunking() of pyramid.hip.  span: one-sided taps including the centre."""
    R = next(r for r in BLUR_RADII if span - 1 <= r)
    S = steps
    if S == 5 and _wgs(W, H, 7 * BR - 2 * R) >= 4096:
        S = 7
    while S > 2:
        cr = S * BR - 2 * R
        if cr >= BR and _wgs(W, H, cr) >= 384:
            break
        S -= 1
    if onestep and S == 2 and BR - 2 * R >= 12 and _wgs(W, H, 2 * BR - 2 * R) < 256:
        S = 1
    cr = S * BR - 2 * R
    if cr < BR // 2 and S > 1:
        cr = BR // 2
    return min(cr, H)


def interp_chunk_rows(W, H, ispan, steps=5, minwg=384, onestep=True):
    """Rows per chunk of a k_blur_interp launch: interp_chunking() of pyramid_interp.hip.  ispan: the level's interpolated span."""
    pairs = (ispan - 1) // 2
    RI = 2 * max(3, pairs)
    S = steps
    while S > 2:
        cr = S * BR - 2 * RI
        if cr >= BR and _wgs(W, H, cr) >= minwg:
            break
        S -= 1
    if onestep and S == 2 and BR - 2 * RI >= 12 and _wgs(W, H, 2 * BR - 2 * RI) < 256:
        S = 1
    return min(max(S * BR - 2 * RI, 4), H)


def chunk_rows(frame, env, tables):
    """{(octave, level): rows per chunk} of the frame's plane-to-plane blurs under the switches env.  tables: the Gauss tables
    of the frame's configuration (oracle.pyoracle.gauss_tables).  For frames upsampled x2 (the default); octaves = -1 counts as
    four.  VLFeat_Relative levels beyond 8 tap pairs run the per-level kernels, which have no chunks, and are left out."""
    w, h, _, kw = FRAMES[frame]
    assert kw.get("upscale_factor", 1.0) == 1.0 and kw.get("scaling_mode", 1) == 1, frame
    steps = int(env.get("POPSIFT_BLUR_STEPS", 5))
    onestep = env.get("POPSIFT_BLUR_ONESTEP", "0").startswith("1")
    minwg = int(env.get("POPSIFT_INTERP_MINWG", 384))
    relative = kw.get("gauss_mode", 0) == 1
    out = {}
    W, H = 2 * w, 2 * h
    for o in range(kw["octaves"] if kw["octaves"] > 0 else 4):
        for l in range(1, kw.get("levels", 3) + 3):
            if relative:
                if (int(tables["inc_ispan"][l]) - 1) // 2 <= 8:
                    out[o, l] = interp_chunk_rows(W, H, int(tables["inc_ispan"][l]), 5, minwg)
            else:
                out[o, l] = blur_chunk_rows(W, H, int(tables["inc_span"][l]), steps, onestep)
        W, H = (W + 1) // 2, (H + 1) // 2
    return out


# ---- the matcher -----------------------------------------------------------------------------------------------------------
MF_TILE, MF_SEGS, MF_SEED, MF_SEEDCH = 32, 32, 2048, 8          # match.hip


def match_plan(l_len, r_len, cus, wgs_per_cu, rounds=1, mfma=True):
    """What match_f32_run derives from the sizes and `resident = workgroups per CU x CUs`: dict(path, nseed, seedlen, mchunks,
    mlen, last) -- path "prefilter" or "exact scan" (below 256 x 4096, or POPSIFT_MATCH_MFMA=0); last = the length of the
    last chunk.  wgs_per_cu: POPSIFT_MATCH_WGS_PER_CU, or the runtime's occupancy answer (3 on gfx950) when it is unset."""
    if not mfma or r_len < 2 * MF_SEED or l_len < 256:
        return dict(path="exact scan")
    resident = wgs_per_cu * cus
    lblocks = (l_len + 255) // 256
    nseed = max(1, min(MF_SEEDCH, resident // lblocks))
    seedlen = (((MF_SEED + nseed - 1) // nseed + MF_TILE - 1) // MF_TILE) * MF_TILE
    mchunks = (rounds * resident) // lblocks
    mchunks = max(1, min(mchunks, (r_len + 8 * MF_TILE - 1) // (8 * MF_TILE), MF_SEGS // 2))
    mlen = (((r_len + mchunks - 1) // mchunks + MF_TILE - 1) // MF_TILE) * MF_TILE
    mchunks = (r_len + mlen - 1) // mlen
    return dict(path="prefilter", nseed=nseed, seedlen=seedlen, mchunks=mchunks, mlen=mlen, last=r_len - (mchunks - 1) * mlen)


def _unit(rng, n):
    """RootSift-like unit-norm descriptors, as test_gpu_parity.py::test_match_mfma_prefilter_equals_exact_scan draws them."""
    v = rng.random((n, 128), dtype=np.float32) ** 4
    return np.sqrt(v / v.sum(1, keepdims=True)).astype(np.float32)


def match_sets(kind, l_len, r_len):
    """(left, right) float32 descriptor sets, the same in the child and in the test.
    "ties"    : unit norm; for every k an exact copy of one left descriptor at the right indices 32k - 1 and 32k and a near
                copy at 32k + 1.  Every chunk and seed boundary is a multiple of 32, so whichever boundaries the device's
                occupancy produces, pairs of equal distance sit on both sides of each: the earlier index must win.
    "overflow": unit norm, most of the right side one descriptor: the candidate segments overflow, the call ends in the exact
                scan of every pair and does not leave the prefilter's counters tidy.
    "plain"   : unit norm."""
    rng = np.random.default_rng(1000003 * l_len + r_len)
    l, r = _unit(rng, l_len), _unit(rng, r_len)
    if kind == "ties":
        for k in range(1, (r_len - 2) // 32 + 1):
            j = (k * 61) % l_len
            r[32 * k - 1] = l[j]
            r[32 * k] = l[j]
            r[32 * k + 1] = l[j] + np.float32(1e-4)
    elif kind == "overflow":
        r[500:r_len - 400] = r[499]
    else:
        assert kind == "plain", kind
    return l, r


# name -> the calls of one child, in order: (label, kind, l_len, r_len)
MATCH_SEQUENCES = {
    # 256 CUs: resident = 256, 33 left blocks: nseed = 7 (the seed slots of the chunk that does not run are filled with +inf
    # by a memset), mchunks = 7.  First the sequence around k_match_exact's early return: an overflow call on fresh buffers
    # (the workgroups that see the flag leave their counters), the chunked call (more left descriptors: the buffers grow),
    # the overflow call again, then MORE left descriptors than that within the capacity, an ordinary call; then the chunked
    # call, one below the prefilter's limits, and the chunked call again.
    "wgs1_sequence": [
        ("overflow on fresh buffers", "overflow", 4352, 9000),
        ("chunked", "ties", 8448, 4300),
        ("overflow within the capacity", "overflow", 4352, 9000),
        ("more left descriptors within the capacity", "ties", 6400, 4300),
        ("ordinary", "plain", 700, 4531),
        ("chunked again", "ties", 8448, 4300),
        ("below the prefilter's limits", "plain", 255, 4095),
        ("chunked a third time", "ties", 8448, 4300),
    ],
    # rounds = 2: mchunks = 15 of 288, the last one 268 long
    "chunked_twice": [("chunked", "ties", 8448, 4300), ("chunked again", "ties", 8448, 4300)],
    # 129 left blocks: nseed = 1, one chunk, two candidate segments per left descriptor (should they overflow, the exact scan
    # of every pair has to give the same answer)
    "long_left": [("long left side", "ties", 33024, 4200)],
    "prefilter_size": [("exact scan at a prefilter size", "ties", 700, 4531)],
    # POPSIFT_MATCH_STATS leaves the candidate counters as they are: the second call has to zero them itself
    "prefilter_size_twice": [("first", "ties", 700, 4531), ("second", "ties", 700, 4531)],
    "overflow_then_ordinary": [("overflow", "overflow", 4352, 9000), ("ordinary", "plain", 700, 4531)],
}
