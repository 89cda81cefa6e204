// psx_tuning.h -- every environment switch of libpopsift_hip.so: one table, one struct, one parser.
//
// Host only (no HIP header: tests/test_tuning_cpu.py builds it with the host compiler).  This is the only file of the
// HIP library that calls getenv.  Lifetime: psx_create takes one snapshot per context and every launcher below api.hip
// receives it; psx_match / psx_match_u8 (no context) keep one in the calling thread's scratch, refreshed when its device
// changes; the no-device planning entries (psx_tile_selfcheck, psx_flow_selfcheck, psx_pyramid_plan, psx_blur_grid_of)
// take one per call.
//
// A row: X(kind, type, field, environment name, default, accepted values as an expression in v, meaning).
// Kinds -- a variable that is not set always leaves the default:
//   ON      flag, default on : off only when the value starts with '0' (the empty string is on)
//   OFF     flag, default off: on only when the value starts with '1'
//   SET     flag, default off: on when the variable is set to anything ("0" included)
//   INT     v = atoi(value)       : taken when accepted, otherwise the default
//   LL      v = atoll(value)      : likewise, 64 bits
//   DIGIT   v = first character - '0' (what follows is ignored): likewise
//   STR     the value as it stands (parsed where it is used)
//   STRICT  one digit and nothing behind it; anything else but the empty string is an ERROR (psx_create fails): a
//           mislabelled A/B run is worse than no run
#pragma once

#include <cstdlib>
#include <string>

#define PSX_TUNING_TABLE(X) \
    /* ---- context, schedule (api.hip) ---- */ \
    X(OFF,    bool,        hip_graph,          "POPSIFT_HIP_GRAPH",          false,   true, "1: replay psx_extract's launch chain as one hipGraph (measured: not faster than the stream launches)") \
    X(ON,     bool,        batch_octaves,      "POPSIFT_BATCH_OCTAVES",      true,    true, "0: one plane per blur launch instead of the diagonal schedule's two octaves per launch") \
    X(DIGIT,  int,         null_device_work,   "PSX_NULL_DEVICE_WORK",       0,       v == 1 || v == 2, "measurement: 1 = no kernels after a context's first frame, 2 = no DMAs either (results are stale)") \
    X(INT,    int,         cu_partitions,      "POPSIFT_CU_PARTITIONS",      0,       v >= 2 && v <= 8, "measurement: the contexts of a process take turns over this many partitions of the chip (CU-masked streams)") \
    X(INT,    int,         cu_partition_mode,  "POPSIFT_CU_PARTITION_MODE",  0,       true, "0: a partition is a set of whole XCDs, otherwise: a slice of the CUs of every XCD") \
    X(INT,    int,         wait_sleep_us,      "POPSIFT_WAIT_SLEEP_US",      40,      true, "blocking wait: microseconds slept between two event queries (0 or negative: the runtime's blocking wait)") \
    /* ---- k_blur_tile (opt-in) ---- */ \
    X(DIGIT,  int,         tile,               "POPSIFT_TILE",               0,       v == 0 || v == 1, "1: the small octaves run several levels per launch on LDS-resident tiles (bit-exact, measured slower)") \
    X(INT,    int,         tile_ty,            "POPSIFT_TILE_TY",            64,      v >= 8 && v <= 128 && (v & 3) == 0, "tile rows") \
    X(INT,    int,         tile_nt,            "POPSIFT_TILE_NT",            1024,    v == 512 || v == 1024, "threads per workgroup of the tile kernel") \
    X(LL,     long long,   tile_maxpx,         "POPSIFT_TILE_MAXPX",         3ll << 20, v >= 0, "largest plane (pixels) that takes the tile kernel") \
    X(ON,     bool,        tile_small,         "POPSIFT_TILE_SMALL",         true,    true, "0: no 32 x 32 tiles for the tiny octaves") \
    /* ---- k_pyramid_flow (opt-in) ---- */ \
    X(STRICT, int,         flow,               "POPSIFT_FLOW",               0,       v >= 0 && v <= 2, "0 (one launch per level), 1 (every level in one launch), 2 (octave 0 by launches)") \
    X(DIGIT,  int,         flow_ld,            "POPSIFT_FLOW_LD",            2,       v == 1 || v == 2, "load path of k_pyramid_flow's instantiation") \
    X(DIGIT,  int,         flow_order,         "POPSIFT_FLOW_ORDER",         0,       v >= 0 && v <= 2, "ticket order: 0 = earliest start in hops, 1 = in estimated durations, 2 = a simulated list schedule") \
    X(STR,    std::string, flow_steps,         "POPSIFT_FLOW_STEPS",         "3,2,1", true, "marching steps per work item of octave 0, 1, 2, .. (the last entry repeats; 0 = the launch-per-level chunking)") \
    X(INT,    int,         flow_grid,          "POPSIFT_FLOW_GRID",          0,       v >= 8, "workgroups of the persistent grid (0: one round of resident workgroups)") \
    X(INT,    int,         flow_debug,         "POPSIFT_FLOW_DEBUG",         0,       true, "measurement, results are wrong: 1 = no dependency waits, 2 = no arithmetic") \
    /* ---- k_blur, level 0 (pyramid.hip) ---- */ \
    X(INT,    int,         blur_dma,           "POPSIFT_BLUR_DMA",           0,       v >= 0 && v <= 3, "0: register-staged k_blur, 1 / 2 / 3: LDS-DMA staging with that many stage buffers (k_blur_dma)") \
    X(INT,    int,         blur_dma_steps,     "POPSIFT_BLUR_DMA_STEPS",     0,       v >= 2 && v <= 64, "marching steps per chunk of k_blur_dma (0: chosen per plane)") \
    X(INT,    int,         blur_steps,         "POPSIFT_BLUR_STEPS",         5,       v >= 2 && v <= 64, "marching steps per chunk on large planes") \
    X(ON,     bool,        blur_defer,         "POPSIFT_BLUR_DEFER",         true,    true, "0: the vertical results are stored at once (the round-1 kernel)") \
    X(OFF,    bool,        blur_onestep,       "POPSIFT_BLUR_ONESTEP",       false,   true, "1: the small octaves as one-step chunks where one step still yields >= 12 rows") \
    X(INT,    int,         blur_dbg,           "POPSIFT_BLUR_DBG",           0,       true, "phase-timing builds only: the phase k_blur stops after") \
    X(INT,    int,         blur_lds_pad,       "POPSIFT_BLUR_LDS_PAD",       0,       true, "measurement: extra dynamic LDS per k_blur workgroup (fewer resident workgroups per CU)") \
    X(ON,     bool,        level0_fused,       "POPSIFT_LEVEL0_FUSED",       true,    true, "0: k_upscale + k_blur<R, true> for every configuration") \
    X(ON,     bool,        level0_x2,          "POPSIFT_LEVEL0_X2",          true,    true, "0: k_level0_fused (general weights) instead of the x2-specialised kernel") \
    /* ---- GaussMode VLFeat_Relative (pyramid_interp.hip, pyramid_alt.hip) ---- */ \
    X(ON,     bool,        interp_fused,       "POPSIFT_INTERP_FUSED",       true,    true, "0: the per-level kernels of pyramid_alt.hip instead of the fused H + V kernels") \
    X(OFF,    bool,        interp_literal,     "POPSIFT_INTERP_LITERAL",     false,   true, "1: every texel fetch of the fused kernels by the literal bilinear formula") \
    X(INT,    int,         interp_steps,       "POPSIFT_INTERP_STEPS",       5,       v >= 2 && v <= 64, "marching steps per chunk on large planes") \
    X(INT,    int,         interp_minwg,       "POPSIFT_INTERP_MINWG",       384,     v > 0, "workgroups a plane must still yield before its chunks get shorter") \
    X(ON,     bool,        interp_onestep,     "POPSIFT_INTERP_ONESTEP",     true,    true, "0: no one-step chunks for the small octaves") \
    X(INT,    int,         interp_pair_rounds, "POPSIFT_INTERP_PAIR_ROUNDS", 100,     v >= 50 && v <= 1000, "percent of one round of resident workgroups two levels sharing a launch may take") \
    X(ON,     bool,        interp_diagonal,    "POPSIFT_INTERP_DIAGONAL",    true,    true, "0: one launch per level instead of the diagonal schedule") \
    /* ---- GaussMode Fixed9 / Fixed15 (pyramid_fixed.hip) ---- */ \
    X(ON,     bool,        fixed_fused,        "POPSIFT_FIXED_FUSED",        true,    true, "0: the per-level kernels of pyramid_alt.hip instead of one launch per octave") \
    X(INT,    int,         fixed_wgs,          "POPSIFT_FIXED_WGS",          0,       true, "measurement: workgroups a launch aims at (0 or negative: one round of resident workgroups)") \
    X(INT,    int,         fixed_minsteps,     "POPSIFT_FIXED_MINSTEPS",     1,       v >= 1 && v <= 8, "measurement: steps per chunk of a plane that does not fill the chip") \
    /* ---- orientation, descriptors (orient_desc.hip) ---- */ \
    X(INT,    int,         ori_wpb,            "POPSIFT_ORI_WPB",            4,       v == 1 || v == 4, "waves per k_orientation workgroup (measured: no difference)") \
    X(INT,    int,         alt_wgs,            "POPSIFT_ALT_WGS",            8,       v >= 1 && v <= 64, "k_descriptors_alt workgroups per CU") \
    X(ON,     bool,        alt_window,         "POPSIFT_ALT_WINDOW",         true,    true, "0: k_descriptors_alt reads every texel from the plane in HBM") \
    X(DIGIT,  int,         desc_occ,           "POPSIFT_DESC_OCC",           0,       v == 5, "5: the k_descriptors instantiation padded to five workgroups per CU") \
    X(INT,    int,         desc_wgs,           "POPSIFT_DESC_WGS",           0,       v >= 1 && v <= 64, "k_descriptors workgroups per CU (0: 12, or 2 with the zero-copy export attached; 10 / 3 under POPSIFT_DESC_OCC=5)") \
    X(ON,     bool,        desc_denorm,        "POPSIFT_DESC_DENORM",        true,    true, "0: round 2's conversion path instead of the denormal products") \
    X(INT,    int,         desc_wpb,           "POPSIFT_DESC_WPB",           0,       v == 1 || v == 2 || v == 4, "waves per k_descriptors workgroup (0: one, or four with the zero-copy export attached)") \
    /* ---- psx_match (match.hip) ---- */ \
    X(ON,     bool,        match_mfma,         "POPSIFT_MATCH_MFMA",         true,    true, "0: the exact scan of every pair instead of the MFMA prefilter") \
    X(INT,    int,         match_wgs_per_cu,   "POPSIFT_MATCH_WGS_PER_CU",   0,       v >= 1 && v <= 8, "prefilter workgroups counted as resident per CU (0: the runtime's occupancy query)") \
    X(SET,    bool,        match_stats,        "POPSIFT_MATCH_STATS",        false,   true, "set to anything: print the prefilter's candidates per left descriptor") \
    X(INT,    int,         match_rounds,       "POPSIFT_MATCH_ROUNDS",       1,       v >= 1 && v <= 4, "rounds of resident workgroups the prefilter's chunking aims at")

struct PsxTuning {
#define X(kind, type, field, env, dflt, accept, doc) type field = dflt;
    PSX_TUNING_TABLE(X)
#undef X
    int cus = 256;      // compute units of the device the snapshot is used on (psx_create, psx_match); 256 when the query fails
};

namespace psx_tuning_detail {
// e: the variable's value (never null), f: the field, ok: the row's accept expression
template <class T, class A> void read_ON(const char* e, T& f, A, const char*, std::string*) { f = e[0] != '0'; }
template <class T, class A> void read_OFF(const char* e, T& f, A, const char*, std::string*) { f = e[0] == '1'; }
template <class T, class A> void read_SET(const char*, T& f, A, const char*, std::string*) { f = true; }
template <class T, class A> void read_INT(const char* e, T& f, A ok, const char*, std::string*) { const int v = atoi(e); if (ok(v)) f = v; }
template <class T, class A> void read_LL(const char* e, T& f, A ok, const char*, std::string*) { const long long v = atoll(e); if (ok(v)) f = v; }
template <class T, class A> void read_DIGIT(const char* e, T& f, A ok, const char*, std::string*) { const int v = e[0] - '0'; if (ok(v)) f = v; }
template <class T, class A> void read_STR(const char* e, T& f, A, const char*, std::string*) { f = e; }
template <class T, class A> void read_STRICT(const char* e, T& f, A ok, const char* env, std::string* error)
{
    if (e[0] != 0 && e[1] == 0 && ok(e[0] - '0')) f = e[0] - '0';
    else if (e[0] != 0 && error && error->empty())
        *error = std::string(env) + "=" + e + ": valid values are 0 (one launch per level), 1 (every level in one launch), 2 (octave 0 by launches)";
}
} // namespace psx_tuning_detail

// walks the table once; *error (optional) is left empty unless a STRICT row holds a bad value
inline PsxTuning psx_tuning_from_env(std::string* error = nullptr)
{
    PsxTuning t;
    if (error) error->clear();
#define X(kind, type, field, env, dflt, accept, doc) \
    if (const char* e = getenv(env)) psx_tuning_detail::read_##kind(e, t.field, [](long long v) { (void)v; return accept; }, env, error);
    PSX_TUNING_TABLE(X)
#undef X
    if (t.wait_sleep_us < 0) t.wait_sleep_us = 0;
    return t;
}
