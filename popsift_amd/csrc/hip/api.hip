// api.hip -- implementation of the C-ABI declared in include/popsift_hip.h.
//
// One psx_ctx == one Pyramid of the reference (sift_pyramid.h:53-163) plus the state the
// reference keeps in global __device__/__constant__/thread_local symbols (gauss tables
// gauss_filter.cu:18-21, constants sift_constants.cu:19-20, counters and buffers
// sift_pyramid.cu:41-49).  Because nothing is global, any number of contexts can live on one
// device; the batch dispatcher uses that to keep several frames in flight per GPU.
//
// Stream model: every context owns one HIP stream; a frame is one stream-ordered chain
//   memset(counters) -> k_level0_fused -> k_blur / k_blur2 in the diagonal schedule (the frame's plan, pyramid_plan.h, built
//   in psx_resize and issued by psx_build_pyramid), a large octave's
//   k_extrema right behind its last level and one batched k_extrema for the small octaves -> k_refine
//   -> k_orientation -> k_scan -> k_descriptors
// (default configuration; the other Gauss and scaling modes build their pyramid in pyramid_alt.hip, POPSIFT_FLOW and
// POPSIFT_TILE select other launch schedules) with no host synchronisation inside the chain (the reference has four
// blocking counter round-trips and four device-wide syncs per image).
#include "psx_internal.h"
#include "psx_owned.h"
#include "blur_tile_core.h"
#include "kp_place.h"
#include "mask_rule.h"
#include "pyramid_plan.h"

#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <memory>
#include <new>
#include <string>
#include <vector>

namespace {

thread_local std::string g_create_error;

inline int imin(int a, int b) { return a < b ? a : b; }
inline int imax(int a, int b) { return a > b ? a : b; }

// ---- Gauss tables: restatement of gauss_filter.cu:127-371 (host arithmetic) -----------------
int vlfeat_span(float sigma) { return imin((int)(ceilf(4.0f * sigma) + 1), PSX_GAUSS_ALIGN - 1); }
int opencv_span(float sigma)
{
    int span = (int)(roundf(2.0f * 4.0f * sigma + 1.0f)) | 1;
    span >>= 1;
    span += 1;
    return imin(span, PSX_GAUSS_ALIGN - 1);
}
int get_span(int mode, float sigma)
{
    switch (mode) {
    case PSX_GAUSS_VLFEAT_RELATIVE_ALL:
    case PSX_GAUSS_VLFEAT_COMPUTE: return vlfeat_span(sigma);
    case PSX_GAUSS_VLFEAT_RELATIVE: { int s = vlfeat_span(sigma); if ((s & 1) == 0) s += 1; return s; }
    case PSX_GAUSS_OPENCV_COMPUTE: return opencv_span(sigma);
    case PSX_GAUSS_FIXED9: return 5;
    case PSX_GAUSS_FIXED15: return 8;
    default: return -1;
    }
}
void blur_table(int mode, int nlev, const float* sigma, int* span, float* filter)
{
    for (int level = 0; level < nlev; level++)
        span[level] = imin(get_span(mode, sigma[level]), PSX_GAUSS_ALIGN - 1);
    for (int level = 0; level < nlev; level++) {
        const float sig = sigma[level];
        const int spn = span[level];
        float* f = filter + level * PSX_GAUSS_ALIGN;
        double sum = 1.0;
        f[0] = 1.0f;
        for (int x = 1; x < spn; x++) {
            const float val = (float)std::exp(-0.5 * (std::pow(double(x) / sig, 2.0)));
            f[x] = val;
            sum += 2.0f * val;
        }
        for (int x = 0; x < spn; x++) f[x] = (float)(f[x] / sum);
        for (int x = spn; x < PSX_GAUSS_ALIGN; x++) f[x] = 0.0f;
    }
}

} // namespace

constexpr size_t CNT_BLOCK = 512;      // bytes reserved for PsxCounters in front of the flow state and the candidate counters
constexpr size_t FLOW_MAX_BYTES = sizeof(int) * (size_t)(PSX_FLOW_HEAD_INTS + PSX_FLOW_MAX_COUNTERS * PSX_FLOW_CNT_STRIDE);
constexpr size_t CAND_CT_BYTES = sizeof(int) * (size_t)PSX_MAX_OCTAVES * PSX_CAND_SUB * 32;

struct psx_ctx {
    // Members are destroyed in reverse order of declaration: the stream goes last, after every buffer, event and graph
    // that work queued on it may use (psx_destroy has waited for it by then).
    Stream      stream;
    int         device = 0;
    psx_config  cfg{};
    PsxTuning   tune;                  // the environment switches as psx_create found them, and the device's CU count
    std::string err;

    PsxGaussTables tab;
    bool  alt_pyramid = false;         // any branch of build_pyramid other than the default one
    DevBuf<float> d_intm, d_vbuf;      // scratch planes of the alternative branches

    int in_w = 0, in_h = 0;
    int octaves_resolved = -1;         // sticky auto-octave value (popsift.cpp:118-122)
    PsxParams    hp{};
    DevBuf<PsxParams>    d_params;
    PinnedBuf<PsxParams> h_params_pin; // pinned mirror: source of the asynchronous parameter updates
    // frame counters, flow state and candidate sub-list counters in ONE allocation (psx_create); d_cnt and d_cand_ct point into it
    DevBuf<unsigned char> d_cnt_block;
    PsxCounters* d_cnt = nullptr;
    int* d_cand_ct = nullptr;
    PinnedBuf<PsxCounters> h_cnt;
    bool counts_valid = false;
    bool counts_partial = false;       // only ext_total / ori_total valid (export fast path)

    Staged<unsigned char> input_own;   // device copy of a host image (bytes); pinned caller memory skips its staging block
    const void* d_input = nullptr;     int input_is_float = 0;

    DevBuf<float> d_pyr;
    DevBuf<float> d_up;                // resampled input of octave 0
    int up_pitch = 0;
    DevBuf<psx_iext> d_iext;
    DevBuf<int> d_iext_off;
    DevBuf<unsigned long long> d_cand;
    DevBuf<psx_extremum> d_extrema;
    DevBuf<psx_feature> d_features;
    DevBuf<float> d_desc;
    // byte descriptors (psx_set_descriptor_format): the quantised copy of d_desc, 128 bytes per descriptor, grown with it
    int desc_fmt = PSX_DESCFMT_F32;
    DevBuf<unsigned char> d_desc_u8;
    DevBuf<int> d_feat_to_ext;
    DevBuf<int> d_ext_nori;

    // grid filter scratch (allocated on first use)
    DevBuf<unsigned long long> d_gf_keys;    // 2 x total
    DevBuf<unsigned> d_gf_vals;              // 2 x total
    DevBuf<unsigned char> d_gf_temp;
    DevBuf<int> d_gf_scratch;
    bool filtered = false;             // the grid filter ran on the current frame
    bool interleave = false;           // psx_extract: launch an octave's extrema scan right behind its last blur level
    bool ext_launched = false;         // ... which has happened for the current frame
    bool pyr_ready = false;            // the pyramid has been (queued to be) built from the current input
    int  resident_blocks = 1024;       // 4 x tune.cus
    bool blocking_wait = false;        // psx_set_wait_mode: sleep on an event instead of spinning in hipStreamSynchronize
    Event ev_wait;

    // psx_extract's whole launch chain captured as a hipGraph; valid for one (input pointer, type, size, mask);
    // everything else the kernels read is device resident (PsxParams) or constant per context (taps)
    struct {
        GraphExec exec;
        const void* input = nullptr; int is_float = 0, w = 0, h = 0;
        const unsigned char* mask = nullptr;                             // the mask the captured graph's kernels carry
        bool off = true;               // !tune.hip_graph (POPSIFT_HIP_GRAPH=1 enables it); switched off again if a capture fails
    } graph;

    // zero-copy export
    struct {
        MappedHost feat, desc;
        MappedHost u8;                 // the byte export (psx_attach_export_u8): replaces desc
        PinnedBuf<int> counts;         // [4]: ext_total, ori_total, ori_raw, flow_error
        // the export targets the frame in flight was LAUNCHED with (psx_orientation): the attach calls may change the
        // targets of the next frame before this one's counters and results have been fetched
        PsxExport fx{};
        const void *fx_host_feat = nullptr, *fx_host_desc = nullptr, *fx_host_u8 = nullptr;
        bool fx_on = false;
    } xp;

    // MEASUREMENT switch PSX_NULL_DEVICE_WORK (bench.py host_ceiling): 1 = after a context's first frame psx_extract launches
    // nothing -- uploads, the counter read-back and the result downloads still run, on the first frame's results (same
    // counts, same bytes): what the HOST path and PCIe sustain without the kernels; 2 = the DMAs are skipped as well: the
    // host software alone (threads, queues, pools, the per-keypoint record loop).  Results are stale by construction.
    struct {
        bool primed = false;
        bool dl_done = false;          // mode 2: this context's one real download has happened
    } nulldev;

    struct {
        bool on = false;               // psx_enable_timers: ev[0..4] bracket the four stages
        Event ev[5];
        Event t0, t1;                  // psx_time_blur
        // in-pipeline timing of the octave-0 separable-Gaussian launches (psx_enable_blur_probe)
        bool probe = false;
        Event ev_blur[2 * PSX_GAUSS_LEVELS];   // [2l], [2l+1]: begin / end of the level-(l+1) kernel
        Event ev_x[4];                 // the probe also brackets octave 0's level 0 [0,1] and its extrema scan [2,3] (stream events)
        bool probe_ext0 = false;       // octave 0's extrema scan was a launch of its own in the last extraction
        int  probe_n = 0;              // levels timed in the last extraction
        double probe_bytes = 0.0;      // algorithmic bytes per timed launch (8 B per pixel of every plane the launch blurs), averaged
    } tm;

    // k_pyramid_flow (POPSIFT_FLOW: 0 = one launch per level -- the default: the one-launch kernel measured 172 us against
    // 190 us of launches for a single 1080p frame but -10 % throughput with several frames in flight, DESIGN.md 3.1b --,
    // 1 = every blur level of the frame in one launch, 2 = octave 0 by launches, octaves >= 1 in one launch)
    struct {
        bool on = false;               // a plan exists for the current size
        int  first = 0, nitems = 0, grid = 0, ncnt = 0, njobs = 0;
        size_t bytes = 0;              // ticket words + chunk counters, between PsxCounters and the candidate counters
        double algo_bytes = 0.0;       // algorithmic bytes of the launch (8 B per pixel and blurred plane + 4 B per decimated pixel)
        DevBuf<PsxFlowJob>  jobs;
        DevBuf<PsxFlowItem> items;
        long long* trace = nullptr;    // psx_flow_trace's buffer while it runs
    } flow;

    // k_blur_tile (pyramid_tile.hip): the octaves that cannot fill the chip run several levels per launch on LDS-resident
    // tiles -- levels 1..L-3 (+ the decimation) of octave o together with levels L-2..L-1 of octave o-1 in ONE launch.
    // OPT-IN (POPSIFT_TILE=1; default: one launch per level, the diagonal schedule): bit-exact, five pyramid launches
    // for octaves 1-4 instead of thirteen, but measured slower on MI355X (profiles/r05_tile_schedule_ab.txt: single frame
    // 0.467 vs 0.436 ms, 8-context throughput -11 %): a tile is a serial chain of passes whose instruction overhead per
    // 8 x 8 block (addresses, predicates, stores) is ~2x its filter arithmetic, and the halo work is 1.65x.
    // POPSIFT_TILE_MAXPX: largest plane (pixels) that takes the tile kernel; POPSIFT_TILE_TY / POPSIFT_TILE_NT: tile rows
    // (32 / 64) and threads per workgroup (512 / 1024); POPSIFT_TILE_SMALL=0: no 32 x 32 tiles for the tiny octaves
    struct TileLaunch { int job0, njobs, grid; size_t lds; };
    struct {
        bool on = false;               // a tile schedule exists for the current size
        int  first = 0;                // first octave on the tile kernel; the octaves in front keep one launch per level
        std::vector<TileLaunch> launches;
        DevBuf<PsxTileJob> jobs;
    } tile;

    // The frame's blur and scan launches in issue order (pyramid_plan.h), rebuilt where sizes or tuning change: in
    // psx_resize.  plan_own: the flow or tile schedule in force, empty when there is none; plan_diagonal: the default
    // schedule, which also serves where the tile schedule steps aside for the blur probe (frame_plan) and, through its
    // scan steps alone, the alternative modes.
    PsxPlan plan_diagonal, plan_own;

    // caller-supplied keypoints (psx_set_keypoints / psx_describe, keypoints.hip)
    struct {
        bool set = false;              // a keypoint list is set (possibly empty)
        bool results = false;          // the last results are a psx_describe's (psx_keypoint_map)
        const psx_keypoint* list = nullptr; int n = 0;                   // the list of the next psx_describe
        Staged<psx_keypoint> own;      // device copy of a host list
        DevBuf<int>   tbl, src, gnori; // side arrays of psx_describe (PsxKpBuffers)
        DevBuf<float> gori;
    } kp;

    // detection mask (psx_set_mask / psx_set_mask_dev, mask_rule.h): sticky until replaced or cleared
    struct {
        const unsigned char* data = nullptr; int w = 0, h = 0;           // the mask in force (nullptr: none)
        Staged<unsigned char> own;     // device copy of a host mask
    } mask;
};

namespace {

inline bool exporting(const psx_ctx* c) { return c->xp.feat.dev != nullptr || c->xp.desc.dev != nullptr || c->xp.u8.dev != nullptr; }
PsxExport export_of(const psx_ctx* c)
{
    PsxExport x;
    x.features = static_cast<psx_feature*>(c->xp.feat.dev); x.desc = static_cast<float*>(c->xp.desc.dev);
    x.counts = exporting(c) ? c->xp.counts.p : nullptr;
    // one descriptor target at a time: every attach call detaches the other one
    x.feat_capacity = c->xp.feat.capacity; x.desc_capacity = c->xp.desc.dev ? c->xp.desc.capacity : c->xp.u8.capacity;
    const bool bytes = c->desc_fmt == PSX_DESCFMT_U8;
    x.desc_u8 = bytes ? c->d_desc_u8.p : nullptr;
    x.xdesc_u8 = bytes ? static_cast<unsigned char*>(c->xp.u8.dev) : nullptr;
    return x;
}
inline PsxMask mask_of(const psx_ctx* c) { return PsxMask{c->mask.data, c->mask.w, c->mask.h}; }
// PSX_OK, or PSX_ERR_STATE when a mask is set whose size is not the current input's (never dropped silently)
int fail(psx_ctx* c, int code, const std::string& msg);
int check_mask(psx_ctx* c, const char* who)
{
    if (!c->mask.data || (c->mask.w == c->in_w && c->mask.h == c->in_h)) return PSX_OK;
    char buf[256];
    snprintf(buf, sizeof(buf), "%s: the detection mask is %d x %d but the input image is %d x %d", who, c->mask.w, c->mask.h,
             c->in_w, c->in_h);
    return fail(c, PSX_ERR_STATE, buf);
}
inline void snapshot_export(psx_ctx* c)
{
    c->xp.fx = export_of(c);
    c->xp.fx_host_feat = c->xp.feat.host; c->xp.fx_host_desc = c->xp.desc.host; c->xp.fx_host_u8 = c->xp.u8.host;
    c->xp.fx_on = exporting(c);
}

int fail(psx_ctx* c, int code, const std::string& msg)
{
    if (c) c->err = msg; else g_create_error = msg;
    return code;
}

#define PSX_HIP(call)                                                                           \
    do {                                                                                        \
        hipError_t e__ = (call);                                                                \
        if (e__ != hipSuccess) {                                                                \
            char buf__[512];                                                                    \
            snprintf(buf__, sizeof(buf__), "%s:%d\n    %s failed: %s", __FILE__, __LINE__, #call, \
                     hipGetErrorString(e__));                                                   \
            return fail(ctx, PSX_ERR_HIP, buf__);                                               \
        }                                                                                       \
    } while (0)

int compute_tables(const psx_config* cfg, PsxGaussTables* t, std::string* why)
{
    const float sigma0 = cfg->sigma;
    const int levels = cfg->levels;
    if (sigma0 > 2.0) { if (why) *why = "ERROR:  Sigma > 2.0 is not supported."; return PSX_ERR_INVALID; }
    if (levels + 3 > PSX_GAUSS_LEVELS) {
        if (why) *why = "ERROR:  More than 12 levels not supported.";
        return PSX_ERR_INVALID;
    }
    if (get_span(cfg->gauss_mode, 1.0f) < 0) {
        if (why) *why = "ERROR: The mode for computing Gauss filter scan is invalid";
        return PSX_ERR_INVALID;
    }
    memset(t->inc_filter, 0, sizeof(float) * PSX_GAUSS_LEVELS * PSX_GAUSS_ALIGN);
    memset(t->inc_sigma, 0, sizeof(float) * PSX_GAUSS_LEVELS);
    memset(t->dd_filter, 0, sizeof(float) * PSX_MAX_OCTAVES * PSX_GAUSS_ALIGN);
    const int stages = levels + 3;
    const float initial_blur = cfg->assume_initial_blur
                             ? cfg->initial_blur * powf(2.0f, cfg->upscale_factor) : 0.0f;
    t->inc_sigma[0] = cfg->assume_initial_blur
                 ? sqrtf(fabsf(sigma0 * sigma0 - initial_blur * initial_blur)) : sigma0;
    for (int lvl = 1; lvl < stages; lvl++) {
        const float sigmaP = sigma0 * powf(2.0f, (float)(lvl - 1) / (float)levels);
        const float sigmaS = sigma0 * powf(2.0f, (float)(lvl) / (float)levels);
        t->inc_sigma[lvl] = sqrtf(sigmaS * sigmaS - sigmaP * sigmaP);
    }
    blur_table(cfg->gauss_mode, PSX_GAUSS_LEVELS, t->inc_sigma, t->inc_span, t->inc_filter);
    for (int oct = 0; oct < PSX_MAX_OCTAVES; oct++) {
        const float oct_sigma = scalbnf(sigma0, oct);
        const float b = sqrtf(fabsf(oct_sigma * oct_sigma - initial_blur * initial_blur));
        t->dd_sigma[oct] = scalbnf(b, -oct);
    }
    blur_table(cfg->gauss_mode, PSX_MAX_OCTAVES, t->dd_sigma, t->dd_span, t->dd_filter);
    return PSX_OK;
}

// abs_o0, abs_oN and the interpolated (ratio, multiplier) form of the inc table
void compute_alt_tables(const psx_config& c, PsxGaussTables* t)
{
    const float sigma0 = c.sigma;
    const int levels = c.levels, stages = levels + 3;
    const float initial_blur = c.assume_initial_blur ? c.initial_blur * powf(2.0f, c.upscale_factor) : 0.0f;
    float *const s0 = t->abs0_sigma, *const sN = t->absN_sigma;
    for (int lvl = 0; lvl < PSX_GAUSS_LEVELS; lvl++) s0[lvl] = sN[lvl] = 0.0f;
    for (int lvl = 0; lvl < stages; lvl++) {
        const float sigmaS = sigma0 * powf(2.0f, (float)(lvl) / (float)levels);
        s0[lvl] = sqrtf(fabsf(sigmaS * sigmaS - initial_blur * initial_blur));
        if (lvl > 0) sN[lvl] = sqrtf(sigmaS * sigmaS - sigma0 * sigma0);
    }
    blur_table(c.gauss_mode, PSX_GAUSS_LEVELS, s0, t->abs0_span, t->abs0_filter);
    blur_table(c.gauss_mode, PSX_GAUSS_LEVELS, sN, t->absN_span, t->absN_filter);
    for (int level = 0; level < PSX_GAUSS_LEVELS; level++) {       // GaussTable::transformBlurTable
        int isp = t->inc_span[level];
        if (!(isp & 1)) isp += 1;
        t->inc_ispan[level] = isp;
        const float* f = t->inc_filter + level * PSX_GAUSS_ALIGN;
        float* fi = t->inc_ifilter + level * PSX_GAUSS_ALIGN;
        for (int x = 0; x < PSX_GAUSS_ALIGN; x++) fi[x] = 0.0f;
        for (int x = 1; x < isp; x += 2) {
            const float a = f[x], b = f[x + 1];
            fi[x] = a / (a + b);
            fi[x + 1] = a + b;
        }
        fi[0] = f[0];
    }
}

PsxTaps taps_from(const float* row)
{
    PsxTaps t;
    for (int i = 0; i < PSX_GAUSS_ALIGN; i++) t.g[i] = row[i];
    return t;
}

// the captured graph carries the input, the mask, the export targets and the descriptor arrays as kernel arguments
void drop_graph(psx_ctx* ctx) { ctx->graph.exec.reset(); }

} // namespace

// ---- k_blur_tile: the schedule of a frame size (psx_resize) --------------------------------------------------------------
// The blur levels 1..L-1 of every octave from tile_first on are cut into groups of consecutive levels, each one job of the
// tile kernel: a group ends at level L-3 (the level that feeds the next octave: the next octave must not wait for more) and
// wherever the plan of blur_tile_core.h says "does not fit" (LDS, Q's width).  A job runs in the launch slot behind its
// producer -- the previous group of its octave, or the group of the octave above that ends at level L-3 -- and all jobs of
// a slot share one launch, the deepest octave (the head of the dependency chain) first.  Default configuration: slot s =
// {levels 1..3 of octave first + s, levels 4..5 of octave first + s - 1}.
struct TileSched { std::vector<PsxTileJob> jobs; std::vector<psx_ctx::TileLaunch> launches; std::vector<int> octave, l0, slot; int first = 0; };
// false: nothing to run on the tile kernel (no octave small enough, or a level it is not built for)
static bool tile_schedule(const PsxParams& P, const int* inc_span, const float* inc_filter, int tile_ty, int tile_nt,
                          long long maxpx, bool small_tiles, TileSched& out)
{
    const int L = P.L, D = L - 3;
    int first = 0;
    while (first < P.num_octaves && (long long)P.oct[first].w * P.oct[first].h > maxpx) first++;
    if (first >= P.num_octaves || D < 1) return false;
    struct Group { int octave, l0, nlev, slot; PsxTileJob job; size_t lds; };
    std::vector<Group> groups;
    int feeder_slot = -1;                              // slot of the group that writes level 0 of the octave being planned
    const int rows_cap = (tile_nt >= 1024 ? 8 : 16);
    for (int o = first; o < P.num_octaves; o++) {
        const PsxOctave& oc = P.oct[o];
        // an octave that cannot give every CU a 64-column tile takes 32 x 32 tiles: a tile is a serial chain of passes,
        // what counts for such an octave is the length of that chain, not the halo work it repeats
        int tx = 64, ty = tile_ty;
        if (small_tiles && ((oc.w + 63) / 64) * ((oc.h + ty - 1) / ty) < 200) { tx = 32; ty = 32; }
        int l = 1, prev_slot = feeder_slot, next_feeder = -1;
        while (l < L) {
            const int lmax = l <= D ? D : L - 1;       // a group does not cross level L-3
            int n = lmax - l + 1;
            if (n > PSX_TILE_MAXLEV) n = PSX_TILE_MAXLEV;
            Group g{};
            for (; n >= 1; n--) {
                int radii[PSX_TILE_MAXLEV];
                for (int k = 0; k < n; k++) radii[k] = inc_span[l + k] - 1;
                memset(&g.job, 0, sizeof(g.job));
                g.lds = psx_tile_plan_job(g.job, oc.w, oc.h, oc.pitch, n, radii, tx, ty);
                if (g.lds != 0 && g.job.h.NR <= rows_cap * (tile_nt >> g.job.h.lpr_shift)) break;
            }
            if (n < 1) return false;                   // a level the tile kernel is not built for: keep the launches
            g.octave = o; g.l0 = l; g.nlev = n; g.slot = prev_slot + 1;
            PsxTileHdr& h = g.job.h;
            h.src = oc.data + (size_t)(l - 1) * oc.plane;
            h.half_dst = nullptr; h.half_pitch = 0; h.half_lev = -1;
            for (int k = 0; k < n; k++) {
                g.job.dst[k] = oc.data + (size_t)(l + k) * oc.plane;
                for (int q = 0; q < PSX_GAUSS_ALIGN; q++) g.job.taps[k].g[q] = inc_filter[(l + k) * PSX_GAUSS_ALIGN + q];
            }
            if (l <= D && l + n - 1 == D) {
                next_feeder = g.slot;
                if (o + 1 < P.num_octaves) { h.half_dst = P.oct[o + 1].data; h.half_pitch = P.oct[o + 1].pitch; h.half_lev = D - l; }
            }
            prev_slot = g.slot;
            groups.push_back(g);
            l += n;
        }
        feeder_slot = next_feeder;
    }
    int nslots = 0;
    for (const Group& g : groups) if (g.slot + 1 > nslots) nslots = g.slot + 1;
    for (int s = 0; s < nslots; s++) {
        psx_ctx::TileLaunch ln{(int)out.jobs.size(), 0, 0, 0};
        for (int o = P.num_octaves - 1; o >= first; o--)
            for (const Group& g : groups)
                if (g.slot == s && g.octave == o) {
                    PsxTileJob j = g.job;
                    j.h.block0 = ln.grid;
                    ln.grid += j.h.tiles_x * j.h.tiles_y;
                    if (g.lds > ln.lds) ln.lds = g.lds;
                    ln.njobs++;
                    out.jobs.push_back(j);
                    out.octave.push_back(g.octave); out.l0.push_back(g.l0); out.slot.push_back(s);
                }
        if (ln.njobs > 0) out.launches.push_back(ln);
    }
    out.first = first;
    return !out.jobs.empty();
}

static int plan_tiles(psx_ctx* ctx)
{
    ctx->tile.on = false;
    ctx->tile.launches.clear();
    const PsxTuning& t = ctx->tune;
    if (t.tile == 0 || ctx->alt_pyramid || ctx->flow.on) return PSX_OK;
    TileSched sc;
    if (!tile_schedule(ctx->hp, ctx->tab.inc_span, ctx->tab.inc_filter, t.tile_ty, t.tile_nt, t.tile_maxpx, t.tile_small, sc)) return PSX_OK;
    PSX_HIP(ctx->tile.jobs.grow(sc.jobs.size()));
    PSX_HIP(hipMemcpy(ctx->tile.jobs, sc.jobs.data(), sizeof(PsxTileJob) * sc.jobs.size(), hipMemcpyHostToDevice));
    ctx->tile.launches = sc.launches;
    ctx->tile.on = true;
    ctx->tile.first = sc.first;
    return PSX_OK;
}

// Host-only self check of a tile schedule (no device needed; tests/test_capi_cpu.py): every level 1..L-1 of every octave
// from the first tiled one on is produced by exactly one job, a job sits in a later launch than the job that writes its
// source plane, the decimated plane of an octave is written by the job that ends at level L-3, workgroup ranges of a
// launch are contiguous.  Returns the number of jobs (0: the kernel would not be used), or a negative code naming the
// violated invariant.  stats (optional, 4 ints): first tiled octave, launches, largest LDS need, largest grid.
extern "C" int psx_tile_selfcheck(int w0, int h0, int num_octaves, int levels, const int* spans, int tile_ty, int tile_nt,
                                  long long maxpx, int* stats)
{
    PsxParams P;
    if (!psx_plan_params(w0, h0, num_octaves, levels, &P)) return -1;
    std::vector<float> filt((size_t)PSX_GAUSS_LEVELS * PSX_GAUSS_ALIGN, 0.0f);
    TileSched sc;
    if (!tile_schedule(P, spans, filt.data(), tile_ty, tile_nt, maxpx, psx_tuning_from_env().tile_small, sc)) return 0;
    const int L = P.L, D = L - 3;
    std::vector<int> writer((size_t)num_octaves * L, -1), wslot((size_t)num_octaves * L, -1);
    for (size_t q = 0; q < sc.jobs.size(); q++) {
        const PsxTileJob& j = sc.jobs[q];
        const int o = sc.octave[q], l0 = sc.l0[q];
        if (o < sc.first || o >= num_octaves || l0 < 1 || l0 + j.h.nlev > L) return -2;
        if (j.h.src != P.oct[o].data + (size_t)(l0 - 1) * P.oct[o].plane || j.h.W != P.oct[o].w || j.h.H != P.oct[o].h) return -3;
        for (int k = 0; k < j.h.nlev; k++) {
            if (j.dst[k] != P.oct[o].data + (size_t)(l0 + k) * P.oct[o].plane) return -3;
            if (spans[l0 + k] - 1 > psx_tile_radius(j.lev[k].rsel)) return -4;
            int& wr = writer[(size_t)o * L + l0 + k];
            if (wr != -1) return -5;
            wr = (int)q; wslot[(size_t)o * L + l0 + k] = sc.slot[q];
        }
        const bool feeds = l0 <= D && l0 + j.h.nlev - 1 == D && o + 1 < num_octaves;
        if (feeds != (j.h.half_dst != nullptr)) return -6;
        if (feeds) {
            if (j.h.half_dst != P.oct[o + 1].data || j.h.half_lev != D - l0 || j.h.half_pitch != P.oct[o + 1].pitch) return -6;
            writer[(size_t)(o + 1) * L] = (int)q; wslot[(size_t)(o + 1) * L] = sc.slot[q];
        }
    }
    for (int o = sc.first; o < num_octaves; o++)
        for (int l = 1; l < L; l++) if (writer[(size_t)o * L + l] < 0) return -7;
    for (size_t q = 0; q < sc.jobs.size(); q++) {
        const int o = sc.octave[q], l0 = sc.l0[q];
        const int src_slot = (o == sc.first && l0 == 1) ? -1 : wslot[(size_t)o * L + l0 - 1];
        if (!(o == sc.first && l0 == 1) && (src_slot < 0 || src_slot >= sc.slot[q])) return -8;   // the producer is not in an earlier launch
    }
    size_t maxlds = 0; int maxgrid = 0;
    for (const psx_ctx::TileLaunch& ln : sc.launches) {
        int at = 0;
        for (int q = 0; q < ln.njobs; q++) {
            const PsxTileJob& j = sc.jobs[(size_t)ln.job0 + q];
            if (j.h.block0 != at) return -9;
            at += j.h.tiles_x * j.h.tiles_y;
            if (sc.slot[(size_t)ln.job0 + q] != sc.slot[(size_t)ln.job0]) return -9;
        }
        if (at != ln.grid || ln.lds == 0 || ln.lds > PSX_TILE_LDS_MAX) return -9;
        if (ln.lds > maxlds) maxlds = ln.lds;
        if (ln.grid > maxgrid) maxgrid = ln.grid;
    }
    if (stats) { stats[0] = sc.first; stats[1] = (int)sc.launches.size(); stats[2] = (int)maxlds; stats[3] = maxgrid; }
    return (int)sc.jobs.size();
}

// psx_pyramid_plan, psx_blur_grid_of (include/popsift_hip.h): the step list a context of this size would issue, no device
extern "C" int psx_pyramid_plan(int w0, int h0, int num_octaves, int levels, const int* spans, int resident_blocks, int schedule,
                                int first, psx_step* steps, int capacity, int* count)
{
    PsxParams P;
    if (!spans || !count || capacity < 0 || (capacity > 0 && !steps) || w0 < 1 || h0 < 1 || levels < 1 || resident_blocks < 1 ||
        schedule < PSX_PLAN_DIAGONAL || schedule > PSX_PLAN_FLOW || !psx_plan_params(w0, h0, num_octaves, levels, &P))
        return PSX_ERR_INVALID;
    const PsxTuning t = psx_tuning_from_env();
    int ntile = 0;
    if (schedule == PSX_PLAN_TILE) {
        std::vector<float> filt((size_t)PSX_GAUSS_LEVELS * PSX_GAUSS_ALIGN, 0.0f);
        TileSched sc;
        if (!tile_schedule(P, spans, filt.data(), t.tile_ty, t.tile_nt, t.tile_maxpx, t.tile_small, sc)) return PSX_ERR_STATE;
        first = sc.first; ntile = (int)sc.launches.size();
    } else if (schedule == PSX_PLAN_FLOW && (first < 0 || first > 1 || first >= num_octaves)) return PSX_ERR_INVALID;
    PsxPlan plan;
    psx_pyramid_steps(P, spans, t, resident_blocks, schedule, first, ntile, plan);
    *count = (int)plan.size();
    for (int i = 0; i < *count && i < capacity; i++) steps[i] = plan[(size_t)i];
    return PSX_OK;
}

extern "C" int psx_blur_grid_of(int W, int H, int span) { return W < 1 || H < 1 || span < 1 ? PSX_ERR_INVALID : psx_blur_grid(psx_tuning_from_env(), W, H, span); }

extern "C" {

const char* psx_version(void) { return "popsift-mi355x 0.1 (gfx950, HIP)"; }

int psx_config_default(psx_config* c)
{
    if (!c) return PSX_ERR_INVALID;
    memset(c, 0, sizeof(*c));
    c->octaves = -1;
    c->levels = 3;
    c->sigma = 1.6f;
    c->edge_limit = 10.0f;
    c->threshold = (float)0.04;
    c->upscale_factor = 1.0f;
    c->gauss_mode = PSX_GAUSS_VLFEAT_COMPUTE;
    c->sift_mode = PSX_MODE_POPSIFT;
    c->scaling_mode = PSX_SCALE_DEFAULT;
    c->desc_mode = PSX_DESC_LOOP;
    c->norm_mode = PSX_NORM_ROOTSIFT;
    c->norm_multi = 0;
    c->max_extrema = 100000;
    c->assume_initial_blur = 1;
    c->initial_blur = 0.5f;
    c->filter_max_extrema = -1;
    c->filter_grid_size = 2;
    c->grid_filter_mode = PSX_FILTER_RANDOM;
    return PSX_OK;
}

float psx_peak_threshold(const psx_config* c) { return c->threshold * 0.5f * 255.0f / c->levels; }

int psx_gauss_tables(const psx_config* cfg, float* inc_filter, int* inc_span, float* inc_sigma,
                     float* dd_filter, int* dd_span, float* dd_sigma)
{
    if (!cfg || !inc_filter || !inc_span || !inc_sigma || !dd_filter || !dd_span || !dd_sigma)
        return PSX_ERR_INVALID;
    PsxGaussTables t{};
    const int rc = compute_tables(cfg, &t, nullptr);
    if (rc != PSX_OK) return rc;
    memcpy(inc_filter, t.inc_filter, sizeof(t.inc_filter)); memcpy(inc_span, t.inc_span, sizeof(t.inc_span));
    memcpy(inc_sigma, t.inc_sigma, sizeof(t.inc_sigma));
    memcpy(dd_filter, t.dd_filter, sizeof(t.dd_filter)); memcpy(dd_span, t.dd_span, sizeof(t.dd_span));
    memcpy(dd_sigma, t.dd_sigma, sizeof(t.dd_sigma));
    return PSX_OK;
}

// Config::setPrintGaussTables: what init_filter prints (gauss_filter.cu:146-161) and what its device-side
// print_gauss_filter_symbol<<<1,1>>>(10) prints (gauss_filter.cu:24-120), from the host tables.
int psx_print_gauss_tables(const psx_config* cfg, int columns)
{
    if (!cfg) return PSX_ERR_INVALID;
    PsxGaussTables t{};
    const int rc = compute_tables(cfg, &t, nullptr);
    if (rc != PSX_OK) return rc;
    compute_alt_tables(*cfg, &t);
    printf("\n"
           "Upscaling factor: %f (i.e. original image is scaled by a factor of %f)\n"
           "\n"
           "Sigma computations\n"
           "    Initial sigma is %f\n"
           "    Input blurriness is assumed to be %f (scaled to %f)\n",
           cfg->upscale_factor, pow(2.0f, cfg->upscale_factor), cfg->sigma, cfg->initial_blur,
           cfg->initial_blur * pow(2.0f, cfg->upscale_factor));
    const int stages = cfg->levels + 3;
    auto table = [&](int rows, const int* span, const float* sigma, const float* filter, bool split_sigma) {
        for (int lvl = 0; lvl < rows; lvl++) {
            if (split_sigma) { printf("      %d %d ", lvl, span[lvl] + span[lvl] - 1); printf("%2.6f: ", sigma[lvl]); }
            else             printf("      %d %d %2.6f: ", lvl, span[lvl] + span[lvl] - 1, sigma[lvl]);
            const int m = span[lvl] < columns ? span[lvl] : columns;
            for (int x = 0; x < m; x++) printf("%0.8f ", filter[lvl * PSX_GAUSS_ALIGN + x]);
            printf(m < span[lvl] ? "...\n" : "\n");
        }
    };
    printf("\nGauss tables\n      level span sigma : center value -> edge value\n    relative sigma\n");
    table(stages, t.inc_span, t.inc_sigma, t.inc_filter, true);
    printf("\n");
    printf("\nGauss tables for hardware interpolation\n"
           "      level span sigma : center value -> ( interpolation value, multiplier ) [one edge value] \n");
    table(stages, t.inc_ispan, t.inc_sigma, t.inc_ifilter, true);
    printf("\n");
    printf("\nGauss tables\n      level span sigma : center value -> edge value\n"
           "      absolute filters octave 0 (compute level 0, all other levels directly from level 0)\n");
    table(stages, t.abs0_span, t.abs0_sigma, t.abs0_filter, false);
    printf("\n      absolute filters other octaves\n      (level 0 via downscaling, all other levels directly from level 0)\n");
    table(stages, t.absN_span, t.absN_sigma, t.absN_filter, false);
    printf("\n");
    printf("    level 0-filters for direct downscaling\n");
    table(PSX_MAX_OCTAVES, t.dd_span, t.dd_sigma, t.dd_filter, false);
    printf("\n");
    fflush(stdout);
    return PSX_OK;
}

const char* psx_last_error(const psx_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int psx_create(int device, const psx_config* cfg, psx_ctx** out)
{
    psx_ctx* ctx = nullptr;   // PSX_HIP reports into g_create_error while ctx == nullptr
    if (!cfg || !out) return fail(nullptr, PSX_ERR_INVALID, "psx_create: null argument");
    *out = nullptr;
    psx_config c = *cfg;
    c.levels = imax(2, c.levels);                      // popsift.cpp:86
    if (c.gauss_mode < PSX_GAUSS_VLFEAT_COMPUTE || c.gauss_mode > PSX_GAUSS_FIXED15)
        return fail(nullptr, PSX_ERR_INVALID, "ERROR: The mode for computing Gauss filter scan is invalid");   // gauss_filter.cu:292-296
    if (c.scaling_mode != PSX_SCALE_DEFAULT && c.scaling_mode != PSX_SCALE_DIRECT)
        return fail(nullptr, PSX_ERR_INVALID, "invalid scaling mode");
    if (c.desc_mode < PSX_DESC_LOOP || c.desc_mode > PSX_DESC_NOTILE)
        return fail(nullptr, PSX_ERR_INVALID, "not yet");   // sift_desc.cu:80-82
    // make_octave exists for levels = 3 only (s_pyramid_fixed.cu:270-292)
    if ((c.gauss_mode == PSX_GAUSS_FIXED9 || c.gauss_mode == PSX_GAUSS_FIXED15) && c.levels != 3)
        return fail(nullptr, PSX_ERR_INVALID, "Unsupported number of levels for making all octaves at once");
    if (c.sift_mode != PSX_MODE_POPSIFT && c.sift_mode != PSX_MODE_OPENCV && c.sift_mode != PSX_MODE_VLFEAT)
        return fail(nullptr, PSX_ERR_INVALID, "invalid sift mode");
    if (c.max_extrema <= 0 || c.filter_grid_size <= 0)
        return fail(nullptr, PSX_ERR_INVALID, "invalid max_extrema / filter_grid_size");
    if (c.filter_max_extrema > 0 && c.filter_grid_size > 64)
        return fail(nullptr, PSX_ERR_INVALID, "filter_grid_size > 64 not supported by the HIP grid filter");
    if (c.grid_filter_mode != PSX_FILTER_RANDOM && c.grid_filter_mode != PSX_FILTER_LARGEST_FIRST &&
        c.grid_filter_mode != PSX_FILTER_SMALLEST_FIRST)
        return fail(nullptr, PSX_ERR_INVALID, "invalid grid_filter_mode");

    PSX_HIP(hipSetDevice(device));
    std::unique_ptr<psx_ctx> n(new (std::nothrow) psx_ctx());   // a failure below deletes the half-built context
    if (!n) return fail(nullptr, PSX_ERR_NOMEM, "out of host memory");
    n->device = device;
    n->cfg = c;
    {
        std::string bad;
        n->tune = psx_tuning_from_env(&bad);
        if (!bad.empty()) return fail(nullptr, PSX_ERR_INVALID, bad);
    }
    if (hipDeviceGetAttribute(&n->tune.cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || n->tune.cus <= 0) n->tune.cus = 256;
    n->resident_blocks = 4 * n->tune.cus;
    // opt-in: measured on MI355X / ROCm 7.2 the replayed graph is not faster than the 36 stream launches
    // (single frame 0.63 vs 0.63 ms, throughput equal): kernel-to-kernel dependencies cost the same either way
    n->graph.off = !n->tune.hip_graph;
    std::string why;
    int rc = compute_tables(&n->cfg, &n->tab, &why);
    if (rc != PSX_OK) return fail(nullptr, rc, why);
    compute_alt_tables(n->cfg, &n->tab);
    n->alt_pyramid = !(c.scaling_mode == PSX_SCALE_DEFAULT &&
                       (c.gauss_mode == PSX_GAUSS_VLFEAT_COMPUTE || c.gauss_mode == PSX_GAUSS_OPENCV_COMPUTE));
    {
        // POPSIFT_CU_PARTITIONS=P (measurement switch, default off): the contexts of a process take turns over P partitions of
        // the chip, each context's stream masked to its partition.  POPSIFT_CU_PARTITION_MODE: 0 = by XCD (mask bit b belongs to
        // XCD b % 8: partition = a set of whole XCDs with their own L2s), 1 = a slice of the CUs of every XCD.
        const int parts = n->tune.cu_partitions, pmode = n->tune.cu_partition_mode, cus = n->tune.cus;
        static std::atomic<int> next_part{0};
        if (parts > 0 && cus >= 64) {
            const int part = next_part.fetch_add(1) % parts;
            uint32_t mask[16] = {0};
            const int nbits = cus < 512 ? cus : 512;
            for (int b = 0; b < nbits; b++) {
                const int xcd = b % 8, cu = b / 8;
                const bool mine = pmode == 0 ? (xcd * parts / 8 == part) : (cu % parts == part);
                if (mine) mask[b / 32] |= 1u << (b % 32);
            }
            PSX_HIP(hipExtStreamCreateWithCUMask(&n->stream.h, (uint32_t)((nbits + 31) / 32), mask));
        } else
            PSX_HIP(hipStreamCreateWithFlags(&n->stream.h, hipStreamNonBlocking));
    }
    PSX_HIP(n->d_params.grow(1));
    PSX_HIP(n->h_params_pin.grow(1));
    // frame counters and the candidate sub-list counters in ONE allocation: one fill kernel clears both per frame
    static_assert(sizeof(PsxCounters) <= CNT_BLOCK, "PsxCounters outgrew its slot");
    // layout: [PsxCounters | flow state (flow.bytes, set per size) | candidate counters]; the per-frame fill covers the
    // used prefix of it
    PSX_HIP(n->d_cnt_block.grow(CNT_BLOCK + FLOW_MAX_BYTES + CAND_CT_BYTES));
    n->d_cnt = reinterpret_cast<PsxCounters*>(n->d_cnt_block.p);
    n->d_cand_ct = reinterpret_cast<int*>(n->d_cnt_block.p + CNT_BLOCK);
    PSX_HIP(n->h_cnt.grow(1));
    PSX_HIP(hipMemset(n->d_cnt, 0, CNT_BLOCK + FLOW_MAX_BYTES + CAND_CT_BYTES));
    PSX_HIP(n->xp.counts.grow(4));
    n->xp.counts[0] = n->xp.counts[1] = n->xp.counts[2] = n->xp.counts[3] = 0;
    for (int i = 0; i < 5; i++) PSX_HIP(n->tm.ev[i].get(hipEventDefault));
    PSX_HIP(n->tm.t0.get(hipEventDefault));
    PSX_HIP(n->tm.t1.get(hipEventDefault));
    *out = n.release();
    return PSX_OK;
}

int psx_destroy(psx_ctx* ctx)
{
    if (!ctx) return PSX_OK;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    delete ctx;
    return PSX_OK;
}

int psx_resize(psx_ctx* ctx, int w, int h)
{
    if (!ctx) return PSX_ERR_INVALID;
    if (w <= 0 || h <= 0) return fail(ctx, PSX_ERR_INVALID, "psx_resize: non-positive image size");
    if (w == ctx->in_w && h == ctx->in_h && ctx->d_pyr) return PSX_OK;
    PSX_HIP(hipSetDevice(ctx->device));
    PSX_HIP(hipStreamSynchronize(ctx->stream));
    drop_graph(ctx);

    const psx_config& c = ctx->cfg;
    // PopSift::private_apply_scale_factor, popsift.cpp:109-126
    const float scaleFactor = 1.0f / powf(2.0f, -c.upscale_factor);
    if (ctx->octaves_resolved < 0) {
        if (c.octaves < 0)
            ctx->octaves_resolved = imax((int)(floorf(logf((float)imin(w, h)) / logf(2.0f)) - 3.0f + scaleFactor), 1);
        else
            ctx->octaves_resolved = c.octaves;
        ctx->octaves_resolved = imin(imax(ctx->octaves_resolved, 1), PSX_MAX_OCTAVES);
    }
    int ow = (int)ceilf(w * scaleFactor);
    int oh = (int)ceilf(h * scaleFactor);
    if (ow <= 0 || oh <= 0) return fail(ctx, PSX_ERR_INVALID, "psx_resize: scaled image is empty");
    // kernels address a plane (and the padded resampled input) with 32-bit byte offsets from its base
    if (((size_t)((ow + 63) & ~63) + 2 * PSX_LEVEL0_PAD) * (size_t)oh * sizeof(float) >= ((size_t)1 << 32))
        return fail(ctx, PSX_ERR_INVALID, "psx_resize: octave 0 plane of 4 GiB or more is not supported");
    // extremum candidates are packed as y << 32 | z << 24 | x
    if (ow >= (1 << 24)) return fail(ctx, PSX_ERR_INVALID, "psx_resize: octave 0 wider than 2^24 - 1 columns is not supported");

    PsxParams& P = ctx->hp;
    memset(&P, 0, sizeof(P));
    P.num_octaves = ctx->octaves_resolved;
    P.levels = c.levels;
    P.L = c.levels + 3;
    P.sift_mode = c.sift_mode;
    P.norm_mode = c.norm_mode;
    P.norm_multi = c.norm_multi;
    P.max_extrema = c.max_extrema;
    P.grid_size = c.filter_grid_size;
    P.up_fac = (int)c.upscale_factor;
    P.sigma0 = c.sigma;
    P.sigma_k = powf(2.0f, 1.0f / c.levels);            // sift_constants.cu:27
    P.threshold = psx_peak_threshold(&c);
    P.edge_limit = c.edge_limit;

    size_t total = 0;
    size_t offs[PSX_MAX_OCTAVES];
    for (int o = 0; o < P.num_octaves; o++) {
        PsxOctave& oc = P.oct[o];
        oc.w = ow; oc.h = oh;
        oc.pitch = (ow + 63) & ~63;
        oc.plane = (size_t)oc.pitch * oh;
        offs[o] = total;
        total += oc.plane * P.L;
        P.w_grid_div[o] = float(ow) / c.filter_grid_size;   // sift_octave.cu:40-41
        P.h_grid_div[o] = float(oh) / c.filter_grid_size;
        ow = (int)ceilf(ow / 2.0f);                          // sift_pyramid.cu:132-133
        oh = (int)ceilf(oh / 2.0f);
    }
    total += 64;   // slack: vector loads never run past the last plane
    PSX_HIP(ctx->d_pyr.grow(total));
    ctx->up_pitch = ((P.oct[0].w + 63) / 64) * 64 + 2 * PSX_LEVEL0_PAD;
    PSX_HIP(ctx->d_up.grow((size_t)ctx->up_pitch * P.oct[0].h));
    for (int o = 0; o < P.num_octaves; o++) P.oct[o].data = ctx->d_pyr + offs[o];
    if (ctx->alt_pyramid) {
        PSX_HIP(ctx->d_intm.grow(P.oct[0].plane + 64));
        PSX_HIP(ctx->d_vbuf.grow((size_t)(P.oct[0].pitch + 64) * P.oct[0].h));
    }

    // Extrema buffers are sized for the worst case (max_extrema per octave, 100 B per entry); the descriptor
    // buffers start at the reference's size, max(2 max_extrema, 1.25 max_extrema) entries of 512 B
    // (sift_pyramid.cu:186-209), never shrink, and grow after the counter read-back when a frame needed more
    // (regrow_descriptors below; the reference reallocates in Pyramid::reallocExtrema the same way).
    const size_t iext_need = (size_t)P.num_octaves * c.max_extrema;
    const size_t ori_floor = (size_t)imax(2 * c.max_extrema, c.max_extrema + c.max_extrema / 4);
    const size_t ori_need = ctx->d_desc.cap / 128 > ori_floor ? ctx->d_desc.cap / 128 : ori_floor;
    PSX_HIP(ctx->d_iext.grow(iext_need));
    PSX_HIP(ctx->d_iext_off.grow(iext_need));
    // candidates before refinement: ~1.3x the survivors on natural images; room for 4x the cap per octave,
    // split over PSX_CAND_SUB sub-lists; a candidate that finds its sub-list full is refined in place
    // k_pyramid_flow: work list of this size (default pyramid modes only), and where the candidate counters start behind
    // its ticket words and chunk counters
    ctx->flow.on = false; ctx->flow.bytes = 0;
    if (!ctx->alt_pyramid && ctx->tune.flow != 0) {
        PsxFlowPlan plan{};
        const int first = ctx->tune.flow == 2 ? 1 : 0;
        if (first < P.num_octaves && psx_flow_plan(ctx->tune, P, ctx->tab.inc_filter, ctx->tab.inc_span, first, ctx->resident_blocks, ctx->tune.flow_order, &plan)) {
            bool ok = ctx->flow.jobs.grow((size_t)plan.njobs) == hipSuccess && ctx->flow.items.grow((size_t)plan.nitems) == hipSuccess;
            ok = ok && hipMemcpy(ctx->flow.jobs, plan.jobs, sizeof(PsxFlowJob) * (size_t)plan.njobs, hipMemcpyHostToDevice) == hipSuccess &&
                       hipMemcpy(ctx->flow.items, plan.items, sizeof(PsxFlowItem) * (size_t)plan.nitems, hipMemcpyHostToDevice) == hipSuccess;
            if (ok) {
                ctx->flow.on = true; ctx->flow.first = first; ctx->flow.nitems = plan.nitems; ctx->flow.grid = plan.grid;
                ctx->flow.ncnt = plan.ncounters; ctx->flow.njobs = plan.njobs;
                ctx->flow.bytes = sizeof(int) * ((size_t)PSX_FLOW_HEAD_INTS + (size_t)plan.ncounters * PSX_FLOW_CNT_STRIDE);
                double by = 0.0;
                for (int q = 0; q < plan.njobs; q++) {
                    by += 8.0 * (double)plan.jobs[q].W * plan.jobs[q].H;
                    if (plan.jobs[q].half_dst) by += 4.0 * (double)((plan.jobs[q].W + 1) / 2) * ((plan.jobs[q].H + 1) / 2);
                }
                ctx->flow.algo_bytes = by;
            }
            free(plan.jobs); free(plan.items);
            if (!ok) return fail(ctx, PSX_ERR_HIP, "psx_resize: could not upload the pyramid work list");
        }
    }
    { const int trc = plan_tiles(ctx); if (trc != PSX_OK) return trc; }
    psx_pyramid_steps(P, ctx->tab.inc_span, ctx->tune, ctx->resident_blocks, PSX_PLAN_DIAGONAL, 0, 0, ctx->plan_diagonal);
    ctx->plan_own.clear();
    if (ctx->flow.on) psx_pyramid_steps(P, ctx->tab.inc_span, ctx->tune, ctx->resident_blocks, PSX_PLAN_FLOW, ctx->flow.first, 0, ctx->plan_own);
    else if (ctx->tile.on)
        psx_pyramid_steps(P, ctx->tab.inc_span, ctx->tune, ctx->resident_blocks, PSX_PLAN_TILE, ctx->tile.first, (int)ctx->tile.launches.size(), ctx->plan_own);
    ctx->d_cand_ct = reinterpret_cast<int*>(reinterpret_cast<char*>(ctx->d_cnt) + CNT_BLOCK + ctx->flow.bytes);
    P.cand_capacity = (4 * c.max_extrema + PSX_CAND_SUB - 1) / PSX_CAND_SUB;
    PSX_HIP(ctx->d_cand.grow((size_t)P.num_octaves * PSX_CAND_SUB * P.cand_capacity));
    P.cand_ct = ctx->d_cand_ct;
    PSX_HIP(ctx->d_extrema.grow(iext_need));
    PSX_HIP(ctx->d_features.grow(iext_need));
    PSX_HIP(ctx->d_desc.grow(ori_need * 128));
    if (ctx->desc_fmt == PSX_DESCFMT_U8) PSX_HIP(ctx->d_desc_u8.grow(ctx->d_desc.cap));
    PSX_HIP(ctx->d_feat_to_ext.grow(ori_need));
    PSX_HIP(ctx->d_ext_nori.grow(iext_need + 64));
    for (int o = 0; o < P.num_octaves; o++) {
        P.iext[o] = ctx->d_iext + (size_t)o * c.max_extrema;
        P.iext_off[o] = ctx->d_iext_off + (size_t)o * c.max_extrema;
        P.cand[o] = ctx->d_cand + (size_t)o * PSX_CAND_SUB * P.cand_capacity;
    }
    P.ext_capacity = (int)iext_need;
    P.ori_capacity = (int)ori_need;
    P.extrema = ctx->d_extrema;
    P.features = ctx->d_features;
    P.desc = ctx->d_desc;
    P.feat_to_ext = ctx->d_feat_to_ext;
    P.ext_nori = ctx->d_ext_nori;

    PSX_HIP(hipMemcpy(ctx->d_params, &P, sizeof(P), hipMemcpyHostToDevice));
    ctx->in_w = w; ctx->in_h = h;
    ctx->counts_valid = false;
    ctx->pyr_ready = false;
    return PSX_OK;
}

int psx_num_octaves(const psx_ctx* ctx) { return ctx ? ctx->hp.num_octaves : 0; }
int psx_num_levels(const psx_ctx* ctx) { return ctx ? ctx->hp.L : 0; }
int psx_octave_dims(const psx_ctx* ctx, int o, int* w, int* h)
{
    if (!ctx || o < 0 || o >= ctx->hp.num_octaves) return PSX_ERR_INVALID;
    if (w) *w = ctx->hp.oct[o].w;
    if (h) *h = ctx->hp.oct[o].h;
    return PSX_OK;
}

static int upload_common(psx_ctx* ctx, const void* host, int w, int h, int is_float, bool known_pinned = false)
{
    if (!ctx || !host) return PSX_ERR_INVALID;
    int rc = psx_resize(ctx, w, h);
    if (rc != PSX_OK) return rc;
    PSX_HIP(hipSetDevice(ctx->device));
    const size_t bytes = (size_t)w * h * (is_float ? 4 : 1);
    Staged<unsigned char>& in = ctx->input_own;
    PSX_HIP(in.reserve(bytes, bytes, 64, ctx->stream));               // 64 bytes of slack behind the image
    const bool dma = !(ctx->tune.null_device_work == 2 && ctx->nulldev.primed);       // PSX_NULL_DEVICE_WORK=2: host software only, no DMA
    hipPointerAttribute_t attr;
    // DMA engine, not a kernel: a copy kernel that reads the mapped host image over PCIe itself was measured
    // (GPU-initiated reads are slow: +0.8 ms per frame in flight, -8 % end-to-end throughput).
    // hipPointerGetAttributes costs ~0.2 ms per call in a process with many mappings: callers that KNOW their
    // buffer is pinned (psx_host_alloc) say so
    if (!known_pinned && (hipPointerGetAttributes(&attr, host) != hipSuccess || attr.type == hipMemoryTypeUnregistered)) {
        (void)hipGetLastError();
        PSX_HIP(in.push(static_cast<const unsigned char*>(host), bytes, bytes, bytes, ctx->stream, 64, dma));
    } else if (dma)
        PSX_HIP(hipMemcpyAsync(in.dev, host, bytes, hipMemcpyHostToDevice, ctx->stream));
    ctx->d_input = in.dev;
    ctx->input_is_float = is_float;
    ctx->pyr_ready = false;
    return PSX_OK;
}

int psx_upload_u8(psx_ctx* ctx, const uint8_t* host, int w, int h) { return upload_common(ctx, host, w, h, 0); }
int psx_upload_f32(psx_ctx* ctx, const float* host, int w, int h) { return upload_common(ctx, host, w, h, 1); }
int psx_upload_pinned(psx_ctx* ctx, const void* pinned_host, int w, int h, int is_float)
{
    return upload_common(ctx, pinned_host, w, h, is_float ? 1 : 0, true);
}

int psx_set_input_dev(psx_ctx* ctx, const void* dev_ptr, int w, int h, int is_float)
{
    if (!ctx || !dev_ptr) return PSX_ERR_INVALID;
    int rc = psx_resize(ctx, w, h);
    if (rc != PSX_OK) return rc;
    ctx->d_input = dev_ptr;
    ctx->input_is_float = is_float ? 1 : 0;
    ctx->pyr_ready = false;
    return PSX_OK;
}

static PsxBlurJob blur_job(const psx_ctx* ctx, int o, int level)
{
    const PsxParams& P = ctx->hp;
    const PsxOctave& oc = P.oct[o];
    PsxBlurJob j;
    j.src = oc.data + (size_t)(level - 1) * oc.plane;
    j.dst = oc.data + (size_t)level * oc.plane;
    j.half_dst = nullptr; j.half_pitch = 0;
    if (level == P.L - 3 && o + 1 < P.num_octaves) {      // PREV_LEVEL 3, s_pyramid_build.cu:21,228
        j.half_dst = P.oct[o + 1].data;
        j.half_pitch = P.oct[o + 1].pitch;
    }
    j.W = oc.w; j.H = oc.h; j.pitch = oc.pitch;
    j.taps = taps_from(ctx->tab.inc_filter + level * PSX_GAUSS_ALIGN);
    j.span = ctx->tab.inc_span[level];
    return j;
}

static int launch_blur_level(psx_ctx* ctx, int o, int level, hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr)
{
    const PsxBlurJob j = blur_job(ctx, o, level);
    PSX_HIP(psx_launch_blur(ctx->tune, j.src, j.dst, j.W, j.H, j.pitch, j.taps, j.span, j.half_dst, j.half_pitch, ctx->stream, ev0, ev1));
    return PSX_OK;
}

// the plan of the schedule in force: with the blur probe on, a tile schedule that would take octave 0 steps aside for the
// diagonal one (the probe times octave 0's launches level by level)
static const PsxPlan& frame_plan(const psx_ctx* ctx)
{
    const bool own = ctx->flow.on || (ctx->tile.on && !(ctx->tm.probe && ctx->tile.first == 0));
    return own ? ctx->plan_own : ctx->plan_diagonal;
}

// One step of the frame's plan.  With the blur probe on, a blur launch whose (first) plane is a level of octave 0 is
// bracketed by that level's events and adds its algorithmic bytes (8 B per pixel of every plane it blurs) to *probe_bytes,
// the flow launch is bracketed when it carries octave 0, and octave 0's own scan launch by ev_x[2] / ev_x[3].
static int issue_step(psx_ctx* ctx, const psx_step& s, double* probe_bytes)
{
    const PsxParams& P = ctx->hp;
    const bool probe = ctx->tm.probe;
    switch (s.kind) {
    case PSX_STEP_BLUR:
    case PSX_STEP_BLUR2: {
        const bool pl = probe && s.a == 0;
        hipEvent_t e0 = pl ? ctx->tm.ev_blur[2 * (s.b - 1)].h : nullptr, e1 = pl ? ctx->tm.ev_blur[2 * (s.b - 1) + 1].h : nullptr;
        if (s.kind == PSX_STEP_BLUR) { const int rc = launch_blur_level(ctx, s.a, s.b, e0, e1); if (rc != PSX_OK) return rc; }
        else PSX_HIP(psx_launch_blur2(ctx->tune, blur_job(ctx, s.a, s.b), blur_job(ctx, s.c, s.d), ctx->stream, e0, e1));
        if (pl) *probe_bytes += 8.0 * ((double)P.oct[s.a].w * P.oct[s.a].h + (s.kind == PSX_STEP_BLUR2 ? (double)P.oct[s.c].w * P.oct[s.c].h : 0.0));
        return PSX_OK;
    }
    case PSX_STEP_TILE: {
        const psx_ctx::TileLaunch& ln = ctx->tile.launches[(size_t)s.a];
        PSX_HIP(psx_launch_blur_tile(ctx->tile.jobs + ln.job0, ln.njobs, ln.grid, ln.lds, ctx->tune.tile_nt, ctx->stream));
        return PSX_OK;
    }
    case PSX_STEP_FLOW: {
        const bool pf = probe && ctx->flow.first == 0;
        int* state = reinterpret_cast<int*>(reinterpret_cast<char*>(ctx->d_cnt) + CNT_BLOCK);
        PSX_HIP(psx_launch_flow(ctx->tune, ctx->flow.jobs, ctx->flow.items, ctx->flow.nitems, state, &ctx->d_cnt->flow_error,
                                ctx->flow.grid, ctx->tune.flow_ld, ctx->stream, pf ? ctx->tm.ev_blur[0].h : nullptr, pf ? ctx->tm.ev_blur[1].h : nullptr,
                                ctx->flow.trace));
        return PSX_OK;
    }
    case PSX_STEP_SCAN: {
        const bool px = probe && s.a == 0;
        if (px) PSX_HIP(hipEventRecord(ctx->tm.ev_x[2].h, ctx->stream));
        PSX_HIP(psx_launch_extrema(ctx->d_params, ctx->hp, ctx->d_cnt, s.a, mask_of(ctx), ctx->stream));
        if (px) { PSX_HIP(hipEventRecord(ctx->tm.ev_x[3].h, ctx->stream)); ctx->tm.probe_ext0 = true; }
        return PSX_OK;
    }
    case PSX_STEP_SCAN_SET: {
        const int octaves[PSX_EXT_BATCH] = {s.a, s.b, s.c, s.d};
        PSX_HIP(psx_launch_extrema_batch(ctx->d_params, ctx->hp, ctx->d_cnt, octaves, s.n, mask_of(ctx), ctx->stream));
        return PSX_OK;
    }
    }
    return fail(ctx, PSX_ERR_STATE, "issue_step: unknown step kind");
}

int psx_build_pyramid(psx_ctx* ctx)
{
    if (!ctx) return PSX_ERR_INVALID;
    if (!ctx->d_input || !ctx->d_pyr) return fail(ctx, PSX_ERR_STATE, "psx_build_pyramid: no input image");
    PSX_HIP(hipSetDevice(ctx->device));
    const PsxParams& P = ctx->hp;
    const psx_config& c = ctx->cfg;
    const bool probe = ctx->tm.probe;
    ctx->counts_valid = false;
    ctx->pyr_ready = true; ctx->kp.results = false;
    ctx->ext_launched = false;
    if (ctx->tm.on) PSX_HIP(hipEventRecord(ctx->tm.ev[0].h, ctx->stream));
    // Pyramid::reset_extrema_mgmt, sift_pyramid.cu:364-371
    PSX_HIP(hipMemsetAsync(ctx->d_cnt, 0, CNT_BLOCK + ctx->flow.bytes + sizeof(int) * (size_t)P.num_octaves * PSX_CAND_SUB * 32, ctx->stream));

    // the scans go out with the pyramid in psx_extract, except behind the flow kernel: there psx_find_extrema issues them
    const bool scans = ctx->interleave && !ctx->flow.on;
    if (ctx->alt_pyramid) {
        PsxAltArgs q;
        q.tune = &ctx->tune; q.hp = &ctx->hp;
        q.img = ctx->d_input; q.w = ctx->in_w; q.h = ctx->in_h; q.is_float = ctx->input_is_float;
        q.gauss_mode = c.gauss_mode; q.scaling_mode = c.scaling_mode; q.sift_mode = c.sift_mode;
        q.upscale_factor = c.upscale_factor;
        q.tab = &ctx->tab;
        q.up = ctx->d_up; q.up_pitch = ctx->up_pitch;
        q.intm = ctx->d_intm; q.vbuf = ctx->d_vbuf; q.vbuf_pitch = P.oct[0].pitch + 64;
        q.user = ctx;
        q.after_octave = scans ? +[](void* u, int o) -> hipError_t {
            psx_ctx* cx = static_cast<psx_ctx*>(u);
            return psx_launch_extrema(cx->d_params, cx->hp, cx->d_cnt, o, mask_of(cx), cx->stream);
        } : nullptr;
        int probe_hit = 0;
        if (probe) { q.probe_ev0 = ctx->tm.ev_blur[0].h; q.probe_ev1 = ctx->tm.ev_blur[1].h; q.probe_hit = &probe_hit; ctx->tm.probe_n = 0; }
        const hipError_t e = psx_launch_pyramid_alt(q, ctx->stream);
        if (probe_hit) {
            // Fixed9 / Fixed15: the one-kernel octave 0 (six planes written from the input image: 24 B per pixel + the image)
            ctx->tm.probe_n = 1;
            ctx->tm.probe_bytes = 24.0 * (double)P.oct[0].w * P.oct[0].h + (double)ctx->in_w * ctx->in_h * (ctx->input_is_float ? 4 : 1);
        }
        if (e == hipErrorInvalidValue) return fail(ctx, PSX_ERR_INVALID, "Unsupported number of levels for making all octaves at once");
        PSX_HIP(e);
    } else {
        PsxLevel0Args a;
        a.img = ctx->d_input; a.w = ctx->in_w; a.h = ctx->in_h; a.is_float = ctx->input_is_float;
        a.dst = P.oct[0].data; a.W = P.oct[0].w; a.H = P.oct[0].h; a.pitch = P.oct[0].pitch;
        a.tmp = ctx->d_up; a.tmp_pitch = ctx->up_pitch;
        a.shift = 0.5f;                                                    // s_pyramid_build.cu:109-114
        if (c.sift_mode == PSX_MODE_POPSIFT || c.sift_mode == PSX_MODE_VLFEAT)
            a.shift = 0.5f * powf(2.0f, c.upscale_factor - 0);
        a.taps_h = taps_from(ctx->tab.dd_filter); a.span_h = ctx->tab.dd_span[0];
        a.taps_v = taps_from(ctx->tab.inc_filter); a.span_v = ctx->tab.inc_span[0];
        if (probe) PSX_HIP(hipEventRecord(ctx->tm.ev_x[0].h, ctx->stream));
        PSX_HIP(psx_launch_level0(ctx->tune, a, ctx->stream));
        if (probe) PSX_HIP(hipEventRecord(ctx->tm.ev_x[1].h, ctx->stream));

        double probe_bytes = 0.0;
        for (const psx_step& s : frame_plan(ctx)) {
            if (psx_step_is_scan(s) && !scans) continue;
            const int rc = issue_step(ctx, s, &probe_bytes);
            if (rc != PSX_OK) return rc;
        }
        // octave 0's L - 1 launches, timed one by one; or the one flow launch that carries octave 0
        const bool pf = ctx->flow.on && ctx->flow.first == 0;
        if (probe) { ctx->tm.probe_n = pf ? 1 : P.L - 1; ctx->tm.probe_bytes = pf ? ctx->flow.algo_bytes : probe_bytes / (P.L - 1); }
    }
    ctx->ext_launched = scans;
    if (ctx->tm.on) PSX_HIP(hipEventRecord(ctx->tm.ev[1].h, ctx->stream));
    return PSX_OK;
}

static int wait_stream(psx_ctx* ctx)
{
    if (ctx->blocking_wait) {
        // The C++ pipeline's workers wait here for most of a frame's life.  hipEventSynchronize on a hipEventBlockingSync
        // event still burnt the core on this stack (POPSIFT_PROFILE: 2.4 ms of thread CPU time per 0.35 ms frame, 8 workers
        // 86 % busy -- 7 cores per GPU, 54 on an 8-GPU host); asking the event and sleeping in between costs a few
        // microseconds of CPU per frame and, with several frames in flight per worker pool, no throughput.
        // POPSIFT_WAIT_SLEEP_US (default 40; 0 = the runtime's blocking wait).
        const int sleep_us = ctx->tune.wait_sleep_us;
        PSX_HIP(ctx->ev_wait.get(hipEventBlockingSync | hipEventDisableTiming));
        PSX_HIP(hipEventRecord(ctx->ev_wait, ctx->stream));
        if (sleep_us == 0) { PSX_HIP(hipEventSynchronize(ctx->ev_wait)); return PSX_OK; }
        for (;;) {
            const hipError_t q = hipEventQuery(ctx->ev_wait);
            if (q == hipSuccess) return PSX_OK;
            if (q != hipErrorNotReady) PSX_HIP(q);
            struct timespec ts = {0, (long)sleep_us * 1000L};
            nanosleep(&ts, nullptr);
        }
    }
    PSX_HIP(hipStreamSynchronize(ctx->stream));
    return PSX_OK;
}

// Pyramid::extrema_filter_grid (s_filtergrid.cu:113-325), gated as in s_orientation.cu:378-383.
// Like the reference, the host reads the per-octave counts once to decide and to size the sort.
static int grid_filter(psx_ctx* ctx)
{
    PSX_HIP(hipMemcpyAsync(ctx->h_cnt, ctx->d_cnt, sizeof(PsxCounters), hipMemcpyDeviceToHost, ctx->stream));
    { int wrc = wait_stream(ctx); if (wrc != PSX_OK) return wrc; }
    int total = 0;
    for (int o = 0; o < ctx->hp.num_octaves; o++) total += imin(ctx->h_cnt->ext_ct[o], ctx->cfg.max_extrema);
    const int fmax = ctx->cfg.filter_max_extrema;
    if (!((int)(fmax * 1.1) < total)) return PSX_OK;

    size_t temp_bytes = 0;
    PSX_HIP(psx_gridfilter_sort_bytes(total, &temp_bytes));
    PSX_HIP(ctx->d_gf_keys.grow(2 * (size_t)total));
    PSX_HIP(ctx->d_gf_vals.grow(2 * (size_t)total));
    PSX_HIP(ctx->d_gf_temp.grow(temp_bytes + 256));
    PSX_HIP(ctx->d_gf_scratch.grow(psx_gridfilter_scratch_ints(ctx->cfg.filter_grid_size)));
    PSX_HIP(psx_launch_gridfilter(ctx->d_params, ctx->d_cnt, ctx->cfg.grid_filter_mode, total, fmax,
                                  ctx->d_gf_keys, ctx->d_gf_keys + total, ctx->d_gf_vals,
                                  ctx->d_gf_vals + total, ctx->d_gf_temp, temp_bytes, ctx->d_gf_scratch,
                                  ctx->stream));
    ctx->filtered = true;
    ctx->counts_valid = false;
    return PSX_OK;
}

int psx_find_extrema(psx_ctx* ctx)
{
    if (!ctx) return PSX_ERR_INVALID;
    if (!ctx->d_pyr) return fail(ctx, PSX_ERR_STATE, "psx_find_extrema: no pyramid");
    { const int mrc = check_mask(ctx, "psx_find_extrema"); if (mrc != PSX_OK) return mrc; }
    PSX_HIP(hipSetDevice(ctx->device));
    if (!ctx->ext_launched)                              // the scans did not go out with the pyramid: the plan's scan steps, in its order
        for (const psx_step& s : frame_plan(ctx)) {
            if (!psx_step_is_scan(s)) continue;
            const int rc = issue_step(ctx, s, nullptr);
            if (rc != PSX_OK) return rc;
        }
    ctx->ext_launched = false;
    PSX_HIP(psx_launch_refine(ctx->d_params, ctx->hp, ctx->d_cnt, mask_of(ctx), ctx->stream));
    ctx->filtered = false;
    if (ctx->tm.on) PSX_HIP(hipEventRecord(ctx->tm.ev[2].h, ctx->stream));
    return PSX_OK;
}

int psx_orientation(psx_ctx* ctx)
{
    if (!ctx) return PSX_ERR_INVALID;
    if (!ctx->d_pyr) return fail(ctx, PSX_ERR_STATE, "psx_orientation: no pyramid");
    PSX_HIP(hipSetDevice(ctx->device));
    if (ctx->cfg.filter_max_extrema > 0 && !ctx->filtered) {
        int rc = grid_filter(ctx);
        if (rc != PSX_OK) return rc;
    }
    PSX_HIP(psx_launch_orientation(ctx->tune, ctx->d_params, ctx->d_cnt, ctx->stream));
    snapshot_export(ctx);
    PSX_HIP(psx_launch_scan(ctx->d_params, ctx->d_cnt, ctx->xp.fx, ctx->stream));
    if (ctx->tm.on) PSX_HIP(hipEventRecord(ctx->tm.ev[3].h, ctx->stream));
    return PSX_OK;
}

// the descriptor kernel of the configured mode, with the export targets of the frame in flight
static int launch_descriptor_stage(psx_ctx* ctx)
{
    if (ctx->cfg.desc_mode == PSX_DESC_LOOP)
        PSX_HIP(psx_launch_descriptors(ctx->tune, ctx->d_params, ctx->d_cnt, ctx->xp.fx, ctx->stream));
    else
        PSX_HIP(psx_launch_descriptors_alt(ctx->tune, ctx->d_params, ctx->d_cnt, ctx->cfg.desc_mode, ctx->xp.fx, ctx->stream));
    return PSX_OK;
}

int psx_descriptors(psx_ctx* ctx)
{
    if (!ctx) return PSX_ERR_INVALID;
    if (!ctx->d_pyr) return fail(ctx, PSX_ERR_STATE, "psx_descriptors: no pyramid");
    PSX_HIP(hipSetDevice(ctx->device));
    { const int rc = launch_descriptor_stage(ctx); if (rc != PSX_OK) return rc; }
    if (ctx->tm.on) PSX_HIP(hipEventRecord(ctx->tm.ev[4].h, ctx->stream));
    return PSX_OK;
}

static int extract_chain(psx_ctx* ctx)
{
    int rc;
    ctx->interleave = !ctx->tm.on;        // per-stage timers need the stages back to back
    rc = psx_build_pyramid(ctx);
    ctx->interleave = false;
    if (rc != PSX_OK) return rc;
    if ((rc = psx_find_extrema(ctx)) != PSX_OK) return rc;
    if ((rc = psx_orientation(ctx)) != PSX_OK) return rc;
    return psx_descriptors(ctx);
}

int psx_extract(psx_ctx* ctx)
{
    if (!ctx) return PSX_ERR_INVALID;
    if (!ctx->d_input || !ctx->d_pyr) return fail(ctx, PSX_ERR_STATE, "psx_extract: no input image");
    { const int mrc = check_mask(ctx, "psx_extract"); if (mrc != PSX_OK) return mrc; }
    if (ctx->tune.null_device_work != 0) {
        if (ctx->nulldev.primed) {                    // measurement: no kernels; the first frame's results stand in
            if (ctx->tune.null_device_work == 1) ctx->counts_valid = false;      // mode 1 reads the counters back per frame, like a real frame
            snapshot_export(ctx);
            return PSX_OK;
        }
        ctx->nulldev.primed = true;
    }
    // Optionally replay the 36-launch chain as one hipGraph (POPSIFT_HIP_GRAPH=1).  Not with the grid filter
    // (it reads counters on the host in mid-chain) and not with the per-stage timers.
    const bool use_graph = !ctx->graph.off && !ctx->tm.on && !ctx->tm.probe && ctx->cfg.filter_max_extrema <= 0;
    if (!use_graph) return extract_chain(ctx);
    PSX_HIP(hipSetDevice(ctx->device));
    if (ctx->graph.exec.h && (ctx->graph.input != ctx->d_input || ctx->graph.is_float != ctx->input_is_float ||
                       ctx->graph.w != ctx->in_w || ctx->graph.h != ctx->in_h || ctx->graph.mask != ctx->mask.data))
        drop_graph(ctx);
    if (!ctx->graph.exec.h) {
        hipGraph_t g = nullptr;
        if (hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal) != hipSuccess) {
            ctx->graph.off = true;
            return extract_chain(ctx);
        }
        const int rc = extract_chain(ctx);
        const hipError_t e = hipStreamEndCapture(ctx->stream, &g);
        if (rc != PSX_OK || e != hipSuccess || g == nullptr ||
            hipGraphInstantiate(&ctx->graph.exec.h, g, nullptr, nullptr, 0) != hipSuccess) {
            if (g) (void)hipGraphDestroy(g);
            ctx->graph.exec.h = nullptr;
            ctx->graph.off = true;
            (void)hipGetLastError();
            return rc != PSX_OK ? rc : extract_chain(ctx);
        }
        (void)hipGraphDestroy(g);
        ctx->graph.input = ctx->d_input; ctx->graph.is_float = ctx->input_is_float;
        ctx->graph.w = ctx->in_w; ctx->graph.h = ctx->in_h;
        ctx->graph.mask = ctx->mask.data;
    }
    ctx->counts_valid = false;
    ctx->filtered = false;
    ctx->pyr_ready = true; ctx->kp.results = false;
    snapshot_export(ctx);             // the captured kernels carry the targets attached at capture time; attach drops the graph
    PSX_HIP(hipGraphLaunch(ctx->graph.exec.h, ctx->stream));
    return PSX_OK;
}

static int fetch_counts(psx_ctx* ctx);

// ---- caller-supplied keypoints (keypoints.hip) --------------------------------------------------------------------------

static int set_keypoints_common(psx_ctx* ctx, const psx_keypoint* p, int n, bool on_device)
{
    if (!ctx) return PSX_ERR_INVALID;
    if (n < 0 || (n > 0 && !p)) return fail(ctx, PSX_ERR_INVALID, "psx_set_keypoints: bad list");
    if (!ctx->d_input || !ctx->d_pyr) return fail(ctx, PSX_ERR_STATE, "psx_set_keypoints: no input image");
    if (on_device) {
        if (((uintptr_t)p & 7u) != 0) return fail(ctx, PSX_ERR_INVALID, "psx_set_keypoints_dev: the records must be 8-byte aligned");
        ctx->kp.list = n > 0 ? p : nullptr; ctx->kp.n = n; ctx->kp.set = true;
        return PSX_OK;
    }
    PSX_HIP(hipSetDevice(ctx->device));
    if (n > 0) {
        const size_t room = (size_t)n + (size_t)n / 4;
        PSX_HIP(ctx->kp.own.push(p, (size_t)n, room, room, ctx->stream));
    }
    ctx->kp.list = n > 0 ? ctx->kp.own.dev.p : nullptr; ctx->kp.n = n; ctx->kp.set = true;
    return PSX_OK;
}

int psx_set_keypoints(psx_ctx* ctx, const psx_keypoint* host, int n) { return set_keypoints_common(ctx, host, n, false); }
int psx_set_keypoints_dev(psx_ctx* ctx, const psx_keypoint* dev, int n) { return set_keypoints_common(ctx, dev, n, true); }

int psx_describe(psx_ctx* ctx, int flags)
{
    if (!ctx) return PSX_ERR_INVALID;
    if ((flags & ~PSX_DESCRIBE_REUSE_PYRAMID) != 0) return fail(ctx, PSX_ERR_INVALID, "psx_describe: unknown flag");
    if (!ctx->d_input || !ctx->d_pyr) return fail(ctx, PSX_ERR_STATE, "psx_describe: no input image");
    if (!ctx->kp.set) return fail(ctx, PSX_ERR_STATE, "psx_describe: no keypoints set");
    const bool reuse = (flags & PSX_DESCRIBE_REUSE_PYRAMID) != 0;
    if (reuse && !ctx->pyr_ready) return fail(ctx, PSX_ERR_STATE, "psx_describe: the context holds no pyramid of the current input");
    PSX_HIP(hipSetDevice(ctx->device));
    const PsxParams& P = ctx->hp;

    // side arrays: one entry per extremum that can come out of this list
    int rc;
    const size_t side = (size_t)imax(1, imin(ctx->kp.n, P.ext_capacity));
    const size_t tbl_need = psx_kp_table_ints(P.num_octaves, ctx->kp.n);
    if (side > ctx->kp.src.cap || tbl_need > ctx->kp.tbl.cap) {
        PSX_HIP(hipStreamSynchronize(ctx->stream));
        const size_t room = side + side / 4;
        PSX_HIP(ctx->kp.tbl.grow(tbl_need + tbl_need / 4));
        PSX_HIP(ctx->kp.src.grow(room));
        PSX_HIP(ctx->kp.gnori.grow(room));
        PSX_HIP(ctx->kp.gori.grow(4 * room));
    }

    if (!reuse) {
        ctx->interleave = false;                   // no detector: the extrema scans are not launched
        if ((rc = psx_build_pyramid(ctx)) != PSX_OK) return rc;
    } else {
        ctx->counts_valid = false;
        if (ctx->tm.on) { PSX_HIP(hipEventRecord(ctx->tm.ev[0].h, ctx->stream)); PSX_HIP(hipEventRecord(ctx->tm.ev[1].h, ctx->stream)); }
    }
    ctx->ext_launched = false;
    ctx->filtered = false;

    PsxKpGeom g;
    memset(&g, 0, sizeof(g));
    psx_kp_geom_scale(&ctx->cfg, &g);
    g.num_octaves = P.num_octaves;
    for (int o = 0; o < P.num_octaves; o++) { g.w[o] = P.oct[o].w; g.h[o] = P.oct[o].h; }
    PsxKpBuffers b;
    b.kps = ctx->kp.list; b.n = ctx->kp.n;
    b.tbl = ctx->kp.tbl; b.src = ctx->kp.src; b.gnori = ctx->kp.gnori; b.gori = ctx->kp.gori;
    // every counter the later stages read is written by the injection (ext_ct of all octaves) or by the scan
    PSX_HIP(psx_launch_kp_inject(ctx->tune, ctx->d_params, ctx->d_cnt, g, b, ctx->stream));
    if (ctx->tm.on) PSX_HIP(hipEventRecord(ctx->tm.ev[2].h, ctx->stream));
    PSX_HIP(psx_launch_orientation(ctx->tune, ctx->d_params, ctx->d_cnt, ctx->stream));
    PSX_HIP(psx_launch_kp_adopt(ctx->tune, ctx->d_params, b, ctx->stream));
    snapshot_export(ctx);
    PSX_HIP(psx_launch_scan(ctx->d_params, ctx->d_cnt, ctx->xp.fx, ctx->stream));
    if (ctx->tm.on) PSX_HIP(hipEventRecord(ctx->tm.ev[3].h, ctx->stream));
    rc = psx_descriptors(ctx);
    ctx->kp.results = rc == PSX_OK;
    return rc;
}

// ---- detection mask (mask_rule.h) ---------------------------------------------------------------------------------------

static int set_mask_common(psx_ctx* ctx, const unsigned char* p, int w, int h, bool on_device)
{
    if (!ctx) return PSX_ERR_INVALID;
    const char* who = on_device ? "psx_set_mask_dev" : "psx_set_mask";
    if (!p) {
        if (w != 0 || h != 0) return fail(ctx, PSX_ERR_INVALID, std::string(who) + ": a null mask with a non-zero size");
        ctx->mask.data = nullptr; ctx->mask.w = 0; ctx->mask.h = 0;         // cleared
        return PSX_OK;
    }
    if (w <= 0 || h <= 0) return fail(ctx, PSX_ERR_INVALID, std::string(who) + ": non-positive mask size");
    if (on_device) {
        ctx->mask.data = p; ctx->mask.w = w; ctx->mask.h = h;
        return PSX_OK;
    }
    PSX_HIP(hipSetDevice(ctx->device));
    const size_t bytes = (size_t)w * (size_t)h;
    PSX_HIP(ctx->mask.own.push(p, bytes, bytes, bytes, ctx->stream));
    ctx->mask.data = ctx->mask.own.dev; ctx->mask.w = w; ctx->mask.h = h;
    return PSX_OK;
}

int psx_set_mask(psx_ctx* ctx, const unsigned char* host, int w, int h) { return set_mask_common(ctx, host, w, h, false); }
int psx_set_mask_dev(psx_ctx* ctx, const unsigned char* dev, int w, int h) { return set_mask_common(ctx, dev, w, h, true); }

int psx_mask_keep(const unsigned char* mask, int w, int h, const float* xpos, const float* ypos, int n, unsigned char* keep_out)
{
    if (!mask || w <= 0 || h <= 0 || n < 0) return PSX_ERR_INVALID;
    if (n > 0 && (!xpos || !ypos || !keep_out)) return PSX_ERR_INVALID;
    for (int i = 0; i < n; i++) keep_out[i] = psx_mask_allows(mask, w, h, xpos[i], ypos[i]) ? 1 : 0;
    return PSX_OK;
}

int psx_keypoint_map(psx_ctx* ctx, int* host_src, int capacity, int* count)
{
    if (!ctx) return PSX_ERR_INVALID;
    if (!ctx->kp.results) return fail(ctx, PSX_ERR_STATE, "psx_keypoint_map: the last results are not a psx_describe call's");
    int rc = fetch_counts(ctx);
    if (rc != PSX_OK) return rc;
    const int n = ctx->h_cnt->ext_total;
    if (count) *count = n;
    if (host_src) {
        if (n > capacity) return fail(ctx, PSX_ERR_INVALID, "psx_keypoint_map: output capacity too small");
        if (n > 0) PSX_HIP(hipMemcpy(host_src, ctx->kp.src, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
    }
    return PSX_OK;
}

int psx_sync(psx_ctx* ctx)
{
    if (!ctx) return PSX_ERR_INVALID;
    PSX_HIP(hipSetDevice(ctx->device));
    PSX_HIP(hipStreamSynchronize(ctx->stream));
    return PSX_OK;
}

static int fetch_counts_full(psx_ctx* ctx)
{
    if (ctx->counts_valid && !ctx->counts_partial) return PSX_OK;
    { int rc0 = fetch_counts(ctx); if (rc0 != PSX_OK) return rc0; }     // grows the descriptor buffers if needed
    if (!ctx->counts_partial) return PSX_OK;
    PSX_HIP(hipSetDevice(ctx->device));
    PSX_HIP(hipMemcpyAsync(ctx->h_cnt, ctx->d_cnt, sizeof(PsxCounters), hipMemcpyDeviceToHost, ctx->stream));
    { int wrc = wait_stream(ctx); if (wrc != PSX_OK) return wrc; }
    ctx->counts_valid = true;
    ctx->counts_partial = false;
    return PSX_OK;
}

// A frame produced more orientations than the descriptor buffers hold (they start at the reference's
// 2 x max_extrema entries): grow them and redo the two stages that depend on the capacity -- the
// orientation scan and the descriptors; the oriented extrema are still in place.  Pyramid::reallocExtrema,
// sift_pyramid.cu:186-209.
static int regrow_descriptors(psx_ctx* ctx, int ori_raw)
{
    PsxParams& P = ctx->hp;
    const size_t need = (size_t)ori_raw + (size_t)ori_raw / 4 + 1024;
    PSX_HIP(hipStreamSynchronize(ctx->stream));
    PSX_HIP(ctx->d_desc.grow(need * 128));
    PSX_HIP(ctx->d_feat_to_ext.grow(need));
    // the byte array of a frame launched in byte mode grows with the floats (it is a kernel argument: the repeat carries the new one)
    if (ctx->xp.fx.desc_u8 != nullptr) {
        PSX_HIP(ctx->d_desc_u8.grow(ctx->d_desc.cap));
        ctx->xp.fx.desc_u8 = ctx->d_desc_u8;
    }
    P.desc = ctx->d_desc;
    P.feat_to_ext = ctx->d_feat_to_ext;
    P.ori_capacity = (int)need;
    *ctx->h_params_pin = P;
    PSX_HIP(hipMemcpyAsync(ctx->d_params, ctx->h_params_pin, sizeof(P), hipMemcpyHostToDevice, ctx->stream));
    drop_graph(ctx);
    // same targets as the launch being repeated
    PSX_HIP(psx_launch_scan(ctx->d_params, ctx->d_cnt, ctx->xp.fx, ctx->stream));
    return launch_descriptor_stage(ctx);
}

static int fetch_counts(psx_ctx* ctx)
{
    if (ctx->counts_valid) return PSX_OK;
    PSX_HIP(hipSetDevice(ctx->device));
    for (int attempt = 0; attempt < 2; attempt++) {
        int raw;
        if (ctx->xp.fx_on) {
            // the frame was launched with export targets: its scan kernel deposited the counters in pinned memory
            { int wrc = wait_stream(ctx); if (wrc != PSX_OK) return wrc; }
            ctx->h_cnt->ext_total = ctx->xp.counts[0];
            ctx->h_cnt->ori_total = ctx->xp.counts[1];
            raw = ctx->xp.counts[2];
            ctx->h_cnt->flow_error = ctx->xp.counts[3];
            ctx->counts_partial = true;
        } else {
            PSX_HIP(hipMemcpyAsync(ctx->h_cnt, ctx->d_cnt, sizeof(PsxCounters), hipMemcpyDeviceToHost, ctx->stream));
            { int wrc = wait_stream(ctx); if (wrc != PSX_OK) return wrc; }
            raw = ctx->h_cnt->ori_raw;
            ctx->counts_partial = false;
        }
        // k_pyramid_flow gave up on a dependency wait (never in a correct run): the planes, hence the features, are invalid
        if (ctx->h_cnt->flow_error != 0)
            return fail(ctx, PSX_ERR_STATE, "the pyramid kernel ran into the bound of a device-side dependency wait: the frame is invalid");
        if (raw <= ctx->hp.ori_capacity || attempt == 1) break;
        int rc = regrow_descriptors(ctx, raw);
        if (rc != PSX_OK) return rc;
    }
    ctx->counts_valid = true;
    return PSX_OK;
}

int psx_counts(psx_ctx* ctx, int* num_features, int* num_descriptors)
{
    if (!ctx) return PSX_ERR_INVALID;
    int rc = fetch_counts(ctx);
    if (rc != PSX_OK) return rc;
    if (num_features) *num_features = ctx->h_cnt->ext_total;
    if (num_descriptors) *num_descriptors = ctx->h_cnt->ori_total;
    return PSX_OK;
}

// both download calls.  who: the caller's name in the error strings; dev_desc: the descriptor array (elem_bytes per value);
// exported_host_desc: the export target of that array the frame in flight was launched with
static int download_results(psx_ctx* ctx, const char* who, psx_feature* features, int feature_capacity, void* descriptors,
                            int descriptor_capacity, size_t elem_bytes, const void* dev_desc, const void* exported_host_desc)
{
    const int ne = ctx->h_cnt->ext_total, no = ctx->h_cnt->ori_total;
    if (ne > feature_capacity || no > descriptor_capacity)
        return fail(ctx, PSX_ERR_INVALID, std::string(who) + ": output capacity too small");
    if (ne > 0 && !features) return fail(ctx, PSX_ERR_INVALID, std::string(who) + ": null feature buffer");
    if (no > 0 && !descriptors) return fail(ctx, PSX_ERR_INVALID, std::string(who) + ": null descriptor buffer");
    const bool feat_exported = (ctx->xp.fx_on && features == ctx->xp.fx_host_feat && ne <= ctx->xp.fx.feat_capacity);
    const bool desc_exported = (ctx->xp.fx_on && descriptors == exported_host_desc && no <= ctx->xp.fx.desc_capacity);
    if (elem_bytes == sizeof(float)) {
        // PSX_NULL_DEVICE_WORK=2: one real download per CONTEXT keeps its host records well formed (a process-wide flag was a
        // data race between the workers and left every context but the first with uninitialised host buffers)
        if (ctx->tune.null_device_work == 2 && ctx->nulldev.primed && ctx->nulldev.dl_done) return PSX_OK;
        if (ctx->tune.null_device_work == 2 && ctx->nulldev.primed) ctx->nulldev.dl_done = true;
    }
    if (ne > 0 && !feat_exported)
        PSX_HIP(hipMemcpyAsync(features, ctx->d_features, (size_t)ne * sizeof(psx_feature),
                               hipMemcpyDeviceToHost, ctx->stream));
    if (no > 0 && !desc_exported)
        PSX_HIP(hipMemcpyAsync(descriptors, dev_desc, (size_t)no * 128 * elem_bytes, hipMemcpyDeviceToHost, ctx->stream));
    // sleep on an event when the context is in blocking mode (the C++ pipeline's workers): hipStreamSynchronize spins, and
    // the ~0.3 ms of a frame's result DMA -- several ms when replicas share a GPU -- were a busy core per worker
    return wait_stream(ctx);
}

int psx_download(psx_ctx* ctx, psx_feature* features, int feature_capacity, float* descriptors,
                 int descriptor_capacity)
{
    if (!ctx) return PSX_ERR_INVALID;
    int rc = fetch_counts(ctx);
    if (rc != PSX_OK) return rc;
    return download_results(ctx, "psx_download", features, feature_capacity, descriptors, descriptor_capacity, sizeof(float),
                            ctx->d_desc, ctx->xp.fx_host_desc);
}

// Detach everything exported; both attach calls start here.  Memory an earlier psx_attach_export had to register is a
// reason to wait first: the frame in flight may still be storing into it.  Without any, no HIP call.
static int detach_exports(psx_ctx* ctx, bool always_wait)
{
    if (always_wait || ctx->xp.feat.registered || ctx->xp.desc.registered || ctx->xp.u8.registered) {
        PSX_HIP(hipSetDevice(ctx->device));
        PSX_HIP(hipStreamSynchronize(ctx->stream));
    }
    ctx->xp.feat.reset(); ctx->xp.desc.reset(); ctx->xp.u8.reset();
    return PSX_OK;
}

int psx_attach_export(psx_ctx* ctx, psx_feature* host_features, int feature_capacity,
                      float* host_descriptors, int descriptor_capacity)
{
    if (!ctx) return PSX_ERR_INVALID;
    { const int rc = detach_exports(ctx, true); if (rc != PSX_OK) return rc; }
    if (host_features && feature_capacity > 0)
        PSX_HIP(ctx->xp.feat.attach(host_features, (size_t)feature_capacity * sizeof(psx_feature), feature_capacity));
    if (host_descriptors && descriptor_capacity > 0)
        PSX_HIP(ctx->xp.desc.attach(host_descriptors, (size_t)descriptor_capacity * 128 * sizeof(float), descriptor_capacity));
    drop_graph(ctx);      // the targets are kernel arguments
    return PSX_OK;
}

int psx_attach_export_mapped(psx_ctx* ctx, psx_feature* host_features, int feature_capacity,
                             float* host_descriptors, int descriptor_capacity)
{
    if (!ctx) return PSX_ERR_INVALID;
    // Normally no HIP call: the targets travel as kernel arguments of the NEXT extraction; the frame in flight (if
    // any) keeps the targets it was launched with, and its counters / results are still fetched from those
    // (psx_ctx::xp.fx).
    { const int rc = detach_exports(ctx, false); if (rc != PSX_OK) return rc; }
    // psx_host_alloc memory: mapped, and its device address is its host address (checked at allocation)
    ctx->xp.feat.adopt(feature_capacity > 0 ? host_features : nullptr, feature_capacity);
    ctx->xp.desc.adopt(descriptor_capacity > 0 ? host_descriptors : nullptr, descriptor_capacity);
    drop_graph(ctx);
    return PSX_OK;
}

// ---- byte descriptors ---------------------------------------------------------------------------------------------------

int psx_set_descriptor_format(psx_ctx* ctx, int fmt)
{
    if (fmt != PSX_DESCFMT_F32 && fmt != PSX_DESCFMT_U8) {
        if (ctx) ctx->err = "psx_set_descriptor_format: unknown descriptor format";
        return PSX_ERR_INVALID;
    }
    if (!ctx) return PSX_ERR_INVALID;
    if (fmt == ctx->desc_fmt) return PSX_OK;
    PSX_HIP(hipSetDevice(ctx->device));
    // switching back to float mode keeps the byte array (a frame in flight may still be storing into it).  grow() replaces
    // it only when the float array has grown since it was sized; hipFree waits for the device to be idle, so no frame in
    // flight still stores into the old one -- the same rule as every other buffer grow() replaces
    if (fmt == PSX_DESCFMT_U8 && ctx->d_desc.cap > 0) {
        PSX_HIP(ctx->d_desc_u8.grow(ctx->d_desc.cap));
    }
    if (fmt == PSX_DESCFMT_F32 && ctx->xp.u8.dev) {
        if (ctx->xp.u8.registered) PSX_HIP(hipStreamSynchronize(ctx->stream));
        ctx->xp.u8.reset();
    }
    ctx->desc_fmt = fmt;
    drop_graph(ctx);      // the byte array is a kernel argument
    return PSX_OK;
}

int psx_download_u8(psx_ctx* ctx, psx_feature* features, int feature_capacity, unsigned char* descriptors,
                    int descriptor_capacity)
{
    if (!ctx) return PSX_ERR_INVALID;
    if (ctx->desc_fmt != PSX_DESCFMT_U8) return fail(ctx, PSX_ERR_STATE, "psx_download_u8: the context is not in byte mode");
    int rc = fetch_counts(ctx);
    if (rc != PSX_OK) return rc;
    // the frame must have been launched in byte mode (the format switched after its launch leaves no bytes of it)
    if (ctx->xp.fx.desc_u8 == nullptr) return fail(ctx, PSX_ERR_STATE, "psx_download_u8: the last extraction ran in float mode");
    return download_results(ctx, "psx_download_u8", features, feature_capacity, descriptors, descriptor_capacity, 1,
                            ctx->d_desc_u8, ctx->xp.fx_host_u8);
}

// both byte attach calls: the float descriptor export is detached, the feature export is replaced
static int attach_u8_common(psx_ctx* ctx, psx_feature* host_features, int feature_capacity,
                            unsigned char* host_descriptors, int descriptor_capacity, bool mapped)
{
    if (!ctx) return PSX_ERR_INVALID;
    if (ctx->desc_fmt != PSX_DESCFMT_U8 && host_descriptors && descriptor_capacity > 0)
        return fail(ctx, PSX_ERR_STATE, "psx_attach_export_u8: the context is not in byte mode");
    int rc = mapped ? psx_attach_export_mapped(ctx, host_features, feature_capacity, nullptr, 0)
                    : psx_attach_export(ctx, host_features, feature_capacity, nullptr, 0);
    if (rc != PSX_OK) return rc;
    if (host_descriptors && descriptor_capacity > 0) {
        if (mapped) ctx->xp.u8.adopt(host_descriptors, descriptor_capacity);
        else PSX_HIP(ctx->xp.u8.attach(host_descriptors, (size_t)descriptor_capacity * 128, descriptor_capacity));
    }
    return PSX_OK;
}

int psx_attach_export_u8(psx_ctx* ctx, psx_feature* host_features, int feature_capacity,
                         unsigned char* host_descriptors, int descriptor_capacity)
{
    return attach_u8_common(ctx, host_features, feature_capacity, host_descriptors, descriptor_capacity, false);
}

int psx_attach_export_mapped_u8(psx_ctx* ctx, psx_feature* host_features, int feature_capacity,
                                unsigned char* host_descriptors, int descriptor_capacity)
{
    return attach_u8_common(ctx, host_features, feature_capacity, host_descriptors, descriptor_capacity, true);
}

int psx_device_results(psx_ctx* ctx, const psx_feature** d_features, const float** d_descriptors,
                       const int** d_feat_to_ext)
{
    if (!ctx) return PSX_ERR_INVALID;
    if (d_features) *d_features = ctx->d_features;
    if (d_descriptors) *d_descriptors = ctx->d_desc;
    if (d_feat_to_ext) *d_feat_to_ext = ctx->d_feat_to_ext;
    return PSX_OK;
}

int psx_host_alloc(size_t bytes, void** out)
{
    psx_ctx* ctx = nullptr;
    if (!out) return PSX_ERR_INVALID;
    PSX_HIP(hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocMapped | hipHostMallocPortable));
    // psx_upload_pinned / psx_attach_export_mapped rely on "device address == host address" for this memory
    void* dev = nullptr;
    if (hipHostGetDevicePointer(&dev, *out, 0) != hipSuccess || dev != *out) {
        (void)hipHostFree(*out); *out = nullptr;
        return fail(nullptr, PSX_ERR_HIP, "psx_host_alloc: mapped host memory has a different device address on this system");
    }
    return PSX_OK;
}

int psx_host_alloc_near(int device, size_t bytes, void** out)
{
    psx_ctx* ctx = nullptr;
    if (device >= 0) PSX_HIP(hipSetDevice(device));
    return psx_host_alloc(bytes, out);
}

int psx_host_free(void* ptr)
{
    psx_ctx* ctx = nullptr;
    if (!ptr) return PSX_OK;
    PSX_HIP(hipHostFree(ptr));
    return PSX_OK;
}

int psx_dev_alloc(int device, size_t bytes, void** out)
{
    psx_ctx* ctx = nullptr;
    if (!out) return PSX_ERR_INVALID;
    PSX_HIP(hipSetDevice(device));
    PSX_HIP(hipMalloc(out, bytes ? bytes : 1));
    return PSX_OK;
}

int psx_dev_free(int device, void* ptr)
{
    psx_ctx* ctx = nullptr;
    if (!ptr) return PSX_OK;
    PSX_HIP(hipSetDevice(device));
    PSX_HIP(hipFree(ptr));
    return PSX_OK;
}

int psx_dev_read(int device, void* host_dst, const void* dev_src, size_t bytes)
{
    psx_ctx* ctx = nullptr;
    if (bytes == 0) return PSX_OK;
    if (!host_dst || !dev_src) return PSX_ERR_INVALID;
    PSX_HIP(hipSetDevice(device));
    PSX_HIP(hipMemcpy(host_dst, dev_src, bytes, hipMemcpyDeviceToHost));
    return PSX_OK;
}

int psx_dev_write(int device, void* dev_dst, const void* host_src, size_t bytes)
{
    psx_ctx* ctx = nullptr;
    if (bytes == 0) return PSX_OK;
    if (!dev_dst || !host_src) return PSX_ERR_INVALID;
    PSX_HIP(hipSetDevice(device));
    PSX_HIP(hipMemcpy(dev_dst, host_src, bytes, hipMemcpyHostToDevice));
    return PSX_OK;
}

int psx_clone_results(psx_ctx* ctx, void* d_features, void* d_descriptors, int* d_reverse_map)
{
    if (!ctx) return PSX_ERR_INVALID;
    int rc = fetch_counts(ctx);
    if (rc != PSX_OK) return rc;
    const int ne = ctx->h_cnt->ext_total, no = ctx->h_cnt->ori_total;
    if (ne > 0 && d_features)
        PSX_HIP(psx_launch_feature_ptrs(ctx->d_features, static_cast<psx_feature_dev*>(d_features), ne,
                                        static_cast<float*>(d_descriptors), d_descriptors ? no : 0, ctx->stream));
    if (no > 0 && d_descriptors)
        PSX_HIP(hipMemcpyAsync(d_descriptors, ctx->d_desc, (size_t)no * 128 * sizeof(float),
                               hipMemcpyDeviceToDevice, ctx->stream));
    if (no > 0 && d_reverse_map)
        PSX_HIP(hipMemcpyAsync(d_reverse_map, ctx->d_feat_to_ext, (size_t)no * sizeof(int),
                               hipMemcpyDeviceToDevice, ctx->stream));
    PSX_HIP(hipStreamSynchronize(ctx->stream));
    return PSX_OK;
}

int psx_device_count(int* count)
{
    psx_ctx* ctx = nullptr;
    if (!count) return PSX_ERR_INVALID;
    *count = 0;
    PSX_HIP(hipGetDeviceCount(count));
    return PSX_OK;
}

int psx_device_info(int device, char* name, int name_len, size_t* total_mem, int* compute_units, int* clock_khz)
{
    psx_ctx* ctx = nullptr;
    hipDeviceProp_t p;
    PSX_HIP(hipGetDeviceProperties(&p, device));
    if (name && name_len > 0) { strncpy(name, p.name, (size_t)name_len - 1); name[name_len - 1] = 0; }
    if (total_mem) *total_mem = p.totalGlobalMem;
    if (compute_units) *compute_units = p.multiProcessorCount;
    if (clock_khz) *clock_khz = p.clockRate;
    return PSX_OK;
}

int psx_device_pci(int device, char* bus_id, int len)
{
    psx_ctx* ctx = nullptr;
    if (!bus_id || len < 16) return PSX_ERR_INVALID;
    bus_id[0] = 0;
    PSX_HIP(hipDeviceGetPCIBusId(bus_id, len, device));
    return PSX_OK;
}

int psx_dump_plane(psx_ctx* ctx, int kind, int octave, int level, float* host_out)
{
    if (!ctx || !host_out) return PSX_ERR_INVALID;
    const PsxParams& P = ctx->hp;
    if (!ctx->d_pyr || octave < 0 || octave >= P.num_octaves) return fail(ctx, PSX_ERR_INVALID, "bad octave");
    const int nl = (kind == PSX_PLANE_DOG) ? P.L - 1 : P.L;
    if (level < 0 || level >= nl) return fail(ctx, PSX_ERR_INVALID, "bad level");
    PSX_HIP(hipSetDevice(ctx->device));
    PSX_HIP(hipStreamSynchronize(ctx->stream));
    const PsxOctave& oc = P.oct[octave];
    const float* src = oc.data + (size_t)level * oc.plane;
    if (kind == PSX_PLANE_GAUSS) {
        PSX_HIP(hipMemcpy2D(host_out, (size_t)oc.w * 4, src, (size_t)oc.pitch * 4, (size_t)oc.w * 4, oc.h,
                            hipMemcpyDeviceToHost));
    } else {
        // make_dog (s_pyramid_build.cu:74-92) into a scratch plane
        float* tmp = nullptr;
        PSX_HIP(hipMalloc(reinterpret_cast<void**>(&tmp), oc.plane * sizeof(float)));
        hipError_t e = psx_launch_dog(src, src + oc.plane, tmp, oc.w, oc.h, oc.pitch, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e == hipSuccess)
            e = hipMemcpy2D(host_out, (size_t)oc.w * 4, tmp, (size_t)oc.pitch * 4, (size_t)oc.w * 4, oc.h,
                            hipMemcpyDeviceToHost);
        (void)hipFree(tmp);
        PSX_HIP(e);
    }
    return PSX_OK;
}

int psx_dump_iext(psx_ctx* ctx, int octave, psx_iext* host_out, int capacity, int* count)
{
    if (!ctx || octave < 0 || octave >= ctx->hp.num_octaves) return PSX_ERR_INVALID;
    if (ctx->counts_partial) { ctx->counts_valid = false; }
    int rc = fetch_counts_full(ctx);
    if (rc != PSX_OK) return rc;
    int n = imin(ctx->filtered ? ctx->h_cnt->iext_ct[octave] : ctx->h_cnt->ext_ct[octave], ctx->cfg.max_extrema);
    if (count) *count = n;
    if (host_out) {
        n = imin(n, capacity);
        if (n > 0) PSX_HIP(hipMemcpy(host_out, ctx->hp.iext[octave], (size_t)n * sizeof(psx_iext), hipMemcpyDeviceToHost));
    }
    return PSX_OK;
}

int psx_dump_extrema(psx_ctx* ctx, psx_extremum* host_out, int capacity, int* count)
{
    if (!ctx) return PSX_ERR_INVALID;
    int rc = fetch_counts(ctx);
    if (rc != PSX_OK) return rc;
    int n = ctx->h_cnt->ext_total;
    if (count) *count = n;
    if (host_out) {
        n = imin(n, capacity);
        if (n > 0) PSX_HIP(hipMemcpy(host_out, ctx->d_extrema, (size_t)n * sizeof(psx_extremum), hipMemcpyDeviceToHost));
    }
    return PSX_OK;
}

int psx_set_wait_mode(psx_ctx* ctx, int blocking)
{
    if (!ctx) return PSX_ERR_INVALID;
    ctx->blocking_wait = blocking != 0;
    return PSX_OK;
}

int psx_enable_timers(psx_ctx* ctx, int on)
{
    if (!ctx) return PSX_ERR_INVALID;
    ctx->tm.on = on != 0;
    return PSX_OK;
}

int psx_stage_times(psx_ctx* ctx, float ms[4])
{
    if (!ctx || !ms) return PSX_ERR_INVALID;
    if (!ctx->tm.on) return fail(ctx, PSX_ERR_STATE, "timers are not enabled");
    PSX_HIP(hipSetDevice(ctx->device));
    PSX_HIP(hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < 4; i++) PSX_HIP(hipEventElapsedTime(&ms[i], ctx->tm.ev[i].h, ctx->tm.ev[i + 1].h));
    return PSX_OK;
}

int psx_time_blur(psx_ctx* ctx, int octave, int level, int reps, float* avg_ms, double* bytes)
{
    if (!ctx || !avg_ms) return PSX_ERR_INVALID;
    const PsxParams& P = ctx->hp;
    if (!ctx->d_pyr || octave < 0 || octave >= P.num_octaves || level < 1 || level >= P.L || reps < 1)
        return fail(ctx, PSX_ERR_INVALID, "psx_time_blur: bad arguments");
    PSX_HIP(hipSetDevice(ctx->device));
    PSX_HIP(hipEventRecord(ctx->tm.t0, ctx->stream));
    for (int r = 0; r < reps; r++) {
        int rc = launch_blur_level(ctx, octave, level);
        if (rc != PSX_OK) return rc;
    }
    PSX_HIP(hipEventRecord(ctx->tm.t1, ctx->stream));
    PSX_HIP(hipStreamSynchronize(ctx->stream));
    float ms = 0.0f;
    PSX_HIP(hipEventElapsedTime(&ms, ctx->tm.t0, ctx->tm.t1));
    *avg_ms = ms / reps;
    if (bytes) *bytes = 8.0 * (double)P.oct[octave].w * (double)P.oct[octave].h;
    return PSX_OK;
}

#ifdef PSX_PHASE_TIMING
int psx_debug_launch_extrema(psx_ctx* ctx, int o)
{
    { const int mrc = check_mask(ctx, "psx_debug_launch_extrema"); if (mrc != PSX_OK) return mrc; }
    PSX_HIP(psx_launch_extrema(ctx->d_params, ctx->hp, ctx->d_cnt, o, mask_of(ctx), ctx->stream));
    return PSX_OK;
}
#endif


int psx_enable_blur_probe(psx_ctx* ctx, int on)
{
    if (!ctx) return PSX_ERR_INVALID;
    PSX_HIP(hipSetDevice(ctx->device));
    for (int i = 0; on && i < 2 * PSX_GAUSS_LEVELS; i++) PSX_HIP(ctx->tm.ev_blur[i].get(hipEventDefault));
    for (int i = 0; on && i < 4; i++) PSX_HIP(ctx->tm.ev_x[i].get(hipEventDefault));
    ctx->tm.probe = on != 0;
    ctx->tm.probe_ext0 = false;
    ctx->tm.probe_n = 0;
    return PSX_OK;
}

int psx_blur_probe_times(psx_ctx* ctx, float* ms, int capacity, int* n, double* bytes_per_launch)
{
    if (!ctx || !ms || !n) return PSX_ERR_INVALID;
    if (!ctx->tm.probe) return fail(ctx, PSX_ERR_STATE, "the blur probe is not enabled");
    PSX_HIP(hipSetDevice(ctx->device));
    PSX_HIP(hipStreamSynchronize(ctx->stream));
    *n = ctx->tm.probe_n;
    for (int i = 0; i < ctx->tm.probe_n && i < capacity; i++)
        PSX_HIP(hipEventElapsedTime(&ms[i], ctx->tm.ev_blur[2 * i].h, ctx->tm.ev_blur[2 * i + 1].h));
    if (bytes_per_launch) *bytes_per_launch = ctx->tm.probe_bytes;
    return PSX_OK;
}

// Measurement: one pyramid build with k_pyramid_flow recording, per work item, the 100 MHz wall clock at dequeue /
// dependencies met / arithmetic done / published, a word (octave << 40 | level << 32 | chunk << 16 | strip) and the
// workgroup: 6 int64 per item, in ticket order.  *nitems = items of the plan (0: the flow kernel is not in use).
int psx_flow_trace(psx_ctx* ctx, long long* host_out, int capacity_items, int* nitems)
{
    if (!ctx || !nitems) return PSX_ERR_INVALID;
    *nitems = ctx->flow.on ? ctx->flow.nitems : 0;
    if (!ctx->flow.on || host_out == nullptr || capacity_items < ctx->flow.nitems) return PSX_OK;
    PSX_HIP(hipSetDevice(ctx->device));
    PSX_HIP(hipStreamSynchronize(ctx->stream));
    const size_t bytes = sizeof(long long) * 6 * (size_t)ctx->flow.nitems;
    DevBuf<long long> trace;
    PSX_HIP(trace.grow(6 * (size_t)ctx->flow.nitems));
    (void)hipMemset(trace, 0, bytes);
    ctx->flow.trace = trace;
    int rc = psx_build_pyramid(ctx);
    ctx->flow.trace = nullptr;
    hipError_t e = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess) e = hipMemcpy(host_out, trace, bytes, hipMemcpyDeviceToHost);
    if (rc != PSX_OK) return rc;
    PSX_HIP(e);
    return PSX_OK;
}

// The probe's two other HBM-bound kernels of octave 0, timed in the pipeline with stream events around the launch (they
// include the gap in front of the kernel): level 0 (k_level0_fused, or k_upscale + k_blur<R, true>) and the extrema scan.
// bytes: the algorithmic figures of SURVEY.md 8d (4 B per octave-0 pixel + the input; 24 B per octave-0 pixel).
// extrema_ms = 0 when octave 0's scan shared a launch with other octaves (small images).
int psx_probe_extra_times(psx_ctx* ctx, float* level0_ms, double* level0_bytes, float* extrema_ms, double* extrema_bytes)
{
    if (!ctx || !level0_ms || !extrema_ms) return PSX_ERR_INVALID;
    if (!ctx->tm.probe) return fail(ctx, PSX_ERR_STATE, "the blur probe is not enabled");
    PSX_HIP(hipSetDevice(ctx->device));
    PSX_HIP(hipStreamSynchronize(ctx->stream));
    const PsxParams& P = ctx->hp;
    *level0_ms = 0.0f; *extrema_ms = 0.0f;
    if (!ctx->alt_pyramid) PSX_HIP(hipEventElapsedTime(level0_ms, ctx->tm.ev_x[0].h, ctx->tm.ev_x[1].h));
    if (ctx->tm.probe_ext0) PSX_HIP(hipEventElapsedTime(extrema_ms, ctx->tm.ev_x[2].h, ctx->tm.ev_x[3].h));
    const double n0 = (double)P.oct[0].w * P.oct[0].h;
    if (level0_bytes) *level0_bytes = 4.0 * n0 + (double)ctx->in_w * ctx->in_h * (ctx->input_is_float ? 4.0 : 1.0);
    if (extrema_bytes) *extrema_bytes = 4.0 * (double)P.L * n0;
    return PSX_OK;
}

void* psx_stream(psx_ctx* ctx) { return ctx ? (void*)ctx->stream : nullptr; }

} // extern "C"
