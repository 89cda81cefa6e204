/*
 * include/popsift_hip.h -- C-ABI of the MI355X-native SIFT extraction hot path.
 *
 * This is the drop-in boundary: the C++14 host library (popsift_amd/csrc/host, classes
 * PopSift / SiftJob / popsift::Config / popsift::FeaturesHost with the reference's
 * signatures) sits above it, the hand-written HIP kernels for gfx950 sit below it.
 * Plain pointers and sizes only; no HIP, torch or C++ types; every function returns an
 * int status (PSX_OK == 0) and never throws.  psx_last_error() gives the message the C++
 * layer turns into std::runtime_error, the reference's error convention
 * (common/debug_macros.h:122-127 POP_FATAL).
 *
 * Each entry point cites the reference interface it replaces (paths relative to
 * /root/reference/src/popsift).
 */
#ifndef POPSIFT_HIP_H
#define POPSIFT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PSX_OK                 0
#define PSX_ERR_INVALID       -1   /* bad argument / unsupported mode          */
#define PSX_ERR_HIP           -2   /* a HIP runtime call failed                */
#define PSX_ERR_NOMEM         -3   /* host or device allocation failed         */
#define PSX_ERR_STATE         -4   /* call sequence error (e.g. no image set)  */

#define PSX_MAX_OCTAVES       20   /* sift_conf.h:12  MAX_OCTAVES              */
#define PSX_GAUSS_ALIGN       32   /* sift_constants.h:37 GAUSS_ALIGN          */
#define PSX_GAUSS_LEVELS      12   /* sift_constants.h:38 GAUSS_LEVELS         */
#define PSX_ORI_MAX            4   /* sift_constants.h:55 ORIENTATION_MAX_COUNT*/

/* popsift::Config::GaussMode, sift_conf.h:38-46 */
enum { PSX_GAUSS_VLFEAT_COMPUTE = 0, PSX_GAUSS_VLFEAT_RELATIVE = 1, PSX_GAUSS_VLFEAT_RELATIVE_ALL = 2,
       PSX_GAUSS_OPENCV_COMPUTE = 3, PSX_GAUSS_FIXED9 = 4, PSX_GAUSS_FIXED15 = 5 };
/* popsift::Config::SiftMode, sift_conf.h:51-61 */
enum { PSX_MODE_POPSIFT = 0, PSX_MODE_OPENCV = 1, PSX_MODE_VLFEAT = 2 };
/* popsift::Config::ScalingMode, sift_conf.h:75-80 */
enum { PSX_SCALE_DIRECT = 0, PSX_SCALE_DEFAULT = 1 };
/* popsift::Config::DescMode, sift_conf.h:85-97 */
enum { PSX_DESC_LOOP = 0, PSX_DESC_ILOOP = 1, PSX_DESC_GRID = 2, PSX_DESC_IGRID = 3, PSX_DESC_NOTILE = 4 };
/* popsift::Config::NormMode, sift_conf.h:102-108 */
enum { PSX_NORM_ROOTSIFT = 0, PSX_NORM_CLASSIC = 1 };
/* popsift::Config::GridFilterMode, sift_conf.h:118-125 */
enum { PSX_FILTER_RANDOM = 0, PSX_FILTER_LARGEST_FIRST = 1, PSX_FILTER_SMALLEST_FIRST = 2 };

/* POD image of popsift::Config (sift_conf.h:29-409; defaults sift_conf.cu:18-41). */
typedef struct psx_config {
    int   octaves;             /* -1: auto = max(floor(log2(min(w,h))) - 3 + 2^up, 1), popsift.cpp:118-122 */
    int   levels;              /* 3 */
    float sigma;               /* 1.6 */
    float edge_limit;          /* 10 */
    float threshold;           /* 0.04 */
    float upscale_factor;      /* 1.0 (Config::setDownsampling stores -v) */
    int   gauss_mode;          /* PSX_GAUSS_VLFEAT_COMPUTE */
    int   sift_mode;           /* PSX_MODE_POPSIFT */
    int   scaling_mode;        /* PSX_SCALE_DEFAULT */
    int   desc_mode;           /* PSX_DESC_LOOP */
    int   norm_mode;           /* PSX_NORM_ROOTSIFT */
    int   norm_multi;          /* 0 */
    int   max_extrema;         /* 100000 per octave */
    int   assume_initial_blur; /* 1 */
    float initial_blur;        /* 0.5 */
    int   filter_max_extrema;  /* -1 (grid filter off) */
    int   filter_grid_size;    /* 2 */
    int   grid_filter_mode;    /* PSX_FILTER_RANDOM */
} psx_config;

/* One keypoint as handed back to the host: popsift::Feature (features.h:23-37) with the
 * four Descriptor* replaced by indices into the descriptor array (-1 == nullptr); the C++
 * layer turns them into pointers into its own FeaturesHost storage, which removes the
 * reference's device-side host-pointer arithmetic (sift_pyramid.cu:242-280). */
typedef struct psx_feature {
    int   debug_octave;
    float xpos;
    float ypos;
    float sigma;
    int   num_ori;
    float orientation[PSX_ORI_MAX];
    int   desc_idx[PSX_ORI_MAX];
} psx_feature;

/* popsift::Feature itself (features.h:23-37) as laid out by the x86-64 and gfx950 ABIs (72 bytes), with
 * DEVICE descriptor pointers: what FeaturesDev::getFeatures() points at (features.h:104-122). */
typedef struct psx_feature_dev {
    int    debug_octave;
    float  xpos;
    float  ypos;
    float  sigma;
    int    num_ori;
    float  orientation[PSX_ORI_MAX];
    int    pad;
    float* desc[PSX_ORI_MAX];
} psx_feature_dev;

/* popsift::InitialExtremum (sift_extremum.h:25-39) as stored by the extrema kernel. */
typedef struct psx_iext {
    float xpos;
    float ypos;
    int   lpos;
    float sigma;
    int   cell;
    int   ignore;
} psx_iext;

/* popsift::Extremum (sift_extremum.h:47-63). */
typedef struct psx_extremum {
    float xpos;
    float ypos;
    int   lpos;
    float sigma;
    int   octave;
    int   num_ori;
    int   idx_ori;
    float orientation[PSX_ORI_MAX];
} psx_extremum;

typedef struct psx_ctx psx_ctx;   /* one Pyramid + its buffers + one HIP stream */

/* ---- configuration -------------------------------------------------------------------- */

/* Config::Config() defaults, sift_conf.cu:18-41 (without its cudaGetDevice side effect). */
int psx_config_default(psx_config* cfg);

/* Config::getPeakThreshold(), sift_conf.cu:276-279. */
float psx_peak_threshold(const psx_config* cfg);

/* init_filter() host part (gauss_filter.cu:127-237): fills the "inc" and "dd" tables.
 * inc_filter: PSX_GAUSS_LEVELS*PSX_GAUSS_ALIGN floats, dd_filter: PSX_MAX_OCTAVES*PSX_GAUSS_ALIGN.
 * Error cases of gauss_filter.cu:131-144 (sigma > 2, too many levels) return PSX_ERR_INVALID. */
int psx_gauss_tables(const psx_config* cfg, float* inc_filter, int* inc_span, float* inc_sigma,
                     float* dd_filter, int* dd_span, float* dd_sigma);
/* Config::setPrintGaussTables / --print-gauss-tables: prints to stdout what the reference's init_filter prints
 * (gauss_filter.cu:146-161) and what print_gauss_filter_symbol<<<1,1>>>(columns) prints from the device copy of the
 * tables (gauss_filter.cu:24-120, 247-256; the reference passes columns = 10): the inc, interpolated inc, abs_o0,
 * abs_oN and dd tables, same layout and number formats, computed on the host. */
int psx_print_gauss_tables(const psx_config* cfg, int columns);


/* ---- context -------------------------------------------------------------------------- */

/* Replaces PopSift::PopSift + applyConfiguration (popsift.cpp:25-48, 91-107): selects the
 * device, computes the Gauss tables and constants of the context on the host (no global symbols; the
 * parameter block goes to the device with psx_resize, the filter taps travel as kernel arguments) and
 * creates the stream.  The environment switches of the library are read here, once per
 * context. */
int psx_create(int device, const psx_config* cfg, psx_ctx** out);
int psx_destroy(psx_ctx* ctx);
const char* psx_last_error(const psx_ctx* ctx);   /* ctx may be NULL: last create() error */

/* Replaces PopSift::private_init / Pyramid::Pyramid / Pyramid::resetDimensions
 * (popsift.cpp:128-144, sift_pyramid.cu:108-177): (re)allocates pyramid planes for an input of
 * w x h pixels.  Buffers only ever grow. */
int psx_resize(psx_ctx* ctx, int w, int h);

/* Octave geometry after psx_resize: popsift.cpp:124-125 and sift_pyramid.cu:129-134. */
int psx_num_octaves(const psx_ctx* ctx);
int psx_num_levels(const psx_ctx* ctx);           /* levels + 3 */
int psx_octave_dims(const psx_ctx* ctx, int octave, int* w, int* h);

/* ---- input ---------------------------------------------------------------------------- */

/* Replaces Image::load / ImageFloat::load (s_image.cu:69-77, 193-201): host -> device copy of
 * a tightly packed w*h plane, stream ordered.  Calls psx_resize when dimensions change. */
int psx_upload_u8(psx_ctx* ctx, const uint8_t* host, int w, int h);
int psx_upload_f32(psx_ctx* ctx, const float* host, int w, int h);

/* The same for an image that already lies in memory from psx_host_alloc (pinned): no pointer query, no staging
 * copy; the DMA reads the buffer directly, so it must stay untouched until the extraction has been waited for. */
int psx_upload_pinned(psx_ctx* ctx, const void* pinned_host, int w, int h, int is_float);

/* Input already resident in HBM (tight w*h plane).  The pointer must stay valid until the
 * extraction that uses it has finished.  No copy is made. */
int psx_set_input_dev(psx_ctx* ctx, const void* dev_ptr, int w, int h, int is_float);

/* ---- stages (all asynchronous on the context's stream) ---------------------------------- */

/* Pyramid::step1 -> build_pyramid (s_pyramid_build.cu:459-594, default branch). */
int psx_build_pyramid(psx_ctx* ctx);
/* Pyramid::find_extrema (s_extrema.cu:560-640). */
int psx_find_extrema(psx_ctx* ctx);
/* Pyramid::orientation incl. ori_prefix_sum (s_orientation.cu:364-441) and, when
 * filter_max_extrema > 0, extrema_filter_grid (s_filtergrid.cu:113-325) on the device.  As in the
 * reference the filter reads the extrema counts on the host first (one stream sync per frame); it
 * runs only if int(filter_max_extrema*1.1) < number of extrema (s_orientation.cu:378-383).
 * LargestScaleFirst / SmallestScaleFirst results are deterministic; RandomScale keeps the first
 * extrema of each cell in buffer (atomicAdd arrival) order, as the reference does. */
int psx_orientation(psx_ctx* ctx);
/* Pyramid::descriptors incl. normalize_histogram (sift_desc.cu:55-110) and prep_features
 * (sift_pyramid.cu:250-280). */
int psx_descriptors(psx_ctx* ctx);
/* step1 + step2 in one call (popsift.cpp:321-324). */
int psx_extract(psx_ctx* ctx);

/* How psx_counts / psx_sync-like waits of this context wait for the GPU: 0 (default) = hipStreamSynchronize
 * (lowest latency, the calling thread may spin), 1 = sleep on a blocking event (for hosts that run one
 * thread per context). */
int psx_set_wait_mode(psx_ctx* ctx, int blocking);

/* Waits for everything queued on the context's stream. */
int psx_sync(psx_ctx* ctx);

/* ---- results -------------------------------------------------------------------------- */

/* Pyramid::readDescCountersFromDevice (sift_pyramid.cu:373-381): synchronises, returns the
 * number of keypoints and descriptors of the last extraction. */
int psx_counts(psx_ctx* ctx, int* num_features, int* num_descriptors);

/* Pyramid::get_descriptors (sift_pyramid.cu:282-322): copies num_features psx_feature records
 * and num_descriptors*128 floats to host memory (capacities in elements); synchronises. */
int psx_download(psx_ctx* ctx, psx_feature* features, int feature_capacity,
                 float* descriptors, int descriptor_capacity);

/* Zero-copy export.  Replaces the per-image cudaHostRegister + 2x cudaMemcpyAsync + unregister of
 * Pyramid::get_descriptors / FeaturesHost::pin (sift_pyramid.cu:300-318, features.cu:86-111):
 * the caller attaches two host buffers (any host memory; they are registered once with the HIP
 * runtime, or pass memory that is already pinned) and the descriptor kernel streams every Feature
 * record and every normalised descriptor straight into them over PCIe while it computes, the scan
 * kernel deposits the two counters.  After psx_sync()/psx_counts() the results are in the buffers;
 * no copy is queued and the host never waits for a transfer.  Capacities are in elements;
 * results beyond a capacity are dropped from the export (the device copy stays complete).
 * Pass NULL/0 to detach. */
int psx_attach_export(psx_ctx* ctx, psx_feature* host_features, int feature_capacity,
                      float* host_descriptors, int descriptor_capacity);

/* psx_attach_export for buffers from psx_host_alloc (already pinned and GPU-mapped): no registration and no
 * pointer queries -- cheap enough to call once per frame when every result keeps its own descriptor buffer. */
int psx_attach_export_mapped(psx_ctx* ctx, psx_feature* host_features, int feature_capacity,
                             float* host_descriptors, int descriptor_capacity);

/* Device-resident results (FeaturesDev, features.h:104-122): pointers valid until the next
 * extraction on this context. */
int psx_device_results(psx_ctx* ctx, const psx_feature** d_features, const float** d_descriptors,
                       const int** d_feat_to_ext);

/* FeaturesDev support (MatchingMode, popsift.cpp:346-383, sift_pyramid.cu:324-362): device
 * buffers owned by the caller and a device-to-device clone of the last results: descriptors,
 * descriptor->extremum map, and the features as psx_feature_dev records (= popsift::Feature, 72 bytes)
 * whose desc[] point INTO d_descriptors, as Pyramid::clone_device_descriptors + prep_features leave them. */
/* pinned, GPU-mapped host memory (hipHostMalloc): cheap targets for psx_attach_export and sources for
 * psx_upload_*.  Allocation is slow (pool the buffers). */
int psx_host_alloc(size_t bytes, void** out);
/* the same with `device` made current on the calling thread first (device < 0: as psx_host_alloc): the HIP runtime
 * places pinned pages near the calling thread's current device or CPUs; a pool that serves device d allocates here. */
int psx_host_alloc_near(int device, size_t bytes, void** out);
int psx_host_free(void* ptr);
int psx_dev_alloc(int device, size_t bytes, void** out);
int psx_dev_free(int device, void* ptr);
/* synchronous device -> host copy of a buffer obtained from psx_dev_alloc / psx_clone_results */
int psx_dev_read(int device, void* host_dst, const void* dev_src, size_t bytes);
/* synchronous host -> device copy into such a buffer */
int psx_dev_write(int device, void* dev_dst, const void* host_src, size_t bytes);
int psx_clone_results(psx_ctx* ctx, void* d_features, void* d_descriptors, int* d_reverse_map);

/* FeaturesDev::match (features.cu:160-304, compute_distance / l2_in_t0): brute-force 2-nearest
 * neighbours of every left descriptor among the right ones, squared L2 distance evaluated with the
 * reference's operation tree, right side scanned in index order with strict '<' (ties keep the earlier
 * index).  d_left / d_right: DEVICE pointers to l_len / r_len descriptors of 128 floats (e.g.
 * psx_device_results / psx_clone_results).  host_match[3*i..3*i+2] = {best, second, accept} with
 * accept = (d_best / d_second < 0.8f), the int3 match_matrix of the reference; host_dist (may be NULL)
 * [2*i..2*i+1] = the two squared distances (what show_distance prints).  Synchronous. */
int psx_match(int device, const float* d_left, int l_len, const float* d_right, int r_len,
              int* host_match, float* host_dist);
/* Frees the calling thread's matcher scratch (a private stream and device buffers that psx_match keeps between
 * calls); optional -- the scratch is also released when the thread exits. */
int psx_match_release(void);

/* ---- byte descriptors ------------------------------------------------------------------
 * The form AliceVision's popSIFT describer hands on (setNormalizationMultiplier(9) and a conversion of every float
 * descriptor to unsigned char[128] on the host), and the byte convention of popsift-demo --write-as-uchar
 * (features.cu:310-330, which prints roundf of each float).  One rule everywhere:
 *     q = (uint8) min(255, max(0, roundf(d)))
 * d = the float the float path produces for that bin (after the normalisation and the norm_multi scale); roundf rounds
 * half away from zero.  Saturation at 255 is the one departure from the reference's text output. */
#define PSX_DESCFMT_F32 0   /* float descriptors (default) */
#define PSX_DESCFMT_U8  1   /* float descriptors AND their quantised bytes */

/* Descriptor format of a context's next extractions.  In byte mode the descriptor kernels also store the quantised
 * bytes into a device byte array of the context; the float array stays complete (psx_download, psx_device_results and
 * psx_clone_results are unchanged).  Any other value returns PSX_ERR_INVALID (ctx is not touched).  Switching to
 * PSX_DESCFMT_F32 detaches a byte export. */
int psx_set_descriptor_format(psx_ctx* ctx, int fmt);

/* psx_download with the bytes: num_features records and num_descriptors * 128 bytes (capacities in elements);
 * PSX_ERR_STATE when the context (or its last extraction) is in float mode.  Synchronises. */
int psx_download_u8(psx_ctx* ctx, psx_feature* features, int feature_capacity,
                    unsigned char* descriptors, int descriptor_capacity);

/* psx_attach_export / psx_attach_export_mapped for byte mode: the descriptor kernels stream the 128 bytes of each
 * descriptor into host_descriptors instead of floats.  Attaching a float export detaches the byte export and vice
 * versa; PSX_ERR_STATE in float mode. */
int psx_attach_export_u8(psx_ctx* ctx, psx_feature* host_features, int feature_capacity,
                         unsigned char* host_descriptors, int descriptor_capacity);
int psx_attach_export_mapped_u8(psx_ctx* ctx, psx_feature* host_features, int feature_capacity,
                                unsigned char* host_descriptors, int descriptor_capacity);

/* The rule above on n descriptors already on the device: d_src n*128 floats -> d_dst n*128 bytes (DEVICE pointers;
 * d_src 16-byte aligned, d_dst 4-byte aligned: the kernel reads float4 and writes 32-bit words).  Synchronous. */
int psx_quantize_desc(int device, const float* d_src, int n, unsigned char* d_dst);

/* FeaturesDev::match (features.cu:160-304) on byte descriptors: for every left descriptor the two right descriptors
 * that are smallest under the (squared distance, index) order -- what the reference's scan with strict '<' keeps,
 * ties to the earlier index.  Every quantity is an integer: a squared distance is at most 128 * 255^2 < 2^24, so the
 * reference's own float operation tree is exact on byte-valued inputs and this integer matcher (i8 MFMA on values
 * shifted by -128, i32 accumulation) returns the reference's result bit for bit.  d_left / d_right: DEVICE pointers
 * to l_len / r_len descriptors of 128 bytes, 16-byte aligned (rows are read as 16-byte vectors).  host_match[3*i..3*i+2] = {best, second, accept} with
 * accept = ((float)d_best / (float)d_second < 0.8f); host_dist (may be NULL) [2*i..2*i+1] = the two squared
 * distances, INT_MAX where psx_match reports +inf (r_len 0 or 1).  Scratch as psx_match (psx_match_release).
 * Synchronous. */
int psx_match_u8(int device, const unsigned char* d_left, int l_len, const unsigned char* d_right, int r_len,
                 int* host_match, int* host_dist);

/* ---- matches as data ---------------------------------------------------------------------
 * The directed matchers above answer per LEFT DESCRIPTOR; these answer with a compact list of PAIRS, filtered by a
 * caller-chosen ratio and optionally cross-checked (what OpenCV's BFMatcher(crossCheck=True) plus the ratio test, or
 * VLFeat's vl_ubcmatch(..., thresh), give).  One rule, shared by host and device (csrc/hip/match_rule.h); INTEGRATION.md
 * ("Matches as data") states it in words.  With F = psx_match(L, R) and B = psx_match(R, L) (psx_match_u8 for bytes), bit
 * for bit, left descriptor i yields the pair (i, j = F[i].best) iff
 *   1. r_len >= 1,
 *   2. (float)F[i].d1 / (float)F[i].d2 < ratio -- a float32 IEEE division and comparison (0/0 is NaN and fails, d2 = +inf
 *      gives 0 and passes; INT_MAX stands for +inf),
 *   3. with PSX_PAIRS_MUTUAL: B[j].best == i.
 * Pairs come out in ascending `left`: a stable, deterministic compaction.  {0.8f, 0} gives exactly the rows whose accept
 * flag is 1; ratio = INFINITY switches the ratio test off (except for NaN); with PSX_PAIRS_MUTUAL every left and every
 * right occurs at most once.
 * *count is always the TOTAL number of pairs that pass; the first min(*count, capacity) are written; capacity = 0 with a
 * NULL output asks "how many?".  l_len = 0 or r_len = 0 gives *count = 0 and PSX_OK.  PSX_ERR_INVALID, with nothing
 * touched: opts == NULL, a ratio that is NaN or <= 0, unknown flag bits, negative sizes, NULL data with a non-zero size,
 * count == NULL.  Descriptor pointers, alignment, scratch (psx_match_release) and thread safety as for psx_match /
 * psx_match_u8; a device output buffer is 16-byte aligned (one 16-byte store per record).  Synchronous. */
#define PSX_PAIRS_MUTUAL 1
typedef struct psx_match_opts    { float ratio; int flags; } psx_match_opts;           /* {0.8f, 0} = today's accept */
typedef struct psx_match_pair    { int left, right; float d1, d2; } psx_match_pair;    /* 16 bytes */
typedef struct psx_match_pair_u8 { int left, right; int   d1, d2; } psx_match_pair_u8; /* 16 bytes, INT_MAX = none */

/* *o = {0.8f, 0} */
int psx_match_opts_default(psx_match_opts* o);

/* host output: 16 bytes per PAIR come back instead of 20 per descriptor of both sides */
int psx_match_pairs(int device, const float* d_left, int l_len, const float* d_right, int r_len,
                    const psx_match_opts* opts, psx_match_pair* host_pairs, int capacity, int* count);
int psx_match_pairs_u8(int device, const unsigned char* d_left, int l_len, const unsigned char* d_right, int r_len,
                       const psx_match_opts* opts, psx_match_pair_u8* host_pairs, int capacity, int* count);
/* device output: the list stays in HBM (d_pairs: DEVICE pointer) for the caller's own kernels / a torch tensor; only
 * the count comes back */
int psx_match_pairs_dev(int device, const float* d_left, int l_len, const float* d_right, int r_len,
                        const psx_match_opts* opts, psx_match_pair* d_pairs, int capacity, int* count);
int psx_match_pairs_u8_dev(int device, const unsigned char* d_left, int l_len, const unsigned char* d_right, int r_len,
                           const psx_match_opts* opts, psx_match_pair_u8* d_pairs, int capacity, int* count);

/* The join alone, on HOST arrays: no device, no context (what the join kernel computes -- for tests and for callers
 * that already hold directed results).  fwd_match / fwd_dist: l_len rows as psx_match(L, R) returns them (3 ints, 2
 * distances); bwd_match: r_len rows of psx_match(R, L), may be NULL when PSX_PAIRS_MUTUAL is not set.  Additionally
 * PSX_ERR_INVALID when a best index lies outside [0, r_len), or a backward best outside [0, l_len), while that side is
 * non-empty: nothing is read out of bounds, nothing is written. */
int psx_pairs_join(const int* fwd_match, const float* fwd_dist, int l_len, const int* bwd_match, int r_len,
                   const psx_match_opts* opts, psx_match_pair* pairs, int capacity, int* count);
int psx_pairs_join_u8(const int* fwd_match, const int* fwd_dist, int l_len, const int* bwd_match, int r_len,
                      const psx_match_opts* opts, psx_match_pair_u8* pairs, int capacity, int* count);

/* ---- one descriptor set against many (byte descriptors) --------------------------------------
 * A view matched against dozens of others, a query against a shortlist, a frame against several keyframes: one left set
 * against n_sets right sets in ONE call -- one synchronisation and a number of kernel launches that does not grow with
 * n_sets, where a loop over psx_match_pairs_u8 pays both per set.  INTEGRATION.md ("One set against many") states the
 * rule in words.  d_left: DEVICE pointer to l_len descriptors of 128 bytes; d_rights / r_lens: HOST arrays of n_sets
 * entries, d_rights[k] a DEVICE pointer to r_lens[k] descriptors of 128 bytes.  Every device pointer is 16-byte aligned;
 * the sets may be separate allocations, slices of one buffer, or the same pointer more than once.
 * With P_k = the list psx_match_pairs_u8 returns for (L, R_k, opts) at unlimited capacity, bit for bit:
 *   - the result is the concatenation P_0, P_1, ..., P_{n_sets-1}: sets ascending, `left` ascending within a set;
 *   - `right` is the index WITHIN ITS SET;
 *   - set_counts[k] = |P_k| (HOST array of n_sets ints), always the set's total: set k starts at the sum of the counts
 *     before it;
 *   - *count = the sum of the |P_k|; the first min(*count, capacity) records of the concatenation are written, nothing at
 *     or past capacity; capacity = 0 with a NULL output asks "how many?".
 * n_sets = 0, l_len = 0 or an empty set give zero counts and PSX_OK; no device is touched when no pair can exist.
 * PSX_ERR_INVALID, with nothing touched and before any device call: everything psx_match_pairs_u8 refuses; n_sets < 0;
 * d_rights, r_lens or set_counts NULL with n_sets > 0; a negative r_lens[k]; a NULL d_rights[k] with r_lens[k] > 0;
 * n_sets * l_len or the sum of r_lens above INT_MAX.  Scratch (psx_match_release) and thread safety as for psx_match_u8.
 * Synchronous, with exactly one stream synchronisation per call.  The float form: psx_match_pairs_many, below ("one
 * descriptor set against many, float descriptors"). */
int psx_match_pairs_many_u8(int device, const unsigned char* d_left, int l_len,
                            const unsigned char* const* d_rights, const int* r_lens, int n_sets,
                            const psx_match_opts* opts, psx_match_pair_u8* host_pairs, int capacity,
                            int* set_counts, int* count);
/* the list stays in HBM: d_pairs is a DEVICE pointer, 16-byte aligned; set_counts and count are still HOST memory */
int psx_match_pairs_many_u8_dev(int device, const unsigned char* d_left, int l_len,
                                const unsigned char* const* d_rights, const int* r_lens, int n_sets,
                                const psx_match_opts* opts, psx_match_pair_u8* d_pairs, int capacity,
                                int* set_counts, int* count);

/* How the one-to-many search cuts its sides, on the HOST: no device, no context (csrc/hip/match_many_plan.h, the
 * function the library itself plans with -- for tests and for callers who want to see the launch shape).
 * backward = 0: the forward direction -- `chunks` cut the n_sets right sets (set = k), `blocks` cut L (set = 0);
 * backward = 1: the cross-check's direction -- `chunks` cut L (set = 0), `blocks` cut the right sets (set = k).
 * A chunk is rows [r0, r1) of one set, r0 a multiple of 32 and r1 - r0 <= 512, a set's chunks ascending and contiguous;
 * a block is rows [row0, row0 + 256) of one set, cut at the set's end.  Either table covers every row of every non-empty
 * set exactly once; nothing spans two sets; empty sets contribute nothing.  *chunk_count / *block_count are always the
 * totals; the first min(total, capacity) entries are written (capacity 0 with NULL: "how many?").  PSX_ERR_INVALID as
 * above for the sets, for a NULL count, a negative capacity, a NULL table with a capacity, backward not 0 or 1. */
typedef struct psx_many_chunk { int set, r0, r1; } psx_many_chunk;
typedef struct psx_many_block { int set, row0; } psx_many_block;
int psx_match_many_plan(int l_len, const int* r_lens, int n_sets, int backward,
                        psx_many_chunk* chunks, int chunk_capacity, int* chunk_count,
                        psx_many_block* blocks, int block_capacity, int* block_count);

/* ---- a list of view pairs over N descriptor sets (byte descriptors) ---------------------------
 * A structure-from-motion or loop-closure front end has N views and an EDGE LIST -- all pairs, a sliding window, a
 * retrieval shortlist per view --, not one left view.  n_edges ordered pairs of sets matched in ONE call: one
 * synchronisation and a number of kernel launches that grows neither with n_edges nor with n_sets; every set named by an
 * edge gets its norms once.  INTEGRATION.md ("A list of view pairs") has the words and the measured cost.
 * d_sets / lens: HOST arrays of n_sets entries, d_sets[s] a DEVICE pointer to lens[s] descriptors of 128 bytes, 16-byte
 * aligned (separate allocations, slices of one buffer, or the same pointer more than once); edges: HOST array of n_edges
 * {left, right} indices into the set array; edge_counts (n_edges ints) and count: HOST memory.
 * With P_e = the list psx_match_pairs_u8 returns for (d_sets[edges[e].left], d_sets[edges[e].right], opts) at unlimited
 * capacity, bit for bit:
 *   - the result is the concatenation P_0, P_1, ..., P_{n_edges-1} in the order of the edge list, which is neither sorted
 *     nor deduplicated: a duplicate edge returns the same list each time, (a, b) and (b, a) are two edges with two lists;
 *   - `left` and `right` index the edge's own two sets;
 *   - an edge with left == right is the single call with the same pointer on both sides (every row finds itself at
 *     distance 0); nothing is special-cased;
 *   - edge_counts[e] = |P_e|, *count their sum: always the totals.  The first min(*count, capacity) records are written --
 *     the cut may fall inside an edge --, nothing at or past capacity; capacity = 0 with a NULL output asks "how many?";
 *   - an edge with an empty side contributes nothing and has count 0.  Only sets named by an edge whose two sides are both
 *     non-empty are read.
 * When the edge list is grouped by `left`, the records of one left view's edges are contiguous: that slice, with its
 * edge_counts, is exactly what psx_match_pairs_many_u8 returns for that star, and goes into psx_ransac_*_many_dev and
 * psx_match_pairs_guided_many_u8_dev unchanged, offset into the device buffer.
 * n_edges = 0, or a call whose every edge has an empty side, gives zero counts and PSX_OK without touching a device.
 * PSX_ERR_INVALID, with nothing touched and before any device call: everything psx_match_pairs_u8 refuses about opts,
 * output, capacity and count; n_sets < 0 or n_edges < 0; d_sets or lens NULL with n_sets > 0; edges or edge_counts NULL
 * with n_edges > 0; a negative length; a NULL set pointer with a non-zero length; an edge index outside [0, n_sets) --
 * every edge is checked before anything runs, so n_sets = 0 admits no edge --; the sum over the edges of lens[left] (the
 * number of pairs that can exist) or of lens[right] (the backward rows) above INT_MAX.  PSX_ERR_NOMEM where a grid or a
 * table would not fit an int.  Scratch (psx_match_release) and thread safety as for psx_match_u8.  Synchronous, with
 * exactly one stream synchronisation per call.  The float form is psx_match_pairs_graph (below).  The next two links over the same edge list,
 * whatever its order: psx_ransac_*_graph* and psx_match_pairs_guided_graph_u8* ("A LIST OF VIEW PAIRS", below). */
typedef struct psx_view_edge { int left, right; } psx_view_edge;   /* indices into the set array */
int psx_match_pairs_graph_u8(int device, const unsigned char* const* d_sets, const int* lens, int n_sets,
                             const psx_view_edge* edges, int n_edges, const psx_match_opts* opts,
                             psx_match_pair_u8* host_pairs, int capacity, int* edge_counts, int* count);
/* the list stays in HBM: d_pairs is a DEVICE pointer, 16-byte aligned; edge_counts and count are still HOST memory */
int psx_match_pairs_graph_u8_dev(int device, const unsigned char* const* d_sets, const int* lens, int n_sets,
                                 const psx_view_edge* edges, int n_edges, const psx_match_opts* opts,
                                 psx_match_pair_u8* d_pairs, int capacity, int* edge_counts, int* count);

/* What the call above plans for these sizes, on the HOST: no device, no context (csrc/hip/match_graph_plan.h, the
 * functions the library itself plans with).  flags: psx_match_opts.flags.  Every referenced set (named by an edge whose
 * two sides are non-empty) is cut ONCE per call into outer blocks of 256 rows and inner chunks of whole tiles, at most
 * chunk_len <= 512 rows; the forward work items of edge e are blocks(left_e) x chunks(right_e), the backward ones (with
 * PSX_PAIRS_MUTUAL only) blocks(right_e) x chunks(left_e); one workgroup per item.  fwd_groups / bwd_groups: the runs of
 * whole edges whose per-chunk partials fit 256 MiB (a single edge above it is a group of its own); join_workgroups: the sum
 * over the edges of ceil(lens[left] / 256); launches: 1 (norms) + 2 per group + 3 (join), 0 when nothing runs;
 * scratch_bytes: the partials of the largest group.  PSX_ERR_INVALID as above for the sets and the edges, for unknown
 * flag bits, out == NULL. */
typedef struct psx_graph_plan_info { int referenced_sets, blocks, chunks, chunk_len;
                                     int fwd_items, bwd_items, fwd_groups, bwd_groups;
                                     int join_workgroups, launches;
                                     long long scratch_bytes; } psx_graph_plan_info;
int psx_match_graph_plan(const int* lens, int n_sets, const psx_view_edge* edges, int n_edges, int flags,
                         psx_graph_plan_info* out);

/* ---- one descriptor set against many (float descriptors) -------------------------------------
 * psx_match_pairs_many_u8's contract, word for word, with psx_match_pairs in place of psx_match_pairs_u8: d_left is a
 * DEVICE pointer to l_len descriptors of 128 floats, d_rights[k] one to r_lens[k] descriptors (d_rights / r_lens: HOST
 * arrays of n_sets entries); every device pointer is 16-byte aligned; the sets may be separate allocations, slices of one
 * buffer, or the same pointer more than once.  With P_k = the list psx_match_pairs returns for (L, R_k, opts) at unlimited
 * capacity, bit for bit (float distances compared as bit patterns):
 *   - the result is the concatenation P_0, P_1, ..., P_{n_sets-1}: sets ascending, `left` ascending within a set;
 *   - `right` is the index WITHIN ITS SET; ties keep the earlier index, a NaN distance never wins, 0/0 fails the ratio
 *     test, a missing second neighbour is +inf;
 *   - set_counts[k] = |P_k| (HOST array of n_sets ints), always the set's total;
 *   - *count = the sum of the |P_k|; the first min(*count, capacity) records of the concatenation are written, nothing at
 *     or past capacity; capacity = 0 with a NULL output asks "how many?".
 * n_sets = 0, l_len = 0 or an empty set give zero counts and PSX_OK; no device is touched when no pair can exist.
 * PSX_ERR_INVALID, with nothing touched and before any device call: everything psx_match_pairs refuses; n_sets < 0;
 * d_rights, r_lens or set_counts NULL with n_sets > 0; a negative r_lens[k]; a NULL d_rights[k] with r_lens[k] > 0;
 * n_sets * l_len or the sum of r_lens above INT_MAX.  Scratch (psx_match_release) and thread safety as for psx_match.
 * Two paths, one result ("One set against many", the float subsection): the MFMA prefilter over all sets
 * when POPSIFT_MATCH_MFMA is on, l_len >= 256 and the sum of r_lens >= 4096 -- the single call's two thresholds on the
 * call's totals --, the exact scan of every pair otherwise.  Synchronous: ONE stream synchronisation per call; a second
 * one only when the prefilter's flag comes back up (a candidate segment overflowed, or a norm is zero, infinite or NaN)
 * and the whole call is repeated by the exact scan.  The number of kernel launches does not grow with n_sets. */
int psx_match_pairs_many(int device, const float* d_left, int l_len,
                         const float* const* d_rights, const int* r_lens, int n_sets,
                         const psx_match_opts* opts, psx_match_pair* host_pairs, int capacity,
                         int* set_counts, int* count);
/* the list stays in HBM: d_pairs is a DEVICE pointer, 16-byte aligned; set_counts and count are still HOST memory */
int psx_match_pairs_many_dev(int device, const float* d_left, int l_len,
                             const float* const* d_rights, const int* r_lens, int n_sets,
                             const psx_match_opts* opts, psx_match_pair* d_pairs, int capacity,
                             int* set_counts, int* count);

/* What psx_match_pairs_many decides for these sizes, on the HOST: no device, no context (csrc/hip/match_many_f32_plan.h,
 * the function the library itself plans with).  flags: psx_match_opts.flags; mfma_enabled: 1 as POPSIFT_MATCH_MFMA's
 * default, 0 as POPSIFT_MATCH_MFMA=0.  path: 1 the exact scan, 2 the prefilter (0: no pair can exist, nothing runs);
 * fwd_groups / bwd_groups: the groups of whole sets each direction is walked in (bwd_groups = 0 without the
 * cross-check); launches: the kernels queued when the flag stays down; scratch_bytes: the largest group's share of the
 * one buffer that grows with (chunks x outer rows), at most 256 MiB unless a single set exceeds it.  PSX_ERR_INVALID as
 * above for the sets, for unknown flag bits, mfma_enabled not 0 or 1, out == NULL. */
typedef struct psx_many_f32_plan { int path;        /* 1 scan, 2 prefilter */
                                   int fwd_groups, bwd_groups;
                                   int launches;    /* kernels queued when the flag stays down */
                                   long long scratch_bytes; } psx_many_f32_plan;
int psx_match_many_f32_plan(int l_len, const int* r_lens, int n_sets, int flags, int mfma_enabled,
                            psx_many_f32_plan* out);
/* The calling thread's last psx_match_pairs_many / _dev call that passed its argument checks (zeros before any): the
 * path it planned, whether the flag came back up and the scan repeated the call, and the kernels launched and stream
 * synchronisations made, counted where the call launches and synchronises.  PSX_ERR_INVALID for out == NULL. */
typedef struct psx_many_f32_info { int path, fell_back, launches, syncs; } psx_many_f32_info;
int psx_match_many_f32_last(psx_many_f32_info* out);

/* ---- a list of view pairs over N descriptor sets (float descriptors) --------------------------
 * The float form of psx_match_pairs_graph_u8: its contract, word for word, with psx_match_pairs in place of
 * psx_match_pairs_u8.  d_sets[s] is a DEVICE pointer to lens[s] descriptors of 128 floats, 16-byte aligned (separate
 * allocations, slices of one buffer, or the same pointer more than once).  With P_e = the list psx_match_pairs returns for
 * (d_sets[edges[e].left], d_sets[edges[e].right], opts) at unlimited capacity, bit for bit (float distances compared as bit
 * patterns):
 *   - the result is the concatenation P_0, P_1, ..., P_{n_edges-1} in the order of the edge list, which is neither sorted
 *     nor deduplicated; a duplicate, both orders of a pair and left == right are ordinary edges, nothing is special-cased;
 *   - ties keep the earlier index, a NaN distance never wins, 0/0 fails the ratio test, a missing second neighbour is +inf;
 *   - edge_counts[e] = |P_e|, *count their sum: always the totals.  The first min(*count, capacity) records are written --
 *     the cut may fall inside an edge --, nothing at or past capacity; capacity = 0 with a NULL output asks "how many?";
 *   - an edge with an empty side contributes nothing and has count 0.  Only sets named by an edge whose two sides are both
 *     non-empty are read.
 * Empty forms (no device is touched), PSX_ERR_INVALID (nothing touched, before any device call) and the pointer rules are
 * psx_match_pairs_graph_u8's; PSX_ERR_NOMEM where a table, a grid, a row's place among the rows of all referenced sets
 * or 32 x a group's candidate segments would not fit an int.  Scratch (psx_match_release) and thread safety as for
 * psx_match.  Two paths, one result, as psx_match_pairs_many ("A list of view pairs", the float subsection):
 * with the LIVE edges -- both sides non-empty, counted as listed -- the MFMA prefilter runs when POPSIFT_MATCH_MFMA is on,
 * the sum of lens[right] is at least 4096 and the sum of lens[left] at least 256 x the number of live edges (for a star:
 * psx_match_pairs_many's rule), the exact scan of every pair otherwise; one decision per call for both directions.  Every
 * referenced set gets its permuted copy, or its norms and f16 copy, ONCE per call.  Synchronous: ONE stream synchronisation
 * per call; a second one only when the prefilter's flag comes back up (a candidate segment overflowed, or a norm is zero
 * everywhere, infinite or NaN) and the whole call is repeated by the exact scan.  The number of kernel launches grows
 * neither with n_edges nor with n_sets.  The records go into psx_ransac_*_graph*, psx_match_pairs_guided_graph* and
 * psx_tracks_graph* as the byte call's do. */
int psx_match_pairs_graph(int device, const float* const* d_sets, const int* lens, int n_sets,
                          const psx_view_edge* edges, int n_edges, const psx_match_opts* opts,
                          psx_match_pair* host_pairs, int capacity, int* edge_counts, int* count);
/* the list stays in HBM: d_pairs is a DEVICE pointer, 16-byte aligned; edge_counts and count are still HOST memory */
int psx_match_pairs_graph_dev(int device, const float* const* d_sets, const int* lens, int n_sets,
                              const psx_view_edge* edges, int n_edges, const psx_match_opts* opts,
                              psx_match_pair* d_pairs, int capacity, int* edge_counts, int* count);

/* What psx_match_pairs_graph decides for these sizes, on the HOST: no device, no context (csrc/hip/match_graph_f32_plan.h,
 * the functions the library itself plans with); the float counterpart of psx_match_graph_plan and psx_match_many_f32_plan.
 * flags: psx_match_opts.flags; mfma_enabled: 1 as POPSIFT_MATCH_MFMA's default, 0 as POPSIFT_MATCH_MFMA=0.  path: 1 the
 * exact scan, 2 the prefilter (0: no edge is live, nothing runs and every other field is 0).  Every referenced set is cut
 * ONCE per call into `blocks` outer blocks of 256 rows and `chunks` inner chunks of at most chunk_len rows: whole tiles, at
 * most 512 rows, on the scan path; on the prefilter path whole staged blocks of 64 rows, the smallest length between 512
 * and 4096 at which the direction with fewer items has at most 768 of them (4096 if none does).  fwd_items / bwd_items:
 * blocks(outer) x chunks(inner) summed over the edges, one workgroup each (bwd: PSX_PAIRS_MUTUAL only); fwd_groups /
 * bwd_groups: the runs of whole edges whose share of the one buffer that grows with (chunks x outer rows) -- 16 bytes per
 * entry on the scan path, 264 on the prefilter path -- fits 256 MiB (a single edge above it is a group of its own);
 * join_workgroups: the sum over the live edges of ceil(lens[left] / 256); launches: the kernels queued when the flag stays
 * down, 1 or 2 + 2 per group + 3; scratch_bytes: that buffer for the largest group.  PSX_ERR_INVALID as above for the sets
 * and the edges, for unknown flag bits, mfma_enabled not 0 or 1, out == NULL; PSX_ERR_NOMEM as the call. */
typedef struct psx_graph_f32_plan_info { int path;        /* 1 scan, 2 prefilter */
                                         int referenced_sets, blocks, chunks, chunk_len;
                                         int fwd_items, bwd_items, fwd_groups, bwd_groups;
                                         int join_workgroups, launches;
                                         long long scratch_bytes; } psx_graph_f32_plan_info;
int psx_match_graph_f32_plan(const int* lens, int n_sets, const psx_view_edge* edges, int n_edges, int flags,
                             int mfma_enabled, psx_graph_f32_plan_info* out);
/* The calling thread's last psx_match_pairs_graph / _dev call that passed its argument checks (zeros before any), as
 * psx_match_many_f32_last reports the one-to-many call's.  PSX_ERR_INVALID for out == NULL. */
int psx_match_graph_f32_last(psx_many_f32_info* out);

/* ---- guided matching ---------------------------------------------------------------------
 * The 2-NN search restricted by what the caller knows about where a match can lie (AliceVision's guidedMatching, a
 * stereo search window, a tracker's prediction; the reference has no counterpart): a homography -- identity H is a plain
 * search window of radius tol -- or a fundamental matrix.  Every left descriptor ranks only its ADMISSIBLE right
 * descriptors; filtering the unguided matcher's pairs afterwards is not the same result (a left descriptor whose globally
 * nearest right one is inadmissible is lost there, and its ratio test ran against a neighbour the geometry excludes).
 * One rule, shared by host and device (csrc/hip/guide_rule.h); INTEGRATION.md ("Guided matching") states it in words.
 * Positions are in INPUT-IMAGE units, as psx_feature reports them.  With left position (xl, yl), right position
 * (xr, yr), float32 arithmetic only, every operation rounded on its own in exactly this order (no fused multiply-add,
 * no division, no square root):
 *     a = (m0*xl + m1*yl) + m2;   b = (m3*xl + m4*yl) + m5;   c = (m6*xl + m7*yl) + m8
 *     HOMOGRAPHY: allowed iff  c > 0  and  (dx*dx + dy*dy) <= (tol*c)*(tol*c),   dx = a - c*xr,  dy = b - c*yr
 *     EPIPOLAR:   e = (a*xr + b*yr) + c;   allowed iff  e*e <= (tol*tol) * (a*a + b*b)
 * The IEEE result of the comparison is the rule: any NaN makes a pair inadmissible.  The relation is defined on (left i,
 * right j) and is NOT symmetric in its roles: the backward pass of a cross-check evaluates the SAME relation with the
 * loops exchanged and never a transposed or inverted matrix.
 * A guide is valid iff kind is 1 or 2, all nine entries are finite and tol is finite and >= 0; anything else is
 * PSX_ERR_INVALID, with nothing touched. */
#define PSX_GUIDE_HOMOGRAPHY 1   /* m = H, row major: right point within tol of H * left point            */
#define PSX_GUIDE_EPIPOLAR   2   /* m = F, row major: right point within tol of the line F * left point   */
typedef struct psx_guide { int kind; float m[9]; float tol; } psx_guide;   /* positions in INPUT-IMAGE units, as psx_feature reports them */

/* The rule on the host, no device and no context: allowed[i * nr + j] = 1 where (left i, right j) is admissible, else 0.
 * left_xy / right_xy: nl / nr (x, y) pairs.  PSX_ERR_INVALID for an invalid guide, negative sizes, or a NULL array with
 * a non-zero size (allowed is needed when nl * nr > 0). */
int psx_guide_allows(const psx_guide* guide, const float* left_xy, int nl, const float* right_xy, int nr,
                     unsigned char* allowed);

/* d_xy[2k], d_xy[2k+1] = xpos, ypos of the feature that descriptor k belongs to: a gather over what psx_clone_results
 * leaves (d_features: its psx_feature_dev records, d_reverse_map: its descriptor -> feature map; every entry must index
 * a record).  All three are DEVICE pointers, d_xy to 2 n_desc floats, 8-byte aligned.  Synchronous. */
int psx_desc_positions(int device, const psx_feature_dev* d_features, const int* d_reverse_map, int n_desc, float* d_xy);

/* psx_match / psx_match_u8 with every left descriptor's search restricted to its admissible right descriptors: the two
 * smallest under (distance, index) order among them.  Output layout and conventions are exactly those of psx_match /
 * psx_match_u8: float distances from the reference's operation tree, bit for bit, byte distances exact integers; a
 * missing neighbour is +inf / INT_MAX with index 0 -- which now also arises with zero or one admissible right
 * descriptor; accept = (d1 / d2 < 0.8f).  An admissible right descriptor whose distance is NaN (a NaN value in either
 * row) or overflows to +inf is never a neighbour: the reference's scan keeps a candidate only on a strict '<' against
 * +inf, which neither passes, so such a row is skipped as if it were inadmissible.
 * d_left_xy / d_right_xy: DEVICE pointers to l_len / r_len (x, y) pairs, 8-byte aligned (psx_desc_positions writes them).  Additionally PSX_ERR_INVALID for an invalid guide or a NULL position array
 * with a non-zero length.  Scratch as psx_match (psx_match_release).  Synchronous. */
int psx_match_guided(int device, const float* d_left, const float* d_left_xy, int l_len,
                     const float* d_right, const float* d_right_xy, int r_len, const psx_guide* guide,
                     int* host_match, float* host_dist);
int psx_match_guided_u8(int device, const unsigned char* d_left, const float* d_left_xy, int l_len,
                        const unsigned char* d_right, const float* d_right_xy, int r_len, const psx_guide* guide,
                        int* host_match, int* host_dist);

/* psx_match_pairs and its three siblings on guided directed passes: F = the guided L -> R pass; with PSX_PAIRS_MUTUAL
 * B = the guided R -> L pass on the SAME relation (right descriptor j ranks the left descriptors i with (i, j)
 * admissible); then the join and compaction of psx_match_pairs, unchanged.  Record types, ordering, capacity and "how
 * many?" semantics, empty sides, argument errors and scratch are as documented there; additionally PSX_ERR_INVALID for
 * an invalid guide or a NULL position array with a non-zero length. */
int psx_match_pairs_guided(int device, const float* d_left, const float* d_left_xy, int l_len,
                           const float* d_right, const float* d_right_xy, int r_len, const psx_guide* guide,
                           const psx_match_opts* opts, psx_match_pair* host_pairs, int capacity, int* count);
int psx_match_pairs_guided_u8(int device, const unsigned char* d_left, const float* d_left_xy, int l_len,
                              const unsigned char* d_right, const float* d_right_xy, int r_len, const psx_guide* guide,
                              const psx_match_opts* opts, psx_match_pair_u8* host_pairs, int capacity, int* count);
int psx_match_pairs_guided_dev(int device, const float* d_left, const float* d_left_xy, int l_len,
                               const float* d_right, const float* d_right_xy, int r_len, const psx_guide* guide,
                               const psx_match_opts* opts, psx_match_pair* d_pairs, int capacity, int* count);
int psx_match_pairs_guided_u8_dev(int device, const unsigned char* d_left, const float* d_left_xy, int l_len,
                                  const unsigned char* d_right, const float* d_right_xy, int r_len, const psx_guide* guide,
                                  const psx_match_opts* opts, psx_match_pair_u8* d_pairs, int capacity, int* count);

/* GUIDED RE-MATCH OF MANY SETS IN ONE CALL (byte descriptors).  The third link of match -> verify -> re-match for one
 * view against n_sets others: psx_match_pairs_many_u8* leaves K pair lists, psx_ransac_*_many* K models,
 * psx_guides_from_ransac (below, after the batched RANSAC) turns them into K guides, and this call re-matches all K sets,
 * each under its OWN guide -- one stream synchronisation and a number of kernel launches that does not grow with n_sets
 * (4 without the cross-check, 6 with it), where a loop over psx_match_pairs_guided_u8_dev pays 3 / 5 launches, a
 * synchronisation and a count read-back per set.  INTEGRATION.md ("Guided re-match of many sets") has the words and the
 * measured cost.  d_left / d_left_xy: DEVICE pointers to l_len descriptors of 128 bytes / l_len (x, y) pairs; d_rights,
 * d_right_xys, r_lens: HOST arrays of n_sets entries, d_rights[k] / d_right_xys[k] DEVICE pointers to r_lens[k]
 * descriptors / positions; guides: HOST array of n_sets guides, guides[k] for set k.  Descriptor pointers are 16-byte
 * aligned, position pointers 8-byte aligned; the sets may be separate allocations, slices of one buffer, or the same
 * pointer more than once, possibly under different guides.
 * With G_k = the list psx_match_pairs_guided_u8 returns for (L, L_xy, R_k, R_xy_k, guides[k], opts) at unlimited capacity,
 * bit for bit:
 *   - the result is the concatenation G_0, G_1, ..., G_{n_sets-1}: sets ascending, `left` ascending within a set;
 *   - `right` is the index WITHIN ITS SET;
 *   - set_counts[k] = |G_k| (HOST array of n_sets ints), always the set's total;
 *   - *count = the sum of the |G_k|; the first min(*count, capacity) records of the concatenation are written, nothing at
 *     or past capacity; capacity = 0 with a NULL output asks "how many?".
 * A set whose guide has kind == PSX_GUIDE_NONE is SKIPPED: it contributes nothing, its count is 0, none of its arrays is
 * read and its d_rights[k] / d_right_xys[k] may be NULL (the rest of that guide is not looked at).  This is how "no model"
 * is said: psx_ransac_*_many reports a set it could not verify with best = -1 and a ZERO matrix, and a zero matrix is a
 * valid guide -- it admits nothing as a homography and EVERYTHING as an epipolar guide.  psx_guides_from_ransac maps such a
 * result to kind 0.  The single-set calls keep refusing kind 0.
 * n_sets = 0, l_len = 0, and a call whose sets are all empty or all skipped give zero counts and PSX_OK without touching
 * a device.  PSX_ERR_INVALID, with nothing touched and before any device call: everything psx_match_pairs_guided_u8 and
 * psx_match_pairs_many_u8 refuse; guides, d_rights, d_right_xys, r_lens or set_counts NULL with n_sets > 0; d_left or
 * d_left_xy NULL with l_len > 0; any guide that is neither valid nor of kind 0 -- EVERY guide is checked before anything
 * runs; a NULL d_rights[k] or d_right_xys[k] for a set that is not skipped and has rows.  PSX_ERR_NOMEM where a grid would
 * not fit an int.  The call runs as psx_match_pairs_guided_graph_u8 on the star -- sets [left, rights...], edges {0, k + 1}
 * --, whose forward search takes 64 workgroups per 256 left rows of every set that is neither skipped nor empty: with
 * tens of millions of such sets of a handful of left rows each, 64 * (those sets) * ceil(l_len / 256) passes INT_MAX and
 * the call returns PSX_ERR_NOMEM where it ran when the star had a grid of n_sets * ceil(l_len / 4) workgroups of its own.
 * Scratch (psx_match_release) and thread safety as for psx_match_u8.  Synchronous, with exactly one stream synchronisation per call.  The float form
 * is psx_match_pairs_guided_many (below). */
#define PSX_GUIDE_NONE 0         /* in the *_many and *_graph calls only: this set / edge is skipped */
int psx_match_pairs_guided_many_u8(int device, const unsigned char* d_left, const float* d_left_xy, int l_len,
                                   const unsigned char* const* d_rights, const float* const* d_right_xys, const int* r_lens,
                                   int n_sets, const psx_guide* guides, const psx_match_opts* opts,
                                   psx_match_pair_u8* host_pairs, int capacity, int* set_counts, int* count);
/* the list stays in HBM: d_pairs is a DEVICE pointer, 16-byte aligned; set_counts and count are still HOST memory */
int psx_match_pairs_guided_many_u8_dev(int device, const unsigned char* d_left, const float* d_left_xy, int l_len,
                                       const unsigned char* const* d_rights, const float* const* d_right_xys, const int* r_lens,
                                       int n_sets, const psx_guide* guides, const psx_match_opts* opts,
                                       psx_match_pair_u8* d_pairs, int capacity, int* set_counts, int* count);
/* The float form of psx_match_pairs_guided_many_u8: the same signature and contract, word for word, with descriptors of 128
 * floats (16-byte aligned), psx_match_pair records and psx_match_pairs_guided as the single call -- set k yields, bit for
 * bit (float distances compared as bit patterns), what psx_match_pairs_guided returns for (L, R_k) under guides[k].  The
 * same driver on (float, float): 4 kernel launches, 6 with the cross-check, one stream synchronisation. */
int psx_match_pairs_guided_many(int device, const float* d_left, const float* d_left_xy, int l_len,
                                const float* const* d_rights, const float* const* d_right_xys, const int* r_lens,
                                int n_sets, const psx_guide* guides, const psx_match_opts* opts,
                                psx_match_pair* host_pairs, int capacity, int* set_counts, int* count);
/* the list stays in HBM: d_pairs is a DEVICE pointer, 16-byte aligned; set_counts and count are still HOST memory */
int psx_match_pairs_guided_many_dev(int device, const float* d_left, const float* d_left_xy, int l_len,
                                    const float* const* d_rights, const float* const* d_right_xys, const int* r_lens,
                                    int n_sets, const psx_guide* guides, const psx_match_opts* opts,
                                    psx_match_pair* d_pairs, int capacity, int* set_counts, int* count);

/* ---- geometric verification ---------------------------------------------------------------
 * The step between a match and a guided re-match: a homography estimated from the pair list by RANSAC on the device
 * (OpenCV's findHomography(RANSAC), the model AliceVision's guidedMatching starts from; the reference has no
 * counterpart).  match -> verify -> re-match guided by the verified model, without the pairs leaving HBM.  Every step
 * is a stated rule, shared by host and device (csrc/hip/ransac_rule.h states it operation by operation;
 * INTEGRATION.md, "Geometric verification", in words), so the device result equals psx_ransac_homography_ref bit for bit:
 *   1. samples:  hypothesis h draws four distinct pair indices from an integer hash of (seed, h);
 *   2. fit:      the four correspondences (and, for the refit, any n >= 4) give a 3 x 3 matrix by normalised DLT --
 *                normal equations, LDL^T without pivoting, in double, rounded once to float32; a degenerate sample gives
 *                NaN / inf entries, there is no special case;
 *   3. score:    count[h] = number of pairs that pass the HOMOGRAPHY rule of guided matching (psx_guide) under model h
 *                and opts->tol; a model with a non-finite entry scores 0;
 *   4. select:   the largest count, ties to the lowest h;
 *   5. refit (PSX_RANSAC_REFIT), one round: fit the winner's inliers (when there are at least 4) in pair order; that
 *                model is kept iff it is finite and its count is >= the winner's;
 *   6. inliers:  the input records that pass the rule under the kept model, compacted stably in input order.
 * Pair records are 16 bytes (psx_match_pair or psx_match_pair_u8: only left and right are read, the record is copied
 * whole); pair p is the correspondence left_xy[pairs[p].left] -> right_xy[pairs[p].right], positions in INPUT-IMAGE units
 * as psx_desc_positions writes them.  The result's m is a valid psx_guide matrix for PSX_GUIDE_HOMOGRAPHY (left -> right).
 * result->best = winning hypothesis, sample_inliers = its count, inliers = the count under the kept model (== *count),
 * refit_kept = 1 when the refit model replaced the sample model.  n < 4, or a kept model with a non-finite entry (every
 * sample degenerate), gives PSX_OK with best = -1, a zero matrix, *count = 0 and no record written.
 * *count, capacity and the "how many?" form are as in psx_match_pairs.  PSX_ERR_INVALID, with nothing touched: opts, result
 * or count NULL, a tol that is NaN, negative or infinite, hypotheses outside [1, 65536], unknown flag bits, negative
 * sizes, NULL data with a non-zero size, a pair index outside its position array. */
#define PSX_RANSAC_REFIT 1
typedef struct psx_ransac_opts   { float tol; int hypotheses; unsigned seed; int flags; } psx_ransac_opts;
typedef struct psx_ransac_result { float m[9]; int best; int sample_inliers; int inliers; int refit_kept; } psx_ransac_result;

/* *o = {2.0f, 1024, 0, PSX_RANSAC_REFIT} */
int psx_ransac_opts_default(psx_ransac_opts* o);

/* Host only, no device and no context (as psx_pairs_join). */
/* step 1: idx[4 * i .. 4 * i + 3] = the four pair indices of hypothesis first + i, in draw order, for i in [0, count);
 * PSX_ERR_INVALID for n < 4, first < 0, count < 0, first + count > 65536 or a NULL idx with count > 0 */
int psx_ransac_samples(unsigned seed, int first, int count, int n, int* idx);
/* step 2 on n >= 4 correspondences left_xy[i] -> right_xy[i] ((x, y) pairs), in the given order; m: 9 floats, row major */
int psx_homography_fit(const float* left_xy, const float* right_xy, int n, float* m);
/* the whole rule on host arrays: left_xy / right_xy hold nl / nr positions; models (N x 9 floats) and counts (N ints)
 * receive every hypothesis' model and count, either may be NULL */
int psx_ransac_homography_ref(const void* pairs, int n, const float* left_xy, int nl, const float* right_xy, int nr,
                              const psx_ransac_opts* opts, psx_ransac_result* result, void* inliers, int capacity, int* count,
                              float* models, int* counts);

/* On the device.  d_left_xy / d_right_xy: DEVICE pointers to l_len / r_len (x, y) pairs, 8-byte aligned.  The host form
 * uploads n records from host memory and returns the inliers to a host buffer; the _dev form reads the records from and
 * writes the inliers to DEVICE memory (16-byte aligned; d_inliers must not overlap d_pairs), so the list psx_match_pairs*_dev left
 * never leaves HBM.  The result struct always comes back to the host; host_models (N x 9 floats) and host_counts (N
 * ints) expose the per-hypothesis layers, either may be NULL.  Scratch as psx_match (psx_match_release).  Synchronous. */
int psx_ransac_homography(int device, const void* host_pairs, int n, const float* d_left_xy, int l_len,
                          const float* d_right_xy, int r_len, const psx_ransac_opts* opts, psx_ransac_result* result,
                          void* host_inliers, int capacity, int* count, float* host_models, int* host_counts);
int psx_ransac_homography_dev(int device, const void* d_pairs, int n, const float* d_left_xy, int l_len,
                              const float* d_right_xy, int r_len, const psx_ransac_opts* opts, psx_ransac_result* result,
                              void* d_inliers, int capacity, int* count, float* host_models, int* host_counts);

/* The same for the general two-view case, a scene with depth: a FUNDAMENTAL MATRIX (OpenCV's findFundamentalMat(RANSAC)),
 * the producer of guided matching's other guide.  The result's m is a valid psx_guide matrix for PSX_GUIDE_EPIPOLAR
 * (left -> right: (xr yr 1) m (xl yl 1)^T = 0), ready for psx_match_pairs_guided*.  The rule has the same six steps, stated
 * operation by operation in csrc/hip/fundamental_rule.h ("Geometric verification", in words), and the
 * device result equals psx_ransac_fundamental_ref bit for bit:
 *   1. samples:  EIGHT distinct pair indices per hypothesis, by the same hash;
 *   2. fit:      the normalised 8-point algorithm for n >= 8 correspondences -- the 9 x 9 moment matrix, LDL^T with
 *                diagonal pivoting (the entry fixed at 1 is whichever the pivoting leaves over), four Newton steps on the
 *                determinant for rank 2 -- in double, rounded once to float32; no special case for a degenerate sample;
 *   3. score:    the EPIPOLAR rule of guided matching under opts->tol (one-sided: what is verified is what will guide); a
 *                model with a non-finite entry, or with all nine entries zero, scores 0;
 *   4 - 6.       as above with 8 in place of 4; the refit model is kept iff it may score and its count is >= the winner's.
 * n < 8, or a kept model that may not score, gives PSX_OK with best = -1, a zero matrix, *count = 0.  Arguments, opts,
 * result, capacity and errors are those of the homography calls. */
/* Host only.  step 1 with k draws per hypothesis, k = 2, 3, 4 (== psx_ransac_samples) or 8: idx[k * i ..]; the draws of a
 * smaller k are the first k of a larger one's.  PSX_ERR_INVALID for another k, n < k, and as psx_ransac_samples */
int psx_ransac_samples_k(unsigned seed, int first, int count, int n, int k, int* idx);
/* step 2 on n >= 8 correspondences left_xy[i] -> right_xy[i], in the given order; m: 9 floats, row major */
int psx_fundamental_fit(const float* left_xy, const float* right_xy, int n, float* m);
int psx_ransac_fundamental_ref(const void* pairs, int n, const float* left_xy, int nl, const float* right_xy, int nr,
                               const psx_ransac_opts* opts, psx_ransac_result* result, void* inliers, int capacity, int* count,
                               float* models, int* counts);
int psx_ransac_fundamental(int device, const void* host_pairs, int n, const float* d_left_xy, int l_len,
                           const float* d_right_xy, int r_len, const psx_ransac_opts* opts, psx_ransac_result* result,
                           void* host_inliers, int capacity, int* count, float* host_models, int* host_counts);
int psx_ransac_fundamental_dev(int device, const void* d_pairs, int n, const float* d_left_xy, int l_len,
                               const float* d_right_xy, int r_len, const psx_ransac_opts* opts, psx_ransac_result* result,
                               void* d_inliers, int capacity, int* count, float* host_models, int* host_counts);

/* The same for the two registration models below a homography: a 2-D AFFINE transform (3 pairs; OpenCV's
 * estimateAffine2D) and a 2-D SIMILARITY (rotation, uniform scale, translation; 2 pairs; OpenCV's
 * estimateAffinePartial2D).  A pair list too short for a homography -- 2 or 3 correct pairs -- still gives a model, fewer
 * hypotheses are needed at the same outlier rate, and no degree of freedom is spent on perspective the scene does not
 * have.  The result's m is a valid psx_guide matrix for PSX_GUIDE_HOMOGRAPHY (left -> right) whose last row is EXACTLY
 * (0, 0, 1): psx_guides_from_ransac(..., PSX_GUIDE_HOMOGRAPHY, ...) and psx_match_pairs_guided* take it as it is.  A
 * similarity has m[0] == m[4] and m[1] == -m[3] up to the final rounding: it cannot represent a reflection (a mirrored
 * scene needs the affine model).  The rule has the same six steps, stated operation by operation in
 * csrc/hip/affine_rule.h ("Geometric verification", in words), and the device result equals
 * psx_ransac_affine_ref / psx_ransac_similarity_ref bit for bit:
 *   1. samples:  the first THREE (affine) or TWO (similarity) of the homography's four draws, by the same hash;
 *   2. fit:      both sides normalised as for the homography; affine: the 3 x 3 normal equations with two right-hand
 *                sides, LDL^T without pivoting; similarity: the closed form p = sum(x*u + y*v) / sum(x*x + y*y),
 *                q = sum(x*v - y*u) / sum(x*x + y*y), rows (p, -q, 0), (q, p, 0) -- in double, rounded once to float32;
 *                no special case for a degenerate sample (a repeated or collinear left point gives non-finite entries);
 *   3 - 6.       as for the homography, the HOMOGRAPHY rule of guided matching, with 3 / 2 in place of 4.
 * n < 3 / n < 2, or a kept model with a non-finite entry, gives PSX_OK with best = -1, a zero matrix, *count = 0.
 * Arguments, opts, result, capacity, the host_models / host_counts layers and errors are those of the homography calls;
 * psx_affine_fit needs n >= 3 and psx_similarity_fit n >= 2 (PSX_ERR_INVALID otherwise). */
int psx_affine_fit(const float* left_xy, const float* right_xy, int n, float* m);
int psx_ransac_affine_ref(const void* pairs, int n, const float* left_xy, int nl, const float* right_xy, int nr,
                          const psx_ransac_opts* opts, psx_ransac_result* result, void* inliers, int capacity, int* count,
                          float* models, int* counts);
int psx_ransac_affine(int device, const void* host_pairs, int n, const float* d_left_xy, int l_len,
                      const float* d_right_xy, int r_len, const psx_ransac_opts* opts, psx_ransac_result* result,
                      void* host_inliers, int capacity, int* count, float* host_models, int* host_counts);
int psx_ransac_affine_dev(int device, const void* d_pairs, int n, const float* d_left_xy, int l_len,
                          const float* d_right_xy, int r_len, const psx_ransac_opts* opts, psx_ransac_result* result,
                          void* d_inliers, int capacity, int* count, float* host_models, int* host_counts);
int psx_similarity_fit(const float* left_xy, const float* right_xy, int n, float* m);
int psx_ransac_similarity_ref(const void* pairs, int n, const float* left_xy, int nl, const float* right_xy, int nr,
                              const psx_ransac_opts* opts, psx_ransac_result* result, void* inliers, int capacity, int* count,
                              float* models, int* counts);
int psx_ransac_similarity(int device, const void* host_pairs, int n, const float* d_left_xy, int l_len,
                          const float* d_right_xy, int r_len, const psx_ransac_opts* opts, psx_ransac_result* result,
                          void* host_inliers, int capacity, int* count, float* host_models, int* host_counts);
int psx_ransac_similarity_dev(int device, const void* d_pairs, int n, const float* d_left_xy, int l_len,
                              const float* d_right_xy, int r_len, const psx_ransac_opts* opts, psx_ransac_result* result,
                              void* d_inliers, int capacity, int* count, float* host_models, int* host_counts);

/* MANY LISTS IN ONE CALL.  psx_match_pairs_many_u8* leaves the concatenation P_0 .. P_{K-1} of K pair lists and their
 * counts; these verify all K in one call -- a number of kernel launches that does not grow with n_sets (7 without the
 * refit, 12 with it) and 1 stream synchronisation without PSX_RANSAC_REFIT, 2 with it, where a loop over psx_ransac_*_dev
 * pays 6 / 11 launches and 1 / 2 synchronisations per list.  INTEGRATION.md ("Many lists in one call") has the words and
 * the measured cost.  The arguments are the outputs of psx_match_pairs_many_u8*, unchanged:
 *   pairs       the concatenation, 16-byte records (host_pairs: HOST; d_pairs: DEVICE, 16-byte aligned);
 *   set_counts  HOST array of n_sets counts; set k's records start at the sum of the counts before it, and their `right`
 *               indexes set k's own position array;
 *   d_left_xy   one left position array of l_len (x, y) pairs;  d_right_xys / r_lens: HOST arrays of n_sets DEVICE
 *               pointers / lengths -- separate allocations, slices of one buffer, or the same pointer more than once;
 *   opts        one tol, hypotheses = N, seed and flags for all sets: hypothesis h of set k draws from its own n_k
 *               exactly as the single call does;
 *   results     HOST array of n_sets results.
 * With (result_k, I_k) = what the single call returns at unlimited capacity for (P_k, left_xy, right_xys[k], opts), bit
 * for bit: results[k] = result_k; the inlier output is the concatenation I_0 .. I_{K-1}, set k's inliers starting at the
 * sum of results[j].inliers for j < k; *count = the sum over all sets; the first min(*count, capacity) records are
 * written, nothing at or past capacity; capacity = 0 with a NULL output asks "how many?".  host_models (n_sets x N x 9
 * floats) and host_counts (n_sets x N ints) receive every set's layers, either may be NULL.
 * A set with fewer than 4 (homography) / 8 (fundamental) / 3 (affine) / 2 (similarity) pairs yields the "no model" result, contributes nothing to the
 * output and has zeros in its rows of host_models / host_counts.  n_sets = 0, or all sets below the minimum, gives
 * PSX_OK without touching a device.
 * PSX_ERR_INVALID, with nothing touched and before any device call: everything the single call refuses; n_sets < 0;
 * set_counts, d_right_xys, r_lens or results NULL with n_sets > 0; a negative count or length; a NULL right array whose
 * set has pairs or a length; a sum of counts, or n_sets * hypotheses, above 0x3fffffff.  A pair index outside its position
 * array, in any set that has a model to estimate, gives PSX_ERR_INVALID for the whole call and no inlier record is written.
 * Scratch (psx_match_release) and thread safety as psx_ransac_*.  Synchronous. */
int psx_ransac_homography_many(int device, const void* host_pairs, const int* set_counts, int n_sets,
                               const float* d_left_xy, int l_len, const float* const* d_right_xys, const int* r_lens,
                               const psx_ransac_opts* opts, psx_ransac_result* results,
                               void* host_inliers, int capacity, int* count, float* host_models, int* host_counts);
int psx_ransac_homography_many_dev(int device, const void* d_pairs, const int* set_counts, int n_sets,
                                   const float* d_left_xy, int l_len, const float* const* d_right_xys, const int* r_lens,
                                   const psx_ransac_opts* opts, psx_ransac_result* results,
                                   void* d_inliers, int capacity, int* count, float* host_models, int* host_counts);
int psx_ransac_fundamental_many(int device, const void* host_pairs, const int* set_counts, int n_sets,
                                const float* d_left_xy, int l_len, const float* const* d_right_xys, const int* r_lens,
                                const psx_ransac_opts* opts, psx_ransac_result* results,
                                void* host_inliers, int capacity, int* count, float* host_models, int* host_counts);
int psx_ransac_fundamental_many_dev(int device, const void* d_pairs, const int* set_counts, int n_sets,
                                    const float* d_left_xy, int l_len, const float* const* d_right_xys, const int* r_lens,
                                    const psx_ransac_opts* opts, psx_ransac_result* results,
                                    void* d_inliers, int capacity, int* count, float* host_models, int* host_counts);
int psx_ransac_affine_many(int device, const void* host_pairs, const int* set_counts, int n_sets,
                         const float* d_left_xy, int l_len, const float* const* d_right_xys, const int* r_lens,
                         const psx_ransac_opts* opts, psx_ransac_result* results,
                         void* host_inliers, int capacity, int* count, float* host_models, int* host_counts);
int psx_ransac_affine_many_dev(int device, const void* d_pairs, const int* set_counts, int n_sets,
                             const float* d_left_xy, int l_len, const float* const* d_right_xys, const int* r_lens,
                             const psx_ransac_opts* opts, psx_ransac_result* results,
                             void* d_inliers, int capacity, int* count, float* host_models, int* host_counts);
int psx_ransac_similarity_many(int device, const void* host_pairs, const int* set_counts, int n_sets,
                         const float* d_left_xy, int l_len, const float* const* d_right_xys, const int* r_lens,
                         const psx_ransac_opts* opts, psx_ransac_result* results,
                         void* host_inliers, int capacity, int* count, float* host_models, int* host_counts);
int psx_ransac_similarity_many_dev(int device, const void* d_pairs, const int* set_counts, int n_sets,
                             const float* d_left_xy, int l_len, const float* const* d_right_xys, const int* r_lens,
                             const psx_ransac_opts* opts, psx_ransac_result* results,
                             void* d_inliers, int capacity, int* count, float* host_models, int* host_counts);
/* Host only, no device and no context: the loop over the single-list rule on host arrays (right_xys: n_sets HOST pointers),
 * with the same argument checks; every pair index of every set is checked before anything is written. */
int psx_ransac_homography_many_ref(const void* pairs, const int* set_counts, int n_sets, const float* left_xy, int nl,
                                   const float* const* right_xys, const int* r_lens, const psx_ransac_opts* opts,
                                   psx_ransac_result* results, void* inliers, int capacity, int* count, float* models, int* counts);
int psx_ransac_fundamental_many_ref(const void* pairs, const int* set_counts, int n_sets, const float* left_xy, int nl,
                                    const float* const* right_xys, const int* r_lens, const psx_ransac_opts* opts,
                                    psx_ransac_result* results, void* inliers, int capacity, int* count, float* models, int* counts);
int psx_ransac_affine_many_ref(const void* pairs, const int* set_counts, int n_sets, const float* left_xy, int nl,
                             const float* const* right_xys, const int* r_lens, const psx_ransac_opts* opts,
                             psx_ransac_result* results, void* inliers, int capacity, int* count, float* models, int* counts);
int psx_ransac_similarity_many_ref(const void* pairs, const int* set_counts, int n_sets, const float* left_xy, int nl,
                             const float* const* right_xys, const int* r_lens, const psx_ransac_opts* opts,
                             psx_ransac_result* results, void* inliers, int capacity, int* count, float* models, int* counts);

/* From the K results of psx_ransac_*_many* to the K guides of psx_match_pairs_guided_many_u8*, on the HOST: no device, no
 * context.  guides[k] = { results[k].best < 0 ? PSX_GUIDE_NONE : kind, results[k].m, tol }: a set without a model is
 * skipped by the re-match instead of being matched under its zero matrix.  kind: PSX_GUIDE_HOMOGRAPHY for the results of
 * psx_ransac_homography_many*, psx_ransac_affine_many* and psx_ransac_similarity_many*, PSX_GUIDE_EPIPOLAR for those of psx_ransac_fundamental_many*.  PSX_ERR_INVALID, with
 * nothing written: n_sets < 0, a NULL array with n_sets > 0, a kind other than 1 or 2, a tol that is not finite and >= 0. */
int psx_guides_from_ransac(const psx_ransac_result* results, int n_sets, int kind, float tol, psx_guide* guides);

/* How the batched calls cut the concatenated list, on the HOST: no device, no context (csrc/hip/ransac_many_plan.h, the
 * function the library itself plans with: block_rows = 512 for the score kernel, 256 for the gather and the compaction).
 * A block is pairs [first, end) of the CONCATENATION, all of one set, end - first <= block_rows; a set's blocks are
 * ascending and contiguous and cover it exactly once; a set with fewer than min_pairs pairs contributes no block.
 * *block_count is always the total; the first min(total, capacity) entries are written (capacity 0 with NULL: "how
 * many?").  PSX_ERR_INVALID for n_sets < 0, a NULL set_counts with n_sets > 0, a negative count, a sum of counts above
 * 0x3fffffff, min_pairs < 1, block_rows < 1, a NULL block_count, a negative capacity, a NULL table with a capacity. */
typedef struct psx_ransac_block { int set, first, end; } psx_ransac_block;
int psx_ransac_many_plan(const int* set_counts, int n_sets, int min_pairs, int block_rows,
                         psx_ransac_block* blocks, int capacity, int* block_count);

/* A LIST OF VIEW PAIRS IN ONE CALL: verify, then re-match.  psx_match_pairs_graph_u8* leaves the concatenation P_0 ..
 * P_{E-1} of the edges' pair lists in the order of the edge list, and their counts.  The calls below are the other two
 * links of match -> verify -> guided re-match for that list, whatever its order -- it need not be grouped by left view:
 *   psx_ransac_*_graph*                   one model per edge;
 *   psx_guides_from_ransac (above)        the E results as E guides, unchanged: n_sets = n_edges;
 *   psx_match_pairs_guided_graph_u8*      every edge re-matched under its own guide.
 * INTEGRATION.md ("Verify and re-match a list of view pairs") has the chain written out and the measured cost.
 *
 * RANSAC over an edge list.  The launch sequence of psx_ransac_*_many* with "set" read as "edge": 7 kernel launches and 1
 * stream synchronisation without PSX_RANSAC_REFIT, 12 and 2 with it, whatever n_edges and n_sets are.
 *   pairs        the concatenation, 16-byte records (host_pairs: HOST; d_pairs: DEVICE, 16-byte aligned), and
 *   edge_counts  HOST array of n_edges counts: exactly what psx_match_pairs_graph_u8[_dev] left, passed on unchanged;
 *   edges        HOST array of n_edges {left, right} indices into the set array;
 *   d_xys, lens  HOST arrays of n_sets entries: d_xys[s] a DEVICE pointer to the lens[s] (x, y) pairs of view s, as
 *                psx_desc_positions gives them, 8-byte aligned; edge e's records index d_xys[edges[e].left] with `left`
 *                and d_xys[edges[e].right] with `right`;
 *   opts         one tol, hypotheses = N, seed and flags for all edges: hypothesis h of edge e draws from its own n_e;
 *   results      HOST array of n_edges results.
 * With (result_e, I_e) = what the single call psx_ransac_<model>[_dev] returns at unlimited capacity for (P_e,
 * d_xys[left_e], lens[left_e], d_xys[right_e], lens[right_e], opts), bit for bit: results[e] = result_e; the inlier output
 * is the concatenation I_0 .. I_{E-1} in the order of the edge list, edge e's inliers starting at the sum of
 * results[j].inliers for j < e; *count = the total; the first min(*count, capacity) records are written, nothing at or
 * past capacity; capacity = 0 with a NULL output asks "how many?".  host_models (n_edges x N x 9 floats) and host_counts
 * (n_edges x N ints) receive every edge's layers, either may be NULL.  The list is neither sorted nor deduplicated: a
 * duplicate edge gives the same result twice, (a, b) and (b, a) are two edges, left == right is the single call with the
 * same array on both sides.  An edge with fewer pairs than its model's minimum (4 / 8 / 3 / 2) yields the "no model"
 * result, contributes nothing to the output and has zeros in its rows of the layers.  n_edges = 0, or all edges below the
 * minimum, gives PSX_OK without touching a device.
 * PSX_ERR_INVALID, with nothing touched and before any device call: everything psx_ransac_*_many* refuses, with edge_counts
 * and n_edges in the place of set_counts and n_sets (a sum of counts, or n_edges * hypotheses, above 0x3fffffff among it);
 * everything psx_match_pairs_graph_u8 refuses about lens, n_sets, edges and n_edges; d_xys NULL with n_sets > 0; a NULL
 * d_xys[s] with lens[s] > 0, or under an edge that has pairs.  A pair index outside ITS OWN edge's left or right position
 * array, in any edge that has a model to estimate, gives PSX_ERR_INVALID for the whole call and no inlier record is
 * written; nothing is read out of bounds.  Scratch (psx_match_release) and thread safety as psx_ransac_*.  Synchronous. */
int psx_ransac_homography_graph(int device, const void* host_pairs, const int* edge_counts, const psx_view_edge* edges, int n_edges,
                                const float* const* d_xys, const int* lens, int n_sets,
                                const psx_ransac_opts* opts, psx_ransac_result* results,
                                void* host_inliers, int capacity, int* count, float* host_models, int* host_counts);
int psx_ransac_homography_graph_dev(int device, const void* d_pairs, const int* edge_counts, const psx_view_edge* edges, int n_edges,
                                    const float* const* d_xys, const int* lens, int n_sets,
                                    const psx_ransac_opts* opts, psx_ransac_result* results,
                                    void* d_inliers, int capacity, int* count, float* host_models, int* host_counts);
int psx_ransac_fundamental_graph(int device, const void* host_pairs, const int* edge_counts, const psx_view_edge* edges, int n_edges,
                                 const float* const* d_xys, const int* lens, int n_sets,
                                 const psx_ransac_opts* opts, psx_ransac_result* results,
                                 void* host_inliers, int capacity, int* count, float* host_models, int* host_counts);
int psx_ransac_fundamental_graph_dev(int device, const void* d_pairs, const int* edge_counts, const psx_view_edge* edges, int n_edges,
                                     const float* const* d_xys, const int* lens, int n_sets,
                                     const psx_ransac_opts* opts, psx_ransac_result* results,
                                     void* d_inliers, int capacity, int* count, float* host_models, int* host_counts);
int psx_ransac_affine_graph(int device, const void* host_pairs, const int* edge_counts, const psx_view_edge* edges, int n_edges,
                            const float* const* d_xys, const int* lens, int n_sets,
                            const psx_ransac_opts* opts, psx_ransac_result* results,
                            void* host_inliers, int capacity, int* count, float* host_models, int* host_counts);
int psx_ransac_affine_graph_dev(int device, const void* d_pairs, const int* edge_counts, const psx_view_edge* edges, int n_edges,
                                const float* const* d_xys, const int* lens, int n_sets,
                                const psx_ransac_opts* opts, psx_ransac_result* results,
                                void* d_inliers, int capacity, int* count, float* host_models, int* host_counts);
int psx_ransac_similarity_graph(int device, const void* host_pairs, const int* edge_counts, const psx_view_edge* edges, int n_edges,
                                const float* const* d_xys, const int* lens, int n_sets,
                                const psx_ransac_opts* opts, psx_ransac_result* results,
                                void* host_inliers, int capacity, int* count, float* host_models, int* host_counts);
int psx_ransac_similarity_graph_dev(int device, const void* d_pairs, const int* edge_counts, const psx_view_edge* edges, int n_edges,
                                    const float* const* d_xys, const int* lens, int n_sets,
                                    const psx_ransac_opts* opts, psx_ransac_result* results,
                                    void* d_inliers, int capacity, int* count, float* host_models, int* host_counts);
/* Host only, no device and no context: the loop over the single-list rule on host arrays (xys: n_sets HOST pointers), with
 * the same argument checks; every pair index of every edge is checked before anything is written. */
int psx_ransac_homography_graph_ref(const void* pairs, const int* edge_counts, const psx_view_edge* edges, int n_edges,
                                    const float* const* xys, const int* lens, int n_sets, const psx_ransac_opts* opts,
                                    psx_ransac_result* results, void* inliers, int capacity, int* count, float* models, int* counts);
int psx_ransac_fundamental_graph_ref(const void* pairs, const int* edge_counts, const psx_view_edge* edges, int n_edges,
                                     const float* const* xys, const int* lens, int n_sets, const psx_ransac_opts* opts,
                                     psx_ransac_result* results, void* inliers, int capacity, int* count, float* models, int* counts);
int psx_ransac_affine_graph_ref(const void* pairs, const int* edge_counts, const psx_view_edge* edges, int n_edges,
                                const float* const* xys, const int* lens, int n_sets, const psx_ransac_opts* opts,
                                psx_ransac_result* results, void* inliers, int capacity, int* count, float* models, int* counts);
int psx_ransac_similarity_graph_ref(const void* pairs, const int* edge_counts, const psx_view_edge* edges, int n_edges,
                                    const float* const* xys, const int* lens, int n_sets, const psx_ransac_opts* opts,
                                    psx_ransac_result* results, void* inliers, int capacity, int* count, float* models, int* counts);

/* Guided re-match over an edge list (byte descriptors).  One stream synchronisation and a number of kernel launches that
 * grows neither with n_edges nor with n_sets: 4 without the cross-check, 6 with it, plus the table copy.
 * d_sets, d_xys, lens: HOST arrays of n_sets entries, d_sets[s] / d_xys[s] DEVICE pointers to the lens[s] descriptors of
 * 128 bytes (16-byte aligned) / (x, y) positions (8-byte aligned) of view s -- separate allocations, slices of one buffer,
 * or the same pointer more than once; edges: HOST array of n_edges {left, right}; guides: HOST array of n_edges guides,
 * guides[e] for EDGE e -- what psx_guides_from_ransac makes of the results of psx_ransac_*_graph*.
 * With G_e = the list psx_match_pairs_guided_u8 returns at unlimited capacity for the two sets and position arrays of edge
 * e under guides[e] and opts, bit for bit: the result is the concatenation G_0 .. G_{E-1} in the order of the edge list;
 * edge_counts[e] = |G_e| (HOST array of n_edges ints), *count their sum: always the totals; the first min(*count,
 * capacity) records are written -- the cut may fall inside an edge --, nothing at or past capacity; capacity = 0 with a
 * NULL output asks "how many?".  An edge whose guide has kind == PSX_GUIDE_NONE is SKIPPED: its count is 0 and nothing of
 * that edge is read (the rest of that guide is not looked at); so is an edge with an empty side.  The list is neither
 * sorted nor deduplicated, left == right is the single call with the same arrays on both sides.
 * n_edges = 0, or a call whose edges are all empty or skipped, gives zero counts and PSX_OK without touching a device.
 * PSX_ERR_INVALID, with nothing touched and before any device call: everything psx_match_pairs_graph_u8 refuses (the sum
 * over the edges of lens[left] or of lens[right] above INT_MAX among it); d_xys NULL with n_sets > 0; a NULL d_xys[s] with
 * lens[s] > 0; guides NULL with n_edges > 0; any guide that is neither valid nor of kind 0 -- EVERY guide is checked before
 * anything runs.  PSX_ERR_NOMEM where a grid would not fit an int.  Scratch (psx_match_release) and thread safety as for
 * psx_match_u8.  Synchronous.  The float form is psx_match_pairs_guided_graph (below). */
int psx_match_pairs_guided_graph_u8(int device, const unsigned char* const* d_sets, const float* const* d_xys,
                                    const int* lens, int n_sets, const psx_view_edge* edges, int n_edges,
                                    const psx_guide* guides, const psx_match_opts* opts,
                                    psx_match_pair_u8* host_pairs, int capacity, int* edge_counts, int* count);
/* the list stays in HBM: d_pairs is a DEVICE pointer, 16-byte aligned; edge_counts and count are still HOST memory */
int psx_match_pairs_guided_graph_u8_dev(int device, const unsigned char* const* d_sets, const float* const* d_xys,
                                        const int* lens, int n_sets, const psx_view_edge* edges, int n_edges,
                                        const psx_guide* guides, const psx_match_opts* opts,
                                        psx_match_pair_u8* d_pairs, int capacity, int* edge_counts, int* count);
/* The float form of psx_match_pairs_guided_graph_u8: the same signature and contract, word for word, with descriptors of
 * 128 floats (16-byte aligned), psx_match_pair records and psx_match_pairs_guided as the single call -- edge e yields, bit
 * for bit (float distances compared as bit patterns), what psx_match_pairs_guided returns for its two sets under guides[e].
 * The same driver on (float, float): 4 kernel launches, 6 with the cross-check, one stream synchronisation.  Its input is
 * what psx_match_pairs_graph[_dev] and psx_ransac_*_graph* leave, its output goes into psx_tracks_graph*: those read only
 * `left` and `right` of a 16-byte record. */
int psx_match_pairs_guided_graph(int device, const float* const* d_sets, const float* const* d_xys,
                                 const int* lens, int n_sets, const psx_view_edge* edges, int n_edges,
                                 const psx_guide* guides, const psx_match_opts* opts,
                                 psx_match_pair* host_pairs, int capacity, int* edge_counts, int* count);
/* the list stays in HBM: d_pairs is a DEVICE pointer, 16-byte aligned; edge_counts and count are still HOST memory */
int psx_match_pairs_guided_graph_dev(int device, const float* const* d_sets, const float* const* d_xys,
                                     const int* lens, int n_sets, const psx_view_edge* edges, int n_edges,
                                     const psx_guide* guides, const psx_match_opts* opts,
                                     psx_match_pair* d_pairs, int capacity, int* edge_counts, int* count);

/* TRACKS FROM A LIST OF VIEW PAIRS: the fourth link.  The chain above ends with E separate pair lists; structure from
 * motion, loop closure and retrieval need TRACKS next: the sets of rows in different views that the pairs connect
 * transitively, one scene point each.  One call over the same edge list and the same concatenated records with per-edge
 * counts; INTEGRATION.md ("Tracks from a list of view pairs") has the four-call chain and the measured cost.
 *   pairs        the concatenation of 16-byte records (host_pairs: HOST; d_pairs: DEVICE, 16-byte aligned), edge e owning
 *                edge_counts[e] consecutive records.  Only the first two ints {left, right} of a record are read: the
 *                buffer may hold psx_match_pair_u8 or psx_match_pair records, a RANSAC inlier list (results[e].inliers as
 *                counts) or a guided re-match list;
 *   edge_counts, edges, lens   HOST arrays, as psx_ransac_*_graph* takes them;
 *   opts         {min_views >= 2, flags}; {2, 0} is the usual choice.
 * THE RULE (csrc/hip/tracks_rule.h, shared by host and device).  Row r of view v is node g = off[v] + r, off = the
 * exclusive prefix sum of lens, M = their sum.  A record of edge e joins node (edges[e].left, left) with node
 * (edges[e].right, right).  Nothing is special-cased: duplicate edges and records join again (a no-op); (a, b) and (b, a)
 * are two edges; on an edge with left == right a record with equal rows is a self-loop (a no-op), one with different rows
 * joins two rows of one view.  A component of the joins is named by its smallest node, its root.  A component is a TRACK
 * iff it has >= 2 members in >= min_views distinct views and no two members in one view -- a CONFLICT, dropped as
 * AliceVision drops it -- unless PSX_TRACKS_KEEP_CONFLICTS is set.  Tracks are numbered by ascending root; the members
 * of a track are ordered by ascending node: by view, then by row.
 * OUTPUTS.  track_starts[0 .. tracks]: a CSR row array, track t owns members[track_starts[t] .. track_starts[t + 1]);
 * the values are always the unclipped offsets.  members: {view, row}, 8 bytes.  labels (M ints, may be NULL): the track
 * number of every node, -1 for a node in no kept track.  info, always the totals whatever the capacities are: tracks;
 * members; components (those of >= 2 members); conflicts (components with two members in one view); too_few_views
 * (components of >= 2 members in fewer than min_views views; a component may count in both, and neither depends on the
 * flags); joined_records (the records that are not self-loops).
 * CAPACITIES.  track_starts has room for track_capacity + 1 ints, entries 0 .. min(tracks, track_capacity) are written;
 * the first min(members, member_capacity) member records are written, the cut may fall inside a track; nothing at or
 * past either capacity is touched.  Capacity 0 with a NULL pointer asks "how many?".
 * n_edges = 0, all counts zero, or M = 0: zero totals and PSX_OK without touching a device; the host form and the
 * reference then set labels to -1 and track_starts[0] to 0 where the arrays are given, the _dev form writes nothing to
 * device memory.
 * PSX_ERR_INVALID, before any device call and with nothing written: everything psx_ransac_*_graph* refuses about lens,
 * n_sets, edges, n_edges and edge_counts (a negative count among it); pairs NULL with a count; NULL opts or info;
 * min_views < 2; unknown flag bits; a negative capacity, or a NULL output with a positive capacity; an edge that has
 * records and an empty side (no row can lie inside it); in the _dev form a misaligned device pointer (records 16 bytes,
 * members 8, ints 4); M or the sum of the counts above 0x3fffffff.  A record whose left or right lies outside ITS OWN
 * edge's view lengths refuses the whole call with PSX_ERR_INVALID, through one device flag: nothing is read or written out
 * of bounds, info and the host outputs are untouched, the contents of device output buffers are unspecified.
 * PSX_ERR_NOMEM where a grid or table would not fit an int.
 * One table copy, 7 kernel launches and one radix sort (rocprim), one stream synchronisation, whatever n_edges, n_sets
 * and M are.  Scratch (psx_match_release) and thread safety as for psx_match_u8.  Synchronous.
 * Out of scope: merging the descriptor rows of one multi-orientation keypoint into one feature (tracks are over
 * descriptor rows, as the pair records are), and triangulation. */
#define PSX_TRACKS_KEEP_CONFLICTS 1
typedef struct psx_track_opts   { int min_views; int flags; } psx_track_opts;      /* {2, 0} */
typedef struct psx_track_member { int view, row; } psx_track_member;
typedef struct psx_tracks_info  { int tracks, members, components, conflicts, too_few_views, joined_records; } psx_tracks_info;
int psx_tracks_graph(int device, const void* host_pairs, const int* edge_counts, const psx_view_edge* edges, int n_edges,
                     const int* lens, int n_sets, const psx_track_opts* opts,
                     int* host_labels, int* host_track_starts, int track_capacity,
                     psx_track_member* host_members, int member_capacity, psx_tracks_info* info);
/* everything stays in HBM: d_pairs, d_labels, d_track_starts and d_members are DEVICE pointers; edge_counts, edges, lens,
 * opts and info stay HOST memory */
int psx_tracks_graph_dev(int device, const void* d_pairs, const int* edge_counts, const psx_view_edge* edges, int n_edges,
                         const int* lens, int n_sets, const psx_track_opts* opts,
                         int* d_labels, int* d_track_starts, int track_capacity,
                         psx_track_member* d_members, int member_capacity, psx_tracks_info* info);
/* Host only, no device: a sequential union-find under the same rule and the same argument checks -- the definition.  Every
 * record of every edge is checked before anything is written. */
int psx_tracks_graph_ref(const void* pairs, const int* edge_counts, const psx_view_edge* edges, int n_edges,
                         const int* lens, int n_sets, const psx_track_opts* opts,
                         int* labels, int* track_starts, int track_capacity,
                         psx_track_member* members, int member_capacity, psx_tracks_info* info);
/* What a call of these sizes plans, on the HOST (csrc/hip/tracks_plan.h, the header the library itself plans with): nodes
 * = M; records = the sum of the counts; record_blocks = the 256-record blocks of the join kernel, none crossing an edge;
 * sort_bits = the key bits of the sort, ceil(log2 M) and at least 1; launches = the library's own kernel launches (the
 * sort's come on top); scratch_bytes = the device scratch of the _dev form without the sort's temporary storage.  A call
 * that touches no device plans zero blocks, launches and bytes.  PSX_ERR_INVALID for what the calls above refuse about
 * lens, n_sets, edge_counts and n_edges, or a NULL out; PSX_ERR_NOMEM where a table would not fit an int. */
typedef struct psx_tracks_plan_info { int nodes, records, record_blocks, sort_bits, launches; long long scratch_bytes; } psx_tracks_plan_info;
int psx_tracks_plan(const int* lens, int n_sets, const int* edge_counts, int n_edges, psx_tracks_plan_info* out);

/* WHICH PAIRS TO MATCH: the zeroth link.  Every graph call above takes its edge list from the caller; all pairs grow as
 * N^2 and a window only helps ordered video.  These three calls answer "which views could see the same thing?" the way
 * structure-from-motion front ends do before feature matching (AliceVision's imageMatching step over a vocabulary tree;
 * Nister & Stewenius, "Scalable recognition with a vocabulary tree", CVPR 2006, for the idf-weighted, L1-normalised
 * scoring; Sivic & Zisserman, "Video Google", ICCV 2003): a visual vocabulary, a bag of words per view, the k most similar
 * views per view.  The reference has no counterpart.  N byte descriptor sets in HBM go in, a sorted, deduplicated
 * psx_view_edge list comes out, which the four graph calls take unchanged; INTEGRATION.md ("Which pairs to match") has the
 * five-call chain and the measured cost.
 * FORMS.  Each call has a form with HOST outputs, a _dev form whose arrays are all DEVICE memory, and a _ref form that runs
 * on the host alone, is sequential and is the definition: the device forms equal it bit for bit.  The descriptor sets
 * (d_sets[v]: lens[v] rows of 128 bytes, 16-byte aligned) are DEVICE pointers in both device forms and host arrays in the
 * _ref form; a vocabulary, a histogram and every output are HOST memory in the host form and DEVICE memory in the _dev
 * form; lens, opts, info and edge_count are always HOST memory.
 * THE RULE (csrc/hip/bow_rule.h, shared by host and device).  Row r of view v is global row g = off[v] + r, off = the
 * exclusive prefix sum of lens, M = their sum; d(x, c) = sum_k (x_k - c_k)^2, an exact integer.
 *   TRAIN   integer k-means, opts = {words W, iterations T}, 2 <= W <= 65536, W <= M <= 2^24, T >= 1.  Word w starts as
 *           global row floor(w M / W).  An iteration assigns every row to the word with the smallest (d, w) -- ties to the
 *           lower word, the byte matcher's order -- and replaces every word that has rows by their mean, byte by byte
 *           (2 sum + cnt) / (2 cnt) in integers (half rounds up); a word without rows keeps its bytes.  It stops after T
 *           iterations or after the first one in which no row changed its word (in the first, every row counts as
 *           changed).  info: iterations run; changed and empty_words of the last assignment; inertia = the sum of d(g, a(g))
 *           of the last assignment against the words it was made with; reserved = 0.  Empty views are allowed.
 *   BAGS    hist[v][w] (n_sets x words, uint32) = the rows of view v assigned to word w; words_out (M ints, may be NULL) =
 *           a(g) of every row.  1 <= words <= 65536, M <= 0x3fffffff.  n_sets = 0 or M = 0 touches no device: the host form
 *           and the reference write a zero histogram, the _dev form writes nothing.
 *   LISTS   n_v = the sum of hist[v][.] (not a trusted length); df[w] = the views with hist[v][w] > 0; weight[w] = 0 for
 *           df = 0, otherwise 1 + floor(16 log2(N / df) + 0.5) in double, evaluated ONLY on the host by psx_bow_weights(df,
 *           words, n_views, out), which the library and the reference both call (the device counts df; one download of W
 *           ints and one upload of W weights); q[v][w] = floor(hist[v][w] 65535 / n_v), 0 for n_v = 0; score(i, j) = sum_w
 *           weight[w] min(q[i][w], q[j][w]), symmetric and below 2^24.  The list of view i: the views j != i with
 *           score(i, j) > 0 by (score descending, j ascending), the first k; neighbours[i][0 .. k) and scores[i][0 .. k)
 *           (either may be NULL), unused entries -1 and 0; k may exceed n_views - 1.  The edges: {(min(i, j), max(i, j)) :
 *           j in the list of i}, once each, ascending by (left, right); with PSX_SHORTLIST_MUTUAL only the pairs in which
 *           each view lists the other.  *edge_count is always the total, the first min(total, edge_capacity) edges are
 *           written, nothing at or past the capacity is touched; capacity 0 with NULL asks "how many?".  n_views = 0: no
 *           edge, nothing else written, no device.
 * PSX_ERR_INVALID, before any device call and with nothing written: n_sets < 0, a NULL array that is needed, a negative
 * length, a NULL set with a positive length, a misaligned device pointer (sets 16 bytes, ints 4, edges 8); NULL opts, info,
 * vocabulary or edge_count; words or iterations out of range, words > M, M too large; n_views > 4096 (or < 0), k < 1,
 * unknown flag bits, n_views * k above INT_MAX, a negative capacity or a NULL edge array with a positive one; for
 * psx_bow_weights a df outside [0, n_views] or n_views < 1.
 * LAUNCHES.  Training, once per call: the table copy, 3 kernels (the gather of all rows into one array, their norms, the
 * initial words) and one clear; then per iteration one clear, 4 kernels (the words' norms, the assignment, the
 * accumulation, the update) and ONE synchronisation that brings back the 16 bytes deciding the stop; the host form ends
 * with one more copy and synchronisation for the vocabulary.  psx_bow_u8*: the table copy, 5 kernels and one clear, one
 * synchronisation.  psx_shortlist_views*: 6 kernels and 2 clears, TWO synchronisations (the first brings df to the host for
 * the weights).  None depends on n_sets, n_views or M.  The assignment is the byte matcher's i8-MFMA tile walk
 * (csrc/hip/match_u8_core.h); the rows of all views are gathered into one scratch array of 128 M bytes first.  Scratch
 * (psx_match_release) and thread safety as for psx_match_u8.  Synchronous. */
#define PSX_SHORTLIST_MUTUAL 1
typedef struct psx_vocab_opts     { int words; int iterations; } psx_vocab_opts;
typedef struct psx_vocab_info     { int iterations, changed, empty_words, reserved; unsigned long long inertia; } psx_vocab_info;
typedef struct psx_shortlist_opts { int k; int flags; } psx_shortlist_opts;
int psx_vocab_train_u8(int device, const unsigned char* const* d_sets, const int* lens, int n_sets, const psx_vocab_opts* opts,
                       unsigned char* host_vocab, psx_vocab_info* info);
int psx_vocab_train_u8_dev(int device, const unsigned char* const* d_sets, const int* lens, int n_sets, const psx_vocab_opts* opts,
                           unsigned char* d_vocab, psx_vocab_info* info);
int psx_vocab_train_u8_ref(const unsigned char* const* sets, const int* lens, int n_sets, const psx_vocab_opts* opts,
                           unsigned char* vocab, psx_vocab_info* info);
int psx_bow_u8(int device, const unsigned char* host_vocab, int words, const unsigned char* const* d_sets, const int* lens, int n_sets,
               unsigned* host_hist, int* host_words_out);
int psx_bow_u8_dev(int device, const unsigned char* d_vocab, int words, const unsigned char* const* d_sets, const int* lens, int n_sets,
                   unsigned* d_hist, int* d_words_out);
int psx_bow_u8_ref(const unsigned char* vocab, int words, const unsigned char* const* sets, const int* lens, int n_sets,
                   unsigned* hist, int* words_out);
int psx_shortlist_views(int device, const unsigned* host_hist, int n_views, int words, const psx_shortlist_opts* opts,
                        int* host_neighbours, unsigned* host_scores, psx_view_edge* host_edges, int edge_capacity, int* edge_count);
int psx_shortlist_views_dev(int device, const unsigned* d_hist, int n_views, int words, const psx_shortlist_opts* opts,
                            int* d_neighbours, unsigned* d_scores, psx_view_edge* d_edges, int edge_capacity, int* edge_count);
int psx_shortlist_views_ref(const unsigned* hist, int n_views, int words, const psx_shortlist_opts* opts,
                            int* neighbours, unsigned* scores, psx_view_edge* edges, int edge_capacity, int* edge_count);
/* HOST only: out[w] = the weight of a word that df[w] of n_views views contain (the one logarithm of the step) */
int psx_bow_weights(const int* df, int words, int n_views, int* out);

/* QUERY A DATABASE OF VIEWS: the k stored views most like each of a few new ones.  psx_shortlist_views answers "every view
 * against every other of one closed collection": when view N + 1 arrives it quantises and scores all N x N again, it stops
 * at 4096 views (12 index bits, N x N scratch), and both follow from the symmetric form.  Incremental structure-from-motion
 * and loop closure ask for one ROW: these calls keep the views as rows of q in the caller's HBM, which grow by appending,
 * and rank n_queries <= 4096 rows against n_db <= 1 048 576 of them.  No n_queries x n_db array goes through HBM.
 * INTEGRATION.md ("Query a database of views") has the chain with an arriving view and the measured cost.
 * FORMS as above: host outputs, _dev (neighbours, scores and edges in HBM) and _ref (all on the host, sequential, the
 * definition; the device forms equal it bit for bit).  d_db_q (n_db x words) and d_query_q (n_queries x words) are DEVICE
 * arrays of uint16 in the first two forms; weights, db_limit, opts and edge_count are HOST memory in every form.
 * THE RULE (csrc/hip/bow_rule.h).
 *   QUANTISE  q[v][w] = floor(hist[v][w] 65535 / n_v), n_v = the row's own sum, 0 for n_v = 0: a view's q depends on nothing
 *             but its own row, so a database grows by quantising new rows behind the old ones.  df_accum (HOST, words ints,
 *             may be NULL): the number of these n_views views with hist[v][w] > 0 is ADDED to df_accum[w].  The weights of a
 *             query are the caller's: psx_bow_weights(df_accum, words, views added so far, out) gives the shortlist's.
 *   SCORE     score(i, j) = sum_w weights[w] min(qq[i][w], dbq[j][w]), weights in [0, 1023]: below 2^26 for rows that
 *             psx_bow_quantize* wrote (their q add up to at most 65535); added in unsigned 32 bits in every form.
 *   LIST      The candidates of query i: the database views j with j < limit_i (db_limit[i], or n_db when db_limit is
 *             NULL), j != self_base + i (when self_base >= 0: query i IS database view self_base + i), score(i, j) > 0 and
 *             score(i, j) >= min_score; by (score descending, j ascending), the first k.  neighbours[i][0 .. k) and
 *             scores[i][0 .. k) (either may be NULL), unused entries -1 and 0; k may exceed n_db.
 *   EDGES     For i ascending, then in list order, {left = edge_base + i, right = j}: grouped by left, every group a star
 *             that the _many calls and the four graph calls take unchanged; a caller who appends the query sets behind the
 *             database's in its set array passes edge_base = n_db.  NOT sorted by right and NOT deduplicated: with
 *             self_base >= 0 a pair can appear as (a, b) and as (b, a), which the graph calls accept.  *edge_count is always
 *             the total, the first min(total, edge_capacity) records are written, nothing at or past the capacity is
 *             touched; capacity 0 with NULL asks "how many?".
 *   With self_base = 0, db_limit = NULL, the database as its own queries and the weights of psx_bow_weights(df, words, N),
 *   neighbours and scores are those of psx_shortlist_views.  db_limit[i] = self_base + i is the loop-closure form: every
 *   view against the views before it.
 * EMPTY FORMS.  n_queries = 0: no device, *edge_count = 0, nothing else written.  n_db = 0: every entry is written as unused
 * (the _dev form launches one kernel for that: the caller's arrays must not stay stale), *edge_count = 0.  psx_bow_quantize*
 * with n_views = 0 touches nothing.
 * PSX_ERR_INVALID, before any device call and with nothing written (csrc/hip/bow_plan.h, once for all forms): a negative
 * count; a NULL array that is needed (q arrays, weights, hist, opts, edge_count, plan); words outside [1, 65536]; n_db above
 * 1 048 576; n_queries above 4096 (psx_bow_quantize*: n_views above 1 048 576); k < 1 or n_queries * k above INT_MAX;
 * non-zero flags or reserved; self_base < -1 or self_base + n_queries > n_db; a weight outside [0, 1023] or a limit outside
 * [0, n_db]; a misaligned device pointer (q arrays 2 bytes, ints 4, edges 8); a negative capacity or a NULL edge array with a
 * positive one; plan.partial_keys above 2^27.
 * PLAN, on the host: blocks = ceil(n_db / 64), the database blocks of the score grid; keys_per_block = min(k, 64);
 * partial_keys = n_queries * blocks * keys_per_block 64-bit keys, the block lists between the two kernels; scratch_bytes =
 * the device scratch of the _dev form called with a neighbours array.  n_queries = 0 or n_db = 0 plans zeros.
 * LAUNCHES.  psx_shortlist_query*: ONE upload (weights and limits), 5 kernels (the score tiles with their block lists, the
 * merge, the edge count / scan / write), no clear, ONE synchronisation, whatever n_db, n_queries, words and k are.
 * psx_bow_quantize_dev: one kernel and ONE synchronisation; with df_accum also one clear before it and one download of
 * words ints behind it.  Scratch (psx_match_release) and thread safety as for psx_match_u8.  Synchronous. */
typedef struct psx_query_opts { int k; int flags /* must be 0 */; int self_base /* -1: none */; int edge_base;
                                unsigned min_score; int reserved /* must be 0 */; } psx_query_opts;
typedef struct psx_query_plan { int blocks; int keys_per_block; long long partial_keys; long long scratch_bytes; } psx_query_plan;
int psx_bow_quantize_dev(int device, const unsigned* d_hist, int n_views, int words, unsigned short* d_q, int* df_accum);
int psx_bow_quantize_ref(const unsigned* hist, int n_views, int words, unsigned short* q, int* df_accum);
int psx_shortlist_query(int device, const unsigned short* d_db_q, int n_db, const unsigned short* d_query_q, int n_queries, int words,
                        const int* weights, const int* db_limit, const psx_query_opts* opts,
                        int* host_neighbours, unsigned* host_scores, psx_view_edge* host_edges, int edge_capacity, int* edge_count);
int psx_shortlist_query_dev(int device, const unsigned short* d_db_q, int n_db, const unsigned short* d_query_q, int n_queries, int words,
                            const int* weights, const int* db_limit, const psx_query_opts* opts,
                            int* d_neighbours, unsigned* d_scores, psx_view_edge* d_edges, int edge_capacity, int* edge_count);
int psx_shortlist_query_ref(const unsigned short* db_q, int n_db, const unsigned short* query_q, int n_queries, int words,
                            const int* weights, const int* db_limit, const psx_query_opts* opts,
                            int* neighbours, unsigned* scores, psx_view_edge* edges, int edge_capacity, int* edge_count);
int psx_shortlist_query_plan(int n_db, int n_queries, int words, int k, psx_query_plan* plan);

/* ---- caller-supplied keypoints ------------------------------------------------------------
 * Describing points the caller brings along instead of the ones the DoG detector finds (what OpenCV calls
 * useProvidedKeypoints and VLFeat calls frames; the reference has no counterpart).  A record carries what a
 * psx_feature reports, in INPUT-IMAGE units; INTEGRATION.md ("Caller-supplied keypoints") states the placement and
 * acceptance rule in words. */
#define PSX_KP_AUTO (-1)
typedef struct psx_keypoint {      /* 40 bytes */
    float xpos, ypos, sigma;       /* INPUT-IMAGE units, exactly what psx_feature reports */
    int   octave;                  /* >= 0: explicit;  PSX_KP_AUTO: placed by the bounds table */
    int   lpos;                    /* Gaussian level of the octave (explicit placement only) */
    int   num_ori;                 /* 0: the library assigns orientations; 1..4: orientation[] is given */
    float orientation[PSX_ORI_MAX];/* radians, as psx_feature reports them */
} psx_keypoint;

#define PSX_DESCRIBE_REUSE_PYRAMID 1

/* The levels + 1 level boundaries of automatic placement, b_l = (float)(sigma * 2^((l + 0.5) / levels)) for
 * l = 0 .. levels, computed in double and rounded once; *n = levels + 1.  PSX_ERR_INVALID when capacity is smaller.
 * Host arithmetic only. */
int psx_keypoint_bounds(const psx_config* cfg, float* bounds, int capacity, int* n);

/* The placement and acceptance rule on the host, for n records and an input of w x h pixels: octave[i] / lpos[i] =
 * where record i lands, octave[i] = -1 for a record the rule drops.  No device and no context are involved; with
 * octaves = -1 in the configuration the octave count is the one a fresh context takes for w x h.  The device kernel and
 * this function call one inline function. */
int psx_place_keypoints(const psx_config* cfg, int w, int h, const psx_keypoint* kps, int n, int* octave, int* lpos);

/* The keypoints of the next psx_describe.  The host form copies the n records in stream order (the caller's array is
 * free again on return); the device form takes no copy: the pointer (8-byte aligned) must stay valid until the
 * describe call has been waited for.  n = 0 is a valid, empty list (the pointer may be NULL then).  PSX_ERR_STATE
 * without an input image / pyramid dimensions. */
int psx_set_keypoints(psx_ctx* ctx, const psx_keypoint* host, int n);
int psx_set_keypoints_dev(psx_ctx* ctx, const psx_keypoint* dev, int n);

/* Orientation (for the records with num_ori = 0), scan and descriptors at the keypoints set before, asynchronous on
 * the context's stream like psx_extract; the detector does not run and the grid filter is never applied.  flags = 0
 * builds the pyramid of the current input first; PSX_DESCRIBE_REUSE_PYRAMID uses the one the context already holds for
 * it (PSX_ERR_STATE when there is none).  Output order: octave-major, caller order within an octave; per octave the
 * first max_extrema accepted records are kept.  Every result call (counts, downloads, exports, device results, clone,
 * extrema dump, stage timers: [1] is then the keypoint injection) works on the outcome as on an extraction's. */
int psx_describe(psx_ctx* ctx, int flags);

/* host_src[i] = index of the input record output feature i of the last psx_describe came from; *count = number of
 * features.  PSX_ERR_STATE when the last results are not a describe call's.  Synchronises. */
int psx_keypoint_map(psx_ctx* ctx, int* host_src, int capacity, int* count);

/* ---- detection mask ------------------------------------------------------------------------
 * A region of interest for the detector (OpenCV's detectAndCompute(image, mask, ...), AliceVision's per-view mask; the
 * reference has no counterpart).  A mask is a tight w x h plane of bytes, the size of the INPUT image; non-zero means
 * "keypoints allowed here".  One rule, applied inside the extrema kernels after the contrast and edge tests: a refined
 * extremum that the feature record will report at (xpos, ypos) is kept iff mask[yi * w + xi] != 0 with
 *     xi = clamp((int)floorf(xpos + 0.5f), 0, w - 1),   yi = clamp((int)floorf(ypos + 0.5f), 0, h - 1)
 * in float32 arithmetic ("Detection mask").  A masked-out point takes no slot of the extremum arrays: it
 * does not count toward max_extrema or toward the grid filter's "int(filter_max_extrema * 1.1) < number of extrema"
 * test and sees no orientation or descriptor work.
 *   - Sticky per context: the mask holds until it is replaced or cleared.
 *   - The size is checked when extrema are searched: psx_find_extrema / psx_extract return PSX_ERR_STATE (the message
 *     names both sizes) while the mask's w x h differs from the current input's; a mask is never dropped silently.
 *   - psx_describe IGNORES the mask: the caller chose those points.
 *   - An all-zero mask gives 0 features and 0 descriptors, and no error.
 * The host form copies the plane in stream order (the caller's array is free again on return); the device form takes no
 * copy: the pointer must stay valid, and its contents ordered against psx_stream, until the extraction has been waited
 * for.  mask == NULL with w == h == 0 clears the mask.  A non-positive size, or NULL with a non-zero size, returns
 * PSX_ERR_INVALID and leaves the context as it was. */
int psx_set_mask(psx_ctx* ctx, const unsigned char* host_mask, int w, int h);
int psx_set_mask_dev(psx_ctx* ctx, const unsigned char* dev_mask, int w, int h);

/* The rule on the host for n reported positions (psx_feature.xpos / ypos): keep_out[i] = 1 where position i is allowed,
 * else 0.  No device and no context are involved; the extrema kernels and this function call one inline function.
 * PSX_ERR_INVALID for a NULL mask, a non-positive size, n < 0, or n > 0 with a NULL array. */
int psx_mask_keep(const unsigned char* mask, int w, int h, const float* xpos, const float* ypos, int n,
                  unsigned char* keep_out);

/* device_prop_t (common/device_prop.h:23-108): enumeration only; there are no texture limits. */
int psx_device_count(int* count);
int psx_device_info(int device, char* name, int name_len, size_t* total_mem, int* compute_units, int* clock_khz);
/* PCI bus id ("0000:c1:00.0") of a device: lets the host library place its worker threads on the CPUs
 * local to the GPU (sysfs local_cpulist) when it drives one PopSift per GPU (popsift.h:158,166-168). */
int psx_device_pci(int device, char* bus_id, int len);

/* ---- introspection for parity tests (Octave::download_and_save_array, sift_octave.cu:111-188) */

#define PSX_PLANE_GAUSS 0
#define PSX_PLANE_DOG   1
/* Copies one W*H float plane (tight) of the current pyramid to host memory; synchronises. */
int psx_dump_plane(psx_ctx* ctx, int kind, int octave, int level, float* host_out);
/* Initial extrema of one octave (i_ext_dat, sift_pyramid.h:44-48); returns the count. */
int psx_dump_iext(psx_ctx* ctx, int octave, psx_iext* host_out, int capacity, int* count);
/* Oriented extrema (dobuf.extrema) in octave-major order. */
int psx_dump_extrema(psx_ctx* ctx, psx_extremum* host_out, int capacity, int* count);

/* ---- measurement ---------------------------------------------------------------------- */

/* Stage timers: when enabled, HIP events bracket each stage group on the context's stream;
 * psx_stage_times synchronises and returns milliseconds of the last extraction
 * [0]=pyramid [1]=extrema [2]=orientation+scan [3]=descriptors+features. */
int psx_enable_timers(psx_ctx* ctx, int on);
int psx_stage_times(psx_ctx* ctx, float ms[4]);

/* Times `reps` launches of the separable-Gaussian kernel of (octave, level>=1) with HIP events
 * on the context's stream and returns the average duration in ms plus the algorithmic bytes
 * of one launch (8 bytes per pixel: plane read once, written once). */
int psx_time_blur(psx_ctx* ctx, int octave, int level, int reps, float* avg_ms, double* bytes);

/* With the blur probe enabled: in-pipeline durations (stream events around the launch) of octave 0's level 0 and of its
 * extrema scan in the last extraction, and their algorithmic bytes (4 B per octave-0 pixel + the input image;
 * 4 B x (levels + 3) planes per octave-0 pixel read by the scan).  extrema_ms = 0 when the scan shared a launch. */
int psx_probe_extra_times(psx_ctx* ctx, float* level0_ms, double* level0_bytes, float* extrema_ms, double* extrema_bytes);

/* Diagnostic (tests): `rounds` hand-overs of one plain device-memory word from a kernel on one stream -- busy with
 * pcie_words_per_thread stores per thread into mapped host memory -- to a kernel on a second stream behind an event, and
 * back.  *stale = number of rounds in which the reader saw another round's value (0 on a stack where stream order across
 * an event carries plain stores between kernels; the assumption every multi-stream use of this library rests on). */
int psx_debug_cross_stream(int device, int rounds, int pcie_words_per_thread, int* stale);

/* The launch schedule of a frame, on the HOST: no device, no context (csrc/hip/pyramid_plan.h, the function psx_resize
 * itself plans with).  Behind the level-0 launch of octave 0, psx_build_pyramid issues the steps of a plan in order, and
 * psx_find_extrema the scan steps when they did not go out with the pyramid.  A step is a kind and four ints, unused
 * ones 0:
 *   PSX_STEP_BLUR      level b of octave a in one launch
 *   PSX_STEP_BLUR2     levels (a, b) and (c, d) in one launch
 *   PSX_STEP_TILE      launch a of the tile schedule
 *   PSX_STEP_FLOW      the one-launch flow kernel
 *   PSX_STEP_SCAN      the extrema scan of octave a as a launch of its own
 *   PSX_STEP_SCAN_SET  one batched scan of the n <= 4 octaves a, b, c, d
 * The frame is w0 x h0 at octave 0 and halves, rounding up, per octave; spans: the levels + 3 one-sided tap counts of the
 * inc table (psx_gauss_tables); resident_blocks: 4 x the device's compute units (1024 on an MI355X).  The tuning is the
 * environment's, as a context created now would read it.  schedule: PSX_PLAN_DIAGONAL (the default), PSX_PLAN_TILE
 * (POPSIFT_TILE=1: `first` is ignored, the tile schedule decides it; PSX_ERR_STATE where no tile schedule exists and a
 * context keeps the diagonal one) or PSX_PLAN_FLOW (POPSIFT_FLOW=1 / 2: first = 0 / 1, the first octave on the flow
 * kernel).  *count is always the total; the first min(total, capacity) steps are written (capacity 0 with NULL: "how
 * many?").  PSX_ERR_INVALID for a NULL spans or count, a NULL steps with a capacity, a negative capacity, a size, level
 * count or resident_blocks below 1, an octave or level count above the library's limits, an unknown schedule, a flow
 * `first` outside 0, 1 or not below num_octaves. */
#define PSX_STEP_BLUR     1
#define PSX_STEP_BLUR2    2
#define PSX_STEP_TILE     3
#define PSX_STEP_FLOW     4
#define PSX_STEP_SCAN     5
#define PSX_STEP_SCAN_SET 6
#define PSX_PLAN_DIAGONAL 0
#define PSX_PLAN_TILE     1
#define PSX_PLAN_FLOW     2
typedef struct psx_step { int kind, n, a, b, c, d; } psx_step;
int psx_pyramid_plan(int w0, int h0, int num_octaves, int levels, const int* spans, int resident_blocks, int schedule,
                     int first, psx_step* steps, int capacity, int* count);
/* Workgroups a plane-to-plane blur of a W x H plane is launched with at this span, under the environment's tuning: the
 * pairing rule of the diagonal schedule is grid(plane 1) + grid(plane 2) <= resident_blocks at the larger span. */
int psx_blur_grid_of(int W, int H, int span);

/* Measurement: one pyramid build with the whole-pyramid kernel (k_pyramid_flow) recording, per work item and in ticket
 * order, six int64: the 100 MHz wall clock at dequeue / dependencies met / arithmetic done / published, a word
 * (octave << 40 | level << 32 | chunk << 16 | strip) and the workgroup index.  *nitems = items of the current plan
 * (0 when the launch-per-level schedule is in use); call with host_out = NULL to ask for the size. */
int psx_flow_trace(psx_ctx* ctx, long long* host_out, int capacity_items, int* nitems);

/* In-pipeline timing of the dominant kernel: when enabled, every separable-Gaussian launch of octave 0
 * (levels 1..L-1) INSIDE psx_extract / psx_build_pyramid carries a begin and an end event of its own
 * dispatch (hipExtLaunchKernel: the kernel's start / end timestamps, the quantity rocprofv3 --kernel-trace
 * reports); the launches run back to back with their real producers and consumers, not replayed in isolation.
 * psx_blur_probe_times synchronises and returns the n = L-1 durations (ms) of the last extraction plus the
 * algorithmic bytes of one launch, averaged over the n launches (8 B per pixel of every plane a launch blurs:
 * octave 0, and from level 4 on also the level of octave 1 that shares the launch). */
int psx_enable_blur_probe(psx_ctx* ctx, int on);
int psx_blur_probe_times(psx_ctx* ctx, float* ms, int capacity, int* n, double* bytes_per_launch);

/* Measured HBM roofline: a hand-written 16 B-per-lane streaming copy kernel over `bytes`
 * (0 = 1 GiB) read + `bytes` written, `reps` timed launches after warm-up, HIP events on its own stream;
 * the better of a plain and a non-temporal variant.  avg_ms per launch, bytes_moved = 2 * bytes. */
int psx_copy_bench(int device, size_t bytes, int reps, float* avg_ms, double* bytes_moved);

/* The HIP stream of the context as an opaque handle (hipStream_t), for callers that need to
 * order their own work (e.g. a torch tensor producer) against it. */
void* psx_stream(psx_ctx* ctx);

/* Library version / build info string. */
const char* psx_version(void);

#ifdef __cplusplus
}
#endif
#endif /* POPSIFT_HIP_H */
