// ransac.hip -- geometric verification: a homography, a fundamental matrix, a 2-D affine transform or a similarity from
// matched pairs by RANSAC on the device (psx_ransac_homography*, psx_ransac_samples, psx_homography_fit,
// psx_ransac_homography_ref; psx_ransac_fundamental*, psx_ransac_samples_k, psx_fundamental_fit,
// psx_ransac_fundamental_ref; psx_ransac_affine*, psx_affine_fit, psx_ransac_similarity*, psx_similarity_fit;
// include/popsift_hip.h).
//
// The rule -- samples, fit, score, select, refit, inliers -- is ransac_rule.h (homography), fundamental_rule.h
// (fundamental matrix) and affine_rule.h (affine, similarity), shared with the host references; the steps of the estimator around them are ransac_core.h, shared
// with the batched driver (ransac_graph.hip).  This file is the call for ONE pair list: kernels that say where a step's
// operands live, and the sequence.  Kernels that evaluate the rule are templates on the model id (RModel).
//   k_ransac_gather  r_gather per pair: the four floats, once, into a packed float4 array; everything after it streams 16 B
//                    per lane, coalesced
//   k_ransac_hyp     one lane per hypothesis: r_sample_fit (four indices and the 4-point fit, eight and the pivoted
//                    8-point fit, or two / three and the similarity / affine fit, in registers); writes the model, clears the count
//   k_ransac_score   the hot kernel, N x n rule evaluations.  Lanes own pairs: R_PPL float4, strided over the workgroup,
//                    stay in VGPRs; r_score_walk over a block of R_HB hypotheses with the strides 9 and 1 as literals
//   k_ransac_select  r_select by a single workgroup
//   k_ransac_inl_count / _write   r_keep into the stable compaction of wg_compact.h, as the pair join (match.hip) runs it;
//                    the payload is any 16-byte record array (the float4s for the refit, the pair records at the end)
//   k_ransac_decide  r_decide for the one set
// The state is the batched call's layout with K = 1 (ROne).  The refit's fit is serial by definition: the winner's float4s
// come to the host through the pinned staging buffer, the model goes back as an RRefit and is scored by the score kernel
// with N = 1.  A memset, then gather, hyp, score, select and the compaction's 2 -- 6 kernels and 1 synchronisation without
// the refit; with it the refit's upload and 4 more kernels (score, decide, the compaction's 2) -- 11 launches and 2.
#include "psx_internal.h"
#include "ransac_core.h"
#include "wg_compact.h"

#include <cstddef>
#include <cstring>
#include <new>

namespace {

constexpr int R_PPL = 4;                     // pairs resident per lane of the score kernel
constexpr int R_HB = 64;                     // hypotheses per workgroup of the score kernel

struct ROne { RHead head; RState state; RRefit refit; };                   // the state layout of ransac_core.h with K = 1
constexpr size_t R_STATE_BYTES = offsetof(ROne, refit);                    // zeroed at the start, downloaded at the end of a stage
static_assert(R_STATE_BYTES == sizeof(RHead) + sizeof(RState) && R_STATE_BYTES % 16 == 0, "state layout");

__global__ void k_ransac_gather(const int4* __restrict__ pairs, int n, const float2* __restrict__ lxy, int l_len,
                                const float2* __restrict__ rxy, int r_len, float4* __restrict__ pts, int* __restrict__ bad)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    r_gather(pairs[p], lxy, l_len, rxy, r_len, pts + p, bad);
}

template <int KIND>
__global__ __launch_bounds__(64) void k_ransac_hyp(const float4* __restrict__ pts, int n, unsigned seed, int N,
                                                   float* __restrict__ models, int* __restrict__ counts)
{
    const int h = blockIdx.x * blockDim.x + threadIdx.x;
    if (h >= N) return;
    float m[9];
    r_sample_fit<KIND>(pts, n, seed, h, m);
#pragma unroll
    for (int k = 0; k < 9; k++) models[9 * (size_t)h + k] = m[k];
    counts[h] = 0;
}

// grid (ceil(n / (256 R_PPL)), ceil(N / R_HB)), 256 threads; the resident pairs are strided over the workgroup
template <int KIND>
__global__ __launch_bounds__(256) void k_ransac_score(const float4* __restrict__ pts, int n, const float* __restrict__ models, int N,
                                                      float tol, int* __restrict__ counts)
{
    const int base = blockIdx.x * (256 * R_PPL) + threadIdx.x;
    psx_ransac_pt q[R_PPL];
    bool in[R_PPL];
#pragma unroll
    for (int k = 0; k < R_PPL; k++) {
        const int p = base + k * 256;
        in[k] = p < n;
        q[k] = r_pt(in[k] ? pts[p] : make_float4(0.f, 0.f, 0.f, 0.f));
    }
    const int h0 = blockIdx.y * R_HB;
    r_score_walk<KIND, R_PPL>(q, in, models, counts, 0, 9, 1, h0, h0 + R_HB < N ? h0 + R_HB : N, tol);
}

// one workgroup of 256 threads
__global__ __launch_bounds__(256) void k_ransac_select(const int* __restrict__ counts, int N, const float* __restrict__ models,
                                                       ROne* __restrict__ st)
{
    r_select(counts, N, models, &st->state);
}

// the call has one set, and it is launched only behind a refit that was tried
template <int KIND>
__global__ void k_ransac_decide(ROne* __restrict__ st)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    r_decide<KIND>(&st->state, &st->refit, 0);
}

template <int KIND>
__global__ __launch_bounds__(256) void k_ransac_inl_count(const float4* __restrict__ pts, int n, const ROne* __restrict__ st, float tol,
                                                          int* __restrict__ wg_tot)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    __shared__ int s_cnt[4];
    wg_count(__ballot(r_keep<KIND>(&st->head, &st->state, i < n, pts, i, tol)), s_cnt);
    if (threadIdx.x == 0) wg_tot[blockIdx.x] = wg_total(s_cnt);
}

// src: n 16-byte records (the correspondences themselves, or the pair records); out: never written at or past `capacity`
template <int KIND>
__global__ __launch_bounds__(256) void k_ransac_inl_write(const float4* __restrict__ pts, int n, const ROne* __restrict__ st, float tol,
                                                          const int* __restrict__ wg_tot, const int4* __restrict__ src,
                                                          int4* __restrict__ out, int capacity, int* __restrict__ total)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool keep = r_keep<KIND>(&st->head, &st->state, i < n, pts, i, tol);
    const int pos = wg_slot(__ballot(keep), wg_tot, total);
    if (keep && pos < capacity) out[pos] = src[i];
}

constexpr size_t R_PIN_STATE = 0, R_PIN_REFIT = 128, R_PIN_REC = 256;      // layout of the pinned staging buffer
static_assert(R_STATE_BYTES <= R_PIN_REFIT && sizeof(RRefit) <= R_PIN_REC - R_PIN_REFIT, "pinned layout");

template <int KIND>
void queue_score(hipStream_t st, const float4* d_pts, int n, const float* d_models, int N, float tol, int* d_counts)
{
    const dim3 grid((unsigned)((n + 256 * R_PPL - 1) / (256 * R_PPL)), (unsigned)((N + R_HB - 1) / R_HB));
    hipLaunchKernelGGL(k_ransac_score<KIND>, grid, dim3(256), 0, st, d_pts, n, d_models, N, tol, d_counts);
}

template <int KIND>
void queue_compact(hipStream_t st, const float4* d_pts, int n, ROne* d_state, float tol, int* d_tot, const void* src, void* out, int cap)
{
    const int nb = (n + 255) / 256;
    hipLaunchKernelGGL(k_ransac_inl_count<KIND>, dim3(nb), dim3(256), 0, st, d_pts, n, d_state, tol, d_tot);
    hipLaunchKernelGGL(k_ransac_inl_write<KIND>, dim3(nb), dim3(256), 0, st, d_pts, n, d_state, tol, d_tot, static_cast<const int4*>(src),
                       static_cast<int4*>(out), cap, &d_state->state.total);
}

// host_pairs or d_pairs_in; host_inl or d_inl (the other is NULL; both NULL with capacity 0)
template <int KIND>
int ransac_run(int device, const void* host_pairs, const void* d_pairs_in, int n, const float* d_lxy, int l_len, const float* d_rxy, int r_len,
               const psx_ransac_opts* opts, psx_ransac_result* result, void* host_inl, void* d_inl, int capacity, int* count,
               float* host_models, int* host_counts)
{
    const void* in = host_pairs ? host_pairs : d_pairs_in;
    const void* outp = host_inl ? host_inl : d_inl;
    if (!psx_ransac_opts_ok(opts) || !result || !count || n < 0 || n > 0x3fffffff || l_len < 0 || r_len < 0 || capacity < 0 ||
        (n > 0 && !in) || (l_len > 0 && !d_lxy) || (r_len > 0 && !d_rxy) || (capacity > 0 && !outp))
        return PSX_ERR_INVALID;
    constexpr int MIN = RModel<KIND>::MIN;
    if (n < MIN) { psx_ransac_no_model(result); *count = 0; return PSX_OK; }
    if (l_len == 0 || r_len == 0) return PSX_ERR_INVALID;                 // no index can lie inside an empty array
    if (hipSetDevice(device) != hipSuccess) return PSX_ERR_HIP;
    MatchScratch& sc = psx_match_scratch();
    if (!sc.bind(device)) return PSX_ERR_HIP;
    const int N = opts->hypotheses;
    const float tol = opts->tol;
    const bool refit = (opts->flags & PSX_RANSAC_REFIT) != 0;
    const int nb = (n + 255) / 256;
    const int nrec = host_inl ? (capacity < n ? capacity : n) : 0;
    // every buffer before the first launch: nothing is reallocated under queued work
    if ((host_pairs && !sc.need(MS_RANSAC_PAIRS, 16 * (size_t)n)) || !sc.need(MS_RANSAC_PTS, 16 * (size_t)n) || !sc.need(MS_RANSAC_MODELS, sizeof(float) * 9 * (size_t)N) ||
        !sc.need(MS_RANSAC_COUNTS, sizeof(int) * (size_t)N) || !sc.need(MS_RANSAC_STATE, sizeof(ROne)) || !sc.need(MS_RANSAC_TOT, sizeof(int) * (size_t)nb) ||
        !sc.need_pinned(R_PIN_REC + 16 * (size_t)(refit ? n : nrec)))
        return PSX_ERR_NOMEM;
    void* dev_pin = r_pinned_dev(sc);
    if (dev_pin == nullptr) return PSX_ERR_HIP;
    char* hpin = static_cast<char*>(sc.hpin);
    void* pin_rec = static_cast<char*>(dev_pin) + R_PIN_REC;
    hipStream_t st = sc.stream;
    const void* d_pairs = d_pairs_in;
    if (host_pairs) {
        if (hipMemcpyAsync(sc.buf[MS_RANSAC_PAIRS], host_pairs, 16 * (size_t)n, hipMemcpyHostToDevice, st) != hipSuccess) return PSX_ERR_HIP;
        d_pairs = sc.buf[MS_RANSAC_PAIRS];
    }
    float4* d_pts = static_cast<float4*>(sc.buf[MS_RANSAC_PTS]);
    float* d_models = static_cast<float*>(sc.buf[MS_RANSAC_MODELS]);
    int* d_counts = static_cast<int*>(sc.buf[MS_RANSAC_COUNTS]);
    ROne* d_state = static_cast<ROne*>(sc.buf[MS_RANSAC_STATE]);
    int* d_tot = static_cast<int*>(sc.buf[MS_RANSAC_TOT]);
    const ROne* hs = reinterpret_cast<const ROne*>(hpin + R_PIN_STATE);   // head and state: the refit part is not downloaded
    const RState& s = hs->state;
    void* final_out = host_inl ? pin_rec : d_inl;
    const int final_cap = host_inl ? nrec : capacity;

    if (hipMemsetAsync(d_state, 0, R_STATE_BYTES, st) != hipSuccess) return PSX_ERR_HIP;
    hipLaunchKernelGGL(k_ransac_gather, dim3(nb), dim3(256), 0, st, static_cast<const int4*>(d_pairs), n, reinterpret_cast<const float2*>(d_lxy),
                       l_len, reinterpret_cast<const float2*>(d_rxy), r_len, d_pts, &d_state->head.bad);
    hipLaunchKernelGGL(k_ransac_hyp<KIND>, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, st, d_pts, n, opts->seed, N, d_models, d_counts);
    queue_score<KIND>(st, d_pts, n, d_models, N, tol, d_counts);
    hipLaunchKernelGGL(k_ransac_select, dim3(1), dim3(256), 0, st, d_counts, N, d_models, d_state);
    // with the refit: the winner's correspondences to the host; without: the inlier records, and the call is complete
    if (refit) queue_compact<KIND>(st, d_pts, n, d_state, tol, d_tot, d_pts, pin_rec, n);
    else queue_compact<KIND>(st, d_pts, n, d_state, tol, d_tot, d_pairs, final_out, final_cap);
    if (!r_stage_end(st, hpin + R_PIN_STATE, d_state, R_STATE_BYTES)) return PSX_ERR_HIP;
    if (hs->head.bad != 0) return PSX_ERR_INVALID;
    if (s.best < 0 || s.best >= N || s.total < 0 || s.total > n) return PSX_ERR_HIP;
    if (refit) {
        RRefit* up = reinterpret_cast<RRefit*>(hpin + R_PIN_REFIT);
        if (r_refit_model<KIND>(s, reinterpret_cast<const psx_ransac_pt*>(hpin + R_PIN_REC), up)) {
            if (hipMemcpyAsync(&d_state->refit, up, sizeof(RRefit), hipMemcpyHostToDevice, st) != hipSuccess) return PSX_ERR_HIP;
            queue_score<KIND>(st, d_pts, n, d_state->refit.m, 1, tol, &d_state->refit.count);
            hipLaunchKernelGGL(k_ransac_decide<KIND>, dim3(1), dim3(64), 0, st, d_state);
        }
        queue_compact<KIND>(st, d_pts, n, d_state, tol, d_tot, d_pairs, final_out, final_cap);
        if (!r_stage_end(st, hpin + R_PIN_STATE, d_state, R_STATE_BYTES)) return PSX_ERR_HIP;
        if (s.total < 0 || s.total > n) return PSX_ERR_HIP;
    }
    if (!r_download_layers(st, host_models, d_models, host_counts, d_counts, (size_t)N)) return PSX_ERR_HIP;
    if (!r_result<KIND>(s, result)) { *count = 0; return PSX_OK; }
    const int total = s.total;
    if (host_inl && total > 0 && nrec > 0) memcpy(host_inl, hpin + R_PIN_REC, 16 * (size_t)(total < nrec ? total : nrec));
    *count = total;
    return PSX_OK;
}

// psx_*_fit: the xy arrays packed into correspondences, then the model's serial fit
template <int KIND>
int fit_xy(const float* left_xy, const float* right_xy, int n, float* m)
{
    if (n < RModel<KIND>::MIN || !left_xy || !right_xy || !m) return PSX_ERR_INVALID;
    psx_ransac_pt* pt = new (std::nothrow) psx_ransac_pt[(size_t)n];
    if (!pt) return PSX_ERR_NOMEM;
    for (int i = 0; i < n; i++) {
        pt[i].xl = left_xy[2 * (size_t)i]; pt[i].yl = left_xy[2 * (size_t)i + 1];
        pt[i].xr = right_xy[2 * (size_t)i]; pt[i].yr = right_xy[2 * (size_t)i + 1];
    }
    RModel<KIND>::fit(pt, n, m);
    delete[] pt;
    return PSX_OK;
}

// psx_ransac_*_ref: the model's host rule on a scratch of n correspondences
template <int KIND>
int ransac_ref(const void* pairs, int n, const float* left_xy, int nl, const float* right_xy, int nr, const psx_ransac_opts* opts,
               psx_ransac_result* result, void* inliers, int capacity, int* count, float* models, int* counts)
{
    psx_ransac_pt* scratch = n >= RModel<KIND>::MIN ? new (std::nothrow) psx_ransac_pt[(size_t)n] : nullptr;
    if (n >= RModel<KIND>::MIN && !scratch) return PSX_ERR_NOMEM;
    const int rc = psx_ransac_host_rule(KIND)(pairs, n, left_xy, nl, right_xy, nr, opts, result, inliers, capacity, count, models, counts, scratch);
    delete[] scratch;
    return rc;
}

} // namespace

extern "C" int psx_ransac_opts_default(psx_ransac_opts* o)
{
    if (!o) return PSX_ERR_INVALID;
    o->tol = 2.0f; o->hypotheses = 1024; o->seed = 0u; o->flags = PSX_RANSAC_REFIT;
    return PSX_OK;
}

extern "C" int psx_ransac_samples(unsigned seed, int first, int count, int n, int* idx)
{
    if (n < 4 || first < 0 || count < 0 || first > PSX_RANSAC_MAX_HYPOTHESES - count || (count > 0 && !idx)) return PSX_ERR_INVALID;
    for (int i = 0; i < count; i++) psx_ransac_sample(seed, first + i, n, idx + 4 * (size_t)i);
    return PSX_OK;
}

extern "C" int psx_homography_fit(const float* left_xy, const float* right_xy, int n, float* m)
{
    return fit_xy<PSX_RANSAC_MODEL_HOMOGRAPHY>(left_xy, right_xy, n, m);
}

extern "C" int psx_ransac_homography_ref(const void* pairs, int n, const float* left_xy, int nl, const float* right_xy, int nr,
                                         const psx_ransac_opts* opts, psx_ransac_result* result, void* inliers, int capacity, int* count,
                                         float* models, int* counts)
{
    return ransac_ref<PSX_RANSAC_MODEL_HOMOGRAPHY>(pairs, n, left_xy, nl, right_xy, nr, opts, result, inliers, capacity, count, models, counts);
}

extern "C" int psx_ransac_homography(int device, const void* host_pairs, int n, const float* d_left_xy, int l_len,
                                     const float* d_right_xy, int r_len, const psx_ransac_opts* opts, psx_ransac_result* result,
                                     void* host_inliers, int capacity, int* count, float* host_models, int* host_counts)
{
    return ransac_run<PSX_RANSAC_MODEL_HOMOGRAPHY>(device, host_pairs, nullptr, n, d_left_xy, l_len, d_right_xy, r_len, opts, result, host_inliers, nullptr, capacity, count,
                      host_models, host_counts);
}

extern "C" int psx_ransac_homography_dev(int device, const void* d_pairs, int n, const float* d_left_xy, int l_len,
                                         const float* d_right_xy, int r_len, const psx_ransac_opts* opts, psx_ransac_result* result,
                                         void* d_inliers, int capacity, int* count, float* host_models, int* host_counts)
{
    return ransac_run<PSX_RANSAC_MODEL_HOMOGRAPHY>(device, nullptr, d_pairs, n, d_left_xy, l_len, d_right_xy, r_len, opts, result, nullptr, d_inliers, capacity, count,
                      host_models, host_counts);
}

extern "C" int psx_ransac_samples_k(unsigned seed, int first, int count, int n, int k, int* idx)
{
    if ((k != PSX_SIMILARITY_MIN && k != PSX_AFFINE_MIN && k != 4 && k != PSX_FUND_MIN) || n < k || first < 0 || count < 0 || first > PSX_RANSAC_MAX_HYPOTHESES - count || (count > 0 && !idx))
        return PSX_ERR_INVALID;
    for (int i = 0; i < count; i++) {
        if (k == PSX_SIMILARITY_MIN) psx_ransac_sample_k<PSX_SIMILARITY_MIN>(seed, first + i, n, idx + PSX_SIMILARITY_MIN * (size_t)i);
        else if (k == PSX_AFFINE_MIN) psx_ransac_sample_k<PSX_AFFINE_MIN>(seed, first + i, n, idx + PSX_AFFINE_MIN * (size_t)i);
        else if (k == 4) psx_ransac_sample_k<4>(seed, first + i, n, idx + 4 * (size_t)i);
        else psx_ransac_sample_k<PSX_FUND_MIN>(seed, first + i, n, idx + PSX_FUND_MIN * (size_t)i);
    }
    return PSX_OK;
}

extern "C" int psx_fundamental_fit(const float* left_xy, const float* right_xy, int n, float* m)
{
    return fit_xy<PSX_RANSAC_MODEL_FUNDAMENTAL>(left_xy, right_xy, n, m);
}

extern "C" int psx_ransac_fundamental_ref(const void* pairs, int n, const float* left_xy, int nl, const float* right_xy, int nr,
                                          const psx_ransac_opts* opts, psx_ransac_result* result, void* inliers, int capacity, int* count,
                                          float* models, int* counts)
{
    return ransac_ref<PSX_RANSAC_MODEL_FUNDAMENTAL>(pairs, n, left_xy, nl, right_xy, nr, opts, result, inliers, capacity, count, models, counts);
}

extern "C" int psx_ransac_fundamental(int device, const void* host_pairs, int n, const float* d_left_xy, int l_len,
                                      const float* d_right_xy, int r_len, const psx_ransac_opts* opts, psx_ransac_result* result,
                                      void* host_inliers, int capacity, int* count, float* host_models, int* host_counts)
{
    return ransac_run<PSX_RANSAC_MODEL_FUNDAMENTAL>(device, host_pairs, nullptr, n, d_left_xy, l_len, d_right_xy, r_len, opts, result, host_inliers, nullptr,
                                          capacity, count, host_models, host_counts);
}

extern "C" int psx_ransac_fundamental_dev(int device, const void* d_pairs, int n, const float* d_left_xy, int l_len,
                                          const float* d_right_xy, int r_len, const psx_ransac_opts* opts, psx_ransac_result* result,
                                          void* d_inliers, int capacity, int* count, float* host_models, int* host_counts)
{
    return ransac_run<PSX_RANSAC_MODEL_FUNDAMENTAL>(device, nullptr, d_pairs, n, d_left_xy, l_len, d_right_xy, r_len, opts, result, nullptr, d_inliers,
                                          capacity, count, host_models, host_counts);
}

extern "C" int psx_affine_fit(const float* left_xy, const float* right_xy, int n, float* m)
{
    return fit_xy<PSX_RANSAC_MODEL_AFFINE>(left_xy, right_xy, n, m);
}

extern "C" int psx_ransac_affine_ref(const void* pairs, int n, const float* left_xy, int nl, const float* right_xy, int nr,
                                   const psx_ransac_opts* opts, psx_ransac_result* result, void* inliers, int capacity, int* count,
                                   float* models, int* counts)
{
    return ransac_ref<PSX_RANSAC_MODEL_AFFINE>(pairs, n, left_xy, nl, right_xy, nr, opts, result, inliers, capacity, count, models, counts);
}

extern "C" int psx_ransac_affine(int device, const void* host_pairs, int n, const float* d_left_xy, int l_len,
                               const float* d_right_xy, int r_len, const psx_ransac_opts* opts, psx_ransac_result* result,
                               void* host_inliers, int capacity, int* count, float* host_models, int* host_counts)
{
    return ransac_run<PSX_RANSAC_MODEL_AFFINE>(device, host_pairs, nullptr, n, d_left_xy, l_len, d_right_xy, r_len, opts, result, host_inliers, nullptr,
                          capacity, count, host_models, host_counts);
}

extern "C" int psx_ransac_affine_dev(int device, const void* d_pairs, int n, const float* d_left_xy, int l_len,
                                   const float* d_right_xy, int r_len, const psx_ransac_opts* opts, psx_ransac_result* result,
                                   void* d_inliers, int capacity, int* count, float* host_models, int* host_counts)
{
    return ransac_run<PSX_RANSAC_MODEL_AFFINE>(device, nullptr, d_pairs, n, d_left_xy, l_len, d_right_xy, r_len, opts, result, nullptr, d_inliers,
                          capacity, count, host_models, host_counts);
}

extern "C" int psx_similarity_fit(const float* left_xy, const float* right_xy, int n, float* m)
{
    return fit_xy<PSX_RANSAC_MODEL_SIMILARITY>(left_xy, right_xy, n, m);
}

extern "C" int psx_ransac_similarity_ref(const void* pairs, int n, const float* left_xy, int nl, const float* right_xy, int nr,
                                   const psx_ransac_opts* opts, psx_ransac_result* result, void* inliers, int capacity, int* count,
                                   float* models, int* counts)
{
    return ransac_ref<PSX_RANSAC_MODEL_SIMILARITY>(pairs, n, left_xy, nl, right_xy, nr, opts, result, inliers, capacity, count, models, counts);
}

extern "C" int psx_ransac_similarity(int device, const void* host_pairs, int n, const float* d_left_xy, int l_len,
                               const float* d_right_xy, int r_len, const psx_ransac_opts* opts, psx_ransac_result* result,
                               void* host_inliers, int capacity, int* count, float* host_models, int* host_counts)
{
    return ransac_run<PSX_RANSAC_MODEL_SIMILARITY>(device, host_pairs, nullptr, n, d_left_xy, l_len, d_right_xy, r_len, opts, result, host_inliers, nullptr,
                          capacity, count, host_models, host_counts);
}

extern "C" int psx_ransac_similarity_dev(int device, const void* d_pairs, int n, const float* d_left_xy, int l_len,
                                   const float* d_right_xy, int r_len, const psx_ransac_opts* opts, psx_ransac_result* result,
                                   void* d_inliers, int capacity, int* count, float* host_models, int* host_counts)
{
    return ransac_run<PSX_RANSAC_MODEL_SIMILARITY>(device, nullptr, d_pairs, n, d_left_xy, l_len, d_right_xy, r_len, opts, result, nullptr, d_inliers,
                          capacity, count, host_models, host_counts);
}
