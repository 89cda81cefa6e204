// ransac.hip -- geometric verification: a homography or a fundamental matrix from matched pairs by RANSAC on the device
// (psx_ransac_homography*, psx_ransac_samples, psx_homography_fit, psx_ransac_homography_ref; psx_ransac_fundamental*,
// psx_ransac_samples_k, psx_fundamental_fit, psx_ransac_fundamental_ref; include/popsift_hip.h).
//
// The rule -- samples, fit, score, select, refit, inliers -- is ransac_rule.h (homography) and fundamental_rule.h
// (fundamental matrix), shared with the host references; this file is the estimator around them.  Kernels that evaluate
// the inlier test are templates on the model kind (RModel), everything else serves both.
//   k_ransac_gather  the four floats of every pair, once, into a packed float4 array (out-of-range indices raise a flag and
//                    read nothing); everything after it streams 16 B per lane, coalesced
//   k_ransac_hyp     one lane per hypothesis: the sample's four indices, their float4s and the double-precision fit, all
//                    loops of constant trip count (registers); writes the model, clears the count
//   k_ransac_hyp_fund  the same for the fundamental matrix: eight indices, the pivoted 8-point fit, still in registers
//   k_ransac_score   the hot kernel, N x n rule evaluations.  Lanes own pairs: R_PPL float4 stay in VGPRs; the workgroup
//                    walks a block of R_HB hypotheses whose nine floats sit at a wave-uniform address (scalar loads); per
//                    hypothesis one wave64 ballot + popcount per resident pair and ONE integer atomic per wave -- integer
//                    atomics are order-free, the counts are deterministic
//   k_ransac_select  single workgroup arg-max on (count descending, index ascending); copies the winner's model
//   k_ransac_inl_count / _write   the stable compaction of wg_compact.h, as the pair join (match.hip) runs it; the payload is
//                    any 16-byte record array (the float4s for the refit, the pair records at the end)
//   k_ransac_decide  keeps the refit model iff it may score and its count is not below the winner's
// The refit's fit is serial by definition: the winner's float4s come to the host through the pinned staging buffer, the
// model goes back and is scored by the score kernel with N = 1.  One synchronisation without the refit, two with it.
#include "psx_internal.h"
#include "match_scratch.h"
#include "ransac_model.h"
#include "wg_compact.h"

#include <cstring>
#include <new>

namespace {

constexpr int R_PPL = 4;                     // pairs resident per lane of the score kernel
constexpr int R_HB = 64;                     // hypotheses per workgroup of the score kernel

struct RState {                              // device resident, copied to the host at the end of a stage
    float kept[9];
    int best, sample_inliers, refit_kept, bad, total;
    int refit_count, pad;                    // from here: uploaded before the refit's score launch (11 words)
    float refit[9];
};

// RModel<KIND> -- what differs between the two estimators -- , r_pt and r_better: ransac_model.h

__global__ void k_ransac_gather(const int4* __restrict__ pairs, int n, const float2* __restrict__ lxy, int l_len,
                                const float2* __restrict__ rxy, int r_len, float4* __restrict__ pts, int* __restrict__ bad)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const int4 rec = pairs[p];
    if (rec.x < 0 || rec.x >= l_len || rec.y < 0 || rec.y >= r_len) {
        atomicOr(bad, 1);
        pts[p] = make_float4(NAN, NAN, NAN, NAN);
        return;
    }
    const float2 a = lxy[rec.x], b = rxy[rec.y];
    pts[p] = make_float4(a.x, a.y, b.x, b.y);
}

__global__ __launch_bounds__(64) void k_ransac_hyp(const float4* __restrict__ pts, int n, unsigned seed, int N,
                                                   float* __restrict__ models, int* __restrict__ counts)
{
    const int h = blockIdx.x * blockDim.x + threadIdx.x;
    if (h >= N) return;
    int idx[4];
    psx_ransac_sample(seed, h, n, idx);
    psx_ransac_pt q[4];
#pragma unroll
    for (int k = 0; k < 4; k++) q[k] = r_pt(pts[idx[k]]);
    float m[9];
    psx_homography_fit_rule<4>(q, 4, m);
#pragma unroll
    for (int k = 0; k < 9; k++) models[9 * (size_t)h + k] = m[k];
    counts[h] = 0;
}

// the same for a fundamental matrix: eight indices, their float4s, the fit of fundamental_rule.h
__global__ __launch_bounds__(64) void k_ransac_hyp_fund(const float4* __restrict__ pts, int n, unsigned seed, int N,
                                                        float* __restrict__ models, int* __restrict__ counts)
{
    const int h = blockIdx.x * blockDim.x + threadIdx.x;
    if (h >= N) return;
    int idx[PSX_FUND_MIN];
    psx_ransac_sample_k<PSX_FUND_MIN>(seed, h, n, idx);
    psx_ransac_pt q[PSX_FUND_MIN];
#pragma unroll
    for (int k = 0; k < PSX_FUND_MIN; k++) q[k] = r_pt(pts[idx[k]]);
    float m[9];
    psx_fundamental_fit_rule<PSX_FUND_MIN>(q, PSX_FUND_MIN, m);
#pragma unroll
    for (int k = 0; k < 9; k++) models[9 * (size_t)h + k] = m[k];
    counts[h] = 0;
}

// grid (ceil(n / (256 R_PPL)), ceil(N / R_HB)), 256 threads
template <int KIND>
__global__ __launch_bounds__(256) void k_ransac_score(const float4* __restrict__ pts, int n, const float* __restrict__ models, int N,
                                                      float tol, int* __restrict__ counts)
{
    const int lane = threadIdx.x & 63;
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
    const int h1 = h0 + R_HB < N ? h0 + R_HB : N;
    for (int h = h0; h < h1; h++) {
        float m[9];
#pragma unroll
        for (int k = 0; k < 9; k++) m[k] = models[9 * (size_t)h + k];       // wave-uniform address
        if (!RModel<KIND>::usable(m)) continue;                           // wave uniform
        int c = 0;
#pragma unroll
        for (int k = 0; k < R_PPL; k++) {
            const psx_guide_line l = psx_guide_left(KIND, m, tol, q[k].xl, q[k].yl);
            c += __popcll(__ballot(in[k] && psx_guide_right(KIND, l, q[k].xr, q[k].yr)));
        }
        if (lane == 0 && c > 0) atomicAdd(counts + h, c);
    }
}

// one workgroup of 256 threads
__global__ __launch_bounds__(256) void k_ransac_select(const int* __restrict__ counts, int N, const float* __restrict__ models,
                                                       RState* __restrict__ st)
{
    int bc = -1, bh = 0x7fffffff;
    for (int h = threadIdx.x; h < N; h += 256) r_better(bc, bh, counts[h], h);
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) {
        const int oc = __shfl_xor(bc, k), oh = __shfl_xor(bh, k);
        r_better(bc, bh, oc, oh);
    }
    __shared__ int s_c[4], s_h[4];
    if ((threadIdx.x & 63) == 0) { s_c[threadIdx.x >> 6] = bc; s_h[threadIdx.x >> 6] = bh; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; w++) r_better(bc, bh, s_c[w], s_h[w]);
        st->best = bh; st->sample_inliers = bc;                            // N >= 1: thread 0 saw hypothesis 0
        for (int k = 0; k < 9; k++) st->kept[k] = models[9 * (size_t)bh + k];
    }
}

template <int KIND>
__global__ void k_ransac_decide(RState* __restrict__ st)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (RModel<KIND>::usable(st->refit) && st->refit_count >= st->sample_inliers) {
        for (int k = 0; k < 9; k++) st->kept[k] = st->refit[k];
        st->refit_kept = 1;
    }
}

// keep: pair i passes under the state's kept model (no pair does under one that may not score, or after a bad index)
template <int KIND>
__device__ __forceinline__ bool r_keep(const float4* __restrict__ pts, int n, const RState* __restrict__ st, float tol, int i)
{
    float m[9];
#pragma unroll
    for (int k = 0; k < 9; k++) m[k] = st->kept[k];
    if (st->bad != 0 || !RModel<KIND>::usable(m) || i >= n) return false;
    const psx_ransac_pt p = r_pt(pts[i]);
    return psx_guide_right(KIND, psx_guide_left(KIND, m, tol, p.xl, p.yl), p.xr, p.yr);
}

template <int KIND>
__global__ __launch_bounds__(256) void k_ransac_inl_count(const float4* __restrict__ pts, int n, const RState* __restrict__ st, float tol,
                                                          int* __restrict__ wg_tot)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    __shared__ int s_cnt[4];
    wg_count(__ballot(r_keep<KIND>(pts, n, st, tol, i)), s_cnt);
    if (threadIdx.x == 0) wg_tot[blockIdx.x] = wg_total(s_cnt);
}

// src: n 16-byte records (the correspondences themselves, or the pair records); out: never written at or past `capacity`
template <int KIND>
__global__ __launch_bounds__(256) void k_ransac_inl_write(const float4* __restrict__ pts, int n, const RState* __restrict__ st, float tol,
                                                          const int* __restrict__ wg_tot, const int4* __restrict__ src,
                                                          int4* __restrict__ out, int capacity, int* __restrict__ total)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool keep = r_keep<KIND>(pts, n, st, tol, i);
    const int pos = wg_slot(__ballot(keep), wg_tot, total);
    if (keep && pos < capacity) out[pos] = src[i];
}

constexpr size_t R_PIN_STATE = 0, R_PIN_REFIT = 128, R_PIN_REC = 256;      // layout of the pinned staging buffer
static_assert(sizeof(RState) <= R_PIN_REFIT, "RState layout");

template <int KIND>
void queue_score(hipStream_t st, const float4* d_pts, int n, const float* d_models, int N, float tol, int* d_counts)
{
    const dim3 grid((unsigned)((n + 256 * R_PPL - 1) / (256 * R_PPL)), (unsigned)((N + R_HB - 1) / R_HB));
    hipLaunchKernelGGL(k_ransac_score<KIND>, grid, dim3(256), 0, st, d_pts, n, d_models, N, tol, d_counts);
}

template <int KIND>
void queue_compact(hipStream_t st, const float4* d_pts, int n, RState* d_state, float tol, int* d_tot, const void* src, void* out, int cap)
{
    const int nb = (n + 255) / 256;
    hipLaunchKernelGGL(k_ransac_inl_count<KIND>, dim3(nb), dim3(256), 0, st, d_pts, n, d_state, tol, d_tot);
    hipLaunchKernelGGL(k_ransac_inl_write<KIND>, dim3(nb), dim3(256), 0, st, d_pts, n, d_state, tol, d_tot, static_cast<const int4*>(src),
                       static_cast<int4*>(out), cap, &d_state->total);
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
        !sc.need(MS_RANSAC_COUNTS, sizeof(int) * (size_t)N) || !sc.need(MS_RANSAC_STATE, sizeof(RState)) || !sc.need(MS_RANSAC_TOT, sizeof(int) * (size_t)nb) ||
        !sc.need_pinned(R_PIN_REC + 16 * (size_t)(refit ? n : nrec)))
        return PSX_ERR_NOMEM;
    void* dev_pin = nullptr;
    if (hipHostGetDevicePointer(&dev_pin, sc.hpin, 0) != hipSuccess || dev_pin == nullptr) return PSX_ERR_HIP;
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
    RState* d_state = static_cast<RState*>(sc.buf[MS_RANSAC_STATE]);
    int* d_tot = static_cast<int*>(sc.buf[MS_RANSAC_TOT]);
    const RState* hs = reinterpret_cast<const RState*>(hpin + R_PIN_STATE);
    void* final_out = host_inl ? pin_rec : d_inl;
    const int final_cap = host_inl ? nrec : capacity;

    if (hipMemsetAsync(d_state, 0, sizeof(RState), st) != hipSuccess) return PSX_ERR_HIP;
    hipLaunchKernelGGL(k_ransac_gather, dim3(nb), dim3(256), 0, st, static_cast<const int4*>(d_pairs), n, reinterpret_cast<const float2*>(d_lxy),
                       l_len, reinterpret_cast<const float2*>(d_rxy), r_len, d_pts, &d_state->bad);
    if (KIND == PSX_GUIDE_HOMOGRAPHY)
        hipLaunchKernelGGL(k_ransac_hyp, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, st, d_pts, n, opts->seed, N, d_models, d_counts);
    else
        hipLaunchKernelGGL(k_ransac_hyp_fund, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, st, d_pts, n, opts->seed, N, d_models, d_counts);
    queue_score<KIND>(st, d_pts, n, d_models, N, tol, d_counts);
    hipLaunchKernelGGL(k_ransac_select, dim3(1), dim3(256), 0, st, d_counts, N, d_models, d_state);
    // with the refit: the winner's correspondences to the host; without: the inlier records, and the call is complete
    if (refit) queue_compact<KIND>(st, d_pts, n, d_state, tol, d_tot, d_pts, pin_rec, n);
    else queue_compact<KIND>(st, d_pts, n, d_state, tol, d_tot, d_pairs, final_out, final_cap);
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(hpin + R_PIN_STATE, d_state, sizeof(RState), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return PSX_ERR_HIP;
    if (hs->bad != 0) return PSX_ERR_INVALID;
    if (hs->best < 0 || hs->best >= N || hs->total < 0 || hs->total > n) return PSX_ERR_HIP;
    if (refit) {
        const int k = hs->sample_inliers;
        if (k >= MIN && hs->total == k) {
            int* up = reinterpret_cast<int*>(hpin + R_PIN_REFIT);           // refit_count, pad, refit[9]
            up[0] = 0; up[1] = 0;
            RModel<KIND>::fit(reinterpret_cast<const psx_ransac_pt*>(hpin + R_PIN_REC), k, reinterpret_cast<float*>(up + 2));
            if (RModel<KIND>::usable(reinterpret_cast<const float*>(up + 2))) {
                if (hipMemcpyAsync(&d_state->refit_count, up, sizeof(int) * 11, hipMemcpyHostToDevice, st) != hipSuccess) return PSX_ERR_HIP;
                queue_score<KIND>(st, d_pts, n, d_state->refit, 1, tol, &d_state->refit_count);
                hipLaunchKernelGGL(k_ransac_decide<KIND>, dim3(1), dim3(64), 0, st, d_state);
            }
        }
        queue_compact<KIND>(st, d_pts, n, d_state, tol, d_tot, d_pairs, final_out, final_cap);
        if (hipGetLastError() != hipSuccess || hipMemcpyAsync(hpin + R_PIN_STATE, d_state, sizeof(RState), hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess)
            return PSX_ERR_HIP;
        if (hs->total < 0 || hs->total > n) return PSX_ERR_HIP;
    }
    if (host_models && (hipMemcpyAsync(host_models, d_models, sizeof(float) * 9 * (size_t)N, hipMemcpyDeviceToHost, st) != hipSuccess)) return PSX_ERR_HIP;
    if (host_counts && (hipMemcpyAsync(host_counts, d_counts, sizeof(int) * (size_t)N, hipMemcpyDeviceToHost, st) != hipSuccess)) return PSX_ERR_HIP;
    if ((host_models || host_counts) && hipStreamSynchronize(st) != hipSuccess) return PSX_ERR_HIP;
    if (!RModel<KIND>::usable(hs->kept)) { psx_ransac_no_model(result); *count = 0; return PSX_OK; }
    const int total = hs->total;
    if (host_inl && total > 0 && nrec > 0) memcpy(host_inl, hpin + R_PIN_REC, 16 * (size_t)(total < nrec ? total : nrec));
    for (int k = 0; k < 9; k++) result->m[k] = hs->kept[k];
    result->best = hs->best; result->sample_inliers = hs->sample_inliers; result->inliers = total; result->refit_kept = hs->refit_kept;
    *count = total;
    return PSX_OK;
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
    if (n < 4 || !left_xy || !right_xy || !m) return PSX_ERR_INVALID;
    psx_ransac_pt* pt = new (std::nothrow) psx_ransac_pt[(size_t)n];
    if (!pt) return PSX_ERR_NOMEM;
    for (int i = 0; i < n; i++) {
        pt[i].xl = left_xy[2 * (size_t)i]; pt[i].yl = left_xy[2 * (size_t)i + 1];
        pt[i].xr = right_xy[2 * (size_t)i]; pt[i].yr = right_xy[2 * (size_t)i + 1];
    }
    psx_homography_fit_rule<0>(pt, n, m);
    delete[] pt;
    return PSX_OK;
}

extern "C" int psx_ransac_homography_ref(const void* pairs, int n, const float* left_xy, int nl, const float* right_xy, int nr,
                                         const psx_ransac_opts* opts, psx_ransac_result* result, void* inliers, int capacity, int* count,
                                         float* models, int* counts)
{
    psx_ransac_pt* scratch = n >= 4 ? new (std::nothrow) psx_ransac_pt[(size_t)n] : nullptr;
    if (n >= 4 && !scratch) return PSX_ERR_NOMEM;
    const int rc = psx_ransac_homography_host(pairs, n, left_xy, nl, right_xy, nr, opts, result, inliers, capacity, count, models, counts, scratch);
    delete[] scratch;
    return rc;
}

extern "C" int psx_ransac_homography(int device, const void* host_pairs, int n, const float* d_left_xy, int l_len,
                                     const float* d_right_xy, int r_len, const psx_ransac_opts* opts, psx_ransac_result* result,
                                     void* host_inliers, int capacity, int* count, float* host_models, int* host_counts)
{
    return ransac_run<PSX_GUIDE_HOMOGRAPHY>(device, host_pairs, nullptr, n, d_left_xy, l_len, d_right_xy, r_len, opts, result, host_inliers, nullptr, capacity, count,
                      host_models, host_counts);
}

extern "C" int psx_ransac_homography_dev(int device, const void* d_pairs, int n, const float* d_left_xy, int l_len,
                                         const float* d_right_xy, int r_len, const psx_ransac_opts* opts, psx_ransac_result* result,
                                         void* d_inliers, int capacity, int* count, float* host_models, int* host_counts)
{
    return ransac_run<PSX_GUIDE_HOMOGRAPHY>(device, nullptr, d_pairs, n, d_left_xy, l_len, d_right_xy, r_len, opts, result, nullptr, d_inliers, capacity, count,
                      host_models, host_counts);
}

extern "C" int psx_ransac_samples_k(unsigned seed, int first, int count, int n, int k, int* idx)
{
    if ((k != 4 && k != PSX_FUND_MIN) || n < k || first < 0 || count < 0 || first > PSX_RANSAC_MAX_HYPOTHESES - count || (count > 0 && !idx))
        return PSX_ERR_INVALID;
    for (int i = 0; i < count; i++) {
        if (k == 4) psx_ransac_sample_k<4>(seed, first + i, n, idx + 4 * (size_t)i);
        else psx_ransac_sample_k<PSX_FUND_MIN>(seed, first + i, n, idx + PSX_FUND_MIN * (size_t)i);
    }
    return PSX_OK;
}

extern "C" int psx_fundamental_fit(const float* left_xy, const float* right_xy, int n, float* m)
{
    if (n < PSX_FUND_MIN || !left_xy || !right_xy || !m) return PSX_ERR_INVALID;
    psx_ransac_pt* pt = new (std::nothrow) psx_ransac_pt[(size_t)n];
    if (!pt) return PSX_ERR_NOMEM;
    for (int i = 0; i < n; i++) {
        pt[i].xl = left_xy[2 * (size_t)i]; pt[i].yl = left_xy[2 * (size_t)i + 1];
        pt[i].xr = right_xy[2 * (size_t)i]; pt[i].yr = right_xy[2 * (size_t)i + 1];
    }
    psx_fundamental_fit_rule<0>(pt, n, m);
    delete[] pt;
    return PSX_OK;
}

extern "C" int psx_ransac_fundamental_ref(const void* pairs, int n, const float* left_xy, int nl, const float* right_xy, int nr,
                                          const psx_ransac_opts* opts, psx_ransac_result* result, void* inliers, int capacity, int* count,
                                          float* models, int* counts)
{
    psx_ransac_pt* scratch = n >= PSX_FUND_MIN ? new (std::nothrow) psx_ransac_pt[(size_t)n] : nullptr;
    if (n >= PSX_FUND_MIN && !scratch) return PSX_ERR_NOMEM;
    const int rc = psx_ransac_fundamental_host(pairs, n, left_xy, nl, right_xy, nr, opts, result, inliers, capacity, count, models, counts, scratch);
    delete[] scratch;
    return rc;
}

extern "C" int psx_ransac_fundamental(int device, const void* host_pairs, int n, const float* d_left_xy, int l_len,
                                      const float* d_right_xy, int r_len, const psx_ransac_opts* opts, psx_ransac_result* result,
                                      void* host_inliers, int capacity, int* count, float* host_models, int* host_counts)
{
    return ransac_run<PSX_GUIDE_EPIPOLAR>(device, host_pairs, nullptr, n, d_left_xy, l_len, d_right_xy, r_len, opts, result, host_inliers, nullptr,
                                          capacity, count, host_models, host_counts);
}

extern "C" int psx_ransac_fundamental_dev(int device, const void* d_pairs, int n, const float* d_left_xy, int l_len,
                                          const float* d_right_xy, int r_len, const psx_ransac_opts* opts, psx_ransac_result* result,
                                          void* d_inliers, int capacity, int* count, float* host_models, int* host_counts)
{
    return ransac_run<PSX_GUIDE_EPIPOLAR>(device, nullptr, d_pairs, n, d_left_xy, l_len, d_right_xy, r_len, opts, result, nullptr, d_inliers,
                                          capacity, count, host_models, host_counts);
}
