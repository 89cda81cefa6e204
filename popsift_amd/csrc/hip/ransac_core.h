// ransac_core.h -- the steps of the RANSAC estimator, each stated once for ransac.hip (one pair list) and ransac_graph.hip
// (many lists in one call): the traits of a model kind (RModel), the state a call keeps on the device (RHead, RState,
// RRefit), the device pieces -- gather of one pair (r_gather), sample and fixed-size fit (r_sample_fit), the score walk
// (r_score_walk), the workgroup arg-max (r_select), the keep test (r_keep), the refit decision (r_decide) -- and the host
// steps that both call sequences take (r_pinned_dev, r_stage_end, r_refit_model, r_download_layers, r_result).  The
// kernels only say where their operands live; the sequences and the argument checks stay in the two files.  The rule
// itself is ransac_rule.h, fundamental_rule.h and affine_rule.h.  Internal to the HIP library.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>

#include "affine_rule.h"
#include "match_scratch.h"

// What differs between the estimators, by the id of the model (PSX_RANSAC_MODEL_HOMOGRAPHY: ransac_rule.h; _FUNDAMENTAL:
// fundamental_rule.h; _AFFINE and _SIMILARITY: affine_rule.h; the first two ids are their guide kinds): the kind of guide
// the model is, the sample size, which models may score, the serial fit of the refit and the fixed-size fit of a sample.
template <int KIND> struct RModel;      // KIND: the model id
template <> struct RModel<PSX_RANSAC_MODEL_HOMOGRAPHY> {
    static constexpr int GUIDE = PSX_GUIDE_HOMOGRAPHY;
    static constexpr int MIN = 4;
    static __host__ __device__ __forceinline__ bool usable(const float* m) { return psx_ransac_model_finite(m); }
    static void fit(const psx_ransac_pt* pt, int n, float* m) { psx_homography_fit_rule<0>(pt, n, m); }
    static __device__ __forceinline__ void sample(unsigned seed, int h, int n, int* idx) { psx_ransac_sample(seed, h, n, idx); }
    static __device__ __forceinline__ void fit_sample(const psx_ransac_pt* q, float* m) { psx_homography_fit_rule<4>(q, 4, m); }
};
template <> struct RModel<PSX_RANSAC_MODEL_FUNDAMENTAL> {
    static constexpr int GUIDE = PSX_GUIDE_EPIPOLAR;
    static constexpr int MIN = PSX_FUND_MIN;
    static __host__ __device__ __forceinline__ bool usable(const float* m) { return psx_fund_model_usable(m); }
    static void fit(const psx_ransac_pt* pt, int n, float* m) { psx_fundamental_fit_rule<0>(pt, n, m); }
    static __device__ __forceinline__ void sample(unsigned seed, int h, int n, int* idx) { psx_ransac_sample_k<PSX_FUND_MIN>(seed, h, n, idx); }
    static __device__ __forceinline__ void fit_sample(const psx_ransac_pt* q, float* m) { psx_fundamental_fit_rule<PSX_FUND_MIN>(q, PSX_FUND_MIN, m); }
};
template <> struct RModel<PSX_RANSAC_MODEL_AFFINE> {
    static constexpr int GUIDE = PSX_GUIDE_HOMOGRAPHY;
    static constexpr int MIN = PSX_AFFINE_MIN;
    static __host__ __device__ __forceinline__ bool usable(const float* m) { return psx_ransac_model_finite(m); }
    static void fit(const psx_ransac_pt* pt, int n, float* m) { psx_affine_fit_rule<0>(pt, n, m); }
    static __device__ __forceinline__ void sample(unsigned seed, int h, int n, int* idx) { psx_ransac_sample_k<PSX_AFFINE_MIN>(seed, h, n, idx); }
    static __device__ __forceinline__ void fit_sample(const psx_ransac_pt* q, float* m) { psx_affine_fit_rule<PSX_AFFINE_MIN>(q, PSX_AFFINE_MIN, m); }
};
template <> struct RModel<PSX_RANSAC_MODEL_SIMILARITY> {
    static constexpr int GUIDE = PSX_GUIDE_HOMOGRAPHY;
    static constexpr int MIN = PSX_SIMILARITY_MIN;
    static __host__ __device__ __forceinline__ bool usable(const float* m) { return psx_ransac_model_finite(m); }
    static void fit(const psx_ransac_pt* pt, int n, float* m) { psx_similarity_fit_rule<0>(pt, n, m); }
    static __device__ __forceinline__ void sample(unsigned seed, int h, int n, int* idx) { psx_ransac_sample_k<PSX_SIMILARITY_MIN>(seed, h, n, idx); }
    static __device__ __forceinline__ void fit_sample(const psx_ransac_pt* q, float* m) { psx_similarity_fit_rule<PSX_SIMILARITY_MIN>(q, PSX_SIMILARITY_MIN, m); }
};

// The state of a call on the device: RHead, K x RState (the single call: K = 1), then from a 16-byte boundary K x RRefit.
// Head and states are zeroed by one memset and copied to the host at the end of a stage.
struct RHead { int bad, total, pad[2]; };    // the one flag; the batched call's sum of the totals
struct RState {                              // per set
    float kept[9];
    int best, sample_inliers, refit_kept, total, pad[3];
};
struct RRefit {                              // per set; uploaded in one copy before the refit's score launch
    int tried, count;
    float m[9];
    int pad;
};
static_assert(sizeof(RHead) == 16 && sizeof(RState) == 64 && sizeof(RRefit) == 48, "state layout");
constexpr int R_REFIT_WORDS = sizeof(RRefit) / 4;

__device__ __forceinline__ psx_ransac_pt r_pt(const float4& v) { psx_ransac_pt p = {v.x, v.y, v.z, v.w}; return p; }

// the arg-max order: count descending, index ascending
__device__ __forceinline__ void r_better(int& bc, int& bh, int c, int h)
{
    if (c > bc || (c == bc && h < bh)) { bc = c; bh = h; }
}

// the four floats of one pair into *dst; an index outside its position array raises the flag, reads nothing and leaves NaNs
__device__ __forceinline__ void r_gather(const int4 rec, const float2* __restrict__ lxy, int l_len, const float2* __restrict__ rxy,
                                         int r_len, float4* __restrict__ dst, int* __restrict__ bad)
{
    if (rec.x < 0 || rec.x >= l_len || rec.y < 0 || rec.y >= r_len) {
        atomicOr(bad, 1);
        *dst = make_float4(NAN, NAN, NAN, NAN);
        return;
    }
    const float2 a = lxy[rec.x], b = rxy[rec.y];
    *dst = make_float4(a.x, a.y, b.x, b.y);
}

// hypothesis h of a list of n correspondences: the sample's indices, their float4s and the fixed-size fit in double, all
// loops of constant trip count (registers)
template <int KIND>
__device__ __forceinline__ void r_sample_fit(const float4* __restrict__ pts, int n, unsigned seed, int h, float m[9])
{
    constexpr int S = RModel<KIND>::MIN;
    int idx[S];
    RModel<KIND>::sample(seed, h, n, idx);
    psx_ransac_pt q[S];
#pragma unroll
    for (int k = 0; k < S; k++) q[k] = r_pt(pts[idx[k]]);
    RModel<KIND>::fit_sample(q, m);
}

// The score walk of one wave: its lanes hold PPL resident pairs each (q, with in[] false past the list's end).  Per
// hypothesis of [h0, h1): nine floats at a workgroup-uniform address (scalar loads), a model that may not score is
// skipped, one wave64 ballot + popcount per resident pair and ONE integer atomic per wave -- integer atomics are
// order-free, the counts are deterministic.  Model h lies at models + (row + h) mstride, its count at
// counts + (row + h) cstride; the strides are literals in the kernels' calls where they are 9 and 1.
template <int KIND, int PPL>
__device__ __forceinline__ void r_score_walk(const psx_ransac_pt (&q)[PPL], const bool (&in)[PPL], const float* __restrict__ models,
                                             int* __restrict__ counts, size_t row, int mstride, int cstride, int h0, int h1, float tol)
{
    constexpr int GUIDE = RModel<KIND>::GUIDE;
    const int lane = threadIdx.x & 63;
    for (int h = h0; h < h1; h++) {
        float m[9];
#pragma unroll
        for (int k = 0; k < 9; k++) m[k] = models[(row + h) * mstride + k];
        if (!RModel<KIND>::usable(m)) continue;                           // workgroup uniform
        int c = 0;
#pragma unroll
        for (int k = 0; k < PPL; k++) {
            const psx_guide_line l = psx_guide_left(GUIDE, m, tol, q[k].xl, q[k].yl);
            c += __popcll(__ballot(in[k] && psx_guide_right(GUIDE, l, q[k].xr, q[k].yr)));
        }
        if (lane == 0 && c > 0) atomicAdd(counts + (row + h) * cstride, c);
    }
}

// A workgroup of 256 threads picks the winner of counts[0 .. N), N >= 1 (thread 0 saw hypothesis 0), and thread 0 writes
// its index, its count and its model into the state.
__device__ __forceinline__ void r_select(const int* __restrict__ counts, int N, const float* __restrict__ models, RState* __restrict__ st)
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
        st->best = bh; st->sample_inliers = bc;
        for (int k = 0; k < 9; k++) st->kept[k] = models[9 * (size_t)bh + k];
    }
}

// keep: pair i of pts passes under the state's kept model, read at a workgroup-uniform address (no pair does under a
// model that may not score, after a bad index, or outside its list -- pts[i] is then not read)
template <int KIND>
__device__ __forceinline__ bool r_keep(const RHead* __restrict__ head, const RState* __restrict__ st, bool inside,
                                       const float4* __restrict__ pts, int i, float tol)
{
    float m[9];
#pragma unroll
    for (int k = 0; k < 9; k++) m[k] = st->kept[k];
    if (head->bad != 0 || !RModel<KIND>::usable(m) || !inside) return false;
    constexpr int GUIDE = RModel<KIND>::GUIDE;
    const psx_ransac_pt p = r_pt(pts[i]);
    return psx_guide_right(GUIDE, psx_guide_left(GUIDE, m, tol, p.xl, p.yl), p.xr, p.yr);
}

// set `set` of the state and refit arrays: the refit model replaces the kept one iff it was tried, may score and has not
// fewer inliers than the sample's winner
template <int KIND>
__device__ __forceinline__ void r_decide(RState* __restrict__ st, const RRefit* __restrict__ rf, int set)
{
    if (rf[set].tried == 0) return;
    float m[9];
    for (int k = 0; k < 9; k++) m[k] = rf[set].m[k];
    if (RModel<KIND>::usable(m) && rf[set].count >= st[set].sample_inliers) {
        for (int k = 0; k < 9; k++) st[set].kept[k] = m[k];
        st[set].refit_kept = 1;
    }
}

// ---- the host steps both call sequences take ----

// the device address of the scratch's pinned staging buffer (NULL: the runtime does not give one)
inline void* r_pinned_dev(MatchScratch& sc)
{
    void* p = nullptr;
    return hipHostGetDevicePointer(&p, sc.hpin, 0) == hipSuccess ? p : nullptr;
}

// the end of a stage: the launches went through, the state comes to the pinned buffer, the stream is drained
inline bool r_stage_end(hipStream_t st, void* pin_state, const void* d_state, size_t bytes)
{
    return hipGetLastError() == hipSuccess && hipMemcpyAsync(pin_state, d_state, bytes, hipMemcpyDeviceToHost, st) == hipSuccess &&
           hipStreamSynchronize(st) == hipSuccess;
}

// Is a set's refit due, and what is its model?  Due: its winner has enough inliers to fit and all c of them arrived in
// rec (total == c; a set without a winner has c = 0).  *up gets the model and tried = 1, or a NaN model, which no rule
// lets score, and tried = 0.
template <int KIND>
bool r_refit_model(const RState& s, const psx_ransac_pt* rec, RRefit* up)
{
    up->tried = 0; up->count = 0; up->pad = 0;
    for (int j = 0; j < 9; j++) up->m[j] = NAN;
    const int c = s.sample_inliers;
    if (c < RModel<KIND>::MIN || s.total != c) return false;
    float m[9];
    RModel<KIND>::fit(rec, c, m);
    if (!RModel<KIND>::usable(m)) return false;
    for (int j = 0; j < 9; j++) up->m[j] = m[j];
    up->tried = 1;
    return true;
}

// the optional download of the `layers` hypotheses' models and counts (either may be NULL)
inline bool r_download_layers(hipStream_t st, float* host_models, const float* d_models, int* host_counts, const int* d_counts, size_t layers)
{
    if (host_models && hipMemcpyAsync(host_models, d_models, sizeof(float) * 9 * layers, hipMemcpyDeviceToHost, st) != hipSuccess) return false;
    if (host_counts && hipMemcpyAsync(host_counts, d_counts, sizeof(int) * layers, hipMemcpyDeviceToHost, st) != hipSuccess) return false;
    return !(host_models || host_counts) || hipStreamSynchronize(st) == hipSuccess;
}

// a set's result from its downloaded state; false, and "no model", when the kept model may not score
template <int KIND>
bool r_result(const RState& s, psx_ransac_result* r)
{
    if (!RModel<KIND>::usable(s.kept)) { psx_ransac_no_model(r); return false; }
    for (int j = 0; j < 9; j++) r->m[j] = s.kept[j];
    r->best = s.best; r->sample_inliers = s.sample_inliers; r->inliers = s.total; r->refit_kept = s.refit_kept;
    return true;
}
