// ransac_many.hip -- geometric verification of many pair lists in one call: psx_ransac_homography_many (+ _dev, _ref),
// psx_ransac_fundamental_many, psx_ransac_affine_many, psx_ransac_similarity_many (+ _dev, _ref each),
// psx_ransac_many_plan (include/popsift_hip.h).
//
// psx_ransac_*_dev (ransac.hip) is a fixed sequence of launches and one or two synchronisations per pair list.  A list
// has a few hundred to a few thousand pairs: at that size the kernels are nearly empty and the call is launch latency and
// round trips, paid again for every list.  Here the K lists that psx_match_pairs_many_u8* left behind one another are
// verified by the SAME sequence, every kernel one grid over all sets, driven by tables in which no block crosses a set
// boundary (ransac_many_plan.h).  The rule -- samples, fit, score, select, refit, inliers -- is ransac_rule.h,
// fundamental_rule.h and affine_rule.h, and every step of the estimator around it is the ONE statement of ransac_core.h that the single call
// runs too: set k's result is the single call's, bit for bit.  The kernels here say where a step's operands live:
//   k_rmany_gather  r_gather per pair of every set that has a model to estimate, into ONE packed float4 array indexed as
//                   the concatenation; set k's right positions through the set table
//   k_rmany_hyp     one lane per (set, hypothesis): r_sample_fit on the set's own n_k; a set below the minimum gets zeros
//   k_rmany_score   the hot kernel: r_score_walk over a block of M_HB hypotheses.  The block-table entry and with it the
//                   model address models[(set N + h) mstride] are workgroup uniform (scalar loads), the counts go to
//                   counts[(set N + h) cstride].  A wave owns M_PPL x 64 CONSECUTIVE pairs of its block, and a wave without
//                   a resident pair leaves before the walk: a short set's last block is mostly such waves
//   k_rmany_select  r_select, one workgroup per set
//   k_rmany_count / k_rmany_scan / k_rmany_write   r_keep into the stable compaction of wg_compact.h, segmented as the
//                   one-to-many join (match_many.hip) runs it: one total per 256-pair workgroup in set-major order, an
//                   exclusive scan of the totals by one workgroup, one 16-byte store per survivor; a set's total is the
//                   difference of the scan at its boundaries.  No atomics.  The payload is any 16-byte record array
//   k_rmany_decide  r_decide, one lane per set
// The refit's fit is serial by definition: every set's winner correspondences come to the host through the pinned
// staging buffer in ONE compaction, the host fits the sets whose refit is due, ONE upload carries all refit models with a
// per-set "tried" word, and the score kernel runs once more with one model per set.
// Launches per call, whatever K is: the table copy and a memset, then gather, hyp, score, select and the compaction's 3 --
// 7 kernels and 1 synchronisation without the refit; with it 5 more (score, decide, the compaction's 3) -- 12 kernels and
// 2 synchronisations.
#include "psx_internal.h"
#include "ransac_core.h"
#include "ransac_many_plan.h"
#include "wg_compact.h"

#include <cstring>
#include <new>

namespace {

constexpr int M_PPL = PSX_RANSAC_MANY_SCORE_ROWS / 256;    // pairs resident per lane of the score kernel
constexpr int M_HB = 64;                                    // hypotheses per workgroup of the score kernel
static_assert(M_PPL * 256 == PSX_RANSAC_MANY_SCORE_ROWS && PSX_RANSAC_MANY_ROWS == 256, "block sizes");

struct RMSet {                               // one entry per set
    const float2* rxy;                       // its right positions
    int r_len;
    int n;                                   // its pairs
    int off;                                 // its first pair in the concatenation
    int b0, b1;                              // its blocks in the 256-pair table (b0 == b1: below the minimum)
    int pad;
};
static_assert(sizeof(RMSet) == 32, "two 16-byte scalar loads per entry");

// grid: the 256-pair blocks
__global__ __launch_bounds__(256) void k_rmany_gather(const int4* __restrict__ pairs, const RMSet* __restrict__ sets,
                                                      const int4* __restrict__ blocks, const float2* __restrict__ lxy, int l_len,
                                                      float4* __restrict__ pts, int* __restrict__ bad)
{
    const int4 blk = blocks[blockIdx.x];
    const RMSet s = sets[blk.x];
    const int p = blk.y + (int)threadIdx.x;
    if (p >= blk.z) return;
    r_gather(pairs[p], lxy, l_len, s.rxy, s.r_len, pts + p, bad);
}

// grid K * hw (hw = ceil(N / 64)) waves, workgroup k * hw + w: one lane per (set, hypothesis)
template <int KIND>
__global__ __launch_bounds__(64) void k_rmany_hyp(const float4* __restrict__ pts, const RMSet* __restrict__ sets, int hw, unsigned seed, int N,
                                                  float* __restrict__ models, int* __restrict__ counts)
{
    const int k = (int)(blockIdx.x / (unsigned)hw);
    const int h = (int)(blockIdx.x % (unsigned)hw) * 64 + (int)threadIdx.x;
    if (h >= N) return;
    const RMSet s = sets[k];
    float m[9];
    if (s.n >= RModel<KIND>::MIN) r_sample_fit<KIND>(pts + s.off, s.n, seed, h, m);       // workgroup uniform
    else {
#pragma unroll
        for (int j = 0; j < 9; j++) m[j] = 0.0f;
    }
    const size_t at = (size_t)k * (size_t)N + (size_t)h;
#pragma unroll
    for (int j = 0; j < 9; j++) models[9 * at + j] = m[j];
    counts[at] = 0;
}

// grid nsb * ceil(N / M_HB), workgroup hb * nsb + b: block b of the score table x hypotheses [hb M_HB, + M_HB) of ITS set.
// Model (set, h) lies at models + (set N + h) mstride, its count at counts + (set N + h) cstride: 9 and 1 for the
// hypotheses, the RRefit array (N = 1) for the refit.  A wave owns M_PPL x 64 consecutive pairs of its block.
template <int KIND>
__global__ __launch_bounds__(256) void k_rmany_score(const float4* __restrict__ pts, const int4* __restrict__ blocks, int nsb,
                                                     const float* __restrict__ models, int N, int mstride, float tol,
                                                     int* __restrict__ counts, int cstride)
{
    const int4 blk = blocks[blockIdx.x % (unsigned)nsb];
    const int lane = threadIdx.x & 63;
    const int wave0 = blk.y + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) * (64 * M_PPL);
    if (wave0 >= blk.z) return;                                            // no resident pair in this wave
    psx_ransac_pt q[M_PPL];
    bool in[M_PPL];
#pragma unroll
    for (int k = 0; k < M_PPL; k++) {
        const int p = wave0 + k * 64 + lane;
        in[k] = p < blk.z;
        q[k] = r_pt(in[k] ? pts[p] : make_float4(0.f, 0.f, 0.f, 0.f));
    }
    const int h0 = (int)(blockIdx.x / (unsigned)nsb) * M_HB;
    r_score_walk<KIND, M_PPL>(q, in, models, counts, (size_t)blk.x * (size_t)N, mstride, cstride, h0, h0 + M_HB < N ? h0 + M_HB : N, tol);
}

// one workgroup of 256 threads per set
__global__ __launch_bounds__(256) void k_rmany_select(const RMSet* __restrict__ sets, const int* __restrict__ counts, int N,
                                                      const float* __restrict__ models, RState* __restrict__ st)
{
    const int set = blockIdx.x;
    if (sets[set].b0 == sets[set].b1) return;                              // below the minimum: its state stays zero
    const size_t row = (size_t)set * (size_t)N;
    r_select(counts + row, N, models + 9 * row, st + set);
}

// one lane per set
template <int KIND>
__global__ __launch_bounds__(256) void k_rmany_decide(RState* __restrict__ st, const RRefit* __restrict__ rf, int n_sets)
{
    const int set = blockIdx.x * 256 + threadIdx.x;
    if (set < n_sets) r_decide<KIND>(st, rf, set);
}

// grid: the 256-pair blocks, set-major as the table is
template <int KIND>
__global__ __launch_bounds__(256) void k_rmany_count(const float4* __restrict__ pts, const int4* __restrict__ blocks,
                                                     const RHead* __restrict__ head, const RState* __restrict__ st, float tol,
                                                     int* __restrict__ wg_tot)
{
    const int4 blk = blocks[blockIdx.x];
    const int i = blk.y + (int)threadIdx.x;
    __shared__ int s_cnt[4];
    wg_count(__ballot(r_keep<KIND>(head, st + blk.x, i < blk.z, pts, i, tol)), s_cnt);
    if (threadIdx.x == 0) wg_tot[blockIdx.x] = wg_total(s_cnt);
}

// ONE workgroup of 1024 threads (wg_compact.h)
__global__ __launch_bounds__(1024) void k_rmany_scan(const int* __restrict__ wg_tot, int n, int* __restrict__ offs)
{
    wg_scan_totals(wg_tot, n, offs);
}

// grid as k_rmany_count.  src: the concatenation's 16-byte records (the correspondences themselves, or the pair records);
// out: never written at or past `capacity`.  A set's first workgroup writes the set's total, workgroup 0 the sum.
template <int KIND>
__global__ __launch_bounds__(256) void k_rmany_write(const float4* __restrict__ pts, const RMSet* __restrict__ sets,
                                                     const int4* __restrict__ blocks, RHead* __restrict__ head, RState* __restrict__ st,
                                                     float tol, const int* __restrict__ offs, const int4* __restrict__ src,
                                                     int4* __restrict__ out, int capacity)
{
    const int4 blk = blocks[blockIdx.x];
    const int i = blk.y + (int)threadIdx.x;
    const bool keep = r_keep<KIND>(head, st + blk.x, i < blk.z, pts, i, tol);
    const unsigned long long m = __ballot(keep);
    __shared__ int s_cnt[4];
    wg_count(m, s_cnt);
    const int pos = offs[blockIdx.x] + wg_offset(m, s_cnt);
    if (keep && pos < capacity) out[pos] = src[i];
    if (threadIdx.x == 0) {
        const RMSet s = sets[blk.x];
        if ((int)blockIdx.x == s.b0) st[blk.x].total = offs[s.b1] - offs[s.b0];
        if (blockIdx.x == 0) head->total = offs[gridDim.x];
    }
}

size_t pad16(size_t b) { return (b + 15) & ~(size_t)15; }

// what a call holds while it queues: the device arrays and the launch shapes
struct RMQueue {
    hipStream_t st;
    const RMSet* d_sets;
    const int4 *d_sblk, *d_cblk;
    int nsb, ncb, K;
    float4* d_pts;
    RHead* d_head;
    RState* d_state;
    int *d_tot, *d_offs;
    float tol;
};

template <int KIND>
void queue_score(const RMQueue& q, const float* d_models, int N, int mstride, int* d_counts, int cstride)
{
    const unsigned hb = (unsigned)((N + M_HB - 1) / M_HB);
    hipLaunchKernelGGL(k_rmany_score<KIND>, dim3((unsigned)q.nsb * hb), dim3(256), 0, q.st, q.d_pts, q.d_sblk, q.nsb, d_models, N, mstride, q.tol,
                       d_counts, cstride);
}

template <int KIND>
void queue_compact(const RMQueue& q, const void* src, void* out, int cap)
{
    hipLaunchKernelGGL(k_rmany_count<KIND>, dim3((unsigned)q.ncb), dim3(256), 0, q.st, q.d_pts, q.d_cblk, q.d_head, q.d_state, q.tol, q.d_tot);
    hipLaunchKernelGGL(k_rmany_scan, dim3(1), dim3(1024), 0, q.st, q.d_tot, q.ncb, q.d_offs);
    hipLaunchKernelGGL(k_rmany_write<KIND>, dim3((unsigned)q.ncb), dim3(256), 0, q.st, q.d_pts, q.d_sets, q.d_cblk, q.d_head, q.d_state, q.tol,
                       q.d_offs, static_cast<const int4*>(src), static_cast<int4*>(out), cap);
}

// host_pairs or d_pairs_in; host_inl or d_inl (the other is NULL; both NULL with capacity 0)
template <int KIND>
int ransac_many_run(int device, const void* host_pairs, const void* d_pairs_in, const int* set_counts, int n_sets, const float* d_lxy, int l_len,
                    const float* const* d_rxys, const int* r_lens, const psx_ransac_opts* opts, psx_ransac_result* results, void* host_inl,
                    void* d_inl, int capacity, int* count, float* host_models, int* host_counts)
{
    long long total_pairs = 0;
    if (!psx_ransac_many_args_ok(host_pairs ? host_pairs : d_pairs_in, set_counts, n_sets, d_lxy, l_len, d_rxys, r_lens, opts, results,
                                 host_inl ? host_inl : d_inl, capacity, count, &total_pairs))
        return PSX_ERR_INVALID;
    constexpr int MIN = RModel<KIND>::MIN;
    const int K = n_sets, N = opts->hypotheses, n = (int)total_pairs;
    const long long nsb = psx_ransac_many_blocks(set_counts, K, MIN, PSX_RANSAC_MANY_SCORE_ROWS, nullptr, 0);
    const long long ncb = psx_ransac_many_blocks(set_counts, K, MIN, PSX_RANSAC_MANY_ROWS, nullptr, 0);
    if (ncb == 0) { psx_ransac_many_none(K, N, results, count, host_models, host_counts); return PSX_OK; }
    for (int k = 0; k < K; k++)
        if (set_counts[k] >= MIN && (l_len == 0 || r_lens[k] == 0)) return PSX_ERR_INVALID;     // no index can lie inside an empty array
    const long long score_wgs = nsb * ((N + M_HB - 1) / M_HB), hyp_wgs = (long long)K * ((N + 63) / 64);
    if (score_wgs > 0x7fffffffLL || hyp_wgs > 0x7fffffffLL) return PSX_ERR_NOMEM;
    if (hipSetDevice(device) != hipSuccess) return PSX_ERR_HIP;
    MatchScratch& sc = psx_match_scratch();
    if (!sc.bind(device)) return PSX_ERR_HIP;
    const float tol = opts->tol;
    const bool refit = (opts->flags & PSX_RANSAC_REFIT) != 0;
    const int nrec = host_inl ? (capacity < n ? capacity : n) : 0;
    // the device blob: set table, score blocks, compaction blocks; the pinned buffer: states, refit models, blob, records
    const size_t sets_b = pad16(sizeof(RMSet) * (size_t)K), sblk_b = sizeof(int4) * (size_t)nsb, cblk_b = sizeof(int4) * (size_t)ncb;
    const size_t blob_b = sets_b + sblk_b + cblk_b;
    const size_t state_b = sizeof(RHead) + sizeof(RState) * (size_t)K, refit_b = sizeof(RRefit) * (size_t)K;
    const size_t pin_state = 0, pin_refit = pad16(state_b), pin_blob = pin_refit + refit_b, pin_rec = pin_blob + blob_b;
    // every buffer before the first launch: nothing is reallocated under queued work
    if ((host_pairs && !sc.need(MS_RANSAC_PAIRS, 16 * (size_t)n)) || !sc.need(MS_RMANY_TABLES, blob_b) || !sc.need(MS_RANSAC_PTS, 16 * (size_t)n) ||
        !sc.need(MS_RANSAC_MODELS, sizeof(float) * 9 * (size_t)K * (size_t)N) || !sc.need(MS_RANSAC_COUNTS, sizeof(int) * (size_t)K * (size_t)N) ||
        !sc.need(MS_RANSAC_STATE, pin_refit + refit_b) || !sc.need(MS_RANSAC_TOT, sizeof(int) * (2 * (size_t)ncb + 1)) ||
        !sc.need_pinned(pin_rec + 16 * (size_t)(refit ? n : nrec)))
        return PSX_ERR_NOMEM;
    void* dev_pin = r_pinned_dev(sc);
    if (dev_pin == nullptr) return PSX_ERR_HIP;
    char* hpin = static_cast<char*>(sc.hpin);
    void* d_pin_rec = static_cast<char*>(dev_pin) + pin_rec;

    // ---- the tables, written into the pinned staging buffer and copied on the stream in ONE copy ----
    {
        RMSet* hs = reinterpret_cast<RMSet*>(hpin + pin_blob);
        psx_ransac_block* tmp = new (std::nothrow) psx_ransac_block[(size_t)ncb];          // nsb <= ncb
        if (!tmp) return PSX_ERR_NOMEM;
        int4* hb = reinterpret_cast<int4*>(hpin + pin_blob + sets_b);
        psx_ransac_many_blocks(set_counts, K, MIN, PSX_RANSAC_MANY_SCORE_ROWS, tmp, nsb);
        for (long long b = 0; b < nsb; b++) hb[b] = make_int4(tmp[b].set, tmp[b].first, tmp[b].end, 0);
        hb += nsb;
        psx_ransac_many_blocks(set_counts, K, MIN, PSX_RANSAC_MANY_ROWS, tmp, ncb);
        long long off = 0;
        for (int k = 0; k < K; k++) {
            hs[k] = RMSet{reinterpret_cast<const float2*>(d_rxys[k]), r_lens[k], set_counts[k], (int)off, 0, 0, 0};
            off += set_counts[k];
        }
        for (long long b = 0; b < ncb; b++) {
            hb[b] = make_int4(tmp[b].set, tmp[b].first, tmp[b].end, 0);
            RMSet& s = hs[tmp[b].set];
            if (s.b1 == 0) s.b0 = (int)b;                                  // a set's blocks are contiguous: first and last + 1
            s.b1 = (int)b + 1;
        }
        delete[] tmp;
    }
    hipStream_t st = sc.stream;
    const void* d_pairs = d_pairs_in;
    if (host_pairs) {
        if (hipMemcpyAsync(sc.buf[MS_RANSAC_PAIRS], host_pairs, 16 * (size_t)n, hipMemcpyHostToDevice, st) != hipSuccess) return PSX_ERR_HIP;
        d_pairs = sc.buf[MS_RANSAC_PAIRS];
    }
    char* d_blob = static_cast<char*>(sc.buf[MS_RMANY_TABLES]);
    char* d_st = static_cast<char*>(sc.buf[MS_RANSAC_STATE]);
    RMQueue q;
    q.st = st; q.K = K; q.nsb = (int)nsb; q.ncb = (int)ncb; q.tol = tol;
    q.d_sets = reinterpret_cast<const RMSet*>(d_blob);
    q.d_sblk = reinterpret_cast<const int4*>(d_blob + sets_b);
    q.d_cblk = reinterpret_cast<const int4*>(d_blob + sets_b + sblk_b);
    q.d_pts = static_cast<float4*>(sc.buf[MS_RANSAC_PTS]);
    q.d_head = reinterpret_cast<RHead*>(d_st);
    q.d_state = reinterpret_cast<RState*>(d_st + sizeof(RHead));
    q.d_tot = static_cast<int*>(sc.buf[MS_RANSAC_TOT]);
    q.d_offs = q.d_tot + ncb;
    RRefit* d_refit = reinterpret_cast<RRefit*>(d_st + pin_refit);
    float* d_models = static_cast<float*>(sc.buf[MS_RANSAC_MODELS]);
    int* d_counts = static_cast<int*>(sc.buf[MS_RANSAC_COUNTS]);
    const RHead* hh = reinterpret_cast<const RHead*>(hpin + pin_state);
    const RState* hs = reinterpret_cast<const RState*>(hpin + pin_state + sizeof(RHead));
    void* final_out = host_inl ? d_pin_rec : d_inl;
    const int final_cap = host_inl ? nrec : capacity;
    const unsigned hw = (unsigned)((N + 63) / 64);

    if (hipMemcpyAsync(d_blob, hpin + pin_blob, blob_b, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemsetAsync(d_st, 0, state_b, st) != hipSuccess)
        return PSX_ERR_HIP;
    hipLaunchKernelGGL(k_rmany_gather, dim3((unsigned)ncb), dim3(256), 0, st, static_cast<const int4*>(d_pairs), q.d_sets, q.d_cblk,
                       reinterpret_cast<const float2*>(d_lxy), l_len, q.d_pts, &q.d_head->bad);
    hipLaunchKernelGGL(k_rmany_hyp<KIND>, dim3((unsigned)K * hw), dim3(64), 0, st, q.d_pts, q.d_sets, (int)hw, opts->seed, N, d_models, d_counts);
    queue_score<KIND>(q, d_models, N, 9, d_counts, 1);
    hipLaunchKernelGGL(k_rmany_select, dim3((unsigned)K), dim3(256), 0, st, q.d_sets, d_counts, N, d_models, q.d_state);
    // with the refit: every set's winner correspondences to the host; without: the inlier records, and the call is complete
    if (refit) queue_compact<KIND>(q, q.d_pts, d_pin_rec, n);
    else queue_compact<KIND>(q, d_pairs, final_out, final_cap);
    if (!r_stage_end(st, hpin + pin_state, d_st, state_b)) return PSX_ERR_HIP;
    if (hh->bad != 0) return PSX_ERR_INVALID;
    auto sane = [&]() {
        long long sum = 0;
        for (int k = 0; k < K; k++) {
            if (hs[k].total < 0 || hs[k].total > set_counts[k]) return false;
            if (set_counts[k] >= MIN && (hs[k].best < 0 || hs[k].best >= N)) return false;
            sum += hs[k].total;
        }
        return sum == hh->total;
    };
    if (!sane()) return PSX_ERR_HIP;
    if (refit) {
        // set k's winner correspondences lie behind those of the sets before it, in pair order; a set below the minimum
        // has a zero state, which is never due
        RRefit* up = reinterpret_cast<RRefit*>(hpin + pin_refit);
        const psx_ransac_pt* rec = reinterpret_cast<const psx_ransac_pt*>(hpin + pin_rec);
        bool any = false;
        size_t at = 0;
        for (int k = 0; k < K; at += (size_t)hs[k].total, k++) any |= r_refit_model<KIND>(hs[k], rec + at, up + k);
        if (any) {
            if (hipMemcpyAsync(d_refit, up, refit_b, hipMemcpyHostToDevice, st) != hipSuccess) return PSX_ERR_HIP;
            queue_score<KIND>(q, d_refit->m, 1, R_REFIT_WORDS, &d_refit->count, R_REFIT_WORDS);
            hipLaunchKernelGGL(k_rmany_decide<KIND>, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, st, q.d_state, d_refit, K);
        }
        queue_compact<KIND>(q, d_pairs, final_out, final_cap);
        if (!r_stage_end(st, hpin + pin_state, d_st, state_b) || !sane()) return PSX_ERR_HIP;
    }
    if (!r_download_layers(st, host_models, d_models, host_counts, d_counts, (size_t)K * (size_t)N)) return PSX_ERR_HIP;
    const int total = hh->total;
    if (host_inl && total > 0 && nrec > 0) memcpy(host_inl, hpin + pin_rec, 16 * (size_t)(total < nrec ? total : nrec));
    for (int k = 0; k < K; k++) {                                          // a set below the minimum has a zero state, which a
        if (set_counts[k] < MIN) psx_ransac_no_model(results + k);         // homography may take for a model
        else r_result<KIND>(hs[k], results + k);
    }
    *count = total;
    return PSX_OK;
}

int many_ref(int model, const void* pairs, const int* set_counts, int n_sets, const float* left_xy, int nl, const float* const* right_xys,
             const int* r_lens, const psx_ransac_opts* opts, psx_ransac_result* results, void* inliers, int capacity, int* count, float* models,
             int* counts)
{
    int longest = 0;
    if (n_sets > 0 && set_counts != nullptr)
        for (int k = 0; k < n_sets; k++) longest = set_counts[k] > longest ? set_counts[k] : longest;
    psx_ransac_pt* scratch = longest > 0 ? new (std::nothrow) psx_ransac_pt[(size_t)longest] : nullptr;
    if (longest > 0 && !scratch) return PSX_ERR_NOMEM;
    const int rc = psx_ransac_many_host(model, pairs, set_counts, n_sets, left_xy, nl, right_xys, r_lens, opts, results, inliers, capacity, count,
                                        models, counts, scratch);
    delete[] scratch;
    return rc;
}

} // namespace

extern "C" int psx_ransac_many_plan(const int* set_counts, int n_sets, int min_pairs, int block_rows, psx_ransac_block* blocks, int capacity,
                                    int* block_count)
{
    return psx_ransac_many_plan_host(set_counts, n_sets, min_pairs, block_rows, blocks, capacity, block_count);
}

extern "C" int psx_ransac_homography_many_ref(const void* pairs, const int* set_counts, int n_sets, const float* left_xy, int nl,
                                              const float* const* right_xys, const int* r_lens, const psx_ransac_opts* opts,
                                              psx_ransac_result* results, void* inliers, int capacity, int* count, float* models, int* counts)
{
    return many_ref(PSX_RANSAC_MODEL_HOMOGRAPHY, pairs, set_counts, n_sets, left_xy, nl, right_xys, r_lens, opts, results, inliers, capacity, count, models, counts);
}

extern "C" int psx_ransac_fundamental_many_ref(const void* pairs, const int* set_counts, int n_sets, const float* left_xy, int nl,
                                               const float* const* right_xys, const int* r_lens, const psx_ransac_opts* opts,
                                               psx_ransac_result* results, void* inliers, int capacity, int* count, float* models, int* counts)
{
    return many_ref(PSX_RANSAC_MODEL_FUNDAMENTAL, pairs, set_counts, n_sets, left_xy, nl, right_xys, r_lens, opts, results, inliers, capacity, count, models, counts);
}

extern "C" int psx_ransac_homography_many(int device, const void* host_pairs, const int* set_counts, int n_sets, const float* d_left_xy, int l_len,
                                          const float* const* d_right_xys, const int* r_lens, const psx_ransac_opts* opts,
                                          psx_ransac_result* results, void* host_inliers, int capacity, int* count, float* host_models,
                                          int* host_counts)
{
    return ransac_many_run<PSX_RANSAC_MODEL_HOMOGRAPHY>(device, host_pairs, nullptr, set_counts, n_sets, d_left_xy, l_len, d_right_xys, r_lens, opts, results,
                                                 host_inliers, nullptr, capacity, count, host_models, host_counts);
}

extern "C" int psx_ransac_homography_many_dev(int device, const void* d_pairs, const int* set_counts, int n_sets, const float* d_left_xy, int l_len,
                                              const float* const* d_right_xys, const int* r_lens, const psx_ransac_opts* opts,
                                              psx_ransac_result* results, void* d_inliers, int capacity, int* count, float* host_models,
                                              int* host_counts)
{
    return ransac_many_run<PSX_RANSAC_MODEL_HOMOGRAPHY>(device, nullptr, d_pairs, set_counts, n_sets, d_left_xy, l_len, d_right_xys, r_lens, opts, results,
                                                 nullptr, d_inliers, capacity, count, host_models, host_counts);
}

extern "C" int psx_ransac_fundamental_many(int device, const void* host_pairs, const int* set_counts, int n_sets, const float* d_left_xy, int l_len,
                                           const float* const* d_right_xys, const int* r_lens, const psx_ransac_opts* opts,
                                           psx_ransac_result* results, void* host_inliers, int capacity, int* count, float* host_models,
                                           int* host_counts)
{
    return ransac_many_run<PSX_RANSAC_MODEL_FUNDAMENTAL>(device, host_pairs, nullptr, set_counts, n_sets, d_left_xy, l_len, d_right_xys, r_lens, opts, results,
                                               host_inliers, nullptr, capacity, count, host_models, host_counts);
}

extern "C" int psx_ransac_fundamental_many_dev(int device, const void* d_pairs, const int* set_counts, int n_sets, const float* d_left_xy, int l_len,
                                               const float* const* d_right_xys, const int* r_lens, const psx_ransac_opts* opts,
                                               psx_ransac_result* results, void* d_inliers, int capacity, int* count, float* host_models,
                                               int* host_counts)
{
    return ransac_many_run<PSX_RANSAC_MODEL_FUNDAMENTAL>(device, nullptr, d_pairs, set_counts, n_sets, d_left_xy, l_len, d_right_xys, r_lens, opts, results,
                                               nullptr, d_inliers, capacity, count, host_models, host_counts);
}

extern "C" int psx_ransac_affine_many_ref(const void* pairs, const int* set_counts, int n_sets, const float* left_xy, int nl,
                                        const float* const* right_xys, const int* r_lens, const psx_ransac_opts* opts,
                                        psx_ransac_result* results, void* inliers, int capacity, int* count, float* models, int* counts)
{
    return many_ref(PSX_RANSAC_MODEL_AFFINE, pairs, set_counts, n_sets, left_xy, nl, right_xys, r_lens, opts, results, inliers, capacity, count, models, counts);
}

extern "C" int psx_ransac_affine_many(int device, const void* host_pairs, const int* set_counts, int n_sets, const float* d_left_xy, int l_len,
                                    const float* const* d_right_xys, const int* r_lens, const psx_ransac_opts* opts,
                                    psx_ransac_result* results, void* host_inliers, int capacity, int* count, float* host_models,
                                    int* host_counts)
{
    return ransac_many_run<PSX_RANSAC_MODEL_AFFINE>(device, host_pairs, nullptr, set_counts, n_sets, d_left_xy, l_len, d_right_xys, r_lens, opts, results,
                               host_inliers, nullptr, capacity, count, host_models, host_counts);
}

extern "C" int psx_ransac_affine_many_dev(int device, const void* d_pairs, const int* set_counts, int n_sets, const float* d_left_xy, int l_len,
                                        const float* const* d_right_xys, const int* r_lens, const psx_ransac_opts* opts,
                                        psx_ransac_result* results, void* d_inliers, int capacity, int* count, float* host_models,
                                        int* host_counts)
{
    return ransac_many_run<PSX_RANSAC_MODEL_AFFINE>(device, nullptr, d_pairs, set_counts, n_sets, d_left_xy, l_len, d_right_xys, r_lens, opts, results,
                               nullptr, d_inliers, capacity, count, host_models, host_counts);
}

extern "C" int psx_ransac_similarity_many_ref(const void* pairs, const int* set_counts, int n_sets, const float* left_xy, int nl,
                                        const float* const* right_xys, const int* r_lens, const psx_ransac_opts* opts,
                                        psx_ransac_result* results, void* inliers, int capacity, int* count, float* models, int* counts)
{
    return many_ref(PSX_RANSAC_MODEL_SIMILARITY, pairs, set_counts, n_sets, left_xy, nl, right_xys, r_lens, opts, results, inliers, capacity, count, models, counts);
}

extern "C" int psx_ransac_similarity_many(int device, const void* host_pairs, const int* set_counts, int n_sets, const float* d_left_xy, int l_len,
                                    const float* const* d_right_xys, const int* r_lens, const psx_ransac_opts* opts,
                                    psx_ransac_result* results, void* host_inliers, int capacity, int* count, float* host_models,
                                    int* host_counts)
{
    return ransac_many_run<PSX_RANSAC_MODEL_SIMILARITY>(device, host_pairs, nullptr, set_counts, n_sets, d_left_xy, l_len, d_right_xys, r_lens, opts, results,
                               host_inliers, nullptr, capacity, count, host_models, host_counts);
}

extern "C" int psx_ransac_similarity_many_dev(int device, const void* d_pairs, const int* set_counts, int n_sets, const float* d_left_xy, int l_len,
                                        const float* const* d_right_xys, const int* r_lens, const psx_ransac_opts* opts,
                                        psx_ransac_result* results, void* d_inliers, int capacity, int* count, float* host_models,
                                        int* host_counts)
{
    return ransac_many_run<PSX_RANSAC_MODEL_SIMILARITY>(device, nullptr, d_pairs, set_counts, n_sets, d_left_xy, l_len, d_right_xys, r_lens, opts, results,
                               nullptr, d_inliers, capacity, count, host_models, host_counts);
}
