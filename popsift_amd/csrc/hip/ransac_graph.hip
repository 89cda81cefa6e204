// ransac_graph.hip -- geometric verification of a list of view pairs in one call: psx_ransac_homography_graph (+ _dev,
// _ref), psx_ransac_fundamental_graph, psx_ransac_affine_graph, psx_ransac_similarity_graph (+ _dev, _ref each)
// (include/popsift_hip.h).
//
// This is the ONE batched RANSAC of the library.  psx_ransac_*_dev (ransac.hip) is a fixed sequence of launches and one
// or two synchronisations per pair list; a list has a few hundred to a few thousand pairs, so the kernels are nearly empty
// and the call is launch latency and round trips, paid again for every list.  Here the same sequence runs once over E
// LISTS WITH TWO SIDES (psx_ransac_sides, ransac_many_plan.h), every kernel one grid over all lists, driven by block
// tables in which no block crosses a list boundary (psx_ransac_many_blocks).  The per-list table entry carries BOTH
// position arrays and both lengths of its list, so the left view may change from list to list:
//   an edge list (psx_ransac_*_graph*, below)         edge e's sides are d_xys[edges[e].left] and d_xys[edges[e].right]
//   a star (psx_ransac_*_many*, ransac_many.hip)      the K lists of ONE left view: every entry names the same left array.
//                                                     That unit only checks the star's arguments and states the sides; it
//                                                     reaches ransac_lists_run through psx_ransac_lists_run
// A star costs nothing here against a gather that takes the left array as a kernel argument: profiles/graph_chain_ms.txt.
// Only the gather reads positions; every kernel behind it works on the packed float4 correspondences.  The rule is
// ransac_rule.h, fundamental_rule.h and affine_rule.h, every step of the estimator is the ONE statement of ransac_core.h
// that the single call runs too: list e's result is the single call's, bit for bit.  "Edge" in the names below is a list.
//   k_rgraph_gather  r_gather per pair of every edge that has a model to estimate, the pair's indices checked against ITS
//                    OWN edge's two lengths, both position arrays through the edge table
//   k_rgraph_hyp     one lane per (edge, hypothesis): r_sample_fit on the edge's own n_e; below the minimum: zeros
//   k_rgraph_score   the hot kernel: r_score_walk over a block of G_HB hypotheses.  The block-table entry and with it the
//                    model address are workgroup uniform (scalar loads).  A wave owns G_PPL x 64 CONSECUTIVE pairs of its
//                    block, and a wave without a resident pair leaves before the walk: a short list's last block is
//                    mostly such waves
//   k_rgraph_select  r_select, one workgroup per edge
//   k_rgraph_count / k_rgraph_scan / k_rgraph_write   r_keep into the stable compaction of wg_compact.h, segmented by edge:
//                    one total per 256-pair workgroup in edge-major order, an exclusive scan of the totals by one
//                    workgroup, one 16-byte store per survivor; an edge's total is the difference of the scan at its
//                    boundaries.  No atomics.  The payload is any 16-byte record array
//   k_rgraph_decide  r_decide, one lane per edge
// The refit's fit is serial by definition and runs on the host: ONE compaction brings every edge's winner
// correspondences through the pinned staging buffer, the host fits the edges whose refit is due, ONE upload carries all
// refit models with a per-edge "tried" word, and the score kernel runs once more with one model per edge.
// Launches per call, whatever the number of lists is: the table copy and a memset, then gather, hyp, score, select and the
// compaction's 3 -- 7 kernels and 1 synchronisation without the refit; with it 5 more (score, decide, the compaction's 3)
// -- 12 kernels and 2 synchronisations.
#include "psx_internal.h"
#include "ransac_core.h"
#include "ransac_graph_plan.h"
#include "wg_compact.h"

#include <cstring>
#include <new>
#include <vector>

namespace {

constexpr int G_PPL = PSX_RANSAC_MANY_SCORE_ROWS / 256;    // pairs resident per lane of the score kernel
constexpr int G_HB = 64;                                    // hypotheses per workgroup of the score kernel
static_assert(G_PPL * 256 == PSX_RANSAC_MANY_SCORE_ROWS && PSX_RANSAC_MANY_ROWS == 256, "block sizes");

struct RGEdge {                              // one entry per edge
    const float2* lxy;                       // the positions of its left view
    const float2* rxy;                       // ... of its right view
    int l_len, r_len;
    int n;                                   // its pairs
    int off;                                 // its first pair in the concatenation
    int b0, b1;                              // its blocks in the 256-pair table (b0 == b1: below the minimum)
    int pad0, pad1;
};
static_assert(sizeof(RGEdge) == 48, "three 16-byte scalar loads per entry");

// grid: the 256-pair blocks
__global__ __launch_bounds__(256) void k_rgraph_gather(const int4* __restrict__ pairs, const RGEdge* __restrict__ edges,
                                                       const int4* __restrict__ blocks, float4* __restrict__ pts, int* __restrict__ bad)
{
    const int4 blk = blocks[blockIdx.x];
    const RGEdge e = edges[blk.x];
    const int p = blk.y + (int)threadIdx.x;
    if (p >= blk.z) return;
    r_gather(pairs[p], e.lxy, e.l_len, e.rxy, e.r_len, pts + p, bad);
}

// grid E * hw (hw = ceil(N / 64)) waves, workgroup e * hw + w: one lane per (edge, hypothesis)
template <int KIND>
__global__ __launch_bounds__(64) void k_rgraph_hyp(const float4* __restrict__ pts, const RGEdge* __restrict__ edges, int hw, unsigned seed, int N,
                                                   float* __restrict__ models, int* __restrict__ counts)
{
    const int e = (int)(blockIdx.x / (unsigned)hw);
    const int h = (int)(blockIdx.x % (unsigned)hw) * 64 + (int)threadIdx.x;
    if (h >= N) return;
    const int n = edges[e].n, off = edges[e].off;
    float m[9];
    if (n >= RModel<KIND>::MIN) r_sample_fit<KIND>(pts + off, n, seed, h, m);              // workgroup uniform
    else {
#pragma unroll
        for (int j = 0; j < 9; j++) m[j] = 0.0f;
    }
    const size_t at = (size_t)e * (size_t)N + (size_t)h;
#pragma unroll
    for (int j = 0; j < 9; j++) models[9 * at + j] = m[j];
    counts[at] = 0;
}

// grid nsb * ceil(N / G_HB), workgroup hb * nsb + b: block b of the score table x hypotheses [hb G_HB, + G_HB) of ITS edge.
// Model (edge, h) lies at models + (edge N + h) mstride, its count at counts + (edge N + h) cstride: 9 and 1 for the
// hypotheses, the RRefit array (N = 1) for the refit.  A wave owns G_PPL x 64 consecutive pairs of its block.
template <int KIND>
__global__ __launch_bounds__(256) void k_rgraph_score(const float4* __restrict__ pts, const int4* __restrict__ blocks, int nsb,
                                                      const float* __restrict__ models, int N, int mstride, float tol,
                                                      int* __restrict__ counts, int cstride)
{
    const int4 blk = blocks[blockIdx.x % (unsigned)nsb];
    const int lane = threadIdx.x & 63;
    const int wave0 = blk.y + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) * (64 * G_PPL);
    if (wave0 >= blk.z) return;                                            // no resident pair in this wave
    psx_ransac_pt q[G_PPL];
    bool in[G_PPL];
#pragma unroll
    for (int k = 0; k < G_PPL; k++) {
        const int p = wave0 + k * 64 + lane;
        in[k] = p < blk.z;
        q[k] = r_pt(in[k] ? pts[p] : make_float4(0.f, 0.f, 0.f, 0.f));
    }
    const int h0 = (int)(blockIdx.x / (unsigned)nsb) * G_HB;
    r_score_walk<KIND, G_PPL>(q, in, models, counts, (size_t)blk.x * (size_t)N, mstride, cstride, h0, h0 + G_HB < N ? h0 + G_HB : N, tol);
}

// one workgroup of 256 threads per edge
__global__ __launch_bounds__(256) void k_rgraph_select(const RGEdge* __restrict__ edges, const int* __restrict__ counts, int N,
                                                       const float* __restrict__ models, RState* __restrict__ st)
{
    const int e = blockIdx.x;
    if (edges[e].b0 == edges[e].b1) return;                                // below the minimum: its state stays zero
    const size_t row = (size_t)e * (size_t)N;
    r_select(counts + row, N, models + 9 * row, st + e);
}

// one lane per edge
template <int KIND>
__global__ __launch_bounds__(256) void k_rgraph_decide(RState* __restrict__ st, const RRefit* __restrict__ rf, int n_edges)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e < n_edges) r_decide<KIND>(st, rf, e);
}

// grid: the 256-pair blocks, edge-major as the table is
template <int KIND>
__global__ __launch_bounds__(256) void k_rgraph_count(const float4* __restrict__ pts, const int4* __restrict__ blocks,
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
__global__ __launch_bounds__(1024) void k_rgraph_scan(const int* __restrict__ wg_tot, int n, int* __restrict__ offs)
{
    wg_scan_totals(wg_tot, n, offs);
}

// grid as k_rgraph_count.  src: the concatenation's 16-byte records (the correspondences themselves, or the pair records);
// out: never written at or past `capacity`.  An edge's first workgroup writes the edge's total, workgroup 0 the sum.
template <int KIND>
__global__ __launch_bounds__(256) void k_rgraph_write(const float4* __restrict__ pts, const RGEdge* __restrict__ edges,
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
        const int b0 = edges[blk.x].b0, b1 = edges[blk.x].b1;
        if ((int)blockIdx.x == b0) st[blk.x].total = offs[b1] - offs[b0];
        if (blockIdx.x == 0) head->total = offs[gridDim.x];
    }
}

size_t pad16(size_t b) { return (b + 15) & ~(size_t)15; }

// what a call holds while it queues: the device arrays and the launch shapes
struct RGQueue {
    hipStream_t st;
    const RGEdge* d_edges;
    const int4 *d_sblk, *d_cblk;
    int nsb, ncb, E;
    float4* d_pts;
    RHead* d_head;
    RState* d_state;
    int *d_tot, *d_offs;
    float tol;
};

template <int KIND>
void queue_score(const RGQueue& q, const float* d_models, int N, int mstride, int* d_counts, int cstride)
{
    const unsigned hb = (unsigned)((N + G_HB - 1) / G_HB);
    hipLaunchKernelGGL(k_rgraph_score<KIND>, dim3((unsigned)q.nsb * hb), dim3(256), 0, q.st, q.d_pts, q.d_sblk, q.nsb, d_models, N, mstride, q.tol,
                       d_counts, cstride);
}

template <int KIND>
void queue_compact(const RGQueue& q, const void* src, void* out, int cap)
{
    hipLaunchKernelGGL(k_rgraph_count<KIND>, dim3((unsigned)q.ncb), dim3(256), 0, q.st, q.d_pts, q.d_cblk, q.d_head, q.d_state, q.tol, q.d_tot);
    hipLaunchKernelGGL(k_rgraph_scan, dim3(1), dim3(1024), 0, q.st, q.d_tot, q.ncb, q.d_offs);
    hipLaunchKernelGGL(k_rgraph_write<KIND>, dim3((unsigned)q.ncb), dim3(256), 0, q.st, q.d_pts, q.d_edges, q.d_cblk, q.d_head, q.d_state, q.tol,
                       q.d_offs, static_cast<const int4*>(src), static_cast<int4*>(out), cap);
}

// The ONE batched driver: E lists with two sides each (psx_ransac_sides, ransac_many_plan.h), their pairs concatenated,
// total_pairs = the sum of list_counts.  The caller has checked its arguments (psx_ransac_graph_args_ok for an edge list,
// psx_ransac_many_args_ok for a star).  host_pairs or d_pairs_in; host_inl or d_inl (the other is NULL; both NULL with
// capacity 0)
template <int KIND>
int ransac_lists_run(int device, const void* host_pairs, const void* d_pairs_in, const int* edge_counts, const psx_ransac_sides* sides, int n_lists,
                     long long total_pairs, const psx_ransac_opts* opts, psx_ransac_result* results, void* host_inl, void* d_inl, int capacity,
                     int* count, float* host_models, int* host_counts)
{
    constexpr int MIN = RModel<KIND>::MIN;
    const int E = n_lists, N = opts->hypotheses, n = (int)total_pairs;
    const long long nsb = psx_ransac_many_blocks(edge_counts, E, MIN, PSX_RANSAC_MANY_SCORE_ROWS, nullptr, 0);
    const long long ncb = psx_ransac_many_blocks(edge_counts, E, MIN, PSX_RANSAC_MANY_ROWS, nullptr, 0);
    if (ncb == 0) { psx_ransac_many_none(E, N, results, count, host_models, host_counts); return PSX_OK; }
    for (int e = 0; e < E; e++)                                            // no index can lie inside an empty array
        if (edge_counts[e] >= MIN && (sides[e].l_len == 0 || sides[e].r_len == 0)) return PSX_ERR_INVALID;
    const long long score_wgs = nsb * ((N + G_HB - 1) / G_HB), hyp_wgs = (long long)E * ((N + 63) / 64);
    if (score_wgs > 0x7fffffffLL || hyp_wgs > 0x7fffffffLL) return PSX_ERR_NOMEM;
    if (hipSetDevice(device) != hipSuccess) return PSX_ERR_HIP;
    MatchScratch& sc = psx_match_scratch();
    if (!sc.bind(device)) return PSX_ERR_HIP;
    const float tol = opts->tol;
    const bool refit = (opts->flags & PSX_RANSAC_REFIT) != 0;
    const int nrec = host_inl ? (capacity < n ? capacity : n) : 0;
    // the device blob: edge table, score blocks, compaction blocks; the pinned buffer: states, refit models, blob, records
    const size_t edges_b = pad16(sizeof(RGEdge) * (size_t)E), sblk_b = sizeof(int4) * (size_t)nsb, cblk_b = sizeof(int4) * (size_t)ncb;
    const size_t blob_b = edges_b + sblk_b + cblk_b;
    const size_t state_b = sizeof(RHead) + sizeof(RState) * (size_t)E, refit_b = sizeof(RRefit) * (size_t)E;
    const size_t pin_state = 0, pin_refit = pad16(state_b), pin_blob = pin_refit + refit_b, pin_rec = pin_blob + blob_b;
    // every buffer before the first launch: nothing is reallocated under queued work
    if ((host_pairs && !sc.need(MS_RANSAC_PAIRS, 16 * (size_t)n)) || !sc.need(MS_RGRAPH_TABLES, blob_b) || !sc.need(MS_RANSAC_PTS, 16 * (size_t)n) ||
        !sc.need(MS_RANSAC_MODELS, sizeof(float) * 9 * (size_t)E * (size_t)N) || !sc.need(MS_RANSAC_COUNTS, sizeof(int) * (size_t)E * (size_t)N) ||
        !sc.need(MS_RANSAC_STATE, pin_refit + refit_b) || !sc.need(MS_RANSAC_TOT, sizeof(int) * (2 * (size_t)ncb + 1)) ||
        !sc.need_pinned(pin_rec + 16 * (size_t)(refit ? n : nrec)))
        return PSX_ERR_NOMEM;
    void* dev_pin = r_pinned_dev(sc);
    if (dev_pin == nullptr) return PSX_ERR_HIP;
    char* hpin = static_cast<char*>(sc.hpin);
    void* d_pin_rec = static_cast<char*>(dev_pin) + pin_rec;

    // ---- the tables, written into the pinned staging buffer and copied on the stream in ONE copy ----
    {
        RGEdge* he = reinterpret_cast<RGEdge*>(hpin + pin_blob);
        psx_ransac_block* tmp = new (std::nothrow) psx_ransac_block[(size_t)ncb];          // nsb <= ncb
        if (!tmp) return PSX_ERR_NOMEM;
        int4* hb = reinterpret_cast<int4*>(hpin + pin_blob + edges_b);
        psx_ransac_many_blocks(edge_counts, E, MIN, PSX_RANSAC_MANY_SCORE_ROWS, tmp, nsb);
        for (long long b = 0; b < nsb; b++) hb[b] = make_int4(tmp[b].set, tmp[b].first, tmp[b].end, 0);
        hb += nsb;
        psx_ransac_many_blocks(edge_counts, E, MIN, PSX_RANSAC_MANY_ROWS, tmp, ncb);
        long long off = 0;
        for (int e = 0; e < E; e++) {
            he[e] = RGEdge{reinterpret_cast<const float2*>(sides[e].lxy), reinterpret_cast<const float2*>(sides[e].rxy), sides[e].l_len, sides[e].r_len,
                           edge_counts[e], (int)off, 0, 0, 0, 0};
            off += edge_counts[e];
        }
        for (long long b = 0; b < ncb; b++) {
            hb[b] = make_int4(tmp[b].set, tmp[b].first, tmp[b].end, 0);
            RGEdge& s = he[tmp[b].set];
            if (s.b1 == 0) s.b0 = (int)b;                                  // an edge's blocks are contiguous: first and last + 1
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
    char* d_blob = static_cast<char*>(sc.buf[MS_RGRAPH_TABLES]);
    char* d_st = static_cast<char*>(sc.buf[MS_RANSAC_STATE]);
    RGQueue q;
    q.st = st; q.E = E; q.nsb = (int)nsb; q.ncb = (int)ncb; q.tol = tol;
    q.d_edges = reinterpret_cast<const RGEdge*>(d_blob);
    q.d_sblk = reinterpret_cast<const int4*>(d_blob + edges_b);
    q.d_cblk = reinterpret_cast<const int4*>(d_blob + edges_b + sblk_b);
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
    hipLaunchKernelGGL(k_rgraph_gather, dim3((unsigned)ncb), dim3(256), 0, st, static_cast<const int4*>(d_pairs), q.d_edges, q.d_cblk, q.d_pts,
                       &q.d_head->bad);
    hipLaunchKernelGGL(k_rgraph_hyp<KIND>, dim3((unsigned)E * hw), dim3(64), 0, st, q.d_pts, q.d_edges, (int)hw, opts->seed, N, d_models, d_counts);
    queue_score<KIND>(q, d_models, N, 9, d_counts, 1);
    hipLaunchKernelGGL(k_rgraph_select, dim3((unsigned)E), dim3(256), 0, st, q.d_edges, d_counts, N, d_models, q.d_state);
    // with the refit: every edge's winner correspondences to the host; without: the inlier records, and the call is complete
    if (refit) queue_compact<KIND>(q, q.d_pts, d_pin_rec, n);
    else queue_compact<KIND>(q, d_pairs, final_out, final_cap);
    if (!r_stage_end(st, hpin + pin_state, d_st, state_b)) return PSX_ERR_HIP;
    if (hh->bad != 0) return PSX_ERR_INVALID;
    auto sane = [&]() {
        long long sum = 0;
        for (int e = 0; e < E; e++) {
            if (hs[e].total < 0 || hs[e].total > edge_counts[e]) return false;
            if (edge_counts[e] >= MIN && (hs[e].best < 0 || hs[e].best >= N)) return false;
            sum += hs[e].total;
        }
        return sum == hh->total;
    };
    if (!sane()) return PSX_ERR_HIP;
    if (refit) {
        // edge e's winner correspondences lie behind those of the edges before it, in pair order; an edge below the
        // minimum has a zero state, which is never due
        RRefit* up = reinterpret_cast<RRefit*>(hpin + pin_refit);
        const psx_ransac_pt* rec = reinterpret_cast<const psx_ransac_pt*>(hpin + pin_rec);
        bool any = false;
        size_t at = 0;
        for (int e = 0; e < E; at += (size_t)hs[e].total, e++) any |= r_refit_model<KIND>(hs[e], rec + at, up + e);
        if (any) {
            if (hipMemcpyAsync(d_refit, up, refit_b, hipMemcpyHostToDevice, st) != hipSuccess) return PSX_ERR_HIP;
            queue_score<KIND>(q, d_refit->m, 1, R_REFIT_WORDS, &d_refit->count, R_REFIT_WORDS);
            hipLaunchKernelGGL(k_rgraph_decide<KIND>, dim3((unsigned)((E + 255) / 256)), dim3(256), 0, st, q.d_state, d_refit, E);
        }
        queue_compact<KIND>(q, d_pairs, final_out, final_cap);
        if (!r_stage_end(st, hpin + pin_state, d_st, state_b) || !sane()) return PSX_ERR_HIP;
    }
    if (!r_download_layers(st, host_models, d_models, host_counts, d_counts, (size_t)E * (size_t)N)) return PSX_ERR_HIP;
    const int total = hh->total;
    if (host_inl && total > 0 && nrec > 0) memcpy(host_inl, hpin + pin_rec, 16 * (size_t)(total < nrec ? total : nrec));
    for (int e = 0; e < E; e++) {                                          // an edge below the minimum has a zero state, which a
        if (edge_counts[e] < MIN) psx_ransac_no_model(results + e);        // homography may take for a model
        else r_result<KIND>(hs[e], results + e);
    }
    *count = total;
    return PSX_OK;
}

// the edge list's entry: its argument checks, then its sides to the driver
template <int KIND>
int ransac_graph_run(int device, const void* host_pairs, const void* d_pairs_in, const int* edge_counts, const psx_view_edge* edges, int n_edges,
                     const float* const* d_xys, const int* lens, int n_sets, const psx_ransac_opts* opts, psx_ransac_result* results,
                     void* host_inl, void* d_inl, int capacity, int* count, float* host_models, int* host_counts)
{
    long long total_pairs = 0;
    if (!psx_ransac_graph_args_ok(host_pairs ? host_pairs : d_pairs_in, edge_counts, edges, n_edges, d_xys, lens, n_sets, opts, results,
                                  host_inl ? host_inl : d_inl, capacity, count, &total_pairs))
        return PSX_ERR_INVALID;
    thread_local std::vector<psx_ransac_sides> sides;
    sides.resize((size_t)n_edges);
    for (int e = 0; e < n_edges; e++) sides[(size_t)e] = psx_ransac_graph_side(edges, d_xys, lens, e);
    return ransac_lists_run<KIND>(device, host_pairs, d_pairs_in, edge_counts, sides.data(), n_edges, total_pairs, opts, results, host_inl, d_inl,
                                  capacity, count, host_models, host_counts);
}

int graph_ref(int model, const void* pairs, const int* edge_counts, const psx_view_edge* edges, int n_edges, const float* const* xys,
              const int* lens, int n_sets, const psx_ransac_opts* opts, psx_ransac_result* results, void* inliers, int capacity, int* count,
              float* models, int* counts)
{
    int longest = 0;
    if (n_edges > 0 && edge_counts != nullptr)
        for (int e = 0; e < n_edges; e++) longest = edge_counts[e] > longest ? edge_counts[e] : longest;
    psx_ransac_pt* scratch = longest > 0 ? new (std::nothrow) psx_ransac_pt[(size_t)longest] : nullptr;
    if (longest > 0 && !scratch) return PSX_ERR_NOMEM;
    const int rc = psx_ransac_graph_host(model, pairs, edge_counts, edges, n_edges, xys, lens, n_sets, opts, results, inliers, capacity, count,
                                         models, counts, scratch);
    delete[] scratch;
    return rc;
}

} // namespace

// the driver for the star adapter (ransac_many.hip): internal, declared in match_scratch.h
int psx_ransac_lists_run(int model, int device, const void* host_pairs, const void* d_pairs, const int* list_counts, const psx_ransac_sides* sides,
                         int n_lists, long long total_pairs, const psx_ransac_opts* opts, psx_ransac_result* results, void* host_inl, void* d_inl,
                         int capacity, int* count, float* host_models, int* host_counts)
{
#define PSX_RUN(KIND)                                                                                                                         \
    case KIND:                                                                                                                                \
        return ransac_lists_run<KIND>(device, host_pairs, d_pairs, list_counts, sides, n_lists, total_pairs, opts, results, host_inl, d_inl, \
                                      capacity, count, host_models, host_counts)
    switch (model) {
        PSX_RUN(PSX_RANSAC_MODEL_HOMOGRAPHY);
        PSX_RUN(PSX_RANSAC_MODEL_FUNDAMENTAL);
        PSX_RUN(PSX_RANSAC_MODEL_AFFINE);
        PSX_RUN(PSX_RANSAC_MODEL_SIMILARITY);
    }
#undef PSX_RUN
    return PSX_ERR_INVALID;
}

// the three forms of one model: lists and inliers on the host, both in HBM, and the host reference
#define PSX_RANSAC_GRAPH_FORMS(name, KIND)                                                                                                      \
    extern "C" int psx_ransac_##name##_graph(int device, const void* host_pairs, const int* edge_counts, const psx_view_edge* edges,            \
                                             int n_edges, const float* const* d_xys, const int* lens, int n_sets,                               \
                                             const psx_ransac_opts* opts, psx_ransac_result* results, void* host_inliers, int capacity,         \
                                             int* count, float* host_models, int* host_counts)                                                  \
    {                                                                                                                                           \
        return ransac_graph_run<KIND>(device, host_pairs, nullptr, edge_counts, edges, n_edges, d_xys, lens, n_sets, opts, results,             \
                                      host_inliers, nullptr, capacity, count, host_models, host_counts);                                        \
    }                                                                                                                                           \
    extern "C" int psx_ransac_##name##_graph_dev(int device, const void* d_pairs, const int* edge_counts, const psx_view_edge* edges,           \
                                                 int n_edges, const float* const* d_xys, const int* lens, int n_sets,                           \
                                                 const psx_ransac_opts* opts, psx_ransac_result* results, void* d_inliers, int capacity,        \
                                                 int* count, float* host_models, int* host_counts)                                              \
    {                                                                                                                                           \
        return ransac_graph_run<KIND>(device, nullptr, d_pairs, edge_counts, edges, n_edges, d_xys, lens, n_sets, opts, results, nullptr,       \
                                      d_inliers, capacity, count, host_models, host_counts);                                                    \
    }                                                                                                                                           \
    extern "C" int psx_ransac_##name##_graph_ref(const void* pairs, const int* edge_counts, const psx_view_edge* edges, int n_edges,            \
                                                 const float* const* xys, const int* lens, int n_sets, const psx_ransac_opts* opts,             \
                                                 psx_ransac_result* results, void* inliers, int capacity, int* count, float* models,            \
                                                 int* counts)                                                                                   \
    {                                                                                                                                           \
        return graph_ref(KIND, pairs, edge_counts, edges, n_edges, xys, lens, n_sets, opts, results, inliers, capacity, count, models, counts); \
    }

PSX_RANSAC_GRAPH_FORMS(homography, PSX_RANSAC_MODEL_HOMOGRAPHY)
PSX_RANSAC_GRAPH_FORMS(fundamental, PSX_RANSAC_MODEL_FUNDAMENTAL)
PSX_RANSAC_GRAPH_FORMS(affine, PSX_RANSAC_MODEL_AFFINE)
PSX_RANSAC_GRAPH_FORMS(similarity, PSX_RANSAC_MODEL_SIMILARITY)
