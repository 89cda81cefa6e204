// bow_query.hip -- query a database of views: psx_bow_quantize_dev, psx_shortlist_query (+ _dev, _ref, _plan)
// (include/popsift_hip.h, "QUERY A DATABASE OF VIEWS").
//
// psx_shortlist_views (bow.hip) ranks every view of one closed collection against every other and keeps N x N scores and
// N x N `listed` bytes in scratch.  Here a few new views are ranked against many stored ones, and NO n_queries x n_db array
// goes through HBM: a score workgroup selects the best of its own 64 x 64 scores before it leaves, and what reaches memory
// is n_queries x blocks x min(k, 64) keys.  The rule is bow_rule.h, the argument checks and the host references are
// bow_plan.h.  Integer arithmetic whose result does not depend on the order in which lanes arrive: the device equals the
// sequential reference bit for bit.
//   k_bow_quantize   one workgroup per view, as k_sl_quant: the row total, q = hist * 65535 / total, df by one atomic per
//                    non-zero bin into a zeroed array that comes down with the call's one synchronisation
//   k_slq_score      grid (ceil(n_db / 64), ceil(n_queries / 64)).  The min-sum tile of k_sl_score over a rectangle: weight * q
//                    staged as 32-bit values in two 32 x 65 LDS tiles, 4 x 4 accumulators per lane, 32 words per step; a
//                    database tile is read once per 64 queries.  Epilogue: the 64 x 64 scores go into the same LDS (the
//                    staging tiles are free by then) as 64 rows of 65; each wave takes 16 query rows, lane l reads column l of
//                    a row -- 64 consecutive words, no two lanes on one bank -- forms psx_query_key (0 where the view is no
//                    candidate) and min(k, 64) rounds of "the largest key below the last one taken" by wave maximum write
//                    partial[i][block][r].  A workgroup whose views lie at or past every limit of its 64 queries writes
//                    empty lists and leaves before the tile.
//   k_slq_merge      one wave per query: k rounds of the same selection over the query's blocks x min(k, 64) keys; writes
//                    neighbours, scores and the unused tail
//   k_slq_edge_count / k_slq_edge_scan / k_slq_edge_write   one lane per list slot (i, r) in row-major order -- the order of
//                    the edge list -- valid where a neighbour was written, into the stable compaction of wg_compact.h
// 5 kernels, one upload (weights and limits), no clear and ONE synchronisation per query call, whatever n_db, n_queries,
// words and k are.  k_sl_score is left as it is: the tile body is stated a second time here, so its figures in
// profiles/shortlist_resources.txt cannot move.
#include "psx_internal.h"
#include "bow_plan.h"
#include "match_scratch.h"
#include "wg_compact.h"

#include <cstring>

namespace {

static_assert(sizeof(psx_view_edge) == 8 && sizeof(psx_query_opts) == 24 && sizeof(psx_query_plan) == 24, "record sizes");

constexpr int SLQ_TILE = PSX_QUERY_TILE;   // views per side of a score workgroup
constexpr int SLQ_KT = 32;                 // words per staged step
constexpr int SLQ_LD = SLQ_TILE + 1;       // the padded row of an LDS tile
static_assert(2 * SLQ_KT == SLQ_TILE, "the two staging tiles hold the 64 x 65 scores of the epilogue exactly");

// grid n_views, one workgroup per view; df may be NULL
__global__ __launch_bounds__(256) void k_bow_quantize(const unsigned* __restrict__ hist, int W, unsigned short* __restrict__ q, int* __restrict__ df)
{
    __shared__ unsigned long long s_part[4];
    const unsigned* h = hist + (size_t)blockIdx.x * (size_t)W;
    unsigned long long n = 0;
    for (int w = threadIdx.x; w < W; w += 256) n += h[w];
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) n += __shfl_xor(n, k);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = n;
    __syncthreads();
    n = s_part[0] + s_part[1] + s_part[2] + s_part[3];
    for (int w = threadIdx.x; w < W; w += 256) {
        const unsigned c = h[w];
        q[(size_t)blockIdx.x * (size_t)W + w] = (unsigned short)psx_bow_quant(c, n);
        if (df != nullptr && c > 0) atomicAdd(df + w, 1);
    }
}

__device__ __forceinline__ unsigned long long wave_max(unsigned long long v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) { const unsigned long long o = __shfl_xor(v, m); v = o > v ? o : v; }
    return v;
}

// grid (blocks, ceil(nq / 64)).  Lane (ty, tx) owns (query 64 bi + ty + 16 r, view 64 bj + tx + 16 c).  partial holds kpb keys
// per (query, block); every workgroup writes all kpb entries of each of its queries, so the array is never cleared.
__global__ __launch_bounds__(256) void k_slq_score(const unsigned short* __restrict__ dbq, int n_db, const unsigned short* __restrict__ qq, int nq,
                                                   int W, const int* __restrict__ weight, const int* __restrict__ limit, int self_base,
                                                   unsigned min_score, int kpb, unsigned long long* __restrict__ partial)
{
    __shared__ unsigned s_mem[2 * SLQ_KT * SLQ_LD];
    __shared__ int s_limit[SLQ_TILE];
    unsigned (*s_i)[SLQ_LD] = reinterpret_cast<unsigned (*)[SLQ_LD]>(s_mem);
    unsigned (*s_j)[SLQ_LD] = reinterpret_cast<unsigned (*)[SLQ_LD]>(s_mem + SLQ_KT * SLQ_LD);
    const int bi = (int)blockIdx.y, bj = (int)blockIdx.x, blocks = (int)gridDim.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x < SLQ_TILE) {
        const int i = bi * SLQ_TILE + (int)threadIdx.x;
        s_limit[threadIdx.x] = i < nq ? limit[i] : 0;
    }
    __syncthreads();
    int most = s_limit[lane];                                  // every wave: the largest limit of the 64 queries
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) most = max(most, __shfl_xor(most, m));
    if (bj * SLQ_TILE >= most) {                               // uniform over the workgroup: no view here is a candidate
        for (int e = threadIdx.x; e < SLQ_TILE * kpb; e += 256) {
            const int i = bi * SLQ_TILE + e / kpb;
            if (i < nq) partial[((size_t)i * blocks + bj) * kpb + e % kpb] = 0ULL;
        }
        return;
    }
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    unsigned acc[4][4];
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
        for (int c = 0; c < 4; c++) acc[r][c] = 0u;
    for (int w0 = 0; w0 < W; w0 += SLQ_KT) {
        for (int e = threadIdx.x; e < SLQ_TILE * SLQ_KT; e += 256) {
            const int r = e / SLQ_KT, k = e % SLQ_KT, w = w0 + k;
            const int vi = bi * SLQ_TILE + r, vj = bj * SLQ_TILE + r;
            const unsigned wt = w < W ? (unsigned)weight[w] : 0u;
            s_i[k][r] = (w < W && vi < nq) ? wt * qq[(size_t)vi * (size_t)W + w] : 0u;
            s_j[k][r] = (w < W && vj < n_db) ? wt * dbq[(size_t)vj * (size_t)W + w] : 0u;
        }
        __syncthreads();
#pragma unroll 4
        for (int k = 0; k < SLQ_KT; k++) {
            unsigned a[4], b[4];
#pragma unroll
            for (int r = 0; r < 4; r++) { a[r] = s_i[k][ty + 16 * r]; b[r] = s_j[k][tx + 16 * r]; }
#pragma unroll
            for (int r = 0; r < 4; r++)
#pragma unroll
                for (int c = 0; c < 4; c++) acc[r][c] += min(a[r], b[c]);
        }
        __syncthreads();                                       // also: the staging tiles are free for the scores
    }
    unsigned (*s_sc)[SLQ_LD] = reinterpret_cast<unsigned (*)[SLQ_LD]>(s_mem);      // 64 rows of 65: query row, view column
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
        for (int c = 0; c < 4; c++) s_sc[ty + 16 * r][tx + 16 * c] = acc[r][c];
    __syncthreads();
    const int j = bj * SLQ_TILE + lane;                        // this lane's database view in every row
    for (int row = wave * 16; row < wave * 16 + 16; row++) {
        const int i = bi * SLQ_TILE + row;
        if (i >= nq) break;                                    // wave uniform
        const unsigned s = s_sc[row][lane];
        const bool cand = j < n_db && psx_query_candidate(s, j, s_limit[row], self_base >= 0 ? self_base + i : -1, min_score);
        const unsigned long long key = cand ? psx_query_key(s, j) : 0ULL;
        unsigned long long* out = partial + ((size_t)i * blocks + bj) * kpb;
        unsigned long long last = ~0ULL;
        int r = 0;
        for (; r < kpb; r++) {                                 // the largest key below the last one taken
            const unsigned long long best = wave_max(key < last ? key : 0ULL);
            if (best == 0) break;
            if (lane == 0) out[r] = best;
            last = best;
        }
        for (int e = r + lane; e < kpb; e += 64) out[e] = 0ULL;
    }
}

// grid ceil(nq / 4), one wave per query; n_keys = blocks * kpb keys per query (0 with an empty database).  nb / sc may be NULL.
__global__ __launch_bounds__(256) void k_slq_merge(const unsigned long long* __restrict__ partial, int nq, int n_keys, int k, int* __restrict__ nb,
                                                   unsigned* __restrict__ sc)
{
    const int i = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= nq) return;                                       // wave uniform
    const unsigned long long* keys = partial + (size_t)i * (size_t)n_keys;
    unsigned long long last = ~0ULL;
    int r = 0;
    for (; r < k; r++) {
        unsigned long long best = 0;
        for (int e = lane; e < n_keys; e += 64) {
            const unsigned long long key = keys[e];
            if (key < last && key > best) best = key;
        }
        best = wave_max(best);
        if (best == 0) break;
        if (lane == 0) {
            if (nb != nullptr) nb[(size_t)i * k + r] = psx_query_key_view(best);
            if (sc != nullptr) sc[(size_t)i * k + r] = psx_query_key_score(best);
        }
        last = best;
    }
    for (int e = r + lane; e < k; e += 64) {
        if (nb != nullptr) nb[(size_t)i * k + e] = -1;
        if (sc != nullptr) sc[(size_t)i * k + e] = 0u;
    }
}

// what the count and the write kernel decide per lane, the same way: lane idx is the list slot (idx / k, idx % k)
__device__ __forceinline__ bool slq_edge(const int* __restrict__ nb, unsigned slots, unsigned* idx, int* j)
{
    *idx = blockIdx.x * 256u + threadIdx.x;
    if (*idx >= slots) return false;
    *j = nb[*idx];
    return *j >= 0;
}

// grid ceil(nq k / 256)
__global__ __launch_bounds__(256) void k_slq_edge_count(const int* __restrict__ nb, unsigned slots, int* __restrict__ wg_tot)
{
    unsigned idx = 0;
    int j = 0;
    __shared__ int s_cnt[4];
    wg_count(__ballot(slq_edge(nb, slots, &idx, &j)), s_cnt);
    if (threadIdx.x == 0) wg_tot[blockIdx.x] = wg_total(s_cnt);
}

// ONE workgroup of 1024 threads
__global__ __launch_bounds__(1024) void k_slq_edge_scan(const int* __restrict__ wg_tot, int n, int* __restrict__ offs)
{
    wg_scan_totals(wg_tot, n, offs);
}

// grid as k_slq_edge_count.  Nothing is written at or past the capacity.
__global__ __launch_bounds__(256) void k_slq_edge_write(const int* __restrict__ nb, unsigned slots, int k, int edge_base, const int* __restrict__ offs,
                                                        psx_view_edge* __restrict__ edges, int capacity, int* __restrict__ total)
{
    unsigned idx = 0;
    int j = 0;
    const bool keep = slq_edge(nb, slots, &idx, &j);
    const unsigned long long m = __ballot(keep);
    __shared__ int s_cnt[4];
    wg_count(m, s_cnt);
    const int slot = offs[blockIdx.x] + wg_offset(m, s_cnt);
    if (keep && slot < capacity) edges[slot] = psx_view_edge{edge_base + (int)(idx / (unsigned)k), j};
    if (blockIdx.x == 0 && threadIdx.x == 0) *total = offs[gridDim.x];
}

int quantize_run(int device, const unsigned* d_hist, int n_views, int W, unsigned short* d_q, int* df_accum)
{
    if (!psx_bow_quantize_args_ok(d_hist, n_views, W, d_q, true)) return PSX_ERR_INVALID;
    if (n_views == 0) return PSX_OK;
    if (hipSetDevice(device) != hipSuccess) return PSX_ERR_HIP;
    MatchScratch& sc = psx_match_scratch();
    if (!sc.bind(device)) return PSX_ERR_HIP;
    hipStream_t st = sc.stream;
    const size_t df_b = 4 * (size_t)W;
    if (df_accum != nullptr && (!sc.need(MS_SLQ_DF, df_b) || !sc.need_pinned(df_b))) return PSX_ERR_NOMEM;
    int* d_df = df_accum != nullptr ? static_cast<int*>(sc.buf[MS_SLQ_DF]) : nullptr;
    if (d_df != nullptr && hipMemsetAsync(d_df, 0, df_b, st) != hipSuccess) return PSX_ERR_HIP;
    hipLaunchKernelGGL(k_bow_quantize, dim3((unsigned)n_views), dim3(256), 0, st, d_hist, W, d_q, d_df);
    if (hipGetLastError() != hipSuccess) return PSX_ERR_HIP;
    if (d_df != nullptr && hipMemcpyAsync(sc.hpin, d_df, df_b, hipMemcpyDeviceToHost, st) != hipSuccess) return PSX_ERR_HIP;
    if (hipStreamSynchronize(st) != hipSuccess) return PSX_ERR_HIP;
    if (d_df != nullptr) {
        const int* h = static_cast<const int*>(sc.hpin);
        for (int w = 0; w < W; w++) {
            if (h[w] < 0 || h[w] > n_views) return PSX_ERR_HIP;
        }
        for (int w = 0; w < W; w++) df_accum[w] += h[w];
    }
    return PSX_OK;
}

// the q arrays: device memory.  nb / scores / edges: all host memory (host_out) or all device memory
int query_run(int device, const unsigned short* d_dbq, int n_db, const unsigned short* d_qq, int nq, int W, const int* weights, const int* db_limit,
              const psx_query_opts* opts, bool host_out, int* nb, unsigned* scores, psx_view_edge* edges, int capacity, int* count)
{
    psx_query_plan plan;
    if (!psx_query_args_ok(d_dbq, n_db, d_qq, nq, W, weights, db_limit, opts, nb, scores, edges, capacity, count, true, !host_out, &plan))
        return PSX_ERR_INVALID;
    if (nq == 0) { *count = 0; return PSX_OK; }
    const int k = opts->k;
    if (n_db == 0 && host_out) { psx_shortlist_none(nq, k, nb, scores); *count = 0; return PSX_OK; }
    const size_t slots = (size_t)nq * (size_t)k, list_b = 4 * slots;
    const size_t most = (size_t)nq * (size_t)(k < n_db ? k : n_db);                                    // edges that can exist
    const int h_cap = (size_t)capacity < most ? capacity : (int)most;
    const int nwg = (int)psx_query_slot_blocks(nq, k);
    const size_t w_b = psx_pad16(4 * (size_t)W), tab_b = w_b + psx_pad16(4 * (size_t)nq);
    // MS_SLQ_OUT: the neighbours (the host form's, or the call's own when a _dev caller passes none), then the host form's
    // scores and edges
    const bool own_nb = host_out || nb == nullptr;
    const size_t out_nb = 0, out_sc = out_nb + (own_nb ? psx_pad16(list_b) : 0), out_ed = out_sc + (host_out && scores ? psx_pad16(list_b) : 0),
                 out_b = out_ed + (host_out && edges ? 8 * (size_t)h_cap : 0);
    const size_t pin_total = 0, pin_tab = 16, pin_out = pin_tab + tab_b;
    if (hipSetDevice(device) != hipSuccess) return PSX_ERR_HIP;
    MatchScratch& sc = psx_match_scratch();
    if (!sc.bind(device)) return PSX_ERR_HIP;
    hipStream_t st = sc.stream;
    // every buffer before the first launch: nothing is reallocated under queued work
    if (!sc.need(MS_SLQ_TABLES, tab_b) || (plan.partial_keys > 0 && !sc.need(MS_SLQ_PARTIAL, 8 * (size_t)plan.partial_keys)) ||
        !sc.need(MS_SLQ_TOT, 4 * (2 * (size_t)nwg + 2)) || (out_b > 0 && !sc.need(MS_SLQ_OUT, out_b)) ||
        !sc.need_pinned(pin_out + (host_out ? out_b : 0)))
        return PSX_ERR_NOMEM;
    char* hpin = static_cast<char*>(sc.hpin);
    char* d_out = static_cast<char*>(sc.buf[MS_SLQ_OUT]);
    int* d_nb = own_nb ? reinterpret_cast<int*>(d_out + out_nb) : nb;
    unsigned* d_sc = host_out ? (scores ? reinterpret_cast<unsigned*>(d_out + out_sc) : nullptr) : scores;
    psx_view_edge* d_edges = host_out ? (edges ? reinterpret_cast<psx_view_edge*>(d_out + out_ed) : nullptr) : edges;
    const int cap = host_out ? (edges ? h_cap : 0) : capacity;
    unsigned long long* d_partial = static_cast<unsigned long long*>(sc.buf[MS_SLQ_PARTIAL]);
    if (n_db == 0) {                                           // the _dev form: every entry unused, no edge
        hipLaunchKernelGGL(k_slq_merge, dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, st, d_partial, nq, 0, k, nb, scores);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return PSX_ERR_HIP;
        *count = 0;
        return PSX_OK;
    }
    // ONE upload: the weights and, behind them, a limit per query
    memcpy(hpin + pin_tab, weights, 4 * (size_t)W);
    int* h_limit = reinterpret_cast<int*>(hpin + pin_tab + w_b);
    for (int i = 0; i < nq; i++) h_limit[i] = db_limit != nullptr ? db_limit[i] : n_db;
    char* d_tab = static_cast<char*>(sc.buf[MS_SLQ_TABLES]);
    if (hipMemcpyAsync(d_tab, hpin + pin_tab, tab_b, hipMemcpyHostToDevice, st) != hipSuccess) return PSX_ERR_HIP;
    const int* d_weight = reinterpret_cast<const int*>(d_tab);
    const int* d_limit = reinterpret_cast<const int*>(d_tab + w_b);
    int* d_tot = static_cast<int*>(sc.buf[MS_SLQ_TOT]);
    int* d_offs = d_tot + (size_t)nwg;
    int* d_total = d_offs + (size_t)nwg + 1;
    const int kpb = plan.keys_per_block;
    hipLaunchKernelGGL(k_slq_score, dim3((unsigned)plan.blocks, (unsigned)((nq + SLQ_TILE - 1) / SLQ_TILE)), dim3(256), 0, st, d_dbq, n_db, d_qq, nq, W,
                       d_weight, d_limit, opts->self_base, opts->min_score, kpb, d_partial);
    hipLaunchKernelGGL(k_slq_merge, dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, st, d_partial, nq, plan.blocks * kpb, k, d_nb, d_sc);
    hipLaunchKernelGGL(k_slq_edge_count, dim3((unsigned)nwg), dim3(256), 0, st, d_nb, (unsigned)slots, d_tot);
    hipLaunchKernelGGL(k_slq_edge_scan, dim3(1), dim3(1024), 0, st, d_tot, nwg, d_offs);
    hipLaunchKernelGGL(k_slq_edge_write, dim3((unsigned)nwg), dim3(256), 0, st, d_nb, (unsigned)slots, k, opts->edge_base, d_offs, d_edges, cap, d_total);
    if (hipGetLastError() != hipSuccess) return PSX_ERR_HIP;
    if (host_out && out_b > 0 && hipMemcpyAsync(hpin + pin_out, d_out, out_b, hipMemcpyDeviceToHost, st) != hipSuccess) return PSX_ERR_HIP;
    if (hipMemcpyAsync(hpin + pin_total, d_total, 4, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
        return PSX_ERR_HIP;
    const int total = *reinterpret_cast<const int*>(hpin + pin_total);
    if (total < 0 || (size_t)total > most) return PSX_ERR_HIP;
    if (host_out) {
        if (nb) memcpy(nb, hpin + pin_out + out_nb, list_b);
        if (scores) memcpy(scores, hpin + pin_out + out_sc, list_b);
        if (edges && h_cap > 0) memcpy(edges, hpin + pin_out + out_ed, 8 * (size_t)(total < h_cap ? total : h_cap));
    }
    *count = total;
    return PSX_OK;
}

} // namespace

extern "C" int psx_bow_quantize_dev(int device, const unsigned* d_hist, int n_views, int words, unsigned short* d_q, int* df_accum)
{
    return quantize_run(device, d_hist, n_views, words, d_q, df_accum);
}

extern "C" int psx_bow_quantize_ref(const unsigned* hist, int n_views, int words, unsigned short* q, int* df_accum)
{
    return psx_bow_quantize_host(hist, n_views, words, q, df_accum);
}

extern "C" int psx_shortlist_query(int device, const unsigned short* d_db_q, int n_db, const unsigned short* d_query_q, int n_queries, int words,
                                   const int* weights, const int* db_limit, const psx_query_opts* opts, int* host_neighbours,
                                   unsigned* host_scores, psx_view_edge* host_edges, int edge_capacity, int* edge_count)
{
    return query_run(device, d_db_q, n_db, d_query_q, n_queries, words, weights, db_limit, opts, true, host_neighbours, host_scores, host_edges,
                     edge_capacity, edge_count);
}

extern "C" int psx_shortlist_query_dev(int device, const unsigned short* d_db_q, int n_db, const unsigned short* d_query_q, int n_queries, int words,
                                       const int* weights, const int* db_limit, const psx_query_opts* opts, int* d_neighbours,
                                       unsigned* d_scores, psx_view_edge* d_edges, int edge_capacity, int* edge_count)
{
    return query_run(device, d_db_q, n_db, d_query_q, n_queries, words, weights, db_limit, opts, false, d_neighbours, d_scores, d_edges,
                     edge_capacity, edge_count);
}

extern "C" int psx_shortlist_query_ref(const unsigned short* db_q, int n_db, const unsigned short* query_q, int n_queries, int words,
                                       const int* weights, const int* db_limit, const psx_query_opts* opts, int* neighbours, unsigned* scores,
                                       psx_view_edge* edges, int edge_capacity, int* edge_count)
{
    return psx_shortlist_query_host(db_q, n_db, query_q, n_queries, words, weights, db_limit, opts, neighbours, scores, edges, edge_capacity,
                                    edge_count);
}

extern "C" int psx_shortlist_query_plan(int n_db, int n_queries, int words, int k, psx_query_plan* plan)
{
    return psx_query_plan_host(n_db, n_queries, words, k, plan);
}
