// bow.hip -- which view pairs to match: psx_vocab_train_u8, psx_bow_u8, psx_shortlist_views (+ _dev, _ref) and
// psx_bow_weights (include/popsift_hip.h).
//
// The chain psx_match_pairs_graph_u8* -> psx_ransac_*_graph* -> psx_match_pairs_guided_graph_u8* -> psx_tracks_graph* takes
// its edge list from the caller; these calls make one: a visual vocabulary, a bag of words per view, the k most similar
// views per view and the sorted, deduplicated edges.  The rule is bow_rule.h, the argument checks and the host references
// are bow_plan.h; here is the device sequence.  Everything is integer arithmetic whose result does not depend on the order
// in which lanes arrive, so the device equals the sequential reference bit for bit.
//
// ASSIGNMENT, shared by training and psx_bow_u8: a 1-NN search of byte descriptors, built from the pieces of
// match_u8_core.h.  The rows of all views are first gathered into ONE array (k_bow_gather), so the outer side is plain
// global rows, 64 per wave, and a workgroup spans a view boundary without knowing it.
//   k_bow_gather   one 16-byte load and store per lane; the view of a row is a search of the offset table
//   k_bow_norms    |x - 128|^2 per row, padded as u8_pad says (the rows once, the words once per iteration)
//   k_bow_assign   one workgroup per 256 rows; a wave loads its 64 rows once (u8_load_cols on the workgroup's slice, so the
//                  row numbers are local), then per chunk of <= U8_CHUNK_MAX words: u8_walk, u8_store_keys into LDS,
//                  u8_merge_chunk in index order -- no per-chunk partials in HBM, whatever W is.  In training it also
//                  counts the rows whose word changed (a ballot) and adds up the distances (a wave sum): one 32-bit and
//                  one 64-bit atomic per wave.
// TRAINING, per iteration: one clear of the sums; k_bow_norms of the words; k_bow_assign; k_bow_accum (32 lanes per row:
// four byte sums each and one count per row, 32-bit atomics -- integer additions, any order gives the same bytes);
// k_bow_update (one lane per byte of a word: psx_bow_mean, empty words counted); one copy of the 16 bytes {changed, empty,
// inertia} and ONE synchronisation that decides the stop.  Once per call: the table copy, k_bow_gather, k_bow_norms of the
// rows, k_bow_init and the clear of the previous words.  The accumulation uses global atomics because a word's 129
// counters are spread over W x 129 addresses: with W in the thousands two lanes rarely meet.  LDS-privatised partials
// need W x 516 bytes per workgroup, which W = 4096 does not fit, and a sort by word costs a radix sort of M keys and a
// 128-byte gather per iteration; neither was measured against it (profiles/shortlist_ms.txt has the call's time).
// BAGS: the table copy, k_bow_gather, k_bow_norms twice, k_bow_assign, one clear, k_bow_hist (one atomic per row); one
// synchronisation.
// LISTS:
//   k_sl_quant     one workgroup per view: the row total, q = hist * 65535 / total (uint16), df by one atomic per non-zero bin
//   (host)         df comes down, psx_bow_weights_host, the weights go up: the device never evaluates a logarithm
//   k_sl_score     the min-sum product: 64 x 64 views per workgroup, 4 x 4 per lane, 32 words per step staged in LDS as
//                  weight * q; only blocks with j >= i are computed, both halves are written.  VALU work, no MFMA
//   k_sl_topk      one wave per view, k selection rounds over psx_shortlist_key; marks listed[i][j]
//   k_sl_edge_count / k_sl_edge_scan / k_sl_edge_write   one lane per (a, b) in row-major order -- the order of the edge
//                  list -- psx_shortlist_edge_keep into the stable compaction of wg_compact.h
// 6 kernels, 2 clears and TWO synchronisations, whatever N and W are.
#include "psx_internal.h"
#include "bow_plan.h"
#include "match_scratch.h"
#include "match_u8_core.h"
#include "wg_compact.h"

#include <cstring>

namespace {

static_assert(PSX_BOW_DIM == 128 && sizeof(psx_view_edge) == 8 && sizeof(psx_vocab_info) == 24, "row and record sizes");

// what an iteration brings back
struct BowHead { int changed, empty; unsigned long long inertia; };
static_assert(sizeof(BowHead) == 16, "one 16-byte copy");

constexpr int SL_TILE = 64;      // views per side of a score workgroup
constexpr int SL_KT = 32;        // words per staged step

// the last view whose offset is <= g: empty views before it lose
__device__ __forceinline__ int bow_view(const int* __restrict__ off, int n_sets, int g)
{
    int lo = 0, hi = n_sets;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= g) lo = mid; else hi = mid;
    }
    return lo;
}

// grid ceil(8 M / 256): lane t copies 16 bytes, row t >> 3
__global__ __launch_bounds__(256) void k_bow_gather(const unsigned char* const* __restrict__ sets, const int* __restrict__ off, int n_sets, int M,
                                                    uint4* __restrict__ rows)
{
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if ((t >> 3) >= (size_t)M) return;
    const int g = (int)(t >> 3), q = (int)(t & 7);
    const int v = bow_view(off, n_sets, g);
    rows[t] = reinterpret_cast<const uint4*>(sets[v] + (size_t)(g - off[v]) * PSX_BOW_DIM)[q];
}

// grid ceil(8 u8_pad(n) / 256): 8 lanes per row, zeros in the padding
__global__ __launch_bounds__(256) void k_bow_norms(const unsigned char* __restrict__ src, int n, int* __restrict__ norms)
{
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t d = t >> 3;
    const int ss = u8_row_norm(src, n, d < (size_t)n ? (int)d : n, (int)(t & 7));       // a row at or past n reads nothing
    if ((t & 7) == 0 && d < (size_t)u8_pad(n)) norms[d] = ss;
}

// grid ceil(8 W / 256): word w = the bytes of global row psx_bow_init_row(w)
__global__ __launch_bounds__(256) void k_bow_init(const uint4* __restrict__ rows, int M, int W, uint4* __restrict__ vocab)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= 8 * W) return;
    vocab[t] = rows[(size_t)psx_bow_init_row(t >> 3, M, W) * 8 + (size_t)(t & 7)];
}

// grid ceil(M / 256).  words[g] = a(g).  head != NULL (training): prev[g] is read, the rows with another word than before
// and the sum of the distances are added to *head.
__global__ __launch_bounds__(256) void k_bow_assign(const unsigned char* __restrict__ rows, const int* __restrict__ xn, int M,
                                                    const unsigned char* __restrict__ vocab, const int* __restrict__ vn, int W,
                                                    int* __restrict__ words, const int* __restrict__ prev, BowHead* head)
{
    __shared__ uint2 s_keys[256];
    const int row0 = (int)blockIdx.x * 256;
    const int left = M - row0;                                 // rows from this workgroup's first on: >= 1
    U8Wave w;
    // the workgroup's slice as a set of its own: row numbers are local, idle columns repeat the last row of all
    u8_load_cols(w, rows + (size_t)row0 * PSX_BOW_DIM, xn + row0, left, (int)(threadIdx.x >> 6) * 64);
    U8Best best;
    const bool live = (int)threadIdx.x < left;
    for (int r0 = 0; r0 < W; r0 += U8_CHUNK_MAX) {
        const int r1 = min(r0 + U8_CHUNK_MAX, W);
#pragma unroll
        for (int c = 0; c < 2; c++) w.m1[c] = w.m2[c] = U8_NONE;
        u8_walk(w, vocab, vn, W, r0, r1);
        u8_store_keys(w, left, s_keys);                        // local rows < 256: inside s_keys
        __syncthreads();
        if (live) u8_merge_chunk(best, s_keys[threadIdx.x], r0);
        __syncthreads();                                       // s_keys is rewritten by the next chunk
    }
    if (live) words[row0 + (int)threadIdx.x] = best.i1;
    if (head == nullptr) return;
    const bool moved = live && prev[row0 + (int)threadIdx.x] != best.i1;
    const unsigned long long m = __ballot(moved);
    unsigned d = live ? (unsigned)best.d1 : 0u;                // 64 distances of at most 128 * 255^2 fit 32 bits
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) d += __shfl_xor(d, k);
    if ((threadIdx.x & 63) == 0) {
        if (m) atomicAdd(&head->changed, __popcll(m));
        if (d) atomicAdd(&head->inertia, (unsigned long long)d);
    }
}

// grid ceil(32 M / 256): lane t adds bytes 4 (t & 31) .. + 3 of row t >> 5 to its word's sums, lane 0 of a row counts it
__global__ __launch_bounds__(256) void k_bow_accum(const unsigned* __restrict__ rows, const int* __restrict__ words, int M,
                                                   unsigned* __restrict__ cnt, unsigned* __restrict__ sum)
{
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if ((t >> 5) >= (size_t)M) return;
    const int k4 = (int)(t & 31);
    const size_t w = (size_t)words[t >> 5];
    const unsigned v = rows[t];
    unsigned* s = sum + w * PSX_BOW_DIM + 4 * k4;
#pragma unroll
    for (int b = 0; b < 4; b++) atomicAdd(s + b, (v >> (8 * b)) & 0xffu);
    if (k4 == 0) atomicAdd(cnt + w, 1u);
}

// grid ceil(128 W / 256): one lane per byte of a word
__global__ __launch_bounds__(256) void k_bow_update(unsigned char* __restrict__ vocab, const unsigned* __restrict__ cnt,
                                                    const unsigned* __restrict__ sum, int W, BowHead* head)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= PSX_BOW_DIM * W) return;
    const unsigned c = cnt[t >> 7];
    if (c == 0) { if ((t & 127) == 0) atomicAdd(&head->empty, 1); }
    else vocab[t] = psx_bow_mean(sum[t], c);
}

// grid ceil(M / 256): one atomic per row
__global__ __launch_bounds__(256) void k_bow_hist(const int* __restrict__ words, const int* __restrict__ off, int n_sets, int M, int W,
                                                  unsigned* __restrict__ hist)
{
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= M) return;
    atomicAdd(hist + (size_t)bow_view(off, n_sets, g) * (size_t)W + (size_t)words[g], 1u);
}

// grid N, one workgroup per view
__global__ __launch_bounds__(256) void k_sl_quant(const unsigned* __restrict__ hist, int W, unsigned short* __restrict__ q, int* __restrict__ df)
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
        if (c > 0) atomicAdd(df + w, 1);
    }
}

// grid (T, T), T = ceil(N / 64); the workgroups below the diagonal leave at once.  Lane (ty, tx) owns views
// (64 bi + ty + 16 r, 64 bj + tx + 16 c).  The staged value is weight * q: min commutes with a weight that is not negative.
__global__ __launch_bounds__(256) void k_sl_score(const unsigned short* __restrict__ q, const int* __restrict__ weight, int N, int W,
                                                  unsigned* __restrict__ score)
{
    const int bi = (int)blockIdx.y, bj = (int)blockIdx.x;
    if (bj < bi) return;
    __shared__ unsigned s_i[SL_KT][SL_TILE + 1], s_j[SL_KT][SL_TILE + 1];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    unsigned acc[4][4];
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
        for (int c = 0; c < 4; c++) acc[r][c] = 0u;
    for (int w0 = 0; w0 < W; w0 += SL_KT) {
        for (int e = threadIdx.x; e < SL_TILE * SL_KT; e += 256) {
            const int r = e / SL_KT, k = e % SL_KT, w = w0 + k;
            const int vi = bi * SL_TILE + r, vj = bj * SL_TILE + r;
            const unsigned wt = w < W ? (unsigned)weight[w] : 0u;
            s_i[k][r] = (w < W && vi < N) ? wt * q[(size_t)vi * (size_t)W + w] : 0u;
            s_j[k][r] = (w < W && vj < N) ? wt * q[(size_t)vj * (size_t)W + w] : 0u;
        }
        __syncthreads();
#pragma unroll 4
        for (int k = 0; k < SL_KT; k++) {
            unsigned a[4], b[4];
#pragma unroll
            for (int r = 0; r < 4; r++) { a[r] = s_i[k][ty + 16 * r]; b[r] = s_j[k][tx + 16 * r]; }
#pragma unroll
            for (int r = 0; r < 4; r++)
#pragma unroll
                for (int c = 0; c < 4; c++) acc[r][c] += min(a[r], b[c]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const int i = bi * SL_TILE + ty + 16 * r, j = bj * SL_TILE + tx + 16 * c;
            if (i < N && j < N) {
                score[(size_t)i * N + j] = acc[r][c];
                score[(size_t)j * N + i] = acc[r][c];
            }
        }
}

// grid ceil(N / 4), one wave per view; kk = min(k, N - 1) rounds at most.  nb / sc may be NULL.
__global__ __launch_bounds__(256) void k_sl_topk(const unsigned* __restrict__ score, int N, int k, int kk, int* __restrict__ nb,
                                                 unsigned* __restrict__ sc, unsigned char* __restrict__ listed)
{
    const int i = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= N) return;                                        // wave uniform
    const unsigned* row = score + (size_t)i * N;
    unsigned long long last = ~0ULL;
    int r = 0;
    for (; r < kk; r++) {                                      // the largest key below the last one taken
        unsigned long long best = 0;
        for (int j = lane; j < N; j += 64) {
            const unsigned s = j != i ? row[j] : 0u;
            const unsigned long long key = s > 0 ? psx_shortlist_key(s, j) : 0ULL;
            if (key < last && key > best) best = key;
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) { const unsigned long long o = __shfl_xor(best, m); best = o > best ? o : best; }
        if (best == 0) break;
        if (lane == 0) {
            const int j = psx_shortlist_key_view(best);
            if (nb != nullptr) nb[(size_t)i * k + r] = j;
            if (sc != nullptr) sc[(size_t)i * k + r] = psx_shortlist_key_score(best);
            listed[(size_t)i * N + j] = 1;
        }
        last = best;
    }
    for (int e = r + lane; e < k; e += 64) {
        if (nb != nullptr) nb[(size_t)i * k + e] = -1;
        if (sc != nullptr) sc[(size_t)i * k + e] = 0u;
    }
}

// what the count and the write kernel decide per lane, the same way: lane idx is the pair (idx / N, idx % N)
__device__ __forceinline__ bool sl_edge(const unsigned char* __restrict__ listed, int N, int flags, int* a, int* b)
{
    const unsigned idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= (unsigned)N * (unsigned)N) return false;
    *a = (int)(idx / (unsigned)N); *b = (int)(idx % (unsigned)N);
    if (*a >= *b) return false;
    return psx_shortlist_edge_keep(listed[(size_t)*a * N + *b] != 0, listed[(size_t)*b * N + *a] != 0, flags);
}

// grid ceil(N N / 256)
__global__ __launch_bounds__(256) void k_sl_edge_count(const unsigned char* __restrict__ listed, int N, int flags, int* __restrict__ wg_tot)
{
    int a = 0, b = 0;
    __shared__ int s_cnt[4];
    wg_count(__ballot(sl_edge(listed, N, flags, &a, &b)), s_cnt);
    if (threadIdx.x == 0) wg_tot[blockIdx.x] = wg_total(s_cnt);
}

// ONE workgroup of 1024 threads
__global__ __launch_bounds__(1024) void k_sl_edge_scan(const int* __restrict__ wg_tot, int n, int* __restrict__ offs)
{
    wg_scan_totals(wg_tot, n, offs);
}

// grid as k_sl_edge_count.  Nothing is written at or past the capacity.
__global__ __launch_bounds__(256) void k_sl_edge_write(const unsigned char* __restrict__ listed, int N, int flags, const int* __restrict__ offs,
                                                       psx_view_edge* __restrict__ edges, int capacity, int* __restrict__ total)
{
    int a = 0, b = 0;
    const bool keep = sl_edge(listed, N, flags, &a, &b);
    const unsigned long long m = __ballot(keep);
    __shared__ int s_cnt[4];
    wg_count(m, s_cnt);
    const int slot = offs[blockIdx.x] + wg_offset(m, s_cnt);
    if (keep && slot < capacity) edges[slot] = psx_view_edge{a, b};
    if (blockIdx.x == 0 && threadIdx.x == 0) *total = offs[gridDim.x];
}

bool aligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
size_t pad16(size_t b) { return (b + 15) & ~(size_t)15; }

bool sets_aligned(const unsigned char* const* d_sets, const int* lens, int n_sets)
{
    for (int v = 0; v < n_sets; v++)
        if (lens[v] > 0 && !aligned(d_sets[v], 16)) return false;
    return true;
}

// What training and the bags share: the views' table goes up, the rows are gathered and their norms taken.  The pinned
// buffer holds the table from pin_at on; every scratch buffer named here is sized before the first launch.
struct BowRows { const unsigned char* rows; const int* xn; const int* off; };

size_t bow_tables_bytes(int n_sets) { return pad16(8 * (size_t)n_sets) + pad16(4 * ((size_t)n_sets + 1)); }

bool bow_rows_need(MatchScratch& sc, int n_sets, int M)
{
    return sc.need(MS_BOW_TABLES, bow_tables_bytes(n_sets)) && sc.need(MS_BOW_ROWS, (size_t)M * PSX_BOW_DIM) &&
           sc.need(MS_BOW_NORMS, 4 * ((size_t)u8_pad(M) + (size_t)u8_pad(PSX_BOW_MAX_WORDS)));
}

bool bow_rows_queue(MatchScratch& sc, const unsigned char* const* d_sets, const int* lens, int n_sets, int M, char* pin, BowRows* out)
{
    const size_t ptr_b = pad16(8 * (size_t)n_sets);
    const unsigned char** hp = reinterpret_cast<const unsigned char**>(pin);
    for (int v = 0; v < n_sets; v++) hp[v] = d_sets[v];
    psx_bow_offsets(lens, n_sets, reinterpret_cast<int*>(pin + ptr_b));
    char* d_tab = static_cast<char*>(sc.buf[MS_BOW_TABLES]);
    if (hipMemcpyAsync(d_tab, pin, bow_tables_bytes(n_sets), hipMemcpyHostToDevice, sc.stream) != hipSuccess) return false;
    out->rows = static_cast<const unsigned char*>(sc.buf[MS_BOW_ROWS]);
    out->xn = static_cast<const int*>(sc.buf[MS_BOW_NORMS]);
    out->off = reinterpret_cast<const int*>(d_tab + ptr_b);
    hipLaunchKernelGGL(k_bow_gather, dim3((unsigned)(((size_t)M * 8 + 255) / 256)), dim3(256), 0, sc.stream,
                       reinterpret_cast<const unsigned char* const*>(d_tab), out->off, n_sets, M, static_cast<uint4*>(sc.buf[MS_BOW_ROWS]));
    hipLaunchKernelGGL(k_bow_norms, dim3((unsigned)(((size_t)u8_pad(M) * 8 + 255) / 256)), dim3(256), 0, sc.stream, out->rows, M,
                       static_cast<int*>(sc.buf[MS_BOW_NORMS]));
    return true;
}

// the words' norms lie behind the rows'
int* bow_word_norms(MatchScratch& sc, int M) { return static_cast<int*>(sc.buf[MS_BOW_NORMS]) + u8_pad(M); }

void bow_word_norms_queue(MatchScratch& sc, const unsigned char* d_vocab, int W, int M)
{
    hipLaunchKernelGGL(k_bow_norms, dim3((unsigned)(((size_t)u8_pad(W) * 8 + 255) / 256)), dim3(256), 0, sc.stream, d_vocab, W, bow_word_norms(sc, M));
}

// vocab: host memory (host_out) or device memory
int vocab_train(int device, const unsigned char* const* d_sets, const int* lens, int n_sets, const psx_vocab_opts* opts, bool host_out,
                unsigned char* vocab, psx_vocab_info* info)
{
    long long rows = 0;
    if (!psx_vocab_args_ok(d_sets, lens, n_sets, opts, vocab, info, &rows) || !sets_aligned(d_sets, lens, n_sets)) return PSX_ERR_INVALID;
    if (!host_out && !aligned(vocab, 16)) return PSX_ERR_INVALID;
    const int M = (int)rows, W = opts->words;                  // 2 <= W <= M: there is always work
    if (hipSetDevice(device) != hipSuccess) return PSX_ERR_HIP;
    MatchScratch& sc = psx_match_scratch();
    if (!sc.bind(device)) return PSX_ERR_HIP;
    hipStream_t st = sc.stream;
    // the head behind the sums is 16-byte aligned: its inertia takes a 64-bit atomic
    const size_t vocab_b = (size_t)W * PSX_BOW_DIM, sums_b = pad16(4 * (size_t)W * (PSX_BOW_DIM + 1)), pin_tab = 16,
                 pin_vocab = pin_tab + bow_tables_bytes(n_sets);
    // every buffer before the first launch: nothing is reallocated under queued work
    if (!bow_rows_need(sc, n_sets, M) || !sc.need(MS_BOW_ASSIGN, 2 * 4 * (size_t)M) || !sc.need(MS_BOW_SUMS, sums_b + sizeof(BowHead)) ||
        (host_out && !sc.need(MS_BOW_VOCAB, vocab_b)) || !sc.need_pinned(pin_vocab + (host_out ? vocab_b : 0)))
        return PSX_ERR_NOMEM;
    char* hpin = static_cast<char*>(sc.hpin);
    BowRows br;
    if (!bow_rows_queue(sc, d_sets, lens, n_sets, M, hpin + pin_tab, &br)) return PSX_ERR_HIP;
    unsigned char* d_vocab = host_out ? static_cast<unsigned char*>(sc.buf[MS_BOW_VOCAB]) : vocab;
    int* cur = static_cast<int*>(sc.buf[MS_BOW_ASSIGN]);
    int* prev = cur + (size_t)M;
    unsigned* d_cnt = static_cast<unsigned*>(sc.buf[MS_BOW_SUMS]);
    unsigned* d_sum = d_cnt + (size_t)W;
    BowHead* d_head = reinterpret_cast<BowHead*>(static_cast<char*>(sc.buf[MS_BOW_SUMS]) + sums_b);
    const BowHead* hh = reinterpret_cast<const BowHead*>(hpin);
    hipLaunchKernelGGL(k_bow_init, dim3((unsigned)((8 * W + 255) / 256)), dim3(256), 0, st, reinterpret_cast<const uint4*>(br.rows), M, W,
                       reinterpret_cast<uint4*>(d_vocab));
    if (hipMemsetAsync(prev, 0xff, 4 * (size_t)M, st) != hipSuccess) return PSX_ERR_HIP;     // no row has a word yet: -1
    psx_vocab_info t = {0, 0, 0, 0, 0ULL};
    for (int it = 1; it <= opts->iterations; it++) {
        if (hipMemsetAsync(d_cnt, 0, sums_b + sizeof(BowHead), st) != hipSuccess) return PSX_ERR_HIP;
        bow_word_norms_queue(sc, d_vocab, W, M);
        hipLaunchKernelGGL(k_bow_assign, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, st, br.rows, br.xn, M, d_vocab, bow_word_norms(sc, M), W,
                           cur, prev, d_head);
        hipLaunchKernelGGL(k_bow_accum, dim3((unsigned)(((size_t)M * 32 + 255) / 256)), dim3(256), 0, st, reinterpret_cast<const unsigned*>(br.rows),
                           cur, M, d_cnt, d_sum);
        hipLaunchKernelGGL(k_bow_update, dim3((unsigned)((PSX_BOW_DIM * W + 255) / 256)), dim3(256), 0, st, d_vocab, d_cnt, d_sum, W, d_head);
        if (hipGetLastError() != hipSuccess) return PSX_ERR_HIP;
        if (hipMemcpyAsync(hpin, d_head, sizeof(BowHead), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
            return PSX_ERR_HIP;
        if (hh->changed < 0 || hh->changed > M || hh->empty < 0 || hh->empty >= W) return PSX_ERR_HIP;
        t = psx_vocab_info{it, hh->changed, hh->empty, 0, hh->inertia};
        int* s = cur; cur = prev; prev = s;
        if (t.changed == 0) break;
    }
    if (host_out) {
        if (hipMemcpyAsync(hpin + pin_vocab, d_vocab, vocab_b, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
            return PSX_ERR_HIP;
        memcpy(vocab, hpin + pin_vocab, vocab_b);
    }
    *info = t;
    return PSX_OK;
}

// vocab / hist / words_out: all host memory (host_out) or all device memory
int bow_run(int device, const unsigned char* vocab, int W, const unsigned char* const* d_sets, const int* lens, int n_sets, bool host_out,
            unsigned* hist, int* words_out)
{
    long long rows = 0;
    if (!psx_bow_args_ok(vocab, W, d_sets, lens, n_sets, hist, &rows) || !sets_aligned(d_sets, lens, n_sets)) return PSX_ERR_INVALID;
    if (!host_out && (!aligned(vocab, 16) || !aligned(hist, 4) || !aligned(words_out, 4))) return PSX_ERR_INVALID;
    const size_t hist_b = 4 * (size_t)n_sets * (size_t)W;
    if (n_sets == 0 || rows == 0) {
        if (host_out && n_sets > 0) memset(hist, 0, hist_b);
        return PSX_OK;
    }
    const int M = (int)rows;
    if (hipSetDevice(device) != hipSuccess) return PSX_ERR_HIP;
    MatchScratch& sc = psx_match_scratch();
    if (!sc.bind(device)) return PSX_ERR_HIP;
    hipStream_t st = sc.stream;
    const size_t vocab_b = (size_t)W * PSX_BOW_DIM, words_b = 4 * (size_t)M;
    const size_t pin_tab = 0, pin_vocab = pin_tab + bow_tables_bytes(n_sets), pin_hist = pin_vocab + (host_out ? pad16(vocab_b) : 0),
                 pin_words = pin_hist + (host_out ? pad16(hist_b) : 0), pin_b = pin_words + (host_out && words_out ? words_b : 0);
    const bool own_words = host_out || words_out == nullptr;   // the rows' words go to scratch
    if (!bow_rows_need(sc, n_sets, M) || (own_words && !sc.need(MS_BOW_ASSIGN, words_b)) || (host_out && !sc.need(MS_BOW_VOCAB, vocab_b)) ||
        (host_out && !sc.need(MS_BOW_OUT, hist_b)) || !sc.need_pinned(pin_b))
        return PSX_ERR_NOMEM;
    char* hpin = static_cast<char*>(sc.hpin);
    BowRows br;
    if (!bow_rows_queue(sc, d_sets, lens, n_sets, M, hpin + pin_tab, &br)) return PSX_ERR_HIP;
    const unsigned char* d_vocab = vocab;
    if (host_out) {
        memcpy(hpin + pin_vocab, vocab, vocab_b);
        if (hipMemcpyAsync(sc.buf[MS_BOW_VOCAB], hpin + pin_vocab, vocab_b, hipMemcpyHostToDevice, st) != hipSuccess) return PSX_ERR_HIP;
        d_vocab = static_cast<const unsigned char*>(sc.buf[MS_BOW_VOCAB]);
    }
    unsigned* d_hist = host_out ? static_cast<unsigned*>(sc.buf[MS_BOW_OUT]) : hist;
    int* d_words = own_words ? static_cast<int*>(sc.buf[MS_BOW_ASSIGN]) : words_out;
    bow_word_norms_queue(sc, d_vocab, W, M);
    hipLaunchKernelGGL(k_bow_assign, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, st, br.rows, br.xn, M, d_vocab, bow_word_norms(sc, M), W, d_words,
                       static_cast<const int*>(nullptr), static_cast<BowHead*>(nullptr));
    if (hipMemsetAsync(d_hist, 0, hist_b, st) != hipSuccess) return PSX_ERR_HIP;
    hipLaunchKernelGGL(k_bow_hist, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, st, d_words, br.off, n_sets, M, W, d_hist);
    if (hipGetLastError() != hipSuccess) return PSX_ERR_HIP;
    if (host_out) {
        if (hipMemcpyAsync(hpin + pin_hist, d_hist, hist_b, hipMemcpyDeviceToHost, st) != hipSuccess) return PSX_ERR_HIP;
        if (words_out && hipMemcpyAsync(hpin + pin_words, d_words, words_b, hipMemcpyDeviceToHost, st) != hipSuccess) return PSX_ERR_HIP;
    }
    if (hipStreamSynchronize(st) != hipSuccess) return PSX_ERR_HIP;
    if (host_out) {
        memcpy(hist, hpin + pin_hist, hist_b);
        if (words_out) memcpy(words_out, hpin + pin_words, words_b);
    }
    return PSX_OK;
}

// hist and the outputs: all host memory (host_out) or all device memory
int shortlist_run(int device, const unsigned* hist, int N, int W, const psx_shortlist_opts* opts, bool host_out, int* nb, unsigned* scores,
                  psx_view_edge* edges, int capacity, int* count)
{
    if (!psx_shortlist_args_ok(hist, N, W, opts, edges, capacity, count)) return PSX_ERR_INVALID;
    if (!host_out && (!aligned(hist, 4) || !aligned(nb, 4) || !aligned(scores, 4) || !aligned(edges, 8))) return PSX_ERR_INVALID;
    if (N == 0) { *count = 0; return PSX_OK; }
    const int k = opts->k, kk = k < N - 1 ? k : N - 1;
    const size_t NN = (size_t)N * (size_t)N, hist_b = 4 * (size_t)N * (size_t)W, list_b = 4 * (size_t)N * (size_t)k;
    const size_t most = (size_t)N * (size_t)kk < NN / 2 ? (size_t)N * (size_t)kk : NN / 2;           // edges that can exist
    const int h_cap = (size_t)capacity < most ? capacity : (int)most;
    const int nwg = (int)((NN + 255) / 256);
    const size_t w_b = pad16(4 * (size_t)W);
    // the host form's outputs on the device and in the pinned buffer: neighbours, scores, edges
    const size_t out_nb = 0, out_sc = out_nb + (host_out && nb ? pad16(list_b) : 0), out_ed = out_sc + (host_out && scores ? pad16(list_b) : 0),
                 out_b = out_ed + (host_out && edges ? 8 * (size_t)h_cap : 0);
    const size_t pin_total = 0, pin_w = 16, pin_hist = pin_w + w_b, pin_out = pin_hist + (host_out ? pad16(hist_b) : 0);
    if (hipSetDevice(device) != hipSuccess) return PSX_ERR_HIP;
    MatchScratch& sc = psx_match_scratch();
    if (!sc.bind(device)) return PSX_ERR_HIP;
    hipStream_t st = sc.stream;
    // every buffer before the first launch: nothing is reallocated under queued work
    if ((host_out && !sc.need(MS_SL_HIST, hist_b)) || !sc.need(MS_SL_Q, 2 * w_b + 2 * (size_t)N * (size_t)W) || !sc.need(MS_SL_SCORE, 4 * NN) ||
        !sc.need(MS_SL_LISTED, NN) || !sc.need(MS_SL_TOT, 4 * (2 * (size_t)nwg + 2)) || (out_b > 0 && !sc.need(MS_SL_OUT, out_b)) ||
        !sc.need_pinned(pin_out + out_b))
        return PSX_ERR_NOMEM;
    char* hpin = static_cast<char*>(sc.hpin);
    const unsigned* d_hist = hist;
    if (host_out) {
        memcpy(hpin + pin_hist, hist, hist_b);
        if (hipMemcpyAsync(sc.buf[MS_SL_HIST], hpin + pin_hist, hist_b, hipMemcpyHostToDevice, st) != hipSuccess) return PSX_ERR_HIP;
        d_hist = static_cast<const unsigned*>(sc.buf[MS_SL_HIST]);
    }
    int* d_df = static_cast<int*>(sc.buf[MS_SL_Q]);
    int* d_weight = reinterpret_cast<int*>(static_cast<char*>(sc.buf[MS_SL_Q]) + w_b);
    unsigned short* d_q = reinterpret_cast<unsigned short*>(static_cast<char*>(sc.buf[MS_SL_Q]) + 2 * w_b);
    unsigned* d_score = static_cast<unsigned*>(sc.buf[MS_SL_SCORE]);
    unsigned char* d_listed = static_cast<unsigned char*>(sc.buf[MS_SL_LISTED]);
    int* d_tot = static_cast<int*>(sc.buf[MS_SL_TOT]);
    int* d_offs = d_tot + (size_t)nwg;
    int* d_total = d_offs + (size_t)nwg + 1;
    char* d_out = static_cast<char*>(sc.buf[MS_SL_OUT]);
    int* d_nb = host_out ? (nb ? reinterpret_cast<int*>(d_out + out_nb) : nullptr) : nb;
    unsigned* d_sc = host_out ? (scores ? reinterpret_cast<unsigned*>(d_out + out_sc) : nullptr) : scores;
    psx_view_edge* d_edges = host_out ? (edges ? reinterpret_cast<psx_view_edge*>(d_out + out_ed) : nullptr) : edges;
    const int cap = host_out ? (edges ? h_cap : 0) : capacity;

    if (hipMemsetAsync(d_df, 0, 4 * (size_t)W, st) != hipSuccess) return PSX_ERR_HIP;
    hipLaunchKernelGGL(k_sl_quant, dim3((unsigned)N), dim3(256), 0, st, d_hist, W, d_q, d_df);
    if (hipGetLastError() != hipSuccess) return PSX_ERR_HIP;
    if (hipMemcpyAsync(hpin + pin_w, d_df, 4 * (size_t)W, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
        return PSX_ERR_HIP;
    // the one logarithm of the step, on the host, in place: df comes down, the weights go up
    int* hw = reinterpret_cast<int*>(hpin + pin_w);
    if (psx_bow_weights_host(hw, W, N, hw) != PSX_OK) return PSX_ERR_HIP;
    if (hipMemcpyAsync(d_weight, hw, 4 * (size_t)W, hipMemcpyHostToDevice, st) != hipSuccess) return PSX_ERR_HIP;
    const unsigned T = (unsigned)((N + SL_TILE - 1) / SL_TILE);
    hipLaunchKernelGGL(k_sl_score, dim3(T, T), dim3(256), 0, st, d_q, d_weight, N, W, d_score);
    if (hipMemsetAsync(d_listed, 0, NN, st) != hipSuccess) return PSX_ERR_HIP;
    hipLaunchKernelGGL(k_sl_topk, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, st, d_score, N, k, kk, d_nb, d_sc, d_listed);
    hipLaunchKernelGGL(k_sl_edge_count, dim3((unsigned)nwg), dim3(256), 0, st, d_listed, N, opts->flags, d_tot);
    hipLaunchKernelGGL(k_sl_edge_scan, dim3(1), dim3(1024), 0, st, d_tot, nwg, d_offs);
    hipLaunchKernelGGL(k_sl_edge_write, dim3((unsigned)nwg), dim3(256), 0, st, d_listed, N, opts->flags, d_offs, d_edges, cap, d_total);
    if (hipGetLastError() != hipSuccess) return PSX_ERR_HIP;
    if (out_b > 0 && hipMemcpyAsync(hpin + pin_out, d_out, out_b, hipMemcpyDeviceToHost, st) != hipSuccess) return PSX_ERR_HIP;
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

extern "C" int psx_vocab_train_u8(int device, const unsigned char* const* d_sets, const int* lens, int n_sets, const psx_vocab_opts* opts,
                                  unsigned char* host_vocab, psx_vocab_info* info)
{
    return vocab_train(device, d_sets, lens, n_sets, opts, true, host_vocab, info);
}

extern "C" int psx_vocab_train_u8_dev(int device, const unsigned char* const* d_sets, const int* lens, int n_sets, const psx_vocab_opts* opts,
                                      unsigned char* d_vocab, psx_vocab_info* info)
{
    return vocab_train(device, d_sets, lens, n_sets, opts, false, d_vocab, info);
}

extern "C" int psx_vocab_train_u8_ref(const unsigned char* const* sets, const int* lens, int n_sets, const psx_vocab_opts* opts,
                                      unsigned char* vocab, psx_vocab_info* info)
{
    return psx_vocab_train_host(sets, lens, n_sets, opts, vocab, info);
}

extern "C" int psx_bow_u8(int device, const unsigned char* host_vocab, int words, const unsigned char* const* d_sets, const int* lens, int n_sets,
                          unsigned* host_hist, int* host_words_out)
{
    return bow_run(device, host_vocab, words, d_sets, lens, n_sets, true, host_hist, host_words_out);
}

extern "C" int psx_bow_u8_dev(int device, const unsigned char* d_vocab, int words, const unsigned char* const* d_sets, const int* lens, int n_sets,
                              unsigned* d_hist, int* d_words_out)
{
    return bow_run(device, d_vocab, words, d_sets, lens, n_sets, false, d_hist, d_words_out);
}

extern "C" int psx_bow_u8_ref(const unsigned char* vocab, int words, const unsigned char* const* sets, const int* lens, int n_sets,
                              unsigned* hist, int* words_out)
{
    return psx_bow_host(vocab, words, sets, lens, n_sets, hist, words_out);
}

extern "C" int psx_shortlist_views(int device, const unsigned* host_hist, int n_views, int words, const psx_shortlist_opts* opts,
                                   int* host_neighbours, unsigned* host_scores, psx_view_edge* host_edges, int edge_capacity, int* edge_count)
{
    return shortlist_run(device, host_hist, n_views, words, opts, true, host_neighbours, host_scores, host_edges, edge_capacity, edge_count);
}

extern "C" int psx_shortlist_views_dev(int device, const unsigned* d_hist, int n_views, int words, const psx_shortlist_opts* opts,
                                       int* d_neighbours, unsigned* d_scores, psx_view_edge* d_edges, int edge_capacity, int* edge_count)
{
    return shortlist_run(device, d_hist, n_views, words, opts, false, d_neighbours, d_scores, d_edges, edge_capacity, edge_count);
}

extern "C" int psx_shortlist_views_ref(const unsigned* hist, int n_views, int words, const psx_shortlist_opts* opts, int* neighbours,
                                       unsigned* scores, psx_view_edge* edges, int edge_capacity, int* edge_count)
{
    return psx_shortlist_host(hist, n_views, words, opts, neighbours, scores, edges, edge_capacity, edge_count);
}

extern "C" int psx_bow_weights(const int* df, int words, int n_views, int* out)
{
    return psx_bow_weights_host(df, words, n_views, out);
}
