// match_many_f32.hip -- one FLOAT descriptor set against many in one call: psx_match_pairs_many (+ _dev),
// psx_match_many_f32_plan, psx_match_many_f32_last.
//
// The contract is psx_match_pairs_many_u8's (match_many.hip) with psx_match_pairs (match.hip) as the single call: the
// result is, bit for bit, the concatenation of the K lists the single call returns.  The float matcher's result is the
// reference's scan -- its operation tree, (distance, index) order, strict '<' -- and that order is total, so the result
// does not depend on where the inner side is cut or on which path evaluates it.  Both paths are driven by the tables of
// match_many_f32_plan.h, in which no chunk and no block crosses a set boundary; forward the outer side is L and the inner
// side the K right sets, backward (PSX_PAIRS_MUTUAL only) the outer side is the K right sets and the inner side is L.
//
// PATH A, the exact scan (k_match_permute / k_match_partial / k_match_merge of match.hip over tables; every input the
// prefilter does not take, and the fallback):
//   k_f32_many_permute   the permuted copy (perm_src) of every inner row of all sets, gathered into one array
//   k_f32_many_partial   workgroup = (outer block, inner chunk): one lane per outer row, the chunk's rows as wave-uniform
//                        operands of l2_tree; the top-2 of the chunk per outer row
//   k_f32_many_merge     per (outer row, inner set) the set's chunks in index order with strict '<': the directed result
// PATH B, the MFMA prefilter over all sets (k_match_norms / k_match_cvt / k_match_mfma<false> / k_match_exact over tables):
//   k_f32_many_norms     the squared norm of every row of all K + 1 sets and the largest one per block
//   k_f32_many_cvt       ONE parameter set per call -- Rmax over all right rows forward, over L backward, M over everything,
//                        match_scale's rule -- and the scaled f16 copy of every row, gathered into one array
//   k_f32_many_mfma      workgroup = (outer block of 256 rows, inner chunk of ONE set): s(l, r) by v_mfma_f32_32x32x16_f16,
//                        running maxima per (outer row, chunk) seeded from the chunk's first rows, candidates appended to
//                        a segment that is private to one lane
//   k_f32_many_exact     one wave per (outer row, inner set), half a wave per candidate: the reference's operation tree
//                        on the candidates of the set's chunks, top2_insert_lex
// then, on either path, the segmented join of match_many_join.h.
//
// Why path B returns path A's result (the proof of match.hip, above its k_match_mfma, restated for one set of a call):
// |s - d| <= E_l holds for any Rmax >= the norm of every row ranked against l and any M >= every norm involved, so one
// parameter set per call is valid.  For a pair (outer row l, inner set S):
//   1. the second-smallest s seen SO FAR -- over the rows of one chunk of S that have entered the running maxima, each
//      once -- is >= the final second-smallest s2 of l over S: it is the second smallest of a subset;
//   2. the true second-best distance is <= s2 + E_l, and every pair with d <= that has s <= s2 + 2 E_l: the set
//      {r in S : s <= s2 + 2 E_l} contains every pair that can be best or second best, INCLUDING all ties; a test against
//      a running value that is >= s2 keeps a superset of it;
//   3. the exact evaluation of that set in (distance, index) order (top2_insert_lex) equals the scan of S.
// Rows past a chunk's end carry -inf and are never candidates; row reads are clamped to the set's own last row and idle
// outer columns repeat the last row of their own set: nothing of a neighbouring set is ever ranked.
//
// The unseeded start.  The single call seeds every chunk's running maxima from a pass over the first 2048 right rows;
// here every (outer row, chunk of one set) starts fresh.  Measured on planted random content (tests/match_many_f32_cases.py,
// 512-row chunks), starting empty and updating before the first test: 10.5 candidates per segment on average, the
// fullest 28 to 33 of 32 -- calls fell back.  So every workgroup seeds ITSELF: phase 0 runs the tile loop over its chunk's
// first 128 rows (two staged blocks) without a test, every value entering the maxima, and the two half waves merge theirs;
// phase 1 walks the whole chunk -- those rows again -- against that threshold, and behind the seeded rows the maxima
// take the largest value of both half waves per tile (one shuffle per column; the seeded rows must not enter twice).
// The same content then leaves 1.9 candidates per segment, the fullest 10 (a host restatement of the test; the device's
// figures per shape: profiles/match_many_f32_ms.txt).  The price is 128 more rows of MFMA per chunk, and chunks are
// long (>= 512 rows unless the set is shorter, match_many_f32_plan.h).
//
// The flag.  Path B queues everything without reading the flag -- norms, conversion, prefilter, exact evaluation, join,
// and a 4-byte copy of the flag behind them -- and synchronises ONCE.  k_f32_many_exact always leaves a directed result
// whose indices lie inside the inner set (from whatever candidates there are), so the join behind it never reads out
// of bounds; when the flag comes back up (a segment overflowed, or match_scale refused the norms) that output is
// discarded and path A runs for the whole call on the same stream, with a second synchronisation.  Nothing is carried
// from call to call: every count the exact evaluation reads was written by this call's prefilter, and the blocks' maxima
// are written, not accumulated -- there is no counter to zero and no "tidy" state.
//
// Launches per call, whatever K is (one group): path A 1 + 2 per direction + 3 = 8 kernels with the cross-check, 6 without;
// path B 2 + 2 per direction + 3 = 9 / 7; the table copy in front and one synchronisation.  Every further group of whole
// sets (match_many_f32_plan.h: the growing buffer above 256 MiB) adds 2 launches and no synchronisation.
#include "psx_internal.h"
#include "match_f32_core.h"
#include "match_f32_many_core.h"
#include "match_join.h"
#include "match_many_f32_plan.h"
#include "match_many_join.h"
#include "match_scratch.h"

#include <climits>
#include <cstdio>
#include <cstring>
#include <vector>

namespace {

static_assert(PSX_MANYF_SEGCAP == MF_SEGCAP && PSX_MANYF_PRE_STEP == MF_SUB * MF_TILE && PSX_MANYF_SCAN_UNIT == sizeof(Top2),
              "match_many_f32_plan.h sizes what the kernels here use");

// one entry per set: 0 .. K-1 the right sets, K the left set
struct FSet {
    const float* desc;           // the set's descriptors
    int len;                     // rows
    int foff;                    // its first row in the gathered arrays (permuted copy; f16 copy and norms)
    int roff;                    // its first row among the rows of its side (the right sets: prefix sum of the lengths; L: 0)
    int c0, c1;                  // its chunks in the chunk table
    int pad[5];
};
static_assert(sizeof(FSet) == 48, "three 16-byte scalar loads per entry");

// which part of the tables a launch walks, and where its rows lie in the partials / candidate segments
struct FPass {
    int nblocks, block_base;     // outer blocks [block_base, block_base + nblocks)
    int chunk_base, nchunks;     // inner chunks [chunk_base, chunk_base + nchunks)
    int row_base, outer_rows;    // the launch's outer rows [row_base, row_base + outer_rows) of the outer side
};

// ---- path A --------------------------------------------------------------------------------------------------------

// grid: the blocks of the inner sides, 256 threads: k_match_permute's layout for the block's rows, at the set's place
__global__ __launch_bounds__(256) void k_f32_many_permute(const FSet* __restrict__ sets, const int2* __restrict__ blocks, float* __restrict__ dst)
{
    const int2 blk = blocks[blockIdx.x];
    const FSet s = sets[blk.x];
    const int rows = min(PSX_MANY_BLOCK, s.len - blk.y);
    fm_permute_block(s.desc + (size_t)blk.y * 128, rows, reinterpret_cast<float2*>(dst + ((size_t)s.foff + blk.y) * 128));
}

// grid nblocks x nchunks, 256 threads; workgroup (ob, ch) = (blockIdx.x % nblocks, blockIdx.x / nblocks).  k_match_partial
// with both sides taken from tables: lane (64 w + j) owns outer row blk.row0 + 64 w + j of ITS block's set (original layout)
// and walks rows [r0, r1) of ITS chunk's set in the permuted copy (wave-uniform: scalar loads).
// partial[ch * outer_rows + (row among the launch's outer rows)] = top-2 within the chunk, indices within the set.
__global__ __launch_bounds__(256) void k_f32_many_partial(const FSet* __restrict__ sets, const int4* __restrict__ chunks,
                                                          const int2* __restrict__ blocks, const float* __restrict__ perm,
                                                          FPass ps, Top2* __restrict__ partial)
{
    const int ob = (int)(blockIdx.x % (unsigned)ps.nblocks), ch = (int)(blockIdx.x / (unsigned)ps.nblocks);
    const int2 blk = blocks[ps.block_base + ob];
    const int4 chk = chunks[ps.chunk_base + ch];
    const FSet os = sets[blk.x], is = sets[chk.x];
    const int row0 = blk.y + (int)(threadIdx.x >> 6) * 64;
    if (row0 >= os.len) return;                                // a wave without rows (wave uniform; no barrier follows)
    const int row = row0 + (int)(threadIdx.x & 63);
    const int lq = min(row, os.len - 1);                       // idle lanes repeat the last row of their own set
    v2f l[64];
    {
        const float* lp = os.desc + (size_t)lq * 128;
#pragma unroll
        for (int k = 0; k < 64; k++) l[k] = (v2f){lp[perm_src(k, 0)], lp[perm_src(k, 1)]};
    }
    const float* rp = perm + (size_t)is.foff * 128;
    const int r1 = min(chk.z, is.len);
    Top2 t = {INFINITY, INFINITY, 0, 0};
    for (int i = chk.y; i < r1; i++) {
        const float d = l2_tree(l, rp + (size_t)i * 128);
        top2_insert(t, d, i);
    }
    if (row < os.len) partial[(size_t)ch * ps.outer_rows + (size_t)(os.roff - ps.row_base) + row] = t;
}

// grid nblocks x ngroups, 256 threads: one thread per (outer row of block ob, inner set group_base + g).  The set's chunks
// in table order = index order, merged as k_match_merge merges them.  The result goes where the join expects the directed
// result of (outer set, inner set): at out + out_stride * (inner set) + 5 * (outer set's first row); out_stride = 5 l_len
// forward (K results per left row), 0 backward (the one inner set is L).
__global__ __launch_bounds__(256) void k_f32_many_merge(const FSet* __restrict__ sets, const int2* __restrict__ blocks, FPass ps,
                                                        int group_base, size_t out_stride, const Top2* __restrict__ partial,
                                                        int* __restrict__ out)
{
    const int ob = (int)(blockIdx.x % (unsigned)ps.nblocks), g = group_base + (int)(blockIdx.x / (unsigned)ps.nblocks);
    const int2 blk = blocks[ps.block_base + ob];
    const FSet os = sets[blk.x], is = sets[g];
    const int row = blk.y + (int)threadIdx.x;
    if (row >= os.len || is.len == 0) return;
    const size_t prow = (size_t)(os.roff - ps.row_base) + row;
    Top2 t = {INFINITY, INFINITY, 0, 0};
    // chunks are visited in index order and a chunk's own entries are already in (distance, index) order, so strict '<'
    // insertion reproduces the sequential scan: ties keep the smaller index
    for (int c = is.c0; c < is.c1; c++) {
        const Top2 p = partial[(size_t)(c - ps.chunk_base) * ps.outer_rows + prow];
        top2_insert(t, p.d1, p.i1);
        top2_insert(t, p.d2, p.i2);
    }
    psx_directed_store<float>(out + out_stride * (size_t)g + 5 * (size_t)os.roff, os.len, (size_t)row, t.i1, t.i2, t.d1 / t.d2 < 0.8f, t.d1, t.d2);
}

// ---- path B --------------------------------------------------------------------------------------------------------

// (the parameters par[], FX_SEGS, FM_SEEDBLK and the device pieces of this path: match_f32_many_core.h)

// grid: every block of both sides, 256 threads, 32 lanes per row (k_match_norms' sum): norm2[foff + row] and the block's
// largest (bits of a non-negative float; a NaN norm has the bit pattern of a huge unsigned and wins)
__global__ __launch_bounds__(256) void k_f32_many_norms(const FSet* __restrict__ sets, const int2* __restrict__ blocks,
                                                        float* __restrict__ norm2, unsigned* __restrict__ bmax)
{
    const int2 blk = blocks[blockIdx.x];
    const FSet s = sets[blk.x];
    const int end = min(blk.y + PSX_MANY_BLOCK, s.len);
    fm_norms_block(s.desc, blk.y, end, norm2 + s.foff, bmax + blockIdx.x);
}

// grid as k_f32_many_norms; blocks [0, br) belong to the right sets, [br, br + bl) to L.  Every workgroup derives the
// parameters from the blocks' maxima itself (k_match_cvt: a 1-thread kernel in between costs a launch); workgroup 0
// publishes them and the flag -- the call's first write of it.  Then the f16 copy of the block's rows, scaled by 2^k.
__global__ __launch_bounds__(256) void k_f32_many_cvt(const FSet* __restrict__ sets, const int2* __restrict__ blocks, int br, int bl,
                                                      const unsigned* __restrict__ bmax, unsigned short* __restrict__ h16,
                                                      float* __restrict__ par, int* __restrict__ flag)
{
    const float sc = fm_cvt_params(br, bl, bmax, par, flag);
    const int2 blk = blocks[blockIdx.x];
    const FSet s = sets[blk.x];
    const int rows = min(PSX_MANY_BLOCK, s.len - blk.y);
    fm_cvt_block(reinterpret_cast<const float4*>(s.desc + (size_t)blk.y * 128), rows, sc,
                 reinterpret_cast<ushort4*>(h16 + ((size_t)s.foff + blk.y) * 128));
}

// grid nblocks x nchunks, 256 threads; workgroup (ob, ch) as k_f32_many_partial.  The tile loop of k_match_mfma<false>
// (match.hip: operand layout, the staged 2 x 32-row blocks, the norm term as the accumulator's initial value, one maximum
// per tile column) with both sides taken from tables: wave w owns outer rows [row0 + 64 w, + 64) of ITS block's set as two B
// fragment sets and walks rows [r0, r1) of ITS chunk's set.  lh / rh: the sets' rows in the gathered f16 copy.
// The loop itself -- fm_prefilter_block and fm_walk, __builtin_amdgcn_mfma_f32_32x32x16_f16 -- is match_f32_many_core.h's.
// Segment of (outer row, chunk, half wave): cand[(((row among the launch's rows) * nchunks + ch) * 2 + half) * MF_SEGCAP + ...],
// its count in cand_ct at the same index without the last factor; indices within the inner set.
__global__ __launch_bounds__(256, 3) void k_f32_many_mfma(const FSet* __restrict__ sets, const int4* __restrict__ chunks,
                                                          const int2* __restrict__ blocks, const unsigned short* __restrict__ h16,
                                                          const float* __restrict__ n2, const float* __restrict__ par, int backward,
                                                          FPass ps, int* __restrict__ cand_ct, int* __restrict__ cand)
{
    __shared__ __attribute__((aligned(16))) unsigned char s_r[2][MF_SUB * MF_TILE * MF_ROW];
    __shared__ __attribute__((aligned(16))) float s_n[2][MF_SUB * MF_TILE];
    const int ob = (int)(blockIdx.x % (unsigned)ps.nblocks), ch = (int)(blockIdx.x / (unsigned)ps.nblocks);
    const int2 blk = blocks[ps.block_base + ob];
    const int4 chk = chunks[ps.chunk_base + ch];
    const FSet os = sets[blk.x], is = sets[chk.x];
    // Rmax: over the rows this direction ranks -- all right rows forward, L backward
    fm_prefilter_block(s_r, s_n, h16 + (size_t)os.foff * 128, n2 + os.foff, os.len, blk.y, h16 + (size_t)is.foff * 128, n2 + is.foff, is.len,
                       chk.y, min(chk.z, is.len), par[1], backward ? par[4] : par[2], par[3], cand_ct, cand, os.roff - ps.row_base, ps.nchunks, ch);
}

// grid nblocks x 64 x ngroups, 256 threads: wave w of workgroup (ob, q, g) takes outer row blk.row0 + 4 q + w against inner
// set group_base + g.  k_match_exact's evaluation -- half a wave per candidate, lane t of a half takes floats 4t..4t+3,
// the shuffle_down tree 16, 8, 4, 2, 1: the tree of l2_tree -- over the candidates of the set's chunks, compacted into one
// list per wave in LDS.  The two halves take disjoint candidates and merge at the end; the (distance, index) order is
// total, so the order of evaluation does not matter.
// ALWAYS writes a result whose indices lie in the inner set (the join behind it reads it whatever the flag says); raises
// the flag for a segment that overflowed.  out / out_stride as k_f32_many_merge.
__global__ __launch_bounds__(256) void k_f32_many_exact(const FSet* __restrict__ sets, const int2* __restrict__ blocks, FPass ps,
                                                        int group_base, size_t out_stride, const int* __restrict__ cand_ct,
                                                        const int* __restrict__ cand, int* __restrict__ out, int* __restrict__ flag)
{
    const int ob = (int)(blockIdx.x % (unsigned)ps.nblocks);
    const unsigned rest = blockIdx.x / (unsigned)ps.nblocks;
    const int g = group_base + (int)(rest >> 6);
    const int2 blk = blocks[ps.block_base + ob];
    const FSet os = sets[blk.x], is = sets[g];
    const int lane = threadIdx.x & 63, tl = lane & 31;
    const int row = blk.y + (int)(rest & 63u) * 4 + (int)(threadIdx.x >> 6);
    if (row >= os.len || is.len == 0) return;                   // wave uniform
    const float4 l4 = reinterpret_cast<const float4*>(os.desc + (size_t)row * 128)[tl];
    const size_t prow = (size_t)(os.roff - ps.row_base) + row;
    // the set's segments -- two per chunk, contiguous for one outer row
    __shared__ int s_list[4][FX_SEGS * MF_SEGCAP];
    Top2 t;
    const bool over = fm_exact_row(l4, is.desc, cand_ct, cand, (prow * ps.nchunks + (size_t)(is.c0 - ps.chunk_base)) * 2, 2 * (is.c1 - is.c0),
                                   s_list[threadIdx.x >> 6], t);
    if (__ballot(over) != 0ull && lane == 0) *flag = 1;
    if (lane == 0) {
        // the reference starts from (inf, inf, index 0, index 0) and never replaces an entry by an equal one
        const int i1 = t.i1 == 0x7fffffff ? 0 : t.i1, i2 = t.i2 == 0x7fffffff ? 0 : t.i2;
        psx_directed_store<float>(out + out_stride * (size_t)g + 5 * (size_t)os.roff, os.len, (size_t)row, i1, i2, t.d1 / t.d2 < 0.8f, t.d1, t.d2);
    }
}

size_t pad16(size_t b) { return (b + 15) & ~(size_t)15; }

thread_local psx_many_f32_info t_info = {0, 0, 0, 0};

// host_pairs or d_pairs (the other is NULL; both NULL with capacity 0)
int match_pairs_many_f32(int device, const float* d_left, int l_len, const float* const* d_rights, const int* r_lens, int n_sets,
                         const psx_match_opts* opts, void* host_pairs, void* d_pairs, int capacity, int* set_counts, int* count)
{
    if (!psx_pairs_args_ok(l_len, 0, opts, host_pairs ? host_pairs : d_pairs, capacity, count) || (l_len > 0 && !d_left) ||
        n_sets < 0 || (n_sets > 0 && (!d_rights || !r_lens || !set_counts)) || !psx_many_sets_ok(l_len, r_lens, n_sets))
        return PSX_ERR_INVALID;
    long long r_total = 0;
    for (int k = 0; k < n_sets; k++) {
        if (r_lens[k] > 0 && !d_rights[k]) return PSX_ERR_INVALID;
        r_total += r_lens[k];
    }
    t_info = psx_many_f32_info{0, 0, 0, 0};
    if (l_len == 0 || r_total == 0) {
        for (int k = 0; k < n_sets; k++) set_counts[k] = 0;
        *count = 0;
        return PSX_OK;
    }
    const bool mutual = (opts->flags & PSX_PAIRS_MUTUAL) != 0;
    const int K = n_sets;
    if (r_total + l_len > INT_MAX) return PSX_ERR_NOMEM;             // a row's place in the gathered arrays is an int
    const long long T = r_total + l_len;

    if (hipSetDevice(device) != hipSuccess) return PSX_ERR_HIP;
    MatchScratch& sc = psx_match_scratch();
    if (!sc.bind(device)) return PSX_ERR_HIP;
    const int planned = psx_manyf_path(l_len, r_lens, K, sc.tune.match_mfma);
    t_info.path = planned;

    const long long nb = (l_len + 255) / 256, ntot = (long long)K * nb;          // the join's workgroups
    if (ntot + 1 > INT_MAX) return PSX_ERR_NOMEM;
    const long long all_pairs = (long long)K * l_len;                 // at most l_len pairs per set exist
    const size_t nrec = host_pairs ? (size_t)(capacity < all_pairs ? capacity : all_pairs) : 0;
    const size_t off_counts = 16, off_flag = off_counts + pad16(sizeof(int) * (size_t)K), off_rec = off_flag + 16, off_blob = off_rec + 16 * nrec;
    std::vector<long long> roff((size_t)K + 1, 0);
    for (int k = 0; k < K; k++) roff[(size_t)k + 1] = roff[(size_t)k] + r_lens[k];
    hipStream_t st = sc.stream;
    thread_local psx_manyf_tables tb;

    // one path over the whole call: tables, directed passes of every group, join, the flag; synchronised on return
    auto run = [&](int path, int* h_flag_out) -> int {
        if (!psx_many_f32_build(l_len, r_lens, K, mutual, path, tb)) return PSX_ERR_NOMEM;
        const long long BR = (long long)tb.rblk.size(), BL = (long long)tb.lblk.size();
        const long long CR = (long long)tb.rchk.size(), CL = (long long)tb.lchk.size();
        const size_t sets_b = pad16(sizeof(FSet) * ((size_t)K + 1));
        const size_t chunks_b = pad16(sizeof(int4) * (size_t)(CR + CL));
        const size_t blocks_b = pad16(sizeof(int2) * (size_t)(BR + BL));
        const size_t blob_b = sets_b + chunks_b + blocks_b;
        const size_t state_b = pad16(sizeof(unsigned) * (size_t)(BR + BL)) + sizeof(float) * FPAR + 16;
        // every buffer before the first launch: nothing is reallocated under queued work
        if (!sc.need(MS_MANYF_TABLES, blob_b) || !sc.need(MS_MANYF_STATE, state_b) ||
            !sc.need(MS_MANYF_FWD, sizeof(int) * 5 * (size_t)all_pairs) || (mutual && !sc.need(MS_MANYF_BWD, sizeof(int) * 5 * (size_t)r_total)) ||
            !sc.need(MS_MANYF_TOT, sizeof(int) * (2 * (size_t)ntot + 1)) || !sc.need_pinned(off_blob + blob_b))
            return PSX_ERR_NOMEM;
        if (path == 1) {
            if (!sc.need(MS_MANYF_PERM, sizeof(float) * 128 * (size_t)T) || !sc.need(MS_MANYF_PARTIAL, (size_t)tb.scratch_bytes)) return PSX_ERR_NOMEM;
        } else {
            const size_t segs = (size_t)(tb.scratch_bytes / PSX_MANYF_PRE_UNIT) * 2;
            if (!sc.need(MS_MANYF_F16, sizeof(unsigned short) * 128 * (size_t)T) || !sc.need(MS_MANYF_NORMS, sizeof(float) * (size_t)T) ||
                !sc.need(MS_MANYF_CAND_CT, sizeof(int) * segs) || !sc.need(MS_MANYF_CAND, sizeof(int) * MF_SEGCAP * segs))
                return PSX_ERR_NOMEM;
        }
        void* dev_pin = nullptr;
        if (hipHostGetDevicePointer(&dev_pin, sc.hpin, 0) != hipSuccess || dev_pin == nullptr) return PSX_ERR_HIP;
        char* hp = static_cast<char*>(sc.hpin);

        // ---- the tables, written into the pinned staging buffer and copied on the stream ----
        {
            FSet* hs = reinterpret_cast<FSet*>(hp + off_blob);
            int4* hc = reinterpret_cast<int4*>(hp + off_blob + sets_b);
            int2* hb = reinterpret_cast<int2*>(hp + off_blob + sets_b + chunks_b);
            for (int k = 0; k < K; k++) hs[k] = FSet{d_rights[k], r_lens[k], (int)roff[(size_t)k], (int)roff[(size_t)k], 0, 0, {0, 0, 0, 0, 0}};
            hs[K] = FSet{d_left, l_len, (int)r_total, 0, (int)CR, (int)(CR + CL), {0, 0, 0, 0, 0}};
            for (long long c = 0; c < CR; c++) {
                const psx_many_chunk& q = tb.rchk[(size_t)c];
                hc[c] = make_int4(q.set, q.r0, q.r1, 0);
                if (hs[q.set].c1 == 0) hs[q.set].c0 = (int)c;            // a set's chunks are contiguous: first and last + 1
                hs[q.set].c1 = (int)c + 1;
            }
            for (long long c = 0; c < CL; c++) hc[CR + c] = make_int4(K, tb.lchk[(size_t)c].r0, tb.lchk[(size_t)c].r1, 0);
            for (long long b = 0; b < BR; b++) hb[b] = make_int2(tb.rblk[(size_t)b].set, tb.rblk[(size_t)b].row0);
            for (long long b = 0; b < BL; b++) hb[BR + b] = make_int2(K, tb.lblk[(size_t)b].row0);
        }
        int* h_total = reinterpret_cast<int*>(hp);
        int* h_flag = reinterpret_cast<int*>(hp + off_flag);
        *h_total = -1;
        *h_flag = 0;
        const FSet* d_sets = static_cast<const FSet*>(sc.buf[MS_MANYF_TABLES]);
        const int4* d_chunks = reinterpret_cast<const int4*>(static_cast<const char*>(sc.buf[MS_MANYF_TABLES]) + sets_b);
        const int2* d_blocks = reinterpret_cast<const int2*>(static_cast<const char*>(sc.buf[MS_MANYF_TABLES]) + sets_b + chunks_b);
        unsigned* d_bmax = static_cast<unsigned*>(sc.buf[MS_MANYF_STATE]);
        float* d_par = reinterpret_cast<float*>(static_cast<char*>(sc.buf[MS_MANYF_STATE]) + pad16(sizeof(unsigned) * (size_t)(BR + BL)));
        int* d_flag = reinterpret_cast<int*>(d_par + FPAR);
        int* d_fwd = static_cast<int*>(sc.buf[MS_MANYF_FWD]);
        int* d_bwd = mutual ? static_cast<int*>(sc.buf[MS_MANYF_BWD]) : nullptr;
        int* d_tot = static_cast<int*>(sc.buf[MS_MANYF_TOT]);
        int* d_total = static_cast<int*>(dev_pin);
        int* d_counts = reinterpret_cast<int*>(static_cast<char*>(dev_pin) + off_counts);
        // the kernel's capacity for the host form is the staging buffer's (nrec <= capacity)
        int4* out = host_pairs ? reinterpret_cast<int4*>(static_cast<char*>(dev_pin) + off_rec) : static_cast<int4*>(d_pairs);
        const int cap = host_pairs ? (int)nrec : capacity;
        const bool stats = path == 2 && sc.tune.match_stats;            // measurement: candidates per (left, set), forward
        long long st_sum = 0, st_n = 0; int st_max = 0, st_seg = 0;

        if (hipMemcpyAsync(sc.buf[MS_MANYF_TABLES], hp + off_blob, blob_b, hipMemcpyHostToDevice, st) != hipSuccess) return PSX_ERR_HIP;
        if (path == 1) {
            Top2* d_partial = static_cast<Top2*>(sc.buf[MS_MANYF_PARTIAL]);
            float* d_perm = static_cast<float*>(sc.buf[MS_MANYF_PERM]);
            // the right sets are the forward direction's inner side, L the backward direction's
            hipLaunchKernelGGL(k_f32_many_permute, dim3((unsigned)(mutual ? BR + BL : BR)), dim3(256), 0, st, d_sets, d_blocks, d_perm);
            t_info.launches++;
            for (int dir = 0; dir < 2; dir++)
                for (const psx_manyf_group& g : (dir == 0 ? tb.fgroups : tb.bgroups)) {
                    const FPass ps = {g.nblocks, g.block0, g.chunk0, g.nchunks, g.row0, g.rows};
                    hipLaunchKernelGGL(k_f32_many_partial, dim3((unsigned)g.nblocks * (unsigned)g.nchunks), dim3(256), 0, st, d_sets, d_chunks,
                                       d_blocks, d_perm, ps, d_partial);
                    if (dir == 0)
                        hipLaunchKernelGGL(k_f32_many_merge, dim3((unsigned)g.nblocks * (unsigned)g.nsets), dim3(256), 0, st, d_sets, d_blocks, ps,
                                           g.set0, 5 * (size_t)l_len, d_partial, d_fwd);
                    else
                        hipLaunchKernelGGL(k_f32_many_merge, dim3((unsigned)g.nblocks), dim3(256), 0, st, d_sets, d_blocks, ps, K, (size_t)0,
                                           d_partial, d_bwd);
                    t_info.launches += 2;
                }
        } else {
            unsigned short* d_h16 = static_cast<unsigned short*>(sc.buf[MS_MANYF_F16]);
            float* d_n2 = static_cast<float*>(sc.buf[MS_MANYF_NORMS]);
            int* d_cct = static_cast<int*>(sc.buf[MS_MANYF_CAND_CT]);
            int* d_cand = static_cast<int*>(sc.buf[MS_MANYF_CAND]);
            hipLaunchKernelGGL(k_f32_many_norms, dim3((unsigned)(BR + BL)), dim3(256), 0, st, d_sets, d_blocks, d_n2, d_bmax);
            hipLaunchKernelGGL(k_f32_many_cvt, dim3((unsigned)(BR + BL)), dim3(256), 0, st, d_sets, d_blocks, (int)BR, (int)BL, d_bmax, d_h16,
                               d_par, d_flag);
            t_info.launches += 2;
            for (int dir = 0; dir < 2; dir++)
                for (const psx_manyf_group& g : (dir == 0 ? tb.fgroups : tb.bgroups)) {
                    const FPass ps = {g.nblocks, g.block0, g.chunk0, g.nchunks, g.row0, g.rows};
                    hipLaunchKernelGGL(k_f32_many_mfma, dim3((unsigned)g.nblocks * (unsigned)g.nchunks), dim3(256), 0, st, d_sets, d_chunks,
                                       d_blocks, d_h16, d_n2, d_par, dir, ps, d_cct, d_cand);
                    if (dir == 0)
                        hipLaunchKernelGGL(k_f32_many_exact, dim3((unsigned)g.nblocks * 64u * (unsigned)g.nsets), dim3(256), 0, st, d_sets, d_blocks,
                                           ps, g.set0, 5 * (size_t)l_len, d_cct, d_cand, d_fwd, d_flag);
                    else
                        hipLaunchKernelGGL(k_f32_many_exact, dim3((unsigned)g.nblocks * 64u), dim3(256), 0, st, d_sets, d_blocks, ps, K, (size_t)0,
                                           d_cct, d_cand, d_bwd, d_flag);
                    t_info.launches += 2;
                    if (stats && dir == 0) {
                        // POPSIFT_MATCH_STATS (measurement only): the group's counts are read back before the next group reuses them
                        std::vector<int> h((size_t)g.rows * g.nchunks * 2);
                        if (hipStreamSynchronize(st) != hipSuccess || hipMemcpy(h.data(), d_cct, sizeof(int) * h.size(), hipMemcpyDeviceToHost) != hipSuccess)
                            return PSX_ERR_HIP;
                        t_info.syncs++;
                        for (int i = 0; i < g.rows; i++) {
                            int c = g.chunk0;
                            while (c < g.chunk0 + g.nchunks) {
                                const int s = tb.rchk[(size_t)c].set;
                                int tsum = 0;
                                for (; c < g.chunk0 + g.nchunks && tb.rchk[(size_t)c].set == s; c++)
                                    for (int hh = 0; hh < 2; hh++) {
                                        const int v = h[((size_t)i * g.nchunks + (size_t)(c - g.chunk0)) * 2 + hh];
                                        tsum += v; if (v > st_seg) st_seg = v;
                                    }
                                st_sum += tsum; st_n++; if (tsum > st_max) st_max = tsum;
                            }
                        }
                    }
                }
        }
        psx_many_join_queue<float>(st, d_sets, d_fwd, l_len, d_bwd, (int)nb, (int)ntot, opts->ratio, mutual, d_tot, out, cap, d_counts, d_total);
        t_info.launches += 3;
        if (path == 2 && hipMemcpyAsync(h_flag, d_flag, sizeof(int), hipMemcpyDeviceToHost, st) != hipSuccess) return PSX_ERR_HIP;
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return PSX_ERR_HIP;
        t_info.syncs++;
        *h_flag_out = *h_flag;
        if (stats)
            fprintf(stderr, "psx_match_pairs_many prefilter: %d x %lld in %d sets, candidates per (left, set): mean %.1f, max %d; fullest segment %d of %d%s\n",
                    l_len, r_total, K, st_n ? (double)st_sum / (double)st_n : 0.0, st_max, st_seg, MF_SEGCAP, *h_flag ? " -> exact scan of every pair" : "");
        return PSX_OK;
    };

    int h_flag = 0;
    int rc = run(planned, &h_flag);
    if (rc != PSX_OK) return rc;
    if (planned == 2 && h_flag != 0) {
        // a segment overflowed or the norms are out of the margin's reach: the whole call again by the exact scan
        t_info.fell_back = 1;
        rc = run(1, &h_flag);
        if (rc != PSX_OK) return rc;
    }
    const char* hp = static_cast<const char*>(sc.hpin);
    const int n = *reinterpret_cast<const int*>(hp);
    if (n < 0 || n > all_pairs) return PSX_ERR_HIP;
    memcpy(set_counts, hp + off_counts, sizeof(int) * (size_t)K);
    if (host_pairs && n > 0 && nrec > 0) memcpy(host_pairs, hp + off_rec, 16 * ((size_t)n < nrec ? (size_t)n : nrec));
    *count = n;
    return PSX_OK;
}

} // namespace

extern "C" int psx_match_pairs_many(int device, const float* d_left, int l_len, const float* const* d_rights, const int* r_lens,
                                    int n_sets, const psx_match_opts* opts, psx_match_pair* host_pairs, int capacity,
                                    int* set_counts, int* count)
{
    return match_pairs_many_f32(device, d_left, l_len, d_rights, r_lens, n_sets, opts, host_pairs, nullptr, capacity, set_counts, count);
}

extern "C" int psx_match_pairs_many_dev(int device, const float* d_left, int l_len, const float* const* d_rights, const int* r_lens,
                                        int n_sets, const psx_match_opts* opts, psx_match_pair* d_pairs, int capacity,
                                        int* set_counts, int* count)
{
    return match_pairs_many_f32(device, d_left, l_len, d_rights, r_lens, n_sets, opts, nullptr, d_pairs, capacity, set_counts, count);
}

extern "C" int psx_match_many_f32_plan(int l_len, const int* r_lens, int n_sets, int flags, int mfma_enabled, psx_many_f32_plan* out)
{
    return psx_many_f32_plan_host(l_len, r_lens, n_sets, flags, mfma_enabled, out);
}

extern "C" int psx_match_many_f32_last(psx_many_f32_info* out)
{
    if (!out) return PSX_ERR_INVALID;
    *out = t_info;
    return PSX_OK;
}
