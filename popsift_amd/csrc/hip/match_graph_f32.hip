// match_graph_f32.hip -- a list of view pairs over N FLOAT descriptor sets in one call: psx_match_pairs_graph (+ _dev),
// psx_match_graph_f32_plan, psx_match_graph_f32_last.
//
// The contract is psx_match_pairs_graph_u8's (match_graph.hip) with psx_match_pairs (match.hip) as the single call: the
// result is, bit for bit, the concatenation in edge order of the lists the single call returns per edge.  The float
// matcher's result is the reference's scan -- its operation tree, (distance, index) order, strict '<' -- and that order is
// total, so the result does not depend on where a set is cut or on which path evaluates it.  The table shape is
// match_graph.hip's (match_graph_f32_plan.h): every referenced set is cut ONCE per call, a flat item table names per
// workgroup an outer block, an inner chunk, where its output goes and its edge, an {edge, row0} table drives the per-row
// kernels and the join, and groups are runs of whole edges under the budget of the one buffer that grows with
// (chunks x outer rows).  The two paths are match_many_f32.hip's, their device pieces the same text
// (match_f32_many_core.h); the kernels here only say where the operands live.
//
// PATH A, the exact scan (every input the prefilter does not take, and the fallback):
//   k_gf_permute   the permuted copy (perm_src) of every row of every referenced set, ONCE per call, gathered into one array
//   k_gf_partial   one workgroup per item: one lane per outer row, the chunk's rows as wave-uniform operands of l2_tree
//                  (k_match_partial's walk); the top-2 of the chunk per outer row at item.pbase + row
//   k_gf_merge     per (edge, outer row) the inner set's chunks in index order with strict '<': the directed result at the
//                  edge's row offset
// PATH B, the MFMA prefilter:
//   k_gf_norms     the squared norm of every row of every referenced set, once, and the largest one per block
//   k_gf_cvt       ONE parameter set per call -- Rmax and M over the rows of ALL referenced sets, the same Rmax for both
//                  directions -- and the scaled f16 copy of every row, once, gathered into one array
//   k_gf_mfma      one workgroup per item: the self-seeding two-phase tile loop of k_f32_many_mfma (fm_prefilter_block:
//                  fm_walk, v_mfma_f32_32x32x16_f16); candidates appended to segments private to one lane
//   k_gf_exact     one wave per (edge, outer row), half a wave per candidate: the reference's operation tree on the
//                  candidates of the inner set's chunks (fm_exact_row), top2_insert_lex
// then, on either path, the join segmented by edge (match_graph_join.h).
//
// Why path B returns path A's result.  The proof in match_many_f32.hip's header (match.hip's, above its k_match_mfma) bounds
// |s - d| <= E_l for ANY Rmax >= the norm of every row ranked against l and ANY M >= every norm involved, and needs nothing
// else of the two.  Here Rmax^2 = M^2 = the largest squared norm over the rows of all referenced sets: every row that any
// edge ranks, in either direction, is such a row, so the one parameter set is valid for every (outer row, inner set) of
// the call without further argument.  Steps 1-3 of that proof are then per (outer row l, inner set S) and hold per edge:
// the running second-smallest s of a chunk is >= the final one over S, {r in S : s <= s2 + 2 E_l} contains every row that
// can be best or second best INCLUDING all ties, and its exact evaluation in (distance, index) order equals the scan of S.
// Rows past a chunk's end carry -inf and are never candidates; row reads are clamped to the set's own last row and idle
// outer columns repeat the last row of their own set: nothing of a neighbouring set is ever ranked.
//
// The candidate segments are laid out so that fm_walk runs unchanged: the segments of one edge are contiguous, the segment
// of (row, chunk c of the inner set, half wave) is fm_seg(row, nchunks(inner), c - c0, half) counted from the edge's
// base -- twice its entries' start (psx_graph_edge.pf / pb) --, which is added to the two pointers.
//
// The flag.  Path B queues everything without reading the flag -- norms, conversion, prefilter and exact evaluation of every
// group and direction, the join, and a 4-byte copy of the flag behind them -- and synchronises ONCE.  k_gf_exact always
// leaves a directed result whose indices lie inside the inner set, so the join behind it never reads out of bounds; when
// the flag comes back up (a segment overflowed, or match_scale refused the norms: zero everywhere, infinite or NaN) that
// output is discarded and path A runs for the whole call on the same stream, with a second synchronisation.  Nothing is
// carried from call to call.
//
// Launches per call, whatever n_edges and n_sets are: path A 1 + 2 per group and direction + 3 = 8 kernels with the
// cross-check, 6 without; path B 2 + 2 per group and direction + 3 = 9 / 7; the table copy in front and one
// synchronisation.  The scratch buffers are the float one-to-many call's (MS_MANYF_*): the two never run at once on a thread.
#include "psx_internal.h"
#include "match_f32_many_core.h"
#include "match_graph_f32_plan.h"
#include "match_graph_join.h"
#include "match_join.h"
#include "match_scratch.h"

#include <climits>
#include <cstdio>
#include <cstring>
#include <vector>

namespace {

static_assert(PSX_MANYF_SEGCAP == MF_SEGCAP && PSX_MANYF_PRE_STEP == MF_SUB * MF_TILE && PSX_MANYF_SCAN_UNIT == sizeof(Top2),
              "match_many_f32_plan.h sizes what the kernels here use");
static_assert(sizeof(psx_graph_edge) == 32 && sizeof(psx_graph_item) == 16 && sizeof(psx_graph_wg) == 8 &&
              sizeof(psx_many_block) == 8 && sizeof(psx_many_chunk) == 12, "the plan's entries are the device's");

// one entry per set of the caller's array; an unreferenced set has len 0 and is never read
struct GFSet {
    const float* desc;           // the set's descriptors
    int len;                     // rows
    int foff;                    // its first row in the gathered arrays (permuted copy; f16 copy and norms)
    int c0, c1;                  // its chunks in the chunk table
    int pad0, pad1;
};
static_assert(sizeof(GFSet) == 32, "two 16-byte scalar loads per entry");

// ---- path A --------------------------------------------------------------------------------------------------------

// grid: every block of every referenced set, 256 threads
__global__ __launch_bounds__(256) void k_gf_permute(const GFSet* __restrict__ sets, const int2* __restrict__ blocks, float* __restrict__ dst)
{
    const int2 blk = blocks[blockIdx.x];
    const GFSet s = sets[blk.x];
    const int rows = min(PSX_MANY_BLOCK, s.len - blk.y);
    fm_permute_block(s.desc + (size_t)blk.y * 128, rows, reinterpret_cast<float2*>(dst + ((size_t)s.foff + blk.y) * 128));
}

// grid: the items of one group, 256 threads.  k_match_partial's walk with the pair (outer block, inner chunk) read from ONE
// item at a wave-uniform address: lane (64 w + j) owns outer row blk.row0 + 64 w + j of the block's set (original layout)
// and walks rows [r0, r1) of the chunk's set in the permuted copy (wave-uniform: scalar loads).
// partial[item.pbase + (row within the outer set)] = top-2 within the chunk, indices within the inner set.
__global__ __launch_bounds__(256) void k_gf_partial(const GFSet* __restrict__ sets, const int4* __restrict__ chunks,
                                                    const int2* __restrict__ blocks, const int4* __restrict__ items,
                                                    const float* __restrict__ perm, Top2* __restrict__ partial)
{
    const int4 it = items[blockIdx.x];
    const int2 blk = blocks[it.x];
    const int4 chk = chunks[it.y];
    const GFSet os = sets[blk.x], is = sets[chk.x];
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
    if (row < os.len) partial[(size_t)it.z + (size_t)row] = t;
}

// grid: the {edge, row0} entries of one group, 256 threads: one thread per (edge, outer row).  The inner set's chunks in
// table order = index order, merged as k_match_merge merges them.  The result goes where the join expects the directed
// result of this edge: at out + 5 * (the edge's first row among all edges' outer rows).
__global__ __launch_bounds__(256) void k_gf_merge(const GFSet* __restrict__ sets, const psx_graph_edge* __restrict__ edges,
                                                  const int2* __restrict__ wgs, int backward, const Top2* __restrict__ partial,
                                                  int* __restrict__ out)
{
    const int2 wg = wgs[blockIdx.x];
    const psx_graph_edge e = edges[wg.x];
    const GFSet os = sets[backward ? e.right : e.left], is = sets[backward ? e.left : e.right];
    const int row = wg.y + (int)threadIdx.x;
    if (row >= os.len) return;
    const Top2* p = partial + (size_t)(backward ? e.pb : e.pf) + row;
    Top2 t = {INFINITY, INFINITY, 0, 0};
    // chunks are visited in index order and a chunk's own entries are already in (distance, index) order, so strict '<'
    // insertion reproduces the sequential scan: ties keep the smaller index
    for (int c = is.c0; c < is.c1; c++, p += os.len) {
        const Top2 q = *p;
        top2_insert(t, q.d1, q.i1);
        top2_insert(t, q.d2, q.i2);
    }
    psx_directed_store<float>(out + 5 * (size_t)(backward ? e.boff : e.foff), os.len, (size_t)row, t.i1, t.i2, t.d1 / t.d2 < 0.8f, t.d1, t.d2);
}

// ---- path B --------------------------------------------------------------------------------------------------------

// grid: every block of every referenced set, 256 threads: norm2[foff + row] and the block's largest
__global__ __launch_bounds__(256) void k_gf_norms(const GFSet* __restrict__ sets, const int2* __restrict__ blocks,
                                                  float* __restrict__ norm2, unsigned* __restrict__ bmax)
{
    const int2 blk = blocks[blockIdx.x];
    const GFSet s = sets[blk.x];
    const int end = min(blk.y + PSX_MANY_BLOCK, s.len);
    fm_norms_block(s.desc, blk.y, end, norm2 + s.foff, bmax + blockIdx.x);
}

// grid as k_gf_norms.  ALL nb blocks count as the ranked side: par[2] = Rmax^2 = M^2 = the largest squared norm of the
// call, which both directions read (par[4] is not used here).  Then the f16 copy of the block's rows, scaled by 2^k.
__global__ __launch_bounds__(256) void k_gf_cvt(const GFSet* __restrict__ sets, const int2* __restrict__ blocks, int nb,
                                                const unsigned* __restrict__ bmax, unsigned short* __restrict__ h16,
                                                float* __restrict__ par, int* __restrict__ flag)
{
    const float sc = fm_cvt_params(nb, 0, bmax, par, flag);
    const int2 blk = blocks[blockIdx.x];
    const GFSet s = sets[blk.x];
    const int rows = min(PSX_MANY_BLOCK, s.len - blk.y);
    fm_cvt_block(reinterpret_cast<const float4*>(s.desc + (size_t)blk.y * 128), rows, sc,
                 reinterpret_cast<ushort4*>(h16 + ((size_t)s.foff + blk.y) * 128));
}

// grid: the items of one group, 256 threads; three workgroups per CU and no scratch, as k_f32_many_mfma.  Wave w owns outer
// rows [row0 + 64 w, + 64) of the item's block and walks the item's chunk.  The segments of the item's edge start at twice
// its entries' start; within the edge fm_seg(row, nchunks(inner), c - c0, half).
__global__ __launch_bounds__(256, 3) void k_gf_mfma(const GFSet* __restrict__ sets, const int4* __restrict__ chunks,
                                                    const int2* __restrict__ blocks, const psx_graph_edge* __restrict__ edges,
                                                    const int4* __restrict__ items, const unsigned short* __restrict__ h16,
                                                    const float* __restrict__ n2, const float* __restrict__ par, int backward,
                                                    int* __restrict__ cand_ct, int* __restrict__ cand)
{
    __shared__ __attribute__((aligned(16))) unsigned char s_r[2][MF_SUB * MF_TILE * MF_ROW];
    __shared__ __attribute__((aligned(16))) float s_n[2][MF_SUB * MF_TILE];
    const int4 it = items[blockIdx.x];
    const int2 blk = blocks[it.x];
    const int4 chk = chunks[it.y];
    const GFSet os = sets[blk.x], is = sets[chk.x];
    const psx_graph_edge e = edges[it.w];
    const size_t seg0 = 2 * (size_t)(backward ? e.pb : e.pf);
    fm_prefilter_block(s_r, s_n, h16 + (size_t)os.foff * 128, n2 + os.foff, os.len, blk.y, h16 + (size_t)is.foff * 128, n2 + is.foff, is.len,
                       chk.y, min(chk.z, is.len), par[1], par[2], par[3], cand_ct + seg0, cand + seg0 * MF_SEGCAP, 0, is.c1 - is.c0, it.y - is.c0);
}

// grid: 64 x the {edge, row0} entries of one group, 256 threads: wave w of workgroup (entry, q) takes outer row row0 + 4 q + w
// of the entry's edge against the edge's inner set.  ALWAYS writes a result whose indices lie in the inner set (the join
// behind it reads it whatever the flag says); raises the flag for a segment that overflowed.  out as k_gf_merge.
__global__ __launch_bounds__(256) void k_gf_exact(const GFSet* __restrict__ sets, const psx_graph_edge* __restrict__ edges,
                                                  const int2* __restrict__ wgs, int backward, const int* __restrict__ cand_ct,
                                                  const int* __restrict__ cand, int* __restrict__ out, int* __restrict__ flag)
{
    const int2 wg = wgs[blockIdx.x >> 6];
    const psx_graph_edge e = edges[wg.x];
    const GFSet os = sets[backward ? e.right : e.left], is = sets[backward ? e.left : e.right];
    const int lane = threadIdx.x & 63, tl = lane & 31;
    const int row = wg.y + (int)(blockIdx.x & 63u) * 4 + (int)(threadIdx.x >> 6);
    if (row >= os.len) return;                                  // wave uniform
    const float4 l4 = reinterpret_cast<const float4*>(os.desc + (size_t)row * 128)[tl];
    const int nch = is.c1 - is.c0;
    __shared__ int s_list[4][FX_SEGS * MF_SEGCAP];
    Top2 t;
    const bool over = fm_exact_row(l4, is.desc, cand_ct, cand, ((size_t)(backward ? e.pb : e.pf) + (size_t)row * nch) * 2, 2 * nch,
                                   s_list[threadIdx.x >> 6], t);
    if (__ballot(over) != 0ull && lane == 0) *flag = 1;
    if (lane == 0) {
        // the reference starts from (inf, inf, index 0, index 0) and never replaces an entry by an equal one
        const int i1 = t.i1 == 0x7fffffff ? 0 : t.i1, i2 = t.i2 == 0x7fffffff ? 0 : t.i2;
        psx_directed_store<float>(out + 5 * (size_t)(backward ? e.boff : e.foff), os.len, (size_t)row, i1, i2, t.d1 / t.d2 < 0.8f, t.d1, t.d2);
    }
}

size_t pad16(size_t b) { return (b + 15) & ~(size_t)15; }

thread_local psx_many_f32_info t_info = {0, 0, 0, 0};

// host_pairs or d_pairs (the other is NULL; both NULL with capacity 0)
int match_pairs_graph_f32(int device, const float* const* d_sets, const int* lens, int n_sets, const psx_view_edge* edges, int n_edges,
                          const psx_match_opts* opts, void* host_pairs, void* d_pairs, int capacity, int* edge_counts, int* count)
{
    if (!psx_pairs_args_ok(0, 0, opts, host_pairs ? host_pairs : d_pairs, capacity, count) || (n_sets > 0 && !d_sets) ||
        (n_edges > 0 && !edge_counts) || !psx_graph_args_ok(lens, n_sets, edges, n_edges))
        return PSX_ERR_INVALID;
    for (int s = 0; s < n_sets; s++)
        if (lens[s] > 0 && !d_sets[s]) return PSX_ERR_INVALID;
    t_info = psx_many_f32_info{0, 0, 0, 0};
    const bool mutual = (opts->flags & PSX_PAIRS_MUTUAL) != 0;
    long long all_pairs = 0, bwd_rows = 0, live = 0;
    for (int e = 0; e < n_edges; e++)
        if (psx_graph_live(lens, edges[e])) { all_pairs += lens[edges[e].left]; bwd_rows += lens[edges[e].right]; live++; }
    if (live == 0) {
        for (int e = 0; e < n_edges; e++) edge_counts[e] = 0;
        *count = 0;
        return PSX_OK;
    }

    if (hipSetDevice(device) != hipSuccess) return PSX_ERR_HIP;
    MatchScratch& sc = psx_match_scratch();
    if (!sc.bind(device)) return PSX_ERR_HIP;
    const int planned = psx_graphf_path(lens, edges, n_edges, sc.tune.match_mfma);
    t_info.path = planned;

    const size_t nrec = host_pairs ? (size_t)(capacity < all_pairs ? capacity : all_pairs) : 0;
    const size_t off_counts = 16, off_flag = off_counts + pad16(sizeof(int) * (size_t)n_edges), off_rec = off_flag + 16, off_blob = off_rec + 16 * nrec;
    hipStream_t st = sc.stream;
    thread_local psx_graphf_tables tb;
    thread_local std::vector<psx_many_chunk> chk;

    // one path over the whole call: tables, directed passes of every group, join, the flag; synchronised on return
    auto run = [&](int path, int* h_flag_out) -> int {
        if (!psx_graph_f32_build(lens, n_sets, edges, n_edges, mutual, path, tb)) return PSX_ERR_NOMEM;
        const long long B = tb.blocks, CH = tb.chunks, FI = tb.items[0], BI = tb.items[1], FW = tb.wgs[0], BW = tb.wgs[1], T = tb.rows;
        const size_t sets_b = pad16(sizeof(GFSet) * (size_t)n_sets), edges_b = pad16(sizeof(psx_graph_edge) * (size_t)n_edges);
        const size_t chunks_b = pad16(sizeof(int4) * (size_t)CH), items_b = pad16(sizeof(psx_graph_item) * (size_t)(FI + BI));
        const size_t blocks_b = pad16(sizeof(int2) * (size_t)B), wgs_b = pad16(sizeof(psx_graph_wg) * (size_t)(FW + BW));
        const size_t o_edges = sets_b, o_chunks = o_edges + edges_b, o_items = o_chunks + chunks_b, o_blocks = o_items + items_b,
                     o_wgs = o_blocks + blocks_b, blob_b = o_wgs + wgs_b;
        const size_t state_b = pad16(sizeof(unsigned) * (size_t)B) + sizeof(float) * FPAR + 16;
        // every buffer before the first launch: nothing is reallocated under queued work
        if (!sc.need(MS_MANYF_TABLES, blob_b) || !sc.need(MS_MANYF_STATE, state_b) ||
            !sc.need(MS_MANYF_FWD, sizeof(int) * 5 * (size_t)all_pairs) || (mutual && !sc.need(MS_MANYF_BWD, sizeof(int) * 5 * (size_t)bwd_rows)) ||
            !sc.need(MS_MANYF_TOT, sizeof(int) * (2 * (size_t)FW + 1)) || !sc.need_pinned(off_blob + blob_b))
            return PSX_ERR_NOMEM;
        if (path == 1) {
            if (!sc.need(MS_MANYF_PERM, sizeof(float) * 128 * (size_t)T) || !sc.need(MS_MANYF_PARTIAL, sizeof(Top2) * (size_t)tb.entries)) return PSX_ERR_NOMEM;
        } else {
            const size_t segs = 2 * (size_t)tb.entries;
            if (!sc.need(MS_MANYF_F16, sizeof(unsigned short) * 128 * (size_t)T) || !sc.need(MS_MANYF_NORMS, sizeof(float) * (size_t)T) ||
                !sc.need(MS_MANYF_CAND_CT, sizeof(int) * segs) || !sc.need(MS_MANYF_CAND, sizeof(int) * MF_SEGCAP * segs))
                return PSX_ERR_NOMEM;
        }
        void* dev_pin = nullptr;
        if (hipHostGetDevicePointer(&dev_pin, sc.hpin, 0) != hipSuccess || dev_pin == nullptr) return PSX_ERR_HIP;
        char* hp = static_cast<char*>(sc.hpin);

        // ---- the tables, written into the pinned staging buffer and copied on the stream ----
        {
            char* blob = hp + off_blob;
            GFSet* hs = reinterpret_cast<GFSet*>(blob);
            for (int s = 0; s < n_sets; s++) {
                const int len = tb.eff[(size_t)s];
                hs[s] = GFSet{len > 0 ? d_sets[s] : nullptr, len, tb.foff[(size_t)s], tb.cuts[(size_t)s].c0, tb.cuts[(size_t)s].c1, 0, 0};
            }
            if (n_edges > 0) memcpy(blob + o_edges, tb.ep.data(), sizeof(psx_graph_edge) * (size_t)n_edges);
            // the chunk table as int4 {set, r0, r1, 0}: cut set by set, at the call's one chunk length
            int4* hc = reinterpret_cast<int4*>(blob + o_chunks);
            chk.resize((size_t)CH);
            psx_graphf_chunks(tb.eff.data(), n_sets, path, tb.chunk_len, chk.data(), CH);
            for (long long c = 0; c < CH; c++) hc[c] = make_int4(chk[(size_t)c].set, chk[(size_t)c].r0, chk[(size_t)c].r1, 0);
            psx_many_blocks(tb.eff.data(), n_sets, reinterpret_cast<psx_many_block*>(blob + o_blocks), B);
            psx_graph_item* hi = reinterpret_cast<psx_graph_item*>(blob + o_items);
            psx_graph_items(tb.eff.data(), tb.cuts.data(), tb.ep.data(), n_edges, 0, hi, FI);
            if (mutual) psx_graph_items(tb.eff.data(), tb.cuts.data(), tb.ep.data(), n_edges, 1, hi + FI, BI);
            psx_graph_wg* hw = reinterpret_cast<psx_graph_wg*>(blob + o_wgs);
            psx_graph_wgs(tb.eff.data(), tb.ep.data(), n_edges, 0, hw, FW);
            if (mutual) psx_graph_wgs(tb.eff.data(), tb.ep.data(), n_edges, 1, hw + FW, BW);
        }
        int* h_total = reinterpret_cast<int*>(hp);
        int* h_flag = reinterpret_cast<int*>(hp + off_flag);
        *h_total = -1;
        *h_flag = 0;
        memset(hp + off_counts, 0, sizeof(int) * (size_t)n_edges);  // an edge with an empty side has no workgroup to write its count
        const char* tbl = static_cast<const char*>(sc.buf[MS_MANYF_TABLES]);
        const GFSet* t_sets = reinterpret_cast<const GFSet*>(tbl);
        const psx_graph_edge* t_edges = reinterpret_cast<const psx_graph_edge*>(tbl + o_edges);
        const int4* t_chunks = reinterpret_cast<const int4*>(tbl + o_chunks);
        const int4* t_items = reinterpret_cast<const int4*>(tbl + o_items);
        const int2* t_blocks = reinterpret_cast<const int2*>(tbl + o_blocks);
        const int2* t_wgs = reinterpret_cast<const int2*>(tbl + o_wgs);
        unsigned* d_bmax = static_cast<unsigned*>(sc.buf[MS_MANYF_STATE]);
        float* d_par = reinterpret_cast<float*>(static_cast<char*>(sc.buf[MS_MANYF_STATE]) + pad16(sizeof(unsigned) * (size_t)B));
        int* d_flag = reinterpret_cast<int*>(d_par + FPAR);
        int* d_fwd = static_cast<int*>(sc.buf[MS_MANYF_FWD]);
        int* d_bwd = mutual ? static_cast<int*>(sc.buf[MS_MANYF_BWD]) : nullptr;
        int* d_tot = static_cast<int*>(sc.buf[MS_MANYF_TOT]);
        int* d_total = static_cast<int*>(dev_pin);
        int* d_counts = reinterpret_cast<int*>(static_cast<char*>(dev_pin) + off_counts);
        // the kernel's capacity for the host form is the staging buffer's (nrec <= capacity)
        int4* out = host_pairs ? reinterpret_cast<int4*>(static_cast<char*>(dev_pin) + off_rec) : static_cast<int4*>(d_pairs);
        const int cap = host_pairs ? (int)nrec : capacity;
        const bool stats = path == 2 && sc.tune.match_stats;            // measurement: candidates per (left, edge), forward
        long long st_sum = 0, st_n = 0; int st_max = 0, st_seg = 0;

        if (hipMemcpyAsync(sc.buf[MS_MANYF_TABLES], hp + off_blob, blob_b, hipMemcpyHostToDevice, st) != hipSuccess) return PSX_ERR_HIP;
        if (path == 1) {
            Top2* d_partial = static_cast<Top2*>(sc.buf[MS_MANYF_PARTIAL]);
            float* d_perm = static_cast<float*>(sc.buf[MS_MANYF_PERM]);
            hipLaunchKernelGGL(k_gf_permute, dim3((unsigned)B), dim3(256), 0, st, t_sets, t_blocks, d_perm);
            t_info.launches++;
            for (int dir = 0; dir < (mutual ? 2 : 1); dir++)
                for (const psx_graph_group& g : (dir == 0 ? tb.fg : tb.bg)) {
                    hipLaunchKernelGGL(k_gf_partial, dim3((unsigned)g.nitems), dim3(256), 0, st, t_sets, t_chunks, t_blocks,
                                       t_items + (dir ? FI : 0) + g.item0, static_cast<const float*>(d_perm), d_partial);
                    hipLaunchKernelGGL(k_gf_merge, dim3((unsigned)g.nwgs), dim3(256), 0, st, t_sets, t_edges, t_wgs + (dir ? FW : 0) + g.wg0, dir,
                                       static_cast<const Top2*>(d_partial), dir ? d_bwd : d_fwd);
                    t_info.launches += 2;
                }
        } else {
            unsigned short* d_h16 = static_cast<unsigned short*>(sc.buf[MS_MANYF_F16]);
            float* d_n2 = static_cast<float*>(sc.buf[MS_MANYF_NORMS]);
            int* d_cct = static_cast<int*>(sc.buf[MS_MANYF_CAND_CT]);
            int* d_cand = static_cast<int*>(sc.buf[MS_MANYF_CAND]);
            hipLaunchKernelGGL(k_gf_norms, dim3((unsigned)B), dim3(256), 0, st, t_sets, t_blocks, d_n2, d_bmax);
            hipLaunchKernelGGL(k_gf_cvt, dim3((unsigned)B), dim3(256), 0, st, t_sets, t_blocks, (int)B, static_cast<const unsigned*>(d_bmax), d_h16,
                               d_par, d_flag);
            t_info.launches += 2;
            for (int dir = 0; dir < (mutual ? 2 : 1); dir++)
                for (const psx_graph_group& g : (dir == 0 ? tb.fg : tb.bg)) {
                    hipLaunchKernelGGL(k_gf_mfma, dim3((unsigned)g.nitems), dim3(256), 0, st, t_sets, t_chunks, t_blocks, t_edges,
                                       t_items + (dir ? FI : 0) + g.item0, static_cast<const unsigned short*>(d_h16),
                                       static_cast<const float*>(d_n2), static_cast<const float*>(d_par), dir, d_cct, d_cand);
                    hipLaunchKernelGGL(k_gf_exact, dim3((unsigned)g.nwgs * 64u), dim3(256), 0, st, t_sets, t_edges, t_wgs + (dir ? FW : 0) + g.wg0,
                                       dir, static_cast<const int*>(d_cct), static_cast<const int*>(d_cand), dir ? d_bwd : d_fwd, d_flag);
                    t_info.launches += 2;
                    if (stats && dir == 0) {
                        // POPSIFT_MATCH_STATS (measurement only): the group's counts are read back before the next group reuses them
                        std::vector<int> h(2 * (size_t)g.entries);
                        if (hipStreamSynchronize(st) != hipSuccess || hipMemcpy(h.data(), d_cct, sizeof(int) * h.size(), hipMemcpyDeviceToHost) != hipSuccess)
                            return PSX_ERR_HIP;
                        t_info.syncs++;
                        for (int e = g.edge0; e < g.edge0 + g.nedges; e++) {
                            if (!psx_graph_live(lens, edges[e])) continue;
                            const psx_graph_edge& pe = tb.ep[(size_t)e];
                            const int nch = tb.cuts[(size_t)pe.right].c1 - tb.cuts[(size_t)pe.right].c0;
                            for (int i = 0; i < lens[pe.left]; i++) {
                                int tsum = 0;
                                for (int k = 0; k < 2 * nch; k++) {
                                    const int v = h[((size_t)pe.pf + (size_t)i * nch) * 2 + k];
                                    tsum += v; if (v > st_seg) st_seg = v;
                                }
                                st_sum += tsum; st_n++; if (tsum > st_max) st_max = tsum;
                            }
                        }
                    }
                }
        }
        psx_graph_join_queue<float>(st, t_sets, t_edges, t_wgs, d_fwd, d_bwd, (int)FW, opts->ratio, mutual, d_tot, out, cap, d_counts, d_total);
        t_info.launches += 3;
        if (path == 2 && hipMemcpyAsync(h_flag, d_flag, sizeof(int), hipMemcpyDeviceToHost, st) != hipSuccess) return PSX_ERR_HIP;
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return PSX_ERR_HIP;
        t_info.syncs++;
        *h_flag_out = *h_flag;
        if (stats)
            fprintf(stderr, "psx_match_pairs_graph prefilter: %lld live edges over %d sets, chunk length %d, candidates per (left, edge): mean %.1f, max %d; fullest segment %d of %d%s\n",
                    live, tb.referenced, tb.chunk_len, st_n ? (double)st_sum / (double)st_n : 0.0, st_max, st_seg, MF_SEGCAP,
                    *h_flag ? " -> exact scan of every pair" : "");
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
    memcpy(edge_counts, hp + off_counts, sizeof(int) * (size_t)n_edges);
    if (host_pairs && n > 0 && nrec > 0) memcpy(host_pairs, hp + off_rec, 16 * ((size_t)n < nrec ? (size_t)n : nrec));
    *count = n;
    return PSX_OK;
}

} // namespace

extern "C" int psx_match_pairs_graph(int device, const float* const* d_sets, const int* lens, int n_sets, const psx_view_edge* edges,
                                     int n_edges, const psx_match_opts* opts, psx_match_pair* host_pairs, int capacity, int* edge_counts,
                                     int* count)
{
    return match_pairs_graph_f32(device, d_sets, lens, n_sets, edges, n_edges, opts, host_pairs, nullptr, capacity, edge_counts, count);
}

extern "C" int psx_match_pairs_graph_dev(int device, const float* const* d_sets, const int* lens, int n_sets, const psx_view_edge* edges,
                                         int n_edges, const psx_match_opts* opts, psx_match_pair* d_pairs, int capacity, int* edge_counts,
                                         int* count)
{
    return match_pairs_graph_f32(device, d_sets, lens, n_sets, edges, n_edges, opts, nullptr, d_pairs, capacity, edge_counts, count);
}

extern "C" int psx_match_graph_f32_plan(const int* lens, int n_sets, const psx_view_edge* edges, int n_edges, int flags, int mfma_enabled,
                                        psx_graph_f32_plan_info* out)
{
    return psx_graph_f32_plan_host(lens, n_sets, edges, n_edges, flags, mfma_enabled, out);
}

extern "C" int psx_match_graph_f32_last(psx_many_f32_info* out)
{
    if (!out) return PSX_ERR_INVALID;
    *out = t_info;
    return PSX_OK;
}
