// match_graph.hip -- a list of view pairs over N byte descriptor sets in one call: psx_match_pairs_graph_u8 (+ _dev),
// psx_match_graph_plan.
//
// psx_match_pairs_many_u8 (match_many.hip) is one left set against K right sets: a caller with N views and an edge list
// loops over it per left view and pays, per call, the synchronisation, the table upload and the norms of every set the
// call touches.  "Edges over N sets" is the same dataflow with BOTH sides taken from a set table per edge
// (match_graph_plan.h): every referenced set is cut once per call, a flat host-built item table names, per workgroup, an
// outer block and an inner chunk, and the (distance, index) order being total, where the chunks are cut cannot change a
// result.  The matcher's device pieces are those of match_u8_core.h; the kernels here only say where the operands live:
//   k_u8_norms_graph        |x - 128|^2 of every row of every referenced set, once, each set padded to u8_pad(len)
//   k_match_u8_graph        the walk of k_match_u8 / k_match_u8_many on the item's outer block and inner chunk; forward and
//                           backward (PSX_PAIRS_MUTUAL only) are the same kernel on the other item table
//   k_match_u8_graph_merge  per (edge, outer row) the inner set's chunks in index order: the directed result
//                           (match_scratch.h) at the edge's row offset
//   k_graph_count / k_graph_scan / k_graph_write   (match_graph_join.h, which the float form match_graph_f32.hip queues too)
//                           the join, segmented by edge with the edge's OWN left length: the rule of
//                           match_rule.h (psx_match_keep) and the backward gather counted per workgroup (wg_compact.h), one
//                           scan of the totals (wg_scan_totals), one 16-byte store per survivor, the per-edge counts and the
//                           total.  The workgroups come from the {edge, row0} table in edge-major order, so the offsets
//                           are the concatenation's.  Nothing depends on arrival order.
// Launches per call, whatever n_edges and n_sets are: the table copy, the norms, 2 per direction per group, 3 for the
// join -- 8 kernels with the cross-check, 6 without; one stream synchronisation.  Above PSX_GRAPH_PARTIAL_BUDGET of per-chunk
// partials the edges are processed in groups of whole edges, each group its own match + merge on the same stream.
#include "psx_internal.h"
#include "match_graph_join.h"
#include "match_graph_plan.h"
#include "match_join.h"
#include "match_rule.h"
#include "match_scratch.h"
#include "match_u8_core.h"
#include "wg_compact.h"

#include <climits>
#include <cstring>
#include <vector>

namespace {

// one entry per set of the caller's array; an unreferenced set has len 0 and is never read
struct GraphSet {
    const unsigned char* desc;   // the set's descriptors
    int len;                     // rows
    int noff;                    // first entry of its norms in the norm array (a multiple of U8_TILE: 16-byte aligned)
    int c0, c1;                  // its chunks in the chunk table
    int pad0, pad1;
};
static_assert(sizeof(GraphSet) == 32, "two 16-byte scalar loads per entry");
static_assert(sizeof(psx_graph_edge) == 32 && sizeof(psx_graph_item) == 16 && sizeof(psx_graph_wg) == 8 &&
              sizeof(psx_many_block) == 8 && sizeof(psx_many_chunk) == 12, "the plan's entries are the device's");

// grid: every block of every referenced set, 256 threads, 8 lanes per descriptor.  A set's norms are written up to
// u8_pad(len), the padding with zeros: the set's last block writes it.
__global__ __launch_bounds__(256) void k_u8_norms_graph(const GraphSet* __restrict__ sets, const int2* __restrict__ blocks,
                                                        int* __restrict__ norms)
{
    const int2 blk = blocks[blockIdx.x];
    const GraphSet s = sets[blk.x];
    const int end = blk.y + PSX_MANY_BLOCK >= s.len ? (int)u8_pad(s.len) : blk.y + PSX_MANY_BLOCK;
    const int q = threadIdx.x & 7;
    for (int d = blk.y + (threadIdx.x >> 3); d < end; d += 32) {
        const int ss = u8_row_norm(s.desc, s.len, d, q);
        if (q == 0) norms[s.noff + d] = ss;
    }
}

// grid: the items of one group, 256 threads.  k_match_u8_many with the pair (outer block, inner chunk) read from ONE item
// at a wave-uniform address: wave w owns outer rows [row0 + 64 w, + 64) of the block's set and walks rows [r0, r1) of the
// chunk's set (match_u8_core.h).  Row reads are clamped to the set's own last row, idle outer columns repeat the last row
// of their own set, keys of rows past the chunk's end are U8_NONE: nothing of a neighbouring set is ever ranked.
// partial[item.pbase + (row within the outer set)] = (smallest, second smallest key).
__global__ __launch_bounds__(256) void k_match_u8_graph(const GraphSet* __restrict__ sets, const int4* __restrict__ chunks,
                                                        const int2* __restrict__ blocks, const int4* __restrict__ items,
                                                        const int* __restrict__ norms, uint2* __restrict__ partial)
{
    const int4 it = items[blockIdx.x];
    const int2 blk = blocks[it.x];
    const int4 chk = chunks[it.y];
    const GraphSet os = sets[blk.x], is = sets[chk.x];
    U8Wave w;
    u8_load_cols(w, os.desc, norms + os.noff, os.len, blk.y + (threadIdx.x >> 6) * 64);
    u8_walk(w, is.desc, norms + is.noff, is.len, chk.y, chk.z);
    u8_store_keys(w, os.len, partial + (size_t)it.z);
}

// grid: the {edge, row0} entries of one group, 256 threads: one thread per (edge, outer row).  The inner set's chunks in
// table order = index order, merged as k_match_u8_merge merges them (u8_merge_chunk).  The result goes where the join
// expects the directed result of this edge: at out + 5 * (the edge's first row among all edges' outer rows).
__global__ __launch_bounds__(256) void k_match_u8_graph_merge(const GraphSet* __restrict__ sets, const int4* __restrict__ chunks,
                                                              const psx_graph_edge* __restrict__ edges, const int2* __restrict__ wgs,
                                                              int backward, const uint2* __restrict__ partial, int* __restrict__ out)
{
    const int2 wg = wgs[blockIdx.x];
    const psx_graph_edge e = edges[wg.x];
    const GraphSet os = sets[backward ? e.right : e.left], is = sets[backward ? e.left : e.right];
    const int row = wg.y + (int)threadIdx.x;
    if (row >= os.len) return;
    const uint2* p = partial + (size_t)(backward ? e.pb : e.pf) + row;
    U8Best t;
    for (int c = is.c0; c < is.c1; c++, p += os.len) u8_merge_chunk(t, *p, chunks[c].y);
    psx_directed_store<int>(out + 5 * (size_t)(backward ? e.boff : e.foff), os.len, (size_t)row, t.i1, t.i2, u8_accept(t.d1, t.d2), t.d1, t.d2);
}

size_t pad16(size_t b) { return (b + 15) & ~(size_t)15; }

// host_pairs or d_pairs (the other is NULL; both NULL with capacity 0)
int match_pairs_graph(int device, const unsigned char* const* d_sets, const int* lens, int n_sets, const psx_view_edge* edges, int n_edges,
                      const psx_match_opts* opts, void* host_pairs, void* d_pairs, int capacity, int* edge_counts, int* count)
{
    if (!psx_pairs_args_ok(0, 0, opts, host_pairs ? host_pairs : d_pairs, capacity, count) || (n_sets > 0 && !d_sets) ||
        (n_edges > 0 && !edge_counts) || !psx_graph_args_ok(lens, n_sets, edges, n_edges))
        return PSX_ERR_INVALID;
    for (int s = 0; s < n_sets; s++)
        if (lens[s] > 0 && !d_sets[s]) return PSX_ERR_INVALID;
    const bool mutual = (opts->flags & PSX_PAIRS_MUTUAL) != 0;

    // ---- the plan (match_graph_plan.h), on the host ----
    thread_local std::vector<int> eff;
    thread_local std::vector<psx_graph_cut> cuts;
    thread_local std::vector<psx_graph_edge> ep;
    thread_local std::vector<psx_graph_group> fg, bg;
    eff.resize((size_t)n_sets + 1);
    if (psx_graph_eff(lens, n_sets, edges, n_edges, eff.data()) == 0) {
        for (int e = 0; e < n_edges; e++) edge_counts[e] = 0;
        *count = 0;
        return PSX_OK;
    }
    cuts.resize((size_t)n_sets); ep.resize((size_t)n_edges);
    const int chunk_len = psx_graph_chunk_len(lens, edges, n_edges, mutual);
    long long B = 0, CH = 0, nfg = 0, nbg = 0, items[2], wgs[2], entries = 0;
    if (!psx_graph_cuts(eff.data(), n_sets, chunk_len, cuts.data(), &B, &CH) ||
        !psx_graph_edges(lens, cuts.data(), edges, n_edges, mutual, PSX_GRAPH_PARTIAL_BUDGET, ep.data(), nullptr, 0, &nfg, nullptr, 0, &nbg,
                         items, wgs, &entries))
        return PSX_ERR_NOMEM;
    fg.resize((size_t)nfg); bg.resize((size_t)nbg);
    psx_graph_edges(lens, cuts.data(), edges, n_edges, mutual, PSX_GRAPH_PARTIAL_BUDGET, ep.data(), fg.data(), nfg, &nfg, bg.data(), nbg, &nbg,
                    items, wgs, &entries);
    const long long FI = items[0], BI = items[1], FW = wgs[0], BW = wgs[1];
    if (FI + BI > INT_MAX || FW + BW + 1 > INT_MAX) return PSX_ERR_NOMEM;

    // ---- sizes: the norms of the referenced sets, the tables, the results ----
    long long npad = 0, all_pairs = 0, bwd_rows = 0;
    for (int s = 0; s < n_sets; s++) npad += eff[s] > 0 ? u8_pad(eff[s]) : 0;
    if (npad > INT_MAX) return PSX_ERR_NOMEM;
    for (int e = 0; e < n_edges; e++)
        if (psx_graph_live(lens, edges[e])) { all_pairs += lens[edges[e].left]; bwd_rows += lens[edges[e].right]; }
    const size_t sets_b = pad16(sizeof(GraphSet) * (size_t)n_sets), edges_b = pad16(sizeof(psx_graph_edge) * (size_t)n_edges);
    const size_t chunks_b = pad16(sizeof(int4) * (size_t)CH), items_b = pad16(sizeof(psx_graph_item) * (size_t)(FI + BI));
    const size_t blocks_b = pad16(sizeof(int2) * (size_t)B), wgs_b = pad16(sizeof(psx_graph_wg) * (size_t)(FW + BW));
    const size_t o_edges = sets_b, o_chunks = o_edges + edges_b, o_items = o_chunks + chunks_b, o_blocks = o_items + items_b,
                 o_wgs = o_blocks + blocks_b, blob_b = o_wgs + wgs_b;
    const size_t nrec = host_pairs ? (size_t)(capacity < all_pairs ? capacity : all_pairs) : 0;
    const size_t off_counts = 16, off_rec = off_counts + pad16(sizeof(int) * (size_t)n_edges), off_blob = off_rec + 16 * nrec;

    if (hipSetDevice(device) != hipSuccess) return PSX_ERR_HIP;
    MatchScratch& sc = psx_match_scratch();
    if (!sc.bind(device)) return PSX_ERR_HIP;
    // every buffer before the first launch: nothing is reallocated under queued work
    if (!sc.need(MS_GRAPH_TABLES, blob_b) || !sc.need(MS_GRAPH_NORMS, sizeof(int) * (size_t)npad) ||
        !sc.need(MS_GRAPH_PARTIAL, sizeof(uint2) * (size_t)entries) || !sc.need(MS_GRAPH_FWD, sizeof(int) * 5 * (size_t)all_pairs) ||
        (mutual && !sc.need(MS_GRAPH_BWD, sizeof(int) * 5 * (size_t)bwd_rows)) ||
        !sc.need(MS_GRAPH_TOT, sizeof(int) * (2 * (size_t)FW + 1)) || !sc.need_pinned(off_blob + blob_b))
        return PSX_ERR_NOMEM;
    void* dev_pin = nullptr;
    if (hipHostGetDevicePointer(&dev_pin, sc.hpin, 0) != hipSuccess || dev_pin == nullptr) return PSX_ERR_HIP;
    char* hp = static_cast<char*>(sc.hpin);

    // ---- the tables, written into the pinned staging buffer and copied on the stream ----
    {
        char* blob = hp + off_blob;
        GraphSet* hs = reinterpret_cast<GraphSet*>(blob);
        long long noff = 0;
        for (int s = 0; s < n_sets; s++) {
            hs[s] = GraphSet{eff[s] > 0 ? d_sets[s] : nullptr, eff[s], (int)noff, cuts[(size_t)s].c0, cuts[(size_t)s].c1, 0, 0};
            noff += eff[s] > 0 ? u8_pad(eff[s]) : 0;
        }
        if (n_edges > 0) memcpy(blob + o_edges, ep.data(), sizeof(psx_graph_edge) * (size_t)n_edges);
        // the chunk table as int4 {set, r0, r1, 0}: cut set by set, at the call's one chunk length
        int4* hc = reinterpret_cast<int4*>(blob + o_chunks);
        psx_many_block* hb = reinterpret_cast<psx_many_block*>(blob + o_blocks);
        psx_many_blocks(eff.data(), n_sets, hb, B);
        thread_local std::vector<psx_many_chunk> chk;
        chk.resize((size_t)CH);
        psx_many_chunks_of(eff.data(), n_sets, chunk_len, chk.data(), CH);
        for (long long c = 0; c < CH; c++) hc[c] = make_int4(chk[(size_t)c].set, chk[(size_t)c].r0, chk[(size_t)c].r1, 0);
        psx_graph_item* hi = reinterpret_cast<psx_graph_item*>(blob + o_items);
        psx_graph_items(eff.data(), cuts.data(), ep.data(), n_edges, 0, hi, FI);
        if (mutual) psx_graph_items(eff.data(), cuts.data(), ep.data(), n_edges, 1, hi + FI, BI);
        psx_graph_wg* hw = reinterpret_cast<psx_graph_wg*>(blob + o_wgs);
        psx_graph_wgs(eff.data(), ep.data(), n_edges, 0, hw, FW);
        if (mutual) psx_graph_wgs(eff.data(), ep.data(), n_edges, 1, hw + FW, BW);
    }
    int* h_total = reinterpret_cast<int*>(hp);
    *h_total = -1;
    memset(hp + off_counts, 0, sizeof(int) * (size_t)n_edges);      // an edge with an empty side has no workgroup to write its count
    const char* tb = static_cast<const char*>(sc.buf[MS_GRAPH_TABLES]);
    const GraphSet* t_sets = reinterpret_cast<const GraphSet*>(tb);
    const psx_graph_edge* t_edges = reinterpret_cast<const psx_graph_edge*>(tb + o_edges);
    const int4* t_chunks = reinterpret_cast<const int4*>(tb + o_chunks);
    const int4* t_items = reinterpret_cast<const int4*>(tb + o_items);
    const int2* t_blocks = reinterpret_cast<const int2*>(tb + o_blocks);
    const int2* t_wgs = reinterpret_cast<const int2*>(tb + o_wgs);
    int* d_norms = static_cast<int*>(sc.buf[MS_GRAPH_NORMS]);
    uint2* d_partial = static_cast<uint2*>(sc.buf[MS_GRAPH_PARTIAL]);
    int* d_fwd = static_cast<int*>(sc.buf[MS_GRAPH_FWD]);
    int* d_bwd = mutual ? static_cast<int*>(sc.buf[MS_GRAPH_BWD]) : nullptr;
    int* d_tot = static_cast<int*>(sc.buf[MS_GRAPH_TOT]);
    int* d_total = static_cast<int*>(dev_pin);
    int* d_counts = reinterpret_cast<int*>(static_cast<char*>(dev_pin) + off_counts);
    // the kernel's capacity for the host form is the staging buffer's (nrec <= capacity)
    int4* out = host_pairs ? reinterpret_cast<int4*>(static_cast<char*>(dev_pin) + off_rec) : static_cast<int4*>(d_pairs);
    const int cap = host_pairs ? (int)nrec : capacity;
    hipStream_t st = sc.stream;

    if (hipMemcpyAsync(sc.buf[MS_GRAPH_TABLES], hp + off_blob, blob_b, hipMemcpyHostToDevice, st) != hipSuccess) return PSX_ERR_HIP;
    hipLaunchKernelGGL(k_u8_norms_graph, dim3((unsigned)B), dim3(256), 0, st, t_sets, t_blocks, d_norms);
    for (const psx_graph_group& g : fg) {
        hipLaunchKernelGGL(k_match_u8_graph, dim3((unsigned)g.nitems), dim3(256), 0, st, t_sets, t_chunks, t_blocks, t_items + g.item0,
                           d_norms, d_partial);
        hipLaunchKernelGGL(k_match_u8_graph_merge, dim3((unsigned)g.nwgs), dim3(256), 0, st, t_sets, t_chunks, t_edges, t_wgs + g.wg0, 0,
                           d_partial, d_fwd);
    }
    for (const psx_graph_group& g : bg) {
        hipLaunchKernelGGL(k_match_u8_graph, dim3((unsigned)g.nitems), dim3(256), 0, st, t_sets, t_chunks, t_blocks, t_items + FI + g.item0,
                           d_norms, d_partial);
        hipLaunchKernelGGL(k_match_u8_graph_merge, dim3((unsigned)g.nwgs), dim3(256), 0, st, t_sets, t_chunks, t_edges, t_wgs + FW + g.wg0, 1,
                           d_partial, d_bwd);
    }
    psx_graph_join_queue<int>(st, t_sets, t_edges, t_wgs, d_fwd, d_bwd, (int)FW, opts->ratio, mutual, d_tot, out, cap, d_counts, d_total);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return PSX_ERR_HIP;
    const int n = *h_total;
    if (n < 0 || n > all_pairs) return PSX_ERR_HIP;
    memcpy(edge_counts, hp + off_counts, sizeof(int) * (size_t)n_edges);
    if (host_pairs && n > 0 && nrec > 0) memcpy(host_pairs, hp + off_rec, 16 * ((size_t)n < nrec ? (size_t)n : nrec));
    *count = n;
    return PSX_OK;
}

} // namespace

extern "C" int psx_match_pairs_graph_u8(int device, const unsigned char* const* d_sets, const int* lens, int n_sets,
                                        const psx_view_edge* edges, int n_edges, const psx_match_opts* opts,
                                        psx_match_pair_u8* host_pairs, int capacity, int* edge_counts, int* count)
{
    return match_pairs_graph(device, d_sets, lens, n_sets, edges, n_edges, opts, host_pairs, nullptr, capacity, edge_counts, count);
}

extern "C" int psx_match_pairs_graph_u8_dev(int device, const unsigned char* const* d_sets, const int* lens, int n_sets,
                                            const psx_view_edge* edges, int n_edges, const psx_match_opts* opts,
                                            psx_match_pair_u8* d_pairs, int capacity, int* edge_counts, int* count)
{
    return match_pairs_graph(device, d_sets, lens, n_sets, edges, n_edges, opts, nullptr, d_pairs, capacity, edge_counts, count);
}

extern "C" int psx_match_graph_plan(const int* lens, int n_sets, const psx_view_edge* edges, int n_edges, int flags,
                                    psx_graph_plan_info* out)
{
    return psx_graph_plan_host(lens, n_sets, edges, n_edges, flags, out);
}
