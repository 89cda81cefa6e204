// match_guided_graph.hip -- the guided re-match of a list of view pairs over N descriptor sets in one call:
// psx_match_pairs_guided_graph_u8 (+ _dev) for byte descriptors, psx_match_pairs_guided_graph (+ _dev) for float ones
// (include/popsift_hip.h).  Everything below is stated once on (T, D) = (descriptor element, distance type) -- (unsigned
// char, int) or (float, float), as g_match_row is -- and instantiated for both; the text speaks of the byte form.
//
// This is the ONE batched guided re-match of the library.  psx_match_pairs_guided_u8 (match_guided.hip) is a fixed launch
// sequence, one synchronisation and one count read-back per call; at 2k-4k descriptors per image that is what a loop over
// view pairs pays per pair.  psx_match_pairs_guided_many_u8 -- ONE left set against K right sets, each under its own guide
// -- is a star, an edge list whose edges share their left set: match_guided_many.hip only checks the star's arguments,
// states it as such a list and calls psx_guided_edges_run below (a star costs nothing here against kernels written for
// it: profiles/graph_chain_ms.txt).  The wave-level search of the single call
// (g_match_row, match_guided_core.h, unchanged: one wave per outer descriptor) is driven over all edges by one grid per
// step, its operands taken from an EDGE TABLE (match_guided_graph_plan.h): one entry per edge with both sides'
// descriptors, positions and lengths, the edge's OWN guide, and its first forward row (which is its first line too) and
// first backward row among all edges' rows.  The table is built in the pinned staging buffer and copied on the stream; an
// entry is read at wave-uniform addresses.  An edge that is skipped (guide of kind PSX_GUIDE_NONE) or has an empty side is
// in the table with lengths 0 and in no block table: none of its arrays is read, the join has nothing to look at.
//   k_gg_lines         (cross-check only) lines[foff_e + i] = the first step of the rule (psx_guide_left) for left row i
//                      of edge e under guide e; one grid over the forward block table = the sum of the left lengths
//   k_gg_match<false>  forward: the blocks are 256 left rows of ONE edge, never crossing an edge, 64 workgroups of 4 waves
//                      per block; wave (e, i) walks the right positions of edge e under guide e; its directed result goes
//                      to fwd + 5 foff_e
//   k_gg_match<true>   backward (cross-check only): the same over the right rows; wave (e, j) walks lines + foff_e, the
//                      SAME relation with the loops exchanged, and writes at bwd + 5 boff_e
//   k_gg_count / k_gg_scan / k_gg_write   the join, segmented by edge with the edge's OWN left length: the rule of
//                      match_rule.h (psx_match_keep) and the backward gather counted per workgroup (wg_compact.h), one
//                      scan of the totals (wg_scan_totals), one 16-byte store per survivor, the per-edge counts and the
//                      total.  The workgroups come from the forward block table in edge-major order, so the offsets are
//                      the concatenation's.  No atomics; nothing depends on arrival order.
// A wave past its edge's last row leaves before any load of a descriptor or a position; every index a wave forms is below
// its own edge's lengths, so nothing of a neighbouring edge is read or ranked.
// Launches per call, whatever n_edges and n_sets are: the table copy, then 4 kernels without the cross-check and 6 with
// it; one stream synchronisation.  Every scratch buffer is sized before the first launch.
#include "psx_internal.h"
#include "guide_rule.h"
#include "match_guided_core.h"
#include "match_guided_graph_plan.h"
#include "match_rule.h"
#include "match_scratch.h"
#include "wg_compact.h"

#include <climits>
#include <cstring>
#include <vector>

namespace {

// one entry per edge
template <class T>
struct GGEdge {
    const T* ldesc;              // the left set's descriptors
    const float2* lxy;           // ... and positions
    const T* rdesc;              // the right set's
    const float2* rxy;
    int l_len, r_len;            // rows; both 0 for an edge that is skipped or has an empty side
    int foff, boff;              // its first forward row (and line) / backward row among all edges' rows
    psx_guide guide;             // the edge's own guide
    int pad;
};
static_assert(sizeof(psx_guide) == 44 && sizeof(GGEdge<unsigned char>) == 96 && sizeof(GGEdge<float>) == 96, "whole 16-byte scalar loads per entry");
static_assert(sizeof(psx_graph_wg) == 8, "the plan's entries are the device's");

// grid: the forward block table, one thread per (edge, left row)
template <class T>
__global__ __launch_bounds__(256) void k_gg_lines(const GGEdge<T>* __restrict__ edges, const int2* __restrict__ blocks, float4* __restrict__ lines)
{
    const int2 blk = blocks[blockIdx.x];
    const GGEdge<T>* e = edges + blk.x;
    const int i = blk.y + (int)threadIdx.x;
    if (i >= e->l_len) return;
    const float2 p = e->lxy[i];
    const psx_guide_line l = psx_guide_left(e->guide.kind, e->guide.m, e->guide.tol, p.x, p.y);
    lines[(size_t)e->foff + (size_t)i] = make_float4(l.a, l.b, l.c, l.w);
}

// 256 threads, one wave per outer descriptor.  grid (blocks of the direction) * 64, workgroup (blk, q) = (blockIdx.x / 64,
// blockIdx.x % 64) owns outer rows row0 + 4 q .. + 3 of its block's edge.  Forward (SWAP = false): the outer side is the
// edge's left set, the inner geometry its right positions; lines is unused.  Backward (SWAP = true): the outer side is
// the right set, the inner geometry the edge's lines.
// The wave's search (g_match_row, match_guided_core.h) on edge e's operands, forward and backward, per descriptor type: the
// distance type follows the element type
__device__ __forceinline__ void gg_forward(const GGEdge<unsigned char>* e, int row, int* __restrict__ out)
{
    g_match_row<unsigned char, int, false>(e->ldesc, e->lxy, e->l_len, row, e->rdesc, e->rxy, e->r_len, e->guide, out + 5 * (size_t)e->foff);
}
__device__ __forceinline__ void gg_backward(const GGEdge<unsigned char>* e, int row, const float4* __restrict__ lines, int* __restrict__ out)
{
    g_match_row<unsigned char, int, true>(e->rdesc, e->rxy, e->r_len, row, e->ldesc, lines + (size_t)e->foff, e->l_len, e->guide,
                                          out + 5 * (size_t)e->boff);
}
__device__ __forceinline__ void gg_forward(const GGEdge<float>* e, int row, int* __restrict__ out)
{
    g_match_row<float, float, false>(e->ldesc, e->lxy, e->l_len, row, e->rdesc, e->rxy, e->r_len, e->guide, out + 5 * (size_t)e->foff);
}
__device__ __forceinline__ void gg_backward(const GGEdge<float>* e, int row, const float4* __restrict__ lines, int* __restrict__ out)
{
    g_match_row<float, float, true>(e->rdesc, e->rxy, e->r_len, row, e->ldesc, lines + (size_t)e->foff, e->l_len, e->guide,
                                    out + 5 * (size_t)e->boff);
}

template <class T, bool SWAP>
__global__ __launch_bounds__(256) void k_gg_match(const GGEdge<T>* __restrict__ edges, const int2* __restrict__ blocks,
                                                  const float4* __restrict__ lines, int* __restrict__ out)
{
    const int2 blk = blocks[blockIdx.x >> 6];
    const GGEdge<T>* e = edges + blk.x;
    const int row = blk.y + 4 * (int)(blockIdx.x & 63u) + (int)(threadIdx.x >> 6);
    if (!SWAP) gg_forward(e, row, out);
    else gg_backward(e, row, lines, out);
}

// the record carries the distance's bits, whichever type it has
__device__ __forceinline__ int gg_bits(float d) { return __float_as_int(d); }
__device__ __forceinline__ int gg_bits(int d) { return d; }

// The rule of match_rule.h for left row i of edge e: the edge's forward result, and with the cross-check the gather into
// the edge's backward rows.
template <class T, class D>
__device__ __forceinline__ bool gg_rule(const GGEdge<T>* __restrict__ e, const int* __restrict__ fwd, const int* __restrict__ bwd, int i,
                                        float ratio, int mutual, int4& rec)
{
    const int l_len = e->l_len;
    if (i >= l_len) return false;
    int j;
    D d1, d2;
    psx_directed_load<D>(fwd + 5 * (size_t)e->foff, l_len, i, j, d1, d2);
    bool keep = psx_match_keep(psx_match_dist(d1), psx_match_dist(d2), ratio);
    if (keep && mutual) keep = psx_directed_best(bwd + 5 * (size_t)e->boff, j) == i;
    rec = make_int4(i, j, gg_bits(d1), gg_bits(d2));
    return keep;
}

// grid: the forward block table, edge-major: one total per workgroup
template <class T, class D>
__global__ __launch_bounds__(256) void k_gg_count(const GGEdge<T>* __restrict__ edges, const int2* __restrict__ blocks, const int* __restrict__ fwd,
                                                  const int* __restrict__ bwd, float ratio, int mutual, int* __restrict__ wg_tot)
{
    const int2 blk = blocks[blockIdx.x];
    int4 rec;
    const bool keep = gg_rule<T, D>(edges + blk.x, fwd, bwd, blk.y + (int)threadIdx.x, ratio, mutual, rec);
    __shared__ int s_cnt[4];
    wg_count(__ballot(keep), s_cnt);
    if (threadIdx.x == 0) wg_tot[blockIdx.x] = wg_total(s_cnt);
}

// ONE workgroup of 1024 threads: offs[w] = the totals before workgroup w, offs[n] = all of them (wg_compact.h)
__global__ __launch_bounds__(1024) void k_gg_scan(const int* __restrict__ wg_tot, int n, int* __restrict__ offs)
{
    wg_scan_totals(wg_tot, n, offs);
}

// grid as k_gg_count.  Evaluates the rule again, ranks its lanes and writes each surviving record with ONE 16-byte store
// at offs[workgroup] + rank, never at or past capacity; an edge's first workgroup writes the edge's count (an edge without
// workgroups keeps the zero the host put there), workgroup 0 the total.
template <class T, class D>
__global__ __launch_bounds__(256) void k_gg_write(const GGEdge<T>* __restrict__ edges, const int2* __restrict__ blocks, const int* __restrict__ fwd,
                                                  const int* __restrict__ bwd, float ratio, int mutual, const int* __restrict__ offs,
                                                  int4* __restrict__ out, int capacity, int* __restrict__ edge_counts, int* __restrict__ total)
{
    const int2 blk = blocks[blockIdx.x];
    const GGEdge<T>* e = edges + blk.x;
    int4 rec = make_int4(0, 0, 0, 0);
    const bool keep = gg_rule<T, D>(e, fwd, bwd, blk.y + (int)threadIdx.x, ratio, mutual, rec);
    const unsigned long long m = __ballot(keep);
    __shared__ int s_cnt[4];
    wg_count(m, s_cnt);
    const int pos = offs[blockIdx.x] + wg_offset(m, s_cnt);
    if (keep && pos < capacity) out[pos] = rec;
    if (threadIdx.x == 0) {
        if (blk.y == 0) edge_counts[blk.x] = offs[blockIdx.x + (unsigned)((e->l_len + 255) / 256)] - offs[blockIdx.x];
        if (blockIdx.x == 0) *total = offs[gridDim.x];
    }
}

size_t pad16(size_t b) { return (b + 15) & ~(size_t)15; }

template <class T> struct GGDist;                                    // the distance type of a descriptor element
template <> struct GGDist<unsigned char> { typedef int type; };
template <> struct GGDist<float> { typedef float type; };

} // namespace

// The ONE batched driver, behind the argument checks of its caller (psx_gg_args_ok for an edge list; the star's own,
// match_guided_many.hip): internal, declared in match_scratch.h and instantiated below for byte and for float descriptors.
// host_pairs or d_pairs (the other is NULL; both NULL with capacity 0)
template <class T>
int psx_guided_edges_run(int device, const T* const* d_sets, const float* const* d_xys, const int* lens, const psx_view_edge* edges,
                         int n_edges, const psx_guide* guides, const psx_match_opts* opts, void* host_pairs, void* d_pairs, int capacity,
                         int* edge_counts, int* count)
{
    typedef GGEdge<T> GGEdge;
    typedef typename GGDist<T>::type D;
    const int E = n_edges;
    thread_local std::vector<psx_gg_edge> ep;
    ep.resize((size_t)E + 1);
    const psx_gg_totals t = psx_gg_edges(lens, edges, E, guides, ep.data());
    if (t.live == 0) {
        for (int e = 0; e < E; e++) edge_counts[e] = 0;
        *count = 0;
        return PSX_OK;
    }
    const bool mutual = (opts->flags & PSX_PAIRS_MUTUAL) != 0;

    // ---- sizes: the grids, the tables, the results ----
    const long long FB = t.fblocks, BB = mutual ? t.bblocks : 0, all_pairs = t.frows;
    if (FB * 64 > INT_MAX || BB * 64 > INT_MAX) return PSX_ERR_NOMEM;
    const size_t edges_b = sizeof(GGEdge) * (size_t)E, fblk_b = pad16(sizeof(int2) * (size_t)FB), bblk_b = pad16(sizeof(int2) * (size_t)BB);
    const size_t blob_b = edges_b + fblk_b + bblk_b;
    const size_t nrec = host_pairs ? (size_t)(capacity < all_pairs ? capacity : all_pairs) : 0;
    const size_t off_counts = 16, off_rec = off_counts + pad16(sizeof(int) * (size_t)E), off_blob = off_rec + 16 * nrec;

    if (hipSetDevice(device) != hipSuccess) return PSX_ERR_HIP;
    MatchScratch& sc = psx_match_scratch();
    if (!sc.bind(device)) return PSX_ERR_HIP;
    // every buffer before the first launch: nothing is reallocated under queued work
    if (!sc.need(MS_GGRAPH_TABLES, blob_b) || !sc.need(MS_GGRAPH_FWD, sizeof(int) * 5 * (size_t)all_pairs) ||
        (mutual && (!sc.need(MS_GGRAPH_BWD, sizeof(int) * 5 * (size_t)t.brows) || !sc.need(MS_GGRAPH_LINES, sizeof(float4) * (size_t)all_pairs))) ||
        !sc.need(MS_GGRAPH_TOT, sizeof(int) * (2 * (size_t)FB + 1)) || !sc.need_pinned(off_blob + blob_b))
        return PSX_ERR_NOMEM;
    void* dev_pin = nullptr;
    if (hipHostGetDevicePointer(&dev_pin, sc.hpin, 0) != hipSuccess || dev_pin == nullptr) return PSX_ERR_HIP;
    char* hp = static_cast<char*>(sc.hpin);

    // ---- the tables, written into the pinned staging buffer and copied on the stream ----
    {
        GGEdge* he = reinterpret_cast<GGEdge*>(hp + off_blob);
        for (int e = 0; e < E; e++) {
            const psx_gg_edge& p = ep[(size_t)e];
            const bool live = p.l_len > 0;
            he[e] = GGEdge{live ? d_sets[p.left] : nullptr, live ? reinterpret_cast<const float2*>(d_xys[p.left]) : nullptr,
                           live ? d_sets[p.right] : nullptr, live ? reinterpret_cast<const float2*>(d_xys[p.right]) : nullptr,
                           p.l_len, p.r_len, p.foff, p.boff, guides[e], 0};
        }
        psx_gg_blocks(ep.data(), E, 0, reinterpret_cast<psx_graph_wg*>(hp + off_blob + edges_b), FB);
        if (mutual) psx_gg_blocks(ep.data(), E, 1, reinterpret_cast<psx_graph_wg*>(hp + off_blob + edges_b + fblk_b), BB);
    }
    int* h_total = reinterpret_cast<int*>(hp);
    *h_total = -1;
    memset(hp + off_counts, 0, sizeof(int) * (size_t)E);            // an edge without rows has no workgroup to write its count
    const char* tb = static_cast<const char*>(sc.buf[MS_GGRAPH_TABLES]);
    const GGEdge* t_edges = reinterpret_cast<const GGEdge*>(tb);
    const int2* t_fblk = reinterpret_cast<const int2*>(tb + edges_b);
    const int2* t_bblk = reinterpret_cast<const int2*>(tb + edges_b + fblk_b);
    int* d_fwd = static_cast<int*>(sc.buf[MS_GGRAPH_FWD]);
    int* d_bwd = mutual ? static_cast<int*>(sc.buf[MS_GGRAPH_BWD]) : nullptr;
    float4* d_lines = mutual ? static_cast<float4*>(sc.buf[MS_GGRAPH_LINES]) : nullptr;
    int* d_tot = static_cast<int*>(sc.buf[MS_GGRAPH_TOT]);
    int* d_offs = d_tot + FB;
    int* d_total = static_cast<int*>(dev_pin);
    int* d_counts = reinterpret_cast<int*>(static_cast<char*>(dev_pin) + off_counts);
    // the kernel's capacity for the host form is the staging buffer's (nrec <= capacity)
    int4* out = host_pairs ? reinterpret_cast<int4*>(static_cast<char*>(dev_pin) + off_rec) : static_cast<int4*>(d_pairs);
    const int cap = host_pairs ? (int)nrec : capacity;
    const int mflag = mutual ? 1 : 0;
    hipStream_t st = sc.stream;

    if (hipMemcpyAsync(sc.buf[MS_GGRAPH_TABLES], hp + off_blob, blob_b, hipMemcpyHostToDevice, st) != hipSuccess) return PSX_ERR_HIP;
    if (mutual) {
        hipLaunchKernelGGL(k_gg_lines<T>, dim3((unsigned)FB), dim3(256), 0, st, t_edges, t_fblk, d_lines);
        hipLaunchKernelGGL((k_gg_match<T, true>), dim3((unsigned)(BB * 64)), dim3(256), 0, st, t_edges, t_bblk, static_cast<const float4*>(d_lines), d_bwd);
    }
    hipLaunchKernelGGL((k_gg_match<T, false>), dim3((unsigned)(FB * 64)), dim3(256), 0, st, t_edges, t_fblk, static_cast<const float4*>(nullptr), d_fwd);
    hipLaunchKernelGGL((k_gg_count<T, D>), dim3((unsigned)FB), dim3(256), 0, st, t_edges, t_fblk, d_fwd, d_bwd, opts->ratio, mflag, d_tot);
    hipLaunchKernelGGL(k_gg_scan, dim3(1), dim3(1024), 0, st, d_tot, (int)FB, d_offs);
    hipLaunchKernelGGL((k_gg_write<T, D>), dim3((unsigned)FB), dim3(256), 0, st, t_edges, t_fblk, d_fwd, d_bwd, opts->ratio, mflag, d_offs, out, cap,
                       d_counts, d_total);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return PSX_ERR_HIP;
    const int n = *h_total;
    if (n < 0 || n > all_pairs) return PSX_ERR_HIP;
    memcpy(edge_counts, hp + off_counts, sizeof(int) * (size_t)E);
    if (host_pairs && n > 0 && nrec > 0) memcpy(host_pairs, hp + off_rec, 16 * ((size_t)n < nrec ? (size_t)n : nrec));
    *count = n;
    return PSX_OK;
}

template int psx_guided_edges_run<unsigned char>(int, const unsigned char* const*, const float* const*, const int*, const psx_view_edge*, int,
                                                  const psx_guide*, const psx_match_opts*, void*, void*, int, int*, int*);
template int psx_guided_edges_run<float>(int, const float* const*, const float* const*, const int*, const psx_view_edge*, int, const psx_guide*,
                                         const psx_match_opts*, void*, void*, int, int*, int*);

namespace {

// the edge list's entry: its argument checks, then the driver
template <class T>
int match_pairs_guided_graph(int device, const T* const* d_sets, const float* const* d_xys, const int* lens, int n_sets,
                             const psx_view_edge* edges, int n_edges, const psx_guide* guides, const psx_match_opts* opts, void* host_pairs,
                             void* d_pairs, int capacity, int* edge_counts, int* count)
{
    if (!psx_gg_args_ok(d_sets, d_xys, lens, n_sets, edges, n_edges, guides, opts, host_pairs ? host_pairs : d_pairs, capacity, edge_counts, count))
        return PSX_ERR_INVALID;
    return psx_guided_edges_run(device, d_sets, d_xys, lens, edges, n_edges, guides, opts, host_pairs, d_pairs, capacity, edge_counts, count);
}

} // namespace

extern "C" int psx_match_pairs_guided_graph_u8(int device, const unsigned char* const* d_sets, const float* const* d_xys, const int* lens,
                                               int n_sets, const psx_view_edge* edges, int n_edges, const psx_guide* guides,
                                               const psx_match_opts* opts, psx_match_pair_u8* host_pairs, int capacity, int* edge_counts,
                                               int* count)
{
    return match_pairs_guided_graph(device, d_sets, d_xys, lens, n_sets, edges, n_edges, guides, opts, host_pairs, nullptr, capacity, edge_counts,
                                    count);
}

extern "C" int psx_match_pairs_guided_graph_u8_dev(int device, const unsigned char* const* d_sets, const float* const* d_xys, const int* lens,
                                                   int n_sets, const psx_view_edge* edges, int n_edges, const psx_guide* guides,
                                                   const psx_match_opts* opts, psx_match_pair_u8* d_pairs, int capacity, int* edge_counts,
                                                   int* count)
{
    return match_pairs_guided_graph(device, d_sets, d_xys, lens, n_sets, edges, n_edges, guides, opts, nullptr, d_pairs, capacity, edge_counts,
                                    count);
}

extern "C" int psx_match_pairs_guided_graph(int device, const float* const* d_sets, const float* const* d_xys, const int* lens, int n_sets,
                                            const psx_view_edge* edges, int n_edges, const psx_guide* guides, const psx_match_opts* opts,
                                            psx_match_pair* host_pairs, int capacity, int* edge_counts, int* count)
{
    return match_pairs_guided_graph(device, d_sets, d_xys, lens, n_sets, edges, n_edges, guides, opts, host_pairs, nullptr, capacity, edge_counts,
                                    count);
}

extern "C" int psx_match_pairs_guided_graph_dev(int device, const float* const* d_sets, const float* const* d_xys, const int* lens, int n_sets,
                                                const psx_view_edge* edges, int n_edges, const psx_guide* guides, const psx_match_opts* opts,
                                                psx_match_pair* d_pairs, int capacity, int* edge_counts, int* count)
{
    return match_pairs_guided_graph(device, d_sets, d_xys, lens, n_sets, edges, n_edges, guides, opts, nullptr, d_pairs, capacity, edge_counts,
                                    count);
}
