// match_graph_join.h -- the pair join of the searches over an edge list, segmented by edge and stated once:
// psx_match_pairs_graph_u8 (match_graph.hip) and psx_match_pairs_graph (match_graph_f32.hip) queue it behind their
// directed passes, as match_many_join.h is queued by the two one-to-many searches.
//
// What it reads: the edge table of match_graph_plan.h (psx_graph_edge: an edge's left set and its first forward /
// backward row among all edges' rows), the forward {edge, row0} table in edge-major order, the directed results
// (match_scratch.h) of all edges, edge e's forward one at fwd + 5 foff_e over its OWN left length and its backward one
// at bwd + 5 boff_e, and of a set table entry `Set` only `len`.  Dist: the directed results' distance type (int: the byte
// matcher, float: the float one); the record carries the distance's bits either way.
//   k_graph_count   the rule of match_rule.h (psx_match_keep) and the backward gather, counted per workgroup (wg_compact.h)
//   k_graph_scan    one scan of the totals (wg_scan_totals)
//   k_graph_write   one 16-byte store per survivor, the per-edge counts and the total
// The workgroups come from the {edge, row0} table in edge-major order, so the offsets are the concatenation's.  Nothing
// depends on arrival order.  Device code and its launcher; the kernels have internal linkage, one copy per including
// translation unit.
#pragma once

#include "match_graph_plan.h"
#include "match_rule.h"
#include "match_scratch.h"
#include "wg_compact.h"

namespace {

__device__ __forceinline__ int graph_bits(float d) { return __float_as_int(d); }
__device__ __forceinline__ int graph_bits(int d) { return d; }

// The rule of match_rule.h for left row i of edge e, whose left set has l_len rows: the edge's forward result, and with the
// cross-check the gather into the edge's backward rows.
template <class Dist>
__device__ __forceinline__ bool graph_rule(const psx_graph_edge& e, int l_len, const int* __restrict__ fwd, const int* __restrict__ bwd,
                                           int i, float ratio, int mutual, int4& rec)
{
    if (i >= l_len) return false;
    int j;
    Dist d1, d2;
    psx_directed_load<Dist>(fwd + 5 * (size_t)e.foff, l_len, i, j, d1, d2);
    bool keep = psx_match_keep(psx_match_dist(d1), psx_match_dist(d2), ratio);
    if (keep && mutual) keep = psx_directed_best(bwd + 5 * (size_t)e.boff, j) == i;
    rec = make_int4(i, j, graph_bits(d1), graph_bits(d2));
    return keep;
}

// grid: the forward {edge, row0} table, edge-major: one total per workgroup
template <class Dist, class Set>
__global__ __launch_bounds__(256) void k_graph_count(const Set* __restrict__ sets, const psx_graph_edge* __restrict__ edges,
                                                     const int2* __restrict__ wgs, const int* __restrict__ fwd, const int* __restrict__ bwd,
                                                     float ratio, int mutual, int* __restrict__ wg_tot)
{
    const int2 wg = wgs[blockIdx.x];
    const psx_graph_edge e = edges[wg.x];
    int4 rec;
    const bool keep = graph_rule<Dist>(e, sets[e.left].len, fwd, bwd, wg.y + (int)threadIdx.x, ratio, mutual, rec);
    __shared__ int s_cnt[4];
    wg_count(__ballot(keep), s_cnt);
    if (threadIdx.x == 0) wg_tot[blockIdx.x] = wg_total(s_cnt);
}

// ONE workgroup of 1024 threads: offs[w] = the totals before workgroup w, offs[n] = all of them (wg_compact.h)
__global__ __launch_bounds__(1024) void k_graph_scan(const int* __restrict__ wg_tot, int n, int* __restrict__ offs)
{
    wg_scan_totals(wg_tot, n, offs);
}

// grid as k_graph_count.  Evaluates the rule again, ranks its lanes and writes each surviving record with ONE 16-byte store
// at offs[workgroup] + rank, never at or past capacity; an edge's first workgroup writes the edge's count (an edge without
// workgroups keeps the zero the host put there), workgroup 0 the total.
template <class Dist, class Set>
__global__ __launch_bounds__(256) void k_graph_write(const Set* __restrict__ sets, const psx_graph_edge* __restrict__ edges,
                                                     const int2* __restrict__ wgs, const int* __restrict__ fwd, const int* __restrict__ bwd,
                                                     float ratio, int mutual, const int* __restrict__ offs, int4* __restrict__ out,
                                                     int capacity, int* __restrict__ edge_counts, int* __restrict__ total)
{
    const int2 wg = wgs[blockIdx.x];
    const psx_graph_edge e = edges[wg.x];
    const int l_len = sets[e.left].len;
    int4 rec = make_int4(0, 0, 0, 0);
    const bool keep = graph_rule<Dist>(e, l_len, fwd, bwd, wg.y + (int)threadIdx.x, ratio, mutual, rec);
    const unsigned long long m = __ballot(keep);
    __shared__ int s_cnt[4];
    wg_count(m, s_cnt);
    const int pos = offs[blockIdx.x] + wg_offset(m, s_cnt);
    if (keep && pos < capacity) out[pos] = rec;
    if (threadIdx.x == 0) {
        if (wg.y == 0) edge_counts[wg.x] = offs[blockIdx.x + (unsigned)((l_len + 255) / 256)] - offs[blockIdx.x];
        if (blockIdx.x == 0) *total = offs[gridDim.x];
    }
}

// Queues the three kernels on st.  nwg = the entries of the forward {edge, row0} table (the caller has checked that
// nwg + 1 fits an int); d_tot: room for 2 nwg + 1 ints (the totals, then their offsets); bwd is read only with mutual.
template <class Dist, class Set>
void psx_graph_join_queue(hipStream_t st, const Set* d_sets, const psx_graph_edge* d_edges, const int2* d_wgs, const int* d_fwd,
                          const int* d_bwd, int nwg, float ratio, bool mutual, int* d_tot, int4* out, int capacity, int* d_counts,
                          int* d_total)
{
    int* d_offs = d_tot + nwg;
    const int mflag = mutual ? 1 : 0;
    hipLaunchKernelGGL((k_graph_count<Dist, Set>), dim3((unsigned)nwg), dim3(256), 0, st, d_sets, d_edges, d_wgs, d_fwd, d_bwd, ratio, mflag, d_tot);
    hipLaunchKernelGGL(k_graph_scan, dim3(1), dim3(1024), 0, st, d_tot, nwg, d_offs);
    hipLaunchKernelGGL((k_graph_write<Dist, Set>), dim3((unsigned)nwg), dim3(256), 0, st, d_sets, d_edges, d_wgs, d_fwd, d_bwd, ratio, mflag,
                       d_offs, out, capacity, d_counts, d_total);
}

} // namespace
