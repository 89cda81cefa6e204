// match_many_join.h -- the segmented pair join of the one-to-many searches, stated once: psx_match_pairs_many_u8
// (match_many.hip) and psx_match_pairs_many (match_many_f32.hip) queue it behind their directed passes.  (The guided
// one-to-many call is a star handed to the edge list's driver, match_guided_graph.hip, and is joined there.)
//
// What it reads: fwd, K directed results (match_scratch.h) of 5 l_len ints each, set k's at fwd + 5 l_len k; bwd (with
// the cross-check), the K sets' backward results, set k's at bwd + 5 * (its first row among all right rows); and of a
// set table entry `Set` only `len` and `roff`.  A set with len 0 -- empty, or skipped by its caller -- has no pairs and no
// results: nothing of it is read.
//   k_many_count   the rule of match_rule.h per (set, left) with the gather into set k's backward rows and the
//                  compaction of wg_compact.h: one total per workgroup in set-major order
//   k_many_scan    an exclusive scan of the totals by ONE workgroup (K x blocks totals: every workgroup summing all
//                  earlier ones, as k_pairs_write does, would be quadratic)
//   k_many_write   one 16-byte store per survivor at (offset of its workgroup) + (its offset within the workgroup), the
//                  per-set counts and the total
// Device code and its launcher; the kernels have internal linkage, one copy per including translation unit.
#pragma once

#include "match_rule.h"
#include "match_scratch.h"
#include "wg_compact.h"

namespace {

__device__ __forceinline__ int many_bits(float d) { return __float_as_int(d); }
__device__ __forceinline__ int many_bits(int d) { return d; }

// The rule of match_rule.h for left row i against set k.  Dist: the directed results' distance type (int: the byte
// matchers, float: match_many_f32.hip); the record carries the distance's bits either way.
template <class Dist, class Set>
__device__ __forceinline__ bool many_rule(const Set* __restrict__ sets, const int* __restrict__ fwd, int l_len,
                                          const int* __restrict__ bwd, int k, int i, float ratio, int mutual, int4& rec)
{
    const Set s = sets[k];
    if (i >= l_len || s.len == 0) return false;
    int j;
    Dist d1, d2;
    psx_directed_load<Dist>(fwd + 5 * (size_t)l_len * k, l_len, i, j, d1, d2);
    bool keep = psx_match_keep(psx_match_dist(d1), psx_match_dist(d2), ratio);
    if (keep && mutual) keep = psx_directed_best(bwd + 5 * (size_t)s.roff, j) == i;
    rec = make_int4(i, j, many_bits(d1), many_bits(d2));
    return keep;
}

// grid K * nb (nb = blocks of 256 left rows), workgroup k * nb + b: set-major, so the offsets are the concatenation's
template <class Dist, class Set>
__global__ __launch_bounds__(256) void k_many_count(const Set* __restrict__ sets, const int* __restrict__ fwd, int l_len,
                                                    const int* __restrict__ bwd, int nb, float ratio, int mutual,
                                                    int* __restrict__ wg_tot)
{
    const int k = (int)(blockIdx.x / (unsigned)nb), b = (int)(blockIdx.x % (unsigned)nb);
    int4 rec;
    const bool keep = many_rule<Dist>(sets, fwd, l_len, bwd, k, b * 256 + (int)threadIdx.x, ratio, mutual, rec);
    __shared__ int s_cnt[4];
    wg_count(__ballot(keep), s_cnt);
    if (threadIdx.x == 0) wg_tot[blockIdx.x] = wg_total(s_cnt);
}

// ONE workgroup of 1024 threads: offs[w] = the totals before workgroup w, offs[n] = all of them (wg_compact.h)
__global__ __launch_bounds__(1024) void k_many_scan(const int* __restrict__ wg_tot, int n, int* __restrict__ offs)
{
    wg_scan_totals(wg_tot, n, offs);
}

// grid as k_many_count.  Evaluates the rule again (k_pairs_write: cheaper than parking the verdicts), ranks its lanes and
// writes each surviving record with ONE 16-byte store at offs[workgroup] + rank, never at or past capacity; a set's first
// workgroup writes the set's count, workgroup 0 the total.
template <class Dist, class Set>
__global__ __launch_bounds__(256) void k_many_write(const Set* __restrict__ sets, const int* __restrict__ fwd, int l_len,
                                                    const int* __restrict__ bwd, int nb, float ratio, int mutual,
                                                    const int* __restrict__ offs, int4* __restrict__ out, int capacity,
                                                    int* __restrict__ set_counts, int* __restrict__ total)
{
    const int k = (int)(blockIdx.x / (unsigned)nb), b = (int)(blockIdx.x % (unsigned)nb);
    int4 rec = make_int4(0, 0, 0, 0);
    const bool keep = many_rule<Dist>(sets, fwd, l_len, bwd, k, b * 256 + (int)threadIdx.x, ratio, mutual, rec);
    const unsigned long long m = __ballot(keep);
    __shared__ int s_cnt[4];
    wg_count(m, s_cnt);
    const int pos = offs[blockIdx.x] + wg_offset(m, s_cnt);
    if (keep && pos < capacity) out[pos] = rec;
    if (threadIdx.x == 0) {
        if (b == 0) set_counts[k] = offs[(size_t)(k + 1) * nb] - offs[(size_t)k * nb];
        if (blockIdx.x == 0) *total = offs[gridDim.x];
    }
}

// Queues the three kernels on st.  nb = blocks of 256 left rows, ntot = K * nb workgroups (the caller has checked that
// ntot + 1 fits an int); d_tot: room for 2 ntot + 1 ints (the totals, then their offsets); bwd is read only with mutual.
template <class Dist, class Set>
void psx_many_join_queue(hipStream_t st, const Set* d_sets, const int* d_fwd, int l_len, const int* d_bwd, int nb, int ntot,
                         float ratio, bool mutual, int* d_tot, int4* out, int capacity, int* d_counts, int* d_total)
{
    int* d_offs = d_tot + ntot;
    const int mflag = mutual ? 1 : 0;
    hipLaunchKernelGGL((k_many_count<Dist, Set>), dim3((unsigned)ntot), dim3(256), 0, st, d_sets, d_fwd, l_len, d_bwd, nb, ratio, mflag, d_tot);
    hipLaunchKernelGGL(k_many_scan, dim3(1), dim3(1024), 0, st, d_tot, ntot, d_offs);
    hipLaunchKernelGGL((k_many_write<Dist, Set>), dim3((unsigned)ntot), dim3(256), 0, st, d_sets, d_fwd, l_len, d_bwd, nb, ratio, mflag,
                       d_offs, out, capacity, d_counts, d_total);
}

} // namespace
