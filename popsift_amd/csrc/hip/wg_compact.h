// wg_compact.h -- the stable compaction that the pair join (match.hip), the one-to-many join (match_many.hip) and the
// RANSAC inlier lists (ransac.hip; ransac_graph.hip, the batched driver of the star and edge-list forms) share.  One lane per row, workgroups of 256 threads, two launches: a count kernel leaves
// one total per workgroup, a write kernel evaluates its rule again and stores each survivor at
//   (survivors of the workgroups before its own) + (survivors of the waves before its own) + (ballot bits below its lane)
// -- ascending row order, no atomics, nothing depends on arrival order.  The kernels keep their own rule and record and
// test `slot < capacity` themselves.  m = __ballot(keep) throughout.
#pragma once

#include <hip/hip_runtime.h>

// set bits of m below this lane
__device__ __forceinline__ int lane_rank(unsigned long long m)
{
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

// every wave's survivors into s_cnt (LDS); holds the compaction's one barrier, the two below read s_cnt after it
__device__ __forceinline__ void wg_count(unsigned long long m, int (&s_cnt)[4])
{
    if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = __popcll(m);
    __syncthreads();
}

__device__ __forceinline__ int wg_total(const int (&s_cnt)[4]) { return s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3]; }

// this lane's offset among the workgroup's survivors
__device__ __forceinline__ int wg_offset(unsigned long long m, const int (&s_cnt)[4])
{
    int woff = 0;
    for (int w = 0; w < (int)(threadIdx.x >> 6); w++) woff += s_cnt[w];
    return woff + lane_rank(m);
}

// The body of a scan kernel of ONE workgroup of 1024 threads (k_many_scan, match_many.hip; k_rgraph_scan,
// ransac_graph.hip): offs[w] = the totals before workgroup w, offs[n] = all of them.  1024 totals per round: a wave scan
// (shuffles), the 16 wave sums through LDS, the carry of the rounds before.
__device__ __forceinline__ void wg_scan_totals(const int* __restrict__ wg_tot, int n, int* __restrict__ offs)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __shared__ int s_wave[16];
    int carry = 0;
    for (int base = 0; base < n; base += 1024) {
        const int w = base + (int)threadIdx.x;
        const int v = w < n ? wg_tot[w] : 0;
        int incl = v;
#pragma unroll
        for (int k = 1; k < 64; k <<= 1) { const int o = __shfl_up(incl, k); if (lane >= k) incl += o; }
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int q = 0; q < 16; q++) { const int t = s_wave[q]; all += t; if (q < wave) before += t; }
        if (w < n) offs[w] = carry + before + incl - v;
        carry += all;
        __syncthreads();                                     // s_wave is rewritten in the next round
    }
    if (threadIdx.x == 0) offs[n] = carry;
}

// This lane's slot when the survivors before the workgroup are the sum of wg_tot[0 .. blockIdx.x): every workgroup scans
// for itself (at most gridDim.x ints each -- quadratic over the grid, for grids of a few hundred workgroups; k_many_write
// and k_rgraph_write take their base from a scan kernel instead).  The last workgroup writes the total.
__device__ __forceinline__ int wg_slot(unsigned long long m, const int* __restrict__ wg_tot, int* __restrict__ total)
{
    __shared__ int s_part[4], s_cnt[4];
    int part = 0;
    for (int b = threadIdx.x; b < (int)blockIdx.x; b += 256) part += wg_tot[b];
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) part += __shfl_xor(part, k);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = part;
    wg_count(m, s_cnt);
    const int base = s_part[0] + s_part[1] + s_part[2] + s_part[3];
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) *total = base + wg_total(s_cnt);
    return base + wg_offset(m, s_cnt);
}
