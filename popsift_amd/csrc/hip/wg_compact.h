// wg_compact.h -- the stable compaction that the pair join (match.hip), the one-to-many join (match_many.hip) and the
// RANSAC inlier list (ransac.hip) share.  One lane per row, workgroups of 256 threads, two launches: a count kernel leaves
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

// This lane's slot when the survivors before the workgroup are the sum of wg_tot[0 .. blockIdx.x): every workgroup scans
// for itself (at most gridDim.x ints each -- quadratic over the grid, for grids of a few hundred workgroups; k_many_write
// takes its base from a scan kernel instead).  The last workgroup writes the total.
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
