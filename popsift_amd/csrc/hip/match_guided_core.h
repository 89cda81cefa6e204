// match_guided_core.h -- the guided directed search of ONE outer descriptor by one wave, stated once: k_match_guided
// (match_guided.hip) hands it the operands of a single call, k_gg_match (match_guided_graph.hip) those of one
// entry of its edge table.  Device code only; the dataflow is described at the top of match_guided.hip.
#pragma once

#include "psx_internal.h"
#include "guide_rule.h"
#include "match_rule.h"
#include "match_scratch.h"

#include <climits>
#include <type_traits>

constexpr int G_NOIDX = 0x7fffffff;          // larger than any real index: an empty slot loses every tie

template <class D> struct GTop2 { D d1, d2; int i1, i2; };

__device__ __forceinline__ float g_none(float) { return INFINITY; }
__device__ __forceinline__ int g_none(int) { return INT_MAX; }

// two smallest under (distance, index) order == the reference's sequential scan with strict '<' over the admissible
// right descriptors in ascending index.  A NaN or +inf distance never passes that '<': it is not a neighbour.
template <class D>
__device__ __forceinline__ void g_insert(GTop2<D>& t, D d, int i)
{
    if (!(d < g_none(d))) return;
    if (d < t.d1 || (d == t.d1 && i < t.i1)) { t.d2 = t.d1; t.i2 = t.i1; t.d1 = d; t.i1 = i; }
    else if (d < t.d2 || (d == t.d2 && i < t.i2)) { t.d2 = d; t.i2 = i; }
}

// this lane's piece of descriptor `idx`: lane t of a half wave holds floats / bytes 4t..4t+3
__device__ __forceinline__ float4 g_row(const float* __restrict__ p, int idx, int tl)
{
    return reinterpret_cast<const float4*>(p + (size_t)idx * 128)[tl];
}
__device__ __forceinline__ unsigned g_row(const unsigned char* __restrict__ p, int idx, int tl)
{
    return reinterpret_cast<const unsigned*>(p + (size_t)idx * 128)[tl];
}

// the pair's squared distance, in every lane of the half wave.  Floats: the operation tree of k_match_exact.
__device__ __forceinline__ float g_dist(const float4& l, const float4& r)
{
    const float qx = l.x - r.x, qy = l.y - r.y, qz = l.z - r.z, qw = l.w - r.w;
    float v = fmaf(qw, qw, fmaf(qz, qz, fmaf(qx, qx, qy * qy)));
    v += __shfl_down(v, 16, 32); v += __shfl_down(v, 8, 32); v += __shfl_down(v, 4, 32);
    v += __shfl_down(v, 2, 32);  v += __shfl_down(v, 1, 32);
    return __shfl(v, 0, 32);
}
// Bytes: integers, exact in any order (at most 128 * 255^2 < 2^23)
__device__ __forceinline__ int g_dist(unsigned l, unsigned r)
{
    int s = 0;
#pragma unroll
    for (int b = 0; b < 4; b++) { const int x = (int)((l >> (8 * b)) & 0xffu) - (int)((r >> (8 * b)) & 0xffu); s += x * x; }
    s += __shfl_xor(s, 16, 32); s += __shfl_xor(s, 8, 32); s += __shfl_xor(s, 4, 32);
    s += __shfl_xor(s, 2, 32);  s += __shfl_xor(s, 1, 32);
    return s;
}

constexpr int G_K = 2;                       // pairs per half wave and round

__device__ __forceinline__ bool g_allowed(int kind, const psx_guide_line& mine, const float2& outer_xy, const float2& p)
{
    return psx_guide_right(kind, mine, p.x, p.y);               // forward: the wave's own line, the inner (right) point
}
__device__ __forceinline__ bool g_allowed(int kind, const psx_guide_line&, const float2& outer_xy, const float4& p)
{
    const psx_guide_line l = {p.x, p.y, p.z, p.w};              // backward: the inner (left) point's line, the wave's own point
    return psx_guide_right(kind, l, outer_xy.x, outer_xy.y);
}

// The calling wave searches outer descriptor oi (wave uniform; a wave with oi >= o_len does nothing: the caller has no
// barrier behind this).  inner_geo: forward (SWAP = false) the inner side's positions (float2), backward the inner
// side's lines (float4, the first step of the rule per left point).  out: the directed result of the o_len outer rows --
// 3 o_len ints (best, second, accept), then 2 o_len distances (D), as the directed matchers of match.hip leave them.
template <class T, class D, bool SWAP>
__device__ __forceinline__ void g_match_row(const T* __restrict__ outer, const float2* __restrict__ outer_xy, int o_len, int oi,
                                            const T* __restrict__ inner, const void* __restrict__ inner_geo, int i_len,
                                            const psx_guide& g, int* __restrict__ out)
{
    typedef typename std::conditional<SWAP, float4, float2>::type Geo;
    const Geo* __restrict__ geo = static_cast<const Geo*>(inner_geo);
    const int lane = threadIdx.x & 63, tl = lane & 31, half = lane >> 5;
    if (oi >= o_len) return;                                   // whole waves leave
    const auto orow = g_row(outer, oi, tl);
    const float2 op = outer_xy[oi];
    const psx_guide_line mine = psx_guide_left(g.kind, g.m, g.tol, op.x, op.y);       // used forward only
    GTop2<D> t = {g_none(D()), g_none(D()), G_NOIDX, G_NOIDX};
    Geo nxt = Geo();
    if (lane < i_len) nxt = geo[lane];
    for (int base = 0; base < i_len; base += 64) {
        const int j = base + lane;
        const Geo p = nxt;
        if (j + 64 < i_len) nxt = geo[j + 64];                 // the next step's records are in flight during this one
        const bool ok = j < i_len && g_allowed(g.kind, mine, op, p);
        unsigned long long m = __ballot(ok);                   // wave uniform: so is every trip count below
        while (m != 0ull) {
            // the set bits in ascending index, dealt to the halves in turn; a slot past the last bit is -1
            int idx[G_K];
#pragma unroll
            for (int k = 0; k < G_K; k++) {
                int b0 = -1, b1 = -1;
                if (m != 0ull) { b0 = __builtin_ctzll(m); m &= m - 1ull; }
                if (m != 0ull) { b1 = __builtin_ctzll(m); m &= m - 1ull; }
                const int b = half ? b1 : b0;
                idx[k] = b < 0 ? -1 : base + b;
            }
            // i_len >= 1 inside this loop: an empty slot reads row 0 and drops the value
            decltype(g_row(inner, 0, 0)) r[G_K];
#pragma unroll
            for (int k = 0; k < G_K; k++) r[k] = g_row(inner, idx[k] < 0 ? 0 : idx[k], tl);
#pragma unroll
            for (int k = 0; k < G_K; k++) {
                const D d = g_dist(orow, r[k]);
                if (idx[k] >= 0) g_insert(t, d, idx[k]);
            }
        }
    }
    {   // the two halves hold disjoint subsets of the admissible set: merge
        const D od1 = __shfl_xor(t.d1, 32), od2 = __shfl_xor(t.d2, 32);
        const int oi1 = __shfl_xor(t.i1, 32), oi2 = __shfl_xor(t.i2, 32);
        g_insert(t, od1, oi1);
        g_insert(t, od2, oi2);
    }
    if (lane == 0) {
        // the reference starts from (inf, inf, index 0, index 0): zero or one admissible inner descriptor leaves them
        const int i1 = t.i1 == G_NOIDX ? 0 : t.i1, i2 = t.i2 == G_NOIDX ? 0 : t.i2;
        const bool accept = psx_match_keep(psx_match_dist(t.d1), psx_match_dist(t.d2), 0.8f);
        psx_directed_store<D>(out, o_len, (size_t)oi, i1, i2, accept, t.d1, t.d2);
    }
}
