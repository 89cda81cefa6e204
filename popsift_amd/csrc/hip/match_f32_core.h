// match_f32_core.h -- the device pieces of the float matcher that more than one translation unit states: match.hip (one
// pair of sets) and match_many_f32.hip (one set against many).  The running top-2 under the reference's scan order, the
// permuted layout and the reference's operation tree of the exact scan, and the constants, the f16 conversion, the scale
// rule and the error margin of the MFMA prefilter.  The derivations are in match.hip's header and in the comment block
// above its k_match_mfma; nothing here launches anything.  Internal linkage: one copy per including translation unit.
#pragma once

#include "psx_internal.h"

namespace {

typedef float v2f __attribute__((ext_vector_type(2)));

struct Top2 { float d1, d2; int i1, i2; };

// two smallest under (distance, index) lexicographic order == result of the reference's sequential scan
__device__ __forceinline__ void top2_insert(Top2& t, float d, int i)
{
    if (d < t.d1) { t.d2 = t.d1; t.i2 = t.i1; t.d1 = d; t.i1 = i; }
    else if (d < t.d2) { t.d2 = d; t.i2 = i; }
}

__device__ __forceinline__ v2f pk_fma2(v2f a, v2f b, v2f c) { return __builtin_elementwise_fma(a, b, c); }

// Descriptors are permuted once so that the two partial sums computed together sit in one register /
// SGPR pair: pair k = c*16 + m (component c of float4 m and of float4 m+16) = (v[4m+c], v[4(m+16)+c]).
__device__ __forceinline__ int perm_src(int k, int half) { return 4 * ((k & 15) + 16 * half) + (k >> 4); }

// distance of this lane's left descriptor (64 permuted pairs) to the wave-uniform, permuted right
// descriptor r: P_m = (p_m, p_{m+16}) for m = 0..15, two partial sums per packed instruction
__device__ __forceinline__ float l2_tree(const v2f* l, const float* __restrict__ r)
{
    float a[16];
#pragma unroll
    for (int m = 0; m < 16; m++) {
        const v2f rx = {r[2 * m], r[2 * m + 1]},           ry = {r[32 + 2 * m], r[32 + 2 * m + 1]};
        const v2f rz = {r[64 + 2 * m], r[64 + 2 * m + 1]}, rw = {r[96 + 2 * m], r[96 + 2 * m + 1]};
        const v2f x = l[m] - rx, y = l[16 + m] - ry, z = l[32 + m] - rz, w = l[48 + m] - rw;
        v2f p = y * y;
        p = pk_fma2(x, x, p);
        p = pk_fma2(z, z, p);
        p = pk_fma2(w, w, p);
        a[m] = p.x + p.y;                                  // a_m = p_m + p_{m+16}
    }
    float b[8], c[4], d[2];
#pragma unroll
    for (int i = 0; i < 8; i++) b[i] = a[i] + a[i + 8];
#pragma unroll
    for (int i = 0; i < 4; i++) c[i] = b[i] + b[i + 4];
#pragma unroll
    for (int i = 0; i < 2; i++) d[i] = c[i] + c[i + 2];
    return d[0] + d[1];
}

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int MF_SEGS = 32;                  // candidate segments per left descriptor: one per (chunk of the right side, half wave) ...
constexpr int MF_SEGCAP = 32;                // ... of this many slots: private to one lane of one workgroup, so appending needs no atomic
constexpr int MF_CAP = MF_SEGS * MF_SEGCAP;  // (a returned global atomic per candidate made the scan wait ~1 us per tile and column set)
constexpr int MF_TILE = 32;                  // right descriptors per MFMA tile
constexpr int MF_SUB = 2;                    // MFMA tiles per staged block (= per barrier)
constexpr int MF_ROW = 272;                  // bytes per staged right descriptor: 256 + 16 (rows 4 banks apart: conflict-free b128 reads)
constexpr int MF_SEED = 2048;                // right descriptors of the seeding pass ...
constexpr int MF_SEEDCH = 8;                 // ... in this many chunks (workgroups per 256 left descriptors)
constexpr int MF_MAXSLOTS = 64;              // the largest squared norm of the right side is kept in 64 slots (same-address atomics serialise)

__device__ __forceinline__ unsigned short to_f16(float f)
{
    const _Float16 h = (_Float16)f;                                                // v_cvt_f16_f32: round to nearest even
    unsigned short b; __builtin_memcpy(&b, &h, 2);
    return b;
}

// par[0] = 2^k, par[1] = -2 / 4^k, par[2] = Rmax^2, par[3] = M; *bad = 1 when the prefilter cannot be used
__device__ __forceinline__ void match_scale(float l2, float r2, float* par, int* bad)
{
    const float m2 = fmaxf(l2, r2);
    // finite, positive, and far enough from both ends of the float range for the squares below
    if (!(l2 == l2) || !(r2 == r2) || !(m2 > 1e-30f) || !(m2 < 1e30f)) { *bad = 1; par[0] = 1.0f; par[1] = -2.0f; par[2] = 0.0f; par[3] = 0.0f; return; }
    const float M = sqrtf(m2);
    const int k = (int)floorf(log2f(16384.0f / M));
    *bad = 0;
    par[0] = ldexpf(1.0f, k);
    par[1] = ldexpf(-2.0f, -2 * k);
    par[2] = r2;
    par[3] = M;
}

// E_l of the prefilter's proof (match.hip, above k_match_mfma): the bound of |s - d| for a row of squared norm nl against
// any row of norm <= rmax (rmax2 = rmax^2), bigM >= every norm involved
__device__ __forceinline__ float match_margin(float nl, float rmax, float rmax2, float bigM)
{
    const float E = 0.00197f * sqrtf(nl) * rmax + 2e-7f * bigM * (sqrtf(nl) + rmax) + 4e-5f * (nl + rmax2);
    return E;
}

// (distance, index) lexicographic order: what the reference's sequential scan with strict '<' yields
__device__ __forceinline__ bool lex_less(float d, int i, float e, int j) { return d < e || (d == e && i < j); }
__device__ __forceinline__ void top2_insert_lex(Top2& t, float d, int i)
{
    if (!(d == d)) return;                                   // NaN never passes the reference's '<'
    if (lex_less(d, i, t.d1, t.i1)) { t.d2 = t.d1; t.i2 = t.i1; t.d1 = d; t.i1 = i; }
    else if (lex_less(d, i, t.d2, t.i2)) { t.d2 = d; t.i2 = i; }
}

} // namespace
