// match_u8_core.h -- the device pieces of the exact byte matcher, each stated once: the padding of a norm array (u8_pad), a
// row's norm (u8_row_norm), the key and the running top-2 (U8_*, u8_frag, key_insert), a wave's walk over a chunk (U8Wave:
// u8_load_cols, u8_walk, u8_store_keys), the merge of a chunk's keys (U8Best, u8_merge_chunk), the accept decision (u8_accept).
// The kernels of match.hip (one left set against one right set) and match_many.hip (both sides from tables) only say where
// their operands live.  The comment block "Byte descriptors" in match.hip explains the arithmetic.
#pragma once

#include <hip/hip_runtime.h>

#include <climits>

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

constexpr int U8_TILE = 32;                  // right descriptors per MFMA tile
constexpr int U8_CHUNK_MAX = 512;            // right descriptors per chunk: 9 index bits in the key
constexpr unsigned U8_NONE = 0xffffffffu;    // empty key: larger than any real one (d << 9 | 511 < 2^32 - 1)

// Entries of a set's norm array: whole tiles plus one tile of zeros.  u8_walk reads the norms of whole tiles, so an array
// padded by less is read out of bounds: every allocation and every norm kernel takes the figure from here.
__host__ __device__ constexpr unsigned u8_pad(int n) { return (((unsigned)n + U8_TILE - 1) / U8_TILE + 1) * U8_TILE; }

// |x - 128|^2 of row d of a set of n rows, zero for a padding row (d >= n); 8 consecutive lanes per row, q = lane & 7
__device__ __forceinline__ int u8_row_norm(const unsigned char* __restrict__ src, int n, int d, int q)
{
    int ss = 0;
    if (d < n) {
        const uint4 v = reinterpret_cast<const uint4*>(src + (size_t)d * 128)[q];
        const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; k++)
#pragma unroll
            for (int b = 0; b < 4; b++) { const int x = (int)((w[k] >> (8 * b)) & 0xffu) - 128; ss += x * x; }
    }
    ss += __shfl_xor(ss, 4, 8); ss += __shfl_xor(ss, 2, 8); ss += __shfl_xor(ss, 1, 8);
    return ss;
}

__device__ __forceinline__ i32x4 u8_frag(const unsigned char* __restrict__ p)
{
    const uint4 v = *reinterpret_cast<const uint4*>(p);
    return (i32x4){(int)(v.x ^ 0x80808080u), (int)(v.y ^ 0x80808080u), (int)(v.z ^ 0x80808080u), (int)(v.w ^ 0x80808080u)};
}

__device__ __forceinline__ void key_insert(unsigned& m1, unsigned& m2, unsigned k)
{
    m2 = min(m2, max(m1, k));                // m1 <= m2: the median of (m1, m2, k)
    m1 = min(m1, k);
}

// What one wave of a 256-thread workgroup holds while it walks a chunk: 64 outer ("left") rows as two B fragment sets of
// 32 columns -- lane l supplies column l & 31 and the 16 bytes of half l >> 5 of each 32-byte k-step -- their norms and
// row numbers, and per column the two smallest keys so far.
struct U8Wave {
    i32x4 bfrag[2][4];
    int nl[2], lidx[2];
    unsigned m1[2], m2[2];
};

// the wave's 64 outer rows [row0, row0 + 64) of a set of l_len rows (l_len >= 1); idle columns repeat the set's last row
__device__ __forceinline__ void u8_load_cols(U8Wave& w, const unsigned char* __restrict__ left, const int* __restrict__ ln2,
                                             int l_len, int row0)
{
    const int lane = threadIdx.x & 63, col = lane & 31, half = lane >> 5;
#pragma unroll
    for (int c = 0; c < 2; c++) {
        const int li = row0 + c * 32 + col;
        w.lidx[c] = li;
        const int lq = min(li, l_len - 1);
        const unsigned char* lp = left + (size_t)lq * 128 + half * 16;
#pragma unroll
        for (int kk = 0; kk < 4; kk++) w.bfrag[c][kk] = u8_frag(lp + kk * 32);
        w.nl[c] = ln2[lq];
        w.m1[c] = w.m2[c] = U8_NONE;
    }
}

// Inner ("right") rows [r0, r1) of a set of r_len rows in tiles of 32, r1 - r0 <= U8_CHUNK_MAX: A fragments straight from
// global memory (row reads clamped to the set's last row), rn2 = the set's norms, padded as u8_pad says.  A key is
// d << 9 | (row - r0); rows at or past r1 get U8_NONE, so nothing beyond the chunk is ever ranked.
__device__ __forceinline__ void u8_walk(U8Wave& w, const unsigned char* __restrict__ right, const int* __restrict__ rn2,
                                        int r_len, int r0, int r1)
{
    const int lane = threadIdx.x & 63, col = lane & 31, half = lane >> 5;
    for (int base = r0; base < r1; base += U8_TILE) {
        const unsigned char* rp = right + (size_t)min(base + col, r_len - 1) * 128 + half * 16;
        i32x4 a[4];
#pragma unroll
        for (int kk = 0; kk < 4; kk++) a[kk] = u8_frag(rp + kk * 32);
        // this lane's 16 rows: base + 8 g + 4 half + e (the norm arrays are padded by a tile of zeros)
        int nr[16];
#pragma unroll
        for (int g = 0; g < 4; g++) {
            const int4 v = *reinterpret_cast<const int4*>(rn2 + base + 8 * g + 4 * half);
            nr[4 * g] = v.x; nr[4 * g + 1] = v.y; nr[4 * g + 2] = v.z; nr[4 * g + 3] = v.w;
        }
        i32x16 acc[2];
#pragma unroll
        for (int c = 0; c < 2; c++) {
            acc[c] = (i32x16){0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
            for (int kk = 0; kk < 4; kk++) acc[c] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[kk], w.bfrag[c][kk], acc[c], 0, 0, 0);
        }
        const unsigned loc0 = (unsigned)(base - r0 + 4 * half);
        const bool full = base + U8_TILE <= r1;             // wave uniform: only a chunk's last tile can be partial
#pragma unroll
        for (int c = 0; c < 2; c++) {
#pragma unroll
            for (int reg = 0; reg < 16; reg++) {
                const int roff = 8 * (reg >> 2) + (reg & 3);
                const unsigned d = (unsigned)(w.nl[c] + nr[reg] - 2 * acc[c][reg]);
                unsigned key = (d << 9) | (loc0 + (unsigned)roff);
                if (!full && base + 4 * half + roff >= r1) key = U8_NONE;
                key_insert(w.m1[c], w.m2[c], key);
            }
        }
    }
}

// the half waves saw disjoint rows of the same columns: one shuffle, then keys[outer row] = (smallest, second smallest key)
__device__ __forceinline__ void u8_store_keys(U8Wave& w, int l_len, uint2* __restrict__ keys)
{
    const int half = (threadIdx.x & 63) >> 5;
#pragma unroll
    for (int c = 0; c < 2; c++) {
        const unsigned o1 = __shfl_xor(w.m1[c], 32), o2 = __shfl_xor(w.m2[c], 32);
        key_insert(w.m1[c], w.m2[c], o1);
        key_insert(w.m1[c], w.m2[c], o2);
        if (half == 0 && w.lidx[c] < l_len) keys[w.lidx[c]] = make_uint2(w.m1[c], w.m2[c]);
    }
}

// The reference's running result: it starts from (inf, inf, index 0, index 0).  Chunks are merged in index order and a
// chunk's two keys are in (distance, index) order, so strict '<' on the distance reproduces the sequential scan.
struct U8Best { int d1 = INT_MAX, d2 = INT_MAX, i1 = 0, i2 = 0; };

// p: the key pair of a chunk whose first row is r0
__device__ __forceinline__ void u8_merge_chunk(U8Best& t, uint2 p, int r0)
{
    const unsigned k[2] = {p.x, p.y};
#pragma unroll
    for (int e = 0; e < 2; e++) {
        if (k[e] == U8_NONE) continue;
        const int d = (int)(k[e] >> 9), i = r0 + (int)(k[e] & 511u);
        if (d < t.d1) { t.d2 = t.d1; t.i2 = t.i1; t.d1 = d; t.i1 = i; }
        else if (d < t.d2) { t.d2 = d; t.i2 = i; }
    }
}

// accept = d1 / d2 < 0.8 as psx_match decides it: IEEE division (no v_rcp), the integers are exact in float, a missing
// neighbour (INT_MAX) is +inf
__device__ __forceinline__ bool u8_accept(int d1, int d2)
{
    const float f1 = d1 == INT_MAX ? INFINITY : (float)d1, f2 = d2 == INT_MAX ? INFINITY : (float)d2;
    return f1 / f2 < 0.8f;
}
