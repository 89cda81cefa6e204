// match_u8_core.h -- the inline device pieces of the exact byte matcher that its translation units share: k_match_u8
// (match.hip) and k_match_u8_many (match_many.hip).  The key, the operand fragment and the running top-2 are stated once;
// the comment block "Byte descriptors" in match.hip explains them.
#pragma once

#include <hip/hip_runtime.h>

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

constexpr int U8_TILE = 32;                  // right descriptors per MFMA tile
constexpr int U8_CHUNK_MAX = 512;            // right descriptors per chunk: 9 index bits in the key
constexpr unsigned U8_NONE = 0xffffffffu;    // empty key: larger than any real one (d << 9 | 511 < 2^32 - 1)

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
