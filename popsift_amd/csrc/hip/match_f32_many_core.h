// match_f32_many_core.h -- the device pieces of the batched float matchers that more than one translation unit states:
// match_many_f32.hip (one set against many) and match_graph_f32.hip (a list of view pairs).  What a workgroup does with ONE
// block or ONE (outer block, inner chunk) once its kernel has said where the operands live: the permuted copy of a block
// (path A), the norms and the scaled f16 copy of a block, the self-seeding two-phase tile walk of the MFMA prefilter and the
// exact evaluation of a row's candidate segments (path B).  The text is match_many_f32.hip's, moved here unchanged; the
// derivations are in that file's header and in match.hip above k_match_mfma.  Nothing here launches anything or reads a
// table.  Internal linkage: one copy per including translation unit.
#pragma once

#include "match_f32_core.h"

namespace {

// par[0] = 2^k, par[1] = -2 / 4^k, par[2] = the largest squared norm of the right sets, par[3] = M (match_scale),
// par[4] = the largest squared norm of L
constexpr int FPAR = 8;
constexpr int FX_SEGS = 32;                    // candidate segments the exact evaluation gathers per round (4 KB of list per wave)
constexpr int FM_SEEDBLK = 2;                  // staged blocks (of 64 rows) at a chunk's start that seed its running maxima

// ---- path A --------------------------------------------------------------------------------------------------------

// 256 threads: k_match_permute's layout for `rows` rows at src, written at out
__device__ __forceinline__ void fm_permute_block(const float* __restrict__ src, int rows, float2* __restrict__ out)
{
    for (int i = threadIdx.x; i < rows * 64; i += 256) {              // one output pair per step
        const int d = i >> 6, k = i & 63;
        const float* p = src + (size_t)d * 128;
        out[i] = make_float2(p[perm_src(k, 0)], p[perm_src(k, 1)]);
    }
}

// ---- path B --------------------------------------------------------------------------------------------------------

// 256 threads, 32 lanes per row (k_match_norms' sum): norm2[row] for rows [row0, end) of the set at desc, and the block's
// largest at *bmax (bits of a non-negative float; a NaN norm has the bit pattern of a huge unsigned and wins)
__device__ __forceinline__ void fm_norms_block(const float* __restrict__ desc, int row0, int end, float* __restrict__ norm2,
                                               unsigned* __restrict__ bmax)
{
    const int q = threadIdx.x & 31;
    float mx = 0.0f;
    for (int d = row0 + (int)(threadIdx.x >> 5); d < end; d += 8) {
        const float4 v = reinterpret_cast<const float4*>(desc + (size_t)d * 128)[q];
        float ss = fmaf(v.w, v.w, fmaf(v.z, v.z, fmaf(v.y, v.y, v.x * v.x)));
        for (int k = 16; k >= 1; k >>= 1) ss += __shfl_xor(ss, k, 32);
        if (q == 0) norm2[d] = ss;
        mx = __uint_as_float(max(__float_as_uint(mx), __float_as_uint(ss < 0.0f ? 0.0f : ss)));
    }
    __shared__ unsigned s_max;
    if (threadIdx.x == 0) s_max = 0u;
    __syncthreads();
    if (q == 0) atomicMax(&s_max, __float_as_uint(mx));
    __syncthreads();
    if (threadIdx.x == 0) *bmax = s_max;
}

// 256 threads.  The parameters from the blocks' maxima -- bmax[0, br) belong to the right side, [br, br + bl) to the left
// one -- derived by every workgroup itself (k_match_cvt: a 1-thread kernel in between costs a launch); workgroup 0
// publishes them and the flag -- the call's first write of it.  Returns the scale 2^k.
__device__ __forceinline__ float fm_cvt_params(int br, int bl, const unsigned* __restrict__ bmax, float* __restrict__ par, int* __restrict__ flag)
{
    __shared__ unsigned s_r, s_l;
    __shared__ float s_scale;
    if (threadIdx.x == 0) { s_r = 0u; s_l = 0u; }
    __syncthreads();
    unsigned rb = 0u, lb = 0u;
    for (int i = threadIdx.x; i < br + bl; i += 256) { const unsigned v = bmax[i]; if (i < br) rb = max(rb, v); else lb = max(lb, v); }
    for (int k = 32; k >= 1; k >>= 1) { rb = max(rb, (unsigned)__shfl_xor((int)rb, k)); lb = max(lb, (unsigned)__shfl_xor((int)lb, k)); }
    if ((threadIdx.x & 63) == 0) { atomicMax(&s_r, rb); atomicMax(&s_l, lb); }
    __syncthreads();
    if (threadIdx.x == 0) {
        float pp[4]; int bad;
        match_scale(__uint_as_float(s_l), __uint_as_float(s_r), pp, &bad);
        s_scale = pp[0];
        if (blockIdx.x == 0) { par[0] = pp[0]; par[1] = pp[1]; par[2] = pp[2]; par[3] = pp[3]; par[4] = bad ? 0.0f : __uint_as_float(s_l); *flag = bad; }
    }
    __syncthreads();
    return s_scale;
}

// 256 threads: the f16 copy of `rows` rows at src, scaled by sc, written at dst
__device__ __forceinline__ void fm_cvt_block(const float4* __restrict__ src, int rows, float sc, ushort4* __restrict__ dst)
{
    for (int g = threadIdx.x; g < rows * 32; g += 256) {              // four elements per step
        const float4 v = src[g];
        ushort4 o; o.x = to_f16(v.x * sc); o.y = to_f16(v.y * sc); o.z = to_f16(v.z * sc); o.w = to_f16(v.w * sc);
        dst[g] = o;
    }
}

// the segment of (outer row among the launch's rows, chunk among the launch's chunks, half wave): recomputed where a
// candidate is stored (rare) instead of held in two registers
__device__ __forceinline__ int fm_seg(int row, int nchunks, int ch, int half) { return (row * nchunks + ch) * 2 + half; }

// One walk of the staged tile loop over staged blocks [0, nt) of the chunk [r0, r1) of the inner set (rh / rn2: its f16
// rows and norms; row reads clamped to ITS last row): the loop of k_match_mfma, as a function so that the workgroup can
// run it twice.  SEEDPH: every value updates the lane's running maxima, no candidates.  Otherwise: the test of k_match_mfma
// against the threshold the column had before the tile; behind the nseed seeded blocks the maxima then take the tile's
// largest value of BOTH half waves (one shuffle per column), which keeps them equal in the two halves.
template <bool SEEDPH>
__device__ __forceinline__ void fm_walk(unsigned char (*s_r)[MF_SUB * MF_TILE * MF_ROW], float (*s_n)[MF_SUB * MF_TILE],
                                        const unsigned short* __restrict__ rh, const float* __restrict__ rn2, int r_len, int r0, int r1,
                                        int nt, int nseed, float inv, bool has_rows, const f16x8 (&bfrag)[2][8], const float (&twoE)[2],
                                        float (&m1)[2], float (&m2)[2], const int (&lidx)[2], int l_len, int (&cnt)[2],
                                        int* __restrict__ cand, int prow, int nchunks, int ch)
{
    const int t = threadIdx.x, half = (t & 63) >> 5, col = t & 31;
    // ---- staging, as k_match_mfma: issue() = global loads of block k + 2 into registers, commit() = registers into the LDS
    // buffer of block k + 1; one barrier per two tiles.  Row reads are clamped to the inner set's own last row. ----
    static_assert(MF_SUB == 2, "four staging loads per thread");
    uint4 pre0 = make_uint4(0u, 0u, 0u, 0u), pre1 = make_uint4(0u, 0u, 0u, 0u), pre2 = make_uint4(0u, 0u, 0u, 0u), pre3 = make_uint4(0u, 0u, 0u, 0u);
    float pre_n = INFINITY;
    const int st_row0 = t >> 4, st_c16 = t & 15;             // rows st_row0 + 16 i, i = 0..3
#define MF_LOAD_(i_) (*reinterpret_cast<const uint4*>(rh + (size_t)min(base_ + st_row0 + 16 * (i_), r_len - 1) * 128 + st_c16 * 8))
#define MF_ISSUE(tile_) do { \
        const int base_ = r0 + (tile_) * (MF_SUB * MF_TILE); \
        pre0 = MF_LOAD_(0); pre1 = MF_LOAD_(1); pre2 = MF_LOAD_(2); pre3 = MF_LOAD_(3); \
        if (t < MF_SUB * MF_TILE) pre_n = (base_ + t < r1) ? rn2[min(base_ + t, r_len - 1)] : INFINITY;     /* rows beyond the chunk never win */ \
    } while (0)
#define MF_COMMIT(buf_) do { \
        *reinterpret_cast<uint4*>(&s_r[buf_][(st_row0 +  0) * MF_ROW + st_c16 * 16]) = pre0; \
        *reinterpret_cast<uint4*>(&s_r[buf_][(st_row0 + 16) * MF_ROW + st_c16 * 16]) = pre1; \
        *reinterpret_cast<uint4*>(&s_r[buf_][(st_row0 + 32) * MF_ROW + st_c16 * 16]) = pre2; \
        *reinterpret_cast<uint4*>(&s_r[buf_][(st_row0 + 48) * MF_ROW + st_c16 * 16]) = pre3; \
        if (t < MF_SUB * MF_TILE) s_n[buf_][t] = pre_n * inv;      /* +inf (rows beyond the chunk) becomes -inf: never a maximum */ \
    } while (0)

    if (nt > 0) { MF_ISSUE(0); MF_COMMIT(0); }
    if (nt > 1) MF_ISSUE(1);
    __syncthreads();
    for (int tile = 0; tile < nt; tile++) {
        const int buf = tile & 1;
        if (tile + 1 < nt) MF_COMMIT(buf ^ 1);           // loaded during the previous iteration
        if (tile + 2 < nt) MF_ISSUE(tile + 2);
        if (has_rows) {
#pragma unroll
        for (int sub = 0; sub < MF_SUB; sub++) {
        // accumulators start at |r|^2 / fneg2 of their row (C/D layout: row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5))
        f32x16 acc[2];
#pragma unroll
        for (int g = 0; g < 4; g++) {
            const f32x4 nr = *reinterpret_cast<const f32x4*>(&s_n[buf][sub * MF_TILE + 8 * g + 4 * half]);
#pragma unroll
            for (int e = 0; e < 4; e++) { acc[0][4 * g + e] = nr[e]; acc[1][4 * g + e] = nr[e]; }
        }
        const unsigned char* rp = &s_r[buf][(sub * MF_TILE + col) * MF_ROW + half * 16];
#pragma unroll
        for (int kk = 0; kk < 8; kk++) {
            const f16x8 a = *reinterpret_cast<const f16x8*>(rp + kk * 32);
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, bfrag[0][kk], acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, bfrag[1][kk], acc[1], 0, 0, 0);
        }
        const int base = r0 + (tile * MF_SUB + sub) * MF_TILE;
#pragma unroll
        for (int c = 0; c < 2; c++) {
            if (SEEDPH) {
                // the two largest of everything this half wave sees: no threshold, every value updates them
#pragma unroll
                for (int reg = 0; reg < 16; reg++) {
                    m2[c] = __builtin_amdgcn_fmed3f(m1[c], m2[c], acc[c][reg]);
                    m1[c] = fmaxf(m1[c], acc[c][reg]);
                }
                continue;
            }
            // The whole tile column against the threshold the column had BEFORE this tile (a superset test): one maximum of the
            // lane's 16 values and one compare (k_match_mfma).  Behind the seeded blocks the maxima then take the tile's largest
            // value of BOTH half waves (disjoint rows of the same column: one shuffle) -- a value below the threshold cannot
            // change either of the two; the seeded blocks' rows are in the maxima already and must not enter twice.
            float gm[4];
#pragma unroll
            for (int g = 0; g < 4; g++) gm[g] = fmaxf(fmaxf(fmaxf(acc[c][4 * g], acc[c][4 * g + 1]), acc[c][4 * g + 2]), acc[c][4 * g + 3]);
            const float mx = fmaxf(fmaxf(fmaxf(gm[0], gm[1]), gm[2]), gm[3]);
            const float thr = m2[c] - twoE[c];
            const bool any = mx >= thr;
            if (tile >= nseed) {
                const float mo = __shfl_xor(mx, 32);
                m2[c] = __builtin_amdgcn_fmed3f(m1[c], m2[c], mx);
                m1[c] = fmaxf(m1[c], mx);
                m2[c] = __builtin_amdgcn_fmed3f(m1[c], m2[c], mo);
                m1[c] = fmaxf(m1[c], mo);
            }
            if (__ballot(any) != 0ull) {
                if (any && lidx[c] < l_len) {
                    unsigned hits = 0u;
#pragma unroll
                    for (int g = 0; g < 4; g++) {
                        if (__ballot(gm[g] >= thr) != 0ull) {
#pragma unroll
                            for (int e = 0; e < 4; e++) hits |= (acc[c][4 * g + e] >= thr ? 1u : 0u) << (15 - (4 * g + e));
                        }
                    }
                    while (hits != 0u) {
                        const int b = 31 - __builtin_clz(hits);
                        hits &= ~(1u << b);
                        const int reg = 15 - b;
                        const int ridx = base + 8 * (reg >> 2) + 4 * half + (reg & 3);
                        if (ridx < r1) {
                            if (cnt[c] < MF_SEGCAP) cand[fm_seg(prow + lidx[c], nchunks, ch, half) * MF_SEGCAP + cnt[c]] = ridx;
                            cnt[c]++;
                        }
                    }
                }
            }
        }
        }   // sub
        }   // has_rows
        __syncthreads();
    }
}

#undef MF_ISSUE
#undef MF_COMMIT
#undef MF_LOAD_

// 256 threads, one workgroup = (outer block, inner chunk).  The tile loop of k_match_mfma<false> (match.hip: operand layout,
// the staged 2 x 32-row blocks, the norm term as the accumulator's initial value, one maximum per tile column): wave w owns
// outer rows [row0 + 64 w, + 64) of the outer set (lh / ln2: its rows in the f16 copy and its norms, l_len rows) as two B
// fragment sets and walks rows [r0, r1) of the inner set (rh / rn2, r_len rows; r1 <= r_len).  rmax2: the largest squared
// norm of the rows this direction ranks.
// Segment of (outer row, chunk, half wave): cand[fm_seg(prow + row, nchunks, ch, half) * MF_SEGCAP + ...], its count in
// cand_ct at the same index without the last factor; indices within the inner set.
__device__ __forceinline__ void fm_prefilter_block(unsigned char (*s_r)[MF_SUB * MF_TILE * MF_ROW], float (*s_n)[MF_SUB * MF_TILE],
                                                   const unsigned short* __restrict__ lh, const float* __restrict__ ln2, int l_len, int row0,
                                                   const unsigned short* __restrict__ rh, const float* __restrict__ rn2, int r_len, int r0, int r1,
                                                   float fneg2, float rmax2, float bigM, int* __restrict__ cand_ct, int* __restrict__ cand,
                                                   int prow, int nchunks, int ch)
{
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int col = lane & 31, half = lane >> 5;
    const int ntiles = (r1 - r0 + MF_SUB * MF_TILE - 1) / (MF_SUB * MF_TILE);      // staged blocks of MF_SUB tiles
    const float rmax = sqrtf(rmax2);
    const float inv = 1.0f / fneg2;                           // the epilogue works on D = s' / fneg2 (k_match_mfma)
    const bool has_rows = row0 + wave * 64 < l_len;           // a wave without outer rows only stages (wave uniform)

    // ---- this wave's outer rows: B operands (8 K-steps x 2 column sets), margins; the running maxima start empty ----
    f16x8 bfrag[2][8];
    float twoE[2], m1[2], m2[2];
    int lidx[2];
#pragma unroll
    for (int c = 0; c < 2; c++) {
        const int li = row0 + wave * 64 + c * 32 + col;
        lidx[c] = li;
        const int lq = min(li, l_len - 1);
        const unsigned short* lp = lh + (size_t)lq * 128 + half * 8;
#pragma unroll
        for (int kk = 0; kk < 8; kk++) bfrag[c][kk] = *reinterpret_cast<const f16x8*>(lp + kk * 16);
        const float nl = ln2[lq];
        const float E = match_margin(nl, rmax, rmax2, bigM);
        twoE[c] = 2.0f * E * -inv;                      // the margin in D units (-inv > 0, a power of two: exact)
        m1[c] = m2[c] = -INFINITY;
    }
    int cnt[2] = {0, 0};                         // candidates of this lane's segment = (outer row, chunk, half wave)
    // (the plan keeps 32 x the segments of a group below 2^31: fm_seg)

    // phase 0 seeds the running maxima from the chunk's first FM_SEEDBLK staged blocks (no candidates; every value updates
    // them), and the two half waves -- different rows of the same columns -- continue with the two largest of the union;
    // phase 1 walks the whole chunk, those blocks again, and tests
    const int nseed = min(FM_SEEDBLK, ntiles);
    fm_walk<true>(s_r, s_n, rh, rn2, r_len, r0, r1, nseed, nseed, inv, has_rows, bfrag, twoE, m1, m2, lidx, l_len, cnt, cand, prow, nchunks, ch);
#pragma unroll
    for (int c = 0; c < 2; c++) {
        const float o1 = __shfl_xor(m1[c], 32), o2 = __shfl_xor(m2[c], 32);
        const float d1 = fmaxf(m1[c], o1), d2 = fmaxf(fminf(m1[c], o1), fmaxf(m2[c], o2));
        m1[c] = d1; m2[c] = d2;
    }
    fm_walk<false>(s_r, s_n, rh, rn2, r_len, r0, r1, ntiles, nseed, inv, has_rows, bfrag, twoE, m1, m2, lidx, l_len, cnt, cand, prow, nchunks, ch);
#pragma unroll
    for (int c = 0; c < 2; c++)
        if (lidx[c] < l_len) cand_ct[fm_seg(prow + lidx[c], nchunks, ch, half)] = cnt[c];
}

// One wave, one outer row (l4: lane tl's four floats of it) against one inner set (idesc): k_match_exact's evaluation --
// half a wave per candidate, lane t of a half takes floats 4t..4t+3, the shuffle_down tree 16, 8, 4, 2, 1: the tree of
// l2_tree -- over the candidates of the nseg segments from seg0 on (two per chunk, contiguous for one outer row), compacted
// into one list per wave in LDS (cl: FX_SEGS * MF_SEGCAP ints of this wave's own).  The two halves take disjoint candidates
// and merge at the end; the (distance, index) order is total, so the order of evaluation does not matter.  t: in every
// lane the row's two nearest, the sentinel index 0x7fffffff where there is none; returns whether a segment overflowed.
__device__ __forceinline__ bool fm_exact_row(const float4& l4, const float* __restrict__ idesc, const int* __restrict__ cand_ct,
                                             const int* __restrict__ cand, size_t seg0, int nseg, int* cl, Top2& t)
{
    const int lane = threadIdx.x & 63, tl = lane & 31, half = lane >> 5;
    // the sentinel index is larger than any real one: an empty slot loses every tie
    t = Top2{INFINITY, INFINITY, 0x7fffffff, 0x7fffffff};
    bool over = false;
    // The set's segments FX_SEGS at a time: lane s < FX_SEGS owns segment s of the round, the segments are compacted into
    // one list in LDS (k_match_exact), and the list is walked two candidates per half wave and step.  One round for a set of
    // up to 16 chunks.
    for (int s0 = 0; s0 < nseg; s0 += FX_SEGS) {
        const bool mine = lane < FX_SEGS && s0 + lane < nseg;
        const int rawct = mine ? cand_ct[seg0 + s0 + lane] : 0;
        over |= rawct > MF_SEGCAP;
        const int myct = min(rawct, MF_SEGCAP);
        int off = myct;                                          // inclusive prefix sum over the 64 lanes
#pragma unroll
        for (int k = 1; k < 64; k <<= 1) { const int o = __shfl_up(off, k); if (lane >= k) off += o; }
        const int n = __shfl(off, 63);
        off -= myct;
        for (int k = 0; k < myct; k++) cl[off + k] = cand[(seg0 + s0 + lane) * MF_SEGCAP + k];
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");   // the wave reads what its own lanes wrote
        __builtin_amdgcn_wave_barrier();
        // 2 x EX_K candidates per step (EX_K per half wave): all 512-byte reads of a half are in flight before the first reduction
        constexpr int EX_K = 2;
        for (int c0 = 0; c0 < n; c0 += 2 * EX_K) {
            int ri[EX_K];
            float4 r4[EX_K];
#pragma unroll
            for (int k = 0; k < EX_K; ++k) {
                const int c = c0 + 2 * k + half;
                ri[k] = c < n ? cl[c] : -1;
                r4[k] = reinterpret_cast<const float4*>(idesc + (size_t)(ri[k] < 0 ? 0 : ri[k]) * 128)[tl];
            }
#pragma unroll
            for (int k = 0; k < EX_K; ++k) {
                const float qx = l4.x - r4[k].x, qy = l4.y - r4[k].y, qz = l4.z - r4[k].z, qw = l4.w - r4[k].w;
                float v = fmaf(qw, qw, fmaf(qz, qz, fmaf(qx, qx, qy * qy)));
                v += __shfl_down(v, 16, 32); v += __shfl_down(v, 8, 32); v += __shfl_down(v, 4, 32);
                v += __shfl_down(v, 2, 32);  v += __shfl_down(v, 1, 32);
                const float d = __shfl(v, 0, 32);                // the half's distance, in all of its lanes
                if (ri[k] >= 0) top2_insert_lex(t, d, ri[k]);
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");   // the next round overwrites the list
        __builtin_amdgcn_wave_barrier();
    }
    {   // the two halves hold disjoint candidate subsets: merge
        const float od1 = __shfl_xor(t.d1, 32), od2 = __shfl_xor(t.d2, 32);
        const int oi1 = __shfl_xor(t.i1, 32), oi2 = __shfl_xor(t.i2, 32);
        top2_insert_lex(t, od1, oi1);
        top2_insert_lex(t, od2, oi2);
    }
    return over;
}

} // namespace
