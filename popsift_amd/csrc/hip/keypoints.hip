// keypoints.hip -- caller-supplied keypoints (psx_set_keypoints / psx_describe, include/popsift_hip.h).
//
// The orientation, scan and descriptor kernels read keypoints only through P->iext[o], P->iext_off[o] and
// cnt->ext_ct[o].  The kernels here fill exactly those from a caller's psx_keypoint records instead of the DoG
// detector: every record is placed and validated by psx_kp_place (kp_place.h, shared with the host), and the accepted
// ones are compacted per octave in CALLER ORDER -- a stable compaction with no atomic-arrival order, so the output
// order is a function of the input alone:
//   k_kp_classify  a chunk = 256 consecutive records; a record's rank among the records of its octave inside its wave
//                  comes from a wave64 ballot + mbcnt, the waves' counts are summed in LDS; the chunk's per-octave
//                  counts go into a small table tbl[octave][chunk];
//   k_kp_offsets   one workgroup scans the table along the chunks (exclusive, in place), writes cnt->ext_ct[o] /
//                  iext_ct[o] for EVERY octave (zeros included) and the octave-major bases of the clamped counts;
//   k_kp_scatter   repeats the chunk's ranking (same code, same result) and writes iext[o][rank] (cell = 0,
//                  ignore = 0), iext_off[o][rank] = rank, the source index of the extremum and its given orientations.
//                  Per octave the first max_extrema accepted records are kept (ext_count(), orient_desc.hip);
//   k_kp_adopt     behind k_orientation: extrema whose record carried orientations get them verbatim
//                  (P->extrema[e].orientation / num_ori, P->ext_nori[e]); k_orientation's own result for them is
//                  overwritten, its code object is untouched.
// Records arrive through coalesced 8-byte loads into LDS (a chunk is 10 KB of consecutive memory); everything is written
// with plain vector stores.
#include "psx_internal.h"
#include "kp_place.h"

#include <cmath>
#include <cstring>

namespace {

constexpr int KP_NT = 256;                          // threads per workgroup = records per chunk
constexpr int KP_NW = KP_NT / PSX_WAVE;
constexpr int KP_WORDS = sizeof(psx_keypoint) / 8;  // 8-byte words per record
constexpr int KP_HEAD = 32;                         // ints in front of the table: octave bases [0..MAX_OCTAVES-1], total
constexpr int OFF_NT = 1024;
static_assert(sizeof(psx_keypoint) == 40, "psx_keypoint layout");
static_assert(PSX_MAX_OCTAVES < KP_HEAD, "table head");

struct KpLane {
    bool        ok;
    PsxKpPlaced pl;
    int         num_ori;
    float       ori[PSX_ORI_MAX];
    int         rank;                               // among the accepted records of its octave in this chunk
};

__device__ __forceinline__ int lanes_below(unsigned long long m)
{
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

// Loads, places and ranks the records of one chunk.  On return s_cnt[w][o] = accepted records of octave o in wave w
// (all workgroup threads have passed a barrier behind the last write).  The caller puts a barrier in front of the next call.
__device__ __forceinline__ void kp_chunk(const psx_keypoint* __restrict__ kps, int n, int chunk, const PsxKpGeom& g,
                                         uint2* s_rec, int (*s_cnt)[PSX_MAX_OCTAVES], KpLane& me)
{
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int first = chunk * KP_NT;
    const int cnt = min(KP_NT, n - first);
    const uint2* src = reinterpret_cast<const uint2*>(kps + first);
    for (int i = t; i < cnt * KP_WORDS; i += KP_NT) s_rec[i] = src[i];
    for (int i = t; i < KP_NW * PSX_MAX_OCTAVES; i += KP_NT) (&s_cnt[0][0])[i] = 0;
    __syncthreads();

    me.ok = false; me.rank = 0; me.num_ori = 0;
    int oct = -1;
    if (t < cnt) {
        psx_keypoint k;
        uint2 wv[KP_WORDS];
#pragma unroll
        for (int q = 0; q < KP_WORDS; q++) wv[q] = s_rec[t * KP_WORDS + q];
        k.xpos = __uint_as_float(wv[0].x); k.ypos = __uint_as_float(wv[0].y);
        k.sigma = __uint_as_float(wv[1].x); k.octave = (int)wv[1].y;
        k.lpos = (int)wv[2].x; k.num_ori = (int)wv[2].y;
        k.orientation[0] = __uint_as_float(wv[3].x); k.orientation[1] = __uint_as_float(wv[3].y);
        k.orientation[2] = __uint_as_float(wv[4].x); k.orientation[3] = __uint_as_float(wv[4].y);
        me.ok = psx_kp_place(g, k, &me.pl);
        if (me.ok) {
            oct = me.pl.octave;
            me.num_ori = k.num_ori;
#pragma unroll
            for (int q = 0; q < PSX_ORI_MAX; q++) me.ori[q] = q < k.num_ori ? k.orientation[q] : 0.0f;
        }
    }
    // stable rank inside the wave, one octave per round (wave uniform: at most num_octaves rounds)
    for (unsigned long long todo = __ballot(oct >= 0); todo != 0ull;) {
        const int lead = __builtin_amdgcn_readfirstlane(__ffsll((long long)todo) - 1);
        const int o = __builtin_amdgcn_readlane(oct, lead);
        const unsigned long long m = __ballot(oct == o);
        if (oct == o) me.rank = lanes_below(m);
        if (lane == 0) s_cnt[wave][o] = __popcll(m);
        todo &= ~m;
    }
    __syncthreads();
    if (me.ok)
        for (int w = 0; w < wave; w++) me.rank += s_cnt[w][oct];
}

__global__ __launch_bounds__(KP_NT) void k_kp_classify(const psx_keypoint* __restrict__ kps, int n, int nchunks, int stride,
                                                       const PsxKpGeom g, int* __restrict__ tbl)
{
    __shared__ uint2 s_rec[KP_NT * KP_WORDS];
    __shared__ int s_cnt[KP_NW][PSX_MAX_OCTAVES];
    for (int chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        KpLane me;
        kp_chunk(kps, n, chunk, g, s_rec, s_cnt, me);
        const int t = threadIdx.x;
        if (t < g.num_octaves) {
            int c = 0;
#pragma unroll
            for (int w = 0; w < KP_NW; w++) c += s_cnt[w][t];
            tbl[KP_HEAD + t * stride + chunk] = c;
        }
        __syncthreads();
    }
}

// One workgroup: exclusive scan of every octave's row of the table (in place), the frame's extrema counters, the bases.
__global__ __launch_bounds__(OFF_NT) void k_kp_offsets(int nchunks, int stride, int num_octaves, int max_extrema,
                                                       int* __restrict__ tbl, PsxCounters* __restrict__ cnt)
{
    __shared__ int s_wsum[OFF_NT / PSX_WAVE];
    __shared__ int s_tot[PSX_MAX_OCTAVES];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    for (int o = 0; o < num_octaves; o++) {
        int* row = tbl + KP_HEAD + o * stride;
        int running = 0;
        for (int c0 = 0; c0 < nchunks; c0 += OFF_NT) {
            const int c = c0 + t;
            const int own = c < nchunks ? row[c] : 0;
            int v = own;
#pragma unroll
            for (int off = 1; off < PSX_WAVE; off <<= 1) {
                const int u = __shfl_up(v, off);
                if (lane >= off) v += u;
            }
            __syncthreads();                      // s_wsum free
            if (lane == PSX_WAVE - 1) s_wsum[wave] = v;
            __syncthreads();
            int before = 0, all = 0;
#pragma unroll
            for (int w = 0; w < OFF_NT / PSX_WAVE; w++) { const int x = s_wsum[w]; before += w < wave ? x : 0; all += x; }
            if (c < nchunks) row[c] = running + before + v - own;
            running += all;
        }
        if (t == 0) s_tot[o] = running;
    }
    __syncthreads();
    if (t == 0) {
        int base = 0;
        for (int o = 0; o < PSX_MAX_OCTAVES; o++) {
            const int c = o < num_octaves ? s_tot[o] : 0;
            cnt->ext_ct[o] = c;
            cnt->iext_ct[o] = c;
            tbl[o] = base;
            base += min(c, max_extrema);
        }
        tbl[PSX_MAX_OCTAVES] = base;
    }
}

__global__ __launch_bounds__(KP_NT) void k_kp_scatter(const psx_keypoint* __restrict__ kps, int n, int nchunks, int stride,
                                                      const PsxKpGeom g, const int* __restrict__ tbl, const PsxParams* __restrict__ P,
                                                      int* __restrict__ src, int* __restrict__ gnori, float4* __restrict__ gori)
{
    __shared__ uint2 s_rec[KP_NT * KP_WORDS];
    __shared__ int s_cnt[KP_NW][PSX_MAX_OCTAVES];
    for (int chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        KpLane me;
        kp_chunk(kps, n, chunk, g, s_rec, s_cnt, me);
        if (me.ok) {
            const int o = me.pl.octave;
            const int rank = tbl[KP_HEAD + o * stride + chunk] + me.rank;
            if (rank < g.max_extrema) {
                psx_iext ie;
                ie.xpos = me.pl.xpos; ie.ypos = me.pl.ypos; ie.lpos = me.pl.lpos; ie.sigma = me.pl.sigma;
                ie.cell = 0; ie.ignore = 0;
                P->iext[o][rank] = ie;
                P->iext_off[o][rank] = rank;
                const int e = tbl[o] + rank;
                src[e] = chunk * KP_NT + (int)threadIdx.x;
                gnori[e] = me.num_ori;
                gori[e] = make_float4(me.ori[0], me.ori[1], me.ori[2], me.ori[3]);
            }
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(KP_NT) void k_kp_adopt(const int* __restrict__ tbl, const PsxParams* __restrict__ P,
                                                    const int* __restrict__ gnori, const float4* __restrict__ gori)
{
    const int total = min(tbl[PSX_MAX_OCTAVES], P->ext_capacity);
    for (int e = blockIdx.x * KP_NT + threadIdx.x; e < total; e += gridDim.x * KP_NT) {
        const int nq = gnori[e];
        if (nq <= 0) continue;
        const float4 a = gori[e];
        psx_extremum* ex = P->extrema + e;
        ex->num_ori = nq;
        ex->orientation[0] = a.x; ex->orientation[1] = a.y; ex->orientation[2] = a.z; ex->orientation[3] = a.w;
        P->ext_nori[e] = nq;
    }
}

inline int kp_chunks(int n) { return (n + KP_NT - 1) / KP_NT; }
inline int kp_stride(int n) { return (kp_chunks(n) + 31) & ~31; }

} // namespace

size_t psx_kp_table_ints(int num_octaves, int n) { return (size_t)KP_HEAD + (size_t)num_octaves * kp_stride(n); }

// the part of the geometry that depends on the configuration alone
void psx_kp_geom_scale(const psx_config* cfg, PsxKpGeom* g)
{
    const int levels = cfg->levels < 2 ? 2 : cfg->levels;          // psx_create, popsift.cpp:86
    g->levels = levels;
    g->L = levels + 3;
    g->up = (int)cfg->upscale_factor;
    g->max_extrema = cfg->max_extrema;
    g->sigma_min = cfg->sigma;
    g->sigma_max = (float)((double)cfg->sigma * std::pow(2.0, (double)(g->L - 1) / levels));
    for (int l = 0; l < PSX_GAUSS_LEVELS; l++)
        g->bounds[l] = l <= levels ? (float)((double)cfg->sigma * std::pow(2.0, ((double)l + 0.5) / levels)) : INFINITY;
}

hipError_t psx_launch_kp_inject(const PsxTuning& t, const PsxParams* d_params, PsxCounters* d_cnt, const PsxKpGeom& g,
                                const PsxKpBuffers& b, hipStream_t s)
{
    const int nchunks = kp_chunks(b.n), stride = kp_stride(b.n);
    const int cus = t.cus > 0 ? t.cus : 256;
    const int grid = nchunks < 8 * cus ? nchunks : 8 * cus;
    if (nchunks > 0)
        hipLaunchKernelGGL(k_kp_classify, dim3(grid), dim3(KP_NT), 0, s, b.kps, b.n, nchunks, stride, g, b.tbl);
    hipLaunchKernelGGL(k_kp_offsets, dim3(1), dim3(OFF_NT), 0, s, nchunks, stride, g.num_octaves, g.max_extrema, b.tbl, d_cnt);
    if (nchunks > 0)
        hipLaunchKernelGGL(k_kp_scatter, dim3(grid), dim3(KP_NT), 0, s, b.kps, b.n, nchunks, stride, g, (const int*)b.tbl, d_params,
                           b.src, b.gnori, reinterpret_cast<float4*>(b.gori));
    return hipGetLastError();
}

hipError_t psx_launch_kp_adopt(const PsxTuning& t, const PsxParams* d_params, const PsxKpBuffers& b, hipStream_t s)
{
    if (b.n <= 0) return hipSuccess;
    const int cus = t.cus > 0 ? t.cus : 256;
    const int want = (b.n + KP_NT - 1) / KP_NT;
    const int grid = want < 8 * cus ? want : 8 * cus;
    hipLaunchKernelGGL(k_kp_adopt, dim3(grid), dim3(KP_NT), 0, s, (const int*)b.tbl, d_params, (const int*)b.gnori,
                       reinterpret_cast<const float4*>(b.gori));
    return hipGetLastError();
}

// ---- host entry points that need no device ----------------------------------------------------------------------------

extern "C" int psx_keypoint_bounds(const psx_config* cfg, float* bounds, int capacity, int* n)
{
    if (!cfg || !bounds) return PSX_ERR_INVALID;
    PsxKpGeom g;
    psx_kp_geom_scale(cfg, &g);
    if (g.L > PSX_GAUSS_LEVELS || capacity < g.levels + 1) return PSX_ERR_INVALID;
    for (int l = 0; l <= g.levels; l++) bounds[l] = g.bounds[l];
    if (n) *n = g.levels + 1;
    return PSX_OK;
}

extern "C" int psx_place_keypoints(const psx_config* cfg, int w, int h, const psx_keypoint* kps, int n, int* octave, int* lpos)
{
    if (!cfg || w <= 0 || h <= 0 || n < 0 || (n > 0 && (!kps || !octave || !lpos))) return PSX_ERR_INVALID;
    PsxKpGeom g;
    memset(&g, 0, sizeof(g));
    psx_kp_geom_scale(cfg, &g);
    if (g.L > PSX_GAUSS_LEVELS || cfg->max_extrema <= 0) return PSX_ERR_INVALID;
    // octave count and sizes as psx_resize derives them (popsift.cpp:109-126, sift_pyramid.cu:129-134)
    const float scale = 1.0f / powf(2.0f, -cfg->upscale_factor);
    int no = cfg->octaves;
    if (no < 0) {
        no = (int)(floorf(logf((float)(w < h ? w : h)) / logf(2.0f)) - 3.0f + scale);
        if (no < 1) no = 1;
    }
    no = no < 1 ? 1 : (no > PSX_MAX_OCTAVES ? PSX_MAX_OCTAVES : no);
    int ow = (int)ceilf(w * scale), oh = (int)ceilf(h * scale);
    if (ow <= 0 || oh <= 0) return PSX_ERR_INVALID;
    g.num_octaves = no;
    for (int o = 0; o < no; o++) {
        g.w[o] = ow; g.h[o] = oh;
        ow = (int)ceilf(ow / 2.0f);
        oh = (int)ceilf(oh / 2.0f);
    }
    for (int i = 0; i < n; i++) {
        PsxKpPlaced p;
        if (psx_kp_place(g, kps[i], &p)) { octave[i] = p.octave; lpos[i] = p.lpos; }
        else { octave[i] = -1; lpos[i] = -1; }
    }
    return PSX_OK;
}
