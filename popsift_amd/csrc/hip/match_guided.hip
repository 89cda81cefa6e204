// match_guided.hip -- guided matching: the 2-NN search restricted by a homography or an epipolar band
// (psx_match_guided*, psx_match_pairs_guided*, psx_guide_allows, psx_desc_positions; include/popsift_hip.h).
//
// A guide (guide_rule.h) says, from the POSITIONS of a left and a right descriptor alone, whether the pair is admissible;
// every left descriptor ranks only its admissible right descriptors.  Typically a handful of the right side survive, so
// the MFMA prefilters of match.hip have nothing to work on: almost every pair is excluded before any distance is formed.
// The work is (1) the rule on every (outer, inner) pair of positions -- a few float operations on 8 or 16 bytes -- and (2) an exact
// distance for the few survivors.
//
// k_match_guided: one wave per OUTER descriptor (the side whose 2-NN are searched: left in the forward pass, right in the
// backward pass of a cross-check).  The wave holds the outer row in the half-wave layout of k_match_exact (match.hip):
// lane t of each half holds floats 4t..4t+3 (bytes: 4t..4t+3 of the 128).  It walks the inner side's positions 64 at a
// time -- one coalesced 8-byte load per lane, the next step's load in flight while this step is evaluated -- each lane
// evaluates the rule for its inner point, and a wave64 ballot gives the step's admissible set as a wave-uniform mask.
// The wave then takes the set bits in ascending index, four per round (two per half wave, so that the row reads of a
// round are in flight together): the half computes the pair's exact distance -- floats: the reference's own operation
// tree (l2_in_t0, features.cu:160-189: lane t takes floats 4t..4t+3, then shuffle_down 16, 8, 4, 2, 1), bit for bit what
// k_match_exact computes; bytes: exact integers -- and keeps a running top-2 under (distance, index) order.  The trip
// counts are wave uniform, there are no atomics and nothing depends on arrival order.  SWAP exchanges which side supplies
// the "left" role of the rule: the backward pass evaluates the SAME relation with the loops exchanged, never a
// transposed matrix.  The rule comes in two steps (guide_rule.h): what depends on the left point alone -- (a, b, c) and the
// right-hand side of the comparison, psx_guide_left(kind, m, tol, xl, yl) -- and the comparison for one right point,
// psx_guide_right(kind, line, xr, yr).  Forward, the left point is the wave's own:
// the first step runs once per wave, on wave-uniform values.  Backward, the left points are the INNER side: k_guide_lines
// takes the first step once per left descriptor and the wave walks those 16-byte records instead of the positions, so
// both directions spend the same 6 to 8 float operations per pair (with the first step taken per pair, 12 operations more,
// 18 432 x 18 432 both ways took 0.506 ms instead of 0.468 under a window and 0.892 instead of 0.806 under an epipolar
// band: profiles/match_guided_ms.txt).  The kernel writes a directed result in the layout of k_match_merge /
// k_match_u8_merge, so the join of psx_match_pairs (k_pairs_count / k_pairs_write) runs on it unchanged.  The wave's
// search itself is g_match_row of match_guided_core.h, which the batched driver (match_guided_graph.hip) drives from an
// edge table.
#include "psx_internal.h"
#include "guide_rule.h"
#include "match_guided_core.h"
#include "match_join.h"
#include "match_scratch.h"

#include <climits>
#include <cstring>

namespace {

// the first step of the rule for every left point: lines[i] = (a, b, c, w) of left_xy[i]
__global__ void k_guide_lines(const float2* __restrict__ left_xy, int n, const psx_guide g, float4* __restrict__ lines)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float2 p = left_xy[i];
    const psx_guide_line l = psx_guide_left(g.kind, g.m, g.tol, p.x, p.y);
    lines[i] = make_float4(l.a, l.b, l.c, l.w);
}

// grid ceil(o_len / 4), 256 threads: wave w of workgroup b owns outer descriptor 4 b + w.  inner_geo: forward (SWAP =
// false) the inner side's positions (float2), backward the inner side's lines (float4, k_guide_lines).  out: 3 o_len ints
// (best, second, accept), then 2 o_len distances (D), as the directed matchers of match.hip leave them.
template <class T, class D, bool SWAP>
__global__ __launch_bounds__(256) void k_match_guided(const T* __restrict__ outer, const float2* __restrict__ outer_xy, int o_len,
                                                      const T* __restrict__ inner, const void* __restrict__ inner_geo, int i_len,
                                                      const psx_guide g, int* __restrict__ out)
{
    g_match_row<T, D, SWAP>(outer, outer_xy, o_len, blockIdx.x * 4 + (threadIdx.x >> 6), inner, inner_geo, i_len, g, out);
}

__global__ void k_desc_positions(const psx_feature_dev* __restrict__ features, const int* __restrict__ reverse_map, int n,
                                 float2* __restrict__ xy)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const psx_feature_dev* f = features + reverse_map[k];
    xy[k] = make_float2(f->xpos, f->ypos);
}

// one directed pass behind whatever is queued on st: forward (outer = left) or backward (outer = right, the rule's roles
// exchanged; d_lines: room for i_len float4, filled here with the inner = left side's lines); d_out: 5 o_len ints
template <class T, class D>
void queue_directed(hipStream_t st, bool backward, const T* outer, const float* outer_xy, int o_len,
                    const T* inner, const float* inner_xy, int i_len, const psx_guide& g, float4* d_lines, int* d_out)
{
    const dim3 grid((unsigned)((o_len + 3) / 4)), block(256);
    const float2* oxy = reinterpret_cast<const float2*>(outer_xy);
    const float2* ixy = reinterpret_cast<const float2*>(inner_xy);
    if (backward) {
        hipLaunchKernelGGL(k_guide_lines, dim3((unsigned)((i_len + 255) / 256)), block, 0, st, ixy, i_len, g, d_lines);
        hipLaunchKernelGGL((k_match_guided<T, D, true>), grid, block, 0, st, outer, oxy, o_len, inner, static_cast<const void*>(d_lines), i_len, g, d_out);
    }
    else hipLaunchKernelGGL((k_match_guided<T, D, false>), grid, block, 0, st, outer, oxy, o_len, inner, static_cast<const void*>(ixy), i_len, g, d_out);
}

template <class T>
bool sides_ok(const T* d_left, const float* d_left_xy, int l_len, const T* d_right, const float* d_right_xy, int r_len)
{
    return l_len >= 0 && r_len >= 0 && (l_len == 0 || (d_left && d_left_xy)) && (r_len == 0 || (d_right && d_right_xy));
}

template <class T, class D>
int match_guided(int device, const T* d_left, const float* d_left_xy, int l_len, const T* d_right, const float* d_right_xy, int r_len,
                 const psx_guide* guide, int* host_match, D* host_dist)
{
    if (!sides_ok(d_left, d_left_xy, l_len, d_right, d_right_xy, r_len) || (l_len > 0 && !host_match) || !psx_guide_valid(guide))
        return PSX_ERR_INVALID;
    if (l_len == 0) return PSX_OK;
    if (hipSetDevice(device) != hipSuccess) return PSX_ERR_HIP;
    MatchScratch& sc = psx_match_scratch();
    if (!sc.bind(device)) return PSX_ERR_HIP;
    const size_t ob = sizeof(int) * 5 * (size_t)l_len;
    if (!sc.need(MS_GUIDED_FWD, ob) || !sc.need_pinned(ob)) return PSX_ERR_NOMEM;
    int* d_out = static_cast<int*>(sc.buf[MS_GUIDED_FWD]);
    hipStream_t st = sc.stream;
    queue_directed<T, D>(st, false, d_left, d_left_xy, l_len, d_right, d_right_xy, r_len, *guide, nullptr, d_out);
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(sc.hpin, d_out, ob, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return PSX_ERR_HIP;
    const int* hp = static_cast<const int*>(sc.hpin);
    memcpy(host_match, hp, sizeof(int) * 3 * (size_t)l_len);
    if (host_dist) memcpy(host_dist, hp + 3 * (size_t)l_len, sizeof(D) * 2 * (size_t)l_len);
    return PSX_OK;
}

// host_pairs or d_pairs (the other is NULL; both NULL with capacity 0)
template <class T, class D>
int match_pairs_guided(int device, const T* d_left, const float* d_left_xy, int l_len, const T* d_right, const float* d_right_xy, int r_len,
                       const psx_guide* guide, const psx_match_opts* opts, void* host_pairs, void* d_pairs, int capacity, int* count)
{
    if (!psx_pairs_args_ok(l_len, r_len, opts, host_pairs ? host_pairs : d_pairs, capacity, count) ||
        !sides_ok(d_left, d_left_xy, l_len, d_right, d_right_xy, r_len) || !psx_guide_valid(guide))
        return PSX_ERR_INVALID;
    if (l_len == 0 || r_len == 0) { *count = 0; return PSX_OK; }
    if (hipSetDevice(device) != hipSuccess) return PSX_ERR_HIP;
    MatchScratch& sc = psx_match_scratch();
    if (!sc.bind(device)) return PSX_ERR_HIP;
    const bool mutual = (opts->flags & PSX_PAIRS_MUTUAL) != 0;
    // both directions' buffers before the first launch: nothing is reallocated under queued work
    if (!sc.need(MS_GUIDED_FWD, sizeof(int) * 5 * (size_t)l_len) ||
        (mutual && (!sc.need(MS_GUIDED_BWD, sizeof(int) * 5 * (size_t)r_len) || !sc.need(MS_GUIDED_LINES, sizeof(float4) * (size_t)l_len))))
        return PSX_ERR_NOMEM;
    int* d_fwd = static_cast<int*>(sc.buf[MS_GUIDED_FWD]);
    int* d_bwd = mutual ? static_cast<int*>(sc.buf[MS_GUIDED_BWD]) : nullptr;
    queue_directed<T, D>(sc.stream, false, d_left, d_left_xy, l_len, d_right, d_right_xy, r_len, *guide, nullptr, d_fwd);
    if (mutual) queue_directed<T, D>(sc.stream, true, d_right, d_right_xy, r_len, d_left, d_left_xy, l_len, *guide, static_cast<float4*>(sc.buf[MS_GUIDED_LINES]), d_bwd);
    return psx_pairs_finish<D>(sc, d_fwd, l_len, d_bwd, opts, host_pairs, d_pairs, capacity, count);
}

} // namespace

extern "C" int psx_guide_allows(const psx_guide* guide, const float* left_xy, int nl, const float* right_xy, int nr,
                                unsigned char* allowed)
{
    if (!psx_guide_valid(guide) || nl < 0 || nr < 0 || (nl > 0 && !left_xy) || (nr > 0 && !right_xy) ||
        (nl > 0 && nr > 0 && !allowed))
        return PSX_ERR_INVALID;
    for (int i = 0; i < nl; i++)
        for (int j = 0; j < nr; j++)
            allowed[(size_t)i * nr + j] = psx_guide_pair(guide->kind, guide->m, guide->tol, left_xy[2 * (size_t)i], left_xy[2 * (size_t)i + 1],
                                                         right_xy[2 * (size_t)j], right_xy[2 * (size_t)j + 1]) ? 1 : 0;
    return PSX_OK;
}

extern "C" int psx_desc_positions(int device, const psx_feature_dev* d_features, const int* d_reverse_map, int n_desc, float* d_xy)
{
    if (n_desc < 0 || (n_desc > 0 && (!d_features || !d_reverse_map || !d_xy))) return PSX_ERR_INVALID;
    if (n_desc == 0) return PSX_OK;
    if (hipSetDevice(device) != hipSuccess) return PSX_ERR_HIP;
    MatchScratch& sc = psx_match_scratch();
    if (!sc.bind(device)) return PSX_ERR_HIP;
    hipLaunchKernelGGL(k_desc_positions, dim3((unsigned)((n_desc + 255) / 256)), dim3(256), 0, sc.stream, d_features, d_reverse_map, n_desc,
                       reinterpret_cast<float2*>(d_xy));
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(sc.stream) != hipSuccess) return PSX_ERR_HIP;
    return PSX_OK;
}

extern "C" int psx_match_guided(int device, const float* d_left, const float* d_left_xy, int l_len,
                                const float* d_right, const float* d_right_xy, int r_len, const psx_guide* guide,
                                int* host_match, float* host_dist)
{
    return match_guided<float, float>(device, d_left, d_left_xy, l_len, d_right, d_right_xy, r_len, guide, host_match, host_dist);
}

extern "C" int psx_match_guided_u8(int device, const unsigned char* d_left, const float* d_left_xy, int l_len,
                                   const unsigned char* d_right, const float* d_right_xy, int r_len, const psx_guide* guide,
                                   int* host_match, int* host_dist)
{
    return match_guided<unsigned char, int>(device, d_left, d_left_xy, l_len, d_right, d_right_xy, r_len, guide, host_match, host_dist);
}

extern "C" int psx_match_pairs_guided(int device, const float* d_left, const float* d_left_xy, int l_len,
                                      const float* d_right, const float* d_right_xy, int r_len, const psx_guide* guide,
                                      const psx_match_opts* opts, psx_match_pair* host_pairs, int capacity, int* count)
{
    return match_pairs_guided<float, float>(device, d_left, d_left_xy, l_len, d_right, d_right_xy, r_len, guide, opts, host_pairs, nullptr, capacity, count);
}

extern "C" int psx_match_pairs_guided_u8(int device, const unsigned char* d_left, const float* d_left_xy, int l_len,
                                         const unsigned char* d_right, const float* d_right_xy, int r_len, const psx_guide* guide,
                                         const psx_match_opts* opts, psx_match_pair_u8* host_pairs, int capacity, int* count)
{
    return match_pairs_guided<unsigned char, int>(device, d_left, d_left_xy, l_len, d_right, d_right_xy, r_len, guide, opts, host_pairs, nullptr, capacity, count);
}

extern "C" int psx_match_pairs_guided_dev(int device, const float* d_left, const float* d_left_xy, int l_len,
                                          const float* d_right, const float* d_right_xy, int r_len, const psx_guide* guide,
                                          const psx_match_opts* opts, psx_match_pair* d_pairs, int capacity, int* count)
{
    return match_pairs_guided<float, float>(device, d_left, d_left_xy, l_len, d_right, d_right_xy, r_len, guide, opts, nullptr, d_pairs, capacity, count);
}

extern "C" int psx_match_pairs_guided_u8_dev(int device, const unsigned char* d_left, const float* d_left_xy, int l_len,
                                             const unsigned char* d_right, const float* d_right_xy, int r_len, const psx_guide* guide,
                                             const psx_match_opts* opts, psx_match_pair_u8* d_pairs, int capacity, int* count)
{
    return match_pairs_guided<unsigned char, int>(device, d_left, d_left_xy, l_len, d_right, d_right_xy, r_len, guide, opts, nullptr, d_pairs, capacity, count);
}
