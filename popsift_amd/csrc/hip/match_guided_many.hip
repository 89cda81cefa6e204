// match_guided_many.hip -- the guided re-match of one byte descriptor set against many in one call:
// psx_match_pairs_guided_many_u8 (+ _dev), psx_guides_from_ransac (include/popsift_hip.h).
//
// psx_match_pairs_guided_u8 (match_guided.hip) is a fixed launch sequence, one synchronisation and one count read-back per
// call; at 2k-4k descriptors per image that is what a loop over K right sets pays K times.  Here the same wave-level search
// (g_match_row, match_guided_core.h: one wave per outer descriptor, the inner positions 64 at a time, a ballot, exact
// integer distances for the survivors) is driven over all sets by one grid per step, its operands taken from a SET TABLE:
// one entry per right set with its descriptors, its positions, its length, its first row among all right rows and its
// OWN guide.  The table is built in the pinned staging buffer and copied on the stream; an entry is read at wave-uniform
// addresses.  A set whose guide has kind PSX_GUIDE_NONE is in the table with length 0: none of its arrays is read, the
// join has nothing to look at.
//   k_guide_lines_many          (cross-check only) lines[k * l_len + i] = the first step of the rule (psx_guide_left) for
//                               left point i under guide k; one grid over K x l_len
//   k_match_guided_many<false>  forward: wave (k, i) walks set k's positions under guide k; its directed result goes to
//                               fwd + 5 l_len k
//   k_match_guided_many<true>   backward (cross-check only): the blocks are psx_many_blocks over the sets' lengths -- 256
//                               rows of ONE set, never crossing a set --, 64 workgroups of 4 waves per block; wave (k, j)
//                               walks lines + k l_len, the SAME relation with the loops exchanged, and writes at
//                               bwd + 5 * (set k's first row)
//   k_many_count / k_many_scan / k_many_write   the segmented join of match_many_join.h, unchanged: the two layouts above
//                               are what it reads
// A wave past its set's last row, or of an empty or skipped set, leaves before any load of a descriptor or a position;
// every index a wave forms is below its own set's length, so nothing of a neighbouring set is read or ranked.
// Launches per call, whatever K is: the table copy, then 4 kernels without the cross-check and 6 with it; one stream
// synchronisation.  Every scratch buffer is sized before the first launch.
#include "psx_internal.h"
#include "guide_rule.h"
#include "match_guided_core.h"
#include "match_join.h"
#include "match_many_join.h"
#include "match_many_plan.h"
#include "match_scratch.h"

#include <climits>
#include <cstring>
#include <vector>

namespace {

// one entry per right set
struct GuidedSet {
    const unsigned char* desc;   // the set's descriptors
    const float2* xy;            // the set's positions
    int len;                     // rows; 0 for a skipped set
    int roff;                    // its first row among the rows of all right sets (prefix sum of the lengths)
    psx_guide guide;             // the set's own guide
    int pad[3];
};
static_assert(sizeof(GuidedSet) == 80 && sizeof(GuidedSet) % 16 == 0, "whole 16-byte scalar loads per entry");

// grid ceil(K l_len / 256): thread (k, i) = (t / l_len, t % l_len)
__global__ __launch_bounds__(256) void k_guide_lines_many(const GuidedSet* __restrict__ sets, const float2* __restrict__ left_xy,
                                                          int l_len, long long n, float4* __restrict__ lines)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    const int k = (int)(t / l_len), i = (int)(t % l_len);
    if (sets[k].len == 0) return;                              // nobody walks the lines of an empty or skipped set
    const float2 p = left_xy[i];
    const psx_guide_line l = psx_guide_left(sets[k].guide.kind, sets[k].guide.m, sets[k].guide.tol, p.x, p.y);
    lines[t] = make_float4(l.a, l.b, l.c, l.w);
}

// 256 threads, one wave per outer descriptor.
// Forward (SWAP = false): grid K * ceil(l_len / 4), workgroup (k, b) = (blockIdx.x / per_set, blockIdx.x % per_set) owns
// left rows 4 b .. 4 b + 3 against set k; geo is unused.
// Backward (SWAP = true): grid (blocks of the right sets) * 64, workgroup (blk, q) = (blockIdx.x / 64, blockIdx.x % 64)
// owns rows row0 + 4 q .. + 3 of its block's set against L; geo = the lines of all sets.
template <bool SWAP>
__global__ __launch_bounds__(256) void k_match_guided_many(const GuidedSet* __restrict__ sets, const int2* __restrict__ blocks,
                                                           const unsigned char* __restrict__ left, const float2* __restrict__ left_xy,
                                                           int l_len, int per_set, const float4* __restrict__ geo, int* __restrict__ out)
{
    const int w = (int)(threadIdx.x >> 6);
    if (!SWAP) {
        const int k = (int)(blockIdx.x / (unsigned)per_set), b = (int)(blockIdx.x % (unsigned)per_set);
        const GuidedSet* s = sets + k;
        if (s->len == 0) return;
        g_match_row<unsigned char, int, false>(left, left_xy, l_len, 4 * b + w, s->desc, s->xy, s->len, s->guide,
                                               out + 5 * (size_t)l_len * k);
    }
    else {
        const int2 blk = blocks[blockIdx.x >> 6];
        const GuidedSet* s = sets + blk.x;
        g_match_row<unsigned char, int, true>(s->desc, s->xy, s->len, blk.y + 4 * (int)(blockIdx.x & 63u) + w, left,
                                              geo + (size_t)l_len * blk.x, l_len, s->guide, out + 5 * (size_t)s->roff);
    }
}

size_t pad16(size_t b) { return (b + 15) & ~(size_t)15; }

bool guide_none(const psx_guide& g) { return g.kind == PSX_GUIDE_NONE; }

// host_pairs or d_pairs (the other is NULL; both NULL with capacity 0)
int match_pairs_guided_many(int device, const unsigned char* d_left, const float* d_left_xy, int l_len,
                            const unsigned char* const* d_rights, const float* const* d_right_xys, const int* r_lens, int n_sets,
                            const psx_guide* guides, const psx_match_opts* opts, void* host_pairs, void* d_pairs, int capacity,
                            int* set_counts, int* count)
{
    if (!psx_pairs_args_ok(l_len, 0, opts, host_pairs ? host_pairs : d_pairs, capacity, count) || (l_len > 0 && (!d_left || !d_left_xy)) ||
        n_sets < 0 || (n_sets > 0 && (!d_rights || !d_right_xys || !r_lens || !set_counts || !guides)) ||
        !psx_many_sets_ok(l_len, r_lens, n_sets))
        return PSX_ERR_INVALID;
    for (int k = 0; k < n_sets; k++)                                 // every guide, before anything else is looked at
        if (!guide_none(guides[k]) && !psx_guide_valid(guides + k)) return PSX_ERR_INVALID;
    const int K = n_sets;
    thread_local std::vector<int> elen;                              // the lengths the call works with: 0 for a skipped set
    elen.resize((size_t)K);
    long long r_total = 0;
    for (int k = 0; k < K; k++) {
        elen[(size_t)k] = guide_none(guides[k]) ? 0 : r_lens[k];
        if (elen[(size_t)k] > 0 && (!d_rights[k] || !d_right_xys[k])) return PSX_ERR_INVALID;
        r_total += elen[(size_t)k];
    }
    if (l_len == 0 || r_total == 0) {
        for (int k = 0; k < K; k++) set_counts[k] = 0;
        *count = 0;
        return PSX_OK;
    }
    const bool mutual = (opts->flags & PSX_PAIRS_MUTUAL) != 0;

    // ---- sizes: the grids, the tables, the results ----
    thread_local std::vector<psx_many_block> rblk;
    const long long BR = mutual ? psx_many_blocks(elen.data(), K, nullptr, 0) : 0;
    const long long per_set = ((long long)l_len + 3) / 4;            // forward workgroups per set
    const long long nb = ((long long)l_len + 255) / 256, ntot = (long long)K * nb;       // the join's workgroups
    const long long all_pairs = (long long)K * l_len;                // at most l_len pairs per set exist
    if (ntot + 1 > INT_MAX || BR * 64 > INT_MAX || (long long)K * per_set > INT_MAX) return PSX_ERR_NOMEM;
    rblk.resize((size_t)BR);
    if (mutual) psx_many_blocks(elen.data(), K, rblk.data(), BR);
    const size_t sets_b = sizeof(GuidedSet) * (size_t)K;
    const size_t blocks_b = pad16(sizeof(int2) * (size_t)BR);
    const size_t blob_b = sets_b + blocks_b;
    const size_t nrec = host_pairs ? (size_t)(capacity < all_pairs ? capacity : all_pairs) : 0;
    const size_t off_counts = 16, off_rec = off_counts + pad16(sizeof(int) * (size_t)K), off_blob = off_rec + 16 * nrec;

    if (hipSetDevice(device) != hipSuccess) return PSX_ERR_HIP;
    MatchScratch& sc = psx_match_scratch();
    if (!sc.bind(device)) return PSX_ERR_HIP;
    // every buffer before the first launch: nothing is reallocated under queued work
    if (!sc.need(MS_GMANY_TABLES, blob_b) || !sc.need(MS_GMANY_FWD, sizeof(int) * 5 * (size_t)all_pairs) ||
        (mutual && (!sc.need(MS_GMANY_BWD, sizeof(int) * 5 * (size_t)r_total) || !sc.need(MS_GMANY_LINES, sizeof(float4) * (size_t)all_pairs))) ||
        !sc.need(MS_GMANY_TOT, sizeof(int) * (2 * (size_t)ntot + 1)) || !sc.need_pinned(off_blob + blob_b))
        return PSX_ERR_NOMEM;
    void* dev_pin = nullptr;
    if (hipHostGetDevicePointer(&dev_pin, sc.hpin, 0) != hipSuccess || dev_pin == nullptr) return PSX_ERR_HIP;
    char* hp = static_cast<char*>(sc.hpin);

    // ---- the tables, written into the pinned staging buffer and copied on the stream ----
    {
        GuidedSet* hs = reinterpret_cast<GuidedSet*>(hp + off_blob);
        int2* hb = reinterpret_cast<int2*>(hp + off_blob + sets_b);
        long long roff = 0;
        for (int k = 0; k < K; k++) {
            const int n = elen[(size_t)k];
            hs[k] = GuidedSet{n > 0 ? d_rights[k] : nullptr, n > 0 ? reinterpret_cast<const float2*>(d_right_xys[k]) : nullptr, n, (int)roff,
                              guides[k], {0, 0, 0}};
            roff += n;
        }
        for (long long b = 0; b < BR; b++) hb[b] = make_int2(rblk[(size_t)b].set, rblk[(size_t)b].row0);
    }
    int* h_total = reinterpret_cast<int*>(hp);
    *h_total = -1;
    const GuidedSet* d_sets = static_cast<const GuidedSet*>(sc.buf[MS_GMANY_TABLES]);
    const int2* d_blocks = reinterpret_cast<const int2*>(static_cast<const char*>(sc.buf[MS_GMANY_TABLES]) + sets_b);
    const float2* lxy = reinterpret_cast<const float2*>(d_left_xy);
    int* d_fwd = static_cast<int*>(sc.buf[MS_GMANY_FWD]);
    int* d_bwd = mutual ? static_cast<int*>(sc.buf[MS_GMANY_BWD]) : nullptr;
    float4* d_lines = mutual ? static_cast<float4*>(sc.buf[MS_GMANY_LINES]) : nullptr;
    int* d_total = static_cast<int*>(dev_pin);
    int* d_counts = reinterpret_cast<int*>(static_cast<char*>(dev_pin) + off_counts);
    // the kernel's capacity for the host form is the staging buffer's (nrec <= capacity)
    int4* out = host_pairs ? reinterpret_cast<int4*>(static_cast<char*>(dev_pin) + off_rec) : static_cast<int4*>(d_pairs);
    const int cap = host_pairs ? (int)nrec : capacity;
    hipStream_t st = sc.stream;

    if (hipMemcpyAsync(sc.buf[MS_GMANY_TABLES], hp + off_blob, blob_b, hipMemcpyHostToDevice, st) != hipSuccess) return PSX_ERR_HIP;
    if (mutual) {
        hipLaunchKernelGGL(k_guide_lines_many, dim3((unsigned)((all_pairs + 255) / 256)), dim3(256), 0, st, d_sets, lxy, l_len, all_pairs, d_lines);
        hipLaunchKernelGGL(k_match_guided_many<true>, dim3((unsigned)(BR * 64)), dim3(256), 0, st, d_sets, d_blocks, d_left, lxy, l_len, 0,
                           static_cast<const float4*>(d_lines), d_bwd);
    }
    hipLaunchKernelGGL(k_match_guided_many<false>, dim3((unsigned)(K * per_set)), dim3(256), 0, st, d_sets, d_blocks, d_left, lxy, l_len,
                       (int)per_set, static_cast<const float4*>(nullptr), d_fwd);
    psx_many_join_queue<int>(st, d_sets, d_fwd, l_len, d_bwd, (int)nb, (int)ntot, opts->ratio, mutual, static_cast<int*>(sc.buf[MS_GMANY_TOT]),
                        out, cap, d_counts, d_total);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return PSX_ERR_HIP;
    const int n = *h_total;
    if (n < 0 || n > all_pairs) return PSX_ERR_HIP;
    memcpy(set_counts, hp + off_counts, sizeof(int) * (size_t)K);
    if (host_pairs && n > 0 && nrec > 0) memcpy(host_pairs, hp + off_rec, 16 * ((size_t)n < nrec ? (size_t)n : nrec));
    *count = n;
    return PSX_OK;
}

} // namespace

extern "C" int psx_match_pairs_guided_many_u8(int device, const unsigned char* d_left, const float* d_left_xy, int l_len,
                                              const unsigned char* const* d_rights, const float* const* d_right_xys, const int* r_lens,
                                              int n_sets, const psx_guide* guides, const psx_match_opts* opts,
                                              psx_match_pair_u8* host_pairs, int capacity, int* set_counts, int* count)
{
    return match_pairs_guided_many(device, d_left, d_left_xy, l_len, d_rights, d_right_xys, r_lens, n_sets, guides, opts, host_pairs, nullptr,
                                   capacity, set_counts, count);
}

extern "C" int psx_match_pairs_guided_many_u8_dev(int device, const unsigned char* d_left, const float* d_left_xy, int l_len,
                                                  const unsigned char* const* d_rights, const float* const* d_right_xys, const int* r_lens,
                                                  int n_sets, const psx_guide* guides, const psx_match_opts* opts,
                                                  psx_match_pair_u8* d_pairs, int capacity, int* set_counts, int* count)
{
    return match_pairs_guided_many(device, d_left, d_left_xy, l_len, d_rights, d_right_xys, r_lens, n_sets, guides, opts, nullptr, d_pairs,
                                   capacity, set_counts, count);
}

extern "C" int psx_guides_from_ransac(const psx_ransac_result* results, int n_sets, int kind, float tol, psx_guide* guides)
{
    if (n_sets < 0 || (n_sets > 0 && (!results || !guides)) || (kind != PSX_GUIDE_HOMOGRAPHY && kind != PSX_GUIDE_EPIPOLAR) ||
        !(tol >= 0.0f && tol < INFINITY))
        return PSX_ERR_INVALID;
    for (int k = 0; k < n_sets; k++) {
        guides[k].kind = results[k].best < 0 ? PSX_GUIDE_NONE : kind;
        memcpy(guides[k].m, results[k].m, sizeof(guides[k].m));
        guides[k].tol = tol;
    }
    return PSX_OK;
}
