// ransac_many_plan.h -- the host side of the batched geometric verification (psx_ransac_homography_many*,
// psx_ransac_fundamental_many*, psx_ransac_many_plan; include/popsift_hip.h): the argument checks every form shares, the
// block table the kernels of the one batched driver (ransac_graph.hip) walk, and the host reference.
//
// Plain C++14, no HIP: ransac_graph.hip builds its device tables with these functions, psx_ransac_many_plan hands them
// out, and a stand-alone program can include the header alone (tests/cpp/ransac_many_plan_san.cpp).
//
// The input is the concatenation P_0 .. P_{K-1} of K pair lists, set_counts[k] = |P_k|.  It is cut into
//   blocks {set, first, end}: pairs [first, end) OF THE CONCATENATION, all of one set, end - first <= block_rows
// A set's blocks are ascending and contiguous in the table and cover it exactly once; nothing spans two sets; a set with
// fewer than min_pairs pairs (4 for a homography, 8 for a fundamental matrix, 3 affine, 2 similarity: it has no model) contributes no block.
// The library plans twice: at PSX_RANSAC_MANY_SCORE_ROWS for the score kernel, at 256 for the gather and the compaction.
//
// The host reference is the loop over the single-list rule (psx_ransac_homography_host, psx_ransac_fundamental_host,
// psx_ransac_affine_host, psx_ransac_similarity_host: ransac_rule.h, fundamental_rule.h, affine_rule.h), nothing of which
// is restated here.  The loop stands once, psx_ransac_lists_host over LISTS WITH TWO SIDES (psx_ransac_sides): the star's
// reference below and the edge list's (ransac_graph_plan.h) check their own arguments and indices and hand it their sides.
#pragma once

#include "affine_rule.h"
#include "popsift_hip.h"

constexpr int PSX_RANSAC_MANY_SCORE_ROWS = 512;      // pairs per workgroup of the score kernel (256 lanes x 2 resident pairs)
constexpr int PSX_RANSAC_MANY_ROWS = 256;            // pairs per workgroup of the gather and of the compaction
constexpr long long PSX_RANSAC_MANY_MAX = 0x3fffffffLL;

// what every batched entry point refuses about its sets: the sum of the counts in *total
inline bool psx_ransac_many_sets_ok(const int* set_counts, int n_sets, long long* total)
{
    if (n_sets < 0 || (n_sets > 0 && set_counts == nullptr)) return false;
    long long sum = 0;
    for (int k = 0; k < n_sets; k++) {
        if (set_counts[k] < 0) return false;
        sum += set_counts[k];
    }
    if (total != nullptr) *total = sum;
    return sum <= PSX_RANSAC_MANY_MAX;
}

// blocks of the concatenation; out may be NULL (count only), nothing is written at or past cap
inline long long psx_ransac_many_blocks(const int* set_counts, int n_sets, int min_pairs, int block_rows, psx_ransac_block* out, long long cap)
{
    long long c = 0, first = 0;
    for (int s = 0; s < n_sets; s++) {
        const long long end = first + set_counts[s];
        if (set_counts[s] >= min_pairs)
            for (long long p = first; p < end; p += block_rows, c++)
                if (out != nullptr && c < cap) { out[c].set = s; out[c].first = (int)p; out[c].end = (int)(p + block_rows < end ? p + block_rows : end); }
        first = end;
    }
    return c;
}

// psx_ransac_many_plan (include/popsift_hip.h)
inline int psx_ransac_many_plan_host(const int* set_counts, int n_sets, int min_pairs, int block_rows, psx_ransac_block* blocks,
                                     int capacity, int* block_count)
{
    if (!psx_ransac_many_sets_ok(set_counts, n_sets, nullptr) || min_pairs < 1 || block_rows < 1 || block_count == nullptr || capacity < 0 ||
        (capacity > 0 && blocks == nullptr))
        return PSX_ERR_INVALID;
    *block_count = (int)psx_ransac_many_blocks(set_counts, n_sets, min_pairs, block_rows, blocks, capacity);       // <= sum + sets
    return PSX_OK;
}

// The argument checks of every batched form (the single call's, per set, and the sets' own), before anything is touched.
// pairs / left_xy / right_xys[k] are host or device pointers alike: only NULL is looked at.  *total = the sum of the counts.
inline bool psx_ransac_many_args_ok(const void* pairs, const int* set_counts, int n_sets, const float* left_xy, int l_len,
                                    const float* const* right_xys, const int* r_lens, const psx_ransac_opts* opts,
                                    const psx_ransac_result* results, const void* inliers, int capacity, const int* count, long long* total)
{
    long long sum = 0;
    if (!psx_ransac_opts_ok(opts) || count == nullptr || l_len < 0 || capacity < 0 || !psx_ransac_many_sets_ok(set_counts, n_sets, &sum)) return false;
    if (n_sets > 0 && (right_xys == nullptr || r_lens == nullptr || results == nullptr)) return false;
    if ((long long)n_sets * opts->hypotheses > PSX_RANSAC_MANY_MAX) return false;
    if ((sum > 0 && pairs == nullptr) || (l_len > 0 && left_xy == nullptr) || (capacity > 0 && inliers == nullptr)) return false;
    for (int k = 0; k < n_sets; k++)
        if (r_lens[k] < 0 || ((r_lens[k] > 0 || set_counts[k] > 0) && right_xys[k] == nullptr)) return false;
    *total = sum;
    return true;
}

// all sets "no model": what a call without a set at or above the minimum returns, and what the device forms start from
inline void psx_ransac_many_none(int n_sets, int N, psx_ransac_result* results, int* count, float* models, int* counts)
{
    for (int k = 0; k < n_sets; k++) psx_ransac_no_model(results + k);
    if (models != nullptr) for (size_t i = 0; i < 9 * (size_t)n_sets * (size_t)N; i++) models[i] = 0.0f;
    if (counts != nullptr) for (size_t i = 0; i < (size_t)n_sets * (size_t)N; i++) counts[i] = 0;
    *count = 0;
}

// the single-list host rule of a model (its id, affine_rule.h; the first two ids are guide kinds) and its sample size
inline psx_ransac_host_fn psx_ransac_many_rule(int model) { return psx_ransac_host_rule(model); }
inline int psx_ransac_many_min(int model) { return psx_ransac_host_min(model); }

// A LIST WITH TWO SIDES: what the star and the edge-list forms hand to the one driver (ransac_graph.hip) and to the one
// host loop below.  A star's lists share their left side; an edge's two sides come from the set array through its edge.
// The pointers are host or device pointers alike.
struct psx_ransac_sides { const float* lxy; int l_len; const float* rxy; int r_len; };

// the star's list k: the shared left array and set k's right array
inline psx_ransac_sides psx_ransac_many_side(const float* left_xy, int l_len, const float* const* right_xys, const int* r_lens, int k)
{
    return psx_ransac_sides{left_xy, l_len, right_xys[k], r_lens[k]};
}

// The host reference's loop, stated once: list e under the single-list rule on its own two sides, side_of(e).  The caller
// has checked its arguments and every pair index against its own lengths; nothing is written before the last refusal.
// `scratch` holds as many psx_ransac_pt as the longest list has pairs and is the caller's (a stand-alone program hands
// exact-size heap arrays to a sanitizer).
template <class SideOf>
inline int psx_ransac_lists_host(int kind, const void* pairs, const int* list_counts, int n_lists, SideOf side_of, const psx_ransac_opts* opts,
                                 psx_ransac_result* results, void* inliers, int capacity, int* count, float* models, int* counts,
                                 psx_ransac_pt* scratch)
{
    const int MIN = psx_ransac_many_min(kind);
    for (int e = 0; e < n_lists; e++)
        if (list_counts[e] >= MIN && scratch == nullptr) return PSX_ERR_INVALID;
    const int* rec = static_cast<const int*>(pairs);                             // 4 ints per record
    const int N = opts->hypotheses;
    psx_ransac_many_none(n_lists, N, results, count, models, counts);
    const psx_ransac_host_fn rule = psx_ransac_many_rule(kind);
    long long written = 0;                                                       // inliers of the lists before e
    size_t at = 0;
    for (int e = 0; e < n_lists; at += (size_t)list_counts[e], e++) {
        if (list_counts[e] < MIN) continue;
        const psx_ransac_sides s = side_of(e);
        const int room = written < capacity ? (int)(capacity - written) : 0;
        int c = 0;
        const int rc = rule(rec + 4 * at, list_counts[e], s.lxy, s.l_len, s.rxy, s.r_len, opts, results + e,
                            room > 0 ? static_cast<char*>(inliers) + 16 * (size_t)written : nullptr, room, &c,
                            models != nullptr ? models + 9 * (size_t)e * (size_t)N : nullptr, counts != nullptr ? counts + (size_t)e * (size_t)N : nullptr,
                            scratch);
        if (rc != PSX_OK) return rc;                                             // not reached: everything was checked above
        written += c;
    }
    *count = (int)written;
    return PSX_OK;
}

// The host reference (psx_ransac_*_many_ref): the star's argument checks, every pair index of every set against the left
// length and ITS OWN right length -- all before anything is written --, then the loop over its sides.
inline int psx_ransac_many_host(int kind, const void* pairs, const int* set_counts, int n_sets, const float* left_xy, int nl,
                                const float* const* right_xys, const int* r_lens, const psx_ransac_opts* opts, psx_ransac_result* results,
                                void* inliers, int capacity, int* count, float* models, int* counts, psx_ransac_pt* scratch)
{
    long long total = 0;
    if (!psx_ransac_many_args_ok(pairs, set_counts, n_sets, left_xy, nl, right_xys, r_lens, opts, results, inliers, capacity, count, &total))
        return PSX_ERR_INVALID;
    const int* rec = static_cast<const int*>(pairs);
    size_t at = 0;
    for (int k = 0; k < n_sets; k++)
        for (int p = 0; p < set_counts[k]; p++, at++)
            if (rec[4 * at] < 0 || rec[4 * at] >= nl || rec[4 * at + 1] < 0 || rec[4 * at + 1] >= r_lens[k]) return PSX_ERR_INVALID;
    return psx_ransac_lists_host(kind, pairs, set_counts, n_sets, [=](int k) { return psx_ransac_many_side(left_xy, nl, right_xys, r_lens, k); },
                                 opts, results, inliers, capacity, count, models, counts, scratch);
}
