// ransac_graph_plan.h -- the host side of the geometric verification over an edge list (psx_ransac_*_graph*,
// include/popsift_hip.h): the argument checks every form shares and the host reference.
//
// Plain C++14, no HIP: ransac_graph.hip checks its arguments with these functions, and a stand-alone program can include
// the header alone (tests/cpp/graph_chain_plan_san.cpp).
//
// The input is what psx_match_pairs_graph_u8* left: the concatenation P_0 .. P_{E-1} of the edges' pair lists in the order
// of the edge list, edge_counts[e] = |P_e|.  "Set" of the batched call becomes "edge": the block tables are those of
// ransac_many_plan.h (psx_ransac_many_blocks over edge_counts), unchanged.  What is new is that BOTH position arrays of a
// list come from the set array, through its edge: d_xys[edges[e].left] and d_xys[edges[e].right].
//
// The host reference is the loop over the single-list rule, which stands once for the star and the edge list
// (psx_ransac_lists_host, ransac_many_plan.h): here are the edge list's own checks and its sides.
#pragma once

#include "match_graph_plan.h"
#include "ransac_many_plan.h"

// The argument checks of every edge-list form, before anything is touched: what the batched forms refuse
// (psx_ransac_many_args_ok, "set" = edge), what psx_match_pairs_graph_u8 refuses about lens, n_sets, edges and n_edges
// (psx_graph_args_ok), and a NULL position array with a length or under an edge that has pairs.  pairs / xys[s] are host
// or device pointers alike: only NULL is looked at.  *total = the sum of the counts.
inline bool psx_ransac_graph_args_ok(const void* pairs, const int* edge_counts, const psx_view_edge* edges, int n_edges,
                                     const float* const* xys, const int* lens, int n_sets, const psx_ransac_opts* opts,
                                     const psx_ransac_result* results, const void* inliers, int capacity, const int* count, long long* total)
{
    long long sum = 0;
    if (!psx_ransac_opts_ok(opts) || count == nullptr || capacity < 0 || !psx_ransac_many_sets_ok(edge_counts, n_edges, &sum)) return false;
    if (!psx_graph_args_ok(lens, n_sets, edges, n_edges) || (n_sets > 0 && xys == nullptr) || (n_edges > 0 && results == nullptr)) return false;
    if ((long long)n_edges * opts->hypotheses > PSX_RANSAC_MANY_MAX) return false;
    if ((sum > 0 && pairs == nullptr) || (capacity > 0 && inliers == nullptr)) return false;
    for (int s = 0; s < n_sets; s++)
        if (lens[s] > 0 && xys[s] == nullptr) return false;
    for (int e = 0; e < n_edges; e++)
        if (edge_counts[e] > 0 && (xys[edges[e].left] == nullptr || xys[edges[e].right] == nullptr)) return false;
    *total = sum;
    return true;
}

// edge e's list: both sides through its edge
inline psx_ransac_sides psx_ransac_graph_side(const psx_view_edge* edges, const float* const* xys, const int* lens, int e)
{
    const int l = edges[e].left, r = edges[e].right;
    return psx_ransac_sides{xys[l], lens[l], xys[r], lens[r]};
}

// The host reference (psx_ransac_*_graph_ref): the edge list's argument checks, every pair index of every edge against
// ITS OWN two lengths -- all before anything is written --, then the loop over its sides (psx_ransac_lists_host).
inline int psx_ransac_graph_host(int kind, const void* pairs, const int* edge_counts, const psx_view_edge* edges, int n_edges,
                                 const float* const* xys, const int* lens, int n_sets, const psx_ransac_opts* opts, psx_ransac_result* results,
                                 void* inliers, int capacity, int* count, float* models, int* counts, psx_ransac_pt* scratch)
{
    long long total = 0;
    if (!psx_ransac_graph_args_ok(pairs, edge_counts, edges, n_edges, xys, lens, n_sets, opts, results, inliers, capacity, count, &total))
        return PSX_ERR_INVALID;
    const int* rec = static_cast<const int*>(pairs);
    size_t at = 0;
    for (int e = 0; e < n_edges; e++) {
        const int nl = lens[edges[e].left], nr = lens[edges[e].right];
        for (int p = 0; p < edge_counts[e]; p++, at++)
            if (rec[4 * at] < 0 || rec[4 * at] >= nl || rec[4 * at + 1] < 0 || rec[4 * at + 1] >= nr) return PSX_ERR_INVALID;
    }
    return psx_ransac_lists_host(kind, pairs, edge_counts, n_edges, [=](int e) { return psx_ransac_graph_side(edges, xys, lens, e); }, opts, results,
                                 inliers, capacity, count, models, counts, scratch);
}
