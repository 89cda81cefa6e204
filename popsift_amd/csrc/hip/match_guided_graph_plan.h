// match_guided_graph_plan.h -- the host side of the guided re-match over an edge list (psx_match_pairs_guided_graph_u8,
// include/popsift_hip.h): the argument checks, and the tables the kernels of match_guided_graph.hip walk.
//
// Plain C++14, no HIP: match_guided_graph.hip builds its device tables with these functions, and a stand-alone program can
// include the header alone (tests/cpp/graph_chain_plan_san.cpp).
//
// An edge is LIVE when its guide is not of kind PSX_GUIDE_NONE and both its sets have rows; every other edge -- skipped or
// with an empty side -- has count 0, appears in no block table and nothing of it is read.  Per edge (psx_gg_edge):
//   l_len, r_len   the lengths the call works with: both 0 for an edge that is not live
//   foff           its first forward row = the sum of l_len over the edges before it; the lines of the backward search
//                  are one per left row, so the edge's first LINE is foff too
//   boff           its first backward row = the sum of r_len over the edges before it
//   jf0            its first entry of the forward block table, which is also the join's
// A direction's block table is {edge, row0}: 256 outer rows of ONE edge, edge-major and ascending within the edge; a block
// never crosses an edge.
#pragma once

#include "guide_rule.h"
#include "match_graph_plan.h"
#include "match_join.h"

struct psx_gg_edge { int left, right, l_len, r_len, foff, boff, jf0, pad; };
struct psx_gg_totals { long long frows, brows, fblocks, bblocks; int live; };

inline bool psx_gg_skipped(const psx_guide& g) { return g.kind == PSX_GUIDE_NONE; }

// What every entry point refuses, before anything else is looked at: what psx_match_pairs_graph_u8 refuses (opts, output,
// capacity, count, the sets and the edges) and what psx_match_pairs_guided_many_u8 refuses (the guides -- every one is
// checked -- and the position arrays).  sets[s] / xys[s] are device pointers: only NULL is looked at.
template <class T>
inline bool psx_gg_args_ok_t(const T* const* sets, const float* const* xys, const int* lens, int n_sets, const psx_view_edge* edges,
                           int n_edges, const psx_guide* guides, const psx_match_opts* opts, const void* pairs, int capacity,
                           const int* edge_counts, const int* count)
{
    if (!psx_pairs_args_ok(0, 0, opts, pairs, capacity, count) || (n_sets > 0 && (sets == nullptr || xys == nullptr)) ||
        (n_edges > 0 && (edge_counts == nullptr || guides == nullptr)) || !psx_graph_args_ok(lens, n_sets, edges, n_edges))
        return false;
    for (int s = 0; s < n_sets; s++)
        if (lens[s] > 0 && (sets[s] == nullptr || xys[s] == nullptr)) return false;
    for (int e = 0; e < n_edges; e++)
        if (!psx_gg_skipped(guides[e]) && !psx_guide_valid(guides + e)) return false;
    return true;
}
inline bool psx_gg_args_ok(const unsigned char* const* sets, const float* const* xys, const int* lens, int n_sets, const psx_view_edge* edges,
                           int n_edges, const psx_guide* guides, const psx_match_opts* opts, const void* pairs, int capacity,
                           const int* edge_counts, const int* count)
{
    return psx_gg_args_ok_t(sets, xys, lens, n_sets, edges, n_edges, guides, opts, pairs, capacity, edge_counts, count);
}
// the float forms (psx_match_pairs_guided_graph): the same checks
inline bool psx_gg_args_ok(const float* const* sets, const float* const* xys, const int* lens, int n_sets, const psx_view_edge* edges,
                           int n_edges, const psx_guide* guides, const psx_match_opts* opts, const void* pairs, int capacity,
                           const int* edge_counts, const int* count)
{
    return psx_gg_args_ok_t(sets, xys, lens, n_sets, edges, n_edges, guides, opts, pairs, capacity, edge_counts, count);
}

inline long long psx_gg_nblocks(int len) { return ((long long)len + PSX_MANY_BLOCK - 1) / PSX_MANY_BLOCK; }

// The per-edge plan (ep: n_edges entries, all of them written) and the totals.  The row sums fit an int: psx_graph_args_ok
// bounds them over ALL edges.
inline psx_gg_totals psx_gg_edges(const int* lens, const psx_view_edge* edges, int n_edges, const psx_guide* guides, psx_gg_edge* ep)
{
    psx_gg_totals t = {0, 0, 0, 0, 0};
    for (int e = 0; e < n_edges; e++) {
        const bool live = !psx_gg_skipped(guides[e]) && psx_graph_live(lens, edges[e]);
        const int l = live ? lens[edges[e].left] : 0, r = live ? lens[edges[e].right] : 0;
        ep[e] = psx_gg_edge{edges[e].left, edges[e].right, l, r, (int)t.frows, (int)t.brows, (int)t.fblocks, 0};
        t.frows += l; t.brows += r;
        t.fblocks += psx_gg_nblocks(l); t.bblocks += psx_gg_nblocks(r);
        t.live += live;
    }
    return t;
}

// one direction's {edge, row0} table, edge-major; out may be NULL (count only), nothing is written at or past cap
inline long long psx_gg_blocks(const psx_gg_edge* ep, int n_edges, int backward, psx_graph_wg* out, long long cap)
{
    long long n = 0;
    for (int e = 0; e < n_edges; e++) {
        const int rows = backward ? ep[e].r_len : ep[e].l_len;
        for (long long row0 = 0; row0 < rows; row0 += PSX_MANY_BLOCK, n++)
            if (out != nullptr && n < cap) { out[n].edge = e; out[n].row0 = (int)row0; }
    }
    return n;
}
