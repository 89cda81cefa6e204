// match_graph_f32_plan.h -- how psx_match_pairs_graph (match_graph_f32.hip, include/popsift_hip.h) lays out one call: which
// of its two paths runs, how every referenced set is cut, the tables its kernels walk and the groups of whole edges.
//
// Plain C++14, no HIP: match_graph_f32.hip plans with psx_graph_f32_build, psx_match_graph_f32_plan reports what it
// decides, and a stand-alone program can include the header alone (tests/cpp/match_graph_f32_plan_san.cpp).
//
// The table shape is match_graph_plan.h's -- referenced sets, ONE cut per set and call, a flat item table of (outer block,
// inner chunk) per edge, the {edge, row0} table, groups of whole edges -- and the two paths and their constants are
// match_many_f32_plan.h's:
//   the rule    one decision per call for both directions.  With the LIVE edges (both sides non-empty, counted as listed,
//               duplicates included): the prefilter (path 2) runs iff POPSIFT_MATCH_MFMA is on, the sum of lens[right] is
//               at least PSX_MANYF_MIN_R and the sum of lens[left] at least PSX_MANYF_MIN_L x the number of live edges;
//               the exact scan (path 1) otherwise.  For a star this is psx_manyf_path.
//   scan        chunks of whole tiles at the call's one length, psx_graph_chunk_len (at most 512 rows)
//   prefilter   chunks of whole staged blocks of 64 rows at the call's one length (psx_graphf_pre_len): the SMALLEST
//               length between PSX_MANYF_PRE_MIN and PSX_MANYF_PRE_MAX at which the direction with fewer items has at most
//               PSX_MANYF_PRE_WGS items, the maximum if no length does.  Every set is cut into equal pieces of at most
//               that length.  The (distance, index) order is total: the result cannot depend on it.
// One buffer grows with (chunks x outer rows) -- 16 bytes per entry for the scan's top-2, PSX_MANYF_PRE_UNIT for the
// prefilter's two candidate segments and their counts -- and a group is a run of whole edges under PSX_MANYF_BUDGET of it
// (a single edge above the budget is a group of its own).  An edge's entries start at pf / pb (psx_graph_edge) in its
// group's buffer: the scan's partial of (chunk c, row) lies at pf + (c - c0) x (outer rows) + row, the prefilter's segments
// of (row, chunk c, half wave) at (pf + row x nchunks(inner) + (c - c0)) x 2 + half, the same count of entries either way.
#pragma once

#include "match_graph_plan.h"
#include "match_many_f32_plan.h"

#include <vector>

struct psx_graphf_tables {
    int path = 0;                                     // 0: no pair can exist, 1: scan, 2: prefilter
    int referenced = 0;                               // sets named by a live edge
    int chunk_len = 0;                                // the call's one chunk length on `path`
    std::vector<int> eff;                             // lens[s] of a referenced set, 0 of every other (n_sets entries)
    std::vector<int> foff;                            // a referenced set's first row in the gathered arrays
    std::vector<psx_graph_cut> cuts;                  // every set's blocks and chunks in the two tables
    std::vector<psx_graph_edge> ep;                   // the edge table
    std::vector<psx_graph_group> fg, bg;              // the groups of whole edges, forward and backward
    long long rows = 0;                               // rows of all referenced sets: the gathered arrays
    long long blocks = 0, chunks = 0;
    long long items[2] = {0, 0}, wgs[2] = {0, 0};     // forward / backward items and {edge, row0} entries
    long long entries = 0;                            // (chunk, outer row) entries of the largest group
    long long scratch_bytes = 0;                      // ... in bytes of the growing buffer
    int launches = 0;                                 // kernels queued when the flag stays down
};

// the rule (see above): 0 when no edge is live
inline int psx_graphf_path(const int* lens, const psx_view_edge* edges, int n_edges, bool mfma_enabled)
{
    long long live = 0, lrows = 0, rrows = 0;
    for (int e = 0; e < n_edges; e++)
        if (psx_graph_live(lens, edges[e])) { live++; lrows += lens[edges[e].left]; rrows += lens[edges[e].right]; }
    if (live == 0) return 0;
    return (mfma_enabled && rrows >= PSX_MANYF_MIN_R && lrows >= (long long)PSX_MANYF_MIN_L * live) ? 2 : 1;
}

// the prefilter's chunks of ONE set at a target length (whole staged blocks): equal pieces of whole staged blocks, as
// psx_manyf_pre_chunks cuts them; out may be NULL (count only), nothing is written at or past cap
inline long long psx_graphf_pre_chunks_of(const int* lens, int n, int target, psx_many_chunk* out, long long cap)
{
    long long c = 0;
    for (int s = 0; s < n; s++) {
        const long long len = lens[s];
        if (len <= 0) continue;
        const long long pieces = (len + target - 1) / target;
        long long step = (len + pieces - 1) / pieces;
        step = ((step + PSX_MANYF_PRE_STEP - 1) / PSX_MANYF_PRE_STEP) * PSX_MANYF_PRE_STEP;      // <= target: target is whole staged blocks
        for (long long r0 = 0; r0 < len; r0 += step, c++)
            if (out != nullptr && c < cap) {
                out[c].set = s; out[c].r0 = (int)r0; out[c].r1 = (int)(r0 + step < len ? r0 + step : len);
            }
    }
    return c;
}

// the prefilter's one chunk length of a call (see above)
inline int psx_graphf_pre_len(const int* lens, const psx_view_edge* edges, int n_edges, bool mutual)
{
    for (int len = PSX_MANYF_PRE_MIN; len < PSX_MANYF_PRE_MAX; len += PSX_MANYF_PRE_STEP) {
        long long wf = 0, wb = 0;
        for (int e = 0; e < n_edges; e++) {
            if (!psx_graph_live(lens, edges[e])) continue;
            const int* l = lens + edges[e].left;
            const int* r = lens + edges[e].right;
            wf += psx_graph_nblocks(*l) * psx_graphf_pre_chunks_of(r, 1, len, nullptr, 0);
            wb += psx_graph_nblocks(*r) * psx_graphf_pre_chunks_of(l, 1, len, nullptr, 0);
        }
        if ((mutual && wb < wf ? wb : wf) <= PSX_MANYF_PRE_WGS) return len;
    }
    return PSX_MANYF_PRE_MAX;
}

// the chunk table of a call on `path` at its chunk length; out may be NULL (count only)
inline long long psx_graphf_chunks(const int* eff, int n_sets, int path, int chunk_len, psx_many_chunk* out, long long cap)
{
    return path == 2 ? psx_graphf_pre_chunks_of(eff, n_sets, chunk_len, out, cap) : psx_many_chunks_of(eff, n_sets, chunk_len, out, cap);
}

// Tables and groups of one call on `path` (1 or 2; 0 leaves everything empty).  false: a table, a grid, a row's place in
// the gathered arrays or 32 x a group's segments does not fit an int (the caller answers PSX_ERR_NOMEM).
inline bool psx_graph_f32_build(const int* lens, int n_sets, const psx_view_edge* edges, int n_edges, bool mutual, int path,
                                psx_graphf_tables& t)
{
    t = psx_graphf_tables();
    t.path = path;
    t.eff.assign((size_t)n_sets + 1, 0);
    t.referenced = psx_graph_eff(lens, n_sets, edges, n_edges, t.eff.data());
    if (path == 0 || t.referenced == 0) { t.path = 0; return true; }
    t.foff.assign((size_t)n_sets + 1, 0);
    for (int s = 0; s < n_sets; s++) { t.foff[(size_t)s] = (int)t.rows; t.rows += t.eff[(size_t)s]; if (t.rows > PSX_GRAPH_INT_MAX) return false; }
    t.chunk_len = path == 2 ? psx_graphf_pre_len(lens, edges, n_edges, mutual) : psx_graph_chunk_len(lens, edges, n_edges, mutual);
    t.cuts.assign((size_t)n_sets + 1, psx_graph_cut{0, 0, 0, 0});
    for (int s = 0; s < n_sets; s++) {
        const long long nb = psx_many_blocks(t.eff.data() + s, 1, nullptr, 0), nc = psx_graphf_chunks(t.eff.data() + s, 1, path, t.chunk_len, nullptr, 0);
        if (t.blocks + nb > PSX_GRAPH_INT_MAX || t.chunks + nc > PSX_GRAPH_INT_MAX) return false;
        t.cuts[(size_t)s] = psx_graph_cut{(int)t.blocks, (int)(t.blocks + nb), (int)t.chunks, (int)(t.chunks + nc)};
        t.blocks += nb; t.chunks += nc;
    }
    // psx_graph_edges tests 8 x entries against its budget: the budget in units of this path's entries, times 8
    const long long unit = path == 2 ? PSX_MANYF_PRE_UNIT : PSX_MANYF_SCAN_UNIT;
    const long long budget8 = PSX_MANYF_BUDGET * 8 / unit;
    t.ep.assign((size_t)n_edges + 1, psx_graph_edge{0, 0, 0, 0, 0, 0, 0, 0});
    long long nfg = 0, nbg = 0;
    if (!psx_graph_edges(lens, t.cuts.data(), edges, n_edges, mutual, budget8, t.ep.data(), nullptr, 0, &nfg, nullptr, 0, &nbg, t.items, t.wgs,
                         &t.entries))
        return false;
    t.fg.resize((size_t)nfg); t.bg.resize((size_t)nbg);
    psx_graph_edges(lens, t.cuts.data(), edges, n_edges, mutual, budget8, t.ep.data(), t.fg.data(), nfg, &nfg, t.bg.data(), nbg, &nbg, t.items,
                    t.wgs, &t.entries);
    // the tables, the grids (one workgroup per item; 64 per {edge, row0} entry in the exact evaluation), a candidate slot's index
    if (t.items[0] + t.items[1] > PSX_GRAPH_INT_MAX || t.wgs[0] + t.wgs[1] + 1 > PSX_GRAPH_INT_MAX) return false;
    if (path == 2 && (64 * (t.wgs[0] > t.wgs[1] ? t.wgs[0] : t.wgs[1]) > PSX_GRAPH_INT_MAX || 2LL * PSX_MANYF_SEGCAP * t.entries > PSX_GRAPH_INT_MAX))
        return false;
    t.scratch_bytes = unit * t.entries;
    t.launches = (path == 2 ? 2 : 1) + 2 * (int)(nfg + nbg) + 3;
    return true;
}

// psx_match_graph_f32_plan (include/popsift_hip.h)
inline int psx_graph_f32_plan_host(const int* lens, int n_sets, const psx_view_edge* edges, int n_edges, int flags, int mfma_enabled,
                                   psx_graph_f32_plan_info* out)
{
    if (out == nullptr || (flags & ~PSX_PAIRS_MUTUAL) != 0 || (mfma_enabled != 0 && mfma_enabled != 1) ||
        !psx_graph_args_ok(lens, n_sets, edges, n_edges))
        return PSX_ERR_INVALID;
    psx_graphf_tables t;
    if (!psx_graph_f32_build(lens, n_sets, edges, n_edges, (flags & PSX_PAIRS_MUTUAL) != 0, psx_graphf_path(lens, edges, n_edges, mfma_enabled != 0), t))
        return PSX_ERR_NOMEM;
    psx_graph_f32_plan_info r = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    r.path = t.path;
    r.referenced_sets = t.referenced;
    r.blocks = (int)t.blocks; r.chunks = (int)t.chunks; r.chunk_len = t.chunk_len;
    r.fwd_items = (int)t.items[0]; r.bwd_items = (int)t.items[1];
    r.fwd_groups = (int)t.fg.size(); r.bwd_groups = (int)t.bg.size();
    r.join_workgroups = (int)t.wgs[0];
    r.launches = t.launches;
    r.scratch_bytes = t.scratch_bytes;
    *out = r;
    return PSX_OK;
}
