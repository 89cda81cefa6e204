// match_graph_plan.h -- the tables of the pair search over an edge list (psx_match_pairs_graph_u8, include/popsift_hip.h):
// which rows every workgroup of k_match_u8_graph (match_graph.hip) takes on its outer and on its inner side, where every
// edge's results and partials lie, and which runs of whole edges share the partials' buffer.
//
// Plain C++14, no HIP: match_graph.hip builds its device tables with these functions, psx_match_graph_plan reports their
// sizes, and a stand-alone program can include the header alone (tests/cpp/match_graph_plan_san.cpp).  The cuts and the
// constants are those of match_many_plan.h.
//
// A set is REFERENCED when an edge with two non-empty sides names it; every other set counts as empty (psx_graph_eff) and
// appears in no table.  Every referenced set is cut ONCE per call -- outer blocks of 256 rows (psx_many_blocks), inner
// chunks of whole tiles at ONE chunk length for the call (psx_graph_chunk_len, psx_many_chunks_of) --, and a cut says
// where the set's blocks and chunks lie in the two tables (psx_graph_cut).  An edge then costs no cutting at all:
//   forward items of edge e   blocks(left_e) x chunks(right_e), one workgroup each; the chunk runs slower than the block
//   backward items            blocks(right_e) x chunks(left_e), with the cross-check only
//   merge / join workgroups   {edge, row0}: 256 outer rows of one edge, edge-major -- the forward table is also the join's
// An item carries where its keys go: (its edge's partials) + (chunk among the inner set's chunks) x (outer rows), counted
// in key pairs from the start of its group's buffer.  A GROUP is a run of whole edges whose partials fit the budget; an
// edge above the budget is a group of its own.
#pragma once

#include "match_many_plan.h"

#include <vector>

constexpr long long PSX_GRAPH_PARTIAL_BUDGET = 256LL << 20;     // bytes of per-chunk partials one group of edges may take
constexpr long long PSX_GRAPH_INT_MAX = 2147483647LL;

struct psx_graph_cut { int b0, b1, c0, c1; };                  // a set's blocks [b0, b1) and chunks [c0, c1) in the tables
struct psx_graph_item { int block, chunk, pbase, edge; };      // 16 bytes: one workgroup of k_match_u8_graph
struct psx_graph_wg { int edge, row0; };                       // 256 outer rows of one edge
// one edge, as the device reads it (32 bytes): its sets, the first row of its forward / backward directed result among
// all edges' rows, the start of its partials in its forward / backward group, its first forward / backward {edge, row0}
struct psx_graph_edge { int left, right, foff, boff, pf, pb, jf0, jb0; };
struct psx_graph_group { int edge0, nedges, item0, nitems, wg0, nwgs; long long entries; };

inline bool psx_graph_live(const int* lens, const psx_view_edge& e) { return lens[e.left] > 0 && lens[e.right] > 0; }

// what every entry point refuses about its sets and edges, before anything else is looked at
inline bool psx_graph_args_ok(const int* lens, int n_sets, const psx_view_edge* edges, int n_edges)
{
    if (n_sets < 0 || n_edges < 0 || (n_sets > 0 && lens == nullptr) || (n_edges > 0 && edges == nullptr)) return false;
    for (int s = 0; s < n_sets; s++)
        if (lens[s] < 0) return false;
    long long lrows = 0, rrows = 0;
    for (int e = 0; e < n_edges; e++) {
        if (edges[e].left < 0 || edges[e].left >= n_sets || edges[e].right < 0 || edges[e].right >= n_sets) return false;
        lrows += lens[edges[e].left];
        rrows += lens[edges[e].right];
    }
    return lrows <= PSX_GRAPH_INT_MAX && rrows <= PSX_GRAPH_INT_MAX;
}

// eff[s] = lens[s] for a referenced set, 0 for every other (n_sets entries); returns the number of referenced sets
inline int psx_graph_eff(const int* lens, int n_sets, const psx_view_edge* edges, int n_edges, int* eff)
{
    for (int s = 0; s < n_sets; s++) eff[s] = 0;
    for (int e = 0; e < n_edges; e++)
        if (psx_graph_live(lens, edges[e])) { eff[edges[e].left] = lens[edges[e].left]; eff[edges[e].right] = lens[edges[e].right]; }
    int n = 0;
    for (int s = 0; s < n_sets; s++) n += eff[s] > 0;
    return n;
}

inline long long psx_graph_nblocks(int len) { return ((long long)len + PSX_MANY_BLOCK - 1) / PSX_MANY_BLOCK; }

// The call's one chunk length, as psx_many_chunk_len chooses it for a star -- enough workgroups for the chip, whole tiles,
// at most 512 rows -- with the whole call in view: a direction's workgroups are the sum over its edges of (outer blocks) x
// (inner rows / chunk length), so the length is that sum of (outer blocks) x (inner rows) over PSX_MANY_WGS.  With the
// cross-check the direction with fewer workgroups decides.  The result of the call cannot depend on it.
inline int psx_graph_chunk_len(const int* lens, const psx_view_edge* edges, int n_edges, bool mutual)
{
    long long wf = 0, wb = 0;
    for (int e = 0; e < n_edges; e++) {
        if (!psx_graph_live(lens, edges[e])) continue;
        const int l = lens[edges[e].left], r = lens[edges[e].right];
        wf += psx_graph_nblocks(l) * r;
        wb += psx_graph_nblocks(r) * l;
    }
    const long long w = mutual && wb < wf ? wb : wf;
    long long len = (w + PSX_MANY_WGS - 1) / PSX_MANY_WGS;
    len = ((len + PSX_MANY_TILE - 1) / PSX_MANY_TILE) * PSX_MANY_TILE;
    if (len < PSX_MANY_TILE) len = PSX_MANY_TILE;
    if (len > PSX_MANY_CHUNK_MAX) len = PSX_MANY_CHUNK_MAX;
    return (int)len;
}

// cuts[s] for every set (n_sets entries; an unreferenced set gets two empty ranges); false when a table would not fit an int
inline bool psx_graph_cuts(const int* eff, int n_sets, int chunk_len, psx_graph_cut* cuts, long long* blocks, long long* chunks)
{
    long long b = 0, c = 0;
    for (int s = 0; s < n_sets; s++) {
        const long long nb = psx_many_blocks(eff + s, 1, nullptr, 0), nc = psx_many_chunks_of(eff + s, 1, chunk_len, nullptr, 0);
        if (b + nb > PSX_GRAPH_INT_MAX || c + nc > PSX_GRAPH_INT_MAX) return false;
        cuts[s].b0 = (int)b; cuts[s].b1 = (int)(b + nb);
        cuts[s].c0 = (int)c; cuts[s].c1 = (int)(c + nc);
        b += nb; c += nc;
    }
    *blocks = b; *chunks = c;
    return true;
}

// The per-edge plan (ep: n_edges entries, all of them written) and the groups of both directions (fg / bg: count and fill,
// nothing written at or past the capacity; *nfg / *nbg are always the totals; the backward direction only with mutual).
// An edge with an empty side has no rows, no partials and no workgroups: its offsets are those of the next edge.
// *items / *wgs [2]: the item and {edge, row0} totals forward and backward; *entries: the key pairs of the largest group.
// False when an offset, a table or a group's partials would not fit an int.
inline bool psx_graph_edges(const int* lens, const psx_graph_cut* cuts, const psx_view_edge* edges, int n_edges, bool mutual,
                            long long budget_bytes, psx_graph_edge* ep, psx_graph_group* fg, long long fcap, long long* nfg,
                            psx_graph_group* bg, long long bcap, long long* nbg, long long* items, long long* wgs, long long* entries)
{
    *nfg = *nbg = 0; items[0] = items[1] = 0; wgs[0] = wgs[1] = 0; *entries = 0;
    long long foff = 0, boff = 0;
    for (int e = 0; e < n_edges; e++) {
        const bool live = psx_graph_live(lens, edges[e]);
        ep[e] = psx_graph_edge{edges[e].left, edges[e].right, (int)foff, (int)boff, 0, 0, 0, 0};
        if (live) { foff += lens[edges[e].left]; boff += lens[edges[e].right]; }       // <= INT_MAX: psx_graph_args_ok
    }
    for (int dir = 0; dir < (mutual ? 2 : 1); dir++) {
        psx_graph_group* out = dir ? bg : fg;
        const long long cap = dir ? bcap : fcap;
        long long ng = 0, nitems = 0, nwgs = 0;
        psx_graph_group g = {0, 0, 0, 0, 0, 0, 0};
        for (int e = 0; e <= n_edges; e++) {
            long long en = 0, it = 0, wg = 0;
            if (e < n_edges && psx_graph_live(lens, edges[e])) {
                const int o = dir ? edges[e].right : edges[e].left, i = dir ? edges[e].left : edges[e].right;
                const long long nb = cuts[o].b1 - cuts[o].b0, nc = cuts[i].c1 - cuts[i].c0;
                en = nc * lens[o]; it = nb * nc; wg = nb;
            }
            // the group ends: at the list's end, or when this edge's partials no longer fit behind the group's
            if (e == n_edges || (g.nitems > 0 && 8 * (g.entries + en) > budget_bytes)) {
                if (g.nitems > 0) {
                    if (out != nullptr && ng < cap) out[ng] = g;
                    if (g.entries > *entries) *entries = g.entries;
                    ng++;
                }
                g = psx_graph_group{e, 0, (int)nitems, 0, (int)nwgs, 0, 0};
                if (e == n_edges) break;
            }
            if (g.entries + en > PSX_GRAPH_INT_MAX || nitems + it > PSX_GRAPH_INT_MAX || nwgs + wg > PSX_GRAPH_INT_MAX) return false;
            if (dir) { ep[e].pb = (int)g.entries; ep[e].jb0 = (int)nwgs; } else { ep[e].pf = (int)g.entries; ep[e].jf0 = (int)nwgs; }
            g.nedges++; g.entries += en; g.nitems += (int)it; g.nwgs += (int)wg;
            nitems += it; nwgs += wg;
        }
        (dir ? *nbg : *nfg) = ng;
        items[dir] = nitems; wgs[dir] = nwgs;
    }
    return true;
}

// one direction's items, edge-major, the chunk slower than the block; nothing is written at or past cap
inline long long psx_graph_items(const int* lens, const psx_graph_cut* cuts, const psx_graph_edge* ep, int n_edges, int backward,
                                 psx_graph_item* out, long long cap)
{
    long long n = 0;
    for (int e = 0; e < n_edges; e++) {
        const int o = backward ? ep[e].right : ep[e].left, i = backward ? ep[e].left : ep[e].right;
        if (lens[o] <= 0 || lens[i] <= 0) continue;
        const long long base = backward ? ep[e].pb : ep[e].pf;
        for (int c = cuts[i].c0; c < cuts[i].c1; c++)
            for (int b = cuts[o].b0; b < cuts[o].b1; b++, n++)
                if (out != nullptr && n < cap) out[n] = psx_graph_item{b, c, (int)(base + (long long)(c - cuts[i].c0) * lens[o]), e};
    }
    return n;
}

// one direction's {edge, row0} table, edge-major; nothing is written at or past cap
inline long long psx_graph_wgs(const int* lens, const psx_graph_edge* ep, int n_edges, int backward, psx_graph_wg* out, long long cap)
{
    long long n = 0;
    for (int e = 0; e < n_edges; e++) {
        const int o = backward ? ep[e].right : ep[e].left, i = backward ? ep[e].left : ep[e].right;
        if (lens[o] <= 0 || lens[i] <= 0) continue;
        for (long long row0 = 0; row0 < lens[o]; row0 += PSX_MANY_BLOCK, n++)
            if (out != nullptr && n < cap) { out[n].edge = e; out[n].row0 = (int)row0; }
    }
    return n;
}

// psx_match_graph_plan (include/popsift_hip.h)
inline int psx_graph_plan_host(const int* lens, int n_sets, const psx_view_edge* edges, int n_edges, int flags, psx_graph_plan_info* out)
{
    if (out == nullptr || (flags & ~PSX_PAIRS_MUTUAL) != 0 || !psx_graph_args_ok(lens, n_sets, edges, n_edges)) return PSX_ERR_INVALID;
    const bool mutual = (flags & PSX_PAIRS_MUTUAL) != 0;
    psx_graph_plan_info r = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    std::vector<int> eff((size_t)n_sets + 1);
    std::vector<psx_graph_cut> cuts((size_t)n_sets + 1);
    std::vector<psx_graph_edge> ep((size_t)n_edges + 1);
    r.referenced_sets = psx_graph_eff(lens, n_sets, edges, n_edges, eff.data());
    if (r.referenced_sets == 0) { *out = r; return PSX_OK; }
    r.chunk_len = psx_graph_chunk_len(lens, edges, n_edges, mutual);
    long long blocks = 0, chunks = 0, nfg = 0, nbg = 0, items[2], wgs[2], entries = 0;
    if (!psx_graph_cuts(eff.data(), n_sets, r.chunk_len, cuts.data(), &blocks, &chunks) ||
        !psx_graph_edges(lens, cuts.data(), edges, n_edges, mutual, PSX_GRAPH_PARTIAL_BUDGET, ep.data(), nullptr, 0, &nfg, nullptr, 0, &nbg,
                         items, wgs, &entries))
        return PSX_ERR_NOMEM;
    r.blocks = (int)blocks; r.chunks = (int)chunks;
    r.fwd_items = (int)items[0]; r.bwd_items = (int)items[1];
    r.fwd_groups = (int)nfg; r.bwd_groups = (int)nbg;
    r.join_workgroups = (int)wgs[0];
    r.launches = 1 + 2 * (r.fwd_groups + r.bwd_groups) + 3;
    r.scratch_bytes = 8 * entries;
    *out = r;
    return PSX_OK;
}
