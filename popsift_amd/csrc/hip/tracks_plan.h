// tracks_plan.h -- the host side of feature tracks over an edge list (psx_tracks_graph*, psx_tracks_plan;
// include/popsift_hip.h): the argument checks every form shares, the sizes and tables the kernels of tracks.hip walk, and
// the host reference.
//
// Plain C++14, no HIP: tracks.hip checks its arguments and plans with these functions, psx_tracks_plan hands the plan
// out, and a stand-alone program can include the header alone (tests/cpp/tracks_plan_san.cpp).
//
// The input is what the graph calls leave: the concatenation P_0 .. P_{E-1} of the edges' record lists in the order of
// the edge list, edge_counts[e] = |P_e|.  The join kernel takes it in the 256-record blocks of ransac_many_plan.h
// (psx_ransac_many_blocks at a minimum of 1 record): {edge, first, end}, none crossing an edge.  The rule is
// tracks_rule.h; the reference below is a sequential union-find under it and is the definition of the result.
#pragma once

#include "match_graph_plan.h"
#include "ransac_many_plan.h"
#include "tracks_rule.h"

#include <new>
#include <vector>

constexpr int PSX_TRACKS_ROWS = 256;                  // records per workgroup of the join kernel, nodes per workgroup of the others
constexpr long long PSX_TRACKS_MAX = 0x3fffffffLL;    // nodes and records of one call
constexpr int PSX_TRACKS_LAUNCHES = 7;                // init, hook, flatten, [sort], segments, count, scan, write

// one edge as the join kernel reads it (16 bytes): the first nodes of its two views and their lengths
struct psx_tracks_edge { int l_off, r_off, l_len, r_len; };

// What every form, the plan among them, refuses about its sets and counts; *nodes = M, *records = the sum of the counts.
inline bool psx_tracks_sizes_ok(const int* lens, int n_sets, const int* edge_counts, int n_edges, long long* nodes, long long* records)
{
    if (n_sets < 0 || (n_sets > 0 && lens == nullptr)) return false;
    long long m = 0, sum = 0;
    for (int s = 0; s < n_sets; s++) {
        if (lens[s] < 0) return false;
        m += lens[s];
    }
    if (m > PSX_TRACKS_MAX || !psx_ransac_many_sets_ok(edge_counts, n_edges, &sum)) return false;     // the sum at most 0x3fffffff
    *nodes = m;
    *records = sum;
    return true;
}

// The argument checks of every form, before anything is touched.  pairs / labels / track_starts / members are host or
// device pointers alike: only NULL is looked at.
inline bool psx_tracks_args_ok(const void* pairs, const int* edge_counts, const psx_view_edge* edges, int n_edges, const int* lens, int n_sets,
                               const psx_track_opts* opts, const int* track_starts, int track_capacity, const psx_track_member* members,
                               int member_capacity, const psx_tracks_info* info, long long* nodes, long long* records)
{
    if (!psx_track_opts_ok(opts) || info == nullptr || track_capacity < 0 || member_capacity < 0) return false;
    if ((track_capacity > 0 && track_starts == nullptr) || (member_capacity > 0 && members == nullptr)) return false;
    if (!psx_tracks_sizes_ok(lens, n_sets, edge_counts, n_edges, nodes, records) || !psx_graph_args_ok(lens, n_sets, edges, n_edges)) return false;
    if (*records > 0 && pairs == nullptr) return false;
    for (int e = 0; e < n_edges; e++)                                            // no row can lie inside an empty view
        if (edge_counts[e] > 0 && (lens[edges[e].left] == 0 || lens[edges[e].right] == 0)) return false;
    return true;
}

// a call that touches no device: nothing to join, or no node
inline bool psx_tracks_trivial(long long nodes, long long records) { return nodes == 0 || records == 0; }

inline long long psx_tracks_record_blocks(const int* edge_counts, int n_edges)
{
    return psx_ransac_many_blocks(edge_counts, n_edges, 1, PSX_TRACKS_ROWS, nullptr, 0);
}

inline int psx_tracks_sort_bits(long long nodes)
{
    int bits = 1;
    while (bits < 31 && (1LL << bits) < nodes) bits++;
    return bits;
}

inline long long psx_tracks_pad16(long long b) { return (b + 15) & ~15LL; }
inline long long psx_tracks_node_wgs(long long nodes) { return (nodes + PSX_TRACKS_ROWS - 1) / PSX_TRACKS_ROWS; }
// the scratch of a call, slot by slot (tracks.hip takes exactly these)
inline long long psx_tracks_tables_bytes(int n_edges, long long blocks, int n_sets)
{
    return 16LL * n_edges + 16LL * blocks + psx_tracks_pad16(4LL * (n_sets + 1LL));
}
inline long long psx_tracks_nodes_bytes(long long nodes) { return 6 * 4 * nodes; }        // parent, view, begin, end, views, conflict
inline long long psx_tracks_sort_bytes(long long nodes) { return 4 * 4 * nodes; }         // keys and values, in and out
inline long long psx_tracks_tot_bytes(long long nodes) { return 4 * (4 * psx_tracks_node_wgs(nodes) + 2); }
constexpr long long PSX_TRACKS_STATE_BYTES = 32;                                          // the six totals, the flag, a pad

// psx_tracks_plan (include/popsift_hip.h)
inline int psx_tracks_plan_host(const int* lens, int n_sets, const int* edge_counts, int n_edges, psx_tracks_plan_info* out)
{
    long long nodes = 0, records = 0;
    if (out == nullptr || !psx_tracks_sizes_ok(lens, n_sets, edge_counts, n_edges, &nodes, &records)) return PSX_ERR_INVALID;
    psx_tracks_plan_info p = {(int)nodes, (int)records, 0, psx_tracks_sort_bits(nodes), 0, 0};
    if (!psx_tracks_trivial(nodes, records)) {
        const long long blocks = psx_tracks_record_blocks(edge_counts, n_edges);
        if (blocks > PSX_GRAPH_INT_MAX) return PSX_ERR_NOMEM;
        p.record_blocks = (int)blocks;
        p.launches = PSX_TRACKS_LAUNCHES;
        p.scratch_bytes = psx_tracks_tables_bytes(n_edges, blocks, n_sets) + psx_tracks_nodes_bytes(nodes) + psx_tracks_sort_bytes(nodes) +
                          psx_tracks_tot_bytes(nodes) + PSX_TRACKS_STATE_BYTES;
    }
    *out = p;
    return PSX_OK;
}

// off[0 .. n_sets]: the exclusive prefix sum of lens and M behind it
inline void psx_tracks_offsets(const int* lens, int n_sets, int* off)
{
    long long at = 0;
    for (int s = 0; s < n_sets; s++) { off[s] = (int)at; at += lens[s]; }
    off[n_sets] = (int)at;
}

// the result of a call that has nothing to join (host arrays): no track, every label -1
inline void psx_tracks_none(long long nodes, int* labels, int* track_starts, psx_tracks_info* info)
{
    if (labels != nullptr) for (long long g = 0; g < nodes; g++) labels[g] = -1;
    if (track_starts != nullptr) track_starts[0] = 0;
    *info = psx_tracks_info{0, 0, 0, 0, 0, 0};
}

inline int psx_tracks_find(std::vector<int>& parent, int x)
{
    while (parent[(size_t)x] != x) {                                            // path halving
        parent[(size_t)x] = parent[(size_t)parent[(size_t)x]];
        x = parent[(size_t)x];
    }
    return x;
}

// The host reference (psx_tracks_graph_ref): a sequential union-find.  Two passes: every argument and every record of
// every edge -- against ITS OWN two lengths -- is checked before anything is written.
inline int psx_tracks_host(const void* pairs, const int* edge_counts, const psx_view_edge* edges, int n_edges, const int* lens, int n_sets,
                           const psx_track_opts* opts, int* labels, int* track_starts, int track_capacity, psx_track_member* members,
                           int member_capacity, psx_tracks_info* info)
{
    long long nodes = 0, records = 0;
    if (!psx_tracks_args_ok(pairs, edge_counts, edges, n_edges, lens, n_sets, opts, track_starts, track_capacity, members, member_capacity, info,
                            &nodes, &records))
        return PSX_ERR_INVALID;
    const int* rec = static_cast<const int*>(pairs);                             // 4 ints per record
    size_t at = 0;
    for (int e = 0; e < n_edges; e++)
        for (int p = 0; p < edge_counts[e]; p++, at++)
            if (!psx_track_record_ok(rec[4 * at], rec[4 * at + 1], lens[edges[e].left], lens[edges[e].right])) return PSX_ERR_INVALID;
    if (psx_tracks_trivial(nodes, records)) { psx_tracks_none(nodes, labels, track_starts, info); return PSX_OK; }
    const size_t M = (size_t)nodes;
    std::vector<int> off, parent, size, views, last, conflict, number;
    try {
        off.resize((size_t)n_sets + 1);
        parent.resize(M); size.assign(M, 0); views.assign(M, 0); last.assign(M, -1); conflict.assign(M, 0); number.assign(M, -1);
    } catch (const std::bad_alloc&) { return PSX_ERR_NOMEM; }
    psx_tracks_offsets(lens, n_sets, off.data());
    for (size_t g = 0; g < M; g++) parent[g] = (int)g;
    psx_tracks_info t = {0, 0, 0, 0, 0, 0};
    at = 0;
    for (int e = 0; e < n_edges; e++)
        for (int p = 0; p < edge_counts[e]; p++, at++) {
            const int a = off[(size_t)edges[e].left] + rec[4 * at], b = off[(size_t)edges[e].right] + rec[4 * at + 1];
            if (a == b) continue;                                                // a self-loop
            t.joined_records++;
            const int ra = psx_tracks_find(parent, a), rb = psx_tracks_find(parent, b);
            if (ra == rb) continue;
            int child, par;
            psx_track_link(ra, rb, &child, &par);
            parent[(size_t)child] = par;
        }
    // per root: members, distinct views and the conflict mark; nodes ascend, so a component's views arrive in order
    int v = 0;
    for (size_t g = 0; g < M; g++) {
        while (off[(size_t)v + 1] <= (int)g) v++;
        const size_t r = (size_t)psx_tracks_find(parent, (int)g);
        size[r]++;
        if (last[r] == v) conflict[r] = 1;
        else { views[r]++; last[r] = v; }
    }
    // tracks by ascending root; number[r] = the track of root r, its members from `first` on
    std::vector<int>& first = last;                                              // reused: where the next member of root r goes
    for (size_t r = 0; r < M; r++) {
        if (parent[r] != (int)r) continue;
        if (psx_track_is_component(size[r])) t.components++;
        if (psx_track_is_conflict(size[r], conflict[r])) t.conflicts++;
        if (psx_track_has_too_few(size[r], views[r], opts->min_views)) t.too_few_views++;
        if (!psx_track_keep(size[r], views[r], conflict[r], opts->min_views, opts->flags)) continue;
        number[r] = t.tracks;
        first[r] = t.members;
        if (track_starts != nullptr && t.tracks <= track_capacity) track_starts[t.tracks] = t.members;
        t.tracks++;
        t.members += size[r];
    }
    if (track_starts != nullptr && t.tracks <= track_capacity) track_starts[t.tracks] = t.members;
    v = 0;
    for (size_t g = 0; g < M; g++) {
        while (off[(size_t)v + 1] <= (int)g) v++;
        const size_t r = (size_t)parent[g] == g ? g : (size_t)psx_tracks_find(parent, (int)g);
        const int n = number[r];
        if (labels != nullptr) labels[g] = n;
        if (n < 0) continue;
        const int slot = first[r]++;
        if (slot < member_capacity) members[slot] = psx_track_member{v, (int)g - off[(size_t)v]};
    }
    *info = t;
    return PSX_OK;
}
