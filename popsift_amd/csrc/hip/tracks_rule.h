// tracks_rule.h -- the rule of feature tracks over a view graph's pair lists (psx_tracks_graph*, include/popsift_hip.h).
//
// ONE set of inline functions, compiled for the host (the reference psx_tracks_graph_ref, tracks_plan.h) and for the
// device (tracks.hip): the two cannot drift apart.  Integers only.
//
// NODES.  Row r of view v is node g = off[v] + r, off = the exclusive prefix sum of lens, M = the sum of lens.
// JOINS.  A 16-byte record of edge e, of which only the first two ints {left, right} are read, joins node
//         (edges[e].left, left) with node (edges[e].right, right).  Nothing is special-cased: duplicate edges and duplicate
//         records join again (a no-op), (a, b) and (b, a) are two edges, on an edge with left == right a record with equal
//         rows is a self-loop (a no-op) and one with different rows joins two rows of ONE view.
// COMPONENTS.  The transitive closure of the joins; a component is named by its smallest node, its ROOT.  Whenever two
//         components are linked, the larger root goes under the smaller (psx_track_link): whatever the order of the
//         links, the root of a finished component is its minimum.
// TRACKS. A component is a track iff psx_track_keep: at least 2 members, in at least min_views distinct views, and no two
//         members in one view (a CONFLICT) unless PSX_TRACKS_KEEP_CONFLICTS is set.
// ORDER.  Tracks by ascending root; members of a track by ascending node, that is by view, then by row.
// TOTALS. components: those of 2 or more members; conflicts: the components with two members in one view; too_few_views:
//         the components of 2 or more members in fewer than min_views views -- a component may count in both, and neither
//         depends on the flags; joined_records: the records that are not self-loops.
#pragma once

#include "popsift_hip.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PSX_TRACKS_HD __host__ __device__
#else
#define PSX_TRACKS_HD
#endif

// options the entry points accept
PSX_TRACKS_HD inline bool psx_track_opts_ok(const psx_track_opts* o)
{
    return o != nullptr && o->min_views >= 2 && (o->flags & ~PSX_TRACKS_KEEP_CONFLICTS) == 0;
}

// a record's two rows lie inside ITS OWN edge's two views
PSX_TRACKS_HD inline bool psx_track_record_ok(int left, int right, int l_len, int r_len)
{
    return left >= 0 && left < l_len && right >= 0 && right < r_len;
}

// which of two different roots goes under the other: the larger under the smaller
PSX_TRACKS_HD inline void psx_track_link(int a, int b, int* child, int* parent)
{
    *child = a > b ? a : b;
    *parent = a > b ? b : a;
}

// is the component of `size` members in `views` distinct views, with (conflict != 0) or without two members in one view,
// a track?
PSX_TRACKS_HD inline bool psx_track_keep(int size, int views, int conflict, int min_views, int flags)
{
    if (size < 2 || views < min_views) return false;
    return conflict == 0 || (flags & PSX_TRACKS_KEEP_CONFLICTS) != 0;
}

// what a component adds to the totals components / conflicts / too_few_views
PSX_TRACKS_HD inline bool psx_track_is_component(int size) { return size >= 2; }
PSX_TRACKS_HD inline bool psx_track_is_conflict(int size, int conflict) { return size >= 2 && conflict != 0; }
PSX_TRACKS_HD inline bool psx_track_has_too_few(int size, int views, int min_views) { return size >= 2 && views < min_views; }
