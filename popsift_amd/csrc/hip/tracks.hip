// tracks.hip -- feature tracks from a view graph's pair lists in one call: psx_tracks_graph (+ _dev, _ref) and
// psx_tracks_plan (include/popsift_hip.h).
//
// The chain psx_match_pairs_graph_u8* -> psx_ransac_*_graph* -> psx_match_pairs_guided_graph_u8* ends with E pair lists in
// HBM; a track is a connected component of the rows they join.  The rule is tracks_rule.h, the argument checks, the sizes
// and the host reference are tracks_plan.h; here is the device sequence, a union-find whose result does not depend on
// the order in which its lanes arrive:
//   k_tracks_init      parent[g] = g, the view of every node (a search of the offset table), zero marks and totals
//   k_tracks_hook      one lane per record of the 256-record blocks (none crosses an edge): the rows checked against ITS
//                      OWN edge's two lengths, both roots found with path halving, the LARGER root linked under the smaller
//                      by a compare-and-swap on the root's own slot; a lane whose swap fails finds again.  Only roots are
//                      linked and always downwards, so the root of a finished component is its smallest node whatever
//                      the arrival order.  No lane waits for another: a retry follows only a link that some other lane
//                      made, and there are fewer than M links.  parent is read and written with relaxed agent-scope
//                      atomics in this kernel (L1 is per CU and is not refreshed by other CUs' stores).
//   k_tracks_flatten   behind the kernel boundary: key[g] = root(g), value[g] = g
//   rocprim            ONE stable radix sort of (root, node) over ceil(log2 M) bits: the nodes arrive ascending, so a
//                      component's members come out in the rule's order
//   k_tracks_segments  per sorted position: begin and end of a component at its head and tail, the number of view changes
//                      inside it (an integer add) and the conflict mark where a neighbour has the same view (a store of
//                      1): integer atomics whose result does not depend on arrival order
//   k_tracks_count / k_tracks_scan / k_tracks_write   psx_track_keep per component into the stable compaction of
//                      wg_compact.h, twice over the same lanes: kept HEADS number the tracks, kept NODES place the members.
//                      The track of a kept node is (kept heads at or before its position) - 1: no lane reads what another
//                      workgroup wrote in the same launch.
// Launches per call, whatever n_edges, n_sets and M are: the table copy, 7 kernels and the sort, then one copy of the 32
// bytes of totals and ONE synchronisation.
#include "psx_internal.h"
#include "match_scratch.h"
#include "tracks_plan.h"
#include "wg_compact.h"

#include <cstring>
#include <rocprim/device/device_radix_sort.hpp>

namespace {

static_assert(PSX_TRACKS_ROWS == 256 && sizeof(psx_tracks_edge) == 16 && sizeof(psx_track_member) == 8, "block and record sizes");

// what the call brings back: the six totals of psx_tracks_info in its order, then the flag of a bad record
struct THead { int tracks, members, components, conflicts, too_few_views, joined_records, bad, pad; };
static_assert(sizeof(THead) == PSX_TRACKS_STATE_BYTES, "one 32-byte copy");

// per node / per root, M ints each
struct TNodes {
    int* parent;     // the union-find forest; after k_tracks_hook every tree's root is its smallest node
    int* view;       // the view of node g
    int* begin;      // [root] its component's first position in the sorted order
    int* end;        // [root] ... and one past its last
    int* changes;    // [root] view changes inside the component: distinct views - 1
    int* conflict;   // [root] 1: two members in one view
};

__device__ __forceinline__ int t_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void t_store(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The root of x's tree, halving the path behind it.  A node that has a parent once is never a root again and its parent
// only ever moves to a smaller ancestor, so every value read is an ancestor and x strictly descends: at most x steps.
__device__ __forceinline__ int t_find(int* parent, int x)
{
    for (;;) {
        const int p = t_load(parent + x);
        if (p == x) return x;
        const int gp = t_load(parent + p);
        if (gp != p) t_store(parent + x, gp);
        x = gp;
    }
}

// grid ceil(M / 256)
__global__ __launch_bounds__(256) void k_tracks_init(TNodes nd, const int* __restrict__ off, int n_sets, int M, THead* __restrict__ head)
{
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g == 0) *head = THead{0, 0, 0, 0, 0, 0, 0, 0};
    if (g >= M) return;
    int lo = 0, hi = n_sets;                                  // the last view whose offset is <= g: empty views before it lose
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= g) lo = mid; else hi = mid;
    }
    nd.parent[g] = g;
    nd.view[g] = lo;
    nd.changes[g] = 0;
    nd.conflict[g] = 0;
}

// grid: the 256-record blocks {edge, first, end}
__global__ __launch_bounds__(256) void k_tracks_hook(const int4* __restrict__ pairs, const psx_tracks_edge* __restrict__ edges,
                                                     const int4* __restrict__ blocks, int* parent, THead* head)
{
    const int4 blk = blocks[blockIdx.x];
    const psx_tracks_edge e = edges[blk.x];
    const int p = blk.y + (int)threadIdx.x;
    int a = 0, b = 0;
    if (p < blk.z) {
        const int4 rec = pairs[p];
        if (psx_track_record_ok(rec.x, rec.y, e.l_len, e.r_len)) { a = e.l_off + rec.x; b = e.r_off + rec.y; }
        else head->bad = 1;                                   // the record is skipped: nothing is indexed with it
    }
    const bool join = a != b;                                 // not a self-loop (a lane without a record: 0 == 0)
    const unsigned long long m = __ballot(join);
    if (m == 0) return;
    if ((threadIdx.x & 63) == 0) atomicAdd(&head->joined_records, __popcll(m));
    if (!join) return;
    for (;;) {
        a = t_find(parent, a);
        b = t_find(parent, b);
        if (a == b) return;                                   // already one component
        int child, par;
        psx_track_link(a, b, &child, &par);
        int expected = child;
        if (__hip_atomic_compare_exchange_strong(parent + child, &expected, par, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
            return;
        // `child` was linked by another lane in the meantime: both trees are found again
    }
}

// grid ceil(M / 256).  Plain loads: the kernel boundary made every link visible; nothing writes parent any more.
__global__ __launch_bounds__(256) void k_tracks_flatten(const int* __restrict__ parent, int M, unsigned* __restrict__ keys, unsigned* __restrict__ vals)
{
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= M) return;
    int x = g;
    for (int p = parent[x]; p != x; p = parent[x]) x = p;
    keys[g] = (unsigned)x;
    vals[g] = (unsigned)g;
}

// grid ceil(M / 256), one lane per sorted position
__global__ __launch_bounds__(256) void k_tracks_segments(const unsigned* __restrict__ roots, const unsigned* __restrict__ ids, int M, TNodes nd)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= M) return;
    const int r = (int)roots[i];
    const bool head = i == 0 || (int)roots[i - 1] != r, tail = i == M - 1 || (int)roots[i + 1] != r;
    if (head) nd.begin[r] = i;
    if (tail) nd.end[r] = i + 1;
    if (!head) {                                              // the members ascend, so equal views are neighbours
        if (nd.view[ids[i - 1]] == nd.view[ids[i]]) nd.conflict[r] = 1;
        else atomicAdd(nd.changes + r, 1);
    }
}

// what the count and the write kernel decide per sorted position, the same way
struct TLane { int root, node; bool head, keep; };

__device__ __forceinline__ TLane t_lane(const unsigned* __restrict__ roots, const unsigned* __restrict__ ids, int M, const TNodes& nd, int i,
                                        int min_views, int flags, int* size, int* views, int* conflict)
{
    TLane l = {0, 0, false, false};
    *size = 0; *views = 0; *conflict = 0;
    if (i >= M) return l;
    l.root = (int)roots[i];
    l.node = (int)ids[i];
    l.head = i == 0 || (int)roots[i - 1] != l.root;
    *size = nd.end[l.root] - nd.begin[l.root];
    *views = nd.changes[l.root] + 1;
    *conflict = nd.conflict[l.root];
    l.keep = psx_track_keep(*size, *views, *conflict, min_views, flags);
    return l;
}

// grid ceil(M / 256): wg_tot[w] = kept heads, wg_tot[gridDim.x + w] = kept nodes of workgroup w; the three component totals
__global__ __launch_bounds__(256) void k_tracks_count(const unsigned* __restrict__ roots, const unsigned* __restrict__ ids, int M, TNodes nd,
                                                      int min_views, int flags, int* __restrict__ wg_tot, THead* head)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    int size, views, conflict;
    const TLane l = t_lane(roots, ids, M, nd, i, min_views, flags, &size, &views, &conflict);
    const unsigned long long mc = __ballot(l.head && psx_track_is_component(size));
    const unsigned long long mx = __ballot(l.head && psx_track_is_conflict(size, conflict));
    const unsigned long long mf = __ballot(l.head && psx_track_has_too_few(size, views, min_views));
    if ((threadIdx.x & 63) == 0) {                            // integer sums: the order of arrival does not show
        if (mc) atomicAdd(&head->components, __popcll(mc));
        if (mx) atomicAdd(&head->conflicts, __popcll(mx));
        if (mf) atomicAdd(&head->too_few_views, __popcll(mf));
    }
    __shared__ int s_head[4], s_node[4];
    wg_count(__ballot(l.keep && l.head), s_head);
    wg_count(__ballot(l.keep), s_node);
    if (threadIdx.x == 0) {
        wg_tot[blockIdx.x] = wg_total(s_head);
        wg_tot[gridDim.x + blockIdx.x] = wg_total(s_node);
    }
}

// TWO workgroups of 1024 threads (wg_compact.h): 0 scans the heads' totals, 1 the nodes'; offs holds n + 1 ints for each
__global__ __launch_bounds__(1024) void k_tracks_scan(const int* __restrict__ wg_tot, int n, int* __restrict__ offs)
{
    wg_scan_totals(wg_tot + (size_t)blockIdx.x * (size_t)n, n, offs + (size_t)blockIdx.x * ((size_t)n + 1));
}

// grid as k_tracks_count.  Nothing is written at or past a capacity; labels may be NULL.
__global__ __launch_bounds__(256) void k_tracks_write(const unsigned* __restrict__ roots, const unsigned* __restrict__ ids, int M, TNodes nd,
                                                      const int* __restrict__ off, int min_views, int flags, const int* __restrict__ offs,
                                                      int* __restrict__ labels, int* __restrict__ track_starts, int track_capacity,
                                                      psx_track_member* __restrict__ members, int member_capacity, THead* head)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    int size, views, conflict;
    const TLane l = t_lane(roots, ids, M, nd, i, min_views, flags, &size, &views, &conflict);
    const bool khead = l.keep && l.head;
    const unsigned long long mh = __ballot(khead), mn = __ballot(l.keep);
    __shared__ int s_head[4], s_node[4];
    wg_count(mh, s_head);
    wg_count(mn, s_node);
    const int n = (int)gridDim.x;
    const int heads_before = offs[blockIdx.x] + wg_offset(mh, s_head);          // kept heads before this position
    const int slot = offs[n + 1 + blockIdx.x] + wg_offset(mn, s_node);          // kept nodes before it
    if (i < M) {
        const int track = heads_before + (khead ? 1 : 0) - 1;                   // a kept node's head is at or before it
        if (l.keep) {
            const int v = nd.view[l.node];
            if (slot < member_capacity) members[slot] = psx_track_member{v, l.node - off[v]};
            if (khead && track_starts != nullptr && track <= track_capacity) track_starts[track] = slot;
        }
        if (labels != nullptr) labels[l.node] = l.keep ? track : -1;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const int tracks = offs[n], total = offs[2 * n + 1];
        head->tracks = tracks;
        head->members = total;
        if (track_starts != nullptr && tracks <= track_capacity) track_starts[tracks] = total;
    }
}

bool aligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// host_pairs or d_pairs_in; the outputs either all host or all device (h_* / d_*), any of them NULL
int tracks_run(int device, const void* host_pairs, const void* d_pairs_in, const int* edge_counts, const psx_view_edge* edges, int n_edges,
               const int* lens, int n_sets, const psx_track_opts* opts, bool host_out, int* labels, int* track_starts, int track_capacity,
               psx_track_member* members, int member_capacity, psx_tracks_info* info)
{
    long long nodes = 0, records = 0;
    if (!psx_tracks_args_ok(host_pairs ? host_pairs : d_pairs_in, edge_counts, edges, n_edges, lens, n_sets, opts, track_starts, track_capacity,
                            members, member_capacity, info, &nodes, &records))
        return PSX_ERR_INVALID;
    if (!aligned(d_pairs_in, 16)) return PSX_ERR_INVALID;
    if (!host_out && (!aligned(labels, 4) || !aligned(track_starts, 4) || !aligned(members, 8))) return PSX_ERR_INVALID;
    if (psx_tracks_trivial(nodes, records)) {
        if (host_out) psx_tracks_none(nodes, labels, track_starts, info);
        else *info = psx_tracks_info{0, 0, 0, 0, 0, 0};
        return PSX_OK;
    }
    const int M = (int)nodes, n = (int)records, E = n_edges;
    const long long nb = psx_tracks_record_blocks(edge_counts, E);
    const long long nwg = psx_tracks_node_wgs(nodes);
    if (nb > PSX_GRAPH_INT_MAX) return PSX_ERR_NOMEM;
    const int bits = psx_tracks_sort_bits(nodes);
    if (hipSetDevice(device) != hipSuccess) return PSX_ERR_HIP;
    MatchScratch& sc = psx_match_scratch();
    if (!sc.bind(device)) return PSX_ERR_HIP;
    hipStream_t st = sc.stream;

    // the sort's temporary storage: a size query, nothing runs
    unsigned* nul = nullptr;
    size_t temp_b = 0;
    if (rocprim::radix_sort_pairs(nullptr, temp_b, nul, nul, nul, nul, (size_t)M, 0, (unsigned)bits, st) != hipSuccess) return PSX_ERR_HIP;
    // what the host form's outputs take on the device: as much as can be written
    const int h_tcap = track_capacity < M / 2 ? track_capacity : M / 2, h_mcap = member_capacity < M ? member_capacity : M;
    const size_t out_lab = 0, out_st = out_lab + (host_out && labels ? (size_t)psx_tracks_pad16(4LL * M) : 0),
                 out_mem = out_st + (host_out && track_starts ? (size_t)psx_tracks_pad16(4LL * (h_tcap + 1)) : 0),
                 out_b = out_mem + (host_out && members ? 8 * (size_t)h_mcap : 0);
    const size_t edges_b = 16 * (size_t)E, blocks_b = 16 * (size_t)nb, tables_b = (size_t)psx_tracks_tables_bytes(E, nb, n_sets);
    const size_t pin_head = 0, pin_tables = PSX_TRACKS_STATE_BYTES, pin_out = pin_tables + tables_b;
    const size_t sort_b = ((size_t)psx_tracks_sort_bytes(nodes) + 255) & ~(size_t)255;       // the sort's storage starts 256-byte aligned
    // every buffer before the first launch: nothing is reallocated under queued work
    if ((host_pairs && !sc.need(MS_TRACKS_PAIRS, 16 * (size_t)n)) || !sc.need(MS_TRACKS_TABLES, tables_b) ||
        !sc.need(MS_TRACKS_NODES, (size_t)psx_tracks_nodes_bytes(nodes)) || !sc.need(MS_TRACKS_SORT, sort_b + temp_b) ||
        !sc.need(MS_TRACKS_TOT, (size_t)psx_tracks_tot_bytes(nodes)) || !sc.need(MS_TRACKS_STATE, PSX_TRACKS_STATE_BYTES) ||
        (out_b > 0 && !sc.need(MS_TRACKS_OUT, out_b)) || !sc.need_pinned(pin_out + out_b))
        return PSX_ERR_NOMEM;
    char* hpin = static_cast<char*>(sc.hpin);

    // ---- the tables, written into the pinned staging buffer and copied on the stream in ONE copy ----
    {
        psx_tracks_edge* he = reinterpret_cast<psx_tracks_edge*>(hpin + pin_tables);
        int4* hb = reinterpret_cast<int4*>(hpin + pin_tables + edges_b);
        int* hoff = reinterpret_cast<int*>(hpin + pin_tables + edges_b + blocks_b);
        psx_tracks_offsets(lens, n_sets, hoff);
        for (int e = 0; e < E; e++) {
            const int l = edges[e].left, r = edges[e].right;
            he[e] = psx_tracks_edge{hoff[l], hoff[r], lens[l], lens[r]};
        }
        long long b = 0, first = 0;                            // the blocks of psx_ransac_many_blocks at a minimum of 1
        for (int e = 0; e < E; first += edge_counts[e], e++)
            for (long long p = first; p < first + edge_counts[e]; p += PSX_TRACKS_ROWS, b++) {
                const long long end = p + PSX_TRACKS_ROWS < first + edge_counts[e] ? p + PSX_TRACKS_ROWS : first + edge_counts[e];
                hb[b] = make_int4(e, (int)p, (int)end, 0);
            }
        if (b != nb) return PSX_ERR_HIP;
    }
    const void* d_pairs = d_pairs_in;
    if (host_pairs) {
        if (hipMemcpyAsync(sc.buf[MS_TRACKS_PAIRS], host_pairs, 16 * (size_t)n, hipMemcpyHostToDevice, st) != hipSuccess) return PSX_ERR_HIP;
        d_pairs = sc.buf[MS_TRACKS_PAIRS];
    }
    char* d_tab = static_cast<char*>(sc.buf[MS_TRACKS_TABLES]);
    const psx_tracks_edge* d_edges = reinterpret_cast<const psx_tracks_edge*>(d_tab);
    const int4* d_blocks = reinterpret_cast<const int4*>(d_tab + edges_b);
    const int* d_off = reinterpret_cast<const int*>(d_tab + edges_b + blocks_b);
    int* nodes_i = static_cast<int*>(sc.buf[MS_TRACKS_NODES]);
    const TNodes nd = {nodes_i, nodes_i + (size_t)M, nodes_i + 2 * (size_t)M, nodes_i + 3 * (size_t)M, nodes_i + 4 * (size_t)M, nodes_i + 5 * (size_t)M};
    unsigned* keys_in = static_cast<unsigned*>(sc.buf[MS_TRACKS_SORT]);
    unsigned *keys_out = keys_in + (size_t)M, *vals_in = keys_in + 2 * (size_t)M, *vals_out = keys_in + 3 * (size_t)M;
    void* d_temp = static_cast<char*>(sc.buf[MS_TRACKS_SORT]) + sort_b;
    int* d_tot = static_cast<int*>(sc.buf[MS_TRACKS_TOT]);
    int* d_offs = d_tot + 2 * (size_t)nwg;
    THead* d_head = static_cast<THead*>(sc.buf[MS_TRACKS_STATE]);
    char* d_out = static_cast<char*>(sc.buf[MS_TRACKS_OUT]);
    int* d_labels = host_out ? (labels ? reinterpret_cast<int*>(d_out + out_lab) : nullptr) : labels;
    int* d_starts = host_out ? (track_starts ? reinterpret_cast<int*>(d_out + out_st) : nullptr) : track_starts;
    psx_track_member* d_members = host_out ? (members ? reinterpret_cast<psx_track_member*>(d_out + out_mem) : nullptr) : members;
    const int tcap = host_out ? h_tcap : track_capacity, mcap = host_out ? h_mcap : member_capacity;
    const dim3 node_grid((unsigned)nwg), wg(256);

    if (hipMemcpyAsync(d_tab, hpin + pin_tables, tables_b, hipMemcpyHostToDevice, st) != hipSuccess) return PSX_ERR_HIP;
    hipLaunchKernelGGL(k_tracks_init, node_grid, wg, 0, st, nd, d_off, n_sets, M, d_head);
    hipLaunchKernelGGL(k_tracks_hook, dim3((unsigned)nb), wg, 0, st, static_cast<const int4*>(d_pairs), d_edges, d_blocks, nd.parent, d_head);
    hipLaunchKernelGGL(k_tracks_flatten, node_grid, wg, 0, st, nd.parent, M, keys_in, vals_in);
    if (rocprim::radix_sort_pairs(d_temp, temp_b, keys_in, keys_out, vals_in, vals_out, (size_t)M, 0, (unsigned)bits, st) != hipSuccess) return PSX_ERR_HIP;
    hipLaunchKernelGGL(k_tracks_segments, node_grid, wg, 0, st, keys_out, vals_out, M, nd);
    hipLaunchKernelGGL(k_tracks_count, node_grid, wg, 0, st, keys_out, vals_out, M, nd, opts->min_views, opts->flags, d_tot, d_head);
    hipLaunchKernelGGL(k_tracks_scan, dim3(2), dim3(1024), 0, st, d_tot, (int)nwg, d_offs);
    hipLaunchKernelGGL(k_tracks_write, node_grid, wg, 0, st, keys_out, vals_out, M, nd, d_off, opts->min_views, opts->flags, d_offs, d_labels, d_starts,
                       tcap, d_members, mcap, d_head);
    if (hipGetLastError() != hipSuccess) return PSX_ERR_HIP;
    if (out_b > 0 && hipMemcpyAsync(hpin + pin_out, d_out, out_b, hipMemcpyDeviceToHost, st) != hipSuccess) return PSX_ERR_HIP;
    if (hipMemcpyAsync(hpin + pin_head, d_head, sizeof(THead), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
        return PSX_ERR_HIP;
    const THead* hh = reinterpret_cast<const THead*>(hpin + pin_head);
    if (hh->bad != 0) return PSX_ERR_INVALID;
    if (hh->tracks < 0 || hh->tracks > M / 2 || hh->members < 2 * hh->tracks || hh->members > M || hh->components < hh->tracks ||
        hh->joined_records < 0 || hh->joined_records > n)
        return PSX_ERR_HIP;
    if (host_out) {
        if (labels) memcpy(labels, hpin + pin_out + out_lab, 4 * (size_t)M);
        if (track_starts) memcpy(track_starts, hpin + pin_out + out_st, 4 * ((size_t)(hh->tracks < h_tcap ? hh->tracks : h_tcap) + 1));
        if (members && h_mcap > 0) memcpy(members, hpin + pin_out + out_mem, 8 * (size_t)(hh->members < h_mcap ? hh->members : h_mcap));
    }
    *info = psx_tracks_info{hh->tracks, hh->members, hh->components, hh->conflicts, hh->too_few_views, hh->joined_records};
    return PSX_OK;
}

} // namespace

extern "C" int psx_tracks_graph(int device, const void* host_pairs, const int* edge_counts, const psx_view_edge* edges, int n_edges,
                                const int* lens, int n_sets, const psx_track_opts* opts, int* host_labels, int* host_track_starts,
                                int track_capacity, psx_track_member* host_members, int member_capacity, psx_tracks_info* info)
{
    return tracks_run(device, host_pairs, nullptr, edge_counts, edges, n_edges, lens, n_sets, opts, true, host_labels, host_track_starts,
                      track_capacity, host_members, member_capacity, info);
}

extern "C" int psx_tracks_graph_dev(int device, const void* d_pairs, const int* edge_counts, const psx_view_edge* edges, int n_edges,
                                    const int* lens, int n_sets, const psx_track_opts* opts, int* d_labels, int* d_track_starts,
                                    int track_capacity, psx_track_member* d_members, int member_capacity, psx_tracks_info* info)
{
    return tracks_run(device, nullptr, d_pairs, edge_counts, edges, n_edges, lens, n_sets, opts, false, d_labels, d_track_starts, track_capacity,
                      d_members, member_capacity, info);
}

extern "C" int psx_tracks_graph_ref(const void* pairs, const int* edge_counts, const psx_view_edge* edges, int n_edges, const int* lens,
                                    int n_sets, const psx_track_opts* opts, int* labels, int* track_starts, int track_capacity,
                                    psx_track_member* members, int member_capacity, psx_tracks_info* info)
{
    return psx_tracks_host(pairs, edge_counts, edges, n_edges, lens, n_sets, opts, labels, track_starts, track_capacity, members, member_capacity,
                           info);
}

extern "C" int psx_tracks_plan(const int* lens, int n_sets, const int* edge_counts, int n_edges, psx_tracks_plan_info* out)
{
    return psx_tracks_plan_host(lens, n_sets, edge_counts, n_edges, out);
}
