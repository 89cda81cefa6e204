// match_scratch.h -- what the matcher's translation units share (match.hip, match_guided.hip, match_many.hip,
// match_many_f32.hip, match_guided_many.hip, match_graph.hip, match_graph_f32.hip, match_guided_graph.hip, ransac.hip, ransac_many.hip,
// ransac_graph.hip, tracks.hip, bow.hip, bow_query.hip):
// the layout of a directed result, the per-thread scratch with its named buffers, the runner of the pair join, and the
// two batched drivers that a star form shares with its edge-list form.
// Internal to the HIP library.
#pragma once

#include "psx_internal.h"

// A DIRECTED RESULT of `len` rows, as every directed matcher leaves it on the device and the joins read it: 3 len ints
// (best, second, accept per row), then 2 len distances (float, or int for the byte matchers) -- 5 len words in all.
// The row offsets are formed in the caller's Row type.  k_match_merge and k_match_u8_merge pass int, as they always did:
// with size_t the row's 64-bit offset stays live across k_match_u8_merge's chunk loop, and psx_match_pairs_u8 at
// 2048 x 2048 measured 2.7 % slower on one MI355X.
template <class Dist, class Row>
__device__ __forceinline__ void psx_directed_store(int* __restrict__ res, size_t len, Row row, int best, int second, bool accept,
                                                   Dist d1, Dist d2)
{
    res[3 * row + 0] = best; res[3 * row + 1] = second; res[3 * row + 2] = accept ? 1 : 0;
    Dist* dist = reinterpret_cast<Dist*>(res + 3 * len);
    dist[2 * row + 0] = d1; dist[2 * row + 1] = d2;
}

// what a join reads of a row: the best index and the two distances; for the cross-check the best index alone
template <class Dist>
__device__ __forceinline__ void psx_directed_load(const int* __restrict__ res, size_t len, size_t row, int& best, Dist& d1, Dist& d2)
{
    const Dist* dist = reinterpret_cast<const Dist*>(res + 3 * len);
    best = res[3 * row];
    d1 = dist[2 * row]; d2 = dist[2 * row + 1];
}
__device__ __forceinline__ int psx_directed_best(const int* __restrict__ res, size_t row) { return res[3 * row]; }

// The buffers of a MatchScratch.  A buffer belongs to ONE use: calls queue work without waiting for the stream, so two
// features sharing a buffer would alias under queued work.  F32: psx_match / psx_match_pairs, U8: psx_match_u8 /
// psx_match_pairs_u8 (match.hip); GUIDED: match_guided.hip; MANY: the one-to-many search (match_many.hip), MANYF: its float form
// (match_many_f32.hip); GRAPH: the pair search over an edge list (match_graph.hip); GGRAPH: the batched guided re-match
// (match_guided_graph.hip), which the star form (match_guided_many.hip) runs too.  RANSAC: ransac.hip AND the one batched
// driver (ransac_graph.hip, for an edge list and for the star of ransac_many.hip), which adds RGRAPH for its tables:
// every call of any of them ends synchronised, so no two ever have work queued on a thread's scratch at once.
enum MatchSlot {
    MS_F32_PARTIAL,      // the exact scan's per-chunk top-2
    MS_F32_RPERM,        // the exact scan's permuted right side
    MS_F32_FWD,          // the directed result (and the prefilter's flag behind it)
    MS_F32_BWD,          // the backward direction's, psx_match_pairs with the cross-check
    MS_F32_LF16,         // the prefilter: the left side as f16 ...
    MS_F32_RF16,         // ... the right side
    MS_F32_LNORM,        // the left norms, then the seeding pass' minima
    MS_F32_RNORM,        // the maximum slots and the parameters, then the right norms
    MS_F32_CAND_CT,      // the candidate counts per (left, segment)
    MS_F32_CAND,         // the candidates
    MS_U8_PARTIAL,       // the per-chunk key pairs (both directions, one after the other)
    MS_U8_NORMS,         // the norms of both sets
    MS_U8_FWD,           // the directed result
    MS_U8_BWD,           // the backward direction's
    MS_PAIRS_TOT,        // the pair join's per-workgroup totals (float and bytes)
    MS_GUIDED_FWD,       // the forward direction's result
    MS_GUIDED_BWD,       // the backward direction's
    MS_GUIDED_LINES,     // the left side's lines for the backward direction
    MS_RANSAC_PAIRS,     // the uploaded pair records (of all sets)
    MS_RANSAC_PTS,       // the packed correspondences
    MS_RANSAC_MODELS,    // the hypotheses' models, every set's
    MS_RANSAC_COUNTS,    // their counts
    MS_RANSAC_STATE,     // the head, the per-set states and the per-set refit models (ransac_core.h)
    MS_RANSAC_TOT,       // the compaction's per-workgroup totals (the batched call: and their offsets)
    MS_MANY_TABLES,      // the set / chunk / block tables
    MS_MANY_NORMS,       // the norms of all sets
    MS_MANY_PARTIAL,     // the per-chunk key pairs
    MS_MANY_FWD,         // the forward direction's results of all sets
    MS_MANY_BWD,         // the backward direction's
    MS_MANY_TOT,         // the join's per-workgroup totals and their offsets
    MS_MANYF_TABLES,     // the float one-to-many search (match_many_f32.hip) and the float edge list (match_graph_f32.hip), which never run
                         // at once on a thread and share these: the set / (edge / item) / chunk / block tables
    MS_MANYF_STATE,      // the blocks' largest norms, the prefilter's parameters and its flag
    MS_MANYF_PERM,       // the scan: the permuted copy of every inner row
    MS_MANYF_PARTIAL,    // the scan: the per-chunk top-2
    MS_MANYF_F16,        // the prefilter: the f16 copy of every row of all sets
    MS_MANYF_NORMS,      // the prefilter: their squared norms
    MS_MANYF_CAND_CT,    // the prefilter: the candidate counts per (outer row, chunk, half wave)
    MS_MANYF_CAND,       // the prefilter: the candidates
    MS_MANYF_FWD,        // the forward direction's results of all sets
    MS_MANYF_BWD,        // the backward direction's
    MS_MANYF_TOT,        // the join's per-workgroup totals and their offsets
    MS_GRAPH_TABLES,     // the pair search over an edge list (match_graph.hip): the set / edge / chunk / item / block / {edge, row0} tables
    MS_GRAPH_NORMS,      // the norms of the referenced sets
    MS_GRAPH_PARTIAL,    // the per-chunk key pairs of one group of edges
    MS_GRAPH_FWD,        // the forward direction's results of all edges
    MS_GRAPH_BWD,        // the backward direction's
    MS_GRAPH_TOT,        // the join's per-workgroup totals and their offsets
    MS_RGRAPH_TABLES,    // the batched RANSAC (ransac_graph.hip; an edge list or a star): the list table and its two block tables; the rest is RANSAC's
    MS_GGRAPH_TABLES,    // the batched guided re-match (match_guided_graph.hip; an edge list or a star): the edge table and the two {edge, row0} tables
    MS_GGRAPH_LINES,     // the left rows' lines under their edge's guide, for the backward direction
    MS_GGRAPH_FWD,       // the forward direction's results of all edges
    MS_GGRAPH_BWD,       // the backward direction's
    MS_GGRAPH_TOT,       // the join's per-workgroup totals and their offsets
    MS_TRACKS_TABLES,    // tracks over an edge list (tracks.hip): the edge table, the record blocks and the views' node offsets
    MS_TRACKS_PAIRS,     // the uploaded records (the host form)
    MS_TRACKS_NODES,     // per node: parent, view; per root: begin, end, view changes, conflict mark
    MS_TRACKS_SORT,      // (root, node) keys and values, in and out, and the sort's temporary storage
    MS_TRACKS_TOT,       // the compaction's per-workgroup totals (heads, nodes) and their offsets
    MS_TRACKS_STATE,     // the six totals and the bad-record flag
    MS_TRACKS_OUT,       // the host form's labels, track starts and members before they are copied back
    MS_BOW_TABLES,       // the view shortlist (bow.hip): the views' pointers and row offsets
    MS_BOW_ROWS,         // the rows of all views gathered into one array
    MS_BOW_NORMS,        // the rows' norms, then the words'
    MS_BOW_ASSIGN,       // per row: its word now and its word one iteration ago
    MS_BOW_SUMS,         // per word: its row count and the 128 byte sums; behind them the 16 bytes that decide the stop
    MS_BOW_VOCAB,        // the host form's vocabulary on the device
    MS_BOW_OUT,          // the host form's histogram and row words before they are copied back
    MS_SL_HIST,          // the host form's uploaded histogram
    MS_SL_Q,             // df and the weights (W ints each), then the quantised histogram (N x W uint16)
    MS_SL_SCORE,         // the N x N scores
    MS_SL_LISTED,        // N x N bytes: is j in the list of i
    MS_SL_TOT,           // the edge compaction's per-workgroup totals and their offsets
    MS_SL_OUT,           // the host form's lists and edges before they are copied back
    MS_SLQ_DF,           // the database query (bow_query.hip): psx_bow_quantize_dev's df counters
    MS_SLQ_TABLES,       // the weights (W ints), then the queries' limits
    MS_SLQ_PARTIAL,      // the block lists: n_queries x blocks x min(k, 64) keys
    MS_SLQ_TOT,          // the edge compaction's per-workgroup totals, their offsets and the total
    MS_SLQ_OUT,          // the host form's lists and edges before they are copied back; the neighbours of a _dev call without that array
    MS_NBUF
};

// Scratch of one calling thread: a private non-blocking stream (no null-stream launch, so nothing else on
// the device is synchronised) and buffers that only ever grow.  Freed when the thread exits.
struct MatchScratch {
    static constexpr int NBUF = MS_NBUF;
    int device = -1;
    hipStream_t stream = nullptr;
    void* buf[NBUF] = {};
    size_t cap[NBUF] = {};
    void* hpin = nullptr;                // pinned staging of the results: a DMA into pageable caller memory goes through the
    size_t hpin_cap = 0;                 // runtime's own bounce buffers, ~0.5 ms per call on this stack
    bool tidy = false;                   // the prefilter's counters are zero (left so by the previous call's last kernel)
    PsxTuning tune;                      // the POPSIFT_MATCH_* switches and the CU count of `device`: taken in bind()
    int mfma_per_cu = 0;                 // workgroups of the prefilter kernel resident per CU on `device` (0: not asked yet)
    void release()
    {
        if (device < 0) return;
        int cur = -1;                                        // the caller's current device is left as it was
        if (hipGetDevice(&cur) != hipSuccess) cur = -1;
        (void)hipSetDevice(device);
        for (int i = 0; i < NBUF; i++) { (void)hipFree(buf[i]); buf[i] = nullptr; cap[i] = 0; }
        tidy = false;
        if (hpin) (void)hipHostFree(hpin);
        hpin = nullptr; hpin_cap = 0;
        if (stream) (void)hipStreamDestroy(stream);
        stream = nullptr; device = -1;
        if (cur >= 0) (void)hipSetDevice(cur);
    }
    // the scratch of `device` (a call for another device releases the previous one's first)
    bool bind(int dev)
    {
        if (device == dev) return true;
        release();
        if (hipStreamCreateWithFlags(&stream, hipStreamNonBlocking) != hipSuccess) return false;
        device = dev;
        tune = psx_tuning_from_env();
        if (hipDeviceGetAttribute(&tune.cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || tune.cus <= 0) tune.cus = 256;
        mfma_per_cu = 0;
        return true;
    }
    bool need_pinned(size_t bytes)
    {
        if (bytes <= hpin_cap && hpin) return true;
        if (hpin) (void)hipHostFree(hpin);
        hpin = nullptr; hpin_cap = 0;
        if (hipHostMalloc(&hpin, bytes, hipHostMallocDefault) != hipSuccess) return false;
        hpin_cap = bytes;
        return true;
    }
    bool need(MatchSlot i, size_t bytes)
    {
        if (bytes <= cap[i] && buf[i]) return true;
        (void)hipFree(buf[i]); buf[i] = nullptr; cap[i] = 0;
        tidy = false;
        if (hipMalloc(&buf[i], bytes) != hipSuccess) return false;
        cap[i] = bytes;
        return true;
    }
    // Thread exit.  For the main thread that is process teardown, where the HIP runtime may already be gone: ask it
    // first (a finalised runtime answers with an error) and then leave the buffers to the process exit.
    ~MatchScratch() { int n = 0; if (device >= 0 && hipGetDeviceCount(&n) == hipSuccess && n > 0) release(); }
};

// the calling thread's scratch (one object per thread, whichever translation unit asks: psx_match_release frees it)
MatchScratch& psx_match_scratch();

// Queues the join (k_pairs_count / k_pairs_write, match.hip) behind the directed passes already queued on sc.stream and
// finishes the call.  d_fwd / d_bwd: a directed pass' device results (float / int distances); d_bwd is read only with
// PSX_PAIRS_MUTUAL.  host_pairs or d_pairs (the other is NULL; both NULL with capacity 0).  One synchronisation.
// Dist = float or int: defined and instantiated for both in match.hip.
template <class Dist>
int psx_pairs_finish(MatchScratch& sc, const int* d_fwd, int l_len, const int* d_bwd, const psx_match_opts* opts,
                     void* host_pairs, void* d_pairs, int capacity, int* count);

// The batched drivers behind their argument checks, each stated once for an edge list and for a star; the star adapters
// (ransac_many.hip, match_guided_many.hip) reach them through these.  Not part of the library's C API.
//
// ransac_graph.hip: n_lists pair lists with two sides each (psx_ransac_sides, ransac_many_plan.h), concatenated;
// total_pairs = the sum of list_counts; model = PSX_RANSAC_MODEL_*.  host_pairs or d_pairs, host_inl or d_inl (the other
// is NULL; both NULL with capacity 0).
struct psx_ransac_sides;
int psx_ransac_lists_run(int model, int device, const void* host_pairs, const void* d_pairs, const int* list_counts, const psx_ransac_sides* sides,
                         int n_lists, long long total_pairs, const psx_ransac_opts* opts, psx_ransac_result* results, void* host_inl, void* d_inl,
                         int capacity, int* count, float* host_models, int* host_counts);
// match_guided_graph.hip: the edges over the set arrays, each under its own guide.  What psx_graph_args_ok asks of lens
// and edges holds; a set that no live edge names (match_guided_graph_plan.h) may have NULL arrays.  host_pairs or d_pairs.
// T: unsigned char (psx_match_pair_u8 records) or float (psx_match_pair records); defined and instantiated for both there.
template <class T>
int psx_guided_edges_run(int device, const T* const* d_sets, const float* const* d_xys, const int* lens, const psx_view_edge* edges,
                         int n_edges, const psx_guide* guides, const psx_match_opts* opts, void* host_pairs, void* d_pairs, int capacity,
                         int* edge_counts, int* count);
