// match_guided_many.hip -- the guided re-match of one descriptor set against many in one call:
// psx_match_pairs_guided_many_u8 (+ _dev), its float form psx_match_pairs_guided_many (+ _dev), psx_guides_from_ransac
// (include/popsift_hip.h).
//
// One left set against K right sets, each under its own guide, is a STAR: an edge list whose edges share their left set.
// This unit is the star's ADAPTER and holds no device code.  It makes the star's own argument checks, answers the calls
// that have nothing to search, states the star as sets [left, rights...], lengths [l_len, r_lens...] and edges {0, k + 1}
// -- edge k is set k, so the driver's per-edge counts are the star's set_counts -- and hands it to the one batched driver
// (psx_guided_edges_run, match_guided_graph.hip), whose edge table, kernels and join serve the edge-list forms too.  A
// set whose guide has kind PSX_GUIDE_NONE, or that is empty, is an edge that is not live there: none of its arrays is read.
// The launch and synchronisation counts are that driver's.
#include "psx_internal.h"
#include "guide_rule.h"
#include "match_join.h"
#include "match_many_plan.h"
#include "match_scratch.h"

#include <climits>
#include <cstring>
#include <vector>

namespace {

bool guide_none(const psx_guide& g) { return g.kind == PSX_GUIDE_NONE; }

// host_pairs or d_pairs (the other is NULL; both NULL with capacity 0).  T: unsigned char or float, the descriptor element
template <class T>
int match_pairs_guided_many(int device, const T* d_left, const float* d_left_xy, int l_len,
                            const T* const* d_rights, const float* const* d_right_xys, const int* r_lens, int n_sets,
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
    long long r_total = 0;                                           // the rows the call works with: none of a skipped set
    for (int k = 0; k < K; k++) {
        const int elen = guide_none(guides[k]) ? 0 : r_lens[k];
        if (elen > 0 && (!d_rights[k] || !d_right_xys[k])) return PSX_ERR_INVALID;
        r_total += elen;
    }
    if (l_len == 0 || r_total == 0) {
        for (int k = 0; k < K; k++) set_counts[k] = 0;
        *count = 0;
        return PSX_OK;
    }
    // one total per 256 left rows of every set, skipped or not, and one more had to fit an int: they still have to
    if ((long long)K * (((long long)l_len + 255) / 256) + 1 > INT_MAX) return PSX_ERR_NOMEM;
    thread_local std::vector<const T*> sets;
    thread_local std::vector<const float*> xys;
    thread_local std::vector<int> lens;
    thread_local std::vector<psx_view_edge> edges;
    sets.assign(1, d_left); xys.assign(1, d_left_xy); lens.assign(1, l_len);
    sets.insert(sets.end(), d_rights, d_rights + K);
    xys.insert(xys.end(), d_right_xys, d_right_xys + K);
    lens.insert(lens.end(), r_lens, r_lens + K);
    edges.resize((size_t)K);
    for (int k = 0; k < K; k++) edges[(size_t)k] = psx_view_edge{0, k + 1};
    return psx_guided_edges_run(device, sets.data(), xys.data(), lens.data(), edges.data(), K, guides, opts, host_pairs, d_pairs, capacity,
                                set_counts, count);
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

extern "C" int psx_match_pairs_guided_many(int device, const float* d_left, const float* d_left_xy, int l_len,
                                           const float* const* d_rights, const float* const* d_right_xys, const int* r_lens, int n_sets,
                                           const psx_guide* guides, const psx_match_opts* opts, psx_match_pair* host_pairs, int capacity,
                                           int* set_counts, int* count)
{
    return match_pairs_guided_many(device, d_left, d_left_xy, l_len, d_rights, d_right_xys, r_lens, n_sets, guides, opts, host_pairs, nullptr,
                                   capacity, set_counts, count);
}

extern "C" int psx_match_pairs_guided_many_dev(int device, const float* d_left, const float* d_left_xy, int l_len,
                                               const float* const* d_rights, const float* const* d_right_xys, const int* r_lens, int n_sets,
                                               const psx_guide* guides, const psx_match_opts* opts, psx_match_pair* d_pairs, int capacity,
                                               int* set_counts, int* count)
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
