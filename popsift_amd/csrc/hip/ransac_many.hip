// ransac_many.hip -- geometric verification of many pair lists in one call: psx_ransac_homography_many (+ _dev, _ref),
// psx_ransac_fundamental_many, psx_ransac_affine_many, psx_ransac_similarity_many (+ _dev, _ref each),
// psx_ransac_many_plan (include/popsift_hip.h).
//
// The K lists that psx_match_pairs_many_u8* left behind one another share ONE left view: a star, which is an edge list
// whose edges share their left side.  This unit is the star's ADAPTER and holds no device code: it checks the star's
// arguments (psx_ransac_many_args_ok, ransac_many_plan.h), states every list's two sides -- the shared left array and the
// set's own right array -- and hands them to the one batched driver (psx_ransac_lists_run, ransac_graph.hip), whose
// kernels, tables, refit stage and result loop serve the edge-list forms too.  Set k's result is the single call's, bit
// for bit, as that driver's header says for a list; the launch and synchronisation counts are stated there.
#include "match_scratch.h"
#include "ransac_many_plan.h"

#include <new>
#include <vector>

namespace {

// host_pairs or d_pairs; host_inl or d_inl (the other is NULL; both NULL with capacity 0)
int many_run(int model, int device, const void* host_pairs, const void* d_pairs, const int* set_counts, int n_sets, const float* d_lxy, int l_len,
             const float* const* d_rxys, const int* r_lens, const psx_ransac_opts* opts, psx_ransac_result* results, void* host_inl, void* d_inl,
             int capacity, int* count, float* host_models, int* host_counts)
{
    long long total_pairs = 0;
    if (!psx_ransac_many_args_ok(host_pairs ? host_pairs : d_pairs, set_counts, n_sets, d_lxy, l_len, d_rxys, r_lens, opts, results,
                                 host_inl ? host_inl : d_inl, capacity, count, &total_pairs))
        return PSX_ERR_INVALID;
    thread_local std::vector<psx_ransac_sides> sides;
    sides.resize((size_t)n_sets);
    for (int k = 0; k < n_sets; k++) sides[(size_t)k] = psx_ransac_many_side(d_lxy, l_len, d_rxys, r_lens, k);
    return psx_ransac_lists_run(model, device, host_pairs, d_pairs, set_counts, sides.data(), n_sets, total_pairs, opts, results, host_inl, d_inl,
                                capacity, count, host_models, host_counts);
}

int many_ref(int model, const void* pairs, const int* set_counts, int n_sets, const float* left_xy, int nl, const float* const* right_xys,
             const int* r_lens, const psx_ransac_opts* opts, psx_ransac_result* results, void* inliers, int capacity, int* count, float* models,
             int* counts)
{
    int longest = 0;
    if (n_sets > 0 && set_counts != nullptr)
        for (int k = 0; k < n_sets; k++) longest = set_counts[k] > longest ? set_counts[k] : longest;
    psx_ransac_pt* scratch = longest > 0 ? new (std::nothrow) psx_ransac_pt[(size_t)longest] : nullptr;
    if (longest > 0 && !scratch) return PSX_ERR_NOMEM;
    const int rc = psx_ransac_many_host(model, pairs, set_counts, n_sets, left_xy, nl, right_xys, r_lens, opts, results, inliers, capacity, count,
                                        models, counts, scratch);
    delete[] scratch;
    return rc;
}

} // namespace

extern "C" int psx_ransac_many_plan(const int* set_counts, int n_sets, int min_pairs, int block_rows, psx_ransac_block* blocks, int capacity,
                                    int* block_count)
{
    return psx_ransac_many_plan_host(set_counts, n_sets, min_pairs, block_rows, blocks, capacity, block_count);
}

// the three forms of one model: lists and inliers on the host, both in HBM, and the host reference
#define PSX_RANSAC_MANY_FORMS(name, KIND)                                                                                                       \
    extern "C" int psx_ransac_##name##_many(int device, const void* host_pairs, const int* set_counts, int n_sets, const float* d_left_xy,      \
                                            int l_len, const float* const* d_right_xys, const int* r_lens, const psx_ransac_opts* opts,         \
                                            psx_ransac_result* results, void* host_inliers, int capacity, int* count, float* host_models,       \
                                            int* host_counts)                                                                                   \
    {                                                                                                                                           \
        return many_run(KIND, device, host_pairs, nullptr, set_counts, n_sets, d_left_xy, l_len, d_right_xys, r_lens, opts, results,            \
                        host_inliers, nullptr, capacity, count, host_models, host_counts);                                                      \
    }                                                                                                                                           \
    extern "C" int psx_ransac_##name##_many_dev(int device, const void* d_pairs, const int* set_counts, int n_sets, const float* d_left_xy,     \
                                                int l_len, const float* const* d_right_xys, const int* r_lens, const psx_ransac_opts* opts,     \
                                                psx_ransac_result* results, void* d_inliers, int capacity, int* count, float* host_models,      \
                                                int* host_counts)                                                                               \
    {                                                                                                                                           \
        return many_run(KIND, device, nullptr, d_pairs, set_counts, n_sets, d_left_xy, l_len, d_right_xys, r_lens, opts, results, nullptr,      \
                        d_inliers, capacity, count, host_models, host_counts);                                                                  \
    }                                                                                                                                           \
    extern "C" int psx_ransac_##name##_many_ref(const void* pairs, const int* set_counts, int n_sets, const float* left_xy, int nl,             \
                                                const float* const* right_xys, const int* r_lens, const psx_ransac_opts* opts,                  \
                                                psx_ransac_result* results, void* inliers, int capacity, int* count, float* models,             \
                                                int* counts)                                                                                    \
    {                                                                                                                                           \
        return many_ref(KIND, pairs, set_counts, n_sets, left_xy, nl, right_xys, r_lens, opts, results, inliers, capacity, count, models,       \
                        counts);                                                                                                                \
    }

PSX_RANSAC_MANY_FORMS(homography, PSX_RANSAC_MODEL_HOMOGRAPHY)
PSX_RANSAC_MANY_FORMS(fundamental, PSX_RANSAC_MODEL_FUNDAMENTAL)
PSX_RANSAC_MANY_FORMS(affine, PSX_RANSAC_MODEL_AFFINE)
PSX_RANSAC_MANY_FORMS(similarity, PSX_RANSAC_MODEL_SIMILARITY)
