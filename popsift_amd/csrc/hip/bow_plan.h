// bow_plan.h -- the host side of the view shortlist (psx_vocab_train_u8*, psx_bow_u8*, psx_shortlist_views*, psx_bow_weights;
// include/popsift_hip.h) and, at the end, of the database query (psx_bow_quantize*, psx_shortlist_query*,
// psx_shortlist_query_plan): the argument checks every form shares, the empty forms, and the host references.
//
// Plain C++14, no HIP: bow.hip and bow_query.hip check their arguments with these functions, and a stand-alone program can
// include the header alone (tests/cpp/shortlist_san.cpp, tests/cpp/query_san.cpp).  The rule is bow_rule.h; the references below are sequential and are the definition
// of the results.
#pragma once

#include "bow_rule.h"

#include <cstring>
#include <new>
#include <vector>

// lens and the set pointers (host or device alike: only NULL is looked at); *rows = M
inline bool psx_bow_sets_ok(const unsigned char* const* sets, const int* lens, int n_sets, long long max_rows, long long* rows)
{
    if (n_sets < 0 || (n_sets > 0 && (sets == nullptr || lens == nullptr))) return false;
    long long m = 0;
    for (int v = 0; v < n_sets; v++) {
        if (lens[v] < 0 || (lens[v] > 0 && sets[v] == nullptr)) return false;
        m += lens[v];
        if (m > max_rows) return false;
    }
    *rows = m;
    return true;
}

inline bool psx_vocab_args_ok(const unsigned char* const* sets, const int* lens, int n_sets, const psx_vocab_opts* opts,
                              const unsigned char* vocab, const psx_vocab_info* info, long long* rows)
{
    if (!psx_vocab_opts_ok(opts) || vocab == nullptr || info == nullptr) return false;
    if (!psx_bow_sets_ok(sets, lens, n_sets, PSX_BOW_TRAIN_MAX_ROWS, rows)) return false;
    return opts->words <= *rows;
}

inline bool psx_bow_args_ok(const unsigned char* vocab, int words, const unsigned char* const* sets, const int* lens, int n_sets,
                            const unsigned* hist, long long* rows)
{
    if (words < 1 || words > PSX_BOW_MAX_WORDS || vocab == nullptr) return false;
    if (!psx_bow_sets_ok(sets, lens, n_sets, PSX_BOW_MAX_ROWS, rows)) return false;
    return n_sets == 0 || hist != nullptr;
}

inline bool psx_shortlist_args_ok(const unsigned* hist, int n_views, int words, const psx_shortlist_opts* opts, const psx_view_edge* edges,
                                  int edge_capacity, const int* edge_count)
{
    if (!psx_shortlist_opts_ok(opts) || n_views < 0 || n_views > PSX_SHORTLIST_MAX_VIEWS || words < 1 || words > PSX_BOW_MAX_WORDS) return false;
    if ((n_views > 0 && hist == nullptr) || edge_count == nullptr || edge_capacity < 0 || (edge_capacity > 0 && edges == nullptr)) return false;
    return (long long)n_views * opts->k <= 0x7fffffffLL;                // the list arrays are indexed with ints
}

// off[0 .. n_sets]: the exclusive prefix sum of lens and M behind it
inline void psx_bow_offsets(const int* lens, int n_sets, int* off)
{
    long long at = 0;
    for (int v = 0; v < n_sets; v++) { off[v] = (int)at; at += lens[v]; }
    off[n_sets] = (int)at;
}

// ASSIGN of one row against W words: the sequential scan, strict order (d, w)
inline int psx_bow_assign_row(const unsigned char* x, const unsigned char* vocab, int W, int* dist)
{
    int bw = 0, bd = psx_bow_dist(x, vocab);
    for (int w = 1; w < W; w++) {
        const int d = psx_bow_dist(x, vocab + (size_t)w * PSX_BOW_DIM);
        if (psx_bow_better(d, w, bd, bw)) { bd = d; bw = w; }
    }
    *dist = bd;
    return bw;
}

// psx_bow_weights
inline int psx_bow_weights_host(const int* df, int words, int n_views, int* out)
{
    if (words < 0 || n_views < 1 || (words > 0 && (df == nullptr || out == nullptr))) return PSX_ERR_INVALID;
    for (int w = 0; w < words; w++)
        if (df[w] < 0 || df[w] > n_views) return PSX_ERR_INVALID;
    for (int w = 0; w < words; w++) out[w] = psx_bow_weight(df[w], n_views);
    return PSX_OK;
}

// psx_vocab_train_u8_ref
inline int psx_vocab_train_host(const unsigned char* const* sets, const int* lens, int n_sets, const psx_vocab_opts* opts,
                                unsigned char* vocab, psx_vocab_info* info)
{
    long long rows = 0;
    if (!psx_vocab_args_ok(sets, lens, n_sets, opts, vocab, info, &rows)) return PSX_ERR_INVALID;
    const size_t M = (size_t)rows;
    const int W = opts->words;
    std::vector<const unsigned char*> row;
    std::vector<int> prev, cur;
    std::vector<unsigned> cnt, sum;
    try {
        row.reserve(M); prev.assign(M, -1); cur.resize(M); cnt.resize((size_t)W); sum.resize((size_t)W * PSX_BOW_DIM);
    } catch (const std::bad_alloc&) { return PSX_ERR_NOMEM; }
    for (int v = 0; v < n_sets; v++)
        for (int r = 0; r < lens[v]; r++) row.push_back(sets[v] + (size_t)r * PSX_BOW_DIM);
    for (int w = 0; w < W; w++) memcpy(vocab + (size_t)w * PSX_BOW_DIM, row[(size_t)psx_bow_init_row(w, rows, W)], PSX_BOW_DIM);
    psx_vocab_info t = {0, 0, 0, 0, 0ULL};
    for (int it = 1; it <= opts->iterations; it++) {
        t.iterations = it; t.changed = 0; t.empty_words = 0; t.inertia = 0;
        std::fill(cnt.begin(), cnt.end(), 0u);
        std::fill(sum.begin(), sum.end(), 0u);
        for (size_t g = 0; g < M; g++) {
            int d = 0;
            const int w = psx_bow_assign_row(row[g], vocab, W, &d);
            cur[g] = w;
            if (w != prev[g]) t.changed++;
            t.inertia += (unsigned long long)d;
            cnt[(size_t)w]++;
            for (int k = 0; k < PSX_BOW_DIM; k++) sum[(size_t)w * PSX_BOW_DIM + k] += row[g][k];
        }
        for (int w = 0; w < W; w++) {
            if (cnt[(size_t)w] == 0) { t.empty_words++; continue; }
            for (int k = 0; k < PSX_BOW_DIM; k++)
                vocab[(size_t)w * PSX_BOW_DIM + k] = psx_bow_mean(sum[(size_t)w * PSX_BOW_DIM + k], cnt[(size_t)w]);
        }
        prev.swap(cur);
        if (t.changed == 0) break;
    }
    *info = t;
    return PSX_OK;
}

// psx_bow_u8_ref
inline int psx_bow_host(const unsigned char* vocab, int words, const unsigned char* const* sets, const int* lens, int n_sets,
                        unsigned* hist, int* words_out)
{
    long long rows = 0;
    if (!psx_bow_args_ok(vocab, words, sets, lens, n_sets, hist, &rows)) return PSX_ERR_INVALID;
    if (n_sets > 0) memset(hist, 0, sizeof(unsigned) * (size_t)n_sets * (size_t)words);
    size_t g = 0;
    for (int v = 0; v < n_sets; v++)
        for (int r = 0; r < lens[v]; r++, g++) {
            int d = 0;
            const int w = psx_bow_assign_row(sets[v] + (size_t)r * PSX_BOW_DIM, vocab, words, &d);
            hist[(size_t)v * (size_t)words + (size_t)w]++;
            if (words_out != nullptr) words_out[g] = w;
        }
    return PSX_OK;
}

// the lists of a call without candidates (host arrays): every entry unused
inline void psx_shortlist_none(int n_views, int k, int* neighbours, unsigned* scores)
{
    const size_t n = (size_t)n_views * (size_t)k;
    if (neighbours != nullptr) for (size_t e = 0; e < n; e++) neighbours[e] = -1;
    if (scores != nullptr) for (size_t e = 0; e < n; e++) scores[e] = 0u;
}

// psx_shortlist_views_ref
inline int psx_shortlist_host(const unsigned* hist, int n_views, int words, const psx_shortlist_opts* opts, int* neighbours,
                              unsigned* scores, psx_view_edge* edges, int edge_capacity, int* edge_count)
{
    if (!psx_shortlist_args_ok(hist, n_views, words, opts, edges, edge_capacity, edge_count)) return PSX_ERR_INVALID;
    const int N = n_views, W = words, k = opts->k;
    psx_shortlist_none(N, k, neighbours, scores);
    if (N == 0) { *edge_count = 0; return PSX_OK; }
    std::vector<int> df, weight;
    std::vector<unsigned> p;                                             // weight[w] * q[v][w]
    std::vector<unsigned long long> keys;
    std::vector<unsigned char> listed;
    try {
        df.assign((size_t)W, 0); weight.resize((size_t)W); p.resize((size_t)N * W); keys.resize((size_t)N); listed.assign((size_t)N * N, 0);
    } catch (const std::bad_alloc&) { return PSX_ERR_NOMEM; }
    for (int v = 0; v < N; v++)
        for (int w = 0; w < W; w++)
            if (hist[(size_t)v * W + w] > 0) df[(size_t)w]++;
    if (psx_bow_weights_host(df.data(), W, N, weight.data()) != PSX_OK) return PSX_ERR_INVALID;
    for (int v = 0; v < N; v++) {
        unsigned long long n = 0;
        for (int w = 0; w < W; w++) n += hist[(size_t)v * W + w];
        for (int w = 0; w < W; w++) p[(size_t)v * W + w] = psx_bow_term((unsigned)weight[(size_t)w], psx_bow_quant(hist[(size_t)v * W + w], n), 65535u);
    }
    const int kk = k < N - 1 ? k : N - 1;
    for (int i = 0; i < N; i++) {
        for (int j = 0; j < N; j++) {
            unsigned s = 0;
            if (j != i)
                for (int w = 0; w < W; w++) { const unsigned a = p[(size_t)i * W + w], b = p[(size_t)j * W + w]; s += a < b ? a : b; }
            keys[(size_t)j] = s > 0 ? psx_shortlist_key(s, j) : 0ULL;
        }
        unsigned long long last = ~0ULL;
        for (int r = 0; r < kk; r++) {                                   // the largest key below the last one taken
            unsigned long long best = 0;
            for (int j = 0; j < N; j++)
                if (keys[(size_t)j] < last && keys[(size_t)j] > best) best = keys[(size_t)j];
            if (best == 0) break;
            const int j = psx_shortlist_key_view(best);
            if (neighbours != nullptr) neighbours[(size_t)i * k + r] = j;
            if (scores != nullptr) scores[(size_t)i * k + r] = psx_shortlist_key_score(best);
            listed[(size_t)i * N + j] = 1;
            last = best;
        }
    }
    int count = 0;
    for (int a = 0; a < N; a++)
        for (int b = a + 1; b < N; b++) {
            if (!psx_shortlist_edge_keep(listed[(size_t)a * N + b] != 0, listed[(size_t)b * N + a] != 0, opts->flags)) continue;
            if (count < edge_capacity) edges[count] = psx_view_edge{a, b};
            count++;
        }
    *edge_count = count;
    return PSX_OK;
}

// ---- query a database of views (psx_bow_quantize*, psx_shortlist_query*, psx_shortlist_query_plan) ---------------------

#include <cstdint>

inline bool psx_aligned_to(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
inline size_t psx_pad16(size_t b) { return (b + 15) & ~(size_t)15; }

// psx_bow_quantize*: device_arrays = the _dev form, whose pointers are looked at for alignment too
inline bool psx_bow_quantize_args_ok(const unsigned* hist, int n_views, int words, const unsigned short* q, bool device_arrays)
{
    if (n_views < 0 || n_views > PSX_QUERY_MAX_VIEWS || words < 1 || words > PSX_BOW_MAX_WORDS) return false;
    if (n_views > 0 && (hist == nullptr || q == nullptr)) return false;
    return !device_arrays || (psx_aligned_to(hist, 4) && psx_aligned_to(q, 2));
}

// the sizes alone: what psx_shortlist_query_plan refuses, and every query call with it
inline bool psx_query_sizes_ok(int n_db, int n_queries, int words, int k)
{
    if (n_db < 0 || n_queries < 0 || n_db > PSX_QUERY_MAX_VIEWS || n_queries > PSX_QUERY_MAX_QUERIES) return false;
    if (words < 1 || words > PSX_BOW_MAX_WORDS || k < 1) return false;
    return (long long)n_queries * k <= 0x7fffffffLL;                    // the list arrays are indexed with ints
}

// the edge compaction's workgroups: one lane per list slot
inline long long psx_query_slot_blocks(int n_queries, int k) { return ((long long)n_queries * k + 255) / 256; }

// the plan of sizes that psx_query_sizes_ok accepts; false where the block lists would pass PSX_QUERY_MAX_PARTIAL_KEYS
inline bool psx_query_plan_make(int n_db, int n_queries, int words, int k, psx_query_plan* plan)
{
    psx_query_plan p = {0, 0, 0, 0};
    if (n_db > 0 && n_queries > 0) {
        p.blocks = (n_db + PSX_QUERY_TILE - 1) / PSX_QUERY_TILE;
        p.keys_per_block = k < PSX_QUERY_TILE ? k : PSX_QUERY_TILE;
        p.partial_keys = (long long)n_queries * p.blocks * p.keys_per_block;
        if (p.partial_keys > PSX_QUERY_MAX_PARTIAL_KEYS) return false;
        // the weights and the limits, the block lists, the compaction's totals, offsets and total
        p.scratch_bytes = (long long)(psx_pad16(4 * (size_t)words) + psx_pad16(4 * (size_t)n_queries)) + 8 * p.partial_keys +
                          4 * (2 * psx_query_slot_blocks(n_queries, k) + 2);
    }
    *plan = p;
    return true;
}

// psx_shortlist_query_plan
inline int psx_query_plan_host(int n_db, int n_queries, int words, int k, psx_query_plan* plan)
{
    psx_query_plan p;
    if (plan == nullptr || !psx_query_sizes_ok(n_db, n_queries, words, k) || !psx_query_plan_make(n_db, n_queries, words, k, &p))
        return PSX_ERR_INVALID;
    *plan = p;
    return PSX_OK;
}

// every check of a query call; device_q: the q arrays are device memory (alignment is all that is looked at),
// device_out: so are neighbours, scores and edges
inline bool psx_query_args_ok(const unsigned short* db_q, int n_db, const unsigned short* query_q, int n_queries, int words, const int* weights,
                              const int* db_limit, const psx_query_opts* opts, const int* neighbours, const unsigned* scores,
                              const psx_view_edge* edges, int edge_capacity, const int* edge_count, bool device_q, bool device_out,
                              psx_query_plan* plan)
{
    if (!psx_query_opts_ok(opts) || !psx_query_sizes_ok(n_db, n_queries, words, opts->k)) return false;
    if (weights == nullptr || (n_db > 0 && db_q == nullptr) || (n_queries > 0 && query_q == nullptr)) return false;
    if (edge_count == nullptr || edge_capacity < 0 || (edge_capacity > 0 && edges == nullptr)) return false;
    if (opts->self_base >= 0 && (long long)opts->self_base + n_queries > n_db) return false;
    for (int w = 0; w < words; w++)
        if (weights[w] < 0 || weights[w] > PSX_QUERY_MAX_WEIGHT) return false;
    if (db_limit != nullptr)
        for (int i = 0; i < n_queries; i++)
            if (db_limit[i] < 0 || db_limit[i] > n_db) return false;
    if (device_q && (!psx_aligned_to(db_q, 2) || !psx_aligned_to(query_q, 2))) return false;
    if (device_out && (!psx_aligned_to(neighbours, 4) || !psx_aligned_to(scores, 4) || !psx_aligned_to(edges, 8))) return false;
    return psx_query_plan_make(n_db, n_queries, words, opts->k, plan);
}

// psx_bow_quantize_ref
inline int psx_bow_quantize_host(const unsigned* hist, int n_views, int words, unsigned short* q, int* df_accum)
{
    if (!psx_bow_quantize_args_ok(hist, n_views, words, q, false)) return PSX_ERR_INVALID;
    for (int v = 0; v < n_views; v++) {
        const unsigned* h = hist + (size_t)v * (size_t)words;
        unsigned long long n = 0;
        for (int w = 0; w < words; w++) n += h[w];
        for (int w = 0; w < words; w++) {
            q[(size_t)v * (size_t)words + (size_t)w] = (unsigned short)psx_bow_quant(h[w], n);
            if (df_accum != nullptr && h[w] > 0) df_accum[w]++;
        }
    }
    return PSX_OK;
}

// psx_shortlist_query_ref
inline int psx_shortlist_query_host(const unsigned short* db_q, int n_db, const unsigned short* query_q, int n_queries, int words,
                                    const int* weights, const int* db_limit, const psx_query_opts* opts, int* neighbours, unsigned* scores,
                                    psx_view_edge* edges, int edge_capacity, int* edge_count)
{
    psx_query_plan plan;
    if (!psx_query_args_ok(db_q, n_db, query_q, n_queries, words, weights, db_limit, opts, neighbours, scores, edges, edge_capacity, edge_count,
                           false, false, &plan))
        return PSX_ERR_INVALID;
    const int k = opts->k;
    const size_t W = (size_t)words;
    std::vector<unsigned long long> keys;
    try { keys.resize((size_t)n_db); } catch (const std::bad_alloc&) { return PSX_ERR_NOMEM; }
    psx_shortlist_none(n_queries, k, neighbours, scores);
    int count = 0;
    for (int i = 0; i < n_queries; i++) {
        const unsigned short* a = query_q + (size_t)i * W;
        const int limit = db_limit != nullptr ? db_limit[i] : n_db, self = opts->self_base >= 0 ? opts->self_base + i : -1;
        for (int j = 0; j < n_db; j++) {
            const unsigned short* b = db_q + (size_t)j * W;
            unsigned s = 0;
            if (j < limit && j != self)
                for (size_t w = 0; w < W; w++) s += psx_bow_term((unsigned)weights[w], a[w], b[w]);
            keys[(size_t)j] = psx_query_candidate(s, j, limit, self, opts->min_score) ? psx_query_key(s, j) : 0ULL;
        }
        unsigned long long last = ~0ULL;
        for (int r = 0; r < k; r++) {                                    // the largest key below the last one taken
            unsigned long long best = 0;
            for (int j = 0; j < n_db; j++)
                if (keys[(size_t)j] < last && keys[(size_t)j] > best) best = keys[(size_t)j];
            if (best == 0) break;
            const int j = psx_query_key_view(best);
            if (neighbours != nullptr) neighbours[(size_t)i * k + r] = j;
            if (scores != nullptr) scores[(size_t)i * k + r] = psx_query_key_score(best);
            if (count < edge_capacity) edges[count] = psx_view_edge{opts->edge_base + i, j};
            count++;
            last = best;
        }
    }
    *edge_count = count;
    return PSX_OK;
}
