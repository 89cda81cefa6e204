// bow_rule.h -- the rules of the view shortlist (psx_vocab_train_u8*, psx_bow_u8*, psx_shortlist_views*; include/popsift_hip.h)
// and of the database query (psx_bow_quantize*, psx_shortlist_query*; QUERY below).
//
// ONE set of inline functions, compiled for the host (the references, bow_plan.h) and for the device (bow.hip, bow_query.hip): the two
// cannot drift apart.  Integers only; the one logarithm of the step (psx_bow_weight) is host code and is never compiled
// for the device.  No HIP header is needed when g++ compiles this file.
//
// ROWS.    Views 0 .. N-1 with lens[v] rows of 128 bytes; row r of view v is global row g = off[v] + r, off = the exclusive
//          prefix sum of lens, M = their sum.  d(x, c) = sum_k (x_k - c_k)^2, an exact integer <= 128 * 255^2.
// INIT.    Word w starts as the bytes of global row floor(w * M / W), the product in 64 bits (psx_bow_init_row).
// ASSIGN.  a(g) = the word with the smallest (d(row g, word w), w): ties go to the lower word (psx_bow_better), the order
//          the byte matcher ranks by.
// UPDATE.  cnt[w] = rows with a(g) = w, sum[w][k] = the sum of their bytes (unsigned 32 bit, no overflow for M <= 2^24);
//          the new byte is (2 sum + cnt) / (2 cnt), which rounds half up; a word with cnt = 0 keeps its bytes
//          (psx_bow_mean).
// STOP.    After T iterations, or after the first iteration in which no row changed its word (in the first iteration
//          every row counts as changed).  The update of that iteration is still applied: it reproduces the same words.
// SCORE.   n_v = the sum of hist[v][.]; df[w] = the views with hist[v][w] > 0; weight[w] = psx_bow_weight(df, N);
//          q[v][w] = floor(hist[v][w] * 65535 / n_v) (0 for n_v = 0); score(i, j) = sum_w weight[w] * min(q[i][w], q[j][w])
//          = sum_w min(weight[w] q[i][w], weight[w] q[j][w]) since the weights are not negative.  The weights are at most
//          193 and sum_w q[v][w] <= 65535, so a score stays below 2^24.
// LIST.    The candidates of view i are the views j != i with score(i, j) > 0, in the order (score descending, j
//          ascending) -- the descending order of psx_shortlist_key -- the first k are kept.
// EDGES.   {(min(i, j), max(i, j)) : j in the list of i}, once each, ascending by (left, right); with
//          PSX_SHORTLIST_MUTUAL only where each view lists the other (psx_shortlist_edge_keep).
#pragma once

#include "popsift_hip.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PSX_BOW_HD __host__ __device__
#else
#define PSX_BOW_HD
#endif

constexpr int PSX_BOW_DIM = 128;                       // bytes of a descriptor
constexpr int PSX_BOW_MAX_WORDS = 65536;
constexpr long long PSX_BOW_TRAIN_MAX_ROWS = 1LL << 24; // the byte sums of a word stay below 2^32
constexpr long long PSX_BOW_MAX_ROWS = 0x3fffffffLL;    // rows of one psx_bow_u8 call
constexpr int PSX_SHORTLIST_MAX_VIEWS = 4096;          // 12 index bits in psx_shortlist_key, scores below 2^24

PSX_BOW_HD inline bool psx_vocab_opts_ok(const psx_vocab_opts* o)
{
    return o != nullptr && o->words >= 2 && o->words <= PSX_BOW_MAX_WORDS && o->iterations >= 1;
}

PSX_BOW_HD inline bool psx_shortlist_opts_ok(const psx_shortlist_opts* o)
{
    return o != nullptr && o->k >= 1 && (o->flags & ~PSX_SHORTLIST_MUTUAL) == 0;
}

// the global row whose bytes word w starts with
PSX_BOW_HD inline long long psx_bow_init_row(int w, long long M, int W) { return (long long)w * M / W; }

PSX_BOW_HD inline int psx_bow_dist(const unsigned char* x, const unsigned char* c)
{
    int d = 0;
    for (int k = 0; k < PSX_BOW_DIM; k++) { const int e = (int)x[k] - (int)c[k]; d += e * e; }
    return d;
}

// does (d, w) come before (bd, bw)?
PSX_BOW_HD inline bool psx_bow_better(int d, int w, int bd, int bw) { return d < bd || (d == bd && w < bw); }

// a word's new byte from the sum of its rows' bytes; cnt > 0
PSX_BOW_HD inline unsigned char psx_bow_mean(unsigned sum, unsigned cnt)
{
    return (unsigned char)((2ULL * sum + cnt) / (2ULL * cnt));
}

PSX_BOW_HD inline unsigned psx_bow_quant(unsigned h, unsigned long long n)
{
    return n == 0 ? 0u : (unsigned)((unsigned long long)h * 65535ULL / n);
}

// one word's part of a score
PSX_BOW_HD inline unsigned psx_bow_term(unsigned weight, unsigned qi, unsigned qj) { return weight * (qi < qj ? qi : qj); }

// larger key = earlier in a view's list; 0 is no candidate (a candidate's score is positive)
PSX_BOW_HD inline unsigned long long psx_shortlist_key(unsigned score, int j)
{
    return ((unsigned long long)score << 12) | (unsigned long long)(PSX_SHORTLIST_MAX_VIEWS - 1 - j);
}
PSX_BOW_HD inline unsigned psx_shortlist_key_score(unsigned long long key) { return (unsigned)(key >> 12); }
PSX_BOW_HD inline int psx_shortlist_key_view(unsigned long long key) { return PSX_SHORTLIST_MAX_VIEWS - 1 - (int)(key & 4095ULL); }

// the pair (a, b), a < b: a_lists_b / b_lists_a = is the one in the other's list
PSX_BOW_HD inline bool psx_shortlist_edge_keep(bool a_lists_b, bool b_lists_a, int flags)
{
    return (flags & PSX_SHORTLIST_MUTUAL) != 0 ? (a_lists_b && b_lists_a) : (a_lists_b || b_lists_a);
}

// QUERY (psx_shortlist_query*): n_queries new views against n_db stored ones, both as rows of q (psx_bow_quantize*), under
// weights the caller brings.  Nothing of the symmetric form is needed: no N x N matrix, 20 index bits instead of 12.
// CANDIDATES of query i: the database views j with j < limit_i (db_limit[i], or n_db), j != self_base + i (when
//          self_base >= 0), score(i, j) = sum_w weight[w] min(qq[i][w], dbq[j][w]) > 0 and score(i, j) >= min_score.
// LIST     of query i: the candidates by (score descending, j ascending) -- the descending order of psx_query_key -- the
//          first k; unused entries -1 and 0; k may exceed n_db.
// EDGES.   For i ascending, then in list order, {edge_base + i, j}: grouped by left, NOT sorted by right and NOT
//          deduplicated (with self_base >= 0 a pair can appear as (a, b) and as (b, a)).
// The weights are at most PSX_QUERY_MAX_WEIGHT and the q of a row written by psx_bow_quantize* add up to at most 65535, so a
// score stays below 2^26 and a key below 2^46.  Scores are added in unsigned 32 bits on both sides, so rows of another
// origin still give the device what the reference gives.
constexpr int PSX_QUERY_MAX_VIEWS = 1 << 20;           // 20 index bits in psx_query_key
constexpr int PSX_QUERY_MAX_WEIGHT = 1023;
constexpr int PSX_QUERY_MAX_QUERIES = 4096;
constexpr long long PSX_QUERY_MAX_PARTIAL_KEYS = 1LL << 27;   // 1 GiB of block lists
constexpr int PSX_QUERY_TILE = 64;                     // views per side of a score workgroup: the block of the partial lists

PSX_BOW_HD inline bool psx_query_opts_ok(const psx_query_opts* o)
{
    return o != nullptr && o->k >= 1 && o->flags == 0 && o->reserved == 0 && o->self_base >= -1;
}

// larger key = earlier in a query's list; 0 is no candidate
PSX_BOW_HD inline unsigned long long psx_query_key(unsigned score, int j)
{
    return ((unsigned long long)score << 20) | (unsigned long long)(PSX_QUERY_MAX_VIEWS - 1 - j);
}
PSX_BOW_HD inline unsigned psx_query_key_score(unsigned long long key) { return (unsigned)(key >> 20); }
PSX_BOW_HD inline int psx_query_key_view(unsigned long long key) { return PSX_QUERY_MAX_VIEWS - 1 - (int)(key & 0xfffffULL); }

// is database view j, with this score, a candidate of the query whose own database index is `self` (-1: none)?
PSX_BOW_HD inline bool psx_query_candidate(unsigned score, int j, int limit, int self, unsigned min_score)
{
    return j < limit && j != self && score > 0u && score >= min_score;
}

#include <cmath>
// HOST ONLY (no device attribute: a kernel that names it does not compile): 0 for df = 0, otherwise
// 1 + floor(16 log2(N / df) + 0.5) in double
inline int psx_bow_weight(int df, int n_views)
{
    if (df <= 0) return 0;
    return 1 + (int)std::floor(16.0 * std::log2((double)n_views / (double)df) + 0.5);
}
