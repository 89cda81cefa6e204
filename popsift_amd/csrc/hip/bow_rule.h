// bow_rule.h -- the rules of the view shortlist (psx_vocab_train_u8*, psx_bow_u8*, psx_shortlist_views*; include/popsift_hip.h).
//
// ONE set of inline functions, compiled for the host (the references, bow_plan.h) and for the device (bow.hip): the two
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

#include <cmath>
// HOST ONLY (no device attribute: a kernel that names it does not compile): 0 for df = 0, otherwise
// 1 + floor(16 log2(N / df) + 0.5) in double
inline int psx_bow_weight(int df, int n_views)
{
    if (df <= 0) return 0;
    return 1 + (int)std::floor(16.0 * std::log2((double)n_views / (double)df) + 0.5);
}
