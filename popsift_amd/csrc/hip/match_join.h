// match_join.h -- the host form of the pair join (psx_pairs_join / psx_pairs_join_u8, include/popsift_hip.h).
//
// Host code only, in a header so that a stand-alone program can compile it with a sanitizer (tests/cpp/match_join_san.cpp);
// match.hip instantiates it behind the two C entry points.  The ratio test is psx_match_keep of match_rule.h, the function
// the join kernels call.  Two passes: the first checks every argument and every index and writes nothing, the second
// writes -- an error leaves the outputs untouched.
#pragma once

#include "match_rule.h"
#include "popsift_hip.h"

// the argument checks every pairs entry point shares (the data pointers are the caller's to check)
inline bool psx_pairs_args_ok(int l_len, int r_len, const psx_match_opts* opts, const void* pairs, int capacity, const int* count)
{
    if (opts == nullptr || count == nullptr || l_len < 0 || r_len < 0 || capacity < 0) return false;
    if (!(opts->ratio > 0.0f)) return false;                       // NaN, zero, negative
    if ((opts->flags & ~PSX_PAIRS_MUTUAL) != 0) return false;
    if (capacity > 0 && pairs == nullptr) return false;
    return true;
}

template <class Dist, class Pair>
inline int psx_pairs_join_host(const int* fwd_match, const Dist* fwd_dist, int l_len, const int* bwd_match, int r_len,
                               const psx_match_opts* opts, Pair* pairs, int capacity, int* count)
{
    if (!psx_pairs_args_ok(l_len, r_len, opts, pairs, capacity, count)) return PSX_ERR_INVALID;
    const bool mutual = (opts->flags & PSX_PAIRS_MUTUAL) != 0;
    if (l_len > 0 && (fwd_match == nullptr || fwd_dist == nullptr)) return PSX_ERR_INVALID;
    if (mutual && r_len > 0 && bwd_match == nullptr) return PSX_ERR_INVALID;
    if (l_len == 0 || r_len == 0) { *count = 0; return PSX_OK; }
    for (int i = 0; i < l_len; i++) {
        const int j = fwd_match[3 * (size_t)i];
        if (j < 0 || j >= r_len) return PSX_ERR_INVALID;
    }
    if (mutual)
        for (int j = 0; j < r_len; j++) {
            const int i = bwd_match[3 * (size_t)j];
            if (i < 0 || i >= l_len) return PSX_ERR_INVALID;
        }
    const float ratio = opts->ratio;
    int n = 0;
    for (int i = 0; i < l_len; i++) {
        const int j = fwd_match[3 * (size_t)i];
        const Dist d1 = fwd_dist[2 * (size_t)i], d2 = fwd_dist[2 * (size_t)i + 1];
        if (!psx_match_keep(psx_match_dist(d1), psx_match_dist(d2), ratio)) continue;
        if (mutual && bwd_match[3 * (size_t)j] != i) continue;
        if (n < capacity) { pairs[n].left = i; pairs[n].right = j; pairs[n].d1 = d1; pairs[n].d2 = d2; }
        n++;
    }
    *count = n;
    return PSX_OK;
}
