// match_rule.h -- the pair rule of psx_match_pairs / psx_pairs_join (include/popsift_hip.h, "matches as data").
//
// ONE inline predicate, compiled for the host (the join of psx_pairs_join, match_join.h) and for the device (k_pairs_count /
// k_pairs_write in match.hip): the two cannot drift apart.  d1 <= d2 are the squared distances of a left descriptor's best and
// second-best right descriptor, as the directed matcher reports them (+inf where there is no such neighbour); the pair is
// kept iff
//     d1 / d2 < ratio
// one float32 IEEE division and one float32 comparison, nothing else: 0 / 0 and inf / inf are NaN and fail, d2 = +inf gives
// 0 and passes, ratio = +inf lets everything but NaN through.  ratio = 0.8f is the accept flag of psx_match.  No reciprocal,
// no fast-math: hipcc's '/' is correctly rounded, as the host's is, so both sides agree bit for bit.
// Byte distances are integers below 2^24 (exact in float32); INT_MAX stands for +inf (psx_match_dist).
#pragma once

#include <limits.h>
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PSX_MATCH_HD __host__ __device__
#else
#define PSX_MATCH_HD
#endif

// true: the ratio test keeps the pair
PSX_MATCH_HD inline bool psx_match_keep(float d1, float d2, float ratio) { return d1 / d2 < ratio; }

// a directed matcher's distance as the float the rule divides: a float as it is, a byte matcher's integer converted
PSX_MATCH_HD inline float psx_match_dist(float d) { return d; }
PSX_MATCH_HD inline float psx_match_dist(int d) { return d == INT_MAX ? INFINITY : (float)d; }
