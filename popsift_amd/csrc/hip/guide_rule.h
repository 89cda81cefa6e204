// guide_rule.h -- the admissibility rule of guided matching (psx_match_guided / psx_match_pairs_guided, include/popsift_hip.h).
//
// ONE inline predicate, compiled for the host (psx_guide_allows) and for the device (k_match_guided in match_guided.hip):
// the two cannot drift apart.  A guide restricts the right descriptors a left descriptor may be matched with by their
// POSITIONS, in input-image units (what psx_feature reports): left (xl, yl), right (xr, yr), matrix m row major,
//     a = (m0*xl + m1*yl) + m2;   b = (m3*xl + m4*yl) + m5;   c = (m6*xl + m7*yl) + m8
//     HOMOGRAPHY: allowed iff  c > 0  and  (dx*dx + dy*dy) <= (tol*c)*(tol*c),   dx = a - c*xr,  dy = b - c*yr
//     EPIPOLAR:   e = (a*xr + b*yr) + c;   allowed iff  e*e <= (tol*tol) * (a*a + b*b)
// Float32 only, every operation rounded on its own in exactly this order: no fmaf, no division, no square root (both
// tests are the squared, denominator-free forms of "within tol pixels"), so host, device and a numpy float32
// restatement agree bit for bit.  The translation units that include this header are compiled with -ffp-contract=off.
// The IEEE result of the comparison is the rule: a NaN anywhere compares false and the pair is inadmissible; a
// right-hand side that overflows to +inf admits everything that is not NaN.  The relation is defined on (left, right) and is
// NOT symmetric in its roles; a backward pass calls the same function with the loops exchanged.
#pragma once

#include <math.h>

#include "popsift_hip.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PSX_GUIDE_HD __host__ __device__
#else
#define PSX_GUIDE_HD
#endif

// The rule in two steps, so that what depends on the left point alone is computed once per left point: the same
// operations in the same order as the formulas above, whichever way they are grouped into calls.
//   psx_guide_left:  (a, b, c) of a left point and the right-hand side w of its comparison,
//                    w = (tol*c)*(tol*c) (homography) or (tol*tol)*(a*a + b*b) (epipolar)
//   psx_guide_right: the comparison for one right point
// kind: PSX_GUIDE_HOMOGRAPHY, anything else is read as PSX_GUIDE_EPIPOLAR (the entry points refuse other kinds before
// they get here).
struct psx_guide_line { float a, b, c, w; };

PSX_GUIDE_HD inline psx_guide_line psx_guide_left(int kind, const float* m, float tol, float xl, float yl)
{
    psx_guide_line l;
    l.a = (m[0] * xl + m[1] * yl) + m[2];
    l.b = (m[3] * xl + m[4] * yl) + m[5];
    l.c = (m[6] * xl + m[7] * yl) + m[8];
    if (kind == PSX_GUIDE_HOMOGRAPHY) { const float tc = tol * l.c; l.w = tc * tc; }
    else l.w = (tol * tol) * (l.a * l.a + l.b * l.b);
    return l;
}

PSX_GUIDE_HD inline bool psx_guide_right(int kind, const psx_guide_line& l, float xr, float yr)
{
    if (kind == PSX_GUIDE_HOMOGRAPHY) {
        const float dx = l.a - l.c * xr, dy = l.b - l.c * yr;
        return l.c > 0.0f && (dx * dx + dy * dy) <= l.w;
    }
    const float e = (l.a * xr + l.b * yr) + l.c;
    return e * e <= l.w;
}

// true: (left at (xl, yl), right at (xr, yr)) is admissible
PSX_GUIDE_HD inline bool psx_guide_pair(int kind, const float* m, float tol, float xl, float yl, float xr, float yr)
{
    return psx_guide_right(kind, psx_guide_left(kind, m, tol, xl, yl), xr, yr);
}

// a guide the entry points accept: a known kind, nine finite entries, a finite tolerance >= 0
PSX_GUIDE_HD inline bool psx_guide_valid(const psx_guide* g)
{
    if (g == nullptr) return false;
    if (g->kind != PSX_GUIDE_HOMOGRAPHY && g->kind != PSX_GUIDE_EPIPOLAR) return false;
    for (int k = 0; k < 9; k++)
        if (!(fabsf(g->m[k]) < INFINITY)) return false;          // NaN and +-inf
    return g->tol >= 0.0f && g->tol < INFINITY;
}
