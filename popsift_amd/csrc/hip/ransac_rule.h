// ransac_rule.h -- the homography RANSAC of psx_ransac_homography* (include/popsift_hip.h, "geometric verification").
//
// ONE set of inline functions, compiled for the host (psx_ransac_samples, psx_homography_fit, psx_ransac_homography_ref)
// and for the device (ransac.hip): the two cannot drift apart.  Every step is stated here operation by operation; the
// tests restate it from this comment.  Integer steps are uint32 / uint64 arithmetic; the fit is IEEE double, every
// operation rounded on its own in exactly the order written (the translation units that include this header are compiled
// with -ffp-contract=off: no fused multiply-add), and uses only + - * /, fabs and comparisons -- no square root, no
// library function -- so host and device agree bit for bit.  There is no special case for a degenerate sample: whatever
// IEEE arithmetic gives (NaN, +-inf) is the result, and a model with a non-finite entry scores 0.
//
// INPUT.  n pair records of 16 bytes, of which only the first two ints (left, right) are read (psx_match_pair and
// psx_match_pair_u8 both serve); two position arrays as psx_desc_positions writes them; tol, hypotheses = N, seed.  Pair p
// is the correspondence (xl, yl) = left_xy[pairs[p].left] -> (xr, yr) = right_xy[pairs[p].right].
//
// 1. SAMPLES (integers only).  mix(x) on uint32:  x ^= x >> 16;  x *= 0x7feb352d;  x ^= x >> 15;  x *= 0x846ca68b;
//    x ^= x >> 16.  For hypothesis h:  base = mix(seed ^ (0x9e3779b9 * (h + 1)))  in uint32.  For k = 0..3:
//        r = mix(base + k);   idx = (uint64(r) * (n - k)) >> 32;
//        for every index c chosen before, taken in ASCENDING ORDER OF VALUE:  if idx >= c then idx++
//    Four distinct pair indices in [0, n), in draw order (n >= 4).
//
// 2. FIT of n >= 4 correspondences (x_i, y_i) -> (u_i, v_i), in the given order, in double (the float32 positions are
//    converted exactly).  Every sum below starts at 0.0 and adds its terms serially, i ascending.
//    a. Each side on its own (shown for the left):  cx = (sum x_i) / n;  cy = (sum y_i) / n;
//       d = sum (fabs(x_i - cx) + fabs(y_i - cy));  s = n / d;  normalised point ((x_i - cx) * s, (y_i - cy) * s).
//       (cx_l, cy_l, s_l) and (cx_r, cy_r, s_r); from here on x, y, u, v are the NORMALISED coordinates.
//    b. Normal equations.  Correspondence i contributes two rows of 8 entries with a right-hand side, first
//           r = [x  y  1  0  0  0  -(u*x)  -(u*y)],  t = u      then
//           r = [0  0  0  x  y  1  -(v*x)  -(v*y)],  t = v.
//       For each row, for i = 0..7:  for j = 0..i:  S[i][j] = S[i][j] + r[i] * r[j];   then  g[i] = g[i] + r[i] * t.
//       All 36 + 8 sums take every row, zero entries included (0 * NaN is NaN).
//    c. LDL^T without pivoting.  For j = 0..7:
//           D[j] = S[j][j] - (sum over k = 0..j-1, ascending, of (L[j][k] * L[j][k]) * D[k])
//           for i = j+1..7:  L[i][j] = (S[i][j] - (sum over k = 0..j-1, ascending, of (L[i][k] * L[j][k]) * D[k])) / D[j]
//       forward:   z[i] = g[i] - (sum over k = 0..i-1, ascending, of L[i][k] * z[k]),   i = 0..7
//       diagonal:  w[i] = z[i] / D[i]
//       backward:  q[i] = w[i] - (sum over k = i+1..7, ascending, of L[k][i] * q[k]),   i = 7..0
//       The normalised model is  [q0 q1 q2; q3 q4 q5; q6 q7 1].
//    d. Denormalise.  For each row (a, b, c) of the normalised model:  A = a * s_l;  B = b * s_l;
//           G = (A, B, (c - A * cx_l) - B * cy_l).          With ir = 1 / s_r and rows G0, G1, G2, entry by entry:
//           H row 0 = G0 * ir + cx_r * G2;   H row 1 = G1 * ir + cy_r * G2;   H row 2 = G2.
//    e. Round the nine doubles to float32 (round to nearest even).
//
// 3. SCORE.  count[h] = number of pairs p with psx_guide_pair(PSX_GUIDE_HOMOGRAPHY, m_h, tol, xl, yl, xr, yr)
//    (guide_rule.h, unchanged); 0 when any of the nine entries of m_h is NaN or +-inf.
// 4. SELECT.  The largest count; ties go to the lowest h.  count[best] is `sample_inliers`.
// 5. REFIT (PSX_RANSAC_REFIT), one round: when sample_inliers >= 4, fit (step 2) the winner's inliers in pair order and
//    score that model; it replaces the sample model iff all its entries are finite and its count >= sample_inliers.
// 6. INLIERS.  The input records whose pair passes the rule under the kept model, in input order; their number is
//    `inliers`.  A kept model with a non-finite entry (every hypothesis degenerate) is reported as "no model": best = -1,
//    a zero matrix, no inliers -- as for n < 4.
#pragma once

#include <math.h>
#include <stdint.h>

#include "guide_rule.h"
#include "popsift_hip.h"

#if defined(__HIPCC__)
#define PSX_RANSAC_UNROLL _Pragma("unroll")
#define PSX_RANSAC_UNROLL_N _Pragma("unroll UN")      // loops over the correspondences: unrolled when their number is fixed
#else
#define PSX_RANSAC_UNROLL
#define PSX_RANSAC_UNROLL_N
#endif

#define PSX_RANSAC_MAX_HYPOTHESES 65536

struct psx_ransac_pt { float xl, yl, xr, yr; };      // one correspondence, 16 bytes (a float4 on the device)

PSX_GUIDE_HD inline uint32_t psx_ransac_mix(uint32_t x)
{
    x ^= x >> 16; x *= 0x7feb352du;
    x ^= x >> 15; x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

// step 1: the four pair indices of hypothesis h among n >= 4 pairs, in draw order
PSX_GUIDE_HD inline void psx_ransac_sample(uint32_t seed, int h, int n, int idx[4])
{
    const uint32_t base = psx_ransac_mix(seed ^ (0x9e3779b9u * ((uint32_t)h + 1u)));
    int s0 = 0, s1 = 0, s2 = 0;                       // the indices chosen so far, ascending (k of them are valid)
    PSX_RANSAC_UNROLL
    for (int k = 0; k < 4; k++) {
        const uint32_t r = psx_ransac_mix(base + (uint32_t)k);
        int v = (int)(((uint64_t)r * (uint64_t)(uint32_t)(n - k)) >> 32);
        if (k > 0 && v >= s0) v++;
        if (k > 1 && v >= s1) v++;
        if (k > 2 && v >= s2) v++;
        idx[k] = v;
        // insert v into the ascending list
        if (k == 0) s0 = v;
        else if (k == 1) { if (v < s0) { s1 = s0; s0 = v; } else s1 = v; }
        else if (k == 2) {
            if (v < s0) { s2 = s1; s1 = s0; s0 = v; }
            else if (v < s1) { s2 = s1; s1 = v; }
            else s2 = v;
        }
    }
}

PSX_GUIDE_HD inline bool psx_ransac_model_finite(const float* m)
{
    bool ok = true;
    PSX_RANSAC_UNROLL
    for (int k = 0; k < 9; k++) ok = ok && (fabsf(m[k]) < INFINITY);
    return ok;
}

// step 3 for one pair under a model already known to be finite
PSX_GUIDE_HD inline bool psx_ransac_inlier(const float* m, float tol, const psx_ransac_pt& p)
{
    return psx_guide_right(PSX_GUIDE_HOMOGRAPHY, psx_guide_left(PSX_GUIDE_HOMOGRAPHY, m, tol, p.xl, p.yl), p.xr, p.yr);
}

// step 2.  NFIX > 0: the number of correspondences is that compile-time constant (every loop unrolls: the device keeps
// the whole fit in registers); NFIX == 0: n of them.
template <int NFIX>
PSX_GUIDE_HD inline void psx_homography_fit_rule(const psx_ransac_pt* pt, int n_dyn, float m[9])
{
    const int n = NFIX > 0 ? NFIX : n_dyn;
    constexpr int UN = NFIX > 0 ? NFIX : 1;
    (void)UN;
    const double dn = (double)n;
    // a. normalisation of each side
    double sxl = 0.0, syl = 0.0, sxr = 0.0, syr = 0.0;
    PSX_RANSAC_UNROLL_N
    for (int i = 0; i < n; i++) {
        sxl = sxl + (double)pt[i].xl; syl = syl + (double)pt[i].yl;
        sxr = sxr + (double)pt[i].xr; syr = syr + (double)pt[i].yr;
    }
    const double cxl = sxl / dn, cyl = syl / dn, cxr = sxr / dn, cyr = syr / dn;
    double dl = 0.0, dr = 0.0;
    PSX_RANSAC_UNROLL_N
    for (int i = 0; i < n; i++) {
        dl = dl + (fabs((double)pt[i].xl - cxl) + fabs((double)pt[i].yl - cyl));
        dr = dr + (fabs((double)pt[i].xr - cxr) + fabs((double)pt[i].yr - cyr));
    }
    const double sl = dn / dl, sr = dn / dr;
    // b. normal equations: S lower triangle (row i holds j = 0..i), g
    double S[8][8], g[8];
    PSX_RANSAC_UNROLL
    for (int i = 0; i < 8; i++) {
        g[i] = 0.0;
        PSX_RANSAC_UNROLL
        for (int j = 0; j < 8; j++) S[i][j] = 0.0;
    }
    PSX_RANSAC_UNROLL_N
    for (int c = 0; c < n; c++) {
        const double x = ((double)pt[c].xl - cxl) * sl, y = ((double)pt[c].yl - cyl) * sl;
        const double u = ((double)pt[c].xr - cxr) * sr, v = ((double)pt[c].yr - cyr) * sr;
        const double r0[8] = {x, y, 1.0, 0.0, 0.0, 0.0, -(u * x), -(u * y)};
        const double r1[8] = {0.0, 0.0, 0.0, x, y, 1.0, -(v * x), -(v * y)};
        PSX_RANSAC_UNROLL
        for (int i = 0; i < 8; i++) {
            PSX_RANSAC_UNROLL
            for (int j = 0; j <= i; j++) S[i][j] = S[i][j] + r0[i] * r0[j];
            g[i] = g[i] + r0[i] * u;
        }
        PSX_RANSAC_UNROLL
        for (int i = 0; i < 8; i++) {
            PSX_RANSAC_UNROLL
            for (int j = 0; j <= i; j++) S[i][j] = S[i][j] + r1[i] * r1[j];
            g[i] = g[i] + r1[i] * v;
        }
    }
    // c. LDL^T in place: L[i][j] replaces S[i][j] for i > j, D[j] is kept apart
    double D[8];
    PSX_RANSAC_UNROLL
    for (int j = 0; j < 8; j++) {
        double sum = 0.0;
        PSX_RANSAC_UNROLL
        for (int k = 0; k < j; k++) sum = sum + (S[j][k] * S[j][k]) * D[k];
        D[j] = S[j][j] - sum;
        PSX_RANSAC_UNROLL
        for (int i = j + 1; i < 8; i++) {
            double t = 0.0;
            PSX_RANSAC_UNROLL
            for (int k = 0; k < j; k++) t = t + (S[i][k] * S[j][k]) * D[k];
            S[i][j] = (S[i][j] - t) / D[j];
        }
    }
    double q[8];
    PSX_RANSAC_UNROLL
    for (int i = 0; i < 8; i++) {
        double t = 0.0;
        PSX_RANSAC_UNROLL
        for (int k = 0; k < i; k++) t = t + S[i][k] * q[k];
        q[i] = g[i] - t;
    }
    PSX_RANSAC_UNROLL
    for (int i = 0; i < 8; i++) q[i] = q[i] / D[i];
    PSX_RANSAC_UNROLL
    for (int i = 7; i >= 0; i--) {
        double t = 0.0;
        PSX_RANSAC_UNROLL
        for (int k = i + 1; k < 8; k++) t = t + S[k][i] * q[k];
        q[i] = q[i] - t;
    }
    // d. denormalise
    const double hn[9] = {q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7], 1.0};
    double G[9];
    PSX_RANSAC_UNROLL
    for (int r = 0; r < 3; r++) {
        const double A = hn[3 * r] * sl, B = hn[3 * r + 1] * sl;
        G[3 * r] = A; G[3 * r + 1] = B;
        G[3 * r + 2] = (hn[3 * r + 2] - A * cxl) - B * cyl;
    }
    const double ir = 1.0 / sr;
    PSX_RANSAC_UNROLL
    for (int k = 0; k < 3; k++) {
        m[k] = (float)(G[k] * ir + cxr * G[6 + k]);
        m[3 + k] = (float)(G[3 + k] * ir + cyr * G[6 + k]);
        m[6 + k] = (float)G[6 + k];
    }
}

// the argument checks every entry point shares (data pointers are the caller's to check)
inline bool psx_ransac_opts_ok(const psx_ransac_opts* o)
{
    if (o == nullptr) return false;
    if (!(o->tol >= 0.0f && o->tol < INFINITY)) return false;                     // NaN, negative, +inf
    if (o->hypotheses < 1 || o->hypotheses > PSX_RANSAC_MAX_HYPOTHESES) return false;
    return (o->flags & ~PSX_RANSAC_REFIT) == 0;
}

inline void psx_ransac_no_model(psx_ransac_result* r)
{
    for (int k = 0; k < 9; k++) r->m[k] = 0.0f;
    r->best = -1; r->sample_inliers = 0; r->inliers = 0; r->refit_kept = 0;
}

// score of one model over n correspondences (step 3)
inline int psx_ransac_count(const float* m, float tol, const psx_ransac_pt* pt, int n)
{
    if (!psx_ransac_model_finite(m)) return 0;
    int c = 0;
    for (int p = 0; p < n; p++) c += psx_ransac_inlier(m, tol, pt[p]) ? 1 : 0;
    return c;
}

// The whole rule on host arrays (psx_ransac_homography_ref).  `scratch` holds n psx_ransac_pt and is the caller's (so that
// a stand-alone program can hand exact-size heap arrays to a sanitizer).  Two passes: every argument and index is checked
// before anything is written.  models (N x 9) and counts (N) may be NULL.
inline int psx_ransac_homography_host(const void* pairs, int n, const float* left_xy, int nl, const float* right_xy, int nr,
                                      const psx_ransac_opts* opts, psx_ransac_result* result, void* inliers, int capacity,
                                      int* count, float* models, int* counts, psx_ransac_pt* scratch)
{
    if (!psx_ransac_opts_ok(opts) || result == nullptr || count == nullptr || n < 0 || nl < 0 || nr < 0 || capacity < 0) return PSX_ERR_INVALID;
    if ((n > 0 && pairs == nullptr) || (nl > 0 && left_xy == nullptr) || (nr > 0 && right_xy == nullptr)) return PSX_ERR_INVALID;
    if ((capacity > 0 && inliers == nullptr) || (n >= 4 && scratch == nullptr)) return PSX_ERR_INVALID;
    const int* rec = static_cast<const int*>(pairs);                             // 4 ints per record: left, right, two distances
    for (int p = 0; p < n; p++)
        if (rec[4 * (size_t)p] < 0 || rec[4 * (size_t)p] >= nl || rec[4 * (size_t)p + 1] < 0 || rec[4 * (size_t)p + 1] >= nr)
            return PSX_ERR_INVALID;
    if (n < 4) { psx_ransac_no_model(result); *count = 0; return PSX_OK; }
    for (int p = 0; p < n; p++) {
        const size_t l = (size_t)rec[4 * (size_t)p], r = (size_t)rec[4 * (size_t)p + 1];
        scratch[p].xl = left_xy[2 * l]; scratch[p].yl = left_xy[2 * l + 1];
        scratch[p].xr = right_xy[2 * r]; scratch[p].yr = right_xy[2 * r + 1];
    }
    const int N = opts->hypotheses;
    const float tol = opts->tol;
    float kept[9] = {};
    int best = -1, best_count = -1;
    for (int h = 0; h < N; h++) {
        int idx[4];
        psx_ransac_sample(opts->seed, h, n, idx);
        const psx_ransac_pt q[4] = {scratch[idx[0]], scratch[idx[1]], scratch[idx[2]], scratch[idx[3]]};
        float m[9];
        psx_homography_fit_rule<4>(q, 4, m);
        const int c = psx_ransac_count(m, tol, scratch, n);
        if (models) for (int k = 0; k < 9; k++) models[9 * (size_t)h + k] = m[k];
        if (counts) counts[h] = c;
        if (c > best_count) { best_count = c; best = h; for (int k = 0; k < 9; k++) kept[k] = m[k]; }
    }
    int refit_kept = 0;
    if ((opts->flags & PSX_RANSAC_REFIT) != 0 && best_count >= 4) {
        // the winner's inliers in pair order, packed behind one another in a buffer of their own
        psx_ransac_pt* in = new psx_ransac_pt[(size_t)best_count];
        int k = 0;
        for (int p = 0; p < n; p++)
            if (psx_ransac_inlier(kept, tol, scratch[p])) in[k++] = scratch[p];
        float m[9];
        psx_homography_fit_rule<0>(in, best_count, m);
        delete[] in;
        const int c = psx_ransac_count(m, tol, scratch, n);
        if (psx_ransac_model_finite(m) && c >= best_count) {
            for (int j = 0; j < 9; j++) kept[j] = m[j];
            refit_kept = 1;
        }
    }
    if (!psx_ransac_model_finite(kept)) { psx_ransac_no_model(result); *count = 0; return PSX_OK; }
    int w = 0;
    for (int p = 0; p < n; p++) {
        if (!psx_ransac_inlier(kept, tol, scratch[p])) continue;
        if (w < capacity) for (int j = 0; j < 4; j++) static_cast<int*>(inliers)[4 * (size_t)w + j] = rec[4 * (size_t)p + j];
        w++;
    }
    for (int k = 0; k < 9; k++) result->m[k] = kept[k];
    result->best = best; result->sample_inliers = best_count; result->inliers = w; result->refit_kept = refit_kept;
    *count = w;
    return PSX_OK;
}
