// affine_rule.h -- the 2-D affine and similarity RANSAC of psx_ransac_affine* and psx_ransac_similarity*
// (include/popsift_hip.h, "geometric verification").
//
// ONE set of inline functions, compiled for the host (psx_affine_fit, psx_similarity_fit, psx_ransac_affine_ref,
// psx_ransac_similarity_ref) and for the device (ransac.hip, ransac_graph.hip): the two cannot drift apart.  Every step is
// stated here operation by operation; the tests restate it from this comment.  The discipline is that of ransac_rule.h:
// integer steps are uint32 / uint64 arithmetic; the fit is IEEE double, every operation rounded on its own in exactly the
// order written (the translation units that include this header are compiled with -ffp-contract=off: no fused
// multiply-add), and uses only + - * /, fabs and comparisons -- no square root, no library function -- so host and device
// agree bit for bit.  There is no special case for a degenerate sample: whatever IEEE arithmetic gives (NaN, +-inf) is the
// result, and a model with a non-finite entry scores 0.
//
// Two models, MIN = 2 (SIMILARITY: rotation, uniform scale, translation; it cannot represent a reflection) and MIN = 3
// (AFFINE).  Both are 3 x 3 row-major matrices whose last row is exactly (0, 0, 1): PSX_GUIDE_HOMOGRAPHY matrices, left ->
// right.
//
// INPUT.  As in ransac_rule.h: n pair records of 16 bytes of which the first two ints (left, right) are read, two
// position arrays, tol, hypotheses = N, seed.  Pair p is (xl, yl) = left_xy[pairs[p].left] -> (xr, yr) =
// right_xy[pairs[p].right].
//
// 1. SAMPLES (integers only).  Step 1 of ransac_rule.h with MIN draws, the first MIN of the homography's four: mix(x) as
//    there;  for hypothesis h:  base = mix(seed ^ (0x9e3779b9 * (h + 1)))  in uint32.  For k = 0..MIN-1:
//        r = mix(base + k);   idx = (uint64(r) * (n - k)) >> 32;
//        for every index c chosen before, taken in ASCENDING ORDER OF VALUE:  if idx >= c then idx++
//    MIN distinct pair indices in [0, n), in draw order (n >= MIN).  (psx_ransac_sample_k<MIN>.)
//
// 2. FIT of n >= MIN correspondences (x_i, y_i) -> (u_i, v_i), in the given order, in double (the float32 positions are
//    converted exactly).  Every sum below starts at 0.0 and adds its terms serially, i ascending.
//    a. Normalise each side on its own exactly as step 2a of ransac_rule.h (shown for the left):  cx = (sum x_i) / n;
//       cy = (sum y_i) / n;  d = sum (fabs(x_i - cx) + fabs(y_i - cy));  s = n / d;  point ((x_i - cx) * s, (y_i - cy) * s).
//       (cx_l, cy_l, s_l) and (cx_r, cy_r, s_r); from here on x, y, u, v are the NORMALISED coordinates.
//    b. SIMILARITY.  den = sum (x*x + y*y);   P = sum (x*u + y*v);   Q = sum (x*v - y*u);   p = P / den;   q = Q / den.
//       The normalised rows are  (p, 0.0 - q, 0.0)  and  (q, p, 0.0).
//    b. AFFINE.  With r = [x  y  1], correspondence i contributes:  for i = 0..2:  for j = 0..i:
//       S[i][j] = S[i][j] + r[i] * r[j];   then, for i = 0..2:  gu[i] = gu[i] + r[i] * u;   gv[i] = gv[i] + r[i] * v.
//       LDL^T without pivoting, step 2c of ransac_rule.h with 3 in place of 8.  For j = 0..2:
//           D[j] = S[j][j] - (sum over k = 0..j-1, ascending, of (L[j][k] * L[j][k]) * D[k])
//           for i = j+1..2:  L[i][j] = (S[i][j] - (sum over k = 0..j-1, ascending, of (L[i][k] * L[j][k]) * D[k])) / D[j]
//       Then once with g = gu (giving normalised row 0) and once with g = gv (row 1):
//           forward:   z[i] = g[i] - (sum over k = 0..i-1, ascending, of L[i][k] * z[k]),   i = 0..2
//           diagonal:  w[i] = z[i] / D[i]
//           backward:  q[i] = w[i] - (sum over k = i+1..2, ascending, of L[k][i] * q[k]),   i = 2..0
//       The normalised row is (q0, q1, q2).
//    c. Denormalise.  With ir = 1 / s_r, for each of the two normalised rows (a, b, c):  A = a * s_l;  B = b * s_l;
//           C = (c - A * cx_l) - B * cy_l.
//       Row 0 of the model, from the first normalised row:   (A * ir, B * ir, C * ir + cx_r);
//       row 1 of the model, from the second normalised row:  (A * ir, B * ir, C * ir + cy_r);
//       row 2 is literally (0, 0, 1).
//    d. Round the six doubles to float32 (round to nearest even); row 2 is 0.0f, 0.0f, 1.0f.
//    A duplicated left point in a 2-sample makes d = 0 and the entries NaN; three collinear left points give a zero pivot
//    and a non-finite model.
//
// 3. SCORE.  count[h] = number of pairs p with psx_guide_pair(PSX_GUIDE_HOMOGRAPHY, m_h, tol, xl, yl, xr, yr)
//    (guide_rule.h, unchanged); 0 when any of the nine entries of m_h is NaN or +-inf.
// 4. SELECT.  The largest count; ties go to the lowest h.  count[best] is `sample_inliers`.
// 5. REFIT (PSX_RANSAC_REFIT), one round: when sample_inliers >= MIN, fit (step 2) the winner's inliers in pair order and
//    score that model; it replaces the sample model iff all its entries are finite and its count >= sample_inliers.
// 6. INLIERS.  The input records whose pair passes the rule under the kept model, in input order; their number is
//    `inliers`.  A kept model with a non-finite entry (every hypothesis degenerate) is reported as "no model": best = -1,
//    a zero matrix, no inliers -- as for n < MIN.
#pragma once

#include "fundamental_rule.h"

// The models of the estimator.  The first two are named by the guide their matrix is; the two of this header are
// PSX_GUIDE_HOMOGRAPHY matrices as well and get ids of their own.
#define PSX_RANSAC_MODEL_HOMOGRAPHY PSX_GUIDE_HOMOGRAPHY
#define PSX_RANSAC_MODEL_FUNDAMENTAL PSX_GUIDE_EPIPOLAR
#define PSX_RANSAC_MODEL_AFFINE 3
#define PSX_RANSAC_MODEL_SIMILARITY 4

#define PSX_AFFINE_MIN 3
#define PSX_SIMILARITY_MIN 2

struct psx_affine_frame { double cxl, cyl, cxr, cyr, sl, sr; };          // step 2a of both sides

// step 2a.  NFIX as in psx_homography_fit_rule.
template <int NFIX>
PSX_GUIDE_HD inline psx_affine_frame psx_affine_normalise(const psx_ransac_pt* pt, int n_dyn)
{
    const int n = NFIX > 0 ? NFIX : n_dyn;
    constexpr int UN = NFIX > 0 ? NFIX : 1;
    (void)UN;
    const double dn = (double)n;
    double sxl = 0.0, syl = 0.0, sxr = 0.0, syr = 0.0;
    PSX_RANSAC_UNROLL_N
    for (int i = 0; i < n; i++) {
        sxl = sxl + (double)pt[i].xl; syl = syl + (double)pt[i].yl;
        sxr = sxr + (double)pt[i].xr; syr = syr + (double)pt[i].yr;
    }
    psx_affine_frame f;
    f.cxl = sxl / dn; f.cyl = syl / dn; f.cxr = sxr / dn; f.cyr = syr / dn;
    double dl = 0.0, dr = 0.0;
    PSX_RANSAC_UNROLL_N
    for (int i = 0; i < n; i++) {
        dl = dl + (fabs((double)pt[i].xl - f.cxl) + fabs((double)pt[i].yl - f.cyl));
        dr = dr + (fabs((double)pt[i].xr - f.cxr) + fabs((double)pt[i].yr - f.cyr));
    }
    f.sl = dn / dl; f.sr = dn / dr;
    return f;
}

// steps 2c and 2d: the two normalised rows (a0 b0 c0), (a1 b1 c1) into the nine floats
PSX_GUIDE_HD inline void psx_affine_denormalise(const psx_affine_frame& f, const double row[6], float m[9])
{
    const double ir = 1.0 / f.sr;
    PSX_RANSAC_UNROLL
    for (int r = 0; r < 2; r++) {
        const double A = row[3 * r] * f.sl, B = row[3 * r + 1] * f.sl;
        const double Cc = (row[3 * r + 2] - A * f.cxl) - B * f.cyl;
        m[3 * r] = (float)(A * ir);
        m[3 * r + 1] = (float)(B * ir);
        m[3 * r + 2] = (float)(Cc * ir + (r == 0 ? f.cxr : f.cyr));
    }
    m[6] = 0.0f; m[7] = 0.0f; m[8] = 1.0f;
}

// step 2, SIMILARITY.  NFIX > 0: the number of correspondences is that compile-time constant (every loop unrolls: the
// device keeps the whole fit in registers); NFIX == 0: n of them.
template <int NFIX>
PSX_GUIDE_HD inline void psx_similarity_fit_rule(const psx_ransac_pt* pt, int n_dyn, float m[9])
{
    const int n = NFIX > 0 ? NFIX : n_dyn;
    constexpr int UN = NFIX > 0 ? NFIX : 1;
    (void)UN;
    const psx_affine_frame f = psx_affine_normalise<NFIX>(pt, n);
    double den = 0.0, P = 0.0, Q = 0.0;
    PSX_RANSAC_UNROLL_N
    for (int c = 0; c < n; c++) {
        const double x = ((double)pt[c].xl - f.cxl) * f.sl, y = ((double)pt[c].yl - f.cyl) * f.sl;
        const double u = ((double)pt[c].xr - f.cxr) * f.sr, v = ((double)pt[c].yr - f.cyr) * f.sr;
        den = den + (x * x + y * y);
        P = P + (x * u + y * v);
        Q = Q + (x * v - y * u);
    }
    const double p = P / den, q = Q / den;
    const double row[6] = {p, 0.0 - q, 0.0, q, p, 0.0};
    psx_affine_denormalise(f, row, m);
}

// step 2, AFFINE.  NFIX as above.
template <int NFIX>
PSX_GUIDE_HD inline void psx_affine_fit_rule(const psx_ransac_pt* pt, int n_dyn, float m[9])
{
    const int n = NFIX > 0 ? NFIX : n_dyn;
    constexpr int UN = NFIX > 0 ? NFIX : 1;
    (void)UN;
    const psx_affine_frame f = psx_affine_normalise<NFIX>(pt, n);
    // b. normal equations: S lower triangle (row i holds j = 0..i), one right-hand side per row of the model
    double S[3][3], g[2][3];
    PSX_RANSAC_UNROLL
    for (int i = 0; i < 3; i++) {
        g[0][i] = 0.0; g[1][i] = 0.0;
        PSX_RANSAC_UNROLL
        for (int j = 0; j < 3; j++) S[i][j] = 0.0;
    }
    PSX_RANSAC_UNROLL_N
    for (int c = 0; c < n; c++) {
        const double x = ((double)pt[c].xl - f.cxl) * f.sl, y = ((double)pt[c].yl - f.cyl) * f.sl;
        const double u = ((double)pt[c].xr - f.cxr) * f.sr, v = ((double)pt[c].yr - f.cyr) * f.sr;
        const double r[3] = {x, y, 1.0};
        PSX_RANSAC_UNROLL
        for (int i = 0; i < 3; i++) {
            PSX_RANSAC_UNROLL
            for (int j = 0; j <= i; j++) S[i][j] = S[i][j] + r[i] * r[j];
        }
        PSX_RANSAC_UNROLL
        for (int i = 0; i < 3; i++) {
            g[0][i] = g[0][i] + r[i] * u;
            g[1][i] = g[1][i] + r[i] * v;
        }
    }
    // LDL^T in place: L[i][j] replaces S[i][j] for i > j, D[j] is kept apart
    double D[3];
    PSX_RANSAC_UNROLL
    for (int j = 0; j < 3; j++) {
        double sum = 0.0;
        PSX_RANSAC_UNROLL
        for (int k = 0; k < j; k++) sum = sum + (S[j][k] * S[j][k]) * D[k];
        D[j] = S[j][j] - sum;
        PSX_RANSAC_UNROLL
        for (int i = j + 1; i < 3; i++) {
            double t = 0.0;
            PSX_RANSAC_UNROLL
            for (int k = 0; k < j; k++) t = t + (S[i][k] * S[j][k]) * D[k];
            S[i][j] = (S[i][j] - t) / D[j];
        }
    }
    double row[6];
    PSX_RANSAC_UNROLL
    for (int e = 0; e < 2; e++) {
        double q[3];
        PSX_RANSAC_UNROLL
        for (int i = 0; i < 3; i++) {
            double t = 0.0;
            PSX_RANSAC_UNROLL
            for (int k = 0; k < i; k++) t = t + S[i][k] * q[k];
            q[i] = g[e][i] - t;
        }
        PSX_RANSAC_UNROLL
        for (int i = 0; i < 3; i++) q[i] = q[i] / D[i];
        PSX_RANSAC_UNROLL
        for (int i = 2; i >= 0; i--) {
            double t = 0.0;
            PSX_RANSAC_UNROLL
            for (int k = i + 1; k < 3; k++) t = t + S[k][i] * q[k];
            q[i] = q[i] - t;
        }
        row[3 * e] = q[0]; row[3 * e + 1] = q[1]; row[3 * e + 2] = q[2];
    }
    psx_affine_denormalise(f, row, m);
}

// the fit of a model of this header by its sample size (PSX_SIMILARITY_MIN or PSX_AFFINE_MIN)
template <int MIN, int NFIX>
PSX_GUIDE_HD inline void psx_affine_fit_by_min(const psx_ransac_pt* pt, int n, float m[9])
{
    if (MIN == PSX_SIMILARITY_MIN) psx_similarity_fit_rule<NFIX>(pt, n, m);
    else psx_affine_fit_rule<NFIX>(pt, n, m);
}

// The whole rule on host arrays (psx_ransac_affine_ref, psx_ransac_similarity_ref); arguments, passes and `scratch`
// (n psx_ransac_pt, the caller's) as psx_ransac_homography_host.  models (N x 9) and counts (N) may be NULL.
template <int MIN>
inline int psx_ransac_affine_host_rule(const void* pairs, int n, const float* left_xy, int nl, const float* right_xy, int nr,
                                       const psx_ransac_opts* opts, psx_ransac_result* result, void* inliers, int capacity,
                                       int* count, float* models, int* counts, psx_ransac_pt* scratch)
{
    if (!psx_ransac_opts_ok(opts) || result == nullptr || count == nullptr || n < 0 || nl < 0 || nr < 0 || capacity < 0) return PSX_ERR_INVALID;
    if ((n > 0 && pairs == nullptr) || (nl > 0 && left_xy == nullptr) || (nr > 0 && right_xy == nullptr)) return PSX_ERR_INVALID;
    if ((capacity > 0 && inliers == nullptr) || (n >= MIN && scratch == nullptr)) return PSX_ERR_INVALID;
    const int* rec = static_cast<const int*>(pairs);                             // 4 ints per record: left, right, two distances
    for (int p = 0; p < n; p++)
        if (rec[4 * (size_t)p] < 0 || rec[4 * (size_t)p] >= nl || rec[4 * (size_t)p + 1] < 0 || rec[4 * (size_t)p + 1] >= nr)
            return PSX_ERR_INVALID;
    if (n < MIN) { psx_ransac_no_model(result); *count = 0; return PSX_OK; }
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
        int idx[MIN];
        psx_ransac_sample_k<MIN>(opts->seed, h, n, idx);
        psx_ransac_pt q[MIN];
        for (int k = 0; k < MIN; k++) q[k] = scratch[idx[k]];
        float m[9];
        psx_affine_fit_by_min<MIN, MIN>(q, MIN, m);
        const int c = psx_ransac_count(m, tol, scratch, n);
        if (models) for (int k = 0; k < 9; k++) models[9 * (size_t)h + k] = m[k];
        if (counts) counts[h] = c;
        if (c > best_count) { best_count = c; best = h; for (int k = 0; k < 9; k++) kept[k] = m[k]; }
    }
    int refit_kept = 0;
    if ((opts->flags & PSX_RANSAC_REFIT) != 0 && best_count >= MIN) {
        // the winner's inliers in pair order, packed behind one another in a buffer of their own
        psx_ransac_pt* in = new psx_ransac_pt[(size_t)best_count];
        int k = 0;
        for (int p = 0; p < n; p++)
            if (psx_ransac_inlier(kept, tol, scratch[p])) in[k++] = scratch[p];
        float m[9];
        psx_affine_fit_by_min<MIN, 0>(in, best_count, m);
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

inline int psx_ransac_affine_host(const void* pairs, int n, const float* left_xy, int nl, const float* right_xy, int nr,
                                  const psx_ransac_opts* opts, psx_ransac_result* result, void* inliers, int capacity, int* count,
                                  float* models, int* counts, psx_ransac_pt* scratch)
{
    return psx_ransac_affine_host_rule<PSX_AFFINE_MIN>(pairs, n, left_xy, nl, right_xy, nr, opts, result, inliers, capacity, count, models,
                                                       counts, scratch);
}

inline int psx_ransac_similarity_host(const void* pairs, int n, const float* left_xy, int nl, const float* right_xy, int nr,
                                      const psx_ransac_opts* opts, psx_ransac_result* result, void* inliers, int capacity, int* count,
                                      float* models, int* counts, psx_ransac_pt* scratch)
{
    return psx_ransac_affine_host_rule<PSX_SIMILARITY_MIN>(pairs, n, left_xy, nl, right_xy, nr, opts, result, inliers, capacity, count,
                                                           models, counts, scratch);
}

// the single-list host rule of a model id and its sample size
typedef int (*psx_ransac_host_fn)(const void*, int, const float*, int, const float*, int, const psx_ransac_opts*, psx_ransac_result*, void*, int,
                                  int*, float*, int*, psx_ransac_pt*);
inline psx_ransac_host_fn psx_ransac_host_rule(int model)
{
    return model == PSX_RANSAC_MODEL_FUNDAMENTAL ? psx_ransac_fundamental_host
         : model == PSX_RANSAC_MODEL_AFFINE      ? psx_ransac_affine_host
         : model == PSX_RANSAC_MODEL_SIMILARITY  ? psx_ransac_similarity_host
                                                 : psx_ransac_homography_host;
}
inline int psx_ransac_host_min(int model)
{
    return model == PSX_RANSAC_MODEL_FUNDAMENTAL ? PSX_FUND_MIN
         : model == PSX_RANSAC_MODEL_AFFINE      ? PSX_AFFINE_MIN
         : model == PSX_RANSAC_MODEL_SIMILARITY  ? PSX_SIMILARITY_MIN
                                                 : 4;
}
