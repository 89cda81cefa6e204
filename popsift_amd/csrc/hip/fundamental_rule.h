// fundamental_rule.h -- the fundamental-matrix RANSAC of psx_ransac_fundamental* (include/popsift_hip.h, "geometric
// verification").
//
// ONE set of inline functions, compiled for the host (psx_ransac_samples_k, psx_fundamental_fit,
// psx_ransac_fundamental_ref) and for the device (ransac.hip): the two cannot drift apart.  Every step is stated here
// operation by operation; the tests restate it from this comment.  The discipline is that of ransac_rule.h: integer steps
// are uint32 / uint64 arithmetic; the fit is IEEE double, every operation rounded on its own in exactly the order written
// (the translation units that include this header are compiled with -ffp-contract=off: no fused multiply-add), and uses
// only + - * /, fabs and comparisons -- no square root, no library function -- so host and device agree bit for bit.
// There is no special case for a degenerate sample and the fit does not generally announce one with NaN (a duplicated
// point, or a pure 2-D translation, gives a finite matrix): whatever IEEE arithmetic gives is the result.
//
// INPUT.  As in ransac_rule.h: n pair records of 16 bytes of which the first two ints (left, right) are read, two
// position arrays, tol, hypotheses = N, seed.  Pair p is (xl, yl) = left_xy[pairs[p].left] -> (xr, yr) =
// right_xy[pairs[p].right].  The model m is the row-major F of  (xr yr 1) F (xl yl 1)^T = 0:  a PSX_GUIDE_EPIPOLAR matrix.
//
// 1. SAMPLES (integers only).  Step 1 of ransac_rule.h with EIGHT draws: mix(x) as there;  for hypothesis h:
//    base = mix(seed ^ (0x9e3779b9 * (h + 1)))  in uint32.  For k = 0..7:
//        r = mix(base + k);   idx = (uint64(r) * (n - k)) >> 32;
//        for every index c chosen before, taken in ASCENDING ORDER OF VALUE:  if idx >= c then idx++
//    Eight distinct pair indices in [0, n), in draw order (n >= 8).  (psx_ransac_sample_k<K> draws K of them; K = 4 gives
//    psx_ransac_sample's four.)
//
// 2. FIT of n >= 8 correspondences (x_i, y_i) -> (u_i, v_i), in the given order, in double (the float32 positions are
//    converted exactly).  Every sum below starts at 0.0 and adds its terms serially, i ascending.
//    a. Normalise each side on its own exactly as step 2a of ransac_rule.h (shown for the left):  cx = (sum x_i) / n;
//       cy = (sum y_i) / n;  d = sum (fabs(x_i - cx) + fabs(y_i - cy));  s = n / d;  point ((x_i - cx) * s, (y_i - cy) * s).
//       (cx_l, cy_l, s_l) and (cx_r, cy_r, s_r); from here on x, y, u, v are the NORMALISED coordinates.
//    b. Accumulate.  Correspondence i gives one row of 9 entries,
//           r = [u*x  u*y  u  v*x  v*y  v  x  y  1].
//       For each row, for i = 0..8:  for j = 0..i:  S[i][j] = S[i][j] + r[i] * r[j].     (45 sums, a lower triangle)
//    c. Pivoted LDL^T of the symmetric 9 x 9 matrix, 8 steps, right-looking (the diagonal is current when the pivot is
//       chosen).  perm starts as 0..8.  For j = 0..7, in this order:
//           pivot:     p = j;  for i = j+1..8:  if fabs(S[i][i]) > fabs(S[p][p]) then p = i      (ties and NaN stay low)
//           exchange:  rows and columns j <-> p of the symmetric matrix -- the finished columns 0..j-1 of the two rows go
//                      with them -- and perm[j] <-> perm[p]
//           for i = j+1..8:  l_i = S[i][j] / S[j][j]
//           for i = j+1..8:  for k = j+1..i:  S[i][k] = S[i][k] - l_i * S[k][j]          (S[k][j] is still undivided)
//           for i = j+1..8:  S[i][j] = l_i
//    d. Null vector.  q[8] = 1;  for i = 7..0:  q[i] = 0.0 - (sum over k = i+1..8, ascending, of S[k][i] * q[k]);
//       then Fn[perm[i]] = q[i], i = 0..8.  The entry fixed at 1 is whichever one the pivoting left over -- NOT always
//       F22: in the normalised frame F22 is the epipolar residual of the two centroids, exactly 0 for rectified stereo.
//    e. Rank correction, FOUR rounds, in the normalised frame: a Newton step on det F along its gradient, the cofactors.
//       With F = Fn, row major:
//           C0 = F4*F8 - F5*F7   C1 = F5*F6 - F3*F8   C2 = F3*F7 - F4*F6
//           C3 = F2*F7 - F1*F8   C4 = F0*F8 - F2*F6   C5 = F1*F6 - F0*F7
//           C6 = F1*F5 - F2*F4   C7 = F2*F3 - F0*F5   C8 = F0*F4 - F1*F3
//           det = (F0*C0 + F1*C1) + F2*C2;   nn = sum over k = 0..8, ascending, of C_k*C_k;   t = det / nn
//           F_k = F_k - t * C_k,  k = 0..8
//    f. Denormalise,  F = Tr^T Fn Tl.  For each row (a, b, c) of Fn:  A = a * s_l;  B = b * s_l;
//           G = (A, B, (c - A * cx_l) - B * cy_l).          With rows G0, G1, G2, entry by entry:
//           row 0 = G0 * s_r;   row 1 = G1 * s_r;   row 2 = (G2 - cx_r * row 0) - cy_r * row 1.
//    g. Round the nine doubles to float32 (round to nearest even).
//
// 3. SCORE.  count[h] = number of pairs p with psx_guide_pair(PSX_GUIDE_EPIPOLAR, m_h, tol, xl, yl, xr, yr)
//    (guide_rule.h, unchanged); 0 when m_h is not USABLE: any of its nine entries is NaN or +-inf, or all nine are zero
//    (the epipolar rule admits every pair under the zero matrix, 0 <= 0: such a model must never win).
// 4. SELECT.  The largest count; ties go to the lowest h.  count[best] is `sample_inliers`.
// 5. REFIT (PSX_RANSAC_REFIT), one round: when sample_inliers >= 8, fit (step 2) the winner's inliers in pair order and
//    score that model; it replaces the sample model iff it is usable and its count >= sample_inliers.
// 6. INLIERS.  The input records whose pair passes the rule under the kept model, in input order; their number is
//    `inliers`.  A kept model that is not usable is reported as "no model": best = -1, a zero matrix, no inliers -- as for
//    n < 8.
#pragma once

#include "ransac_rule.h"

#define PSX_FUND_MIN 8

// step 1 with K draws (K = 4: the indices of psx_ransac_sample).  s[] holds the indices chosen so far, ascending; every
// subscript is a compile-time constant once the loops are unrolled.
template <int K>
PSX_GUIDE_HD inline void psx_ransac_sample_k(uint32_t seed, int h, int n, int idx[K])
{
    const uint32_t base = psx_ransac_mix(seed ^ (0x9e3779b9u * ((uint32_t)h + 1u)));
    int s[K];
    PSX_RANSAC_UNROLL
    for (int k = 0; k < K; k++) {
        const uint32_t r = psx_ransac_mix(base + (uint32_t)k);
        int v = (int)(((uint64_t)r * (uint64_t)(uint32_t)(n - k)) >> 32);
        PSX_RANSAC_UNROLL
        for (int j = 0; j < K; j++)
            if (j < k && v >= s[j]) v++;
        idx[k] = v;
        int carry = v;                                // insert v: below it the list stays, above it everything moves up
        PSX_RANSAC_UNROLL
        for (int j = 0; j < K; j++)
            if (j < k) { const int lo = s[j] < carry ? s[j] : carry; carry = s[j] < carry ? carry : s[j]; s[j] = lo; }
        s[k] = carry;
    }
}

// usable (step 3): nine finite entries, not all of them zero
PSX_GUIDE_HD inline bool psx_fund_model_usable(const float* m)
{
    bool any = false;
    PSX_RANSAC_UNROLL
    for (int k = 0; k < 9; k++) any = any || (m[k] != 0.0f);
    return any && psx_ransac_model_finite(m);
}

// step 3 for one pair under a model already known to be usable
PSX_GUIDE_HD inline bool psx_fund_inlier(const float* m, float tol, const psx_ransac_pt& p)
{
    return psx_guide_right(PSX_GUIDE_EPIPOLAR, psx_guide_left(PSX_GUIDE_EPIPOLAR, m, tol, p.xl, p.yl), p.xr, p.yr);
}

// exchange a <-> b when sw: two selects, no branch and no run-time subscript
template <typename T>
PSX_GUIDE_HD inline void psx_fund_cswap(bool sw, T& a, T& b)
{
    const T x = a, y = b;
    a = sw ? y : x;
    b = sw ? x : y;
}

// step 2.  NFIX > 0: the number of correspondences is that compile-time constant (every loop unrolls: the device keeps the
// whole fit in registers); NFIX == 0: n of them.  free_index (may be NULL): the entry of Fn that step 2d fixed at 1.
template <int NFIX>
PSX_GUIDE_HD inline void psx_fundamental_fit_rule(const psx_ransac_pt* pt, int n_dyn, float m[9], int* free_index = nullptr)
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
    // b. the lower triangle of S (row i holds j = 0..i)
    double S[9][9];
    PSX_RANSAC_UNROLL
    for (int i = 0; i < 9; i++) {
        PSX_RANSAC_UNROLL
        for (int j = 0; j < 9; j++) S[i][j] = 0.0;
    }
    PSX_RANSAC_UNROLL_N
    for (int c = 0; c < n; c++) {
        const double x = ((double)pt[c].xl - cxl) * sl, y = ((double)pt[c].yl - cyl) * sl;
        const double u = ((double)pt[c].xr - cxr) * sr, v = ((double)pt[c].yr - cyr) * sr;
        const double r[9] = {u * x, u * y, u, v * x, v * y, v, x, y, 1.0};
        PSX_RANSAC_UNROLL
        for (int i = 0; i < 9; i++) {
            PSX_RANSAC_UNROLL
            for (int j = 0; j <= i; j++) S[i][j] = S[i][j] + r[i] * r[j];
        }
    }
    // c. pivoted LDL^T in place: l_i replaces S[i][j], the diagonal keeps D.  The exchange is written as compare-and-select
    // over compile-time indices: a run-time subscript would send the 45 doubles to scratch on the device.
    int perm[9];
    PSX_RANSAC_UNROLL
    for (int i = 0; i < 9; i++) perm[i] = i;
    PSX_RANSAC_UNROLL
    for (int j = 0; j < 8; j++) {
        int p = j;
        double big = fabs(S[j][j]);                    // fabs(S[p][p])
        PSX_RANSAC_UNROLL
        for (int i = j + 1; i < 9; i++) {
            const double a = fabs(S[i][i]);
            if (a > big) { big = a; p = i; }
        }
        PSX_RANSAC_UNROLL
        for (int c = j + 1; c < 9; c++) {              // the candidate c is a constant; at most one of them is p
            const bool sw = p == c;
            psx_fund_cswap(sw, perm[j], perm[c]);
            PSX_RANSAC_UNROLL
            for (int k = 0; k < j; k++) psx_fund_cswap(sw, S[j][k], S[c][k]);          // the finished columns
            psx_fund_cswap(sw, S[j][j], S[c][c]);
            PSX_RANSAC_UNROLL
            for (int k = j + 1; k < c; k++) psx_fund_cswap(sw, S[k][j], S[c][k]);      // between the two: column j <-> row c
            PSX_RANSAC_UNROLL
            for (int k = c + 1; k < 9; k++) psx_fund_cswap(sw, S[k][j], S[k][c]);      // below both: column j <-> column c
        }
        double l[9];
        PSX_RANSAC_UNROLL
        for (int i = j + 1; i < 9; i++) l[i] = S[i][j] / S[j][j];
        PSX_RANSAC_UNROLL
        for (int i = j + 1; i < 9; i++) {
            PSX_RANSAC_UNROLL
            for (int k = j + 1; k <= i; k++) S[i][k] = S[i][k] - l[i] * S[k][j];
        }
        PSX_RANSAC_UNROLL
        for (int i = j + 1; i < 9; i++) S[i][j] = l[i];
    }
    // d. the null vector of the permuted matrix, then back through perm
    double q[9];
    q[8] = 1.0;
    PSX_RANSAC_UNROLL
    for (int i = 7; i >= 0; i--) {
        double t = 0.0;
        PSX_RANSAC_UNROLL
        for (int k = i + 1; k < 9; k++) t = t + S[k][i] * q[k];
        q[i] = 0.0 - t;
    }
    double F[9];
    PSX_RANSAC_UNROLL
    for (int k = 0; k < 9; k++) {
        double f = 0.0;
        PSX_RANSAC_UNROLL
        for (int i = 0; i < 9; i++) f = perm[i] == k ? q[i] : f;                      // perm is a permutation: exactly one i
        F[k] = f;
    }
    if (free_index) *free_index = perm[8];
    // e. four Newton steps on the determinant along its gradient
    PSX_RANSAC_UNROLL
    for (int round = 0; round < 4; round++) {
        const double C[9] = {F[4] * F[8] - F[5] * F[7], F[5] * F[6] - F[3] * F[8], F[3] * F[7] - F[4] * F[6],
                             F[2] * F[7] - F[1] * F[8], F[0] * F[8] - F[2] * F[6], F[1] * F[6] - F[0] * F[7],
                             F[1] * F[5] - F[2] * F[4], F[2] * F[3] - F[0] * F[5], F[0] * F[4] - F[1] * F[3]};
        const double det = (F[0] * C[0] + F[1] * C[1]) + F[2] * C[2];
        double nn = 0.0;
        PSX_RANSAC_UNROLL
        for (int k = 0; k < 9; k++) nn = nn + C[k] * C[k];
        const double t = det / nn;
        PSX_RANSAC_UNROLL
        for (int k = 0; k < 9; k++) F[k] = F[k] - t * C[k];
    }
    // f, g. denormalise and round
    double G[9];
    PSX_RANSAC_UNROLL
    for (int r = 0; r < 3; r++) {
        const double A = F[3 * r] * sl, B = F[3 * r + 1] * sl;
        G[3 * r] = A; G[3 * r + 1] = B;
        G[3 * r + 2] = (F[3 * r + 2] - A * cxl) - B * cyl;
    }
    PSX_RANSAC_UNROLL
    for (int k = 0; k < 3; k++) {
        const double row0 = G[k] * sr, row1 = G[3 + k] * sr;
        m[k] = (float)row0;
        m[3 + k] = (float)row1;
        m[6 + k] = (float)((G[6 + k] - cxr * row0) - cyr * row1);
    }
}

// score of one model over n correspondences (step 3)
inline int psx_fund_count(const float* m, float tol, const psx_ransac_pt* pt, int n)
{
    if (!psx_fund_model_usable(m)) return 0;
    int c = 0;
    for (int p = 0; p < n; p++) c += psx_fund_inlier(m, tol, pt[p]) ? 1 : 0;
    return c;
}

// The whole rule on host arrays (psx_ransac_fundamental_ref); arguments, passes and `scratch` (n psx_ransac_pt, the
// caller's) as psx_ransac_homography_host.  models (N x 9) and counts (N) may be NULL.
inline int psx_ransac_fundamental_host(const void* pairs, int n, const float* left_xy, int nl, const float* right_xy, int nr,
                                       const psx_ransac_opts* opts, psx_ransac_result* result, void* inliers, int capacity,
                                       int* count, float* models, int* counts, psx_ransac_pt* scratch)
{
    if (!psx_ransac_opts_ok(opts) || result == nullptr || count == nullptr || n < 0 || nl < 0 || nr < 0 || capacity < 0) return PSX_ERR_INVALID;
    if ((n > 0 && pairs == nullptr) || (nl > 0 && left_xy == nullptr) || (nr > 0 && right_xy == nullptr)) return PSX_ERR_INVALID;
    if ((capacity > 0 && inliers == nullptr) || (n >= PSX_FUND_MIN && scratch == nullptr)) return PSX_ERR_INVALID;
    const int* rec = static_cast<const int*>(pairs);                             // 4 ints per record: left, right, two distances
    for (int p = 0; p < n; p++)
        if (rec[4 * (size_t)p] < 0 || rec[4 * (size_t)p] >= nl || rec[4 * (size_t)p + 1] < 0 || rec[4 * (size_t)p + 1] >= nr)
            return PSX_ERR_INVALID;
    if (n < PSX_FUND_MIN) { psx_ransac_no_model(result); *count = 0; return PSX_OK; }
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
        int idx[PSX_FUND_MIN];
        psx_ransac_sample_k<PSX_FUND_MIN>(opts->seed, h, n, idx);
        psx_ransac_pt q[PSX_FUND_MIN];
        for (int k = 0; k < PSX_FUND_MIN; k++) q[k] = scratch[idx[k]];
        float m[9];
        psx_fundamental_fit_rule<PSX_FUND_MIN>(q, PSX_FUND_MIN, m);
        const int c = psx_fund_count(m, tol, scratch, n);
        if (models) for (int k = 0; k < 9; k++) models[9 * (size_t)h + k] = m[k];
        if (counts) counts[h] = c;
        if (c > best_count) { best_count = c; best = h; for (int k = 0; k < 9; k++) kept[k] = m[k]; }
    }
    int refit_kept = 0;
    if ((opts->flags & PSX_RANSAC_REFIT) != 0 && best_count >= PSX_FUND_MIN) {
        // the winner's inliers in pair order, packed behind one another in a buffer of their own
        psx_ransac_pt* in = new psx_ransac_pt[(size_t)best_count];
        int k = 0;
        for (int p = 0; p < n; p++)
            if (psx_fund_inlier(kept, tol, scratch[p])) in[k++] = scratch[p];
        float m[9];
        psx_fundamental_fit_rule<0>(in, best_count, m);
        delete[] in;
        const int c = psx_fund_count(m, tol, scratch, n);
        if (psx_fund_model_usable(m) && c >= best_count) {
            for (int j = 0; j < 9; j++) kept[j] = m[j];
            refit_kept = 1;
        }
    }
    if (!psx_fund_model_usable(kept)) { psx_ransac_no_model(result); *count = 0; return PSX_OK; }
    int w = 0;
    for (int p = 0; p < n; p++) {
        if (!psx_fund_inlier(kept, tol, scratch[p])) continue;
        if (w < capacity) for (int j = 0; j < 4; j++) static_cast<int*>(inliers)[4 * (size_t)w + j] = rec[4 * (size_t)p + j];
        w++;
    }
    for (int k = 0; k < 9; k++) result->m[k] = kept[k];
    result->best = best; result->sample_inliers = best_count; result->inliers = w; result->refit_kept = refit_kept;
    *count = w;
    return PSX_OK;
}
