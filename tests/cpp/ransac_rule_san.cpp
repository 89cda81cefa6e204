// A stand-alone program (its own main) over csrc/hip/ransac_rule.h alone: the host form of the homography RANSAC on
// exact-size heap arrays, for a build with -fsanitize=address,undefined (tests/test_ransac_cpu.py compiles and runs it).
// Never loaded into Python, never run on a GPU.
#include "ransac_rule.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

static int failures = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); failures++; } } while (0)

static unsigned lcg_state = 12345u;
static float unit() { lcg_state = lcg_state * 1664525u + 1013904223u; return (float)(lcg_state >> 8) / 16777216.0f; }

static const float H[9] = {1.25f, 0.03f, 4.0f, -0.02f, 1.2f, -3.0f, 1e-4f, -5e-5f, 1.0f};

static void apply(float x, float y, float* u, float* v)
{
    const double c = H[6] * (double)x + H[7] * (double)y + H[8];
    *u = (float)((H[0] * (double)x + H[1] * (double)y + H[2]) / c);
    *v = (float)((H[3] * (double)x + H[4] * (double)y + H[5]) / c);
}

// n pairs; every pair with p % 5 >= 3 is an outlier (n > 4); records index the arrays in reverse
static void run_case(int n, int N, unsigned seed, int flags)
{
    psx_match_pair* pairs = new psx_match_pair[(size_t)n];
    float* lxy = new float[2 * (size_t)n];
    float* rxy = new float[2 * (size_t)n];
    int planted = 0;
    for (int p = 0; p < n; p++) {
        const int l = n - 1 - p, r = p;
        lxy[2 * l] = 640.0f * unit(); lxy[2 * l + 1] = 480.0f * unit();
        if (n > 4 && p % 5 >= 3) { rxy[2 * r] = 800.0f * unit(); rxy[2 * r + 1] = 560.0f * unit(); }
        else { apply(lxy[2 * l], lxy[2 * l + 1], &rxy[2 * r], &rxy[2 * r + 1]); rxy[2 * r] += 0.25f; planted++; }
        pairs[p].left = l; pairs[p].right = r; pairs[p].d1 = (float)p; pairs[p].d2 = (float)(2 * p);
    }
    psx_ransac_opts o = {2.0f, N, seed, flags};
    psx_ransac_result res;
    int count = -1;
    float* models = new float[9 * (size_t)N];
    int* counts = new int[(size_t)N];
    psx_ransac_pt* scratch = n >= 4 ? new psx_ransac_pt[(size_t)n] : nullptr;
    // "how many?" first, then the exact capacity
    CHECK(psx_ransac_homography_host(pairs, n, lxy, n, rxy, n, &o, &res, nullptr, 0, &count, models, counts, scratch) == PSX_OK);
    const int total = count;
    psx_match_pair* inl = new psx_match_pair[(size_t)(total > 0 ? total : 1)];
    CHECK(psx_ransac_homography_host(pairs, n, lxy, n, rxy, n, &o, &res, inl, total, &count, nullptr, nullptr, scratch) == PSX_OK);
    CHECK(count == total && res.inliers == total);
    if (n < 4) CHECK(res.best == -1 && total == 0);
    else {
        CHECK(res.best >= 0 && res.best < N && counts[res.best] == res.sample_inliers);
        for (int h = 0; h < N; h++) CHECK(counts[h] <= res.sample_inliers && (counts[h] < res.sample_inliers || h >= res.best));
        if (n >= 60) CHECK(total >= planted - 2 && total <= planted + 2);
        for (int k = 0; k < total; k++) {
            CHECK(k == 0 || inl[k].d1 > inl[k - 1].d1);                       // input order
            const psx_ransac_pt pt = {lxy[2 * inl[k].left], lxy[2 * inl[k].left + 1], rxy[2 * inl[k].right], rxy[2 * inl[k].right + 1]};
            CHECK(psx_ransac_inlier(res.m, o.tol, pt));
        }
    }
    // an index outside its array: refused, nothing written
    if (n >= 1) {
        psx_ransac_result keep; memset(&keep, 0x5a, sizeof keep);
        psx_ransac_result r2 = keep;
        int c2 = -77;
        pairs[n / 2].right = n;
        CHECK(psx_ransac_homography_host(pairs, n, lxy, n, rxy, n, &o, &r2, inl, total, &c2, nullptr, nullptr, scratch) == PSX_ERR_INVALID);
        CHECK(c2 == -77 && memcmp(&r2, &keep, sizeof keep) == 0);
    }
    delete[] pairs; delete[] lxy; delete[] rxy; delete[] models; delete[] counts; delete[] scratch; delete[] inl;
}

int main()
{
    // samples: four distinct indices in range, for the smallest n and a large one
    const int ns[3] = {4, 5, 1000};
    for (int t = 0; t < 3; t++)
        for (int h = 0; h < 65536; h += (t == 2 ? 7 : 1)) {
            int* idx = new int[4];
            psx_ransac_sample(99u + (unsigned)t, h, ns[t], idx);
            for (int a = 0; a < 4; a++) {
                CHECK(idx[a] >= 0 && idx[a] < ns[t]);
                for (int b = 0; b < a; b++) CHECK(idx[a] != idx[b]);
            }
            delete[] idx;
        }
    // the fit: an exact model from four and from twelve exact correspondences; degenerate inputs give non-finite entries
    for (int n = 4; n <= 12; n += 8) {
        psx_ransac_pt* pt = new psx_ransac_pt[(size_t)n];
        for (int i = 0; i < n; i++) { pt[i].xl = 640.0f * unit(); pt[i].yl = 480.0f * unit(); apply(pt[i].xl, pt[i].yl, &pt[i].xr, &pt[i].yr); }
        float* m = new float[9];
        if (n == 4) psx_homography_fit_rule<4>(pt, 4, m); else psx_homography_fit_rule<0>(pt, n, m);
        CHECK(psx_ransac_model_finite(m));
        for (int k = 0; k < 9; k++) CHECK(std::fabs(m[k] / m[8] - H[k]) <= 2e-3f * (std::fabs(H[k]) + 1e-3f));
        for (int i = 0; i < n; i++) CHECK(psx_ransac_inlier(m, 0.05f, pt[i]));
        for (int i = 0; i < n; i++) { pt[i].xl = 7.0f; pt[i].yl = 9.0f; }       // coincident left points
        if (n == 4) psx_homography_fit_rule<4>(pt, 4, m); else psx_homography_fit_rule<0>(pt, n, m);
        CHECK(!psx_ransac_model_finite(m));
        for (int i = 0; i < n; i++) { pt[i].xl = (float)i; pt[i].yl = 2.0f * i; pt[i].xr = 3.0f * i; pt[i].yr = (float)i; }   // collinear
        if (n == 4) psx_homography_fit_rule<4>(pt, 4, m); else psx_homography_fit_rule<0>(pt, n, m);
        CHECK(!psx_ransac_model_finite(m));
        delete[] pt; delete[] m;
    }
    const int shapes[8][2] = {{0, 8}, {3, 8}, {4, 8}, {5, 64}, {63, 64}, {65, 64}, {129, 128}, {300, 256}};
    for (int s = 0; s < 8; s++)
        for (int flags = 0; flags <= 1; flags++) run_case(shapes[s][0], shapes[s][1], 17u + (unsigned)s, flags);
    // option errors
    psx_ransac_opts bad[5] = {{-1.0f, 8, 0u, 0}, {NAN, 8, 0u, 0}, {INFINITY, 8, 0u, 0}, {2.0f, 0, 0u, 0}, {2.0f, 8, 0u, 2}};
    for (int k = 0; k < 5; k++) CHECK(!psx_ransac_opts_ok(&bad[k]));
    psx_ransac_opts big = {0.0f, 65536, 0u, 1};
    CHECK(psx_ransac_opts_ok(&big));
    big.hypotheses = 65537;
    CHECK(!psx_ransac_opts_ok(&big));
    if (failures) { printf("%d FAILURES\n", failures); return 1; }
    printf("ALL OK\n");
    return 0;
}
