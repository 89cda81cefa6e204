// A stand-alone program (its own main) over csrc/hip/fundamental_rule.h alone: the host form of the fundamental-matrix
// RANSAC on exact-size heap arrays, for a build with -fsanitize=address,undefined (tests/test_fundamental_cpu.py compiles
// and runs it).  Never loaded into Python, never run on a GPU.
#include "fundamental_rule.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

static int failures = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); failures++; } } while (0)

static unsigned lcg_state = 12345u;
static float unit() { lcg_state = lcg_state * 1664525u + 1013904223u; return (float)(lcg_state >> 8) / 16777216.0f; }

// a left point at depth z seen by a second camera: K = (500, 500, 320, 240), rotation 0.15 rad about y, t = (-1, 0.1, 0.2)
static void project(float x, float y, float z, float* u, float* v)
{
    const double X = ((double)x - 320.0) / 500.0 * z, Y = ((double)y - 240.0) / 500.0 * z, Z = z;
    const double c = std::cos(0.15), s = std::sin(0.15);
    const double xr = c * X + s * Z - 1.0, yr = Y + 0.1, zr = -s * X + c * Z + 0.2;
    *u = (float)(500.0 * xr / zr + 320.0);
    *v = (float)(500.0 * yr / zr + 240.0);
}

// distance of the right point from the line of the left point, in double
static double line_distance(const float* m, const psx_ransac_pt& p)
{
    const double a = (double)m[0] * p.xl + (double)m[1] * p.yl + m[2], b = (double)m[3] * p.xl + (double)m[4] * p.yl + m[5];
    const double c = (double)m[6] * p.xl + (double)m[7] * p.yl + m[8];
    return std::fabs(a * p.xr + b * p.yr + c) / std::sqrt(a * a + b * b);
}

// n pairs; every pair with p % 5 >= 3 is an outlier (n > 8); records index the arrays in reverse
static void run_case(int n, int N, unsigned seed, int flags)
{
    psx_match_pair* pairs = new psx_match_pair[(size_t)n];
    float* lxy = new float[2 * (size_t)n];
    float* rxy = new float[2 * (size_t)n];
    int planted = 0;
    for (int p = 0; p < n; p++) {
        const int l = n - 1 - p, r = p;
        lxy[2 * l] = 640.0f * unit(); lxy[2 * l + 1] = 480.0f * unit();
        if (n > 8 && p % 5 >= 3) { rxy[2 * r] = 640.0f * unit(); rxy[2 * r + 1] = 480.0f * unit(); }
        else { project(lxy[2 * l], lxy[2 * l + 1], 3.0f + 6.0f * unit(), &rxy[2 * r], &rxy[2 * r + 1]); planted++; }
        pairs[p].left = l; pairs[p].right = r; pairs[p].d1 = (float)p; pairs[p].d2 = (float)(2 * p);
    }
    psx_ransac_opts o = {2.0f, N, seed, flags};
    psx_ransac_result res;
    int count = -1;
    float* models = new float[9 * (size_t)N];
    int* counts = new int[(size_t)N];
    psx_ransac_pt* scratch = n >= 8 ? new psx_ransac_pt[(size_t)n] : nullptr;
    // "how many?" first, then the exact capacity
    CHECK(psx_ransac_fundamental_host(pairs, n, lxy, n, rxy, n, &o, &res, nullptr, 0, &count, models, counts, scratch) == PSX_OK);
    const int total = count;
    psx_match_pair* inl = new psx_match_pair[(size_t)(total > 0 ? total : 1)];
    CHECK(psx_ransac_fundamental_host(pairs, n, lxy, n, rxy, n, &o, &res, inl, total, &count, nullptr, nullptr, scratch) == PSX_OK);
    CHECK(count == total && res.inliers == total);
    if (n < 8) CHECK(res.best == -1 && total == 0);
    else {
        CHECK(res.best >= 0 && res.best < N && counts[res.best] == res.sample_inliers);
        for (int h = 0; h < N; h++) CHECK(counts[h] <= res.sample_inliers && (counts[h] < res.sample_inliers || h >= res.best));
        for (int k = 0; k < total; k++) {
            CHECK(k == 0 || inl[k].d1 > inl[k - 1].d1);                       // input order
            const psx_ransac_pt pt = {lxy[2 * inl[k].left], lxy[2 * inl[k].left + 1], rxy[2 * inl[k].right], rxy[2 * inl[k].right + 1]};
            CHECK(psx_fund_inlier(res.m, o.tol, pt));
        }
    }
    // an index outside its array: refused, nothing written
    if (n >= 1) {
        psx_ransac_result keep; memset(&keep, 0x5a, sizeof keep);
        psx_ransac_result r2 = keep;
        int c2 = -77;
        pairs[n / 2].right = n;
        CHECK(psx_ransac_fundamental_host(pairs, n, lxy, n, rxy, n, &o, &r2, inl, total, &c2, nullptr, nullptr, scratch) == PSX_ERR_INVALID);
        CHECK(c2 == -77 && memcmp(&r2, &keep, sizeof keep) == 0);
    }
    delete[] pairs; delete[] lxy; delete[] rxy; delete[] models; delete[] counts; delete[] scratch; delete[] inl;
}

int main()
{
    // samples: eight distinct indices in range, for the smallest n and a large one; four draws are psx_ransac_sample's
    const int ns[3] = {8, 9, 1000};
    for (int t = 0; t < 3; t++)
        for (int h = 0; h < 65536; h += (t == 2 ? 7 : 1)) {
            int* idx = new int[8];
            psx_ransac_sample_k<8>(99u + (unsigned)t, h, ns[t], idx);
            for (int a = 0; a < 8; a++) {
                CHECK(idx[a] >= 0 && idx[a] < ns[t]);
                for (int b = 0; b < a; b++) CHECK(idx[a] != idx[b]);
            }
            int* i4 = new int[4];
            int* j4 = new int[4];
            psx_ransac_sample_k<4>(99u + (unsigned)t, h, ns[t], i4);
            psx_ransac_sample(99u + (unsigned)t, h, ns[t], j4);
            CHECK(memcmp(i4, j4, 4 * sizeof(int)) == 0);
            delete[] idx; delete[] i4; delete[] j4;
        }
    // the fit: exact correspondences lie on their lines, from eight (constant trip counts) and from twenty (dynamic n)
    for (int n = 8; n <= 20; n += 12) {
        psx_ransac_pt* pt = new psx_ransac_pt[(size_t)n];
        for (int i = 0; i < n; i++) { pt[i].xl = 640.0f * unit(); pt[i].yl = 480.0f * unit(); project(pt[i].xl, pt[i].yl, 3.0f + 6.0f * unit(), &pt[i].xr, &pt[i].yr); }
        float* m = new float[9];
        int free_index = -1;
        if (n == 8) psx_fundamental_fit_rule<8>(pt, 8, m, &free_index); else psx_fundamental_fit_rule<0>(pt, n, m, &free_index);
        CHECK(psx_fund_model_usable(m) && free_index >= 0 && free_index <= 8);
        for (int i = 0; i < n; i++) CHECK(line_distance(m, pt[i]) < 0.01);
        for (int i = 0; i < n; i++) CHECK(psx_fund_inlier(m, 0.05f, pt[i]));
        // a duplicated point, then a side of zero extent: no special case, no trap; whatever comes out scores or does not
        pt[1] = pt[0];
        if (n == 8) psx_fundamental_fit_rule<8>(pt, 8, m); else psx_fundamental_fit_rule<0>(pt, n, m);
        CHECK(psx_fund_count(m, 2.0f, pt, n) >= 0);
        for (int i = 0; i < n; i++) { pt[i].xl = 7.0f; pt[i].yl = 9.0f; }
        if (n == 8) psx_fundamental_fit_rule<8>(pt, 8, m); else psx_fundamental_fit_rule<0>(pt, n, m);
        CHECK(!psx_fund_model_usable(m) && psx_fund_count(m, 2.0f, pt, n) == 0);          // n / 0: NaN all the way
        delete[] pt; delete[] m;
    }
    // the zero matrix and non-finite matrices may not score
    {
        psx_ransac_pt* pt = new psx_ransac_pt[3];
        for (int i = 0; i < 3; i++) { pt[i].xl = pt[i].yl = pt[i].xr = pt[i].yr = (float)i; }
        float* m = new float[9];
        for (int k = 0; k < 9; k++) m[k] = 0.0f;
        CHECK(psx_fund_inlier(m, 2.0f, pt[1]) && psx_fund_count(m, 2.0f, pt, 3) == 0);   // 0 <= 0 admits; the count refuses
        m[4] = -0.0f;
        CHECK(psx_fund_count(m, 2.0f, pt, 3) == 0);
        m[4] = INFINITY;
        CHECK(psx_fund_count(m, 2.0f, pt, 3) == 0);
        m[4] = NAN;
        CHECK(psx_fund_count(m, 2.0f, pt, 3) == 0);
        delete[] pt; delete[] m;
    }
    const int shapes[8][2] = {{0, 8}, {7, 8}, {8, 8}, {9, 64}, {63, 64}, {65, 64}, {129, 128}, {300, 256}};
    for (int s = 0; s < 8; s++)
        for (int flags = 0; flags <= 1; flags++) run_case(shapes[s][0], shapes[s][1], 17u + (unsigned)s, flags);
    if (failures) { printf("%d FAILURES\n", failures); return 1; }
    printf("ALL OK\n");
    return 0;
}
