// A stand-alone program (its own main) over csrc/hip/affine_rule.h alone: the host form of the affine and similarity
// RANSAC on exact-size heap arrays, for a build with -fsanitize=address,undefined (tests/test_affine_cpu.py compiles and
// runs it).  Never loaded into Python, never run on a GPU.
#include "affine_rule.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

static int failures = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); failures++; } } while (0)

static unsigned lcg_state = 12345u;
static float unit() { lcg_state = lcg_state * 1664525u + 1013904223u; return (float)(lcg_state >> 8) / 16777216.0f; }

// the planted transforms: a similarity (rotation 0.3 rad, scale 1.2) and a sheared affine map
static void plant(bool similarity, float x, float y, float* u, float* v)
{
    if (similarity) {
        const double c = 1.2 * std::cos(0.3), s = 1.2 * std::sin(0.3);
        *u = (float)(c * x - s * y + 25.0); *v = (float)(s * x + c * y - 14.0);
    } else {
        *u = (float)(1.15 * x + 0.32 * y - 20.0); *v = (float)(-0.08 * x + 0.9 * y + 31.0);
    }
}

static double transfer_error(const float* m, const psx_ransac_pt& p)
{
    const double a = (double)m[0] * p.xl + (double)m[1] * p.yl + m[2], b = (double)m[3] * p.xl + (double)m[4] * p.yl + m[5];
    return std::hypot(a - p.xr, b - p.yr);
}

template <int MIN>
static void fit(const psx_ransac_pt* pt, int n, float* m)
{
    if (n == MIN) psx_affine_fit_by_min<MIN, MIN>(pt, n, m); else psx_affine_fit_by_min<MIN, 0>(pt, n, m);
}

// n pairs; every pair with p % 5 >= 3 is an outlier (n > 4); with `shared` every pair with p % 4 == 1 has the left point of
// the pair before it; records index the arrays in reverse
template <int MIN>
static void run_case(int n, int N, unsigned seed, int flags, bool shared)
{
    const auto rule = psx_ransac_host_rule(MIN == PSX_SIMILARITY_MIN ? PSX_RANSAC_MODEL_SIMILARITY : PSX_RANSAC_MODEL_AFFINE);
    CHECK(psx_ransac_host_min(MIN == PSX_SIMILARITY_MIN ? PSX_RANSAC_MODEL_SIMILARITY : PSX_RANSAC_MODEL_AFFINE) == MIN);
    psx_match_pair* pairs = new psx_match_pair[(size_t)n];
    float* lxy = new float[2 * (size_t)n];
    float* rxy = new float[2 * (size_t)n];
    for (int p = 0; p < n; p++) {
        const int l = n - 1 - p, r = p;
        lxy[2 * l] = 640.0f * unit(); lxy[2 * l + 1] = 480.0f * unit();
        if (shared && p % 4 == 1) { lxy[2 * l] = lxy[2 * (l + 1)]; lxy[2 * l + 1] = lxy[2 * (l + 1) + 1]; }
        if (n > 4 && p % 5 >= 3) { rxy[2 * r] = 800.0f * unit(); rxy[2 * r + 1] = 700.0f * unit(); }
        else plant(MIN == PSX_SIMILARITY_MIN, lxy[2 * l], lxy[2 * l + 1], &rxy[2 * r], &rxy[2 * r + 1]);
        pairs[p].left = l; pairs[p].right = r; pairs[p].d1 = (float)p; pairs[p].d2 = (float)(2 * p);
    }
    psx_ransac_opts o = {2.0f, N, seed, flags};
    psx_ransac_result res;
    int count = -1;
    float* models = new float[9 * (size_t)N];
    int* counts = new int[(size_t)N];
    psx_ransac_pt* scratch = n >= MIN ? new psx_ransac_pt[(size_t)n] : nullptr;
    // "how many?" first, then the exact capacity
    CHECK(rule(pairs, n, lxy, n, rxy, n, &o, &res, nullptr, 0, &count, models, counts, scratch) == PSX_OK);
    const int total = count;
    psx_match_pair* inl = new psx_match_pair[(size_t)(total > 0 ? total : 1)];
    CHECK(rule(pairs, n, lxy, n, rxy, n, &o, &res, inl, total, &count, nullptr, nullptr, scratch) == PSX_OK);
    CHECK(count == total && res.inliers == total);
    if (n < MIN) CHECK(res.best == -1 && total == 0);
    else if (res.best >= 0) {
        CHECK(res.best < N && counts[res.best] == res.sample_inliers);
        CHECK(res.m[6] == 0.0f && res.m[7] == 0.0f && res.m[8] == 1.0f && psx_ransac_model_finite(res.m));
        for (int h = 0; h < N; h++) CHECK(counts[h] <= res.sample_inliers && (counts[h] < res.sample_inliers || h >= res.best));
        for (int k = 0; k < total; k++) {
            CHECK(k == 0 || inl[k].d1 > inl[k - 1].d1);                       // input order
            const psx_ransac_pt pt = {lxy[2 * inl[k].left], lxy[2 * inl[k].left + 1], rxy[2 * inl[k].right], rxy[2 * inl[k].right + 1]};
            CHECK(psx_ransac_inlier(res.m, o.tol, pt));
        }
    } else {
        CHECK(shared && total == 0);                                           // every sample degenerate
        for (int k = 0; k < 9; k++) CHECK(res.m[k] == 0.0f);
    }
    // an index outside its array: refused, nothing written
    if (n >= 1) {
        psx_ransac_result keep; memset(&keep, 0x5a, sizeof keep);
        psx_ransac_result r2 = keep;
        int c2 = -77;
        pairs[n / 2].right = n;
        CHECK(rule(pairs, n, lxy, n, rxy, n, &o, &r2, inl, total, &c2, nullptr, nullptr, scratch) == PSX_ERR_INVALID);
        CHECK(c2 == -77 && memcmp(&r2, &keep, sizeof keep) == 0);
    }
    delete[] pairs; delete[] lxy; delete[] rxy; delete[] models; delete[] counts; delete[] scratch; delete[] inl;
}

template <int MIN>
static void fits()
{
    // exact correspondences come back, from MIN (constant trip counts) and from twenty (dynamic n)
    for (int n = MIN; n <= 20; n += 20 - MIN) {
        psx_ransac_pt* pt = new psx_ransac_pt[(size_t)n];
        for (int i = 0; i < n; i++) { pt[i].xl = 640.0f * unit(); pt[i].yl = 480.0f * unit(); plant(MIN == PSX_SIMILARITY_MIN, pt[i].xl, pt[i].yl, &pt[i].xr, &pt[i].yr); }
        float* m = new float[9];
        fit<MIN>(pt, n, m);
        CHECK(psx_ransac_model_finite(m) && m[6] == 0.0f && m[7] == 0.0f && m[8] == 1.0f);
        for (int i = 0; i < n; i++) CHECK(transfer_error(m, pt[i]) < 0.01);
        for (int i = 0; i < n; i++) CHECK(psx_ransac_inlier(m, 0.05f, pt[i]));
        // a duplicated point: no special case, no trap; whatever comes out scores or does not
        pt[1] = pt[0];
        fit<MIN>(pt, n, m);
        CHECK(psx_ransac_count(m, 2.0f, pt, n) >= 0);
        if (n == PSX_SIMILARITY_MIN) CHECK(!psx_ransac_model_finite(m));                  // d = 0: NaN
        // a left side of zero extent: n / 0, NaN all the way
        for (int i = 0; i < n; i++) { pt[i].xl = 7.0f; pt[i].yl = 9.0f; }
        fit<MIN>(pt, n, m);
        CHECK(!psx_ransac_model_finite(m) && psx_ransac_count(m, 2.0f, pt, n) == 0);
        // collinear left points: a zero pivot for the affine fit, an ordinary input for the similarity
        for (int i = 0; i < n; i++) { pt[i].xl = 10.0f * (float)i; pt[i].yl = 20.0f * (float)i; plant(MIN == PSX_SIMILARITY_MIN, pt[i].xl, pt[i].yl, &pt[i].xr, &pt[i].yr); }
        fit<MIN>(pt, n, m);
        CHECK(psx_ransac_count(m, 2.0f, pt, n) >= 0);
        if (MIN == PSX_SIMILARITY_MIN) CHECK(psx_ransac_model_finite(m));
        delete[] pt; delete[] m;
    }
}

int main()
{
    // samples: two and three distinct indices in range, the first draws of psx_ransac_sample's four
    const int ns[3] = {3, 4, 1000};
    for (int t = 0; t < 3; t++)
        for (int h = 0; h < 65536; h += (t == 2 ? 7 : 1)) {
            int* i2 = new int[2];
            int* i3 = new int[3];
            psx_ransac_sample_k<2>(99u + (unsigned)t, h, ns[t], i2);
            psx_ransac_sample_k<3>(99u + (unsigned)t, h, ns[t], i3);
            CHECK(i2[0] >= 0 && i2[0] < ns[t] && i2[1] >= 0 && i2[1] < ns[t] && i2[0] != i2[1]);
            CHECK(i3[2] >= 0 && i3[2] < ns[t] && i3[2] != i3[0] && i3[2] != i3[1] && memcmp(i2, i3, 2 * sizeof(int)) == 0);
            if (ns[t] >= 4) {
                int* j4 = new int[4];
                psx_ransac_sample(99u + (unsigned)t, h, ns[t], j4);
                CHECK(memcmp(i3, j4, 3 * sizeof(int)) == 0);
                delete[] j4;
            }
            delete[] i2; delete[] i3;
        }
    fits<PSX_SIMILARITY_MIN>();
    fits<PSX_AFFINE_MIN>();
    // the smallest shapes of each model, the degenerate ones included, and a few larger ones
    const int shapes[9][2] = {{0, 8}, {1, 8}, {2, 8}, {3, 8}, {4, 64}, {5, 64}, {65, 64}, {129, 128}, {300, 256}};
    for (int s = 0; s < 9; s++)
        for (int flags = 0; flags <= 1; flags++)
            for (int shared = 0; shared <= 1; shared++) {
                run_case<PSX_SIMILARITY_MIN>(shapes[s][0], shapes[s][1], 17u + (unsigned)s, flags, shared != 0);
                run_case<PSX_AFFINE_MIN>(shapes[s][0], shapes[s][1], 17u + (unsigned)s, flags, shared != 0);
            }
    if (failures) { printf("%d FAILURES\n", failures); return 1; }
    printf("ALL OK\n");
    return 0;
}
