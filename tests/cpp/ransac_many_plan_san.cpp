// Stand-alone program (its own main, no library): the host side of the batched geometric verification --
// csrc/hip/ransac_many_plan.h and the host rule headers it includes, nothing else -- built with -ffp-contract=off
// -fsanitize=address,undefined by tests/test_ransac_many_cpu.py and run directly.  Never loaded into Python, never run on
// a GPU.  Every array is a heap array of the exact size, so a read or write past an end is the sanitizer's to report:
//   - the plan at both block sizes the library uses, and at every smaller capacity: every pair of every set at or above
//     the minimum covered exactly once, nothing spanning two sets, a set's blocks ascending and contiguous, smaller sets
//     absent;
//   - a three-set host reference (one set below the minimum in the middle) against the loop of the single-list host rule,
//     at the full capacity, at total - 1, at 0 with a NULL output; a bad index in the last set refuses the whole call
//     with nothing written.
#include "ransac_many_plan.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

static int fails = 0;
#define CHECK(c) do { if(!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); fails++; } } while(0)

static void check_plan( const std::vector<int>& counts, int min_pairs, int rows )
{
    const int K = (int)counts.size();
    int nb = -1;
    CHECK( psx_ransac_many_plan_host( K ? counts.data() : nullptr, K, min_pairs, rows, nullptr, 0, &nb ) == PSX_OK && nb >= 0 );
    psx_ransac_block* bl = new psx_ransac_block[(size_t)nb];
    int nb2 = -1;
    CHECK( psx_ransac_many_plan_host( K ? counts.data() : nullptr, K, min_pairs, rows, nb ? bl : nullptr, nb, &nb2 ) == PSX_OK && nb2 == nb );
    long long total = 0;
    std::vector<long long> first( (size_t)K + 1, 0 );
    for( int k = 0; k < K; k++ ) { first[(size_t)k + 1] = first[(size_t)k] + counts[k]; total += counts[k]; }
    std::vector<int> cover( (size_t)total, 0 );
    for( int b = 0; b < nb; b++ ) {
        const psx_ransac_block q = bl[b];
        CHECK( q.set >= 0 && q.set < K );
        if( q.set < 0 || q.set >= K ) break;
        CHECK( counts[q.set] >= min_pairs && q.first >= first[q.set] && q.end <= first[(size_t)q.set + 1] && q.end > q.first && q.end - q.first <= rows );
        if( b == 0 || bl[b - 1].set != q.set ) CHECK( q.first == first[q.set] && ( b == 0 || bl[b - 1].set < q.set ) );
        else CHECK( q.first == bl[b - 1].end && bl[b - 1].end - bl[b - 1].first == rows );      // contiguous, only the last one short
        for( int p = q.first; p < q.end && p < total; p++ ) cover[(size_t)p]++;
    }
    for( int k = 0; k < K; k++ )
        for( long long p = first[k]; p < first[(size_t)k + 1]; p++ )
            if( cover[(size_t)p] != ( counts[k] >= min_pairs ? 1 : 0 ) ) { CHECK( cover[(size_t)p] == ( counts[k] >= min_pairs ? 1 : 0 ) ); return; }
    for( int cap = 0; cap < nb && cap < 20; cap++ ) {
        psx_ransac_block* part = new psx_ransac_block[(size_t)cap];
        int a = -1;
        CHECK( psx_ransac_many_plan_host( counts.data(), K, min_pairs, rows, cap ? part : nullptr, cap, &a ) == PSX_OK && a == nb );
        for( int c = 0; c < cap; c++ ) CHECK( part[c].set == bl[c].set && part[c].first == bl[c].first && part[c].end == bl[c].end );
        delete[] part;
    }
    delete[] bl;
}

static unsigned lcg_state = 2024u;
static float unit() { lcg_state = lcg_state * 1664525u + 1013904223u; return (float)( lcg_state >> 8 ) / 16777216.0f; }

// three sets over one left array: pure translations by (5, 3), (-4, 2), (1, -6) with every fifth pair an outlier
static void check_host( int kind, const int counts[3], int N, int flags )
{
    const int K = 3, MIN = psx_ransac_many_min( kind );
    int total = 0, longest = 0;
    for( int k = 0; k < K; k++ ) { total += counts[k]; longest = counts[k] > longest ? counts[k] : longest; }
    const float shift[3][2] = { { 5.f, 3.f }, { -4.f, 2.f }, { 1.f, -6.f } };
    float* lxy = new float[2 * (size_t)total];
    float* rxy[3];
    psx_match_pair* pairs = new psx_match_pair[(size_t)total];
    int at = 0;
    for( int k = 0; k < K; k++ ) {
        rxy[k] = new float[2 * (size_t)counts[k]];
        for( int p = 0; p < counts[k]; p++, at++ ) {
            const int r = counts[k] - 1 - p;
            lxy[2 * at] = 640.f * unit(); lxy[2 * at + 1] = 480.f * unit();
            const float depth = kind == PSX_GUIDE_EPIPOLAR ? 1.f + unit() : 1.f;       // a scene with depth for F
            if( p % 5 == 4 ) { rxy[k][2 * r] = 640.f * unit(); rxy[k][2 * r + 1] = 480.f * unit(); }
            else { rxy[k][2 * r] = lxy[2 * at] + shift[k][0] * depth; rxy[k][2 * r + 1] = lxy[2 * at + 1] + shift[k][1] * depth; }
            pairs[at].left = at; pairs[at].right = r; pairs[at].d1 = (float)at; pairs[at].d2 = (float)k;
        }
    }
    const int lens[3] = { counts[0], counts[1], counts[2] };
    psx_ransac_opts o = { 2.0f, N, 77u, flags };
    psx_ransac_pt* scratch = new psx_ransac_pt[(size_t)longest];
    // the loop of the single-list rule
    psx_ransac_result one[3];
    psx_match_pair* inl1 = new psx_match_pair[(size_t)total];
    float* models1 = new float[9 * (size_t)K * N];
    int* counts1 = new int[(size_t)K * N];
    for( size_t i = 0; i < 9 * (size_t)K * N; i++ ) models1[i] = 0.f;
    for( size_t i = 0; i < (size_t)K * N; i++ ) counts1[i] = 0;
    int sum = 0;
    at = 0;
    for( int k = 0; k < K; at += counts[k], k++ ) {
        int c = -1;
        CHECK( psx_ransac_many_rule( kind )( pairs + at, counts[k], lxy, total, rxy[k], lens[k], &o, &one[k], inl1 + sum, total - sum, &c,
                                             models1 + 9 * (size_t)k * N, counts1 + (size_t)k * N, scratch ) == PSX_OK );
        CHECK( c == one[k].inliers && ( counts[k] >= MIN || c == 0 ) );
        sum += c;
    }
    CHECK( one[0].best >= 0 && one[1].best == -1 && one[2].best >= 0 && sum >= 2 * MIN );
    // the batched reference: full capacity, total - 1, "how many?"
    const int caps[3] = { sum, sum - 1, 0 };
    for( int t = 0; t < 3; t++ ) {
        const int cap = caps[t];
        psx_ransac_result* res = new psx_ransac_result[K];
        psx_match_pair* inl = cap ? new psx_match_pair[(size_t)cap] : nullptr;
        float* models = new float[9 * (size_t)K * N];
        int* hc = new int[(size_t)K * N];
        int c = -1;
        CHECK( psx_ransac_many_host( kind, pairs, counts, K, lxy, total, rxy, lens, &o, res, inl, cap, &c, t == 0 ? models : nullptr, t == 0 ? hc : nullptr,
                                     scratch ) == PSX_OK );
        CHECK( c == sum && std::memcmp( res, one, sizeof one ) == 0 );
        if( cap ) CHECK( std::memcmp( inl, inl1, sizeof(psx_match_pair) * (size_t)cap ) == 0 );
        if( t == 0 ) CHECK( std::memcmp( models, models1, sizeof(float) * 9 * (size_t)K * N ) == 0 && std::memcmp( hc, counts1, sizeof(int) * (size_t)K * N ) == 0 );
        delete[] res; delete[] inl; delete[] models; delete[] hc;
    }
    {   // a bad index in the last set: the whole call is refused, nothing is written
        psx_ransac_result keep[3];
        std::memset( keep, 0x5a, sizeof keep );
        psx_ransac_result* res = new psx_ransac_result[K];
        std::memcpy( res, keep, sizeof keep );
        psx_match_pair* inl = new psx_match_pair[(size_t)sum];
        std::memset( inl, 0x5a, sizeof(psx_match_pair) * (size_t)sum );
        int c = -77;
        pairs[total - 1].right = lens[2];
        CHECK( psx_ransac_many_host( kind, pairs, counts, K, lxy, total, rxy, lens, &o, res, inl, sum, &c, nullptr, nullptr, scratch ) == PSX_ERR_INVALID );
        CHECK( c == -77 && std::memcmp( res, keep, sizeof keep ) == 0 );
        for( int i = 0; i < sum; i++ ) { int w; std::memcpy( &w, &inl[i].left, 4 ); CHECK( w == 0x5a5a5a5a ); }
        delete[] res; delete[] inl;
    }
    delete[] lxy; delete[] pairs; delete[] scratch; delete[] inl1; delete[] models1; delete[] counts1;
    for( int k = 0; k < K; k++ ) delete[] rxy[k];
}

int main()
{
    const int rows[2] = { PSX_RANSAC_MANY_SCORE_ROWS, PSX_RANSAC_MANY_ROWS };
    for( int r = 0; r < 2; r++ )
        for( int min_pairs = 4; min_pairs <= 8; min_pairs += 4 ) {
            check_plan( { 0, 7, 8, 9, 63, 64, 65, 0, 255, 256, 257, 1023, 1024, 1025, 0 }, min_pairs, rows[r] );
            check_plan( { 0, 3, 4, 5, 511, 512, 513 }, min_pairs, rows[r] );
            check_plan( { 4000 }, min_pairs, rows[r] );
            check_plan( std::vector<int>( 64, 500 ), min_pairs, rows[r] );
            check_plan( { 0, 0, 0 }, min_pairs, rows[r] );
            check_plan( { 3, 2, 1 }, min_pairs, rows[r] );
            check_plan( {}, min_pairs, rows[r] );
        }
    {   // what is refused: nothing is written, the count stays
        int nb = -5;
        const int neg[2] = { 4, -1 }, big[2] = { 0x3fffffff, 1 }, ok[2] = { 300, 4 };
        psx_ransac_block b[4];
        CHECK( psx_ransac_many_plan_host( neg, 2, 4, 256, b, 4, &nb ) == PSX_ERR_INVALID );
        CHECK( psx_ransac_many_plan_host( big, 2, 4, 256, b, 4, &nb ) == PSX_ERR_INVALID );
        CHECK( psx_ransac_many_plan_host( ok, -1, 4, 256, b, 4, &nb ) == PSX_ERR_INVALID );
        CHECK( psx_ransac_many_plan_host( nullptr, 2, 4, 256, b, 4, &nb ) == PSX_ERR_INVALID );
        CHECK( psx_ransac_many_plan_host( ok, 2, 0, 256, b, 4, &nb ) == PSX_ERR_INVALID );
        CHECK( psx_ransac_many_plan_host( ok, 2, 4, 0, b, 4, &nb ) == PSX_ERR_INVALID );
        CHECK( psx_ransac_many_plan_host( ok, 2, 4, 256, nullptr, 4, &nb ) == PSX_ERR_INVALID );
        CHECK( psx_ransac_many_plan_host( ok, 2, 4, 256, b, -1, &nb ) == PSX_ERR_INVALID );
        CHECK( psx_ransac_many_plan_host( ok, 2, 4, 256, b, 4, nullptr ) == PSX_ERR_INVALID );
        CHECK( nb == -5 );
        CHECK( psx_ransac_many_plan_host( ok, 2, 4, 256, b, 4, &nb ) == PSX_OK && nb == 3 && b[2].set == 1 && b[2].first == 300 && b[2].end == 304 );
    }
    const int shapes[3][3] = { { 40, 3, 70 }, { 9, 2, 300 }, { 64, 0, 65 } };
    for( int s = 0; s < 3; s++ )
        for( int kind = PSX_GUIDE_HOMOGRAPHY; kind <= PSX_GUIDE_EPIPOLAR; kind++ )
            for( int flags = 0; flags <= 1; flags++ ) check_host( kind, shapes[s], 48, flags );
    std::printf( "%s\n", fails ? "FAILED" : "ALL OK" );
    return fails ? 1 : 0;
}
