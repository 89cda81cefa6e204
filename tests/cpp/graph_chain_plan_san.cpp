// Stand-alone program (its own main, no library): the host side of the two edge-list calls behind the graph matcher --
// csrc/hip/ransac_graph_plan.h and csrc/hip/match_guided_graph_plan.h and the plain-C++ headers they include, nothing
// else -- built with -ffp-contract=off -fsanitize=address,undefined by tests/test_graph_chain_cpu.py and run directly.
// Never loaded into Python, never run on a GPU.  Every array is a heap array of the exact size, so a read or write past an
// end is the sanitizer's to report:
//   - the host reference of RANSAC over an edge list on views of unequal length (an unsorted list with a duplicate, both
//     orders, a self edge, an edge below the minimum) against the loop of the single-list host rule, at the full capacity,
//     at a capacity inside an edge, at 0 with a NULL output; an index that is in range for a longer view but outside its
//     own edge's refuses the whole call with nothing written;
//   - what the argument checks of both families refuse;
//   - the guided call's tables: the prefix offsets, blocks that never cross an edge, no block for a skipped or empty edge.
#include "match_guided_graph_plan.h"
#include "ransac_graph_plan.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

static int fails = 0;
#define CHECK(c) do { if(!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); fails++; } } while(0)

static unsigned lcg_state = 4242u;
static float unit() { lcg_state = lcg_state * 1664525u + 1013904223u; return (float)( lcg_state >> 8 ) / 16777216.0f; }
static int below( int n ) { const int v = (int)( unit() * (float)n ); return v < n ? v : n - 1; }

// four views of 90, 40, 0 and 130 positions; edge e's pairs follow a translation of its own, every fifth pair an outlier
static void check_host( int kind, int N, int flags )
{
    const int S = 4, E = 6, MIN = psx_ransac_many_min( kind );
    const int lens[S] = { 90, 40, 0, 130 };
    const psx_view_edge edges[E] = { { 3, 0 }, { 0, 1 }, { 1, 0 }, { 0, 0 }, { 3, 1 }, { 0, 1 } };
    const int counts[E] = { 70, 64, MIN - 1, 33, 0, 64 };
    float* xys[S];
    for( int s = 0; s < S; s++ ) {
        xys[s] = lens[s] ? new float[2 * (size_t)lens[s]] : nullptr;
        for( int i = 0; i < 2 * lens[s]; i++ ) xys[s][i] = 500.f * unit();
    }
    int total = 0, longest = 0;
    for( int e = 0; e < E; e++ ) { total += counts[e]; longest = counts[e] > longest ? counts[e] : longest; }
    psx_match_pair* pairs = new psx_match_pair[(size_t)total];
    int at = 0;
    for( int e = 0; e < E; e++ )
        for( int p = 0; p < counts[e]; p++, at++ ) {
            pairs[at].left = below( lens[edges[e].left] ); pairs[at].right = below( lens[edges[e].right] );
            pairs[at].d1 = (float)at; pairs[at].d2 = (float)e;
        }
    for( int p = 0; p < counts[5]; p++ ) pairs[total - counts[5] + p] = pairs[counts[0] + p];      // the duplicate edge: the same list
    CHECK( pairs[0].left < lens[3] );
    pairs[0].left = lens[3] - 1;                                                                 // out of range for every other view
    psx_ransac_opts o = { 2.0f, N, 77u, flags };
    psx_ransac_pt* scratch = new psx_ransac_pt[(size_t)longest];
    // the loop of the single-list rule
    psx_ransac_result one[E];
    psx_match_pair* inl1 = new psx_match_pair[(size_t)total];
    float* models1 = new float[9 * (size_t)E * N];
    int* counts1 = new int[(size_t)E * N];
    for( size_t i = 0; i < 9 * (size_t)E * N; i++ ) models1[i] = 0.f;
    for( size_t i = 0; i < (size_t)E * N; i++ ) counts1[i] = 0;
    int sum = 0;
    at = 0;
    for( int e = 0; e < E; at += counts[e], e++ ) {
        int c = -1;
        const int l = edges[e].left, r = edges[e].right;
        CHECK( psx_ransac_many_rule( kind )( pairs + at, counts[e], xys[l], lens[l], xys[r], lens[r], &o, &one[e], inl1 + sum, total - sum, &c,
                                             models1 + 9 * (size_t)e * N, counts1 + (size_t)e * N, scratch ) == PSX_OK );
        CHECK( c == one[e].inliers && ( counts[e] >= MIN || c == 0 ) );
        sum += c;
    }
    CHECK( one[2].best == -1 && one[4].best == -1 && std::memcmp( &one[1], &one[5], sizeof one[1] ) == 0 );
    const int caps[3] = { sum, one[0].inliers + 1, 0 };
    for( int t = 0; t < 3; t++ ) {
        const int cap = caps[t] < sum ? caps[t] : sum;
        psx_ransac_result* res = new psx_ransac_result[E];
        psx_match_pair* inl = cap ? new psx_match_pair[(size_t)cap] : nullptr;
        float* models = new float[9 * (size_t)E * N];
        int* hc = new int[(size_t)E * N];
        int c = -1;
        CHECK( psx_ransac_graph_host( kind, pairs, counts, edges, E, xys, lens, S, &o, res, inl, cap, &c, t == 0 ? models : nullptr,
                                      t == 0 ? hc : nullptr, scratch ) == PSX_OK );
        CHECK( c == sum && std::memcmp( res, one, sizeof one ) == 0 );
        if( cap ) CHECK( std::memcmp( inl, inl1, sizeof(psx_match_pair) * (size_t)cap ) == 0 );
        if( t == 0 ) CHECK( std::memcmp( models, models1, sizeof(float) * 9 * (size_t)E * N ) == 0 && std::memcmp( hc, counts1, sizeof(int) * (size_t)E * N ) == 0 );
        delete[] res; delete[] inl; delete[] models; delete[] hc;
    }
    {   // in range for view 3, outside the last edge's own left view: the whole call is refused, nothing is written
        psx_ransac_result keep[E];
        std::memset( keep, 0x5a, sizeof keep );
        psx_ransac_result* res = new psx_ransac_result[E];
        std::memcpy( res, keep, sizeof keep );
        const int room = sum > 0 ? sum : 1;
        psx_match_pair* inl = new psx_match_pair[(size_t)room];
        std::memset( inl, 0x5a, sizeof(psx_match_pair) * (size_t)room );
        int c = -77;
        pairs[total - 1].left = lens[0];
        CHECK( lens[0] < lens[3] );
        CHECK( psx_ransac_graph_host( kind, pairs, counts, edges, E, xys, lens, S, &o, res, inl, room, &c, nullptr, nullptr, scratch ) == PSX_ERR_INVALID );
        CHECK( c == -77 && std::memcmp( res, keep, sizeof keep ) == 0 );
        for( int i = 0; i < room; i++ ) { int w; std::memcpy( &w, &inl[i].left, 4 ); CHECK( w == 0x5a5a5a5a ); }
        delete[] res; delete[] inl;
    }
    delete[] pairs; delete[] scratch; delete[] inl1; delete[] models1; delete[] counts1;
    for( int s = 0; s < S; s++ ) delete[] xys[s];
}

static void check_ransac_args()
{
    const int lens[3] = { 40, 30, 30 };
    const psx_view_edge edges[2] = { { 0, 1 }, { 2, 0 } };
    const int counts[2] = { 9, 12 };
    float dummy[2] = { 0.f, 0.f };
    const float* xys[3] = { dummy, dummy, dummy };              // only NULL is looked at
    psx_ransac_opts o = { 2.0f, 16, 0u, 1 };
    psx_ransac_result res[2];
    psx_match_pair out[4];
    int count = 0;
    long long total = -1;
    CHECK( psx_ransac_graph_args_ok( dummy, counts, edges, 2, xys, lens, 3, &o, res, out, 4, &count, &total ) && total == 21 );
    const psx_view_edge far_[2] = { { 0, 1 }, { 3, 0 } };
    const int neg[2] = { 9, -1 }, big[2] = { 0x3fffffff, 1 }, neglen[3] = { 40, -1, 30 };
    const float* hole[3] = { dummy, nullptr, dummy };
    CHECK( !psx_ransac_graph_args_ok( dummy, counts, far_, 2, xys, lens, 3, &o, res, out, 4, &count, &total ) );
    CHECK( !psx_ransac_graph_args_ok( dummy, neg, edges, 2, xys, lens, 3, &o, res, out, 4, &count, &total ) );
    CHECK( !psx_ransac_graph_args_ok( dummy, big, edges, 2, xys, lens, 3, &o, res, out, 4, &count, &total ) );
    CHECK( !psx_ransac_graph_args_ok( dummy, counts, edges, 2, xys, neglen, 3, &o, res, out, 4, &count, &total ) );
    CHECK( !psx_ransac_graph_args_ok( dummy, counts, edges, 2, hole, lens, 3, &o, res, out, 4, &count, &total ) );
    CHECK( !psx_ransac_graph_args_ok( dummy, counts, edges, 2, nullptr, lens, 3, &o, res, out, 4, &count, &total ) );
    CHECK( !psx_ransac_graph_args_ok( nullptr, counts, edges, 2, xys, lens, 3, &o, res, out, 4, &count, &total ) );
    CHECK( !psx_ransac_graph_args_ok( dummy, counts, edges, 2, xys, lens, 3, &o, nullptr, out, 4, &count, &total ) );
    CHECK( !psx_ransac_graph_args_ok( dummy, counts, edges, 2, xys, lens, 3, &o, res, nullptr, 4, &count, &total ) );
    CHECK( !psx_ransac_graph_args_ok( dummy, counts, edges, 2, xys, lens, 3, &o, res, out, 4, nullptr, &total ) );
    CHECK( !psx_ransac_graph_args_ok( dummy, counts, edges, 2, xys, lens, 3, nullptr, res, out, 4, &count, &total ) );
    CHECK( !psx_ransac_graph_args_ok( dummy, counts, edges, 2, xys, lens, 0, &o, res, out, 4, &count, &total ) );
    CHECK( total == 21 );
}

static psx_guide guide_of( int kind )
{
    psx_guide g;
    g.kind = kind;
    for( int k = 0; k < 9; k++ ) g.m[k] = ( k % 4 == 0 ) ? 1.f : 0.f;
    g.tol = 2.f;
    return g;
}

// the guided call's tables on exact-size heap arrays
static void check_guided_tables( const std::vector<int>& lens, const std::vector<psx_view_edge>& edges, const std::vector<int>& kinds )
{
    const int S = (int)lens.size(), E = (int)edges.size();
    int* hl = new int[(size_t)S];
    psx_view_edge* he = new psx_view_edge[(size_t)E];
    psx_guide* hg = new psx_guide[(size_t)E];
    for( int s = 0; s < S; s++ ) hl[s] = lens[s];
    for( int e = 0; e < E; e++ ) { he[e] = edges[e]; hg[e] = guide_of( kinds[e] ); }
    psx_gg_edge* ep = new psx_gg_edge[(size_t)E];
    const psx_gg_totals t = psx_gg_edges( hl, he, E, hg, ep );
    long long frows = 0, brows = 0, fb = 0, bb = 0;
    int live = 0;
    for( int e = 0; e < E; e++ ) {
        const bool on = kinds[e] != PSX_GUIDE_NONE && lens[he[e].left] > 0 && lens[he[e].right] > 0;
        CHECK( ep[e].left == he[e].left && ep[e].right == he[e].right );
        CHECK( ep[e].l_len == ( on ? lens[he[e].left] : 0 ) && ep[e].r_len == ( on ? lens[he[e].right] : 0 ) );
        CHECK( ep[e].foff == frows && ep[e].boff == brows && ep[e].jf0 == fb );                  // the prefix sums over the live edges
        frows += ep[e].l_len; brows += ep[e].r_len;
        fb += ( ep[e].l_len + 255 ) / 256; bb += ( ep[e].r_len + 255 ) / 256;
        live += on;
    }
    CHECK( t.frows == frows && t.brows == brows && t.fblocks == fb && t.bblocks == bb && t.live == live );
    for( int dir = 0; dir < 2; dir++ ) {
        const long long nb = dir ? bb : fb;
        CHECK( psx_gg_blocks( ep, E, dir, nullptr, 0 ) == nb );
        psx_graph_wg* bl = new psx_graph_wg[(size_t)nb];
        CHECK( psx_gg_blocks( ep, E, dir, bl, nb ) == nb );
        std::vector<std::vector<int>> cover( (size_t)E );
        for( int e = 0; e < E; e++ ) cover[(size_t)e].assign( (size_t)( dir ? ep[e].r_len : ep[e].l_len ), 0 );
        for( long long b = 0; b < nb; b++ ) {
            const int e = bl[b].edge, rows = ( e >= 0 && e < E ) ? ( dir ? ep[e].r_len : ep[e].l_len ) : 0;
            CHECK( e >= 0 && e < E && rows > 0 && bl[b].row0 % 256 == 0 && bl[b].row0 < rows );  // no block for a skipped or empty edge
            if( e < 0 || e >= E ) break;
            if( b == 0 || bl[b - 1].edge != e ) CHECK( bl[b].row0 == 0 && ( b == 0 || bl[b - 1].edge < e ) && ( dir || ep[e].jf0 == b ) );
            else CHECK( bl[b].row0 == bl[b - 1].row0 + 256 );
            for( int r = bl[b].row0; r < bl[b].row0 + 256 && r < rows; r++ ) cover[(size_t)e][(size_t)r]++;      // a block ends with its edge
        }
        for( int e = 0; e < E; e++ )
            for( int c : cover[(size_t)e] ) if( c != 1 ) { CHECK( c == 1 ); break; }
        if( nb > 1 ) {                                           // a smaller capacity: the prefix, nothing past it
            psx_graph_wg* part = new psx_graph_wg[(size_t)nb - 1];
            CHECK( psx_gg_blocks( ep, E, dir, part, nb - 1 ) == nb );
            CHECK( std::memcmp( part, bl, sizeof(psx_graph_wg) * (size_t)( nb - 1 ) ) == 0 );
            delete[] part;
        }
        delete[] bl;
    }
    delete[] hl; delete[] he; delete[] hg; delete[] ep;
}

static void check_guided_args()
{
    const int lens[3] = { 3, 5, 4 };
    const psx_view_edge edges[2] = { { 0, 1 }, { 2, 0 } };
    unsigned char d = 0;
    float x = 0.f;
    const unsigned char* sets[3] = { &d, &d, &d };              // only NULL is looked at
    const float* xys[3] = { &x, &x, &x };
    psx_guide g[2] = { guide_of( PSX_GUIDE_HOMOGRAPHY ), guide_of( PSX_GUIDE_NONE ) };
    psx_match_opts o = { 0.8f, PSX_PAIRS_MUTUAL };
    psx_match_pair_u8 out[2];
    int ec[2], count = 0;
    CHECK( psx_gg_args_ok( sets, xys, lens, 3, edges, 2, g, &o, out, 2, ec, &count ) );
    g[1].tol = NAN; g[1].m[3] = INFINITY;                        // kind 0: the rest is not looked at
    CHECK( psx_gg_args_ok( sets, xys, lens, 3, edges, 2, g, &o, out, 2, ec, &count ) );
    g[1].kind = PSX_GUIDE_EPIPOLAR;
    CHECK( !psx_gg_args_ok( sets, xys, lens, 3, edges, 2, g, &o, out, 2, ec, &count ) );
    g[1] = guide_of( 3 );
    CHECK( !psx_gg_args_ok( sets, xys, lens, 3, edges, 2, g, &o, out, 2, ec, &count ) );
    g[1] = guide_of( PSX_GUIDE_EPIPOLAR );
    const float* hole[3] = { &x, nullptr, &x };
    const unsigned char* dhole[3] = { &d, &d, nullptr };
    const psx_view_edge far_[2] = { { 0, 1 }, { 0, 3 } };
    CHECK( !psx_gg_args_ok( sets, hole, lens, 3, edges, 2, g, &o, out, 2, ec, &count ) );
    CHECK( !psx_gg_args_ok( dhole, xys, lens, 3, edges, 2, g, &o, out, 2, ec, &count ) );
    CHECK( !psx_gg_args_ok( sets, nullptr, lens, 3, edges, 2, g, &o, out, 2, ec, &count ) );
    CHECK( !psx_gg_args_ok( sets, xys, lens, 3, far_, 2, g, &o, out, 2, ec, &count ) );
    CHECK( !psx_gg_args_ok( sets, xys, lens, 3, edges, 2, nullptr, &o, out, 2, ec, &count ) );
    CHECK( !psx_gg_args_ok( sets, xys, lens, 3, edges, 2, g, &o, out, 2, nullptr, &count ) );
    CHECK( !psx_gg_args_ok( sets, xys, lens, 3, edges, 2, g, &o, nullptr, 2, ec, &count ) );
    CHECK( !psx_gg_args_ok( sets, xys, lens, 3, edges, 2, g, nullptr, out, 2, ec, &count ) );
    CHECK( psx_gg_args_ok( sets, xys, lens, 3, edges, 2, g, &o, out, 2, ec, &count ) );
}

int main()
{
    for( int kind = PSX_RANSAC_MODEL_HOMOGRAPHY; kind <= PSX_RANSAC_MODEL_SIMILARITY; kind++ )
        for( int flags = 0; flags <= 1; flags++ ) check_host( kind, 48, flags );
    check_ransac_args();
    const int H = PSX_GUIDE_HOMOGRAPHY, F = PSX_GUIDE_EPIPOLAR, Z = PSX_GUIDE_NONE;
    check_guided_tables( { 300, 257, 0, 33, 513, 1 }, { {3,4}, {0,1}, {4,5}, {0,0}, {0,2}, {1,0}, {5,4}, {2,0}, {4,3}, {0,1} },
                         { H, F, Z, H, F, Z, H, F, Z, H } );
    check_guided_tables( { 600, 1, 255, 256, 257, 300 }, { {1,0}, {2,5}, {3,0}, {4,5}, {0,5}, {4,0}, {0,3} }, { F, H, H, Z, H, F, H } );
    check_guided_tables( { 600, 1, 255, 256, 257, 300 }, { {1,0}, {2,5}, {3,0} }, { Z, Z, Z } );
    check_guided_tables( { 0, 0 }, { {0,1}, {1,1} }, { H, F } );
    check_guided_tables( { 5 }, {}, {} );
    check_guided_args();
    std::printf( "%s\n", fails ? "FAILED" : "ALL OK" );
    return fails ? 1 : 0;
}
