// Stand-alone program (its own main, no library): the admissibility rule of guided matching (csrc/hip/guide_rule.h) on
// 2 x 256 pairs of quarter-pixel points whose expected outcome is written out below row by row (one 16-bit word per left
// point, bit j = right point j; computed from the rule's formulas in float32, independently of this header), on the edge
// inputs the rule names -- tol = 0, NaN and infinite positions, c <= 0, a degenerate line, a tolerance whose square
// overflows -- and the guide validation.  Built with -ffp-contract=off -fsanitize=address,undefined by
// tests/test_match_guided_cpu.py and run directly.  The point arrays are heap vectors of the exact size.
#include "guide_rule.h"

#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

static int fails = 0;
#define CHECK(c) do { if(!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); fails++; } } while(0)

static const float H[9] = { 1.25f, 0.03125f, 4.0f, -0.015625f, 1.25f, -3.0f, 0.0001220703125f, -6.103515625e-05f, 1.0f };
static const float F[9] = { 0.0f, -0.015625f, 0.5f, 0.015625f, 0.0f, -1.0f, -0.5f, 1.0f, 0.25f };
// H with tol 3, F with tol 0.75
static const unsigned ROWS_H[16] = { 0x0100, 0x0000, 0x0204, 0x0000, 0x0008, 0x0000, 0x1010, 0x0000, 0x2020, 0x0000, 0x4000, 0x0000, 0x0102, 0x0000, 0x0204, 0x1000 };
static const unsigned ROWS_F[16] = { 0x4002, 0x0000, 0x0004, 0x2020, 0x0008, 0x4042, 0x0101, 0x0800, 0x0200, 0x4042, 0x0000, 0x0004, 0x0200, 0x0008, 0x0400, 0x2001 };

static bool pair( int kind, const float* m, float tol, float xl, float yl, float xr, float yr )
{
    return psx_guide_pair( kind, m, tol, xl, yl, xr, yr );
}

int main()
{
    const int n = 16;
    std::vector<float> lx( n ), ly( n ), rx( n ), ry( n );
    for( int i = 0; i < n; i++ ) {
        lx[i] = (float)( ( i * 37 + 5 ) % 64 ) * 0.25f;  ly[i] = (float)( ( i * 43 + 15 ) % 64 ) * 0.25f;
        rx[i] = (float)( ( i * 13 + 7 ) % 96 ) * 0.25f;  ry[i] = (float)( ( i * 21 + 2 ) % 80 ) * 0.25f;
    }
    int admitted = 0;
    for( int i = 0; i < n; i++ ) {
        unsigned h = 0, f = 0;
        for( int j = 0; j < n; j++ ) {
            if( pair( PSX_GUIDE_HOMOGRAPHY, H, 3.0f, lx[i], ly[i], rx[j], ry[j] ) ) h |= 1u << j;
            if( pair( PSX_GUIDE_EPIPOLAR, F, 0.75f, lx[i], ly[i], rx[j], ry[j] ) ) f |= 1u << j;
        }
        if( h != ROWS_H[i] ) { std::printf( "FAIL homography row %d: 0x%04x, expected 0x%04x\n", i, h, ROWS_H[i] ); fails++; }
        if( f != ROWS_F[i] ) { std::printf( "FAIL epipolar row %d: 0x%04x, expected 0x%04x\n", i, f, ROWS_F[i] ); fails++; }
        admitted += __builtin_popcount( h ) + __builtin_popcount( f );
    }
    CHECK( admitted == 14 + 22 );

    const float I[9] = { 1, 0, 0, 0, 1, 0, 0, 0, 1 };
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = INFINITY;
    // identity H is a search window of radius tol, the boundary included; tol = 0 admits the point itself only
    CHECK( pair( 1, I, 5.0f, 10.0f, 10.0f, 13.0f, 14.0f ) );            // distance exactly 5
    CHECK( !pair( 1, I, 5.0f, 10.0f, 10.0f, 13.0f, 14.25f ) );
    CHECK( pair( 1, I, 0.0f, 7.5f, 2.25f, 7.5f, 2.25f ) );
    CHECK( !pair( 1, I, 0.0f, 7.5f, 2.25f, 7.5f, 2.5f ) );
    // the relation is not symmetric in its roles
    CHECK( pair( 1, H, 3.0f, lx[0], ly[0], rx[8], ry[8] ) && !pair( 1, H, 3.0f, rx[8], ry[8], lx[0], ly[0] ) );
    // NaN anywhere: inadmissible; infinite positions: inf - inf or 0 * inf is NaN
    CHECK( !pair( 1, I, 5.0f, nan, 10.0f, 13.0f, 14.0f ) && !pair( 1, I, 5.0f, 10.0f, 10.0f, 13.0f, nan ) );
    CHECK( !pair( 2, F, 0.75f, nan, 1.0f, 1.0f, 1.0f ) && !pair( 2, F, 0.75f, 1.0f, 1.0f, nan, 1.0f ) );
    CHECK( !pair( 1, I, 5.0f, inf, 10.0f, inf, 14.0f ) && !pair( 1, I, 5.0f, 10.0f, 10.0f, inf, 14.0f ) );
    CHECK( !pair( 2, F, 0.75f, inf, 1.0f, 1.0f, 1.0f ) );
    // c <= 0: behind the plane of the homography, never admissible -- also with the point on its image
    const float NEG[9] = { 1, 0, 0, 0, 1, 0, 0, 0, -1 }, ZERO[9] = { 1, 0, 0, 0, 1, 0, 0, 0, 0 };
    CHECK( !pair( 1, NEG, 5.0f, 1.0f, 1.0f, -1.0f, -1.0f ) && !pair( 1, ZERO, 5.0f, 0.0f, 0.0f, 0.0f, 0.0f ) );
    // a degenerate line a = b = 0: e = c, allowed iff c * c <= 0
    const float DEG[9] = { 0, 0, 0, 0, 0, 0, 0, 0, 1 }, DEG0[9] = { 0, 0, 0, 0, 0, 0, 0, 0, 0 };
    CHECK( !pair( 2, DEG, 2.0f, 3.0f, 4.0f, 5.0f, 6.0f ) && pair( 2, DEG0, 2.0f, 3.0f, 4.0f, 5.0f, 6.0f ) );
    // a tolerance whose square overflows: the right-hand side is +inf and everything finite is admissible
    CHECK( pair( 1, I, 1e30f, 0.0f, 0.0f, 1e6f, -1e6f ) && pair( 2, F, 1e30f, 3.0f, 4.0f, 1e6f, -1e6f ) );
    CHECK( !pair( 1, I, 1e30f, 0.0f, 0.0f, nan, 0.0f ) );

    // validation
    psx_guide g = { PSX_GUIDE_HOMOGRAPHY, { 1, 0, 0, 0, 1, 0, 0, 0, 1 }, 2.0f };
    CHECK( psx_guide_valid( &g ) && !psx_guide_valid( nullptr ) );
    g.kind = PSX_GUIDE_EPIPOLAR; CHECK( psx_guide_valid( &g ) );
    g.tol = 0.0f; CHECK( psx_guide_valid( &g ) );
    const int kinds[] = { 0, 3, -1, 1 << 30 };
    for( int k : kinds ) { psx_guide b = g; b.kind = k; CHECK( !psx_guide_valid( &b ) ); }
    const float tols[] = { -1.0f, -0.0f - 1e-30f, nan, inf, -inf };
    for( float t : tols ) { psx_guide b = g; b.tol = t; CHECK( !psx_guide_valid( &b ) ); }
    for( int k = 0; k < 9; k++ ) {
        const float bad[] = { nan, inf, -inf };
        for( float v : bad ) { psx_guide b = g; b.m[k] = v; CHECK( !psx_guide_valid( &b ) ); }
    }
    std::printf( "%s\n", fails ? "FAILED" : "ALL OK" );
    return fails ? 1 : 0;
}
