// Stand-alone program (its own main, no library): the host join of csrc/hip/match_join.h and the predicate of match_rule.h on
// crafted rows -- NaN, +inf, INT_MAX, ties, many-to-one, every capacity from 0 to past the count, out-of-range indices -- built
// with -fsanitize=address,undefined by tests/test_match_pairs_cpu.py and run directly.  The arrays are heap vectors of the exact
// size, so a read or write past an end is the sanitizer's to report; the expected lists are restated here row by row.
#include "match_join.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

static int fails = 0;
#define CHECK(c) do { if(!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); fails++; } } while(0)

template <class Dist> static Dist none();
template <> float none<float>() { return INFINITY; }
template <> int none<int>() { return INT_MAX; }

template <class Dist, class Pair> static void run( const char* what )
{
    const int nl = 300, nr = 211;
    std::vector<int> fm( 3 * nl ), bm( 3 * nr );
    std::vector<Dist> fd( 2 * nl );
    unsigned s = 99u;
    auto rnd = [&]() { s = s * 1664525u + 1013904223u; return s >> 8; };
    for( int j = 0; j < nr; j++ ) { bm[3 * j] = (int)( rnd() % nl ); bm[3 * j + 1] = (int)( rnd() % nl ); bm[3 * j + 2] = 0; }
    for( int i = 0; i < nl; i++ ) {
        int j = (int)( rnd() % nr );
        Dist d1, d2;
        switch( i % 10 ) {
        case 0: d1 = (Dist)0; d2 = (Dist)0; break;                              // 0 / 0: NaN, never kept
        case 1: d1 = none<Dist>(); d2 = none<Dist>(); break;                    // inf / inf: NaN, never kept
        case 2: d1 = (Dist)( 1 + rnd() % 1000 ); d2 = none<Dist>(); break;      // no second neighbour: quotient 0, kept
        case 3: d1 = (Dist)( 1 + rnd() % 1000 ); d2 = d1; break;                // a tie: exactly 1
        case 4: d1 = (Dist)4; d2 = (Dist)5; break;                              // exactly 0.8f? 4/5 rounds to 0.8f: not < 0.8f
        case 5: d1 = (Dist)0; d2 = (Dist)( 1 + rnd() % 9 ); break;              // an exact copy: quotient 0
        default: d1 = (Dist)( 1 + rnd() % 5000 ); d2 = (Dist)( (unsigned)d1 + rnd() % 5000 ); break;
        }
        if( i % 3 == 0 ) bm[3 * j] = i;                                         // mutual for a third of the rows ...
        if( i % 7 == 0 && i > 0 ) j = fm[3 * ( i - 1 )];                        // ... and several rows on one right row
        fm[3 * i] = j; fm[3 * i + 1] = (int)( rnd() % nr ); fm[3 * i + 2] = 0;
        fd[2 * i] = d1; fd[2 * i + 1] = d2;
    }
    const float ratios[] = { 0.6f, 0.8f, 1.0f, INFINITY };
    for( float ratio : ratios ) for( int flags = 0; flags < 2; flags++ ) {
        std::vector<int> want;
        for( int i = 0; i < nl; i++ ) {
            const float a = fd[2 * i] == none<Dist>() ? INFINITY : (float)fd[2 * i];
            const float b = fd[2 * i + 1] == none<Dist>() ? INFINITY : (float)fd[2 * i + 1];
            const float q = a / b;
            if( !( q < ratio ) ) continue;
            if( flags && bm[3 * fm[3 * i]] != i ) continue;
            want.push_back( i );
        }
        const psx_match_opts o = { ratio, flags };
        const int total = (int)want.size();
        CHECK( total > 0 && total < nl );
        const int caps[] = { 0, 1, total - 1, total, total + 5, nl };
        for( int cap : caps ) {
            std::vector<Pair> out( cap );               // exactly `cap` records: one more write is a heap overflow
            int n = -1;
            const int rc = psx_pairs_join_host<Dist, Pair>( fm.data(), fd.data(), nl, flags ? bm.data() : nullptr, nr, &o,
                                                           cap ? out.data() : nullptr, cap, &n );
            CHECK( rc == PSX_OK && n == total );
            for( int k = 0; k < cap && k < total; k++ )
                CHECK( out[k].left == want[k] && out[k].right == fm[3 * want[k]] &&
                       std::memcmp( &out[k].d1, &fd[2 * want[k]], 4 ) == 0 && std::memcmp( &out[k].d2, &fd[2 * want[k] + 1], 4 ) == 0 );
        }
    }
    // the predicate itself on the corners
    CHECK( !psx_match_keep( 0.0f, 0.0f, INFINITY ) && !psx_match_keep( INFINITY, INFINITY, INFINITY ) );
    CHECK( psx_match_keep( 3.0f, INFINITY, 0.6f ) && !psx_match_keep( 4.0f, 5.0f, 0.8f ) && psx_match_keep( 4.0f, 5.0f, 1.0f ) );
    CHECK( !psx_match_keep( 7.0f, 7.0f, 1.0f ) && psx_match_keep( 7.0f, 7.0f, INFINITY ) );
    CHECK( psx_match_dist( INT_MAX ) == INFINITY && psx_match_dist( 8323200 ) == 8323200.0f && psx_match_dist( 2.5f ) == 2.5f );
    // out-of-range indices are refused before anything is written; the arrays are never indexed with them
    {
        const psx_match_opts o = { 0.8f, PSX_PAIRS_MUTUAL };
        std::vector<Pair> out( nl );
        std::memset( out.data(), 0x5a, out.size() * sizeof(Pair) );
        int n = -77;
        const int bad[] = { -1, nr, INT_MAX, INT_MIN };
        for( int b : bad ) {
            const int keep = fm[3 * 17];
            fm[3 * 17] = b;
            CHECK( ( psx_pairs_join_host<Dist, Pair>( fm.data(), fd.data(), nl, bm.data(), nr, &o, out.data(), nl, &n ) ) == PSX_ERR_INVALID );
            fm[3 * 17] = keep;
        }
        const int badl[] = { -1, nl, INT_MAX };
        for( int b : badl ) {
            const int keep = bm[3 * ( nr - 1 )];
            bm[3 * ( nr - 1 )] = b;
            CHECK( ( psx_pairs_join_host<Dist, Pair>( fm.data(), fd.data(), nl, bm.data(), nr, &o, out.data(), nl, &n ) ) == PSX_ERR_INVALID );
            bm[3 * ( nr - 1 )] = keep;
        }
        CHECK( n == -77 );
        const unsigned char* p = reinterpret_cast<const unsigned char*>( out.data() );
        bool untouched = true;
        for( size_t k = 0; k < out.size() * sizeof(Pair); k++ ) untouched = untouched && p[k] == 0x5a;
        CHECK( untouched );
        // empty sides: no array is read at all (null pointers)
        CHECK( ( psx_pairs_join_host<Dist, Pair>( nullptr, nullptr, 0, nullptr, 0, &o, nullptr, 0, &n ) ) == PSX_OK && n == 0 );
        n = -1;
        CHECK( ( psx_pairs_join_host<Dist, Pair>( fm.data(), fd.data(), nl, nullptr, 0, &o, nullptr, 0, &n ) ) == PSX_OK && n == 0 );
    }
    std::printf( "%s: %s\n", what, fails ? "failed" : "ok" );
}

int main()
{
    run<float, psx_match_pair>( "float" );
    run<int, psx_match_pair_u8>( "bytes" );
    std::printf( "%s\n", fails ? "FAILED" : "ALL OK" );
    return fails ? 1 : 0;
}
