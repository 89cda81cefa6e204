// Stand-alone program (its own main, no library): the plan of the one-to-many pair search, csrc/hip/match_many_plan.h alone,
// built with -fsanitize=address,undefined by tests/test_match_many_cpu.py and run directly.  The tables are heap arrays of
// the exact size the "how many?" form reports -- and of every smaller capacity -- so a write past an end is the sanitizer's
// to report.  The invariants are restated here: every row of every non-empty set covered exactly once by the chunks and by
// the blocks, nothing spanning two sets, r0 a multiple of 32, at most 512 rows per chunk, a set's chunks ascending and
// contiguous, empty sets absent.
#include "match_many_plan.h"

#include <climits>
#include <cstdio>
#include <vector>

static int fails = 0;
#define CHECK(c) do { if(!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); fails++; } } while(0)

static void check_side( const std::vector<int>& lens, const std::vector<psx_many_chunk>& ch, const std::vector<psx_many_block>& bl,
                        bool chunks_cut_these )
{
    // `lens`: the side the table under test cuts; chunks_cut_these: look at ch, otherwise at bl
    std::vector<std::vector<int>> cover( lens.size() );
    for( size_t s = 0; s < lens.size(); s++ ) cover[s].assign( (size_t)lens[s], 0 );
    if( chunks_cut_these ) {
        int last_set = -1;
        std::vector<char> seen( lens.size(), 0 );
        for( size_t c = 0; c < ch.size(); c++ ) {
            const psx_many_chunk q = ch[c];
            CHECK( q.set >= 0 && q.set < (int)lens.size() );
            if( q.set < 0 || q.set >= (int)lens.size() ) return;
            CHECK( q.r0 % 32 == 0 && q.r0 >= 0 && q.r1 > q.r0 && q.r1 <= lens[q.set] && q.r1 - q.r0 <= 512 );
            if( q.set != last_set ) { CHECK( !seen[q.set] && q.set > last_set && q.r0 == 0 ); seen[q.set] = 1; last_set = q.set; }
            else CHECK( q.r0 == ch[c - 1].r1 );                    // ascending, contiguous, no gap
            for( int r = q.r0; r < q.r1 && r < lens[q.set]; r++ ) cover[q.set][r]++;
        }
    } else {
        for( size_t b = 0; b < bl.size(); b++ ) {
            const psx_many_block q = bl[b];
            CHECK( q.set >= 0 && q.set < (int)lens.size() );
            if( q.set < 0 || q.set >= (int)lens.size() ) return;
            CHECK( q.row0 % 256 == 0 && q.row0 >= 0 && q.row0 < lens[q.set] );
            if( b > 0 ) CHECK( q.set > bl[b - 1].set || ( q.set == bl[b - 1].set && q.row0 == bl[b - 1].row0 + 256 ) );
            for( int r = q.row0; r < q.row0 + 256 && r < lens[q.set]; r++ ) cover[q.set][r]++;
        }
    }
    for( size_t s = 0; s < lens.size(); s++ )
        for( int r = 0; r < lens[s]; r++ ) if( cover[s][r] != 1 ) { CHECK( cover[s][r] == 1 ); return; }
}

static void run( int l_len, const std::vector<int>& r_lens )
{
    const int K = (int)r_lens.size();
    for( int backward = 0; backward < 2; backward++ ) {
        int nc = -1, nb = -1;
        CHECK( psx_many_plan_host( l_len, K ? r_lens.data() : nullptr, K, backward, nullptr, 0, &nc, nullptr, 0, &nb ) == PSX_OK );
        CHECK( nc >= 0 && nb >= 0 );
        std::vector<psx_many_chunk> ch( (size_t)nc );
        std::vector<psx_many_block> bl( (size_t)nb );
        int nc2 = -1, nb2 = -1;
        CHECK( psx_many_plan_host( l_len, K ? r_lens.data() : nullptr, K, backward, nc ? ch.data() : nullptr, nc, &nc2,
                                   nb ? bl.data() : nullptr, nb, &nb2 ) == PSX_OK );
        CHECK( nc2 == nc && nb2 == nb );
        const std::vector<int> lside( 1, l_len );
        check_side( backward ? lside : r_lens, ch, bl, true );
        check_side( backward ? r_lens : lside, ch, bl, false );
        // enough workgroups: blocks x chunks reaches the target unless every chunk is already one tile
        bool one_tile = true;
        for( const psx_many_chunk& q : ch ) if( q.r1 - q.r0 > 32 ) one_tile = false;
        if( nc > 0 && nb > 0 && !one_tile ) CHECK( (long long)nc * nb >= PSX_MANY_WGS / 2 );
        // every smaller capacity: the totals are still reported, the prefix is the same, nothing is written past it
        for( int cap = 0; cap < nc && cap < 40; cap++ ) {
            std::vector<psx_many_chunk> part( (size_t)cap );
            std::vector<psx_many_block> pb( (size_t)( cap < nb ? cap : nb ) );
            int a = -1, b = -1;
            CHECK( psx_many_plan_host( l_len, r_lens.data(), K, backward, cap ? part.data() : nullptr, cap, &a,
                                       pb.empty() ? nullptr : pb.data(), (int)pb.size(), &b ) == PSX_OK );
            CHECK( a == nc && b == nb );
            for( int c = 0; c < cap; c++ ) CHECK( part[c].set == ch[c].set && part[c].r0 == ch[c].r0 && part[c].r1 == ch[c].r1 );
            for( size_t c = 0; c < pb.size(); c++ ) CHECK( pb[c].set == bl[c].set && pb[c].row0 == bl[c].row0 );
        }
    }
}

int main()
{
    run( 300, { 257, 0, 1, 31, 32, 33, 512, 513, 255, 256 } );
    run( 257, { 64, 1000, 300 } );
    run( 1, { 1, 2, 40 } );
    run( 2500, { 2300, 700, 1200 } );
    {
        std::vector<int> tiny;
        for( int i = 0; i < 200; i++ ) tiny.push_back( i % 41 );
        run( 70, tiny );
    }
    run( 18432, { 18432 } );
    run( 2048, std::vector<int>( 64, 2048 ) );
    run( 0, { 5, 6 } );
    run( 7, {} );
    run( 9, { 0, 0, 0 } );
    {   // what is refused: nothing is written, the counts stay
        int nc = -5, nb = -5;
        const int neg[2] = { 4, -1 }, big[2] = { INT_MAX, 1 }, ok[2] = { 3, 4 };
        psx_many_chunk c[4]; psx_many_block b[4];
        CHECK( psx_many_plan_host( 5, neg, 2, 0, c, 4, &nc, b, 4, &nb ) == PSX_ERR_INVALID );
        CHECK( psx_many_plan_host( 5, big, 2, 0, c, 4, &nc, b, 4, &nb ) == PSX_ERR_INVALID );      // sum of lengths above INT_MAX
        CHECK( psx_many_plan_host( INT_MAX, ok, 2, 0, c, 4, &nc, b, 4, &nb ) == PSX_ERR_INVALID ); // n_sets * l_len above INT_MAX
        CHECK( psx_many_plan_host( -1, ok, 2, 0, c, 4, &nc, b, 4, &nb ) == PSX_ERR_INVALID );
        CHECK( psx_many_plan_host( 5, ok, -1, 0, c, 4, &nc, b, 4, &nb ) == PSX_ERR_INVALID );
        CHECK( psx_many_plan_host( 5, nullptr, 2, 0, c, 4, &nc, b, 4, &nb ) == PSX_ERR_INVALID );
        CHECK( psx_many_plan_host( 5, ok, 2, 2, c, 4, &nc, b, 4, &nb ) == PSX_ERR_INVALID );
        CHECK( psx_many_plan_host( 5, ok, 2, 0, nullptr, 4, &nc, b, 4, &nb ) == PSX_ERR_INVALID );
        CHECK( psx_many_plan_host( 5, ok, 2, 0, c, 4, &nc, nullptr, 4, &nb ) == PSX_ERR_INVALID );
        CHECK( psx_many_plan_host( 5, ok, 2, 0, c, -1, &nc, b, 4, &nb ) == PSX_ERR_INVALID );
        CHECK( psx_many_plan_host( 5, ok, 2, 0, c, 4, nullptr, b, 4, &nb ) == PSX_ERR_INVALID );
        CHECK( psx_many_plan_host( 5, ok, 2, 0, c, 4, &nc, b, 4, nullptr ) == PSX_ERR_INVALID );
        CHECK( nc == -5 && nb == -5 );
        CHECK( psx_many_plan_host( 5, ok, 2, 0, c, 4, &nc, b, 4, &nb ) == PSX_OK && nc == 2 && nb == 1 );
    }
    std::printf( "%s\n", fails ? "FAILED" : "ALL OK" );
    return fails ? 1 : 0;
}
