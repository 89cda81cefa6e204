// Stand-alone program (its own main, no library): the plan of the one-to-many FLOAT pair search,
// csrc/hip/match_many_f32_plan.h alone, built with -fsanitize=address,undefined by tests/test_match_many_f32_cpu.py and run
// directly.  For both paths and both flag values psx_many_f32_build's tables are checked here: every row of every
// non-empty set covered exactly once by the chunks and by the blocks, nothing spanning two sets, a set's chunks ascending
// and contiguous, the prefilter's chunks whole staged blocks of 64 rows; the groups partition the sets, every group's
// share of the growing buffer is what its chunks x rows cost and stays within the budget unless it is a single set; the
// launch count is 2 per group plus the fixed kernels; the path follows the rule.
#include "match_many_f32_plan.h"

#include <climits>
#include <cstdio>
#include <vector>

static int fails = 0;
#define CHECK(c) do { if(!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); fails++; } } while(0)

static void check_chunks( const std::vector<int>& lens, const std::vector<psx_many_chunk>& ch, int path )
{
    std::vector<std::vector<int>> cover( lens.size() );
    for( size_t s = 0; s < lens.size(); s++ ) cover[s].assign( (size_t)lens[s], 0 );
    int last_set = -1;
    for( size_t c = 0; c < ch.size(); c++ ) {
        const psx_many_chunk q = ch[c];
        CHECK( q.set >= 0 && q.set < (int)lens.size() );
        if( q.set < 0 || q.set >= (int)lens.size() ) return;
        CHECK( q.r0 >= 0 && q.r1 > q.r0 && q.r1 <= lens[q.set] );
        if( path == 2 ) CHECK( q.r0 % PSX_MANYF_PRE_STEP == 0 );
        else CHECK( q.r0 % 32 == 0 && q.r1 - q.r0 <= 512 );
        if( q.set != last_set ) { CHECK( q.set > last_set && q.r0 == 0 ); last_set = q.set; }
        else CHECK( q.r0 == ch[c - 1].r1 );
        for( int r = q.r0; r < q.r1 && r < lens[q.set]; r++ ) cover[q.set][r]++;
    }
    for( size_t s = 0; s < lens.size(); s++ )
        for( int r = 0; r < lens[s]; r++ ) if( cover[s][r] != 1 ) { CHECK( cover[s][r] == 1 ); return; }
}

static void check_blocks( const std::vector<int>& lens, const std::vector<psx_many_block>& bl )
{
    std::vector<std::vector<int>> cover( lens.size() );
    for( size_t s = 0; s < lens.size(); s++ ) cover[s].assign( (size_t)lens[s], 0 );
    for( size_t b = 0; b < bl.size(); b++ ) {
        const psx_many_block q = bl[b];
        CHECK( q.set >= 0 && q.set < (int)lens.size() );
        if( q.set < 0 || q.set >= (int)lens.size() ) return;
        CHECK( q.row0 % 256 == 0 && q.row0 >= 0 && q.row0 < lens[q.set] );
        for( int r = q.row0; r < q.row0 + 256 && r < lens[q.set]; r++ ) cover[q.set][r]++;
    }
    for( size_t s = 0; s < lens.size(); s++ )
        for( int r = 0; r < lens[s]; r++ ) if( cover[s][r] != 1 ) { CHECK( cover[s][r] == 1 ); return; }
}

static void run( int l_len, const std::vector<int>& r_lens )
{
    const int K = (int)r_lens.size();
    const int* lens = K ? r_lens.data() : nullptr;
    long long rows = 0;
    for( int v : r_lens ) rows += v;
    for( int mfma = 0; mfma < 2; mfma++ ) {
        const int want = ( l_len == 0 || rows == 0 ) ? 0 : ( mfma && l_len >= 256 && rows >= 4096 ) ? 2 : 1;
        CHECK( psx_manyf_path( l_len, lens, K, mfma != 0 ) == want );
        for( int mutual = 0; mutual < 2; mutual++ ) {
            psx_many_f32_plan rep;
            CHECK( psx_many_f32_plan_host( l_len, lens, K, mutual ? PSX_PAIRS_MUTUAL : 0, mfma, &rep ) == PSX_OK );
            CHECK( rep.path == want );
            if( want == 0 ) { CHECK( rep.fwd_groups == 0 && rep.bwd_groups == 0 && rep.launches == 0 && rep.scratch_bytes == 0 ); continue; }
            psx_manyf_tables t;
            CHECK( psx_many_f32_build( l_len, lens, K, mutual != 0, want, t ) );
            const std::vector<int> lside( 1, l_len );
            check_chunks( r_lens, t.rchk, want );
            check_blocks( r_lens, t.rblk );
            check_blocks( lside, t.lblk );
            if( mutual ) check_chunks( lside, t.lchk, want ); else CHECK( t.lchk.empty() && t.bgroups.empty() );
            CHECK( rep.fwd_groups == (int)t.fgroups.size() && rep.bwd_groups == (int)t.bgroups.size() && rep.fwd_groups >= 1 );
            CHECK( rep.bwd_groups == ( mutual ? rep.bwd_groups : 0 ) && ( !mutual || rep.bwd_groups >= 1 ) );
            CHECK( rep.launches == ( want == 2 ? 2 : 1 ) + 2 * ( rep.fwd_groups + rep.bwd_groups ) + 3 );
            const long long unit = want == 2 ? PSX_MANYF_PRE_UNIT : PSX_MANYF_SCAN_UNIT;
            long long biggest = 0;
            int next_chunk = 0, next_set = -1;
            for( const psx_manyf_group& g : t.fgroups ) {                       // runs of whole sets, in order, all chunks
                CHECK( g.chunk0 == next_chunk && g.nchunks >= 1 && g.set0 > next_set && g.rows == l_len && g.row0 == 0 );
                CHECK( g.block0 == (int)t.rblk.size() && g.nblocks == (int)t.lblk.size() );
                CHECK( t.rchk[(size_t)g.chunk0].r0 == 0 && t.rchk[(size_t)g.chunk0].set == g.set0 );
                CHECK( t.rchk[(size_t)( g.chunk0 + g.nchunks - 1 )].set == g.set0 + g.nsets - 1 );
                next_chunk = g.chunk0 + g.nchunks; next_set = g.set0 + g.nsets - 1;
                const long long b = unit * g.nchunks * l_len;
                bool one_set = t.rchk[(size_t)g.chunk0].set == t.rchk[(size_t)( g.chunk0 + g.nchunks - 1 )].set;
                CHECK( b <= PSX_MANYF_BUDGET || one_set );
                if( b > biggest ) biggest = b;
            }
            CHECK( next_chunk == (int)t.rchk.size() );
            int next_block = 0; long long next_row = -1;
            for( const psx_manyf_group& g : t.bgroups ) {
                CHECK( g.block0 == next_block && g.nblocks >= 1 && g.row0 > next_row && g.rows >= 1 );
                CHECK( g.chunk0 == (int)t.rchk.size() && g.nchunks == (int)t.lchk.size() );
                CHECK( t.rblk[(size_t)g.block0].row0 == 0 && t.rblk[(size_t)g.block0].set == g.set0 );
                next_block = g.block0 + g.nblocks; next_row = g.row0;
                const long long b = unit * g.nchunks * g.rows;
                const bool one_set = t.rblk[(size_t)g.block0].set == t.rblk[(size_t)( g.block0 + g.nblocks - 1 )].set;
                CHECK( b <= PSX_MANYF_BUDGET || one_set );
                if( b > biggest ) biggest = b;
            }
            if( mutual ) CHECK( next_block == (int)t.rblk.size() );
            CHECK( rep.scratch_bytes == biggest && t.scratch_bytes == biggest );
        }
    }
}

int main()
{
    run( 300, { 257, 0, 1, 31, 32, 33, 63, 64, 65, 512, 513, 255, 256, 3000 } );
    run( 257, { 64, 1000, 300, 2800 } );
    run( 1, { 1, 2, 40 } );
    run( 2500, { 2300, 700, 1200 } );
    run( 255, { 4096 } );
    run( 256, { 4095 } );
    run( 256, { 4096 } );
    {
        std::vector<int> tiny;
        for( int i = 0; i < 200; i++ ) tiny.push_back( i % 41 );
        tiny.push_back( 4100 );
        run( 70, tiny );
        run( 300, tiny );
    }
    run( 18432, { 18432 } );
    run( 2048, std::vector<int>( 64, 2048 ) );
    run( 4096, std::vector<int>( 300, 4096 ) );               // above the budget both ways: several groups
    run( 0, { 5, 6 } );
    run( 7, {} );
    run( 9, { 0, 0, 0 } );
    {   // launches do not depend on the number of sets within one group
        psx_many_f32_plan a, b;
        const std::vector<int> k3( 3, 1400 ), k40( 40, 1400 );
        for( int mfma = 0; mfma < 2; mfma++ ) {
            CHECK( psx_many_f32_plan_host( 300, k3.data(), 3, PSX_PAIRS_MUTUAL, mfma, &a ) == PSX_OK );
            CHECK( psx_many_f32_plan_host( 300, k40.data(), 40, PSX_PAIRS_MUTUAL, mfma, &b ) == PSX_OK );
            CHECK( a.fwd_groups == 1 && b.fwd_groups == 1 && a.bwd_groups == 1 && b.bwd_groups == 1 && a.launches == b.launches );
        }
    }
    {   // what is refused: the report stays as it was
        psx_many_f32_plan rep;
        rep.path = -5;
        const int neg[2] = { 4, -1 }, big[2] = { INT_MAX, 1 }, ok[2] = { 3, 4 };
        CHECK( psx_many_f32_plan_host( 5, neg, 2, 0, 1, &rep ) == PSX_ERR_INVALID );
        CHECK( psx_many_f32_plan_host( 5, big, 2, 0, 1, &rep ) == PSX_ERR_INVALID );
        CHECK( psx_many_f32_plan_host( INT_MAX, ok, 2, 0, 1, &rep ) == PSX_ERR_INVALID );
        CHECK( psx_many_f32_plan_host( -1, ok, 2, 0, 1, &rep ) == PSX_ERR_INVALID );
        CHECK( psx_many_f32_plan_host( 5, ok, -1, 0, 1, &rep ) == PSX_ERR_INVALID );
        CHECK( psx_many_f32_plan_host( 5, nullptr, 2, 0, 1, &rep ) == PSX_ERR_INVALID );
        CHECK( psx_many_f32_plan_host( 5, ok, 2, 2, 1, &rep ) == PSX_ERR_INVALID );
        CHECK( psx_many_f32_plan_host( 5, ok, 2, 0, 2, &rep ) == PSX_ERR_INVALID );
        CHECK( psx_many_f32_plan_host( 5, ok, 2, 0, 1, nullptr ) == PSX_ERR_INVALID );
        CHECK( rep.path == -5 );
        CHECK( psx_many_f32_plan_host( 5, ok, 2, 0, 1, &rep ) == PSX_OK && rep.path == 1 && rep.launches == 6 );
    }
    std::printf( "%s\n", fails ? "FAILED" : "ALL OK" );
    return fails ? 1 : 0;
}
