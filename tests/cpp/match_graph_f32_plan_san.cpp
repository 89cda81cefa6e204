// Stand-alone check of match_graph_f32_plan.h (plain C++14, no HIP, its own main): compiled with
// -fsanitize=address,undefined by tests/test_match_graph_f32_cpu.py and run directly.  On the cases of
// tests/match_graph_f32_cases.py, both paths and both flag values, the tables are filled into exact-size heap arrays, as the
// library fills them, and checked entry by entry:
//   - the chunks of every referenced set are ascending, contiguous, cover it exactly, start at whole tiles (scan) or whole
//     staged blocks (prefilter) and are no longer than the call's chunk length; unreferenced sets have none;
//   - every (edge, block of the outer set, chunk of the inner set) triple is an item exactly once per direction, and where
//     an item's output goes stays inside its edge's entries, inside its group's buffer;
//   - the scan's partial (pbase + row) and the prefilter's segment ((base + row x nchunks + c - c0) x 2 + half) of every
//     (edge, row, chunk) are distinct within a group and below the group's entries;
//   - the groups are runs of whole edges in order, under the budget unless a single edge exceeds it;
//   - the rule at its edges, and the int overflow refusals.
#include "match_graph_f32_plan.h"

#include <cstdio>
#include <memory>
#include <vector>

static int fails = 0;
#define CHECK(c) do { if(!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); fails++; } } while(0)

typedef std::vector<int> Lens;
typedef std::vector<psx_view_edge> Edges;

static void check_case( const char* name, const Lens& lens, const Edges& edges, bool mutual, int path )
{
    const int N = (int)lens.size(), E = (int)edges.size();
    psx_graphf_tables t;
    CHECK( psx_graph_f32_build( lens.data(), N, edges.data(), E, mutual, path, t ) );
    if( t.path == 0 ) return;
    const int step = path == 2 ? PSX_MANYF_PRE_STEP : PSX_MANY_TILE;
    const long long unit = path == 2 ? PSX_MANYF_PRE_UNIT : PSX_MANYF_SCAN_UNIT;
    CHECK( t.chunk_len % step == 0 && t.chunk_len >= step && t.chunk_len <= ( path == 2 ? PSX_MANYF_PRE_MAX : PSX_MANY_CHUNK_MAX ) );
    if( path == 2 ) CHECK( t.chunk_len >= PSX_MANYF_PRE_MIN );
    // exact-size arrays: a write past a count is the sanitizer's to find
    std::unique_ptr<psx_many_chunk[]> chk( new psx_many_chunk[(size_t)t.chunks] );
    std::unique_ptr<psx_many_block[]> blk( new psx_many_block[(size_t)t.blocks] );
    CHECK( psx_graphf_chunks( t.eff.data(), N, path, t.chunk_len, chk.get(), t.chunks ) == t.chunks );
    CHECK( psx_many_blocks( t.eff.data(), N, blk.get(), t.blocks ) == t.blocks );
    long long rows = 0;
    for( int s = 0; s < N; s++ ) {
        const psx_graph_cut& c = t.cuts[(size_t)s];
        CHECK( t.foff[(size_t)s] == rows );
        rows += t.eff[(size_t)s];
        if( t.eff[(size_t)s] == 0 ) { CHECK( c.c0 == c.c1 && c.b0 == c.b1 ); continue; }
        int at = 0;
        for( int q = c.c0; q < c.c1; q++ ) {
            CHECK( chk[q].set == s && chk[q].r0 == at && chk[q].r0 % step == 0 && chk[q].r1 > chk[q].r0 && chk[q].r1 - chk[q].r0 <= t.chunk_len );
            at = chk[q].r1;
        }
        CHECK( at == t.eff[(size_t)s] );
        for( int q = c.b0; q < c.b1; q++ ) CHECK( blk[q].set == s && blk[q].row0 == ( q - c.b0 ) * PSX_MANY_BLOCK );
        CHECK( (long long)( c.b1 - c.b0 ) * PSX_MANY_BLOCK >= t.eff[(size_t)s] && (long long)( c.b1 - c.b0 - 1 ) * PSX_MANY_BLOCK < t.eff[(size_t)s] );
    }
    CHECK( rows == t.rows );
    for( int dir = 0; dir < ( mutual ? 2 : 1 ); dir++ ) {
        const std::vector<psx_graph_group>& groups = dir ? t.bg : t.fg;
        const long long NI = t.items[dir], NW = t.wgs[dir];
        std::unique_ptr<psx_graph_item[]> items( new psx_graph_item[(size_t)NI] );
        std::unique_ptr<psx_graph_wg[]> wgs( new psx_graph_wg[(size_t)NW] );
        CHECK( psx_graph_items( t.eff.data(), t.cuts.data(), t.ep.data(), E, dir, items.get(), NI ) == NI );
        CHECK( psx_graph_wgs( t.eff.data(), t.ep.data(), E, dir, wgs.get(), NW ) == NW );
        int edge = 0;
        long long item = 0, wg = 0;
        for( const psx_graph_group& g : groups ) {
            CHECK( g.edge0 == edge && g.item0 == item && g.wg0 == wg && g.nedges > 0 && g.nitems > 0 );
            CHECK( g.entries <= t.entries );
            std::vector<char> hit( (size_t)g.entries, 0 );               // every (edge, row, chunk) entry of the group, once
            int live = 0;
            long long sum = 0;
            for( int e = g.edge0; e < g.edge0 + g.nedges; e++ ) {
                if( !psx_graph_live( lens.data(), edges[e] ) ) continue;
                live++;
                const int o = dir ? edges[e].right : edges[e].left, i = dir ? edges[e].left : edges[e].right;
                const long long base = dir ? t.ep[(size_t)e].pb : t.ep[(size_t)e].pf;
                const int nc = t.cuts[(size_t)i].c1 - t.cuts[(size_t)i].c0, nb = t.cuts[(size_t)o].b1 - t.cuts[(size_t)o].b0;
                CHECK( base == sum );
                sum += (long long)nc * lens[o];
                for( int c = 0; c < nc; c++ )
                    for( int b = 0; b < nb; b++, item++ ) {
                        const psx_graph_item& it = items[item];
                        CHECK( it.edge == e && it.block == t.cuts[(size_t)o].b0 + b && it.chunk == t.cuts[(size_t)i].c0 + c );
                        CHECK( it.pbase == base + (long long)c * lens[o] );
                        for( int r = b * PSX_MANY_BLOCK; r < lens[o] && r < ( b + 1 ) * PSX_MANY_BLOCK; r++ ) {
                            // the scan's place and the prefilter's: both below the group's entries, each taken once
                            const long long scan = it.pbase + r, seg = base + (long long)r * nc + c;
                            CHECK( scan < g.entries && seg < g.entries );
                            const long long at = path == 2 ? seg : scan;
                            if( at < g.entries ) { CHECK( !hit[(size_t)at] ); hit[(size_t)at] = 1; }
                        }
                    }
                for( int b = 0; b < nb; b++, wg++ ) CHECK( wgs[wg].edge == e && wgs[wg].row0 == b * PSX_MANY_BLOCK );
                CHECK( ( dir ? t.ep[(size_t)e].jb0 : t.ep[(size_t)e].jf0 ) == wg - nb );
            }
            CHECK( sum == g.entries && live > 0 );
            for( char h : hit ) CHECK( h == 1 );
            if( unit * g.entries > PSX_MANYF_BUDGET ) CHECK( live == 1 );       // only a single edge may exceed the budget
            CHECK( item == g.item0 + g.nitems && wg == g.wg0 + g.nwgs );
            edge += g.nedges;
        }
        CHECK( item == NI && wg == NW );
        // every edge behind the last group is not live
        for( int e = edge; e < E; e++ ) CHECK( !psx_graph_live( lens.data(), edges[e] ) );
    }
    CHECK( t.scratch_bytes == unit * t.entries );
    CHECK( t.launches == ( path == 2 ? 2 : 1 ) + 2 * (int)( t.fg.size() + t.bg.size() ) + 3 );
    psx_graph_f32_plan_info info;
    CHECK( psx_graph_f32_plan_host( lens.data(), N, edges.data(), E, mutual ? PSX_PAIRS_MUTUAL : 0, 1, &info ) == PSX_OK );
    if( info.path == path ) CHECK( info.chunk_len == t.chunk_len && info.fwd_items == t.items[0] && info.launches == t.launches );
    std::printf( "%s mutual %d path %d: chunk length %d, %lld blocks, %lld chunks, %lld + %lld items, %zu + %zu groups\n", name, (int)mutual, path,
                 t.chunk_len, t.blocks, t.chunks, t.items[0], t.items[1], t.fg.size(), t.bg.size() );
}

static Edges all_pairs( int n ) { Edges e; for( int a = 0; a < n; a++ ) for( int b = a + 1; b < n; b++ ) e.push_back( { a, b } ); return e; }

int main()
{
    struct Case { const char* name; Lens lens; Edges edges; };
    std::vector<Case> cases;
    cases.push_back( { "mixed", { 300, 257, 0, 33, 513, 1 }, { { 3, 4 }, { 0, 1 }, { 4, 5 }, { 0, 0 }, { 0, 2 }, { 1, 0 }, { 5, 4 }, { 2, 0 }, { 4, 3 }, { 0, 1 } } } );
    cases.push_back( { "lefts", { 600, 1, 255, 256, 257, 300 }, { { 1, 0 }, { 2, 5 }, { 3, 0 }, { 4, 5 }, { 0, 5 }, { 4, 0 }, { 0, 3 } } } );
    cases.push_back( { "big", { 2500, 2300, 700 }, { { 0, 1 }, { 0, 2 }, { 1, 0 }, { 1, 2 }, { 2, 0 }, { 2, 1 } } } );
    {
        Case c = { "edges", { 3100, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 512, 513, 4097 }, {} };
        for( int s = 1; s < 17; s++ ) c.edges.push_back( { s, 0 } );
        c.edges.push_back( { 0, 0 } );
        for( int s = 1; s < 17; s++ ) c.edges.push_back( { 0, s } );
        c.edges.push_back( { 13, 16 } ); c.edges.push_back( { 0, 13 } ); c.edges.push_back( { 16, 13 } );
        cases.push_back( c );
    }
    {
        Case c = { "tiny400", {}, {} };
        for( int i = 0; i < 200; i++ ) c.lens.push_back( i % 41 );
        for( int i = 0; i < 400; i++ ) c.edges.push_back( { i % 200, ( 7 * i + 3 ) % 200 } );
        cases.push_back( c );
    }
    cases.push_back( { "groups12", { 18432 }, Edges( 12, psx_view_edge{ 0, 0 } ) } );
    cases.push_back( { "32x2048-all", Lens( 32, 2048 ), all_pairs( 32 ) } );
    cases.push_back( { "16x4096-all", Lens( 16, 4096 ), all_pairs( 16 ) } );
    {
        Case c = { "64x2048-next8", Lens( 64, 2048 ), {} };
        for( int a = 0; a < 64; a++ ) for( int b = a + 1; b < 64 && b < a + 9; b++ ) c.edges.push_back( { a, b } );
        cases.push_back( c );
    }
    {
        Case c = { "star64", Lens( 65, 2048 ), {} };
        for( int b = 1; b < 65; b++ ) c.edges.push_back( { 0, b } );
        cases.push_back( c );
    }
    cases.push_back( { "one-18432", { 18432, 18432 }, { { 0, 1 } } } );
    for( const Case& c : cases )
        for( int mutual = 0; mutual < 2; mutual++ )
            for( int path = 1; path <= 2; path++ ) check_case( c.name, c.lens, c.edges, mutual != 0, path );

    {   // the rule at its edges
        const psx_view_edge e01 = { 0, 1 };
        const int a[2] = { 255, 4096 }, b[2] = { 256, 4095 }, c[2] = { 256, 4096 }, d[2] = { 256, 2048 }, f[3] = { 256, 4096, 1 }, z[3] = { 256, 4096, 0 };
        const psx_view_edge two[2] = { { 0, 1 }, { 0, 1 } }, small[2] = { { 0, 1 }, { 2, 2 } }, dead[2] = { { 0, 2 }, { 2, 1 } };
        CHECK( psx_graphf_path( a, &e01, 1, true ) == 1 );
        CHECK( psx_graphf_path( b, &e01, 1, true ) == 1 );
        CHECK( psx_graphf_path( c, &e01, 1, true ) == 2 );
        CHECK( psx_graphf_path( d, two, 2, true ) == 2 );
        CHECK( psx_graphf_path( f, small, 2, true ) == 1 );          // the mean left side is below 256
        CHECK( psx_graphf_path( c, &e01, 1, false ) == 1 );
        CHECK( psx_graphf_path( z, dead, 2, true ) == 0 && psx_graphf_path( c, nullptr, 0, true ) == 0 );
        // a star is psx_manyf_path
        const int star[4] = { 300, 2000, 0, 2200 };
        const psx_view_edge se[3] = { { 0, 1 }, { 0, 2 }, { 0, 3 } };
        CHECK( psx_graphf_path( star, se, 3, true ) == psx_manyf_path( 300, star + 1, 3, true ) );
        // the plan ignores what no live edge names
        psx_graph_f32_plan_info p, q;
        const int l4[4] = { 40, 50, 60, 0 }, l1[1] = { 50 };
        const psx_view_edge e4[2] = { { 1, 1 }, { 0, 3 } }, e1[1] = { { 0, 0 } };
        CHECK( psx_graph_f32_plan_host( l4, 4, e4, 2, PSX_PAIRS_MUTUAL, 1, &p ) == PSX_OK && psx_graph_f32_plan_host( l1, 1, e1, 1, PSX_PAIRS_MUTUAL, 1, &q ) == PSX_OK );
        CHECK( p.path == 1 && p.referenced_sets == 1 && p.blocks == q.blocks && p.chunks == q.chunks && p.fwd_items == q.fwd_items && p.launches == 8 );
        // argument errors
        CHECK( psx_graph_f32_plan_host( l1, 1, e1, 1, 2, 1, &p ) == PSX_ERR_INVALID && psx_graph_f32_plan_host( l1, 1, e1, 1, 0, 2, &p ) == PSX_ERR_INVALID );
        CHECK( psx_graph_f32_plan_host( l1, 1, e1, 1, 0, 1, nullptr ) == PSX_ERR_INVALID && psx_graph_f32_plan_host( l1, 1, e4, 2, 0, 1, &p ) == PSX_ERR_INVALID );
    }
    {   // what does not fit an int is refused
        psx_graphf_tables t;
        psx_graph_f32_plan_info p;
        // the gathered rows of all referenced sets: 3 x (2^30 - 1) rows in three sets, two edges (each side's sum is below 2^31)
        const int big3[3] = { ( 1 << 30 ) - 1, ( 1 << 30 ) - 1, ( 1 << 30 ) - 1 };
        const psx_view_edge e3[2] = { { 0, 1 }, { 1, 2 } };
        CHECK( psx_graph_args_ok( big3, 3, e3, 2 ) );
        CHECK( !psx_graph_f32_build( big3, 3, e3, 2, true, 1, t ) && !psx_graph_f32_build( big3, 3, e3, 2, false, 2, t ) );
        CHECK( psx_graph_f32_plan_host( big3, 3, e3, 2, 0, 1, &p ) == PSX_ERR_NOMEM );
        // 32 x a group's segments: one edge of 2^19 x 2^19 rows has 2^19 x 128 (chunk, row) entries on the prefilter path,
        // 2^32 candidate slots; the scan path takes it (2^19 x 1024 entries fit an int)
        const int sq[2] = { 1 << 19, 1 << 19 };
        const psx_view_edge e01 = { 0, 1 };
        CHECK( !psx_graph_f32_build( sq, 2, &e01, 1, false, 2, t ) );
        CHECK( psx_graph_f32_build( sq, 2, &e01, 1, false, 1, t ) && t.fg.size() == 1 && t.entries == ( 1LL << 19 ) * 1024 );
        CHECK( psx_graph_f32_plan_host( sq, 2, &e01, 1, 0, 1, &p ) == PSX_ERR_NOMEM && psx_graph_f32_plan_host( sq, 2, &e01, 1, 0, 0, &p ) == PSX_OK );
        // the scan's entries of one group: 2^22 x 2^22 rows are 2^22 x 8192 entries = 2^35
        const int sq2[2] = { 1 << 22, 1 << 22 };
        CHECK( !psx_graph_f32_build( sq2, 2, &e01, 1, false, 1, t ) );
    }
    std::printf( "%s\n", fails ? "FAILED" : "ALL OK" );
    return fails ? 1 : 0;
}
