// Stand-alone program (its own main, no library): the plan of the pair search over an edge list,
// csrc/hip/match_graph_plan.h alone, built with -fsanitize=address,undefined by tests/test_match_graph_cpu.py and run
// directly.  Every table is a heap array of exactly the size the count-only form reports -- and of every smaller capacity (up
// to 40) -- so a write past an end is the sanitizer's to report.  The invariants are restated here:
//   - every row of every referenced set is covered exactly once by the blocks and once by the chunks, nothing spans two sets,
//     chunks are whole tiles of at most chunk_len <= 512 rows, a set's chunks ascending and contiguous, unreferenced sets absent;
//   - every (edge, block of the outer set, chunk of the inner set) triple appears exactly once per direction, and no other;
//   - an item's keys lie inside its group's partials and no two items of a group overlap;
//   - the per-edge row offsets are the prefix sums over the edges with two non-empty sides;
//   - the {edge, row0} tables are edge-major and cover every outer row of every such edge once;
//   - the groups are runs of whole edges within the budget (or a single edge), and tile the item and {edge, row0} tables;
//   - launches = 1 + 2 groups + 3.
#include "match_graph_plan.h"

#include <climits>
#include <cstdio>
#include <map>
#include <set>
#include <tuple>
#include <vector>

static int fails = 0;
#define CHECK(c) do { if(!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); fails++; } } while(0)

typedef std::vector<psx_view_edge> Edges;

static void run( const char* name, const std::vector<int>& lens, const Edges& edges, long long budget = PSX_GRAPH_PARTIAL_BUDGET )
{
    const int N = (int)lens.size(), E = (int)edges.size();
    for( int mutual = 0; mutual < 2; mutual++ ) {
        CHECK( psx_graph_args_ok( lens.data(), N, edges.data(), E ) );
        std::vector<int> eff( (size_t)N );
        const int nref = psx_graph_eff( lens.data(), N, edges.data(), E, eff.data() );
        std::set<int> ref;
        for( const psx_view_edge& e : edges ) if( lens[e.left] > 0 && lens[e.right] > 0 ) { ref.insert( e.left ); ref.insert( e.right ); }
        CHECK( nref == (int)ref.size() );
        for( int s = 0; s < N; s++ ) CHECK( eff[s] == ( ref.count( s ) ? lens[s] : 0 ) );
        const int cl = psx_graph_chunk_len( lens.data(), edges.data(), E, mutual != 0 );
        CHECK( cl >= 32 && cl <= 512 && cl % 32 == 0 );
        std::vector<psx_graph_cut> cuts( (size_t)N );
        long long B = -1, C = -1;
        CHECK( psx_graph_cuts( eff.data(), N, cl, cuts.data(), &B, &C ) );
        std::vector<psx_many_block> bl( (size_t)B );
        std::vector<psx_many_chunk> ch( (size_t)C );
        CHECK( psx_many_blocks( eff.data(), N, bl.data(), B ) == B );
        CHECK( psx_many_chunks_of( eff.data(), N, cl, ch.data(), C ) == C );
        // the cover, and the cuts name exactly each set's entries
        std::vector<std::vector<int>> bc( (size_t)N ), cc( (size_t)N );
        for( int s = 0; s < N; s++ ) { bc[s].assign( (size_t)lens[s], 0 ); cc[s].assign( (size_t)lens[s], 0 ); }
        for( long long b = 0; b < B; b++ ) {
            const psx_many_block q = bl[b];
            CHECK( q.set >= 0 && q.set < N && ref.count( q.set ) && q.row0 % 256 == 0 && q.row0 < lens[q.set] );
            CHECK( b >= cuts[q.set].b0 && b < cuts[q.set].b1 && q.row0 == 256 * ( b - cuts[q.set].b0 ) );
            for( int r = q.row0; r < q.row0 + 256 && r < lens[q.set]; r++ ) bc[q.set][r]++;
        }
        for( long long c = 0; c < C; c++ ) {
            const psx_many_chunk q = ch[c];
            CHECK( q.set >= 0 && q.set < N && ref.count( q.set ) && q.r0 % 32 == 0 && q.r0 >= 0 && q.r1 > q.r0 && q.r1 <= lens[q.set] && q.r1 - q.r0 <= cl );
            CHECK( c >= cuts[q.set].c0 && c < cuts[q.set].c1 );
            CHECK( c == cuts[q.set].c0 ? q.r0 == 0 : ( ch[c - 1].set == q.set && ch[c - 1].r1 == q.r0 ) );
            for( int r = q.r0; r < q.r1; r++ ) cc[q.set][r]++;
        }
        for( int s = 0; s < N; s++ ) {
            if( !ref.count( s ) ) { CHECK( cuts[s].b0 == cuts[s].b1 && cuts[s].c0 == cuts[s].c1 ); continue; }
            for( int r = 0; r < lens[s]; r++ ) if( bc[s][r] != 1 || cc[s][r] != 1 ) { CHECK( bc[s][r] == 1 && cc[s][r] == 1 ); break; }
        }
        // edges and groups: count, then exact-size fill
        std::vector<psx_graph_edge> ep( (size_t)E ), ep2( (size_t)E );
        long long nfg = -1, nbg = -1, items[2], wgs[2], entries = -1;
        CHECK( psx_graph_edges( lens.data(), cuts.data(), edges.data(), E, mutual != 0, budget, ep.data(), nullptr, 0, &nfg, nullptr, 0, &nbg, items, wgs, &entries ) );
        std::vector<psx_graph_group> fg( (size_t)nfg ), bg( (size_t)nbg );
        long long a = -1, b2 = -1, it2[2], wg2[2], en2 = -1;
        CHECK( psx_graph_edges( lens.data(), cuts.data(), edges.data(), E, mutual != 0, budget, ep2.data(), fg.data(), nfg, &a, bg.data(), nbg, &b2, it2, wg2, &en2 ) );
        CHECK( a == nfg && b2 == nbg && it2[0] == items[0] && it2[1] == items[1] && wg2[0] == wgs[0] && wg2[1] == wgs[1] && en2 == entries );
        if( !mutual ) CHECK( nbg == 0 && items[1] == 0 && wgs[1] == 0 );
        for( long long cap = 0; cap < nfg && cap < 40; cap++ ) {       // every smaller capacity: the totals stay, the prefix is the same
            std::vector<psx_graph_group> part( (size_t)cap ), pb( (size_t)( cap < nbg ? cap : nbg ) );
            CHECK( psx_graph_edges( lens.data(), cuts.data(), edges.data(), E, mutual != 0, budget, ep2.data(), part.data(), cap, &a, pb.data(), (long long)pb.size(), &b2, it2, wg2, &en2 ) );
            CHECK( a == nfg && b2 == nbg );
            for( long long g = 0; g < cap; g++ ) CHECK( part[g].item0 == fg[g].item0 && part[g].nitems == fg[g].nitems && part[g].entries == fg[g].entries );
        }
        long long foff = 0, boff = 0;
        for( int e = 0; e < E; e++ ) {
            CHECK( ep[e].left == edges[e].left && ep[e].right == edges[e].right && ep[e].foff == foff && ep[e].boff == boff );
            if( lens[edges[e].left] > 0 && lens[edges[e].right] > 0 ) { foff += lens[edges[e].left]; boff += lens[edges[e].right]; }
        }
        for( int dir = 0; dir < ( mutual ? 2 : 1 ); dir++ ) {
            const std::vector<psx_graph_group>& gr = dir ? bg : fg;
            const long long NI = items[dir], NW = wgs[dir];
            std::vector<psx_graph_item> it( (size_t)NI );
            std::vector<psx_graph_wg> wg( (size_t)NW );
            CHECK( psx_graph_items( eff.data(), cuts.data(), ep.data(), E, dir, nullptr, 0 ) == NI );
            CHECK( psx_graph_items( eff.data(), cuts.data(), ep.data(), E, dir, it.data(), NI ) == NI );
            CHECK( psx_graph_wgs( eff.data(), ep.data(), E, dir, nullptr, 0 ) == NW );
            CHECK( psx_graph_wgs( eff.data(), ep.data(), E, dir, wg.data(), NW ) == NW );
            for( long long cap = 0; cap < NI && cap < 40; cap++ ) {
                std::vector<psx_graph_item> part( (size_t)cap );
                std::vector<psx_graph_wg> pw( (size_t)( cap < NW ? cap : NW ) );
                CHECK( psx_graph_items( eff.data(), cuts.data(), ep.data(), E, dir, part.data(), cap ) == NI );
                CHECK( psx_graph_wgs( eff.data(), ep.data(), E, dir, pw.data(), (long long)pw.size() ) == NW );
                for( long long q = 0; q < cap; q++ ) CHECK( part[q].block == it[q].block && part[q].chunk == it[q].chunk && part[q].pbase == it[q].pbase && part[q].edge == it[q].edge );
                for( size_t q = 0; q < pw.size(); q++ ) CHECK( pw[q].edge == wg[q].edge && pw[q].row0 == wg[q].row0 );
            }
            // every (edge, block, chunk) triple exactly once, and no other
            std::set<std::tuple<int, int, int>> seen;
            long long want = 0;
            for( int e = 0; e < E; e++ ) {
                const int o = dir ? edges[e].right : edges[e].left, i = dir ? edges[e].left : edges[e].right;
                if( lens[o] > 0 && lens[i] > 0 ) want += (long long)( cuts[o].b1 - cuts[o].b0 ) * ( cuts[i].c1 - cuts[i].c0 );
            }
            CHECK( want == NI );
            // the groups tile both tables; an item's keys lie inside its group's partials, disjoint from every other item's
            long long item_at = 0, wg_at = 0;
            int edge_at = 0;
            for( const psx_graph_group& g : gr ) {
                CHECK( g.item0 == item_at && g.wg0 == wg_at && g.nitems > 0 && g.nwgs > 0 && g.edge0 >= edge_at && g.nedges >= 1 );
                CHECK( 8 * g.entries <= budget || g.nedges == 1 || g.nitems == 0 );
                CHECK( g.entries <= entries );
                std::map<long long, long long> spans;                  // pbase -> end, of this group
                for( long long q = g.item0; q < g.item0 + g.nitems && q < NI; q++ ) {
                    const psx_graph_item x = it[q];
                    CHECK( x.edge >= g.edge0 && x.edge < g.edge0 + g.nedges );
                    if( x.edge < 0 || x.edge >= E ) continue;
                    const int o = dir ? edges[x.edge].right : edges[x.edge].left, i = dir ? edges[x.edge].left : edges[x.edge].right;
                    CHECK( x.block >= cuts[o].b0 && x.block < cuts[o].b1 && x.chunk >= cuts[i].c0 && x.chunk < cuts[i].c1 );
                    CHECK( seen.insert( std::make_tuple( x.edge, x.block, x.chunk ) ).second );
                    CHECK( x.pbase >= 0 && (long long)x.pbase + lens[o] <= g.entries );
                    CHECK( x.pbase == ( dir ? ep[x.edge].pb : ep[x.edge].pf ) + (long long)( x.chunk - cuts[i].c0 ) * lens[o] );
                    spans[x.pbase] = (long long)x.pbase + lens[o];         // the blocks of one (edge, chunk) share a span
                }
                long long end = 0;
                for( const auto& sp : spans ) { CHECK( sp.first >= end ); end = sp.second; }
                for( long long q = g.wg0; q < g.wg0 + g.nwgs && q < NW; q++ ) CHECK( wg[q].edge >= g.edge0 && wg[q].edge < g.edge0 + g.nedges );
                item_at += g.nitems; wg_at += g.nwgs; edge_at = g.edge0 + g.nedges;
            }
            CHECK( item_at == NI && wg_at == NW && (long long)seen.size() == NI );
            // the {edge, row0} table: edge-major, every outer row of every live edge once
            long long q = 0;
            for( int e = 0; e < E; e++ ) {
                const int o = dir ? edges[e].right : edges[e].left, i = dir ? edges[e].left : edges[e].right;
                if( lens[o] <= 0 || lens[i] <= 0 ) continue;
                CHECK( ( dir ? ep[e].jb0 : ep[e].jf0 ) == q );
                for( int row0 = 0; row0 < lens[o]; row0 += 256, q++ ) CHECK( q < NW && wg[q].edge == e && wg[q].row0 == row0 );
            }
            CHECK( q == NW );
        }
        // the report
        psx_graph_plan_info info;
        CHECK( psx_graph_plan_host( lens.data(), N, edges.data(), E, mutual ? PSX_PAIRS_MUTUAL : 0, &info ) == PSX_OK );
        if( budget == PSX_GRAPH_PARTIAL_BUDGET && nref > 0 ) {
            CHECK( info.referenced_sets == nref && info.blocks == B && info.chunks == C && info.chunk_len == cl );
            CHECK( info.fwd_items == items[0] && info.bwd_items == items[1] && info.fwd_groups == nfg && info.bwd_groups == nbg );
            CHECK( info.join_workgroups == wgs[0] && info.launches == 4 + 2 * ( nfg + nbg ) && info.scratch_bytes == 8 * entries );
        }
        if( nref == 0 ) CHECK( info.launches == 0 && info.fwd_items == 0 && info.scratch_bytes == 0 );
        std::printf( "%s mutual %d: %d sets, chunk %d, %lld blocks, %lld chunks, items %lld / %lld, groups %lld / %lld, join %lld\n", name, mutual, nref,
                     cl, B, C, items[0], items[1], nfg, nbg, wgs[0] );
    }
}

int main()
{
    run( "mixed", { 300, 257, 0, 33, 513, 1 }, { {3,4}, {0,1}, {4,5}, {0,0}, {0,2}, {1,0}, {5,4}, {2,0}, {4,3}, {0,1} } );
    run( "lefts", { 600, 1, 255, 256, 257, 300 }, { {1,0}, {2,5}, {3,0}, {4,5}, {0,5}, {4,0}, {0,3} } );
    run( "big", { 2500, 2300, 700 }, { {0,1}, {0,2}, {1,0}, {1,2}, {2,0}, {2,1} } );
    {
        std::vector<int> tiny;
        Edges e;
        for( int i = 0; i < 200; i++ ) tiny.push_back( i % 41 );
        for( int i = 0; i < 400; i++ ) e.push_back( psx_view_edge{ i % 200, ( 7 * i + 3 ) % 200 } );
        run( "tiny400", tiny, e );
        run( "tiny400 small budget", tiny, e, 4096 );            // many groups, some of a single edge
    }
    {
        Edges e;
        for( int a = 0; a < 32; a++ ) for( int b = a + 1; b < 32; b++ ) e.push_back( psx_view_edge{ a, b } );
        run( "32x2048 all pairs", std::vector<int>( 32, 2048 ), e );
    }
    run( "budget", { 18432 }, Edges( 64, psx_view_edge{ 0, 0 } ) );
    run( "unreferenced", { 40, 50, 60, 0 }, { {1,1}, {0,3} } );  // set 0 only faces an empty set, set 2 is not named
    run( "nothing", { 5, 0 }, { {0,1}, {1,0}, {1,1} } );
    run( "no edges", { 5, 6 }, {} );
    run( "no sets", {}, {} );
    {   // the budget case runs in two groups per direction, as the GPU test expects
        psx_graph_plan_info info;
        const int len = 18432;
        const Edges e( 64, psx_view_edge{ 0, 0 } );
        CHECK( psx_graph_plan_host( &len, 1, e.data(), 64, PSX_PAIRS_MUTUAL, &info ) == PSX_OK );
        CHECK( info.fwd_groups == 2 && info.bwd_groups == 2 && info.launches == 12 && info.chunk_len == 512 && info.chunks == 36 && info.blocks == 72 );
        CHECK( info.scratch_bytes <= PSX_GRAPH_PARTIAL_BUDGET && info.scratch_bytes > PSX_GRAPH_PARTIAL_BUDGET / 2 );
    }
    {   // what is refused: nothing is written
        psx_graph_plan_info info;
        info.launches = -5;
        const int ok[2] = { 3, 4 }, neg[2] = { 3, -1 }, big[2] = { INT_MAX, 1 };
        const psx_view_edge e01[2] = { {0,1}, {1,0} }, out_hi[1] = { {0,2} }, out_lo[1] = { {-1,0} }, twice[2] = { {0,1}, {0,0} };
        CHECK( psx_graph_plan_host( ok, 2, e01, 2, 0, nullptr ) == PSX_ERR_INVALID );
        CHECK( psx_graph_plan_host( ok, 2, e01, 2, 2, &info ) == PSX_ERR_INVALID );
        CHECK( psx_graph_plan_host( ok, -1, e01, 2, 0, &info ) == PSX_ERR_INVALID );
        CHECK( psx_graph_plan_host( ok, 2, e01, -1, 0, &info ) == PSX_ERR_INVALID );
        CHECK( psx_graph_plan_host( nullptr, 2, e01, 2, 0, &info ) == PSX_ERR_INVALID );
        CHECK( psx_graph_plan_host( ok, 2, nullptr, 2, 0, &info ) == PSX_ERR_INVALID );
        CHECK( psx_graph_plan_host( neg, 2, e01, 2, 0, &info ) == PSX_ERR_INVALID );
        CHECK( psx_graph_plan_host( ok, 2, out_hi, 1, 0, &info ) == PSX_ERR_INVALID );
        CHECK( psx_graph_plan_host( ok, 2, out_lo, 1, 0, &info ) == PSX_ERR_INVALID );
        CHECK( psx_graph_plan_host( nullptr, 0, e01, 2, 0, &info ) == PSX_ERR_INVALID );          // no sets: no edge is in range
        CHECK( psx_graph_plan_host( big, 2, twice, 2, 0, &info ) == PSX_ERR_INVALID );            // sum of lens[left] above INT_MAX
        CHECK( info.launches == -5 );
        CHECK( psx_graph_plan_host( ok, 2, e01, 2, PSX_PAIRS_MUTUAL, &info ) == PSX_OK && info.launches == 8 );
        CHECK( psx_graph_plan_host( ok, 2, e01, 2, 0, &info ) == PSX_OK && info.launches == 6 );
    }
    std::printf( "%s\n", fails ? "FAILED" : "ALL OK" );
    return fails ? 1 : 0;
}
