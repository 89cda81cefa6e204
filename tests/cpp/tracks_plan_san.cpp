// Stand-alone program (its own main, no library): the host side of the tracks call -- csrc/hip/tracks_plan.h and the
// plain-C++ headers it includes, nothing else -- built with -fsanitize=address,undefined by tests/test_tracks_cpu.py and
// run directly.  Never loaded into Python, never run on a GPU.  Every array is a heap array of the exact size, so a read or
// write past an end is the sanitizer's to report:
//   - the plan on the edge-boundary shapes: counts of 0, 1, 255, 256, 257 and 513 records, views of 0, 1, 63, 64, 65 and
//     257 rows, against figures worked out here, and the block table it counts: no block crosses an edge;
//   - the host reference on those shapes against a quadratic labelling that shares nothing with it, at the exact
//     capacities, one short of each (the member cut inside a track), at 0 with buffers and at 0 with NULL;
//   - a record that is in range for a longer view but outside its own edge's refuses the call with nothing written;
//   - what the argument checks refuse.
#include "tracks_plan.h"

#include <cstdio>
#include <cstring>
#include <vector>

static int fails = 0;
#define CHECK(c) do { if(!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); fails++; } } while(0)

static const int S = 7, E = 9;
static const int LENS[S] = { 0, 1, 63, 64, 65, 257, 64 };
static const psx_view_edge EDGES[E] = { { 5, 4 }, { 2, 3 }, { 0, 3 }, { 3, 4 }, { 1, 2 }, { 4, 5 }, { 5, 5 }, { 2, 4 }, { 5, 6 } };
static const int COUNTS[E] = { 513, 255, 0, 256, 1, 257, 64, 0, 64 };

// exact-size heap copies: a sanitizer sees every index
template <class T> static T* heap( const T* src, size_t n )
{
    T* p = new T[n ? n : 1];
    for( size_t i = 0; i < n; i++ ) p[i] = src[i];
    return p;
}

static void check_plan()
{
    int* lens = heap( LENS, S );
    int* counts = heap( COUNTS, E );
    psx_tracks_plan_info p;
    CHECK( psx_tracks_plan_host( lens, S, counts, E, &p ) == PSX_OK );
    // 514 nodes; 1410 records; blocks 3 + 1 + 0 + 1 + 1 + 2 + 1 + 0 + 1; 2^9 < 514 <= 2^10
    CHECK( p.nodes == 514 && p.records == 1410 && p.record_blocks == 10 && p.sort_bits == 10 && p.launches == 7 );
    // tables 16 * 9 + 16 * 10 + 32; nodes 6 * 4 * 514; sort 4 * 4 * 514; totals 4 * (4 * 3 + 2); state 32
    CHECK( p.scratch_bytes == 336 + 12336 + 8224 + 56 + 32 );
    psx_ransac_block* blocks = new psx_ransac_block[10];
    CHECK( psx_ransac_many_blocks( counts, E, 1, PSX_TRACKS_ROWS, blocks, 10 ) == 10 );
    std::vector<int> cover( 1410, 0 ), first( E + 1, 0 );
    for( int e = 0; e < E; e++ ) first[e + 1] = first[e] + counts[e];
    for( int b = 0; b < 10; b++ ) {
        const psx_ransac_block& k = blocks[b];
        CHECK( k.set >= 0 && k.set < E && first[k.set] <= k.first && k.first < k.end && k.end <= first[k.set + 1] && k.end - k.first <= 256 );
        for( int i = k.first; i < k.end; i++ ) cover[(size_t)i]++;
    }
    for( int i = 0; i < 1410; i++ ) CHECK( cover[(size_t)i] == 1 );
    delete[] blocks;
    // sort bits at the powers of two
    CHECK( psx_tracks_sort_bits( 1 ) == 1 && psx_tracks_sort_bits( 2 ) == 1 && psx_tracks_sort_bits( 3 ) == 2 && psx_tracks_sort_bits( 256 ) == 8 &&
           psx_tracks_sort_bits( 257 ) == 9 && psx_tracks_sort_bits( 0x3fffffff ) == 30 );
    // a call with nothing to join plans nothing
    int* zero = new int[E]();
    CHECK( psx_tracks_plan_host( lens, S, zero, E, &p ) == PSX_OK && p.nodes == 514 && p.records == 0 && p.record_blocks == 0 && p.launches == 0 &&
           p.scratch_bytes == 0 );
    CHECK( psx_tracks_plan_host( nullptr, 0, nullptr, 0, &p ) == PSX_OK && p.nodes == 0 && p.sort_bits == 1 );
    CHECK( psx_tracks_plan_host( lens, S, counts, E, nullptr ) == PSX_ERR_INVALID );
    CHECK( psx_tracks_plan_host( lens, -1, counts, E, &p ) == PSX_ERR_INVALID && psx_tracks_plan_host( nullptr, S, counts, E, &p ) == PSX_ERR_INVALID );
    zero[3] = -1;
    CHECK( psx_tracks_plan_host( lens, S, zero, E, &p ) == PSX_ERR_INVALID );
    int big[2] = { 0x3fffffff, 1 };
    CHECK( psx_tracks_plan_host( big, 2, nullptr, 0, &p ) == PSX_ERR_INVALID && psx_tracks_plan_host( lens, S, big, 2, &p ) == PSX_ERR_INVALID );
    delete[] zero; delete[] lens; delete[] counts;
}

// the records of the edge-boundary case: strides walk the views, a self edge with self-loops, one clean edge
static psx_match_pair_u8* make_records( int total )
{
    psx_match_pair_u8* rec = new psx_match_pair_u8[(size_t)total];
    int at = 0;
    for( int e = 0; e < E; e++ ) {
        const int la = LENS[EDGES[e].left] > 0 ? LENS[EDGES[e].left] : 1, lb = LENS[EDGES[e].right] > 0 ? LENS[EDGES[e].right] : 1;
        for( int i = 0; i < COUNTS[e]; i++, at++ ) {
            int l = ( i * 5 + e ) % la, r = ( i * 3 + 1 ) % lb;
            if( e == 6 ) { l = 200 + i % 57; r = i % 9 ? l : 200; }          // self-loops, a same-view join at every 9th
            if( e == 8 ) { l = 100 + i; r = i; }                               // clean pairs on rows that nothing else touches
            if( e == 0 || e == 5 ) { l %= 90; r %= 90; }
            rec[at].left = l; rec[at].right = r; rec[at].d1 = -at; rec[at].d2 = 0x7fffffff;
        }
    }
    return rec;
}

// labels by repeated relabelling until nothing changes: comp[g] = the smallest node of g's component
static std::vector<int> brute_components( const psx_match_pair_u8* rec, const std::vector<int>& off, int M, int* joined )
{
    std::vector<int> comp( (size_t)M );
    for( int g = 0; g < M; g++ ) comp[(size_t)g] = g;
    *joined = 0;
    bool first = true;
    for( bool changed = true; changed; first = false ) {
        changed = false;
        int at = 0;
        for( int e = 0; e < E; e++ )
            for( int i = 0; i < COUNTS[e]; i++, at++ ) {
                const size_t a = (size_t)( off[(size_t)EDGES[e].left] + rec[at].left ), b = (size_t)( off[(size_t)EDGES[e].right] + rec[at].right );
                if( first && a != b ) ( *joined )++;
                const int m = comp[a] < comp[b] ? comp[a] : comp[b];
                if( comp[a] != m || comp[b] != m ) { comp[a] = comp[b] = m; changed = true; }
            }
    }
    return comp;
}

static void check_host( int min_views, int flags )
{
    int total = 0, M = 0;
    for( int e = 0; e < E; e++ ) total += COUNTS[e];
    std::vector<int> off( S + 1, 0 ), view;
    for( int s = 0; s < S; s++ ) { off[(size_t)s + 1] = off[(size_t)s] + LENS[s]; for( int r = 0; r < LENS[s]; r++ ) view.push_back( s ); }
    M = off[S];
    psx_match_pair_u8* rec = make_records( total );
    int* lens = heap( LENS, S );
    int* counts = heap( COUNTS, E );
    psx_view_edge* edges = heap( EDGES, E );
    const psx_track_opts o = { min_views, flags };

    // what the rule says, from the brute-force components
    int joined = 0;
    const std::vector<int> comp = brute_components( rec, off, M, &joined );
    psx_tracks_info want = { 0, 0, 0, 0, 0, joined };
    std::vector<int> wstarts( 1, 0 ), wlabels( (size_t)M, -1 );
    std::vector<psx_track_member> wmem;
    for( int r = 0; r < M; r++ ) {
        if( comp[(size_t)r] != r ) continue;
        std::vector<int> mem;
        for( int g = r; g < M; g++ ) if( comp[(size_t)g] == r ) mem.push_back( g );
        if( mem.size() < 2 ) continue;
        int views = 1, conflict = 0;
        for( size_t i = 1; i < mem.size(); i++ ) {
            if( view[(size_t)mem[i]] == view[(size_t)mem[i - 1]] ) conflict = 1; else views++;
        }
        want.components++; want.conflicts += conflict; want.too_few_views += views < min_views;
        if( views < min_views || ( conflict && !( flags & PSX_TRACKS_KEEP_CONFLICTS ) ) ) continue;
        for( int g : mem ) { wlabels[(size_t)g] = want.tracks; wmem.push_back( psx_track_member{ view[(size_t)g], g - off[(size_t)view[(size_t)g]] } ); }
        want.tracks++;
        wstarts.push_back( (int)wmem.size() );
    }
    want.members = (int)wmem.size();
    CHECK( want.components >= 60 && want.conflicts >= 1 );

    const int caps[5][2] = { { want.tracks, want.members }, { want.tracks, want.members - 1 }, { want.tracks - 1, want.members }, { 0, 0 }, { -1, -1 } };
    for( int c = 0; c < 5; c++ ) {
        const bool null = c == 4;                                              // capacity 0 with NULL: "how many?"
        if( !null && ( caps[c][0] < 0 || caps[c][1] < 0 ) ) continue;         // no track to be short of
        const int tcap = null ? 0 : caps[c][0], mcap = null ? 0 : caps[c][1];
        int* labels = new int[(size_t)M];
        int* starts = null ? nullptr : new int[(size_t)tcap + 1];
        psx_track_member* mem = null ? nullptr : new psx_track_member[mcap ? (size_t)mcap : 1];
        psx_tracks_info got = { -1, -1, -1, -1, -1, -1 };
        CHECK( psx_tracks_host( rec, counts, edges, E, lens, S, &o, c % 2 ? nullptr : labels, starts, tcap, mem, mcap, &got ) == PSX_OK );
        CHECK( std::memcmp( &got, &want, sizeof got ) == 0 );
        if( c % 2 == 0 ) for( int g = 0; g < M; g++ ) CHECK( labels[g] == wlabels[(size_t)g] );
        if( !null ) {
            for( int t = 0; t <= want.tracks && t <= tcap; t++ ) CHECK( starts[t] == wstarts[(size_t)t] );
            for( int i = 0; i < want.members && i < mcap; i++ ) CHECK( mem[i].view == wmem[(size_t)i].view && mem[i].row == wmem[(size_t)i].row );
        }
        delete[] labels; delete[] starts; delete[] mem;
    }

    // right == its own edge's right length, in range for the longer view 5: the whole call is refused, nothing written
    {
        psx_match_pair_u8* bad = heap( rec, (size_t)total );
        const int at = COUNTS[0] + 100;                                         // a record of edge 1 = (2, 3)
        bad[at].right = LENS[3];
        CHECK( LENS[3] < LENS[5] );
        int* labels = new int[(size_t)M];
        for( int g = 0; g < M; g++ ) labels[g] = -7;
        int starts[2] = { -7, -7 };
        psx_track_member mem[1] = { { -7, -7 } };
        psx_tracks_info got = { -7, -7, -7, -7, -7, -7 };
        CHECK( psx_tracks_host( bad, counts, edges, E, lens, S, &o, labels, starts, 1, mem, 1, &got ) == PSX_ERR_INVALID );
        bad[at].right = -1;
        CHECK( psx_tracks_host( bad, counts, edges, E, lens, S, &o, labels, starts, 1, mem, 1, &got ) == PSX_ERR_INVALID );
        for( int g = 0; g < M; g++ ) CHECK( labels[g] == -7 );
        CHECK( starts[0] == -7 && starts[1] == -7 && mem[0].view == -7 && got.tracks == -7 && got.joined_records == -7 );
        delete[] labels; delete[] bad;
    }
    delete[] rec; delete[] lens; delete[] counts; delete[] edges;
}

static void check_arguments()
{
    int* lens = heap( LENS, S );
    int* counts = heap( COUNTS, E );
    psx_view_edge* edges = heap( EDGES, E );
    int total = 0;
    for( int e = 0; e < E; e++ ) total += COUNTS[e];
    psx_match_pair_u8* rec = make_records( total );
    psx_track_opts o = { 2, 0 };
    psx_tracks_info info = { -7, -7, -7, -7, -7, -7 };
    int starts[4];
    psx_track_member mem[4];
    auto call = [&]( const void* p, const int* c, const psx_view_edge* ed, int ne, const int* l, int ns, const psx_track_opts* op, int* st, int tc,
                     psx_track_member* m, int mc, psx_tracks_info* in ) { return psx_tracks_host( p, c, ed, ne, l, ns, op, nullptr, st, tc, m, mc, in ); };
    CHECK( call( rec, counts, edges, E, lens, S, &o, starts, 3, mem, 4, &info ) == PSX_OK );
    CHECK( call( nullptr, counts, edges, E, lens, S, &o, starts, 3, mem, 4, &info ) == PSX_ERR_INVALID );
    CHECK( call( rec, nullptr, edges, E, lens, S, &o, starts, 3, mem, 4, &info ) == PSX_ERR_INVALID );
    CHECK( call( rec, counts, nullptr, E, lens, S, &o, starts, 3, mem, 4, &info ) == PSX_ERR_INVALID );
    CHECK( call( rec, counts, edges, -1, lens, S, &o, starts, 3, mem, 4, &info ) == PSX_ERR_INVALID );
    CHECK( call( rec, counts, edges, E, nullptr, S, &o, starts, 3, mem, 4, &info ) == PSX_ERR_INVALID );
    CHECK( call( rec, counts, edges, E, lens, S - 1, &o, starts, 3, mem, 4, &info ) == PSX_ERR_INVALID );      // edges name view 6
    CHECK( call( rec, counts, edges, E, lens, S, nullptr, starts, 3, mem, 4, &info ) == PSX_ERR_INVALID );
    CHECK( call( rec, counts, edges, E, lens, S, &o, starts, 3, mem, 4, nullptr ) == PSX_ERR_INVALID );
    CHECK( call( rec, counts, edges, E, lens, S, &o, nullptr, 3, mem, 4, &info ) == PSX_ERR_INVALID );
    CHECK( call( rec, counts, edges, E, lens, S, &o, starts, 3, nullptr, 4, &info ) == PSX_ERR_INVALID );
    CHECK( call( rec, counts, edges, E, lens, S, &o, starts, -1, mem, 4, &info ) == PSX_ERR_INVALID );
    CHECK( call( rec, counts, edges, E, lens, S, &o, starts, 3, mem, -1, &info ) == PSX_ERR_INVALID );
    psx_track_opts bad = { 1, 0 };
    CHECK( call( rec, counts, edges, E, lens, S, &bad, starts, 3, mem, 4, &info ) == PSX_ERR_INVALID );
    bad = psx_track_opts{ 2, 2 };
    CHECK( call( rec, counts, edges, E, lens, S, &bad, starts, 3, mem, 4, &info ) == PSX_ERR_INVALID );
    counts[2] = 1;                                                              // a record on the edge with an empty side
    CHECK( call( rec, counts, edges, E, lens, S, &o, starts, 3, mem, 4, &info ) == PSX_ERR_INVALID );
    counts[2] = 0; counts[7] = -1;
    CHECK( call( rec, counts, edges, E, lens, S, &o, starts, 3, mem, 4, &info ) == PSX_ERR_INVALID );
    delete[] rec; delete[] lens; delete[] counts; delete[] edges;
}

int main()
{
    check_plan();
    for( int mv = 2; mv <= 3; mv++ )
        for( int flags = 0; flags < 2; flags++ ) check_host( mv, flags );
    check_arguments();
    std::printf( "%s\n", fails ? "FAILED" : "ALL OK" );
    return fails ? 1 : 0;
}
