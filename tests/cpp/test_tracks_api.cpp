// Test of FeaturesDev::buildTracks through the C++ host API: its argument errors (an edge index out of range, a size
// mismatch, a null referenced entry, views on different devices, min_views < 2) and its empty forms -- all before a
// device is touched (this part runs without a GPU).
// With POPSIFT_TEST_EXPECT_GPU set (the -m gpu test): four views of a synthetic frame go through PopSift in MatchingMode;
// over an unsorted edge list -- both orders of a pair, a self edge, a duplicate, an empty view -- the tracks of the lists
// matchPairsGraph returns, and of the inliers of estimateHomographyGraph, equal a union-find looped over `matches` on the
// host: starts, members, labels and the six totals.
#include <popsift/popsift.h>
#include <popsift/features.h>
#include <popsift/sift_conf.h>
#include <popsift_hip.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <string>
#include <utility>
#include <vector>

static int fails = 0;
#define CHECK(c) do { if(!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); fails++; } } while(0)

template <class F> static std::string runtime_error_of( F f )
{
    try { f(); } catch( const std::runtime_error& e ) { return std::string( "E:" ) + e.what(); } catch( ... ) { return ""; }
    return "";
}

typedef std::vector<std::pair<int,int>> Edges;
typedef std::vector<std::vector<popsift::Match>> Lists;
typedef popsift::FeaturesDev FD;

static bool has( const std::string& s, const char* what ) { return s.find( what ) != std::string::npos; }

// the rule on the host: components as sets of (view, descriptor), looped over the matches
static popsift::Tracks host_tracks( const std::vector<int>& lens, const Edges& edges, const Lists& matches, const popsift::TrackOptions& opts )
{
    typedef std::pair<int,int> Node;
    std::map<Node, Node> rep;
    auto find = [&]( Node x ) { while( rep.count( x ) && rep[x] != x ) x = rep[x]; return x; };
    popsift::Tracks t;
    t.joined_records = 0;
    for( size_t e = 0; e < edges.size(); e++ )
        for( const popsift::Match& m : matches[e] ) {
            const Node a( edges[e].first, m.left_descriptor ), b( edges[e].second, m.right_descriptor );
            if( a == b ) continue;
            t.joined_records++;
            const Node ra = find( a ), rb = find( b );
            if( ra != rb ) rep[std::max( ra, rb )] = std::min( ra, rb );
        }
    std::map<Node, std::vector<Node>> comps;                 // by smallest member: view-major node order is the pair order
    t.view_offsets.assign( lens.size() + 1, 0 );
    for( size_t v = 0; v < lens.size(); v++ ) {
        t.view_offsets[v + 1] = t.view_offsets[v] + lens[v];
        for( int d = 0; d < lens[v]; d++ ) comps[find( Node( (int)v, d ) )].push_back( Node( (int)v, d ) );
    }
    t.labels.assign( (size_t)t.view_offsets[lens.size()], -1 );
    t.starts.assign( 1, 0 );
    t.n_tracks = t.n_members = t.components = t.conflicts = t.too_few_views = 0;
    for( const auto& c : comps ) {
        if( c.second.size() < 2 ) continue;
        std::set<int> views;
        for( const Node& n : c.second ) views.insert( n.first );
        const bool conflict = views.size() < c.second.size(), few = (int)views.size() < opts.min_views;
        t.components++; t.conflicts += conflict; t.too_few_views += few;
        if( few || ( conflict && !opts.keep_conflicts ) ) continue;
        for( const Node& n : c.second ) {
            t.labels[(size_t)t.view_offsets[n.first] + n.second] = t.n_tracks;
            popsift::TrackMember m; m.view = n.first; m.descriptor = n.second;
            t.members.push_back( m );
        }
        t.n_tracks++;
        t.starts.push_back( (int)t.members.size() );
    }
    t.n_members = (int)t.members.size();
    return t;
}

static bool same( const popsift::Tracks& a, const popsift::Tracks& b )
{
    if( a.n_tracks != b.n_tracks || a.n_members != b.n_members || a.components != b.components || a.conflicts != b.conflicts ||
        a.too_few_views != b.too_few_views || a.joined_records != b.joined_records )
        return false;
    if( a.starts != b.starts || a.labels != b.labels || a.view_offsets != b.view_offsets || a.members.size() != b.members.size() ) return false;
    for( size_t i = 0; i < a.members.size(); i++ )
        if( a.members[i].view != b.members[i].view || a.members[i].descriptor != b.members[i].descriptor ) return false;
    return true;
}

int main()
{
    const bool gpu = std::getenv( "POPSIFT_TEST_EXPECT_GPU" ) != nullptr;
    {   // argument errors, in the file:line + message format, before any device call
        FD a, b, c;
        const std::string e0 = runtime_error_of( [&]{ FD::buildTracks( { &a, &b }, Edges{ {0,1}, {0,2} }, Lists( 2 ) ); } );
        CHECK( has( e0, "features.cpp:" ) && has( e0, "buildTracks" ) && has( e0, "out of range" ) );
        CHECK( has( runtime_error_of( [&]{ FD::buildTracks( { &a, &b }, Edges{ {-1,1} }, Lists( 1 ) ); } ), "out of range" ) );
        CHECK( has( runtime_error_of( [&]{ FD::buildTracks( { &a, &b }, Edges{ {0,1} }, Lists( 2 ) ); } ), "buildTracks: 1 edges but 2 match lists" ) );
        CHECK( has( runtime_error_of( [&]{ FD::buildTracks( { &a, nullptr }, Edges{ {0,1} }, Lists( 1 ) ); } ), "null argument" ) );
        c.setDevice( 1 );
        CHECK( has( runtime_error_of( [&]{ FD::buildTracks( { &a, &b, &c }, Edges{ {0,1}, {1,2} }, Lists( 2 ) ); } ), "different devices" ) );
        c.setDevice( 0 );
        popsift::TrackOptions bad;
        bad.min_views = 1;
        CHECK( has( runtime_error_of( [&]{ FD::buildTracks( { &a, &b }, Edges{ {0,1} }, Lists( 1 ), bad ); } ), "invalid options" ) );
        // empty lists, a null entry that no edge names, no edges, no views: no tracks, no device call
        const popsift::Tracks t = FD::buildTracks( { &a, nullptr, &b }, Edges{ {0,2}, {2,0} }, Lists( 2 ) );
        CHECK( t.n_tracks == 0 && t.n_members == 0 && t.components == 0 && t.conflicts == 0 && t.too_few_views == 0 && t.joined_records == 0 );
        CHECK( t.starts == std::vector<int>( 1, 0 ) && t.members.empty() && t.labels.empty() && t.view_offsets == std::vector<int>( 4, 0 ) );
        const popsift::Tracks t0 = FD::buildTracks( {}, Edges{}, Lists() );
        CHECK( t0.n_tracks == 0 && t0.starts.size() == 1 && t0.view_offsets.size() == 1 );
        // a match in an empty object: its descriptor index lies outside
        Lists one( 1 );
        one[0].resize( 1 );
        one[0][0].left_descriptor = one[0][0].right_descriptor = 0;
        CHECK( has( runtime_error_of( [&]{ FD::buildTracks( { &a, &b }, Edges{ {0,1} }, one ); } ), "buildTracks failed" ) );
    }
    if( gpu ) {
        const int w = 320, h = 240;
        std::vector<unsigned char> img( (size_t)w * h );
        unsigned s = 4711u;
        std::vector<unsigned char> coarse( (size_t)( w / 8 + 2 ) * ( h / 8 + 2 ) );
        for( auto& c : coarse ) { s = s * 1664525u + 1013904223u; c = (unsigned char)( s >> 24 ); }
        for( int y = 0; y < h; y++ ) for( int x = 0; x < w; x++ ) {
            const int cw = w / 8 + 2;
            const int v = ( 3 * coarse[(size_t)( y / 8 ) * cw + x / 8] + coarse[(size_t)( y / 5 % ( h / 8 ) ) * cw + ( x / 3 ) % ( w / 8 )] ) / 4;
            img[(size_t)y * w + x] = (unsigned char)v;
        }
        popsift::Config cfg;
        cfg.setOctaves( 3 );
        cfg.setNormalizationMultiplier( 9 );              // descriptors on the byte scale: the byte form keeps their structure
        PopSift ps( cfg, popsift::Config::MatchingMode, PopSift::ByteImages );
        const int shifts[4] = { 0, 3, 5, 2 };
        std::vector<SiftJob*> jobs;
        std::vector<FD*> f;
        for( int k = 0; k < 4; k++ ) {
            std::vector<unsigned char> v( img.size() );
            for( int y = 0; y < h; y++ ) for( int x = 0; x < w; x++ ) v[(size_t)y * w + x] = img[(size_t)y * w + ( x + w - shifts[k] ) % w];
            jobs.push_back( ps.enqueue( w, h, v.data() ) );
            f.push_back( jobs.back()->getDev() );
            CHECK( f.back() != nullptr );
        }
        if( f[0] && f[1] && f[2] && f[3] ) {
            FD empty;
            const std::vector<FD*> views = { f[0], f[1], f[2], &empty, f[3], nullptr };      // the null entry is not named
            const Edges edges = { {2,4}, {0,1}, {1,0}, {0,0}, {0,3}, {3,1}, {4,2}, {0,1}, {1,2} };
            std::vector<int> lens;
            for( FD* v : views ) lens.push_back( v ? v->getDescriptorCount() : 0 );
            popsift::MatchOptions mo;
            mo.mutual = true;
            mo.bytes = true;
            const Lists lists = FD::matchPairsGraph( views, edges, mo );
            CHECK( lists.size() == edges.size() );
            popsift::RansacOptions ro;
            ro.hypotheses = 200;
            ro.seed = 5;
            const std::vector<popsift::HomographyEstimate> est = FD::estimateHomographyGraph( views, edges, lists, ro );
            Lists inliers;
            for( const auto& e : est ) inliers.push_back( e.inliers );
            for( int source = 0; source < 2; source++ ) {
                const Lists& m = source == 0 ? lists : inliers;
                for( int mv = 2; mv <= 3; mv++ ) for( int keep = 0; keep < 2; keep++ ) {
                    popsift::TrackOptions to;
                    to.min_views = mv; to.keep_conflicts = keep != 0;
                    const popsift::Tracks got = FD::buildTracks( views, edges, m, to );
                    const popsift::Tracks want = host_tracks( lens, edges, m, to );
                    CHECK( same( got, want ) );
                    CHECK( (int)got.starts.size() == got.n_tracks + 1 && (int)got.members.size() == got.n_members );
                    if( mv == 2 ) CHECK( got.n_tracks > 10 );
                    std::printf( "buildTracks: %s min_views %d keep %d: %d tracks, %d members, %d components, %d conflicts, %d joined\n",
                                 source == 0 ? "matches" : "inliers", mv, keep, got.n_tracks, got.n_members, got.components, got.conflicts,
                                 got.joined_records );
                }
            }
            // a descriptor index outside its own edge's view
            Lists badl = lists;
            if( !badl[1].empty() ) {
                badl[1][0].right_descriptor = lens[1];
                CHECK( has( runtime_error_of( [&]{ FD::buildTracks( views, edges, badl ); } ), "buildTracks failed" ) );
            }
            CHECK( same( FD::buildTracks( views, edges, lists ), host_tracks( lens, edges, lists, popsift::TrackOptions() ) ) );
        }
        for( auto* p : f ) delete p;
        for( auto* j : jobs ) delete j;
        ps.uninit();
    }
    std::printf( "%s\n", fails ? "FAILED" : "ALL OK" );
    return fails ? 1 : 0;
}
