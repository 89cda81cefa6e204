// Test of the float edge-list and batched guided calls through the C++ host API: the signatures of
// FeaturesDev::matchPairsGraphFloat, matchPairsGuidedManyFloat and matchPairsGuidedGraphFloat, their argument errors (a null
// entry, an object on another device, byte descriptors asked for, an edge out of range, guide counts, an invalid guide) and
// their empty forms -- all before a device is touched (this runs without a GPU); the byte forms keep their byte-only throw.
// With POPSIFT_TEST_EXPECT_GPU set (the -m gpu test): four views of a synthetic frame go through PopSift in MatchingMode;
// with and without the cross-check every element of the three calls equals matchPairs / matchPairsGuided of its pair of
// objects on the float descriptors, field by field; a guide of kind None gives an empty element; a refused ratio throws.
#include <popsift/popsift.h>
#include <popsift/features.h>
#include <popsift/sift_conf.h>
#include <popsift_hip.h>

#include <cstdio>
#include <cstdlib>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

static int fails = 0;
#define CHECK(c) do { if(!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); fails++; } } while(0)

using popsift::FeaturesDev;
using popsift::Match;
using popsift::MatchGuide;
using popsift::MatchOptions;
typedef std::vector<std::vector<Match>> Lists;
typedef std::vector<std::pair<int,int>> Edges;

// the signatures: two static members over views and edges, one member over this object and others
static_assert( std::is_same<decltype( &FeaturesDev::matchPairsGraphFloat ),
                            Lists (*)( const std::vector<FeaturesDev*>&, const Edges&, const MatchOptions& )>::value, "matchPairsGraphFloat" );
static_assert( std::is_same<decltype( &FeaturesDev::matchPairsGuidedGraphFloat ),
                            Lists (*)( const std::vector<FeaturesDev*>&, const Edges&, const std::vector<MatchGuide>&, const MatchOptions& )>::value,
               "matchPairsGuidedGraphFloat" );
static_assert( std::is_same<decltype( &FeaturesDev::matchPairsGuidedManyFloat ),
                            Lists (FeaturesDev::*)( const std::vector<FeaturesDev*>&, const std::vector<MatchGuide>&, const MatchOptions& )>::value,
               "matchPairsGuidedManyFloat" );

template <class F> static std::string runtime_error_of( F f )
{
    try { f(); } catch( const std::runtime_error& e ) { return std::string( "E:" ) + e.what(); } catch( ... ) { return ""; }
    return "";
}

static bool has( const std::string& s, const char* what ) { return s.find( what ) != std::string::npos; }

static bool same( const Match& a, const Match& b )
{
    return a.left_feature == b.left_feature && a.right_feature == b.right_feature && a.left_descriptor == b.left_descriptor &&
           a.right_descriptor == b.right_descriptor && a.distance == b.distance && a.second_distance == b.second_distance;
}

static bool same_list( const std::vector<Match>& a, const std::vector<Match>& b )
{
    if( a.size() != b.size() ) return false;
    for( size_t q = 0; q < a.size(); q++ ) if( !same( a[q], b[q] ) ) return false;
    return true;
}

int main()
{
    const bool gpu = std::getenv( "POPSIFT_TEST_EXPECT_GPU" ) != nullptr;
    {   // argument errors, in the file:line + message format, before any device call
        FeaturesDev a, b, c;
        MatchOptions mo, by;
        by.bytes = true;
        MatchGuide window;
        window.kind = MatchGuide::Homography;
        for( int q = 0; q < 9; q++ ) window.m[q] = ( q % 4 == 0 ) ? 1.0f : 0.0f;
        window.tol = 2.0f;
        const Edges edges = { { 0, 1 }, { 1, 0 }, { 0, 0 } };
        const std::vector<MatchGuide> g3( 3, window );

        std::string e = runtime_error_of( [&]{ FeaturesDev::matchPairsGraphFloat( { &a, nullptr }, edges, mo ); } );
        CHECK( has( e, "features.cpp:" ) && has( e, "matchPairsGraphFloat" ) && has( e, "null argument" ) );
        CHECK( has( runtime_error_of( [&]{ FeaturesDev::matchPairsGraphFloat( { &a, &b }, { { 0, 2 } }, mo ); } ), "out of range" ) );
        c.setDevice( 1 );
        CHECK( has( runtime_error_of( [&]{ FeaturesDev::matchPairsGraphFloat( { &a, &c }, edges, mo ); } ), "different devices" ) );
        CHECK( has( runtime_error_of( [&]{ FeaturesDev::matchPairsGuidedGraphFloat( { &a, &c }, edges, g3, mo ); } ), "different devices" ) );
        CHECK( has( runtime_error_of( [&]{ a.matchPairsGuidedManyFloat( { &b, &c }, { window, window }, mo ); } ), "different devices" ) );
        c.setDevice( 0 );
        CHECK( has( runtime_error_of( [&]{ FeaturesDev::matchPairsGraphFloat( { &a, &b }, edges, by ); } ), "float descriptors only" ) );
        CHECK( has( runtime_error_of( [&]{ FeaturesDev::matchPairsGuidedGraphFloat( { &a, &b }, edges, g3, by ); } ), "float descriptors only" ) );
        CHECK( has( runtime_error_of( [&]{ a.matchPairsGuidedManyFloat( { &b }, { window }, by ); } ), "float descriptors only" ) );
        CHECK( has( runtime_error_of( [&]{ a.matchPairsGuidedManyFloat( { &b, nullptr }, { window, window }, mo ); } ), "null argument" ) );
        CHECK( has( runtime_error_of( [&]{ a.matchPairsGuidedManyFloat( { &b, &c }, { window }, mo ); } ), "2 objects but 1 guides" ) );
        CHECK( has( runtime_error_of( [&]{ FeaturesDev::matchPairsGuidedGraphFloat( { &a, &b }, edges, { window }, mo ); } ), "3 edges but 1 guides" ) );
        MatchGuide bad = window;
        bad.kind = (MatchGuide::Kind)7;
        CHECK( has( runtime_error_of( [&]{ a.matchPairsGuidedManyFloat( { &b }, { bad }, mo ); } ), "invalid guide" ) );
        CHECK( has( runtime_error_of( [&]{ FeaturesDev::matchPairsGuidedGraphFloat( { &a, &b }, edges, { window, bad, window }, mo ); } ), "invalid guide" ) );
        // the byte forms still refuse float descriptors
        CHECK( has( runtime_error_of( [&]{ FeaturesDev::matchPairsGraph( { &a, &b }, edges, mo ); } ), "byte-only" ) );
        CHECK( has( runtime_error_of( [&]{ FeaturesDev::matchPairsGuidedGraph( { &a, &b }, edges, g3, mo ); } ), "byte-only" ) );
        CHECK( has( runtime_error_of( [&]{ a.matchPairsGuidedMany( { &b }, { window }, mo ); } ), "byte-only" ) );
        // empty objects, no edges, an unreferenced null view: no pairs, no device call; the options default to MatchOptions()
        const Lists r = FeaturesDev::matchPairsGraphFloat( { &a, &b, nullptr }, edges );
        CHECK( r.size() == 3 && r[0].empty() && r[1].empty() && r[2].empty() );
        CHECK( FeaturesDev::matchPairsGraphFloat( { &a }, {} ).empty() );
        CHECK( FeaturesDev::matchPairsGuidedGraphFloat( { &a, &b }, edges, g3 ).size() == 3 );
        CHECK( a.matchPairsGuidedManyFloat( { &b, &c }, { window, MatchGuide::none() } ).size() == 2 );
        CHECK( a.matchPairsGuidedManyFloat( {}, {} ).empty() );
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
        PopSift ps( cfg, popsift::Config::MatchingMode, PopSift::ByteImages );
        const int shifts[4] = { 0, 3, 5, 2 };
        std::vector<SiftJob*> jobs;
        std::vector<FeaturesDev*> f;
        for( int k = 0; k < 4; k++ ) {
            std::vector<unsigned char> v( img.size() );
            for( int y = 0; y < h; y++ ) for( int x = 0; x < w; x++ ) v[(size_t)y * w + x] = img[(size_t)y * w + ( x + w - shifts[k] ) % w];
            jobs.push_back( ps.enqueue( w, h, v.data() ) );
            f.push_back( jobs.back()->getDev() );
            CHECK( f.back() != nullptr );
        }
        if( f[0] && f[1] && f[2] && f[3] ) {
            std::printf( "descriptors: %d, %d, %d, %d\n", f[0]->getDescriptorCount(), f[1]->getDescriptorCount(), f[2]->getDescriptorCount(),
                         f[3]->getDescriptorCount() );
            // unsorted, both orders, a self edge, a duplicate
            const Edges edges = { { 2, 3 }, { 0, 1 }, { 1, 0 }, { 0, 0 }, { 3, 1 }, { 0, 1 } };
            // view k is the frame shifted by shifts[k] columns: a translation, as a window of 3 px; one edge is skipped, one
            // guide is wrong on purpose (the re-match of its edge finds little, and still equals the single call)
            std::vector<MatchGuide> guides( edges.size() );
            for( size_t e = 0; e < edges.size(); e++ ) {
                MatchGuide g;
                g.kind = MatchGuide::Homography;
                for( int q = 0; q < 9; q++ ) g.m[q] = ( q % 4 == 0 ) ? 1.0f : 0.0f;
                g.m[2] = (float)( shifts[edges[e].second] - shifts[edges[e].first] );
                g.tol = 3.0f;
                guides[e] = g;
            }
            guides[2] = MatchGuide::none();
            guides[4].m[2] += 40.0f;
            for( int mutual = 0; mutual < 2; mutual++ ) {
                MatchOptions mo;
                mo.mutual = mutual != 0;
                const Lists graph = FeaturesDev::matchPairsGraphFloat( f, edges, mo );
                CHECK( graph.size() == edges.size() );
                size_t total = 0;
                for( size_t e = 0; e < edges.size() && e < graph.size(); e++ ) {
                    const std::vector<Match> one = f[edges[e].first]->matchPairs( f[edges[e].second], mo );
                    CHECK( one.size() > 10 && same_list( graph[e], one ) );
                    total += graph[e].size();
                }
                std::printf( "matchPairsGraphFloat: mutual %d, %zu pairs over %zu edges\n", mutual, total, edges.size() );

                const Lists gg = FeaturesDev::matchPairsGuidedGraphFloat( f, edges, guides, mo );
                CHECK( gg.size() == edges.size() );
                total = 0;
                for( size_t e = 0; e < edges.size() && e < gg.size(); e++ ) {
                    if( guides[e].kind == MatchGuide::None ) { CHECK( gg[e].empty() ); continue; }
                    const std::vector<Match> one = f[edges[e].first]->matchPairsGuided( f[edges[e].second], guides[e], mo );
                    CHECK( same_list( gg[e], one ) );
                    if( e != 4 ) CHECK( one.size() > 10 );
                    total += gg[e].size();
                }
                std::printf( "matchPairsGuidedGraphFloat: mutual %d, %zu pairs\n", mutual, total );

                const std::vector<FeaturesDev*> others = { f[1], f[2], f[3], f[1] };
                std::vector<MatchGuide> sg( others.size() );
                const int oshift[4] = { shifts[1], shifts[2], shifts[3], shifts[1] };
                for( size_t k = 0; k < others.size(); k++ ) {
                    sg[k] = guides[1];
                    sg[k].m[2] = (float)( oshift[k] - shifts[0] );
                }
                sg[2] = MatchGuide::none();
                const Lists gm = f[0]->matchPairsGuidedManyFloat( others, sg, mo );
                CHECK( gm.size() == others.size() );
                total = 0;
                for( size_t k = 0; k < others.size() && k < gm.size(); k++ ) {
                    if( sg[k].kind == MatchGuide::None ) { CHECK( gm[k].empty() ); continue; }
                    const std::vector<Match> one = f[0]->matchPairsGuided( others[k], sg[k], mo );
                    CHECK( one.size() > 10 && same_list( gm[k], one ) );
                    total += gm[k].size();
                }
                std::printf( "matchPairsGuidedManyFloat: mutual %d, %zu pairs\n", mutual, total );
            }
            MatchOptions bad;
            bad.ratio = -1.0f;
            CHECK( has( runtime_error_of( [&]{ FeaturesDev::matchPairsGraphFloat( f, edges, bad ); } ), "matchPairsGraphFloat failed" ) );
            CHECK( has( runtime_error_of( [&]{ FeaturesDev::matchPairsGuidedGraphFloat( f, edges, guides, bad ); } ), "matchPairsGuidedGraphFloat failed" ) );
            CHECK( has( runtime_error_of( [&]{ f[0]->matchPairsGuidedManyFloat( { f[1] }, { guides[1] }, bad ); } ), "matchPairsGuidedManyFloat failed" ) );
        }
        for( auto* p : f ) delete p;
        for( auto* j : jobs ) delete j;
        ps.uninit();
    }
    std::printf( "%s\n", fails ? "FAILED" : "ALL OK" );
    return fails ? 1 : 0;
}
