// Test of the pair search over an edge list through the C++ host API: FeaturesDev::matchPairsGraph's argument errors (an edge
// index out of range, a null referenced entry, views on different devices, float descriptors asked for) and its empty forms
// -- all before a device is touched (this runs without a GPU).
// With POPSIFT_TEST_EXPECT_GPU set (the -m gpu test): four views of a synthetic frame go through PopSift in MatchingMode;
// with and without the cross-check, matchPairsGraph over an unsorted edge list -- both orders of a pair, a self edge, a
// duplicate -- equals the loop of views[left]->matchPairs( views[right] ) with MatchOptions::bytes, field by field; a refused
// ratio throws.
#include <popsift/popsift.h>
#include <popsift/features.h>
#include <popsift/sift_conf.h>
#include <popsift_hip.h>

#include <cstdio>
#include <cstdlib>
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

static bool same( const popsift::Match& a, const popsift::Match& b )
{
    return a.left_feature == b.left_feature && a.right_feature == b.right_feature && a.left_descriptor == b.left_descriptor &&
           a.right_descriptor == b.right_descriptor && a.distance == b.distance && a.second_distance == b.second_distance;
}

typedef std::vector<std::pair<int,int>> Edges;

int main()
{
    const bool gpu = std::getenv( "POPSIFT_TEST_EXPECT_GPU" ) != nullptr;
    {   // argument errors, in the file:line + message format, before any device call
        popsift::FeaturesDev a, b, c;
        popsift::MatchOptions mo;
        mo.bytes = true;
        const std::string e0 = runtime_error_of( [&]{ popsift::FeaturesDev::matchPairsGraph( { &a, &b }, Edges{ {0,1}, {0,2} }, mo ); } );
        CHECK( e0.find( "features.cpp:" ) != std::string::npos && e0.find( "matchPairsGraph" ) != std::string::npos && e0.find( "out of range" ) != std::string::npos );
        CHECK( runtime_error_of( [&]{ popsift::FeaturesDev::matchPairsGraph( { &a, &b }, Edges{ {-1,1} }, mo ); } ).find( "out of range" ) != std::string::npos );
        CHECK( runtime_error_of( [&]{ popsift::FeaturesDev::matchPairsGraph( {}, Edges{ {0,0} }, mo ); } ).find( "out of range" ) != std::string::npos );
        const std::string e1 = runtime_error_of( [&]{ popsift::FeaturesDev::matchPairsGraph( { &a, nullptr }, Edges{ {0,1} }, mo ); } );
        CHECK( e1.find( "null argument" ) != std::string::npos );
        // a null entry that no edge names is not looked at
        CHECK( popsift::FeaturesDev::matchPairsGraph( { &a, nullptr, &b }, Edges{ {0,2} }, mo ).size() == 1 );
        c.setDevice( 1 );
        const std::string e2 = runtime_error_of( [&]{ popsift::FeaturesDev::matchPairsGraph( { &a, &b, &c }, Edges{ {0,1}, {1,2} }, mo ); } );
        CHECK( e2.find( "different devices" ) != std::string::npos );
        c.setDevice( 0 );
        popsift::MatchOptions fl;
        const std::string e3 = runtime_error_of( [&]{ popsift::FeaturesDev::matchPairsGraph( { &a, &b }, Edges{ {0,1} }, fl ); } );
        CHECK( e3.find( "byte-only" ) != std::string::npos );
        // empty objects, no edges: no pairs, no device call
        const std::vector<std::vector<popsift::Match>> r = popsift::FeaturesDev::matchPairsGraph( { &a, &b, &c }, Edges{ {0,1}, {2,2}, {1,0} }, mo );
        CHECK( r.size() == 3 && r[0].empty() && r[1].empty() && r[2].empty() );
        CHECK( popsift::FeaturesDev::matchPairsGraph( { &a, &b }, Edges{}, mo ).empty() );
        CHECK( popsift::FeaturesDev::matchPairsGraph( {}, Edges{}, mo ).empty() );
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
        std::vector<popsift::FeaturesDev*> f;
        for( int k = 0; k < 4; k++ ) {
            std::vector<unsigned char> v( img.size() );
            for( int y = 0; y < h; y++ ) for( int x = 0; x < w; x++ ) v[(size_t)y * w + x] = img[(size_t)y * w + ( x + w - shifts[k] ) % w];
            jobs.push_back( ps.enqueue( w, h, v.data() ) );
            f.push_back( jobs.back()->getDev() );
            CHECK( f.back() != nullptr );
        }
        if( f[0] && f[1] && f[2] && f[3] ) {
            std::printf( "descriptors: %d, %d, %d, %d\n", f[0]->getDescriptorCount(), f[1]->getDescriptorCount(),
                         f[2]->getDescriptorCount(), f[3]->getDescriptorCount() );
            popsift::FeaturesDev empty;
            const std::vector<popsift::FeaturesDev*> views = { f[0], f[1], f[2], &empty, f[3], nullptr };      // the null entry is not named
            const Edges edges = { {2,4}, {0,1}, {1,0}, {0,0}, {0,3}, {3,1}, {4,2}, {0,1}, {1,2} };
            for( int mutual = 0; mutual < 2; mutual++ ) {
                popsift::MatchOptions mo;
                mo.mutual = mutual != 0;
                mo.bytes = true;
                const std::vector<std::vector<popsift::Match>> got = popsift::FeaturesDev::matchPairsGraph( views, edges, mo );
                CHECK( got.size() == edges.size() );
                size_t total = 0;
                for( size_t e = 0; e < edges.size() && e < got.size(); e++ ) {
                    const std::vector<popsift::Match> one = views[edges[e].first]->matchPairs( views[edges[e].second], mo );
                    const bool live = edges[e].first != 3 && edges[e].second != 3;
                    CHECK( live ? one.size() > 10 : one.empty() );
                    CHECK( got[e].size() == one.size() );
                    for( size_t q = 0; q < one.size() && q < got[e].size(); q++ ) CHECK( same( got[e][q], one[q] ) );
                    total += got[e].size();
                }
                std::printf( "mutual %d: %zu pairs over %zu edges\n", mutual, total, got.size() );
            }
            popsift::MatchOptions bad;
            bad.bytes = true;
            bad.ratio = -1.0f;
            CHECK( runtime_error_of( [&]{ popsift::FeaturesDev::matchPairsGraph( views, edges, bad ); } ).find( "matchPairsGraph failed" ) != std::string::npos );
        }
        for( auto* p : f ) delete p;
        for( auto* j : jobs ) delete j;
        ps.uninit();
    }
    std::printf( "%s\n", fails ? "FAILED" : "ALL OK" );
    return fails ? 1 : 0;
}
