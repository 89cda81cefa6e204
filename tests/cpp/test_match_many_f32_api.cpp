// Test of the one-to-many FLOAT pair search through the C++ host API: FeaturesDev::matchPairsManyFloat's argument errors (a
// null entry, an object on another device, byte descriptors asked for) and its empty forms -- all before a device is
// touched (this runs without a GPU); matchPairsMany keeps its byte-only throw.
// With POPSIFT_TEST_EXPECT_GPU set (the -m gpu test): four views of a synthetic frame go through PopSift in MatchingMode;
// with and without the cross-check, matchPairsManyFloat( { R0, R1, R2, R0 } ) equals the loop of matchPairs( Rk ) on the
// float descriptors, field by field; estimateHomographyMany accepts its lists and equals the loop of estimateHomography;
// a refused ratio throws.
#include <popsift/popsift.h>
#include <popsift/features.h>
#include <popsift/sift_conf.h>
#include <popsift_hip.h>

#include <cstdio>
#include <cstdlib>
#include <string>
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

int main()
{
    const bool gpu = std::getenv( "POPSIFT_TEST_EXPECT_GPU" ) != nullptr;
    {   // argument errors, in the file:line + message format, before any device call
        popsift::FeaturesDev a, b, c;
        popsift::MatchOptions mo;
        const std::string e = runtime_error_of( [&]{ a.matchPairsManyFloat( { &b, nullptr }, mo ); } );
        CHECK( e.find( "features.cpp:" ) != std::string::npos && e.find( "matchPairsManyFloat" ) != std::string::npos && e.find( "null argument" ) != std::string::npos );
        c.setDevice( 1 );
        const std::string e2 = runtime_error_of( [&]{ a.matchPairsManyFloat( { &b, &c }, mo ); } );
        CHECK( e2.find( "different devices" ) != std::string::npos );
        c.setDevice( 0 );
        popsift::MatchOptions by;
        by.bytes = true;
        const std::string e3 = runtime_error_of( [&]{ a.matchPairsManyFloat( { &b, &c }, by ); } );
        CHECK( e3.find( "use matchPairsMany" ) != std::string::npos );
        // the byte form still refuses float descriptors
        const std::string e4 = runtime_error_of( [&]{ a.matchPairsMany( { &b, &c }, mo ); } );
        CHECK( e4.find( "byte-only" ) != std::string::npos );
        // empty objects, no objects: no pairs, no device call
        const std::vector<std::vector<popsift::Match>> r = a.matchPairsManyFloat( { &b, &c, &b }, mo );
        CHECK( r.size() == 3 && r[0].empty() && r[1].empty() && r[2].empty() );
        CHECK( a.matchPairsManyFloat( {}, mo ).empty() );
        CHECK( a.matchPairsManyFloat( { &b } ).size() == 1 );      // the options default to MatchOptions()
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
        std::vector<popsift::FeaturesDev*> f;
        for( int k = 0; k < 4; k++ ) {
            std::vector<unsigned char> v( img.size() );
            for( int y = 0; y < h; y++ ) for( int x = 0; x < w; x++ ) v[(size_t)y * w + x] = img[(size_t)y * w + ( x + w - shifts[k] ) % w];
            jobs.push_back( ps.enqueue( w, h, v.data() ) );
            f.push_back( jobs.back()->getDev() );
            CHECK( f.back() != nullptr );
        }
        if( f[0] && f[1] && f[2] && f[3] ) {
            std::printf( "descriptors: %d against %d, %d, %d\n", f[0]->getDescriptorCount(), f[1]->getDescriptorCount(),
                         f[2]->getDescriptorCount(), f[3]->getDescriptorCount() );
            const std::vector<popsift::FeaturesDev*> others = { f[1], f[2], f[3], f[1] };      // the same object twice
            for( int mutual = 0; mutual < 2; mutual++ ) {
                popsift::MatchOptions mo;
                mo.mutual = mutual != 0;
                const std::vector<std::vector<popsift::Match>> many = f[0]->matchPairsManyFloat( others, mo );
                CHECK( many.size() == others.size() );
                size_t total = 0;
                for( size_t k = 0; k < others.size() && k < many.size(); k++ ) {
                    const std::vector<popsift::Match> one = f[0]->matchPairs( others[k], mo );
                    CHECK( one.size() > 10 && many[k].size() == one.size() );
                    for( size_t q = 0; q < one.size() && q < many[k].size(); q++ ) CHECK( same( many[k][q], one[q] ) );
                    total += many[k].size();
                }
                std::printf( "mutual %d: %zu pairs in %zu sets\n", mutual, total, many.size() );
                if( mutual && many.size() == others.size() ) {
                    // the lists go into the batched verification unchanged
                    const std::vector<popsift::HomographyEstimate> est = f[0]->estimateHomographyMany( others, many );
                    CHECK( est.size() == others.size() );
                    for( size_t k = 0; k < est.size(); k++ ) {
                        const popsift::HomographyEstimate one = f[0]->estimateHomography( others[k], many[k] );
                        CHECK( est[k].best == one.best && est[k].inliers.size() == one.inliers.size() && est[k].best >= 0 );
                        for( int q = 0; q < 9; q++ ) CHECK( est[k].guide.m[q] == one.guide.m[q] );
                    }
                    std::printf( "homographies: %zu\n", est.size() );
                }
            }
            popsift::MatchOptions bad;
            bad.ratio = -1.0f;
            CHECK( runtime_error_of( [&]{ f[0]->matchPairsManyFloat( others, bad ); } ).find( "matchPairsManyFloat failed" ) != std::string::npos );
        }
        for( auto* p : f ) delete p;
        for( auto* j : jobs ) delete j;
        ps.uninit();
    }
    std::printf( "%s\n", fails ? "FAILED" : "ALL OK" );
    return fails ? 1 : 0;
}
