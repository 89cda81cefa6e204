// Test of the guided re-match of many sets through the C++ host API: FeaturesDev::matchPairsGuidedMany's argument errors (a
// null entry, an object on another device, float descriptors asked for, a guide count that differs from the object count,
// an invalid guide) and its empty forms -- all before a device is touched (this runs without a GPU).
// With POPSIFT_TEST_EXPECT_GPU set (the -m gpu test): four views of a synthetic frame, shifted horizontally, go through
// PopSift in MatchingMode; with and without the cross-check, matchPairsGuidedMany( { R0, R1, R2, R0, R1 }, guides ) -- a
// window around each view's own shift, an epipolar band along the rows, the same object again under another window, and
// one set skipped -- equals the loop of matchPairsGuided( Rk, guides[k] ) with MatchOptions::bytes, field by field.
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

static popsift::MatchGuide window( float dx, float tol )
{
    popsift::MatchGuide g = popsift::MatchGuide::none();
    g.kind = popsift::MatchGuide::Homography;
    g.m[0] = g.m[4] = g.m[8] = 1.0f;
    g.m[2] = dx;
    g.tol = tol;
    return g;
}

int main()
{
    const bool gpu = std::getenv( "POPSIFT_TEST_EXPECT_GPU" ) != nullptr;
    {   // argument errors, in the file:line + message format, before any device call
        popsift::FeaturesDev a, b, c;
        popsift::MatchOptions mo;
        mo.bytes = true;
        const popsift::MatchGuide w = window( 0.0f, 2.0f ), none = popsift::MatchGuide::none();
        CHECK( none.kind == popsift::MatchGuide::None && (int)popsift::MatchGuide::None == PSX_GUIDE_NONE );
        const std::string e = runtime_error_of( [&]{ a.matchPairsGuidedMany( { &b, nullptr }, { w, w }, mo ); } );
        CHECK( e.find( "features.cpp:" ) != std::string::npos && e.find( "matchPairsGuidedMany" ) != std::string::npos && e.find( "null argument" ) != std::string::npos );
        c.setDevice( 1 );
        const std::string e2 = runtime_error_of( [&]{ a.matchPairsGuidedMany( { &b, &c }, { w, w }, mo ); } );
        CHECK( e2.find( "different devices" ) != std::string::npos );
        c.setDevice( 0 );
        popsift::MatchOptions fl;
        const std::string e3 = runtime_error_of( [&]{ a.matchPairsGuidedMany( { &b, &c }, { w, w }, fl ); } );
        CHECK( e3.find( "byte-only" ) != std::string::npos );
        const std::string e4 = runtime_error_of( [&]{ a.matchPairsGuidedMany( { &b, &c }, { w }, mo ); } );
        CHECK( e4.find( "2 objects but 1 guides" ) != std::string::npos );
        popsift::MatchGuide bad = w;
        bad.tol = -1.0f;
        const std::string e5 = runtime_error_of( [&]{ a.matchPairsGuidedMany( { &b, &c }, { w, bad }, mo ); } );     // the LAST guide
        CHECK( e5.find( "invalid guide" ) != std::string::npos );
        bad = w;
        bad.kind = (popsift::MatchGuide::Kind)3;
        CHECK( runtime_error_of( [&]{ a.matchPairsGuidedMany( { &b, &c }, { w, bad }, mo ); } ).find( "invalid guide" ) != std::string::npos );
        // the single call keeps refusing kind None
        CHECK( runtime_error_of( [&]{ a.matchPairsGuided( &b, none, mo ); } ).find( "invalid guide" ) != std::string::npos );
        // empty objects, skipped sets, no objects: no pairs, no device call
        const std::vector<std::vector<popsift::Match>> r = a.matchPairsGuidedMany( { &b, &c, &b }, { w, none, w }, mo );
        CHECK( r.size() == 3 && r[0].empty() && r[1].empty() && r[2].empty() );
        CHECK( a.matchPairsGuidedMany( {}, {}, mo ).empty() );
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
            std::printf( "descriptors: %d against %d, %d, %d\n", f[0]->getDescriptorCount(), f[1]->getDescriptorCount(),
                         f[2]->getDescriptorCount(), f[3]->getDescriptorCount() );
            popsift::MatchGuide rows = popsift::MatchGuide::none();            // F of a horizontal shift: the line y = yl
            rows.kind = popsift::MatchGuide::Epipolar;
            rows.m[5] = -1.0f; rows.m[7] = 1.0f;
            rows.tol = 1.5f;
            const std::vector<popsift::FeaturesDev*> others = { f[1], f[2], f[3], f[1], f[2] };      // the same objects twice
            const std::vector<popsift::MatchGuide> guides = { window( 3.0f, 2.0f ), rows, window( 2.0f, 3.0f ), window( 3.0f, 8.0f ),
                                                              popsift::MatchGuide::none() };
            for( int mutual = 0; mutual < 2; mutual++ ) {
                popsift::MatchOptions mo;
                mo.mutual = mutual != 0;
                mo.bytes = true;
                const std::vector<std::vector<popsift::Match>> many = f[0]->matchPairsGuidedMany( others, guides, mo );
                CHECK( many.size() == others.size() );
                size_t total = 0;
                for( size_t k = 0; k < others.size() && k < many.size(); k++ ) {
                    if( guides[k].kind == popsift::MatchGuide::None ) { CHECK( many[k].empty() ); continue; }
                    const std::vector<popsift::Match> one = f[0]->matchPairsGuided( others[k], guides[k], mo );
                    CHECK( one.size() > 10 && many[k].size() == one.size() );
                    for( size_t q = 0; q < one.size() && q < many[k].size(); q++ ) CHECK( same( many[k][q], one[q] ) );
                    total += many[k].size();
                }
                std::printf( "mutual %d: %zu pairs in %zu sets\n", mutual, total, many.size() );
            }
            popsift::MatchOptions bad;
            bad.bytes = true;
            bad.ratio = -1.0f;
            CHECK( runtime_error_of( [&]{ f[0]->matchPairsGuidedMany( others, guides, bad ); } ).find( "matchPairsGuidedMany failed" ) != std::string::npos );
        }
        for( auto* p : f ) delete p;
        for( auto* j : jobs ) delete j;
        ps.uninit();
    }
    std::printf( "%s\n", fails ? "FAILED" : "ALL OK" );
    return fails ? 1 : 0;
}
