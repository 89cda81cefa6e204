// Test of guided matching through the C++ host API: psx_guide's layout, popsift::MatchGuide, and
// FeaturesDev::matchPairsGuided's argument errors (a null argument, two objects on different devices, an invalid guide) --
// all before a device is touched (this runs without a GPU); the C-ABI's own argument checks likewise.
// With POPSIFT_TEST_EXPECT_GPU set (the -m gpu test): two views of a synthetic frame, the second shifted by 3 pixels, go
// through PopSift in MatchingMode; under the guide "translation by 3, tolerance 1.5", for float and for byte descriptors,
// with and without the cross-check, matchPairsGuided's descriptor indices and distances equal the C-ABI's guided pairs on
// the same device arrays (positions from psx_desc_positions), its feature indices are the reverse maps applied to them,
// and every pair satisfies the guide on the features' own positions.
#include <popsift/popsift.h>
#include <popsift/features.h>
#include <popsift/sift_conf.h>
#include <popsift_hip.h>

#include <climits>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

static int fails = 0;
#define CHECK(c) do { if(!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); fails++; } } while(0)

template <class F> static std::string runtime_error_of( F f )
{
    try { f(); } catch( const std::runtime_error& e ) { return std::string( "E:" ) + e.what(); } catch( ... ) { return ""; }
    return "";
}

static_assert( sizeof(psx_guide) == 44 && offsetof(psx_guide, m) == 4 && offsetof(psx_guide, tol) == 40, "psx_guide layout" );
static_assert( (int)popsift::MatchGuide::Homography == PSX_GUIDE_HOMOGRAPHY && (int)popsift::MatchGuide::Epipolar == PSX_GUIDE_EPIPOLAR, "kinds" );

static popsift::MatchGuide shift_guide( float dx, float tol )
{
    popsift::MatchGuide g;
    g.kind = popsift::MatchGuide::Homography;
    const float m[9] = { 1, 0, dx, 0, 1, 0, 0, 0, 1 };
    for( int k = 0; k < 9; k++ ) g.m[k] = m[k];
    g.tol = tol;
    return g;
}

int main()
{
    const bool gpu = std::getenv( "POPSIFT_TEST_EXPECT_GPU" ) != nullptr;
    const float nan = std::numeric_limits<float>::quiet_NaN();
    {   // argument errors, in the file:line + message format, before any device call
        popsift::FeaturesDev a, b;
        const popsift::MatchGuide g = shift_guide( 3.0f, 1.5f );
        const std::string e = runtime_error_of( [&]{ a.matchPairsGuided( nullptr, g ); } );
        CHECK( e.find( "features.cpp:" ) != std::string::npos && e.find( "null argument" ) != std::string::npos );
        b.setDevice( 1 );
        CHECK( runtime_error_of( [&]{ a.matchPairsGuided( &b, g ); } ).find( "different devices" ) != std::string::npos );
        b.setDevice( 0 );
        CHECK( a.matchPairsGuided( &b, g ).empty() );         // two empty objects: no pairs, no device call
        // an invalid guide throws, for empty objects too
        popsift::MatchGuide bad = g;
        bad.kind = (popsift::MatchGuide::Kind)3;
        CHECK( runtime_error_of( [&]{ a.matchPairsGuided( &b, bad ); } ).find( "invalid guide" ) != std::string::npos );
        bad = g; bad.tol = -1.0f;
        CHECK( runtime_error_of( [&]{ a.matchPairsGuided( &b, bad ); } ).find( "invalid guide" ) != std::string::npos );
        bad = g; bad.tol = nan;
        CHECK( runtime_error_of( [&]{ a.matchPairsGuided( &b, bad ); } ).find( "invalid guide" ) != std::string::npos );
        bad = g; bad.m[4] = INFINITY;
        CHECK( runtime_error_of( [&]{ a.matchPairsGuided( &b, bad ); } ).find( "invalid guide" ) != std::string::npos );
        CHECK( runtime_error_of( [&]{ a.matchPairs( nullptr ); } ).find( "FeaturesDev::matchPairs:" ) != std::string::npos );   // unchanged
    }
    {   // the C-ABI checks its arguments before it touches a device
        psx_guide g = { PSX_GUIDE_HOMOGRAPHY, { 1, 0, 0, 0, 1, 0, 0, 0, 1 }, 2.0f };
        psx_match_opts po = { 0.8f, 0 };
        int n = -5;
        CHECK( psx_match_pairs_guided( 0, nullptr, nullptr, 0, nullptr, nullptr, 0, &g, &po, nullptr, 0, &n ) == PSX_OK && n == 0 );
        n = -5;
        CHECK( psx_match_pairs_guided( 0, nullptr, nullptr, 0, nullptr, nullptr, 0, nullptr, &po, nullptr, 0, &n ) == PSX_ERR_INVALID );
        g.kind = 0;
        CHECK( psx_match_pairs_guided_u8( 0, nullptr, nullptr, 0, nullptr, nullptr, 0, &g, &po, nullptr, 0, &n ) == PSX_ERR_INVALID );
        CHECK( psx_match_guided( 0, nullptr, nullptr, 0, nullptr, nullptr, 0, &g, nullptr, nullptr ) == PSX_ERR_INVALID );
        g.kind = PSX_GUIDE_EPIPOLAR;
        CHECK( psx_match_guided( 0, nullptr, nullptr, 0, nullptr, nullptr, 0, &g, nullptr, nullptr ) == PSX_OK );
        float one[2] = { 0, 0 };
        CHECK( psx_match_guided( 0, one, nullptr, 1, nullptr, nullptr, 0, &g, (int*)one, nullptr ) == PSX_ERR_INVALID );   // NULL positions with a length
        CHECK( psx_desc_positions( 0, nullptr, nullptr, 0, nullptr ) == PSX_OK && psx_desc_positions( 0, nullptr, nullptr, 2, nullptr ) == PSX_ERR_INVALID );
        CHECK( n == -5 );
    }
    if( gpu ) {
        const int w = 320, h = 240, shift = 3;
        std::vector<unsigned char> img( (size_t)w * h ), img2( (size_t)w * h );
        unsigned s = 12345u;
        std::vector<unsigned char> coarse( (size_t)( w / 8 + 2 ) * ( h / 8 + 2 ) );
        for( auto& c : coarse ) { s = s * 1664525u + 1013904223u; c = (unsigned char)( s >> 24 ); }
        for( int y = 0; y < h; y++ ) for( int x = 0; x < w; x++ ) {
            const int cw = w / 8 + 2;
            const int v = ( 3 * coarse[(size_t)( y / 8 ) * cw + x / 8] + coarse[(size_t)( y / 5 % ( h / 8 ) ) * cw + ( x / 3 ) % ( w / 8 )] ) / 4;
            img[(size_t)y * w + x] = (unsigned char)v;
        }
        for( int y = 0; y < h; y++ ) for( int x = 0; x < w; x++ ) img2[(size_t)y * w + x] = img[(size_t)y * w + ( x + w - shift ) % w];
        popsift::Config cfg;
        cfg.setOctaves( 3 );
        cfg.setNormalizationMultiplier( 9 );              // descriptors on the byte scale: the byte form keeps their structure
        PopSift ps( cfg, popsift::Config::MatchingMode, PopSift::ByteImages );
        SiftJob* lj = ps.enqueue( w, h, img.data() );
        SiftJob* rj = ps.enqueue( w, h, img2.data() );
        popsift::FeaturesDev* L = lj->getDev();
        popsift::FeaturesDev* R = rj->getDev();
        CHECK( L != nullptr && R != nullptr );
        if( L && R ) {
            const int nl = L->getDescriptorCount(), nr = R->getDescriptorCount();
            std::printf( "descriptors: %d and %d\n", nl, nr );
            CHECK( nl > 50 && nr > 50 );
            std::vector<int> lrev( nl ), rrev( nr );
            CHECK( psx_dev_read( 0, lrev.data(), L->getReverseMap(), (size_t)nl * sizeof(int) ) == PSX_OK );
            CHECK( psx_dev_read( 0, rrev.data(), R->getReverseMap(), (size_t)nr * sizeof(int) ) == PSX_OK );
            std::vector<popsift::Feature> lf( L->getFeatureCount() ), rf( R->getFeatureCount() );
            CHECK( psx_dev_read( 0, lf.data(), L->getFeatures(), lf.size() * sizeof(popsift::Feature) ) == PSX_OK );
            CHECK( psx_dev_read( 0, rf.data(), R->getFeatures(), rf.size() * sizeof(popsift::Feature) ) == PSX_OK );
            void *lxy = nullptr, *rxy = nullptr;
            CHECK( psx_dev_alloc( 0, (size_t)nl * 8, &lxy ) == PSX_OK && psx_dev_alloc( 0, (size_t)nr * 8, &rxy ) == PSX_OK );
            CHECK( psx_desc_positions( 0, (const psx_feature_dev*)L->getFeatures(), L->getReverseMap(), nl, (float*)lxy ) == PSX_OK );
            CHECK( psx_desc_positions( 0, (const psx_feature_dev*)R->getFeatures(), R->getReverseMap(), nr, (float*)rxy ) == PSX_OK );
            const popsift::MatchGuide g = shift_guide( (float)shift, 1.5f );
            psx_guide pg;
            pg.kind = PSX_GUIDE_HOMOGRAPHY; pg.tol = g.tol;
            for( int k = 0; k < 9; k++ ) pg.m[k] = g.m[k];
            for( int mutual = 0; mutual < 2; mutual++ ) {
                popsift::MatchOptions mo;
                mo.mutual = mutual != 0;
                const std::vector<popsift::Match> mm = L->matchPairsGuided( R, g, mo );
                psx_match_opts po = { 0.8f, mutual ? PSX_PAIRS_MUTUAL : 0 };
                std::vector<psx_match_pair> pp( nl );
                int n = -1;
                CHECK( psx_match_pairs_guided( 0, (const float*)L->getDescriptors(), (const float*)lxy, nl, (const float*)R->getDescriptors(), (const float*)rxy, nr,
                                               &pg, &po, pp.data(), nl, &n ) == PSX_OK );
                std::printf( "float, mutual %d: %d guided pairs\n", mutual, n );
                CHECK( n > 10 && (int)mm.size() == n );
                for( int k = 0; k < n && k < (int)mm.size(); k++ ) {
                    CHECK( mm[k].left_descriptor == pp[k].left && mm[k].right_descriptor == pp[k].right );
                    CHECK( mm[k].distance == pp[k].d1 && mm[k].second_distance == pp[k].d2 );
                    CHECK( mm[k].left_feature == lrev[pp[k].left] && mm[k].right_feature == rrev[pp[k].right] );
                    if( k > 0 ) CHECK( mm[k].left_descriptor > mm[k - 1].left_descriptor );
                    // the pair satisfies the guide on the features' own positions (the window, restated)
                    const popsift::Feature& a = lf[mm[k].left_feature];
                    const popsift::Feature& b = rf[mm[k].right_feature];
                    const float dx = ( a.xpos + (float)shift ) - b.xpos, dy = a.ypos - b.ypos;
                    CHECK( dx * dx + dy * dy <= 1.5f * 1.5f );
                }
                mo.bytes = true;
                const std::vector<popsift::Match> mb = L->matchPairsGuided( R, g, mo );
                void *lb = nullptr, *rb = nullptr;
                CHECK( psx_dev_alloc( 0, (size_t)nl * 128, &lb ) == PSX_OK && psx_dev_alloc( 0, (size_t)nr * 128, &rb ) == PSX_OK );
                CHECK( psx_quantize_desc( 0, (const float*)L->getDescriptors(), nl, (unsigned char*)lb ) == PSX_OK );
                CHECK( psx_quantize_desc( 0, (const float*)R->getDescriptors(), nr, (unsigned char*)rb ) == PSX_OK );
                std::vector<psx_match_pair_u8> pb( nl );
                n = -1;
                CHECK( psx_match_pairs_guided_u8( 0, (const unsigned char*)lb, (const float*)lxy, nl, (const unsigned char*)rb, (const float*)rxy, nr,
                                                  &pg, &po, pb.data(), nl, &n ) == PSX_OK );
                std::printf( "bytes, mutual %d: %d guided pairs\n", mutual, n );
                CHECK( n > 10 && (int)mb.size() == n );
                for( int k = 0; k < n && k < (int)mb.size(); k++ ) {
                    CHECK( mb[k].left_descriptor == pb[k].left && mb[k].right_descriptor == pb[k].right );
                    CHECK( mb[k].distance == ( pb[k].d1 == INT_MAX ? INFINITY : (float)pb[k].d1 ) );
                    CHECK( mb[k].second_distance == ( pb[k].d2 == INT_MAX ? INFINITY : (float)pb[k].d2 ) );
                    CHECK( mb[k].left_feature == lrev[pb[k].left] && mb[k].right_feature == rrev[pb[k].right] );
                }
                psx_dev_free( 0, lb ); psx_dev_free( 0, rb );
            }
            psx_dev_free( 0, lxy ); psx_dev_free( 0, rxy );
            // a failing call: a ratio the C-ABI refuses
            popsift::MatchOptions bad;
            bad.ratio = -1.0f;
            CHECK( runtime_error_of( [&]{ L->matchPairsGuided( R, g, bad ); } ).find( "matchPairsGuided failed" ) != std::string::npos );
        }
        delete L; delete R; delete lj; delete rj;
        ps.uninit();
    }
    std::printf( "%s\n", fails ? "FAILED" : "ALL OK" );
    return fails ? 1 : 0;
}
