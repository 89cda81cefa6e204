// Test of the pair search through the C++ host API: the record layouts of include/popsift_hip.h, popsift::MatchOptions'
// defaults, and FeaturesDev::matchPairs' argument errors (a null argument, two objects on different devices) -- all
// before a device is touched (this runs without a GPU).
// With POPSIFT_TEST_EXPECT_GPU set (the -m gpu test): two views of a synthetic frame go through PopSift in MatchingMode;
// for float and for byte descriptors, with and without the cross-check, matchPairs' descriptor indices and distances equal
// the C-ABI's pairs on the same device arrays and its feature indices are the reverse maps applied to them.
#include <popsift/popsift.h>
#include <popsift/features.h>
#include <popsift/sift_conf.h>
#include <popsift_hip.h>

#include <climits>
#include <cmath>
#include <cstddef>
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

static_assert( sizeof(psx_match_pair) == 16 && sizeof(psx_match_pair_u8) == 16 && sizeof(psx_match_opts) == 8, "record sizes" );
static_assert( offsetof(psx_match_pair, right) == 4 && offsetof(psx_match_pair, d1) == 8 && offsetof(psx_match_pair, d2) == 12, "layout" );
static_assert( offsetof(psx_match_pair_u8, right) == 4 && offsetof(psx_match_pair_u8, d1) == 8 && offsetof(psx_match_pair_u8, d2) == 12, "layout" );

int main()
{
    const bool gpu = std::getenv( "POPSIFT_TEST_EXPECT_GPU" ) != nullptr;
    {
        popsift::MatchOptions mo;
        CHECK( mo.ratio == 0.8f && !mo.mutual && !mo.bytes );
        psx_match_opts po = { 0.0f, 7 };
        CHECK( psx_match_opts_default( &po ) == PSX_OK && po.ratio == 0.8f && po.flags == 0 );
        CHECK( psx_match_opts_default( nullptr ) == PSX_ERR_INVALID );
        CHECK( PSX_PAIRS_MUTUAL == 1 );
        popsift::Match m = { 1, 2, 3, 4, 5.0f, 6.0f };
        CHECK( m.left_feature == 1 && m.right_feature == 2 && m.left_descriptor == 3 && m.right_descriptor == 4 &&
               m.distance == 5.0f && m.second_distance == 6.0f );
    }
    {   // argument errors, in the file:line + message format, before any device call
        popsift::FeaturesDev a, b;
        const std::string e = runtime_error_of( [&]{ a.matchPairs( nullptr ); } );
        CHECK( e.find( "features.cpp:" ) != std::string::npos && e.find( "\n    " ) != std::string::npos && e.find( "null argument" ) != std::string::npos );
        CHECK( !runtime_error_of( [&]{ a.matchPairs( nullptr, popsift::MatchOptions() ); } ).empty() );
        b.setDevice( 1 );
        const std::string e2 = runtime_error_of( [&]{ a.matchPairs( &b ); } );
        CHECK( e2.find( "different devices" ) != std::string::npos );
        b.setDevice( 0 );
        CHECK( a.matchPairs( &b ).empty() );                  // two empty objects: no pairs, no device call
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
        cfg.setNormalizationMultiplier( 9 );              // descriptors on the byte scale (up to 512): the byte form keeps their structure
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
            for( int mutual = 0; mutual < 2; mutual++ ) {
                popsift::MatchOptions mo;
                mo.mutual = mutual != 0;
                const std::vector<popsift::Match> mm = L->matchPairs( R, mo );
                psx_match_opts po = { 0.8f, mutual ? PSX_PAIRS_MUTUAL : 0 };
                std::vector<psx_match_pair> pp( nl );
                int n = -1;
                CHECK( psx_match_pairs( 0, (const float*)L->getDescriptors(), nl, (const float*)R->getDescriptors(), nr, &po, pp.data(), nl, &n ) == PSX_OK );
                std::printf( "float, mutual %d: %d pairs\n", mutual, n );
                CHECK( n > 10 && (int)mm.size() == n );
                for( int k = 0; k < n && k < (int)mm.size(); k++ ) {
                    CHECK( mm[k].left_descriptor == pp[k].left && mm[k].right_descriptor == pp[k].right );
                    CHECK( mm[k].distance == pp[k].d1 && mm[k].second_distance == pp[k].d2 );
                    CHECK( mm[k].left_feature == lrev[pp[k].left] && mm[k].right_feature == rrev[pp[k].right] );
                    if( k > 0 ) CHECK( mm[k].left_descriptor > mm[k - 1].left_descriptor );
                }
                // bytes: the C-ABI on descriptors quantised the same way
                mo.bytes = true;
                const std::vector<popsift::Match> mb = L->matchPairs( R, mo );
                void *lb = nullptr, *rb = nullptr;
                CHECK( psx_dev_alloc( 0, (size_t)nl * 128, &lb ) == PSX_OK && psx_dev_alloc( 0, (size_t)nr * 128, &rb ) == PSX_OK );
                CHECK( psx_quantize_desc( 0, (const float*)L->getDescriptors(), nl, (unsigned char*)lb ) == PSX_OK );
                CHECK( psx_quantize_desc( 0, (const float*)R->getDescriptors(), nr, (unsigned char*)rb ) == PSX_OK );
                std::vector<psx_match_pair_u8> pb( nl );
                n = -1;
                CHECK( psx_match_pairs_u8( 0, (const unsigned char*)lb, nl, (const unsigned char*)rb, nr, &po, pb.data(), nl, &n ) == PSX_OK );
                std::printf( "bytes, mutual %d: %d pairs\n", mutual, n );
                CHECK( n > 10 && (int)mb.size() == n );
                for( int k = 0; k < n && k < (int)mb.size(); k++ ) {
                    CHECK( mb[k].left_descriptor == pb[k].left && mb[k].right_descriptor == pb[k].right );
                    CHECK( mb[k].distance == ( pb[k].d1 == INT_MAX ? INFINITY : (float)pb[k].d1 ) );
                    CHECK( mb[k].second_distance == ( pb[k].d2 == INT_MAX ? INFINITY : (float)pb[k].d2 ) );
                    CHECK( mb[k].left_feature == lrev[pb[k].left] && mb[k].right_feature == rrev[pb[k].right] );
                }
                psx_dev_free( 0, lb ); psx_dev_free( 0, rb );
            }
            // a failing call: a ratio the C-ABI refuses
            popsift::MatchOptions bad;
            bad.ratio = -1.0f;
            CHECK( runtime_error_of( [&]{ L->matchPairs( R, bad ); } ).find( "matchPairs failed" ) != std::string::npos );
        }
        delete L; delete R; delete lj; delete rj;
        ps.uninit();
    }
    std::printf( "%s\n", fails ? "FAILED" : "ALL OK" );
    return fails ? 1 : 0;
}
