// Test of the fundamental-matrix estimator through the C++ host API: FeaturesDev::estimateFundamental's argument errors (a
// null argument, two objects on different devices, invalid options) and the C-ABI's own argument checks -- all before a
// device is touched (this part runs without a GPU).
// With POPSIFT_TEST_EXPECT_GPU set (the -m gpu test): two views of a synthetic frame, the second shifted by 3 pixels, go
// through PopSift in MatchingMode; estimateFundamental on matchPairs' list equals psx_ransac_fundamental on the same device
// arrays (model bit for bit, counts, the inlier list), the returned guide is an epipolar one accepted by matchPairsGuided
// and every inlier reappears in the guided list.
#include <popsift/popsift.h>
#include <popsift/features.h>
#include <popsift/sift_conf.h>
#include <popsift_hip.h>

#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

int main()
{
    const bool gpu = std::getenv( "POPSIFT_TEST_EXPECT_GPU" ) != nullptr;
    const float nan = std::numeric_limits<float>::quiet_NaN();
    {   // argument errors, in the file:line + message format, before any device call
        popsift::FeaturesDev a, b;
        std::vector<popsift::Match> none;
        const std::string e = runtime_error_of( [&]{ a.estimateFundamental( nullptr, none ); } );
        CHECK( e.find( "features.cpp:" ) != std::string::npos && e.find( "estimateFundamental: null argument" ) != std::string::npos );
        b.setDevice( 1 );
        CHECK( runtime_error_of( [&]{ a.estimateFundamental( &b, none ); } ).find( "different devices" ) != std::string::npos );
        b.setDevice( 0 );
        std::vector<popsift::Match> seven( 7 );                                        // fewer than 8: no model, no device call
        std::memset( seven.data(), 0, seven.size() * sizeof(popsift::Match) );
        const popsift::FundamentalEstimate est = a.estimateFundamental( &b, seven );
        CHECK( est.best == -1 && est.inliers.empty() && est.guide.kind == popsift::MatchGuide::Epipolar && est.guide.tol == 2.0f );
        for( int k = 0; k < 9; k++ ) CHECK( est.guide.m[k] == 0.0f );
        popsift::RansacOptions bad;
        bad.tol = nan;
        CHECK( runtime_error_of( [&]{ a.estimateFundamental( &b, none, bad ); } ).find( "invalid options" ) != std::string::npos );
        bad = popsift::RansacOptions(); bad.hypotheses = 65537;
        CHECK( runtime_error_of( [&]{ a.estimateFundamental( &b, none, bad ); } ).find( "invalid options" ) != std::string::npos );
        // eight matches on two empty objects: the indices lie outside
        std::vector<popsift::Match> eight( 8 );
        std::memset( eight.data(), 0, eight.size() * sizeof(popsift::Match) );
        CHECK( runtime_error_of( [&]{ a.estimateFundamental( &b, eight ); } ).find( "estimateFundamental failed" ) != std::string::npos );
    }
    {   // the C-ABI checks its arguments before it touches a device
        psx_ransac_opts o;
        CHECK( psx_ransac_opts_default( &o ) == PSX_OK );
        psx_ransac_result r;
        int n = -5;
        CHECK( psx_ransac_fundamental( 0, nullptr, 0, nullptr, 0, nullptr, 0, &o, &r, nullptr, 0, &n, nullptr, nullptr ) == PSX_OK && n == 0 && r.best == -1 );
        n = -5;
        CHECK( psx_ransac_fundamental( 0, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, &r, nullptr, 0, &n, nullptr, nullptr ) == PSX_ERR_INVALID );
        CHECK( psx_ransac_fundamental_dev( 0, nullptr, 9, nullptr, 0, nullptr, 0, &o, &r, nullptr, 0, &n, nullptr, nullptr ) == PSX_ERR_INVALID );
        o.flags = 2;
        CHECK( psx_ransac_fundamental_dev( 0, nullptr, 0, nullptr, 0, nullptr, 0, &o, &r, nullptr, 0, &n, nullptr, nullptr ) == PSX_ERR_INVALID );
        CHECK( n == -5 );
        int idx[8] = { -7, -7, -7, -7, -7, -7, -7, -7 };
        CHECK( psx_ransac_samples_k( 0u, 0, 1, 8, 5, idx ) == PSX_ERR_INVALID && psx_ransac_samples_k( 0u, 0, 1, 7, 8, idx ) == PSX_ERR_INVALID && idx[0] == -7 );
        CHECK( psx_ransac_samples_k( 0u, 0, 1, 8, 8, idx ) == PSX_OK );
        int seen = 0;
        for( int k = 0; k < 8; k++ ) if( idx[k] >= 0 && idx[k] < 8 ) seen |= 1 << idx[k];
        CHECK( seen == 255 );                                                          // eight of eight: a permutation
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
        cfg.setNormalizationMultiplier( 9 );
        PopSift ps( cfg, popsift::Config::MatchingMode, PopSift::ByteImages );
        SiftJob* lj = ps.enqueue( w, h, img.data() );
        SiftJob* rj = ps.enqueue( w, h, img2.data() );
        popsift::FeaturesDev* L = lj->getDev();
        popsift::FeaturesDev* R = rj->getDev();
        CHECK( L != nullptr && R != nullptr );
        if( L && R ) {
            const int nl = L->getDescriptorCount(), nr = R->getDescriptorCount();
            popsift::MatchOptions mo;
            mo.mutual = true;
            const std::vector<popsift::Match> mm = L->matchPairs( R, mo );
            const int n = (int)mm.size();
            CHECK( n > 30 );
            popsift::RansacOptions ro;
            ro.tol = 1.5f; ro.hypotheses = 300; ro.seed = 5u;
            for( int refit = 0; refit < 2; refit++ ) {
                ro.refit = refit != 0;
                const popsift::FundamentalEstimate est = L->estimateFundamental( R, mm, ro );
                // the C-ABI on the same arrays
                void *lxy = nullptr, *rxy = nullptr;
                CHECK( psx_dev_alloc( 0, (size_t)nl * 8, &lxy ) == PSX_OK && psx_dev_alloc( 0, (size_t)nr * 8, &rxy ) == PSX_OK );
                CHECK( psx_desc_positions( 0, (const psx_feature_dev*)L->getFeatures(), L->getReverseMap(), nl, (float*)lxy ) == PSX_OK );
                CHECK( psx_desc_positions( 0, (const psx_feature_dev*)R->getFeatures(), R->getReverseMap(), nr, (float*)rxy ) == PSX_OK );
                std::vector<psx_match_pair> rec( n ), inl( n );
                for( int k = 0; k < n; k++ ) { rec[k].left = mm[k].left_descriptor; rec[k].right = mm[k].right_descriptor; rec[k].d1 = mm[k].distance; rec[k].d2 = mm[k].second_distance; }
                psx_ransac_opts po = { ro.tol, ro.hypotheses, ro.seed, refit ? PSX_RANSAC_REFIT : 0 };
                psx_ransac_result res;
                int cnt = -1;
                CHECK( psx_ransac_fundamental( 0, rec.data(), n, (const float*)lxy, nl, (const float*)rxy, nr, &po, &res, inl.data(), n, &cnt, nullptr, nullptr ) == PSX_OK );
                psx_dev_free( 0, lxy ); psx_dev_free( 0, rxy );
                std::printf( "estimateFundamental: refit %d, %d matches, %d inliers (sample %d), model %g %g %g / %g %g %g / %g %g %g\n", refit, n, cnt,
                             res.sample_inliers, res.m[0], res.m[1], res.m[2], res.m[3], res.m[4], res.m[5], res.m[6], res.m[7], res.m[8] );
                CHECK( est.guide.kind == popsift::MatchGuide::Epipolar );
                CHECK( std::memcmp( est.guide.m, res.m, sizeof res.m ) == 0 && est.best == res.best && est.sample_inliers == res.sample_inliers );
                CHECK( est.refit_kept == ( res.refit_kept != 0 ) && (int)est.inliers.size() == cnt && cnt * 2 > n && est.guide.tol == ro.tol );
                for( int k = 0; k < cnt && k < (int)est.inliers.size(); k++ ) {
                    CHECK( est.inliers[k].left_descriptor == inl[k].left && est.inliers[k].right_descriptor == inl[k].right );
                    CHECK( est.inliers[k].distance == inl[k].d1 && est.inliers[k].second_distance == inl[k].d2 );
                }
                // the guide is accepted, and every inlier is a pair of the guided list (best among all is best among the admissible)
                const std::vector<popsift::Match> gm = L->matchPairsGuided( R, est.guide, mo );
                CHECK( (int)gm.size() >= cnt );
                size_t g = 0;
                for( int k = 0; k < (int)est.inliers.size(); k++ ) {
                    while( g < gm.size() && gm[g].left_descriptor < est.inliers[k].left_descriptor ) g++;
                    CHECK( g < gm.size() && gm[g].left_descriptor == est.inliers[k].left_descriptor && gm[g].right_descriptor == est.inliers[k].right_descriptor );
                }
            }
            ro.hypotheses = 70000;
            CHECK( runtime_error_of( [&]{ L->estimateFundamental( R, mm, ro ); } ).find( "invalid options" ) != std::string::npos );
            std::vector<popsift::Match> outside( mm.begin(), mm.begin() + 9 );
            outside[3].right_descriptor = nr;
            ro.hypotheses = 16;
            CHECK( runtime_error_of( [&]{ L->estimateFundamental( R, outside, ro ); } ).find( "estimateFundamental failed" ) != std::string::npos );
        }
        delete L; delete R; delete lj; delete rj;
        ps.uninit();
    }
    std::printf( "%s\n", fails ? "FAILED" : "ALL OK" );
    return fails ? 1 : 0;
}
