// Test of the affine and similarity estimators through the C++ host API: FeaturesDev::estimateAffine's and
// estimateSimilarity's argument errors (a null argument, two objects on different devices, invalid options), the batched
// forms' and the C-ABI's own argument checks -- all before a device is touched (this part runs without a GPU).
// With POPSIFT_TEST_EXPECT_GPU set (the -m gpu test): two views of a synthetic frame, the second shifted by 3 pixels, go
// through PopSift in MatchingMode; each estimate on matchPairs' list equals its psx_ransac_* call on the same device arrays
// (model bit for bit, counts, the inlier list), the model's last row is exactly (0, 0, 1), the returned guide is a
// homography accepted by matchPairsGuided and every inlier reappears in the guided list; the first three matches alone
// give an affine and a similarity model where estimateHomography has none.
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

typedef popsift::HomographyEstimate (popsift::FeaturesDev::*EstimateFn)( popsift::FeaturesDev*, const std::vector<popsift::Match>&, const popsift::RansacOptions& );
typedef std::vector<popsift::HomographyEstimate> (popsift::FeaturesDev::*EstimateManyFn)( const std::vector<popsift::FeaturesDev*>&,
                                                                                          const std::vector<std::vector<popsift::Match>>&,
                                                                                          const popsift::RansacOptions& );
typedef int (*RansacFn)( int, const void*, int, const float*, int, const float*, int, const psx_ransac_opts*, psx_ransac_result*, void*, int, int*, float*, int* );
typedef int (*RansacManyFn)( int, const void*, const int*, int, const float*, int, const float* const*, const int*, const psx_ransac_opts*,
                             psx_ransac_result*, void*, int, int*, float*, int* );
typedef int (*FitFn)( const float*, const float*, int, float* );

struct Model {
    const char* name; int min_pairs; EstimateFn estimate; EstimateManyFn estimate_many; RansacFn host, dev; RansacManyFn many, many_dev; FitFn fit;
};
static const Model models[2] = {
    { "estimateAffine", 3, &popsift::FeaturesDev::estimateAffine, &popsift::FeaturesDev::estimateAffineMany, psx_ransac_affine, psx_ransac_affine_dev,
      psx_ransac_affine_many, psx_ransac_affine_many_dev, psx_affine_fit },
    { "estimateSimilarity", 2, &popsift::FeaturesDev::estimateSimilarity, &popsift::FeaturesDev::estimateSimilarityMany, psx_ransac_similarity,
      psx_ransac_similarity_dev, psx_ransac_similarity_many, psx_ransac_similarity_many_dev, psx_similarity_fit },
};

int main()
{
    const bool gpu = std::getenv( "POPSIFT_TEST_EXPECT_GPU" ) != nullptr;
    const float nan = std::numeric_limits<float>::quiet_NaN();
    for( const Model& M : models ) {
        {   // argument errors, in the file:line + message format, before any device call
            popsift::FeaturesDev a, b;
            std::vector<popsift::Match> none;
            const std::string e = runtime_error_of( [&]{ ( a.*M.estimate )( nullptr, none, popsift::RansacOptions() ); } );
            CHECK( e.find( "features.cpp:" ) != std::string::npos && e.find( std::string( M.name ) + ": null argument" ) != std::string::npos );
            b.setDevice( 1 );
            CHECK( runtime_error_of( [&]{ ( a.*M.estimate )( &b, none, popsift::RansacOptions() ); } ).find( "different devices" ) != std::string::npos );
            b.setDevice( 0 );
            std::vector<popsift::Match> few( M.min_pairs - 1 );                          // below the minimum: no model, no device call
            std::memset( few.data(), 0, few.size() * sizeof(popsift::Match) );
            const popsift::HomographyEstimate est = ( a.*M.estimate )( &b, few, popsift::RansacOptions() );
            CHECK( est.best == -1 && est.inliers.empty() && est.guide.kind == popsift::MatchGuide::Homography && est.guide.tol == 2.0f );
            for( int k = 0; k < 9; k++ ) CHECK( est.guide.m[k] == 0.0f );
            popsift::RansacOptions bad;
            bad.tol = nan;
            CHECK( runtime_error_of( [&]{ ( a.*M.estimate )( &b, none, bad ); } ).find( "invalid options" ) != std::string::npos );
            bad = popsift::RansacOptions(); bad.hypotheses = 65537;
            CHECK( runtime_error_of( [&]{ ( a.*M.estimate )( &b, none, bad ); } ).find( "invalid options" ) != std::string::npos );
            // enough matches on two empty objects: the indices lie outside
            std::vector<popsift::Match> enough( M.min_pairs );
            std::memset( enough.data(), 0, enough.size() * sizeof(popsift::Match) );
            CHECK( runtime_error_of( [&]{ ( a.*M.estimate )( &b, enough, popsift::RansacOptions() ); } ).find( std::string( M.name ) + " failed" ) != std::string::npos );
            // the batched form: sizes, null entries, and lists below the minimum without a device
            std::vector<popsift::FeaturesDev*> others( 2, &b );
            std::vector<std::vector<popsift::Match>> lists( 1 );
            CHECK( runtime_error_of( [&]{ ( a.*M.estimate_many )( others, lists, popsift::RansacOptions() ); } ).find( "2 objects but 1 match lists" ) != std::string::npos );
            lists.resize( 2 );
            lists[1] = few;
            const std::vector<popsift::HomographyEstimate> ests = ( a.*M.estimate_many )( others, lists, popsift::RansacOptions() );
            CHECK( ests.size() == 2 && ests[0].best == -1 && ests[1].best == -1 && ests[1].guide.kind == popsift::MatchGuide::Homography );
            others[1] = nullptr;
            CHECK( runtime_error_of( [&]{ ( a.*M.estimate_many )( others, lists, popsift::RansacOptions() ); } ).find( "null argument" ) != std::string::npos );
        }
        {   // the C-ABI checks its arguments before it touches a device
            psx_ransac_opts o;
            CHECK( psx_ransac_opts_default( &o ) == PSX_OK );
            psx_ransac_result r;
            int n = -5;
            CHECK( M.host( 0, nullptr, 0, nullptr, 0, nullptr, 0, &o, &r, nullptr, 0, &n, nullptr, nullptr ) == PSX_OK && n == 0 && r.best == -1 );
            n = -5;
            CHECK( M.host( 0, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, &r, nullptr, 0, &n, nullptr, nullptr ) == PSX_ERR_INVALID );
            CHECK( M.dev( 0, nullptr, 9, nullptr, 0, nullptr, 0, &o, &r, nullptr, 0, &n, nullptr, nullptr ) == PSX_ERR_INVALID );
            CHECK( M.many( 0, nullptr, nullptr, 1, nullptr, 0, nullptr, nullptr, &o, &r, nullptr, 0, &n, nullptr, nullptr ) == PSX_ERR_INVALID );
            CHECK( M.many_dev( 0, nullptr, nullptr, -1, nullptr, 0, nullptr, nullptr, &o, &r, nullptr, 0, &n, nullptr, nullptr ) == PSX_ERR_INVALID );
            o.flags = 2;
            CHECK( M.dev( 0, nullptr, 0, nullptr, 0, nullptr, 0, &o, &r, nullptr, 0, &n, nullptr, nullptr ) == PSX_ERR_INVALID );
            CHECK( M.many( 0, nullptr, nullptr, 0, nullptr, 0, nullptr, nullptr, &o, nullptr, nullptr, 0, &n, nullptr, nullptr ) == PSX_ERR_INVALID );
            CHECK( n == -5 );
            o.flags = 0;
            CHECK( M.many( 0, nullptr, nullptr, 0, nullptr, 0, nullptr, nullptr, &o, nullptr, nullptr, 0, &n, nullptr, nullptr ) == PSX_OK && n == 0 );
            // the fit: too few points, null arrays; then the identity from points onto themselves
            const float xy[6] = { 10.f, 20.f, 300.f, 40.f, 150.f, 400.f };
            float m[9] = { -7.f, -7.f, -7.f, -7.f, -7.f, -7.f, -7.f, -7.f, -7.f };
            CHECK( M.fit( xy, xy, M.min_pairs - 1, m ) == PSX_ERR_INVALID && M.fit( nullptr, xy, 3, m ) == PSX_ERR_INVALID );
            CHECK( M.fit( xy, nullptr, 3, m ) == PSX_ERR_INVALID && M.fit( xy, xy, 3, nullptr ) == PSX_ERR_INVALID && m[0] == -7.f && m[8] == -7.f );
            CHECK( M.fit( xy, xy, 3, m ) == PSX_OK );
            const float ident[9] = { 1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f };
            for( int k = 0; k < 9; k++ ) CHECK( std::fabs( m[k] - ident[k] ) < 1e-4f );
            CHECK( m[6] == 0.0f && m[7] == 0.0f && m[8] == 1.0f );
            int idx[3] = { -7, -7, -7 };
            CHECK( psx_ransac_samples_k( 0u, 0, 1, M.min_pairs - 1, M.min_pairs, idx ) == PSX_ERR_INVALID && idx[0] == -7 );
            CHECK( psx_ransac_samples_k( 0u, 0, 1, M.min_pairs, M.min_pairs, idx ) == PSX_OK );
            int seen = 0;
            for( int k = 0; k < M.min_pairs; k++ ) if( idx[k] >= 0 && idx[k] < M.min_pairs ) seen |= 1 << idx[k];
            CHECK( seen == ( 1 << M.min_pairs ) - 1 );                                 // all of them: a permutation
        }
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
            void *lxy = nullptr, *rxy = nullptr;
            CHECK( psx_dev_alloc( 0, (size_t)nl * 8, &lxy ) == PSX_OK && psx_dev_alloc( 0, (size_t)nr * 8, &rxy ) == PSX_OK );
            CHECK( psx_desc_positions( 0, (const psx_feature_dev*)L->getFeatures(), L->getReverseMap(), nl, (float*)lxy ) == PSX_OK );
            CHECK( psx_desc_positions( 0, (const psx_feature_dev*)R->getFeatures(), R->getReverseMap(), nr, (float*)rxy ) == PSX_OK );
            for( const Model& M : models ) {
                popsift::RansacOptions ro;
                ro.tol = 1.5f; ro.hypotheses = 300; ro.seed = 5u;
                for( int refit = 0; refit < 2; refit++ ) {
                    ro.refit = refit != 0;
                    const popsift::HomographyEstimate est = ( L->*M.estimate )( R, mm, ro );
                    std::vector<psx_match_pair> rec( n ), inl( n );
                    for( int k = 0; k < n; k++ ) { rec[k].left = mm[k].left_descriptor; rec[k].right = mm[k].right_descriptor; rec[k].d1 = mm[k].distance; rec[k].d2 = mm[k].second_distance; }
                    psx_ransac_opts po = { ro.tol, ro.hypotheses, ro.seed, refit ? PSX_RANSAC_REFIT : 0 };
                    psx_ransac_result res;
                    int cnt = -1;
                    CHECK( M.host( 0, rec.data(), n, (const float*)lxy, nl, (const float*)rxy, nr, &po, &res, inl.data(), n, &cnt, nullptr, nullptr ) == PSX_OK );
                    std::printf( "%s: refit %d, %d matches, %d inliers (sample %d), model %g %g %g / %g %g %g / %g %g %g\n", M.name, refit, n, cnt,
                                 res.sample_inliers, res.m[0], res.m[1], res.m[2], res.m[3], res.m[4], res.m[5], res.m[6], res.m[7], res.m[8] );
                    CHECK( est.guide.kind == popsift::MatchGuide::Homography );
                    CHECK( res.m[6] == 0.0f && res.m[7] == 0.0f && res.m[8] == 1.0f );
                    CHECK( std::memcmp( est.guide.m, res.m, sizeof res.m ) == 0 && est.best == res.best && est.sample_inliers == res.sample_inliers );
                    CHECK( est.refit_kept == ( res.refit_kept != 0 ) && (int)est.inliers.size() == cnt && cnt * 2 > n && est.guide.tol == ro.tol );
                    // the planted shift: the identity moved by 3 pixels along x
                    CHECK( std::fabs( res.m[0] - 1.0f ) < 0.02f && std::fabs( res.m[4] - 1.0f ) < 0.02f && std::fabs( res.m[2] - (float)shift ) < 1.5f );
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
                    // the batched form on the same list, next to a list below the minimum
                    std::vector<popsift::FeaturesDev*> others( 2, R );
                    std::vector<std::vector<popsift::Match>> lists( 2 );
                    lists[0] = mm;
                    lists[1].assign( mm.begin(), mm.begin() + ( M.min_pairs - 1 ) );
                    const std::vector<popsift::HomographyEstimate> ests = ( L->*M.estimate_many )( others, lists, ro );
                    CHECK( ests.size() == 2 && ests[1].best == -1 && ests[1].inliers.empty() );
                    CHECK( std::memcmp( ests[0].guide.m, res.m, sizeof res.m ) == 0 && ests[0].best == res.best && (int)ests[0].inliers.size() == cnt );
                }
                // three matches: a model here, none from estimateHomography
                std::vector<popsift::Match> three;                                   // of three different features: three different positions
                for( const popsift::Match& m : mm )
                    if( three.size() < 3 && ( three.empty() || m.left_feature > three.back().left_feature + 20 ) ) three.push_back( m );
                CHECK( three.size() == 3 );
                ro.hypotheses = 16; ro.refit = false;
                const popsift::HomographyEstimate small = ( L->*M.estimate )( R, three, ro );
                CHECK( small.best >= 0 && small.guide.m[8] == 1.0f && L->estimateHomography( R, three, ro ).best == -1 );
                ro.hypotheses = 70000;
                CHECK( runtime_error_of( [&]{ ( L->*M.estimate )( R, mm, ro ); } ).find( "invalid options" ) != std::string::npos );
                std::vector<popsift::Match> outside( mm.begin(), mm.begin() + 9 );
                outside[3].right_descriptor = nr;
                ro.hypotheses = 16;
                CHECK( runtime_error_of( [&]{ ( L->*M.estimate )( R, outside, ro ); } ).find( std::string( M.name ) + " failed" ) != std::string::npos );
            }
            psx_dev_free( 0, lxy ); psx_dev_free( 0, rxy );
        }
        delete L; delete R; delete lj; delete rj;
        ps.uninit();
    }
    std::printf( "%s\n", fails ? "FAILED" : "ALL OK" );
    return fails ? 1 : 0;
}
