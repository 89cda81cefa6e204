// Test of the batched geometric verification through the C++ host API: FeaturesDev::estimateHomographyMany /
// estimateFundamentalMany's argument errors (a size mismatch between the objects and the lists, a null entry, an object on
// another device, invalid options), their "no model" form for short lists and the C-ABI's own argument checks -- all
// before a device is touched (this part runs without a GPU).
// With POPSIFT_TEST_EXPECT_GPU set (the -m gpu test): four views of a synthetic frame go through PopSift in MatchingMode;
// on matchPairsMany's lists (one of them cut below the minimum, one object twice) estimate*Many equals
// psx_ransac_*_many on the same objects' arrays and the loop of estimate*( others[k], lists[k] ), field by field, with
// and without the refit.
#include <popsift/popsift.h>
#include <popsift/features.h>
#include <popsift/sift_conf.h>
#include <popsift_hip.h>

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

static bool same( const popsift::Match& a, const popsift::Match& b )
{
    return a.left_feature == b.left_feature && a.right_feature == b.right_feature && a.left_descriptor == b.left_descriptor &&
           a.right_descriptor == b.right_descriptor && a.distance == b.distance && a.second_distance == b.second_distance;
}

static bool same( const popsift::HomographyEstimate& a, const popsift::HomographyEstimate& b )
{
    if( a.guide.kind != b.guide.kind || std::memcmp( a.guide.m, b.guide.m, sizeof a.guide.m ) != 0 || a.guide.tol != b.guide.tol ) return false;
    if( a.best != b.best || a.sample_inliers != b.sample_inliers || a.refit_kept != b.refit_kept || a.inliers.size() != b.inliers.size() ) return false;
    for( size_t q = 0; q < a.inliers.size(); q++ ) if( !same( a.inliers[q], b.inliers[q] ) ) return false;
    return true;
}

int main()
{
    const bool gpu = std::getenv( "POPSIFT_TEST_EXPECT_GPU" ) != nullptr;
    typedef std::vector<std::vector<popsift::Match>> Lists;
    {   // argument errors, in the file:line + message format, before any device call
        popsift::FeaturesDev a, b, c;
        const std::string e = runtime_error_of( [&]{ a.estimateFundamentalMany( { &b, &c }, Lists( 3 ) ); } );
        CHECK( e.find( "features.cpp:" ) != std::string::npos && e.find( "estimateFundamentalMany: 2 objects but 3 match lists" ) != std::string::npos );
        CHECK( runtime_error_of( [&]{ a.estimateHomographyMany( { &b }, Lists() ); } ).find( "estimateHomographyMany: 1 objects but 0 match lists" ) != std::string::npos );
        CHECK( runtime_error_of( [&]{ a.estimateHomographyMany( { &b, nullptr }, Lists( 2 ) ); } ).find( "null argument" ) != std::string::npos );
        c.setDevice( 1 );
        CHECK( runtime_error_of( [&]{ a.estimateFundamentalMany( { &b, &c }, Lists( 2 ) ); } ).find( "different devices" ) != std::string::npos );
        c.setDevice( 0 );
        popsift::RansacOptions bad;
        bad.tol = std::numeric_limits<float>::quiet_NaN();
        CHECK( runtime_error_of( [&]{ a.estimateFundamentalMany( { &b, &c }, Lists( 2 ), bad ); } ).find( "invalid options" ) != std::string::npos );
        bad = popsift::RansacOptions(); bad.hypotheses = 0;
        CHECK( runtime_error_of( [&]{ a.estimateHomographyMany( { &b, &c }, Lists( 2 ), bad ); } ).find( "invalid options" ) != std::string::npos );
        // lists below the minimum, no lists: "no model" per list, no device call
        Lists small( 2 );
        small[0].resize( 7 ); small[1].resize( 3 );
        std::memset( small[0].data(), 0, 7 * sizeof(popsift::Match) );
        std::memset( small[1].data(), 0, 3 * sizeof(popsift::Match) );
        const std::vector<popsift::FundamentalEstimate> f = a.estimateFundamentalMany( { &b, &c }, small );
        CHECK( f.size() == 2 );
        for( const auto& est : f ) {
            CHECK( est.best == -1 && est.inliers.empty() && est.guide.kind == popsift::MatchGuide::Epipolar && est.guide.tol == 2.0f );
            for( int k = 0; k < 9; k++ ) CHECK( est.guide.m[k] == 0.0f );
        }
        CHECK( a.estimateHomographyMany( {}, Lists() ).empty() );
        // seven matches may have a homography: the indices lie outside the empty objects
        CHECK( runtime_error_of( [&]{ a.estimateHomographyMany( { &b, &c }, small ); } ).find( "estimateHomographyMany failed" ) != std::string::npos );
    }
    {   // the C-ABI checks its arguments before it touches a device
        psx_ransac_opts o;
        CHECK( psx_ransac_opts_default( &o ) == PSX_OK );
        psx_ransac_result r[2];
        int n = -5;
        const int counts[2] = { 7, 0 }, lens[2] = { 9, 0 };
        const float* const fake = reinterpret_cast<const float*>( 0x1000 );
        const float* rxy[2] = { fake, nullptr };
        CHECK( psx_ransac_fundamental_many( 0, nullptr, nullptr, 0, nullptr, 0, nullptr, nullptr, &o, nullptr, nullptr, 0, &n, nullptr, nullptr ) == PSX_OK && n == 0 );
        n = -5;
        CHECK( psx_ransac_fundamental_many_dev( 0, fake, counts, 2, fake, 9, rxy, lens, &o, r, nullptr, 0, &n, nullptr, nullptr ) == PSX_OK && n == 0 );
        CHECK( r[0].best == -1 && r[1].best == -1 );                                   // seven pairs: below the minimum
        n = -5;
        CHECK( psx_ransac_homography_many_dev( 0, fake, counts, -1, fake, 9, rxy, lens, &o, r, nullptr, 0, &n, nullptr, nullptr ) == PSX_ERR_INVALID );
        CHECK( psx_ransac_homography_many( 0, fake, counts, 2, fake, 9, rxy, lens, nullptr, r, nullptr, 0, &n, nullptr, nullptr ) == PSX_ERR_INVALID );
        rxy[0] = nullptr;
        CHECK( psx_ransac_homography_many( 0, fake, counts, 2, fake, 9, rxy, lens, &o, r, nullptr, 0, &n, nullptr, nullptr ) == PSX_ERR_INVALID );
        CHECK( n == -5 );
        psx_ransac_block blk[4];
        int nb = -5;
        const int three[3] = { 600, 3, 256 };
        CHECK( psx_ransac_many_plan( three, 3, 4, 256, blk, 4, &nb ) == PSX_OK && nb == 4 );
        CHECK( blk[0].set == 0 && blk[0].first == 0 && blk[2].end == 600 && blk[3].set == 2 && blk[3].first == 603 && blk[3].end == 859 );
        CHECK( psx_ransac_many_plan( three, 3, 0, 256, blk, 4, &nb ) == PSX_ERR_INVALID && psx_ransac_many_plan( three, 3, 4, 0, blk, 4, &nb ) == PSX_ERR_INVALID );
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
            const std::vector<popsift::FeaturesDev*> others = { f[1], f[2], f[3], f[1] };      // the same object twice
            popsift::MatchOptions mo;
            mo.mutual = true;
            mo.bytes = true;
            Lists lists = f[0]->matchPairsMany( others, mo );
            CHECK( lists.size() == 4 && lists[0].size() > 30 && lists[1].size() > 30 && lists[2].size() > 30 );
            if( lists.size() == 4 && lists[2].size() > 30 ) {
                lists[2].resize( 3 );                                                          // below either minimum: no model
                const int K = 4, nl = f[0]->getDescriptorCount();
                popsift::RansacOptions ro;
                ro.tol = 1.5f; ro.hypotheses = 300; ro.seed = 5u;
                for( int fundamental = 0; fundamental < 2; fundamental++ )
                    for( int refit = 0; refit < 2; refit++ ) {
                        ro.refit = refit != 0;
                        const std::vector<popsift::HomographyEstimate> est = fundamental ? f[0]->estimateFundamentalMany( others, lists, ro )
                                                                                         : f[0]->estimateHomographyMany( others, lists, ro );
                        CHECK( est.size() == 4 );
                        // the loop of single estimates
                        for( int k = 0; k < K && k < (int)est.size(); k++ ) {
                            const popsift::HomographyEstimate one = fundamental ? f[0]->estimateFundamental( others[k], lists[k], ro )
                                                                                : f[0]->estimateHomography( others[k], lists[k], ro );
                            CHECK( same( est[k], one ) );
                            CHECK( k == 2 ? est[k].best == -1 : ( est[k].best >= 0 && 2 * est[k].inliers.size() > lists[k].size() ) );
                        }
                        // the C-ABI on the same objects' arrays
                        std::vector<void*> bufs( K + 1, nullptr );
                        std::vector<const float*> rxy( K, nullptr );
                        std::vector<int> counts( K ), lens( K );
                        std::vector<psx_match_pair> rec;
                        CHECK( psx_dev_alloc( 0, (size_t)nl * 8, &bufs[K] ) == PSX_OK );
                        CHECK( psx_desc_positions( 0, (const psx_feature_dev*)f[0]->getFeatures(), f[0]->getReverseMap(), nl, (float*)bufs[K] ) == PSX_OK );
                        for( int k = 0; k < K; k++ ) {
                            lens[k] = others[k]->getDescriptorCount();
                            counts[k] = (int)lists[k].size();
                            CHECK( psx_dev_alloc( 0, (size_t)lens[k] * 8, &bufs[k] ) == PSX_OK );
                            CHECK( psx_desc_positions( 0, (const psx_feature_dev*)others[k]->getFeatures(), others[k]->getReverseMap(), lens[k], (float*)bufs[k] ) == PSX_OK );
                            rxy[k] = (const float*)bufs[k];
                            for( const popsift::Match& m : lists[k] ) { psx_match_pair p = { m.left_descriptor, m.right_descriptor, m.distance, m.second_distance }; rec.push_back( p ); }
                        }
                        std::vector<psx_match_pair> inl( rec.size() );
                        std::vector<psx_ransac_result> res( K );
                        psx_ransac_opts po = { ro.tol, ro.hypotheses, ro.seed, refit ? PSX_RANSAC_REFIT : 0 };
                        int cnt = -1;
                        CHECK( ( fundamental ? psx_ransac_fundamental_many : psx_ransac_homography_many )( 0, rec.data(), counts.data(), K, (const float*)bufs[K], nl,
                                   rxy.data(), lens.data(), &po, res.data(), inl.data(), (int)inl.size(), &cnt, nullptr, nullptr ) == PSX_OK );
                        for( void* b : bufs ) psx_dev_free( 0, b );
                        size_t at = 0;
                        for( int k = 0; k < K && k < (int)est.size(); k++ ) {
                            CHECK( std::memcmp( est[k].guide.m, res[k].m, sizeof res[k].m ) == 0 && est[k].best == res[k].best );
                            CHECK( est[k].sample_inliers == res[k].sample_inliers && est[k].refit_kept == ( res[k].refit_kept != 0 ) );
                            CHECK( (int)est[k].inliers.size() == res[k].inliers );
                            for( size_t q = 0; q < est[k].inliers.size(); q++, at++ )
                                CHECK( est[k].inliers[q].left_descriptor == inl[at].left && est[k].inliers[q].right_descriptor == inl[at].right &&
                                       est[k].inliers[q].distance == inl[at].d1 );
                        }
                        CHECK( (int)at == cnt );
                        std::printf( "estimate%sMany: refit %d, %zu + %zu + %zu + %zu matches, %d inliers\n", fundamental ? "Fundamental" : "Homography", refit,
                                     lists[0].size(), lists[1].size(), lists[2].size(), lists[3].size(), cnt );
                    }
                ro.hypotheses = 70000;
                CHECK( runtime_error_of( [&]{ f[0]->estimateFundamentalMany( others, lists, ro ); } ).find( "invalid options" ) != std::string::npos );
                ro.hypotheses = 16;
                CHECK( runtime_error_of( [&]{ f[0]->estimateFundamentalMany( { f[1], f[2] }, lists, ro ); } ).find( "2 objects but 4 match lists" ) != std::string::npos );
                Lists outside = lists;
                outside[1][3].right_descriptor = others[1]->getDescriptorCount();
                CHECK( runtime_error_of( [&]{ f[0]->estimateHomographyMany( others, outside, ro ); } ).find( "estimateHomographyMany failed" ) != std::string::npos );
            }
        }
        for( auto* p : f ) delete p;
        for( auto* j : jobs ) delete j;
        ps.uninit();
    }
    std::printf( "%s\n", fails ? "FAILED" : "ALL OK" );
    return fails ? 1 : 0;
}
