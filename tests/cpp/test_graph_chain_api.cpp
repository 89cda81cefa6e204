// Test of the two edge-list calls behind matchPairsGraph through the C++ host API: the argument errors of
// FeaturesDev::estimate*Graph and matchPairsGuidedGraph (an edge index out of range, a size mismatch, a null referenced
// entry, views on different devices, invalid options, an invalid guide, float descriptors asked for) and their empty forms
// -- all before a device is touched (this part runs without a GPU).
// With POPSIFT_TEST_EXPECT_GPU set (the -m gpu test): four views of a synthetic frame go through PopSift in MatchingMode;
// over an unsorted edge list -- both orders of a pair, a self edge, a duplicate, an empty view -- the chain matchPairsGraph
// -> estimate*Graph -> matchPairsGuidedGraph equals, element by element and field by field, the loop of the single-edge
// member calls views[left]->estimate*( views[right], ... ) and views[left]->matchPairsGuided( views[right], ... ).
#include <popsift/popsift.h>
#include <popsift/features.h>
#include <popsift/sift_conf.h>
#include <popsift_hip.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
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

static bool same( const popsift::HomographyEstimate& a, const popsift::HomographyEstimate& b )
{
    if( a.guide.kind != b.guide.kind || std::memcmp( a.guide.m, b.guide.m, sizeof a.guide.m ) != 0 || a.guide.tol != b.guide.tol ) return false;
    if( a.best != b.best || a.sample_inliers != b.sample_inliers || a.refit_kept != b.refit_kept || a.inliers.size() != b.inliers.size() ) return false;
    for( size_t q = 0; q < a.inliers.size(); q++ ) if( !same( a.inliers[q], b.inliers[q] ) ) return false;
    return true;
}

typedef std::vector<std::pair<int,int>> Edges;
typedef std::vector<std::vector<popsift::Match>> Lists;
typedef popsift::FeaturesDev FD;

static bool has( const std::string& s, const char* what ) { return s.find( what ) != std::string::npos; }

int main()
{
    const bool gpu = std::getenv( "POPSIFT_TEST_EXPECT_GPU" ) != nullptr;
    {   // argument errors, in the file:line + message format, before any device call
        FD a, b, c;
        const std::string e0 = runtime_error_of( [&]{ FD::estimateHomographyGraph( { &a, &b }, Edges{ {0,1}, {0,2} }, Lists( 2 ) ); } );
        CHECK( has( e0, "features.cpp:" ) && has( e0, "estimateHomographyGraph" ) && has( e0, "out of range" ) );
        CHECK( has( runtime_error_of( [&]{ FD::estimateFundamentalGraph( { &a, &b }, Edges{ {-1,1} }, Lists( 1 ) ); } ), "out of range" ) );
        CHECK( has( runtime_error_of( [&]{ FD::estimateAffineGraph( {}, Edges{ {0,0} }, Lists( 1 ) ); } ), "out of range" ) );
        CHECK( has( runtime_error_of( [&]{ FD::estimateSimilarityGraph( { &a, &b }, Edges{ {0,1} }, Lists( 2 ) ); } ),
                    "estimateSimilarityGraph: 1 edges but 2 match lists" ) );
        CHECK( has( runtime_error_of( [&]{ FD::estimateHomographyGraph( { &a, nullptr }, Edges{ {0,1} }, Lists( 1 ) ); } ), "null argument" ) );
        // a null entry that no edge names is not looked at
        CHECK( FD::estimateHomographyGraph( { &a, nullptr, &b }, Edges{ {0,2} }, Lists( 1 ) ).size() == 1 );
        c.setDevice( 1 );
        CHECK( has( runtime_error_of( [&]{ FD::estimateFundamentalGraph( { &a, &b, &c }, Edges{ {0,1}, {1,2} }, Lists( 2 ) ); } ), "different devices" ) );
        c.setDevice( 0 );
        popsift::RansacOptions bad;
        bad.tol = std::numeric_limits<float>::quiet_NaN();
        CHECK( has( runtime_error_of( [&]{ FD::estimateFundamentalGraph( { &a, &b }, Edges{ {0,1} }, Lists( 1 ), bad ); } ), "invalid options" ) );
        bad = popsift::RansacOptions(); bad.hypotheses = 0;
        CHECK( has( runtime_error_of( [&]{ FD::estimateAffineGraph( { &a, &b }, Edges{ {0,1} }, Lists( 1 ), bad ); } ), "invalid options" ) );
        // lists below the minimum, no edges: "no model" per edge, no device call
        Lists small( 2 );
        small[0].resize( 7 ); small[1].resize( 3 );
        std::memset( small[0].data(), 0, 7 * sizeof(popsift::Match) );
        std::memset( small[1].data(), 0, 3 * sizeof(popsift::Match) );
        const std::vector<popsift::FundamentalEstimate> f = FD::estimateFundamentalGraph( { &a, &b, &c }, Edges{ {0,1}, {2,0} }, small );
        CHECK( f.size() == 2 );
        for( const auto& est : f ) {
            CHECK( est.best == -1 && est.inliers.empty() && est.guide.kind == popsift::MatchGuide::Epipolar && est.guide.tol == 2.0f );
            for( int k = 0; k < 9; k++ ) CHECK( est.guide.m[k] == 0.0f );
        }
        CHECK( FD::estimateHomographyGraph( {}, Edges{}, Lists() ).empty() );
        // seven matches may have a homography: the indices lie outside the empty objects
        CHECK( has( runtime_error_of( [&]{ FD::estimateHomographyGraph( { &a, &b, &c }, Edges{ {0,1}, {2,0} }, small ); } ), "estimateHomographyGraph failed" ) );

        popsift::MatchOptions mo;
        mo.bytes = true;
        popsift::MatchGuide h;
        h.kind = popsift::MatchGuide::Homography;
        for( int k = 0; k < 9; k++ ) h.m[k] = k % 4 == 0 ? 1.0f : 0.0f;
        h.tol = 2.0f;
        const std::vector<popsift::MatchGuide> g2 = { h, popsift::MatchGuide::none() };
        const std::string m0 = runtime_error_of( [&]{ FD::matchPairsGuidedGraph( { &a, &b }, Edges{ {0,1}, {0,2} }, g2, mo ); } );
        CHECK( has( m0, "features.cpp:" ) && has( m0, "matchPairsGuidedGraph" ) && has( m0, "out of range" ) );
        CHECK( has( runtime_error_of( [&]{ FD::matchPairsGuidedGraph( { &a, nullptr }, Edges{ {0,1}, {1,0} }, g2, mo ); } ), "null argument" ) );
        c.setDevice( 1 );
        CHECK( has( runtime_error_of( [&]{ FD::matchPairsGuidedGraph( { &a, &b, &c }, Edges{ {0,1}, {1,2} }, g2, mo ); } ), "different devices" ) );
        c.setDevice( 0 );
        CHECK( has( runtime_error_of( [&]{ FD::matchPairsGuidedGraph( { &a, &b }, Edges{ {0,1}, {1,0} }, g2, popsift::MatchOptions() ); } ), "byte-only" ) );
        CHECK( has( runtime_error_of( [&]{ FD::matchPairsGuidedGraph( { &a, &b }, Edges{ {0,1} }, g2, mo ); } ), "1 edges but 2 guides" ) );
        std::vector<popsift::MatchGuide> gb = g2;
        gb[1] = h; gb[1].tol = -1.0f;
        CHECK( has( runtime_error_of( [&]{ FD::matchPairsGuidedGraph( { &a, &b }, Edges{ {0,1}, {1,0} }, gb, mo ); } ), "invalid guide" ) );
        gb[1] = h; gb[1].m[4] = std::numeric_limits<float>::infinity();
        CHECK( has( runtime_error_of( [&]{ FD::matchPairsGuidedGraph( { &a, &b }, Edges{ {0,1}, {1,0} }, gb, mo ); } ), "invalid guide" ) );
        // empty objects, no edges: no pairs, no device call
        const Lists r = FD::matchPairsGuidedGraph( { &a, &b }, Edges{ {0,1}, {1,0} }, g2, mo );
        CHECK( r.size() == 2 && r[0].empty() && r[1].empty() );
        CHECK( FD::matchPairsGuidedGraph( {}, Edges{}, {}, mo ).empty() );
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
            std::printf( "descriptors: %d, %d, %d, %d\n", f[0]->getDescriptorCount(), f[1]->getDescriptorCount(),
                         f[2]->getDescriptorCount(), f[3]->getDescriptorCount() );
            FD empty;
            const std::vector<FD*> views = { f[0], f[1], f[2], &empty, f[3], nullptr };      // the null entry is not named
            const Edges edges = { {2,4}, {0,1}, {1,0}, {0,0}, {0,3}, {3,1}, {4,2}, {0,1}, {1,2} };
            popsift::MatchOptions mo;
            mo.mutual = true;
            mo.bytes = true;
            Lists lists = FD::matchPairsGraph( views, edges, mo );
            CHECK( lists.size() == edges.size() );
            lists[8].resize( 3 );                          // one list below the minimum of a homography and of a fundamental matrix
            for( int refit = 0; refit < 2; refit++ ) {
                popsift::RansacOptions ro;
                ro.hypotheses = 200;
                ro.seed = 5;
                ro.refit = refit != 0;
                for( int model = 0; model < 4; model++ ) {
                    std::vector<popsift::HomographyEstimate> got;
                    if( model == 0 ) got = FD::estimateHomographyGraph( views, edges, lists, ro );
                    if( model == 1 ) got = FD::estimateFundamentalGraph( views, edges, lists, ro );
                    if( model == 2 ) got = FD::estimateAffineGraph( views, edges, lists, ro );
                    if( model == 3 ) got = FD::estimateSimilarityGraph( views, edges, lists, ro );
                    CHECK( got.size() == edges.size() );
                    int models = 0;
                    for( size_t e = 0; e < edges.size() && e < got.size(); e++ ) {
                        FD* l = views[edges[e].first];
                        FD* r = views[edges[e].second];
                        popsift::HomographyEstimate one;
                        if( model == 0 ) one = l->estimateHomography( r, lists[e], ro );
                        if( model == 1 ) one = l->estimateFundamental( r, lists[e], ro );
                        if( model == 2 ) one = l->estimateAffine( r, lists[e], ro );
                        if( model == 3 ) one = l->estimateSimilarity( r, lists[e], ro );
                        CHECK( same( got[e], one ) );
                        models += got[e].best >= 0;
                    }
                    CHECK( models >= 5 );                 // the six live lists; a view against itself may have no fundamental matrix
                    std::printf( "estimate*Graph: model %d refit %d: %d of %zu edges have a model\n", model, refit, models, got.size() );
                    if( model > 1 ) continue;
                    // the results as guides (an estimate without a model skips its edge), then the guided re-match of all edges
                    std::vector<popsift::MatchGuide> guides;
                    for( const auto& est : got ) guides.push_back( est.best < 0 ? popsift::MatchGuide::none() : est.guide );
                    const Lists re = FD::matchPairsGuidedGraph( views, edges, guides, mo );
                    CHECK( re.size() == edges.size() );
                    size_t total = 0;
                    for( size_t e = 0; e < edges.size() && e < re.size(); e++ ) {
                        if( guides[e].kind == popsift::MatchGuide::None ) { CHECK( re[e].empty() ); continue; }
                        const std::vector<popsift::Match> one = views[edges[e].first]->matchPairsGuided( views[edges[e].second], guides[e], mo );
                        CHECK( re[e].size() == one.size() && !one.empty() );
                        for( size_t q = 0; q < one.size() && q < re[e].size(); q++ ) CHECK( same( re[e][q], one[q] ) );
                        total += re[e].size();
                    }
                    std::printf( "matchPairsGuidedGraph: model %d refit %d: %zu pairs over %zu edges\n", model, refit, total, re.size() );
                }
            }
            popsift::MatchOptions bad = mo;
            bad.ratio = -1.0f;
            std::vector<popsift::MatchGuide> all( edges.size(), popsift::MatchGuide::none() );
            all[1].kind = popsift::MatchGuide::Homography; all[1].m[0] = all[1].m[4] = all[1].m[8] = 1.0f; all[1].tol = 3.0f;
            CHECK( has( runtime_error_of( [&]{ FD::matchPairsGuidedGraph( views, edges, all, bad ); } ), "matchPairsGuidedGraph failed" ) );
        }
        for( auto* p : f ) delete p;
        for( auto* j : jobs ) delete j;
        ps.uninit();
    }
    std::printf( "%s\n", fails ? "FAILED" : "ALL OK" );
    return fails ? 1 : 0;
}
