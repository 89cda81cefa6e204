// Test of popsift::Vocabulary through the C++ host API: its argument errors and empty forms, all before a device is touched
// (this part runs without a GPU), and Vocabulary::shortlist's host reference.
// With POPSIFT_TEST_EXPECT_GPU set (the -m gpu test): six views -- three shifts each of two synthetic frames -- go through
// PopSift in MatchingMode; a vocabulary is trained on them, every view's bag holds one count per descriptor, the shortlist
// equals psx_shortlist_views_ref of the bags, every view lists the two other shifts of its own frame, and the edge list goes
// into FeaturesDev::matchPairsGraph as it came out.
#include <popsift/popsift.h>
#include <popsift/features.h>
#include <popsift/shortlist.h>
#include <popsift/sift_conf.h>
#include <popsift_hip.h>

#include <algorithm>
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

typedef popsift::FeaturesDev FD;
typedef popsift::Vocabulary Voc;

static bool has( const std::string& s, const char* what ) { return s.find( what ) != std::string::npos; }

static std::vector<unsigned char> frame( int w, int h, unsigned seed )
{
    std::vector<unsigned char> img( (size_t)w * h );
    unsigned s = seed;
    const int cw = w / 8 + 2;
    std::vector<unsigned char> coarse( (size_t)cw * ( h / 8 + 2 ) );
    for( auto& c : coarse ) { s = s * 1664525u + 1013904223u; c = (unsigned char)( s >> 24 ); }
    for( int y = 0; y < h; y++ ) for( int x = 0; x < w; x++ ) {
        const int v = ( 3 * coarse[(size_t)( y / 8 ) * cw + x / 8] + coarse[(size_t)( y / 5 % ( h / 8 ) ) * cw + ( x / 3 ) % ( w / 8 )] ) / 4;
        img[(size_t)y * w + x] = (unsigned char)v;
    }
    return img;
}

int main()
{
    const bool gpu = std::getenv( "POPSIFT_TEST_EXPECT_GPU" ) != nullptr;
    {   // argument errors, in the file:line + message format, before any device call
        FD a, b, c;
        Voc v;
        const std::string e0 = runtime_error_of( [&]{ v.train( { &a, &b }, 1, 3 ); } );
        CHECK( has( e0, "shortlist.cpp:" ) && has( e0, "Vocabulary::train" ) && has( e0, "invalid options" ) );
        CHECK( has( runtime_error_of( [&]{ v.train( { &a, &b }, 65537, 3 ); } ), "invalid options" ) );
        CHECK( has( runtime_error_of( [&]{ v.train( { &a, &b }, 4, 0 ); } ), "invalid options" ) );
        CHECK( has( runtime_error_of( [&]{ v.train( { &a, nullptr, &b }, 4, 3 ); } ), "fewer descriptors than words" ) );
        CHECK( v.wordCount() == 0 && v.info().iterations == 0 );
        CHECK( has( runtime_error_of( [&]{ v.bagOfWords( { &a } ); } ), "no vocabulary" ) );
        popsift::BagsOfWords bags;
        bags.views = 3; bags.words = 2;
        bags.counts = { 1, 1, 1, 1, 2, 0 };
        CHECK( has( runtime_error_of( [&]{ Voc::shortlist( bags, 0 ); } ), "invalid arguments" ) );
        popsift::BagsOfWords wrong = bags;
        wrong.counts.pop_back();
        CHECK( has( runtime_error_of( [&]{ Voc::shortlist( wrong, 2 ); } ), "invalid arguments" ) );
        wrong.views = 4097;
        CHECK( has( runtime_error_of( [&]{ Voc::shortlist( wrong, 2 ); } ), "invalid arguments" ) );
        popsift::BagsOfWords none;
        none.words = 2;
        const popsift::Shortlist s0 = Voc::shortlist( none, 3 );
        CHECK( s0.k == 3 && s0.edges.empty() && s0.neighbours.empty() && s0.pairs().empty() );
    }
    if( gpu ) {
        const int w = 320, h = 240;
        popsift::Config cfg;
        cfg.setOctaves( 3 );
        cfg.setNormalizationMultiplier( 9 );              // descriptors on the byte scale: the byte form keeps their structure
        PopSift ps( cfg, popsift::Config::MatchingMode, PopSift::ByteImages );
        const int shifts[3] = { 0, 3, 5 };
        std::vector<SiftJob*> jobs;
        std::vector<FD*> f;
        for( int g = 0; g < 2; g++ ) {
            const std::vector<unsigned char> img = frame( w, h, g == 0 ? 4711u : 1234567u );
            for( int k = 0; k < 3; k++ ) {
                std::vector<unsigned char> v( img.size() );
                for( int y = 0; y < h; y++ ) for( int x = 0; x < w; x++ ) v[(size_t)y * w + x] = img[(size_t)y * w + ( x + w - shifts[k] ) % w];
                jobs.push_back( ps.enqueue( w, h, v.data() ) );
                f.push_back( jobs.back()->getDev() );
                CHECK( f.back() != nullptr );
            }
        }
        if( std::find( f.begin(), f.end(), nullptr ) == f.end() ) {
            FD empty;
            std::vector<FD*> views = f;
            views.push_back( &empty );
            views.push_back( nullptr );
            const int N = (int)views.size();
            Voc voc;
            voc.train( views, 64, 6 );
            CHECK( voc.wordCount() == 64 && voc.words().size() == 64 * 128 );
            CHECK( voc.info().iterations >= 1 && voc.info().iterations <= 6 && voc.info().inertia > 0 );
            const popsift::BagsOfWords bags = voc.bagOfWords( views );
            CHECK( bags.views == N && bags.words == 64 && bags.counts.size() == (size_t)N * 64 );
            for( int v = 0; v < N; v++ ) {
                long long n = 0;
                for( int q = 0; q < 64; q++ ) n += bags.counts[(size_t)v * 64 + q];
                CHECK( n == ( views[v] ? views[v]->getDescriptorCount() : 0 ) );
            }
            Voc again;                                     // two trainings: the same bytes
            again.train( views, 64, 6 );
            CHECK( again.words() == voc.words() && again.info().inertia == voc.info().inertia );
            for( int mutual = 0; mutual < 2; mutual++ ) {
                const popsift::Shortlist s = Voc::shortlist( bags, 2, mutual != 0 );
                std::vector<int> nb( (size_t)N * 2, -7 );
                std::vector<unsigned> sc( (size_t)N * 2, 7u );
                std::vector<psx_view_edge> ed( (size_t)N * 2 );
                psx_shortlist_opts o = { 2, mutual ? PSX_SHORTLIST_MUTUAL : 0 };
                int count = -1;
                CHECK( psx_shortlist_views_ref( bags.counts.data(), N, 64, &o, nb.data(), sc.data(), ed.data(), (int)ed.size(), &count ) == PSX_OK );
                CHECK( s.neighbours == nb && s.scores == sc && (int)s.edges.size() == count );
                for( int e = 0; e < count && e < (int)s.edges.size(); e++ ) CHECK( s.edges[e].left == ed[e].left && s.edges[e].right == ed[e].right );
                for( int v = 0; v < 6; v++ ) {             // the two other shifts of the view's own frame
                    std::vector<int> got( s.neighbours.begin() + 2 * v, s.neighbours.begin() + 2 * v + 2 ), want;
                    for( int m = v / 3 * 3; m < v / 3 * 3 + 3; m++ ) if( m != v ) want.push_back( m );
                    std::sort( got.begin(), got.end() );
                    CHECK( got == want );
                }
                CHECK( s.neighbours[12] == -1 && s.neighbours[14] == -1 );        // the empty and the null view list nobody
                CHECK( s.edges.size() == 6 );
                std::printf( "shortlist: mutual %d: %d edges over %d views, %d iterations, %d empty words\n", mutual, (int)s.edges.size(), N,
                             voc.info().iterations, voc.info().empty_words );
                popsift::MatchOptions mo;
                mo.mutual = true;
                mo.bytes = true;
                const std::vector<std::vector<popsift::Match>> lists = FD::matchPairsGraph( views, s.pairs(), mo );
                CHECK( lists.size() == s.edges.size() );
                size_t matches = 0;
                for( const auto& l : lists ) matches += l.size();
                CHECK( matches > 0 );
            }
        }
        for( auto* p : f ) delete p;
        for( auto* j : jobs ) delete j;
        ps.uninit();
    }
    std::printf( "%s\n", fails ? "FAILED" : "ALL OK" );
    return fails ? 1 : 0;
}
