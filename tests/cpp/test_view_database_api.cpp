// Test of popsift::ViewDatabase and the vocabulary file through the C++ host API.  Without a GPU: Vocabulary::assign / save /
// load with their errors, and what ViewDatabase refuses before a device is touched.
// With POPSIFT_TEST_EXPECT_GPU set (the -m gpu test): six views -- three shifts each of two synthetic frames -- go through
// PopSift in MatchingMode; a vocabulary is trained, saved and loaded again and gives the same bags; five views are stored in
// two steps, the sixth and an empty view arrive; add / query / queryStored equal psx_bow_quantize_ref, psx_bow_weights and
// psx_shortlist_query_ref on the same bags, the arriving view's first neighbour is a shift of its own frame, and the edges go
// into FeaturesDev::matchPairsGraph as they came out.  argv[1]: a directory to write the vocabulary file in.
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
typedef popsift::ViewDatabase DB;

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

// what the C calls give for these bags: database rows [0, n_db), query rows [q0, q0 + nq)
static void reference( const popsift::BagsOfWords& bags, int n_db, int q0, int nq, const psx_query_opts& o, const int* limits,
                       const popsift::QueryResult& got, const std::vector<int>& got_weights )
{
    const int W = bags.words;
    std::vector<unsigned short> q( (size_t)bags.views * W );
    std::vector<int> df( (size_t)W, 0 ), rest( (size_t)W, 0 ), weights( (size_t)W, 0 );
    CHECK( psx_bow_quantize_ref( bags.counts.data(), n_db, W, q.data(), df.data() ) == PSX_OK );
    CHECK( psx_bow_quantize_ref( bags.counts.data() + (size_t)n_db * W, bags.views - n_db, W, q.data() + (size_t)n_db * W, rest.data() ) == PSX_OK );
    CHECK( psx_bow_weights( df.data(), W, n_db, weights.data() ) == PSX_OK );
    CHECK( got_weights == weights );
    std::vector<int> nb( (size_t)nq * o.k, -7 );
    std::vector<unsigned> sc( (size_t)nq * o.k, 7u );
    std::vector<psx_view_edge> ed( (size_t)nq * o.k );
    int count = -1;
    CHECK( psx_shortlist_query_ref( q.data(), n_db, q.data() + (size_t)q0 * W, nq, W, weights.data(), limits, &o, nb.data(), sc.data(), ed.data(),
                                    (int)ed.size(), &count ) == PSX_OK );
    CHECK( got.k == o.k && got.edge_base == o.edge_base && got.neighbours == nb && got.scores == sc && (int)got.edges.size() == count );
    for( int e = 0; e < count && e < (int)got.edges.size(); e++ ) CHECK( got.edges[e].left == ed[e].left && got.edges[e].right == ed[e].right );
    CHECK( got.pairs().size() == got.edges.size() );
}

int main( int argc, char** argv )
{
    const bool gpu = std::getenv( "POPSIFT_TEST_EXPECT_GPU" ) != nullptr;
    const std::string dir = argc > 1 ? argv[1] : ".";
    {   // the vocabulary file and the argument errors, before any device call
        std::vector<unsigned char> bytes( 5 * 128 );
        for( size_t i = 0; i < bytes.size(); i++ ) bytes[i] = (unsigned char)( i * 13 + i / 128 );
        Voc v;
        CHECK( has( runtime_error_of( [&]{ v.save( dir + "/none.psxvocab" ); } ), "no vocabulary" ) );
        CHECK( has( runtime_error_of( [&]{ v.assign( nullptr, 5 ); } ), "invalid arguments" ) );
        CHECK( has( runtime_error_of( [&]{ v.assign( bytes.data(), 1 ); } ), "invalid arguments" ) );
        CHECK( has( runtime_error_of( [&]{ v.assign( bytes.data(), 65537 ); } ), "invalid arguments" ) );
        CHECK( v.wordCount() == 0 );
        v.assign( bytes.data(), 5 );
        CHECK( v.wordCount() == 5 && v.words() == bytes && v.info().iterations == 0 );
        v.save( dir + "/five.psxvocab" );
        const Voc back = Voc::load( dir + "/five.psxvocab" );
        CHECK( back.wordCount() == 5 && back.words() == bytes );
        CHECK( has( runtime_error_of( [&]{ Voc::load( dir + "/missing.psxvocab" ); } ), "cannot open" ) );
        CHECK( has( runtime_error_of( [&]{ v.save( dir + "/no/such/directory/v.psxvocab" ); } ), "cannot create" ) );
        std::FILE* f = std::fopen( ( dir + "/five.psxvocab" ).c_str(), "r+b" );
        CHECK( f != nullptr );
        if( f ) { std::fseek( f, 40, SEEK_SET ); std::fputc( bytes[20] ^ 0xff, f ); std::fclose( f ); }
        CHECK( has( runtime_error_of( [&]{ Voc::load( dir + "/five.psxvocab" ); } ), "checksum" ) );
        Voc none;
        CHECK( has( runtime_error_of( [&]{ DB d( none, 0, 8 ); } ), "no vocabulary" ) );
        CHECK( has( runtime_error_of( [&]{ DB d( v, 0, 0 ); } ), "capacity outside" ) );
        CHECK( has( runtime_error_of( [&]{ DB d( v, 0, ( 1 << 20 ) + 1 ); } ), "capacity outside" ) );
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
            Voc trained;
            trained.train( f, 64, 6 );
            trained.save( dir + "/trained.psxvocab" );
            const Voc voc = Voc::load( dir + "/trained.psxvocab" );
            CHECK( voc.words() == trained.words() );
            // stored: views 0 .. 4; arriving: view 5 (a shift of frame 1, as the stored views 3 and 4 are) and an empty view
            std::vector<FD*> all = f;
            all.push_back( &empty );
            const popsift::BagsOfWords bags = voc.bagOfWords( all );
            CHECK( bags.counts == trained.bagOfWords( all ).counts );
            DB db( voc, 0, 6 );
            CHECK( db.size() == 0 && db.capacity() == 6 && db.weights() == std::vector<int>( 64, 0 ) );
            CHECK( db.add( { f[0], f[1], f[2], f[3] } ) == 0 && db.size() == 4 );
            CHECK( db.add( { } ) == 4 && db.size() == 4 );
            CHECK( db.add( { f[4] } ) == 4 && db.size() == 5 );
            CHECK( has( runtime_error_of( [&]{ db.add( { f[5], &empty } ); } ), "capacity exceeded" ) && db.size() == 5 );
            const std::vector<int> weights = db.weights();
            {
                const popsift::QueryResult r = db.query( { f[5], &empty }, 2 );
                const psx_query_opts o = { 2, 0, -1, 5, 0u, 0 };
                reference( bags, 5, 5, 2, o, nullptr, r, weights );
                CHECK( r.neighbours[0] == 3 || r.neighbours[0] == 4 );
                CHECK( r.neighbours[2] == -1 && r.neighbours[3] == -1 );                    // the empty view lists nobody
                CHECK( r.edges.size() == 2 && r.edges[0].left == 5 && r.edges[1].left == 5 );
                std::printf( "view database: the arriving view lists %d (%u) and %d (%u)\n", r.neighbours[0], r.scores[0], r.neighbours[1], r.scores[1] );
                const unsigned between = ( r.scores[0] + r.scores[1] ) / 2 + 1;             // keeps the first alone, when the two differ
                const popsift::QueryResult cut = db.query( { f[5], &empty }, 2, between );
                const psx_query_opts oc = { 2, 0, -1, 5, between, 0 };
                reference( bags, 5, 5, 2, oc, nullptr, cut, weights );
                CHECK( r.scores[0] == r.scores[1] || cut.edges.size() == 1 );
                CHECK( db.query( { }, 3 ).edges.empty() );
                // the fifth call: the stored views with the arriving ones behind them
                popsift::MatchOptions mo;
                mo.mutual = true;
                mo.bytes = true;
                const std::vector<std::vector<popsift::Match>> lists = FD::matchPairsGraph( all, r.pairs(), mo );
                CHECK( lists.size() == r.edges.size() );
                size_t matches = 0;
                for( const auto& l : lists ) matches += l.size();
                CHECK( matches > 0 );
            }
            {
                const popsift::QueryResult r = db.queryStored( 0, 5, 2, false );
                const psx_query_opts o = { 2, 0, 0, 0, 0u, 0 };
                reference( bags, 5, 0, 5, o, nullptr, r, weights );
                for( int v = 0; v < 5; v++ ) CHECK( r.neighbours[2 * v] >= 0 && r.neighbours[2 * v] / 3 == v / 3 );    // a shift of its own frame first
            }
            {
                const popsift::QueryResult r = db.queryStored( 1, 4, 3, true );
                const psx_query_opts o = { 3, 0, 1, 1, 0u, 0 };
                const int limits[4] = { 1, 2, 3, 4 };
                reference( bags, 5, 1, 4, o, limits, r, weights );
                for( const popsift::ViewEdge& e : r.edges ) CHECK( e.right < e.left );
            }
            CHECK( has( runtime_error_of( [&]{ db.queryStored( 3, 3, 2, false ); } ), "invalid arguments" ) );
            CHECK( has( runtime_error_of( [&]{ db.query( { f[5] }, 0 ); } ), "invalid arguments" ) );
        }
        for( auto* p : f ) delete p;
        for( auto* j : jobs ) delete j;
        ps.uninit();
    }
    std::printf( "%s\n", fails ? "FAILED" : "ALL OK" );
    return fails ? 1 : 0;
}
