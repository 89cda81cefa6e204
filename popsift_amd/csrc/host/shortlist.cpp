/* popsift::Vocabulary and popsift::ViewDatabase (popsift/shortlist.h) over psx_vocab_train_u8, psx_bow_u8, psx_shortlist_views,
 * psx_bow_quantize_dev and psx_shortlist_query. */
#include <popsift/shortlist.h>
#include <popsift/vocabulary_file.h>
#include <popsift_hip.h>

#include <sstream>
#include <stdexcept>

namespace popsift {

namespace {

[[noreturn]] void fail( int line, const std::string& what )
{
    std::ostringstream o;
    o << "shortlist.cpp:" << line << "\n    " << what;
    throw std::runtime_error( o.str() );
}
#define SHORTLIST_FAIL( what ) fail( __LINE__, what )

// the byte form of every view's descriptors in device buffers that live as long as this object
class ByteViews
{
    int                               _device = 0;
    std::vector<void*>                _bufs;
public:
    std::vector<const unsigned char*> sets;
    std::vector<int>                  lens;

    ByteViews( const char* who, const std::vector<FeaturesDev*>& views )
    {
        bool first = true;
        for( FeaturesDev* v : views ) {
            if( v == nullptr || v->getDescriptorCount() <= 0 ) continue;
            if( first ) { _device = v->getDevice(); first = false; }
            else if( v->getDevice() != _device ) SHORTLIST_FAIL( std::string( who ) + ": views on different devices" );
        }
        for( FeaturesDev* v : views ) {
            const int len = v != nullptr && v->getDescriptorCount() > 0 ? v->getDescriptorCount() : 0;
            void* b = nullptr;
            if( len > 0 ) {
                if( psx_dev_alloc( _device, (size_t)len * 128, &b ) != PSX_OK ) { release(); SHORTLIST_FAIL( std::string( who ) + ": out of device memory" ); }
                _bufs.push_back( b );
                if( psx_quantize_desc( _device, (const float*)v->getDescriptors(), len, (unsigned char*)b ) != PSX_OK ) {
                    release();
                    SHORTLIST_FAIL( std::string( who ) + ": psx_quantize_desc failed" );
                }
            }
            sets.push_back( (const unsigned char*)b );
            lens.push_back( len );
        }
    }
    ~ByteViews( ) { release(); }
    ByteViews( const ByteViews& ) = delete;
    ByteViews& operator=( const ByteViews& ) = delete;
    void release( ) { for( void* b : _bufs ) psx_dev_free( _device, b ); _bufs.clear(); }
    int device( ) const { return _device; }
};

} // namespace

std::vector<std::pair<int,int>> Shortlist::pairs( ) const
{
    std::vector<std::pair<int,int>> out;
    out.reserve( edges.size() );
    for( const ViewEdge& e : edges ) out.emplace_back( e.left, e.right );
    return out;
}

void Vocabulary::train( const std::vector<FeaturesDev*>& views, int words, int iterations )
{
    const char* who = "Vocabulary::train";
    if( words < 2 || words > 65536 || iterations < 1 ) SHORTLIST_FAIL( std::string( who ) + ": invalid options" );
    ByteViews bv( who, views );
    long long rows = 0;
    for( int l : bv.lens ) rows += l;
    if( rows < words ) SHORTLIST_FAIL( std::string( who ) + ": fewer descriptors than words" );
    std::vector<unsigned char> out( (size_t)words * 128 );
    psx_vocab_opts o = { words, iterations };
    psx_vocab_info i;
    const int rc = psx_vocab_train_u8( bv.device(), bv.sets.data(), bv.lens.data(), (int)bv.lens.size(), &o, out.data(), &i );
    if( rc != PSX_OK ) { std::ostringstream m; m << who << ": psx_vocab_train_u8 failed (" << rc << ")"; SHORTLIST_FAIL( m.str() ); }
    _words.swap( out );
    _info.iterations = i.iterations; _info.changed = i.changed; _info.empty_words = i.empty_words; _info.inertia = i.inertia;
}

BagsOfWords Vocabulary::bagOfWords( const std::vector<FeaturesDev*>& views ) const
{
    const char* who = "Vocabulary::bagOfWords";
    if( _words.empty() ) SHORTLIST_FAIL( std::string( who ) + ": no vocabulary" );
    ByteViews bv( who, views );
    BagsOfWords b;
    b.views = (int)views.size();
    b.words = wordCount();
    b.counts.assign( (size_t)b.views * b.words, 0u );
    if( b.views == 0 ) return b;
    const int rc = psx_bow_u8( bv.device(), _words.data(), b.words, bv.sets.data(), bv.lens.data(), b.views, b.counts.data(), nullptr );
    if( rc != PSX_OK ) { std::ostringstream m; m << who << ": psx_bow_u8 failed (" << rc << ")"; SHORTLIST_FAIL( m.str() ); }
    return b;
}

Shortlist Vocabulary::shortlist( const BagsOfWords& bags, int k, bool mutual, int device )
{
    const char* who = "Vocabulary::shortlist";
    if( k < 1 || bags.views < 0 || bags.views > 4096 || bags.words < 1 || bags.counts.size() != (size_t)bags.views * bags.words )
        SHORTLIST_FAIL( std::string( who ) + ": invalid arguments" );
    Shortlist s;
    s.k = k;
    s.neighbours.assign( (size_t)bags.views * k, -1 );
    s.scores.assign( (size_t)bags.views * k, 0u );
    if( bags.views == 0 ) return s;
    const int per_view = k < bags.views - 1 ? k : bags.views - 1;
    std::vector<psx_view_edge> edges( (size_t)bags.views * per_view );                // no more pairs can exist
    psx_shortlist_opts o = { k, mutual ? PSX_SHORTLIST_MUTUAL : 0 };
    int count = 0;
    const int rc = psx_shortlist_views( device, bags.counts.data(), bags.views, bags.words, &o, s.neighbours.data(), s.scores.data(),
                                        edges.empty() ? nullptr : edges.data(), (int)edges.size(), &count );
    if( rc != PSX_OK ) { std::ostringstream m; m << who << ": psx_shortlist_views failed (" << rc << ")"; SHORTLIST_FAIL( m.str() ); }
    s.edges.resize( (size_t)count );
    for( int e = 0; e < count; e++ ) { s.edges[(size_t)e].left = edges[(size_t)e].left; s.edges[(size_t)e].right = edges[(size_t)e].right; }
    return s;
}

void Vocabulary::save( const std::string& path ) const
{
    if( _words.empty() ) SHORTLIST_FAIL( "Vocabulary::save: no vocabulary" );
    vocabulary_file::write( path, _words.data(), (unsigned)wordCount() );
}

Vocabulary Vocabulary::load( const std::string& path )
{
    Vocabulary v;
    v._words = vocabulary_file::read( path );
    return v;
}

void Vocabulary::assign( const unsigned char* bytes, int words )
{
    if( bytes == nullptr || words < 2 || words > 65536 ) SHORTLIST_FAIL( "Vocabulary::assign: invalid arguments" );
    _words.assign( bytes, bytes + (size_t)words * 128 );
    _info = VocabularyInfo();
}

std::vector<std::pair<int,int>> QueryResult::pairs( ) const
{
    std::vector<std::pair<int,int>> out;
    out.reserve( edges.size() );
    for( const ViewEdge& e : edges ) out.emplace_back( e.left, e.right );
    return out;
}

namespace {

// a device buffer that lives as long as this object
struct DevBuf
{
    int   device;
    void* p = nullptr;
    DevBuf( const char* who, int dev, size_t bytes ) : device( dev )
    {
        if( psx_dev_alloc( dev, bytes, &p ) != PSX_OK ) SHORTLIST_FAIL( std::string( who ) + ": out of device memory" );
    }
    ~DevBuf( ) { psx_dev_free( device, p ); }
    DevBuf( const DevBuf& ) = delete;
    DevBuf& operator=( const DevBuf& ) = delete;
};

void check( const char* who, const char* call, int rc )
{
    if( rc == PSX_OK ) return;
    std::ostringstream m;
    m << who << ": " << call << " failed (" << rc << ")";
    SHORTLIST_FAIL( m.str() );
}

} // namespace

ViewDatabase::ViewDatabase( const Vocabulary& vocabulary, int device, int capacity )
    : _voc( vocabulary ), _device( device ), _capacity( capacity )
{
    const char* who = "ViewDatabase";
    if( _voc.wordCount() < 1 ) SHORTLIST_FAIL( std::string( who ) + ": no vocabulary" );
    if( capacity < 1 || capacity > ( 1 << 20 ) ) SHORTLIST_FAIL( std::string( who ) + ": capacity outside [1, 1048576]" );
    _df.assign( (size_t)_voc.wordCount(), 0 );
    if( psx_dev_alloc( device, (size_t)capacity * _voc.wordCount() * 2, &_q ) != PSX_OK ) SHORTLIST_FAIL( std::string( who ) + ": out of device memory" );
}

ViewDatabase::~ViewDatabase( ) { if( _q ) psx_dev_free( _device, _q ); }

std::vector<int> ViewDatabase::weights( ) const
{
    std::vector<int> w( _df.size(), 0 );
    if( _size > 0 ) check( "ViewDatabase::weights", "psx_bow_weights", psx_bow_weights( _df.data(), (int)_df.size(), _size, w.data() ) );
    return w;
}

int ViewDatabase::add( const std::vector<FeaturesDev*>& views )
{
    const char* who = "ViewDatabase::add";
    const int n = (int)views.size(), W = _voc.wordCount();
    if( n > _capacity - _size ) SHORTLIST_FAIL( std::string( who ) + ": capacity exceeded" );
    if( n == 0 ) return _size;
    const BagsOfWords bags = _voc.bagOfWords( views );
    DevBuf hist( who, _device, bags.counts.size() * 4 );
    check( who, "psx_dev_write", psx_dev_write( _device, hist.p, bags.counts.data(), bags.counts.size() * 4 ) );
    std::vector<int> df = _df;                             // a failing call leaves the database as it was
    check( who, "psx_bow_quantize_dev", psx_bow_quantize_dev( _device, (const unsigned*)hist.p, n, W, (unsigned short*)_q + (size_t)_size * W, df.data() ) );
    _df.swap( df );
    const int first = _size;
    _size += n;
    return first;
}

QueryResult ViewDatabase::run( const void* d_query_q, int n, int k, unsigned min_score, int self_base, const int* limits, int edge_base ) const
{
    const char* who = "ViewDatabase::query";
    QueryResult r;
    r.k = k;
    r.edge_base = edge_base;
    r.neighbours.assign( (size_t)n * k, -1 );
    r.scores.assign( (size_t)n * k, 0u );
    if( n == 0 ) return r;
    const std::vector<int> w = weights();
    std::vector<psx_view_edge> edges( (size_t)n * ( k < _size ? k : _size ) );                        // no more can exist
    psx_query_opts o = { k, 0, self_base, edge_base, min_score, 0 };
    int count = 0;
    check( who, "psx_shortlist_query", psx_shortlist_query( _device, (const unsigned short*)_q, _size, (const unsigned short*)d_query_q, n,
                                                            _voc.wordCount(), w.data(), limits, &o, r.neighbours.data(), r.scores.data(),
                                                            edges.empty() ? nullptr : edges.data(), (int)edges.size(), &count ) );
    r.edges.resize( (size_t)count );
    for( int e = 0; e < count; e++ ) { r.edges[(size_t)e].left = edges[(size_t)e].left; r.edges[(size_t)e].right = edges[(size_t)e].right; }
    return r;
}

QueryResult ViewDatabase::query( const std::vector<FeaturesDev*>& views, int k, unsigned min_score ) const
{
    const char* who = "ViewDatabase::query";
    const int n = (int)views.size(), W = _voc.wordCount();
    if( k < 1 || n > 4096 || (long long)n * k > 0x7fffffffLL ) SHORTLIST_FAIL( std::string( who ) + ": invalid arguments" );
    if( n == 0 ) return run( nullptr, 0, k, min_score, -1, nullptr, _size );
    const BagsOfWords bags = _voc.bagOfWords( views );
    DevBuf hist( who, _device, bags.counts.size() * 4 ), q( who, _device, bags.counts.size() * 2 );
    check( who, "psx_dev_write", psx_dev_write( _device, hist.p, bags.counts.data(), bags.counts.size() * 4 ) );
    check( who, "psx_bow_quantize_dev", psx_bow_quantize_dev( _device, (const unsigned*)hist.p, n, W, (unsigned short*)q.p, nullptr ) );
    return run( q.p, n, k, min_score, -1, nullptr, _size );
}

QueryResult ViewDatabase::queryStored( int first, int count, int k, bool earlier_only ) const
{
    const char* who = "ViewDatabase::queryStored";
    if( k < 1 || first < 0 || count < 0 || count > 4096 || first > _size - count || (long long)count * k > 0x7fffffffLL )
        SHORTLIST_FAIL( std::string( who ) + ": invalid arguments" );
    std::vector<int> limits;
    if( earlier_only ) for( int i = 0; i < count; i++ ) limits.push_back( first + i );
    return run( (const unsigned short*)_q + (size_t)first * _voc.wordCount(), count, k, 0u, first, earlier_only && count > 0 ? limits.data() : nullptr, first );
}

} // namespace popsift
