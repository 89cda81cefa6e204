/* popsift::Vocabulary (popsift/shortlist.h) over psx_vocab_train_u8, psx_bow_u8 and psx_shortlist_views. */
#include <popsift/shortlist.h>
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

} // namespace popsift
