// features_wrappers_san.cpp -- the host steps of popsift::FeaturesDev's matching, RANSAC and track wrappers, on the CPU.
//
// A stand-alone program (its own main), compiled together with popsift_amd/csrc/host/features.cpp under
// -fsanitize=address,undefined and linked against nothing else of the project: the 36 psx_* functions features.cpp reaches
// the device through are the stubs below.  "Device" memory is malloc memory with live counters, psx_quantize_desc and
// psx_desc_positions tag their output with the view they were given, and the match / RANSAC / tracks entry points write
// canned results computed from their arguments alone.  Every device-work call is logged; the program prints a transcript
// (per wrapper call: the preparation calls as a sorted set, the final call exactly, the returned fields) that
// tests/test_features_wrappers_cpu.py compares with tests/golden/features_wrappers_transcript.txt byte for byte.  The
// last part makes the n-th device-work call of five wrappers fail, for every n, and checks that the wrapper throws
// "<name> failed" and gives back every device buffer.  FEATURES_WRAPPERS_READS in the environment adds the number of
// psx_dev_read calls per wrapper call (not part of the transcript: it may only go down).
#include "popsift/features.h"
#include "popsift_hip.h"

#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <map>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

using namespace popsift;

#define CHECK( c ) do { if( !( c ) ) { printf( "HARNESS CHECK FAILED line %d: %s\n", __LINE__, #c ); fflush( stdout ); abort(); } } while( 0 )

namespace {

struct State
{
    long   live = 0;                               // device buffers that are allocated and not freed
    size_t live_bytes = 0;
    std::map<const void*, size_t>      sizes;      // every live device buffer
    std::map<const void*, std::string> tags;       // what psx_quantize_desc / psx_desc_positions wrote where
    std::map<const void*, int>         ori, ext, rev;   // a view's own arrays -> the view
    bool logging = false;
    std::vector<std::string> prep;                 // the preparation calls of the running wrapper call
    std::string              final_call;
    int work = 0;                                  // device-work calls of the running wrapper call
    int fail_n = 0;                                // > 0: that device-work call fails
    int reads = 0;
} S;

std::string fmt( const char* f, ... )
{
    char buf[4096];
    va_list ap;
    va_start( ap, f );
    vsnprintf( buf, sizeof(buf), f, ap );
    va_end( ap );
    return buf;
}

std::string tag( const void* p )
{
    if( p == nullptr ) return "null";
    auto t = S.tags.find( p );
    if( t != S.tags.end() ) return t->second;
    auto o = S.ori.find( p );
    if( o != S.ori.end() ) return fmt( "float(%d)", o->second );
    return "?";
}
std::string tags_of( const void* const* p, int n )
{
    if( p == nullptr ) return "null";
    std::string s = "[";
    for( int i = 0; i < n; i++ ) s += ( i ? "," : "" ) + tag( p[i] );
    return s + "]";
}
std::string ints( const int* p, int n )
{
    if( p == nullptr ) return "null";
    std::string s = "[";
    for( int i = 0; i < n; i++ ) s += fmt( i ? ",%d" : "%d", p[i] );
    return s + "]";
}
std::string edges_of( const psx_view_edge* p, int n )
{
    if( p == nullptr ) return "null";
    std::string s = "[";
    for( int i = 0; i < n; i++ ) s += fmt( "(%d,%d)", p[i].left, p[i].right );
    return s + "]";
}
std::string mopts( const psx_match_opts* o ) { return o ? fmt( "{ratio=%g,flags=%d}", o->ratio, o->flags ) : "null"; }
std::string ropts( const psx_ransac_opts* o ) { return o ? fmt( "{tol=%g,hyp=%d,seed=%u,flags=%d}", o->tol, o->hypotheses, o->seed, o->flags ) : "null"; }
std::string guide_of( const psx_guide& g )
{
    std::string s = fmt( "{kind=%d,m=[", g.kind );
    for( int j = 0; j < 9; j++ ) s += fmt( j ? ",%g" : "%g", g.m[j] );
    return s + fmt( "],tol=%g}", g.tol );
}
std::string guides_of( const psx_guide* g, int n )
{
    if( g == nullptr ) return "null";
    std::string s = "[";
    for( int i = 0; i < n; i++ ) s += guide_of( g[i] );
    return s + "]";
}
std::string records( const void* p, long n )
{
    if( p == nullptr ) return "null";
    const psx_match_pair_u8* r = (const psx_match_pair_u8*)p;
    std::string s = "[";
    for( long i = 0; i < n; i++ ) s += fmt( "(%d,%d,%d,%d)", r[i].left, r[i].right, r[i].d1, r[i].d2 );
    return s + "]";
}

// a preparation call: counted, may be the one that fails (with a code other than PSX_ERR_INVALID), logged
#define PREP( text ) do { if( S.logging ) { if( ++S.work == S.fail_n ) return PSX_ERR_HIP; S.prep.push_back( text ); } } while( 0 )
// the final call: counted, may be the one that fails (PSX_ERR_INVALID), logged exactly
#define FINAL( text ) do { if( S.logging ) { CHECK( S.final_call.empty() ); S.final_call = text; if( ++S.work == S.fail_n ) return PSX_ERR_INVALID; } } while( 0 )

void fill( psx_match_pair& p, int i, int j, int e )    { p.left = i; p.right = j; p.d1 = i + 0.25f * e; p.d2 = 2.0f * p.d1 + 1.0f; }
void fill( psx_match_pair_u8& p, int i, int j, int e ) { p.left = i; p.right = j; p.d1 = 10 * i + e; p.d2 = ( i % 2 ) ? INT32_MAX : 20 * i + e + 1; }

// the canned pair lists: left row i of list e pairs with right row (7 i + e) % r_len unless (i + e) % 3 == 0 (the
// cross-check drops the rows with i % 5 == 4 as well); an empty side gives an empty list
template<class P>
int canned_lists( int n, const int* l_lens, const int* r_lens, const psx_match_opts* opts, P* out, int capacity, int* counts, int* count )
{
    CHECK( opts != nullptr && count != nullptr && capacity >= 0 );
    const bool mutual = ( opts->flags & PSX_PAIRS_MUTUAL ) != 0;
    int total = 0;
    for( int e = 0; e < n; e++ ) {
        int c = 0;
        if( l_lens[e] > 0 && r_lens[e] > 0 )
            for( int i = 0; i < l_lens[e]; i++ ) {
                if( ( i + e ) % 3 == 0 || ( mutual && i % 5 == 4 ) ) continue;
                CHECK( out != nullptr && total < capacity );
                fill( out[total], i, ( 7 * i + e ) % r_lens[e], e );
                total++; c++;
            }
        if( counts ) counts[e] = c;
    }
    *count = total;
    return PSX_OK;
}

// the canned estimates: the records at the odd positions of each counted list are its inliers, the matrix says which
// model and which list
int canned_ransac( int model, const void* pairs, const int* counts, int n, psx_ransac_result* res, void* inliers, int capacity, int* count )
{
    CHECK( pairs != nullptr && res != nullptr && inliers != nullptr && count != nullptr );
    const psx_match_pair_u8* rec = (const psx_match_pair_u8*)pairs;
    psx_match_pair_u8* inl = (psx_match_pair_u8*)inliers;
    int at = 0, total = 0;
    for( int e = 0; e < n; e++ ) {
        memset( &res[e], 0, sizeof(res[e]) );
        res[e].best = -1;
        if( counts[e] <= 0 ) continue;
        for( int j = 0; j < 9; j++ ) res[e].m[j] = 100.0f * model + e + 0.5f * j;
        res[e].best = e + 1; res[e].sample_inliers = counts[e] / 2 + 1; res[e].refit_kept = e & 1;
        for( int q = 0; q < counts[e]; q++ )
            if( q % 2 == 1 ) { CHECK( total < capacity ); inl[total++] = rec[at + q]; res[e].inliers++; }
        at += counts[e];
    }
    *count = total;
    return PSX_OK;
}

long sum( const int* p, int n ) { long s = 0; for( int i = 0; i < n; i++ ) s += p[i]; return s; }

} // namespace

extern "C" {

int psx_dev_alloc( int device, size_t bytes, void** out )
{
    PREP( fmt( "alloc dev=%d bytes=%zu", device, bytes ) );
    void* p = malloc( bytes ? bytes : 1 );
    CHECK( p != nullptr && out != nullptr );
    S.sizes[p] = bytes; S.live++; S.live_bytes += bytes;
    *out = p;
    return PSX_OK;
}
int psx_dev_free( int, void* p )
{
    if( p == nullptr ) return PSX_OK;
    auto it = S.sizes.find( p );
    CHECK( it != S.sizes.end() );
    S.live--; S.live_bytes -= it->second;
    S.sizes.erase( it ); S.tags.erase( p );
    free( p );
    return PSX_OK;
}
int psx_dev_read( int, void* dst, const void* src, size_t bytes )
{
    S.reads++;
    if( bytes ) memcpy( dst, src, bytes );
    return PSX_OK;
}
int psx_host_alloc( size_t bytes, void** out )           { *out = malloc( bytes ? bytes : 1 ); return *out ? PSX_OK : PSX_ERR_NOMEM; }
int psx_host_alloc_near( int, size_t bytes, void** out ) { return psx_host_alloc( bytes, out ); }
int psx_host_free( void* p )                             { free( p ); return PSX_OK; }
int psx_device_pci( int, char* bus, int len )            { if( bus && len > 0 ) bus[0] = 0; return PSX_ERR_INVALID; }

int psx_quantize_desc( int device, const float* src, int n, unsigned char* dst )
{
    PREP( fmt( "quantize dev=%d %s n=%d", device, tag( src ).c_str(), n ) );
    CHECK( S.ori.count( src ) && S.sizes.count( dst ) && S.sizes[dst] >= (size_t)n * 128 );
    memset( dst, 0, (size_t)n * 128 );
    S.tags[dst] = fmt( "bytes(%d)", S.ori[src] );
    return PSX_OK;
}
int psx_desc_positions( int device, const psx_feature_dev* feats, const int* rev, int n, float* dst )
{
    PREP( fmt( "positions dev=%d view=%d n=%d", device, S.ext.count( feats ) ? S.ext[feats] : -1, n ) );
    CHECK( S.ext.count( feats ) && S.rev.count( rev ) && S.ext[feats] == S.rev[rev] );
    CHECK( S.sizes.count( dst ) && S.sizes[dst] >= (size_t)n * 2 * sizeof(float) );
    memset( dst, 0, (size_t)n * 2 * sizeof(float) );
    S.tags[dst] = fmt( "xy(%d)", S.ext[feats] );
    return PSX_OK;
}

// the print forms: row i's neighbours are (7 i) % r_len and (7 i + 1) % r_len, accepted when i is odd
int psx_match( int device, const float* l, int l_len, const float* r, int r_len, int* mm, float* dd )
{
    FINAL( fmt( "psx_match dev=%d %s l_len=%d %s r_len=%d", device, tag( l ).c_str(), l_len, tag( r ).c_str(), r_len ) );
    for( int i = 0; i < l_len; i++ ) {
        mm[3*i] = r_len > 0 ? ( 7 * i ) % r_len : 0; mm[3*i+1] = r_len > 0 ? ( 7 * i + 1 ) % r_len : 0; mm[3*i+2] = i & 1;
        if( dd ) { dd[2*i] = i + 0.5f; dd[2*i+1] = r_len > 1 ? 2.0f * i + 1.0f : INFINITY; }
    }
    return PSX_OK;
}
int psx_match_u8( int device, const unsigned char* l, int l_len, const unsigned char* r, int r_len, int* mm, int* dd )
{
    FINAL( fmt( "psx_match_u8 dev=%d %s l_len=%d %s r_len=%d", device, tag( l ).c_str(), l_len, tag( r ).c_str(), r_len ) );
    for( int i = 0; i < l_len; i++ ) {
        mm[3*i] = r_len > 0 ? ( 7 * i ) % r_len : 0; mm[3*i+1] = r_len > 0 ? ( 7 * i + 1 ) % r_len : 0; mm[3*i+2] = i & 1;
        if( dd ) { dd[2*i] = r_len > 0 ? 10 * i : INT32_MAX; dd[2*i+1] = r_len > 1 && i % 2 == 0 ? 20 * i + 1 : INT32_MAX; }
    }
    return PSX_OK;
}

// ---- one pair
int psx_match_pairs( int device, const float* l, int l_len, const float* r, int r_len, const psx_match_opts* opts, psx_match_pair* out, int capacity, int* count )
{
    FINAL( fmt( "psx_match_pairs dev=%d %s l_len=%d %s r_len=%d opts=%s capacity=%d", device, tag( l ).c_str(), l_len, tag( r ).c_str(), r_len,
                mopts( opts ).c_str(), capacity ) );
    return canned_lists( 1, &l_len, &r_len, opts, out, capacity, nullptr, count );
}
int psx_match_pairs_u8( int device, const unsigned char* l, int l_len, const unsigned char* r, int r_len, const psx_match_opts* opts, psx_match_pair_u8* out,
                        int capacity, int* count )
{
    FINAL( fmt( "psx_match_pairs_u8 dev=%d %s l_len=%d %s r_len=%d opts=%s capacity=%d", device, tag( l ).c_str(), l_len, tag( r ).c_str(), r_len,
                mopts( opts ).c_str(), capacity ) );
    return canned_lists( 1, &l_len, &r_len, opts, out, capacity, nullptr, count );
}
int psx_match_pairs_guided( int device, const float* l, const float* lxy, int l_len, const float* r, const float* rxy, int r_len, const psx_guide* g,
                            const psx_match_opts* opts, psx_match_pair* out, int capacity, int* count )
{
    FINAL( fmt( "psx_match_pairs_guided dev=%d %s %s l_len=%d %s %s r_len=%d guide=%s opts=%s capacity=%d", device, tag( l ).c_str(), tag( lxy ).c_str(),
                l_len, tag( r ).c_str(), tag( rxy ).c_str(), r_len, guides_of( g, 1 ).c_str(), mopts( opts ).c_str(), capacity ) );
    return canned_lists( 1, &l_len, &r_len, opts, out, capacity, nullptr, count );
}
int psx_match_pairs_guided_u8( int device, const unsigned char* l, const float* lxy, int l_len, const unsigned char* r, const float* rxy, int r_len,
                               const psx_guide* g, const psx_match_opts* opts, psx_match_pair_u8* out, int capacity, int* count )
{
    FINAL( fmt( "psx_match_pairs_guided_u8 dev=%d %s %s l_len=%d %s %s r_len=%d guide=%s opts=%s capacity=%d", device, tag( l ).c_str(),
                tag( lxy ).c_str(), l_len, tag( r ).c_str(), tag( rxy ).c_str(), r_len, guides_of( g, 1 ).c_str(), mopts( opts ).c_str(), capacity ) );
    return canned_lists( 1, &l_len, &r_len, opts, out, capacity, nullptr, count );
}

// ---- the star: list k is (left, rights[k]); a set under a guide of kind None is skipped
} // extern "C"
template<class D, class P>
int star( const char* name, int device, const D* l, const float* lxy, int l_len, const D* const* rs, const float* const* rxys, const int* r_lens, int n,
          const psx_guide* g, bool guided, const psx_match_opts* opts, P* out, int capacity, int* counts, int* count )
{
    std::string s = fmt( "%s dev=%d %s", name, device, tag( l ).c_str() );
    if( guided ) s += " " + tag( lxy );
    s += fmt( " l_len=%d rights=%s", l_len, tags_of( (const void* const*)rs, n ).c_str() );
    if( guided ) s += " right_xys=" + tags_of( (const void* const*)rxys, n );
    s += fmt( " r_lens=%s n_sets=%d", ints( r_lens, n ).c_str(), n );
    if( guided ) s += " guides=" + guides_of( g, n );
    s += fmt( " opts=%s capacity=%d", mopts( opts ).c_str(), capacity );
    FINAL( s );
    std::vector<int> ll( n ), rl( n );
    for( int k = 0; k < n; k++ ) { ll[k] = l_len; rl[k] = ( guided && g[k].kind == PSX_GUIDE_NONE ) ? 0 : r_lens[k]; }
    return canned_lists( n, ll.data(), rl.data(), opts, out, capacity, counts, count );
}
extern "C" {
int psx_match_pairs_many_u8( int device, const unsigned char* l, int l_len, const unsigned char* const* rs, const int* r_lens, int n,
                             const psx_match_opts* opts, psx_match_pair_u8* out, int capacity, int* counts, int* count )
{
    return star( "psx_match_pairs_many_u8", device, l, nullptr, l_len, rs, nullptr, r_lens, n, nullptr, false, opts, out, capacity, counts, count );
}
int psx_match_pairs_many( int device, const float* l, int l_len, const float* const* rs, const int* r_lens, int n, const psx_match_opts* opts,
                          psx_match_pair* out, int capacity, int* counts, int* count )
{
    return star( "psx_match_pairs_many", device, l, nullptr, l_len, rs, nullptr, r_lens, n, nullptr, false, opts, out, capacity, counts, count );
}
int psx_match_pairs_guided_many_u8( int device, const unsigned char* l, const float* lxy, int l_len, const unsigned char* const* rs,
                                    const float* const* rxys, const int* r_lens, int n, const psx_guide* g, const psx_match_opts* opts,
                                    psx_match_pair_u8* out, int capacity, int* counts, int* count )
{
    return star( "psx_match_pairs_guided_many_u8", device, l, lxy, l_len, rs, rxys, r_lens, n, g, true, opts, out, capacity, counts, count );
}
int psx_match_pairs_guided_many( int device, const float* l, const float* lxy, int l_len, const float* const* rs, const float* const* rxys,
                                 const int* r_lens, int n, const psx_guide* g, const psx_match_opts* opts, psx_match_pair* out, int capacity,
                                 int* counts, int* count )
{
    return star( "psx_match_pairs_guided_many", device, l, lxy, l_len, rs, rxys, r_lens, n, g, true, opts, out, capacity, counts, count );
}

// ---- the edge list: list e is (sets[left], sets[right])
} // extern "C"
template<class D, class P>
int graph( const char* name, int device, const D* const* sets, const float* const* xys, const int* lens, int n_sets, const psx_view_edge* edges, int n,
           const psx_guide* g, bool guided, const psx_match_opts* opts, P* out, int capacity, int* counts, int* count )
{
    std::string s = fmt( "%s dev=%d sets=%s", name, device, tags_of( (const void* const*)sets, n_sets ).c_str() );
    if( guided ) s += " xys=" + tags_of( (const void* const*)xys, n_sets );
    s += fmt( " lens=%s n_sets=%d edges=%s n_edges=%d", ints( lens, n_sets ).c_str(), n_sets, edges_of( edges, n ).c_str(), n );
    if( guided ) s += " guides=" + guides_of( g, n );
    s += fmt( " opts=%s capacity=%d", mopts( opts ).c_str(), capacity );
    FINAL( s );
    std::vector<int> ll( n ), rl( n );
    for( int e = 0; e < n; e++ ) {
        CHECK( edges[e].left >= 0 && edges[e].left < n_sets && edges[e].right >= 0 && edges[e].right < n_sets );
        const bool skip = guided && g[e].kind == PSX_GUIDE_NONE;
        ll[e] = skip ? 0 : lens[edges[e].left]; rl[e] = skip ? 0 : lens[edges[e].right];
    }
    return canned_lists( n, ll.data(), rl.data(), opts, out, capacity, counts, count );
}
extern "C" {
int psx_match_pairs_graph_u8( int device, const unsigned char* const* sets, const int* lens, int n_sets, const psx_view_edge* edges, int n,
                              const psx_match_opts* opts, psx_match_pair_u8* out, int capacity, int* counts, int* count )
{
    return graph( "psx_match_pairs_graph_u8", device, sets, nullptr, lens, n_sets, edges, n, nullptr, false, opts, out, capacity, counts, count );
}
int psx_match_pairs_graph( int device, const float* const* sets, const int* lens, int n_sets, const psx_view_edge* edges, int n,
                           const psx_match_opts* opts, psx_match_pair* out, int capacity, int* counts, int* count )
{
    return graph( "psx_match_pairs_graph", device, sets, nullptr, lens, n_sets, edges, n, nullptr, false, opts, out, capacity, counts, count );
}
int psx_match_pairs_guided_graph_u8( int device, const unsigned char* const* sets, const float* const* xys, const int* lens, int n_sets,
                                     const psx_view_edge* edges, int n, const psx_guide* g, const psx_match_opts* opts, psx_match_pair_u8* out,
                                     int capacity, int* counts, int* count )
{
    return graph( "psx_match_pairs_guided_graph_u8", device, sets, xys, lens, n_sets, edges, n, g, true, opts, out, capacity, counts, count );
}
int psx_match_pairs_guided_graph( int device, const float* const* sets, const float* const* xys, const int* lens, int n_sets,
                                  const psx_view_edge* edges, int n, const psx_guide* g, const psx_match_opts* opts, psx_match_pair* out, int capacity,
                                  int* counts, int* count )
{
    return graph( "psx_match_pairs_guided_graph", device, sets, xys, lens, n_sets, edges, n, g, true, opts, out, capacity, counts, count );
}

// ---- RANSAC: four models, three forms each
#define RANSAC_STUBS( model, name ) \
int psx_ransac_##name( int device, const void* pairs, int n, const float* lxy, int l_len, const float* rxy, int r_len, const psx_ransac_opts* opts, \
                       psx_ransac_result* res, void* inl, int capacity, int* count, float* models, int* hcounts ) \
{ \
    FINAL( fmt( "psx_ransac_" #name " dev=%d n=%d %s l_len=%d %s r_len=%d opts=%s capacity=%d models=%s counts=%s pairs=", device, n, tag( lxy ).c_str(), \
                l_len, tag( rxy ).c_str(), r_len, ropts( opts ).c_str(), capacity, models ? "host" : "null", hcounts ? "host" : "null" ) + records( pairs, n ) ); \
    return canned_ransac( model, pairs, &n, 1, res, inl, capacity, count ); \
} \
int psx_ransac_##name##_many( int device, const void* pairs, const int* counts, int n_sets, const float* lxy, int l_len, const float* const* rxys, \
                              const int* r_lens, const psx_ransac_opts* opts, psx_ransac_result* res, void* inl, int capacity, int* count, \
                              float* models, int* hcounts ) \
{ \
    FINAL( fmt( "psx_ransac_" #name "_many dev=%d set_counts=%s n_sets=%d %s l_len=%d right_xys=%s r_lens=%s opts=%s capacity=%d models=%s counts=%s pairs=", \
                device, ints( counts, n_sets ).c_str(), n_sets, tag( lxy ).c_str(), l_len, tags_of( (const void* const*)rxys, n_sets ).c_str(), \
                ints( r_lens, n_sets ).c_str(), ropts( opts ).c_str(), capacity, models ? "host" : "null", hcounts ? "host" : "null" ) \
           + records( pairs, sum( counts, n_sets ) ) ); \
    return canned_ransac( model, pairs, counts, n_sets, res, inl, capacity, count ); \
} \
int psx_ransac_##name##_graph( int device, const void* pairs, const int* counts, const psx_view_edge* edges, int n_edges, const float* const* xys, \
                               const int* lens, int n_sets, const psx_ransac_opts* opts, psx_ransac_result* res, void* inl, int capacity, int* count, \
                               float* models, int* hcounts ) \
{ \
    FINAL( fmt( "psx_ransac_" #name "_graph dev=%d edge_counts=%s edges=%s n_edges=%d xys=%s lens=%s n_sets=%d opts=%s capacity=%d models=%s counts=%s pairs=", \
                device, ints( counts, n_edges ).c_str(), edges_of( edges, n_edges ).c_str(), n_edges, tags_of( (const void* const*)xys, n_sets ).c_str(), \
                ints( lens, n_sets ).c_str(), n_sets, ropts( opts ).c_str(), capacity, models ? "host" : "null", hcounts ? "host" : "null" ) \
           + records( pairs, sum( counts, n_edges ) ) ); \
    return canned_ransac( model, pairs, counts, n_edges, res, inl, capacity, count ); \
}
RANSAC_STUBS( 0, homography )
RANSAC_STUBS( 1, fundamental )
RANSAC_STUBS( 2, affine )
RANSAC_STUBS( 3, similarity )

// ---- tracks: a fixed small answer (two tracks of two members)
int psx_tracks_graph( int device, const void* pairs, const int* counts, const psx_view_edge* edges, int n_edges, const int* lens, int n_sets,
                      const psx_track_opts* opts, int* labels, int* starts, int track_capacity, psx_track_member* members, int member_capacity,
                      psx_tracks_info* info )
{
    FINAL( fmt( "psx_tracks_graph dev=%d edge_counts=%s edges=%s n_edges=%d lens=%s n_sets=%d opts={min_views=%d,flags=%d} track_capacity=%d "
                "member_capacity=%d pairs=", device, ints( counts, n_edges ).c_str(), edges_of( edges, n_edges ).c_str(), n_edges,
                ints( lens, n_sets ).c_str(), n_sets, opts->min_views, opts->flags, track_capacity, member_capacity )
           + records( pairs, sum( counts, n_edges ) ) );
    CHECK( info != nullptr && track_capacity >= 2 && member_capacity >= 4 && member_capacity == sum( lens, n_sets ) );
    for( int i = 0; i < member_capacity; i++ ) labels[i] = i % 3 == 0 ? -1 : i % 2;
    starts[0] = 0; starts[1] = 2; starts[2] = 4;
    for( int i = 0; i < 4; i++ ) { members[i].view = 2 * ( i % 2 ); members[i].row = i + 1; }
    info->tracks = 2; info->members = 4; info->components = 3; info->conflicts = 1; info->too_few_views = 1; info->joined_records = (int)sum( counts, n_edges );
    return PSX_OK;
}

} // extern "C"

namespace {

// ---- the views: 5, 0, 7 and 3 descriptors over 3, 0, 4 and 2 features, and a null view that no edge names
FeaturesDev* V[5] = { nullptr, nullptr, nullptr, nullptr, nullptr };

FeaturesDev* make_view( int v, int n_desc, int n_ext )
{
    FeaturesDev* f = new FeaturesDev( n_ext, n_desc );
    for( int d = 0; d < n_desc; d++ ) f->getReverseMap()[d] = ( 3 * d + 1 ) % n_ext;     // not the identity
    S.ori[f->getDescriptors()] = v; S.ext[f->getFeatures()] = v; S.rev[f->getReverseMap()] = v;
    return f;
}

MatchGuide make_guide( MatchGuide::Kind kind, int seed )
{
    MatchGuide g;
    g.kind = kind;
    for( int j = 0; j < 9; j++ ) g.m[j] = seed + 0.125f * j;
    g.tol = 1.5f + seed;
    return g;
}

// a match list of n entries whose every field differs, descriptor indices inside [0, l_len) x [0, r_len)
std::vector<Match> make_list( int n, int l_len, int r_len, int salt )
{
    std::vector<Match> ms( n );
    for( int q = 0; q < n; q++ ) {
        Match& m = ms[q];
        m.left_descriptor = ( q + salt ) % ( l_len > 0 ? l_len : 1 ); m.right_descriptor = ( 2 * q + 1 ) % ( r_len > 0 ? r_len : 1 );
        m.left_feature = 100 * salt + q; m.right_feature = 200 * salt + q;
        m.distance = q + 0.5f; m.second_distance = q % 4 == 3 ? INFINITY : 3.0f * q + 1.0f;
    }
    return ms;
}

void show( const Match& m, const char* indent )
{
    printf( "%sL%d R%d l%d r%d d=%g d2=%g\n", indent, m.left_feature, m.right_feature, m.left_descriptor, m.right_descriptor, m.distance, m.second_distance );
}
void show( int ) { }
void show( const std::vector<Match>& ms ) { printf( " %zu matches\n", ms.size() ); for( const Match& m : ms ) show( m, "   " ); }
void show( const std::vector<std::vector<Match>>& ls )
{
    printf( " %zu lists\n", ls.size() );
    for( size_t k = 0; k < ls.size(); k++ ) { printf( "  list %zu: %zu matches\n", k, ls[k].size() ); for( const Match& m : ls[k] ) show( m, "   " ); }
}
void show( const HomographyEstimate& e )
{
    printf( " estimate kind=%d m=[", (int)e.guide.kind );
    for( int j = 0; j < 9; j++ ) printf( j ? ",%g" : "%g", e.guide.m[j] );
    printf( "] tol=%g best=%d sample_inliers=%d refit_kept=%d inliers=%zu\n", e.guide.tol, e.best, e.sample_inliers, (int)e.refit_kept, e.inliers.size() );
    for( const Match& m : e.inliers ) show( m, "   " );
}
void show( const std::vector<HomographyEstimate>& es ) { printf( " %zu estimates\n", es.size() ); for( const HomographyEstimate& e : es ) show( e ); }
void show( const Tracks& t )
{
    printf( " tracks n_tracks=%d n_members=%d components=%d conflicts=%d too_few_views=%d joined_records=%d\n", t.n_tracks, t.n_members, t.components,
            t.conflicts, t.too_few_views, t.joined_records );
    printf( "  starts=%s\n  labels=%s\n  view_offsets=%s\n  members=[", ints( t.starts.data(), (int)t.starts.size() ).c_str(),
            ints( t.labels.data(), (int)t.labels.size() ).c_str(), ints( t.view_offsets.data(), (int)t.view_offsets.size() ).c_str() );
    for( const TrackMember& m : t.members ) printf( "(%d,%d)", m.view, m.descriptor );
    printf( "]\n" );
}

// "<path>/features.cpp:<line>\n    <text>" -> "features.cpp:N <text>": the line moves with every edit
std::string message( const std::exception& e )
{
    std::string s = e.what();
    const size_t nl = s.find( '\n' );
    if( nl == std::string::npos ) return s;
    std::string head = s.substr( 0, nl );
    const size_t slash = head.rfind( '/' ), colon = head.rfind( ':' );
    if( colon == std::string::npos ) return s;
    head = head.substr( slash == std::string::npos ? 0 : slash + 1, colon - ( slash == std::string::npos ? 0 : slash + 1 ) );
    size_t at = nl + 1;
    while( at < s.size() && s[at] == ' ' ) at++;
    return head + ":N " + s.substr( at );
}

const bool show_reads = getenv( "FEATURES_WRAPPERS_READS" ) != nullptr;     // not part of the transcript: may only go down

template<class F>
void run( const std::string& label, F f )
{
    printf( "== %s\n", label.c_str() );
    S.prep.clear(); S.final_call.clear(); S.work = 0; S.reads = 0;
    const long live0 = S.live;
    const size_t bytes0 = S.live_bytes;
    S.logging = true;
    try {
        auto r = f();
        S.logging = false;
        std::sort( S.prep.begin(), S.prep.end() );
        for( const std::string& p : S.prep ) printf( " prep: %s\n", p.c_str() );
        printf( " final: %s\n", S.final_call.empty() ? "none" : S.final_call.c_str() );
        show( r );
    } catch( const std::runtime_error& e ) {
        S.logging = false;
        printf( " throws: %s\n", message( e ).c_str() );       // without the calls before it: their order among views is free
    }
    if( show_reads ) printf( " reads: %d\n", S.reads );
    CHECK( S.live == live0 && S.live_bytes == bytes0 );
}

// the n-th device-work call of f fails, for every n: f throws "<name> failed" and every device buffer comes back
template<class F>
void inject( const char* name, F f )
{
    S.prep.clear(); S.final_call.clear(); S.work = 0; S.fail_n = 0;
    S.logging = true; f(); S.logging = false;
    const int N = S.work;
    printf( "== inject %s: %d device-work calls\n", name, N );
    CHECK( N >= 3 );
    for( int n = 1; n <= N; n++ ) {
        const long live0 = S.live;
        const size_t bytes0 = S.live_bytes;
        S.prep.clear(); S.final_call.clear(); S.work = 0; S.fail_n = n;
        std::string msg;
        S.logging = true;
        try { f(); } catch( const std::runtime_error& e ) { msg = message( e ); }
        S.logging = false; S.fail_n = 0;
        CHECK( msg.find( std::string( name ) + " failed" ) != std::string::npos );
        CHECK( S.live == live0 && S.live_bytes == bytes0 );
        printf( " n=%d: %s\n", n, msg.c_str() );
    }
}

typedef std::vector<std::vector<Match>> Lists;
typedef std::vector<HomographyEstimate> Estimates;

} // namespace

int main()
{
    V[0] = make_view( 0, 5, 3 ); V[1] = make_view( 1, 0, 0 ); V[2] = make_view( 2, 7, 4 ); V[3] = make_view( 3, 3, 2 );
    const int LEN[4] = { 5, 0, 7, 3 };
    const std::vector<FeaturesDev*> views( V, V + 5 );
    const std::vector<FeaturesDev*> others = { V[2], V[1], V[3], V[2] };                  // the star: this = view 0
    const int OTHER[4] = { 2, 1, 3, 2 };
    const std::vector<std::pair<int,int>> edges = { {2,3}, {0,2}, {2,0}, {0,0}, {0,1}, {0,2} };   // unsorted, both orders, self, empty side, duplicate
    const MatchGuide H = make_guide( MatchGuide::Homography, 1 ), E = make_guide( MatchGuide::Epipolar, 2 );
    const std::vector<MatchGuide> star_guides = { H, E, MatchGuide::none(), E };          // view 3 is skipped
    const std::vector<MatchGuide> edge_guides = { H, MatchGuide::none(), E, H, E, make_guide( MatchGuide::Homography, 3 ) };
    MatchOptions fo, fm, bo, bm;                                                          // float / bytes, mutual off / on
    fm.mutual = true; fm.ratio = 0.7f; bo.bytes = true; bm.bytes = true; bm.mutual = true; bm.ratio = INFINITY;
    struct { const char* name; const MatchOptions* o; } F2[2] = { { "", &fo }, { " mutual", &fm } }, B2[2] = { { "", &bo }, { " mutual", &bm } };

    // ---- the print forms
    run( "match 0 2", [&]{ V[0]->match( V[2] ); return 0; } );
    run( "match 0 1", [&]{ V[0]->match( V[1] ); return 0; } );
    run( "match 1 0", [&]{ V[1]->match( V[0] ); return 0; } );
    run( "match null", [&]{ V[0]->match( nullptr ); return 0; } );
    run( "matchBytes 0 2", [&]{ V[0]->matchBytes( V[2] ); return 0; } );
    run( "matchBytes 2 3", [&]{ V[2]->matchBytes( V[3] ); return 0; } );
    run( "matchBytes 0 1", [&]{ V[0]->matchBytes( V[1] ); return 0; } );
    run( "matchBytes null", [&]{ V[0]->matchBytes( nullptr ); return 0; } );
    fflush( stdout );

    // ---- one pair
    for( int b = 0; b < 2; b++ )
        for( int m = 0; m < 2; m++ ) {
            const MatchOptions& o = *( b ? B2 : F2 )[m].o;
            const std::string sfx = std::string( b ? " bytes" : " float" ) + F2[m].name;
            run( "matchPairs 0 2" + sfx, [&]{ return V[0]->matchPairs( V[2], o ); } );
            run( "matchPairs 2 0" + sfx, [&]{ return V[2]->matchPairs( V[0], o ); } );
            run( "matchPairs 0 0" + sfx, [&]{ return V[0]->matchPairs( V[0], o ); } );
            run( "matchPairs 0 1" + sfx, [&]{ return V[0]->matchPairs( V[1], o ); } );
            run( "matchPairsGuided 0 2 H" + sfx, [&]{ return V[0]->matchPairsGuided( V[2], H, o ); } );
            run( "matchPairsGuided 2 3 E" + sfx, [&]{ return V[2]->matchPairsGuided( V[3], E, o ); } );
            run( "matchPairsGuided 1 0 H" + sfx, [&]{ return V[1]->matchPairsGuided( V[0], H, o ); } );
        }
    run( "matchPairs null", [&]{ return V[0]->matchPairs( nullptr, fo ); } );
    run( "matchPairsGuided null", [&]{ return V[0]->matchPairsGuided( nullptr, H, fo ); } );
    run( "matchPairsGuided kind None", [&]{ return V[0]->matchPairsGuided( V[2], MatchGuide::none(), bo ); } );
    { MatchGuide bad = H; bad.tol = -1.0f; run( "matchPairsGuided tol < 0, empty side", [&]{ return V[0]->matchPairsGuided( V[1], bad, fo ); } ); }
    { MatchGuide bad = E; bad.m[4] = NAN;  run( "matchPairsGuided NaN entry", [&]{ return V[0]->matchPairsGuided( V[2], bad, fo ); } ); }

    // ---- the star and the edge list, bytes and float, unguided and guided
    for( int m = 0; m < 2; m++ ) {
        const MatchOptions &b = *B2[m].o, &f = *F2[m].o;
        const std::string sfx = F2[m].name;
        run( "matchPairsMany" + sfx, [&]{ return V[0]->matchPairsMany( others, b ); } );
        run( "matchPairsManyFloat" + sfx, [&]{ return V[0]->matchPairsManyFloat( others, f ); } );
        run( "matchPairsGuidedMany" + sfx, [&]{ return V[0]->matchPairsGuidedMany( others, star_guides, b ); } );
        run( "matchPairsGuidedManyFloat" + sfx, [&]{ return V[0]->matchPairsGuidedManyFloat( others, star_guides, f ); } );
        run( "matchPairsGraph" + sfx, [&]{ return FeaturesDev::matchPairsGraph( views, edges, b ); } );
        run( "matchPairsGraphFloat" + sfx, [&]{ return FeaturesDev::matchPairsGraphFloat( views, edges, f ); } );
        run( "matchPairsGuidedGraph" + sfx, [&]{ return FeaturesDev::matchPairsGuidedGraph( views, edges, edge_guides, b ); } );
        run( "matchPairsGuidedGraphFloat" + sfx, [&]{ return FeaturesDev::matchPairsGuidedGraphFloat( views, edges, edge_guides, f ); } );
    }
    {   // a view that only a skipped edge and an edge with an empty side name is neither quantised nor gathered
        const std::vector<std::pair<int,int>> e3 = { {2,3}, {0,2}, {3,1} };
        const std::vector<MatchGuide> g3 = { MatchGuide::none(), H, E };
        run( "matchPairsGuidedGraph, view 3 unused", [&]{ return FeaturesDev::matchPairsGuidedGraph( views, e3, g3, bo ); } );
        run( "matchPairsGuidedGraphFloat, view 3 unused", [&]{ return FeaturesDev::matchPairsGuidedGraphFloat( views, e3, g3, fo ); } );
        const std::vector<std::pair<int,int>> e2 = { {0,2}, {3,1}, {1,3} };
        run( "matchPairsGraph, view 3 unused", [&]{ return FeaturesDev::matchPairsGraph( views, e2, bo ); } );
        run( "matchPairsGraphFloat, view 3 unused", [&]{ return FeaturesDev::matchPairsGraphFloat( views, e2, fo ); } );
    }
    {   // nothing to do: no device is touched
        const std::vector<FeaturesDev*> empties = { V[1], V[1] };
        const std::vector<MatchGuide> g2 = { H, E }, gn = { MatchGuide::none(), MatchGuide::none(), MatchGuide::none(), MatchGuide::none() };
        const std::vector<std::pair<int,int>> ee = { {0,1}, {1,2}, {1,1} }, none;
        const std::vector<MatchGuide> g3 = { H, E, H }, g0;
        run( "matchPairsMany, empty this", [&]{ return V[1]->matchPairsMany( others, bo ); } );
        run( "matchPairsMany, empty others", [&]{ return V[0]->matchPairsMany( empties, bo ); } );
        run( "matchPairsMany, no others", [&]{ return V[0]->matchPairsMany( std::vector<FeaturesDev*>(), bo ); } );
        run( "matchPairsManyFloat, empty this", [&]{ return V[1]->matchPairsManyFloat( others, fo ); } );
        run( "matchPairsManyFloat, empty others", [&]{ return V[0]->matchPairsManyFloat( empties, fo ); } );
        run( "matchPairsGuidedMany, empty this", [&]{ return V[1]->matchPairsGuidedMany( others, star_guides, bo ); } );
        run( "matchPairsGuidedMany, empty others", [&]{ return V[0]->matchPairsGuidedMany( empties, g2, bo ); } );
        run( "matchPairsGuidedMany, all skipped", [&]{ return V[0]->matchPairsGuidedMany( others, gn, bo ); } );
        run( "matchPairsGuidedManyFloat, empty this", [&]{ return V[1]->matchPairsGuidedManyFloat( others, star_guides, fo ); } );
        run( "matchPairsGuidedManyFloat, all skipped", [&]{ return V[0]->matchPairsGuidedManyFloat( others, gn, fo ); } );
        run( "matchPairsGraph, empty sides", [&]{ return FeaturesDev::matchPairsGraph( views, ee, bo ); } );
        run( "matchPairsGraph, no edge", [&]{ return FeaturesDev::matchPairsGraph( views, none, bo ); } );
        run( "matchPairsGraphFloat, empty sides", [&]{ return FeaturesDev::matchPairsGraphFloat( views, ee, fo ); } );
        run( "matchPairsGuidedGraph, empty sides", [&]{ return FeaturesDev::matchPairsGuidedGraph( views, ee, g3, bo ); } );
        run( "matchPairsGuidedGraph, no edge", [&]{ return FeaturesDev::matchPairsGuidedGraph( views, none, g0, bo ); } );
        run( "matchPairsGuidedGraphFloat, empty sides", [&]{ return FeaturesDev::matchPairsGuidedGraphFloat( views, ee, g3, fo ); } );
    }

    // ---- RANSAC: lists of 9, 1, 0 and 4 matches (the edge list: 9, 2, 0, 4, 1, 3), so the lists below min_pairs differ per model
    const int STAR_N[4] = { 9, 1, 0, 4 }, EDGE_N[6] = { 9, 2, 0, 4, 1, 3 };
    Lists star_lists( 4 ), edge_lists( 6 );
    for( int k = 0; k < 4; k++ ) star_lists[k] = make_list( STAR_N[k], LEN[0], LEN[OTHER[k]], k + 1 );
    for( int e = 0; e < 6; e++ ) edge_lists[e] = make_list( EDGE_N[e], LEN[edges[e].first], LEN[edges[e].second], e + 1 );
    RansacOptions ro; ro.tol = 1.25f; ro.hypotheses = 77; ro.seed = 5u; ro.refit = false;
    const RansacOptions rd;
    const char* MODEL[4] = { "Homography", "Fundamental", "Affine", "Similarity" };
    for( int model = 0; model < 4; model++ ) {
        const std::string nm = MODEL[model];
        auto one = [&]( FeaturesDev* l, FeaturesDev* r, const std::vector<Match>& ms, const RansacOptions& o ) {
            return model == 0 ? l->estimateHomography( r, ms, o ) : model == 1 ? l->estimateFundamental( r, ms, o )
                 : model == 2 ? l->estimateAffine( r, ms, o ) : l->estimateSimilarity( r, ms, o ); };
        auto many = [&]( FeaturesDev* l, const std::vector<FeaturesDev*>& os, const Lists& ls, const RansacOptions& o ) {
            return model == 0 ? l->estimateHomographyMany( os, ls, o ) : model == 1 ? l->estimateFundamentalMany( os, ls, o )
                 : model == 2 ? l->estimateAffineMany( os, ls, o ) : l->estimateSimilarityMany( os, ls, o ); };
        auto graph = [&]( const std::vector<FeaturesDev*>& vs, const std::vector<std::pair<int,int>>& es, const Lists& ls, const RansacOptions& o ) {
            return model == 0 ? FeaturesDev::estimateHomographyGraph( vs, es, ls, o ) : model == 1 ? FeaturesDev::estimateFundamentalGraph( vs, es, ls, o )
                 : model == 2 ? FeaturesDev::estimateAffineGraph( vs, es, ls, o ) : FeaturesDev::estimateSimilarityGraph( vs, es, ls, o ); };
        for( int k = 0; k < 4; k++ ) {
            const std::vector<Match> ms = make_list( STAR_N[k], LEN[0], LEN[2], k + 1 );
            run( "estimate" + nm + " 0 2, " + std::to_string( STAR_N[k] ) + " matches", [&]{ return one( V[0], V[2], ms, k % 2 ? rd : ro ); } );
        }
        run( "estimate" + nm + "Many", [&]{ return many( V[0], others, star_lists, ro ); } );
        run( "estimate" + nm + "Graph", [&]{ return graph( views, edges, edge_lists, rd ); } );
        if( model != 1 ) continue;
        // what each form refuses (one path for the four models)
        const std::vector<Match> nine = make_list( 9, LEN[0], 1, 7 );
        RansacOptions bad = ro; bad.hypotheses = 0;
        run( "estimate" + nm + " null", [&]{ return one( V[0], nullptr, nine, ro ); } );
        run( "estimate" + nm + " invalid options", [&]{ return one( V[0], V[2], nine, bad ); } );
        run( "estimate" + nm + " empty right", [&]{ return one( V[0], V[1], nine, ro ); } );
        run( "estimate" + nm + "Many invalid options", [&]{ return many( V[0], others, star_lists, bad ); } );
        run( "estimate" + nm + "Many 4 objects, 3 lists", [&]{ return many( V[0], others, Lists( 3 ), ro ); } );
        Lists on_empty = star_lists; on_empty[1] = nine;
        run( "estimate" + nm + "Many empty right", [&]{ return many( V[0], others, on_empty, ro ); } );
        run( "estimate" + nm + "Many empty this", [&]{ return many( V[1], others, star_lists, ro ); } );
        run( "estimate" + nm + "Many short lists", [&]{ return many( V[0], others, Lists( 4 ), ro ); } );
        run( "estimate" + nm + "Graph invalid options", [&]{ return graph( views, edges, edge_lists, bad ); } );
        run( "estimate" + nm + "Graph 6 edges, 5 lists", [&]{ return graph( views, edges, Lists( 5 ), ro ); } );
        Lists edge_on_empty = edge_lists; edge_on_empty[4] = nine;
        run( "estimate" + nm + "Graph empty side", [&]{ return graph( views, edges, edge_on_empty, ro ); } );
        run( "estimate" + nm + "Graph short lists", [&]{ return graph( views, edges, Lists( 6 ), ro ); } );
    }

    // ---- tracks
    TrackOptions to, tk; tk.min_views = 3; tk.keep_conflicts = true;
    run( "buildTracks", [&]{ return FeaturesDev::buildTracks( views, edges, edge_lists, to ); } );
    run( "buildTracks keep_conflicts", [&]{ return FeaturesDev::buildTracks( views, edges, edge_lists, tk ); } );
    { TrackOptions bad; bad.min_views = 1; run( "buildTracks min_views 1", [&]{ return FeaturesDev::buildTracks( views, edges, edge_lists, bad ); } ); }
    run( "buildTracks 6 edges, 5 lists", [&]{ return FeaturesDev::buildTracks( views, edges, Lists( 5 ), to ); } );

    // ---- what every batched form refuses about its views, edges, guides and options (one defect each)
    {
        const std::vector<FeaturesDev*> with_null = { V[2], nullptr, V[3] };
        const std::vector<MatchGuide> g3 = { H, E, H }, g5 = { H, E, H, E, H };
        std::vector<MatchGuide> bad_star = star_guides, bad_edge = edge_guides;
        bad_star[3].kind = (MatchGuide::Kind)3; bad_edge[2].tol = INFINITY;
        const std::vector<std::pair<int,int>> out_of_range = { {0,2}, {2,5} }, names_null = { {0,2}, {4,0} }, negative = { {-1,0} };
        const std::vector<MatchGuide> g2 = { H, E };
        run( "matchPairsMany null", [&]{ return V[0]->matchPairsMany( with_null, bo ); } );
        run( "matchPairsMany float options", [&]{ return V[0]->matchPairsMany( others, fo ); } );
        run( "matchPairsManyFloat null", [&]{ return V[0]->matchPairsManyFloat( with_null, fo ); } );
        run( "matchPairsManyFloat byte options", [&]{ return V[0]->matchPairsManyFloat( others, bo ); } );
        run( "matchPairsGuidedMany null", [&]{ return V[0]->matchPairsGuidedMany( with_null, g3, bo ); } );
        run( "matchPairsGuidedMany float options", [&]{ return V[0]->matchPairsGuidedMany( others, star_guides, fo ); } );
        run( "matchPairsGuidedMany 4 objects, 3 guides", [&]{ return V[0]->matchPairsGuidedMany( others, g3, bo ); } );
        run( "matchPairsGuidedMany invalid guide", [&]{ return V[0]->matchPairsGuidedMany( others, bad_star, bo ); } );
        run( "matchPairsGuidedManyFloat null", [&]{ return V[0]->matchPairsGuidedManyFloat( with_null, g3, fo ); } );
        run( "matchPairsGuidedManyFloat byte options", [&]{ return V[0]->matchPairsGuidedManyFloat( others, star_guides, bo ); } );
        run( "matchPairsGuidedManyFloat 4 objects, 3 guides", [&]{ return V[0]->matchPairsGuidedManyFloat( others, g3, fo ); } );
        run( "matchPairsGuidedManyFloat invalid guide", [&]{ return V[0]->matchPairsGuidedManyFloat( others, bad_star, fo ); } );
        run( "estimateHomographyMany null", [&]{ return V[0]->estimateHomographyMany( with_null, Lists( 3 ), ro ); } );
        run( "matchPairsGraph edge out of range", [&]{ return FeaturesDev::matchPairsGraph( views, out_of_range, bo ); } );
        run( "matchPairsGraph negative edge", [&]{ return FeaturesDev::matchPairsGraph( views, negative, bo ); } );
        run( "matchPairsGraph null named", [&]{ return FeaturesDev::matchPairsGraph( views, names_null, bo ); } );
        run( "matchPairsGraph float options", [&]{ return FeaturesDev::matchPairsGraph( views, edges, fo ); } );
        run( "matchPairsGraphFloat edge out of range", [&]{ return FeaturesDev::matchPairsGraphFloat( views, out_of_range, fo ); } );
        run( "matchPairsGraphFloat null named", [&]{ return FeaturesDev::matchPairsGraphFloat( views, names_null, fo ); } );
        run( "matchPairsGraphFloat byte options", [&]{ return FeaturesDev::matchPairsGraphFloat( views, edges, bo ); } );
        run( "matchPairsGuidedGraph edge out of range", [&]{ return FeaturesDev::matchPairsGuidedGraph( views, out_of_range, g2, bo ); } );
        run( "matchPairsGuidedGraph null named", [&]{ return FeaturesDev::matchPairsGuidedGraph( views, names_null, g2, bo ); } );
        run( "matchPairsGuidedGraph float options", [&]{ return FeaturesDev::matchPairsGuidedGraph( views, edges, edge_guides, fo ); } );
        run( "matchPairsGuidedGraph 6 edges, 5 guides", [&]{ return FeaturesDev::matchPairsGuidedGraph( views, edges, g5, bo ); } );
        run( "matchPairsGuidedGraph invalid guide", [&]{ return FeaturesDev::matchPairsGuidedGraph( views, edges, bad_edge, bo ); } );
        run( "matchPairsGuidedGraphFloat byte options", [&]{ return FeaturesDev::matchPairsGuidedGraphFloat( views, edges, edge_guides, bo ); } );
        run( "matchPairsGuidedGraphFloat 6 edges, 5 guides", [&]{ return FeaturesDev::matchPairsGuidedGraphFloat( views, edges, g5, fo ); } );
        run( "matchPairsGuidedGraphFloat invalid guide", [&]{ return FeaturesDev::matchPairsGuidedGraphFloat( views, edges, bad_edge, fo ); } );
        run( "estimateAffineGraph edge out of range", [&]{ return FeaturesDev::estimateAffineGraph( views, out_of_range, Lists( 2 ), ro ); } );
        run( "estimateAffineGraph null named", [&]{ return FeaturesDev::estimateAffineGraph( views, names_null, Lists( 2 ), ro ); } );
        run( "buildTracks edge out of range", [&]{ return FeaturesDev::buildTracks( views, out_of_range, Lists( 2 ), to ); } );
        run( "buildTracks null named", [&]{ return FeaturesDev::buildTracks( views, names_null, Lists( 2 ), to ); } );

        V[3]->setDevice( 1 );                                  // another device
        run( "matchPairs devices", [&]{ return V[2]->matchPairs( V[3], fo ); } );
        run( "matchPairsGuided devices", [&]{ return V[3]->matchPairsGuided( V[2], H, fo ); } );
        run( "estimateSimilarity devices", [&]{ return V[2]->estimateSimilarity( V[3], star_lists[0], ro ); } );
        run( "matchPairsMany devices", [&]{ return V[0]->matchPairsMany( others, bo ); } );
        run( "matchPairsManyFloat devices", [&]{ return V[0]->matchPairsManyFloat( others, fo ); } );
        run( "matchPairsGuidedMany devices", [&]{ return V[0]->matchPairsGuidedMany( others, star_guides, bo ); } );
        run( "matchPairsGuidedManyFloat devices", [&]{ return V[0]->matchPairsGuidedManyFloat( others, star_guides, fo ); } );
        run( "estimateFundamentalMany devices", [&]{ return V[0]->estimateFundamentalMany( others, star_lists, ro ); } );
        run( "matchPairsGraph devices", [&]{ return FeaturesDev::matchPairsGraph( views, edges, bo ); } );
        run( "matchPairsGraphFloat devices", [&]{ return FeaturesDev::matchPairsGraphFloat( views, edges, fo ); } );
        run( "matchPairsGuidedGraph devices", [&]{ return FeaturesDev::matchPairsGuidedGraph( views, edges, edge_guides, bo ); } );
        run( "estimateHomographyGraph devices", [&]{ return FeaturesDev::estimateHomographyGraph( views, edges, edge_lists, ro ); } );
        run( "buildTracks devices", [&]{ return FeaturesDev::buildTracks( views, edges, edge_lists, to ); } );
        V[3]->setDevice( 0 );
        for( int v = 0; v < 4; v++ ) V[v]->setDevice( 1 );     // all of them on device 1: that is the device of every call
        run( "matchPairsGuidedMany on device 1", [&]{ return V[0]->matchPairsGuidedMany( others, star_guides, bo ); } );
        run( "matchPairsGuidedGraph on device 1", [&]{ return FeaturesDev::matchPairsGuidedGraph( views, edges, edge_guides, bo ); } );
        run( "estimateHomographyGraph on device 1", [&]{ return FeaturesDev::estimateHomographyGraph( views, edges, edge_lists, ro ); } );
        run( "buildTracks on device 1", [&]{ return FeaturesDev::buildTracks( views, edges, edge_lists, to ); } );
        for( int v = 0; v < 4; v++ ) V[v]->setDevice( 0 );
    }

    // ---- failure injection
    inject( "FeaturesDev::matchPairsGuidedGraph", [&]{ FeaturesDev::matchPairsGuidedGraph( views, edges, edge_guides, bm ); } );
    inject( "FeaturesDev::matchPairsGuidedMany", [&]{ V[0]->matchPairsGuidedMany( others, star_guides, bm ); } );
    inject( "FeaturesDev::estimateHomographyGraph", [&]{ FeaturesDev::estimateHomographyGraph( views, edges, edge_lists, ro ); } );
    inject( "FeaturesDev::matchPairsGuided", [&]{ V[0]->matchPairsGuided( V[2], E, bm ); } );
    inject( "FeaturesDev::estimateAffineMany", [&]{ V[0]->estimateAffineMany( others, star_lists, ro ); } );

    for( int v = 0; v < 4; v++ ) delete V[v];
    CHECK( S.live == 0 && S.live_bytes == 0 );
    printf( "ALL OK\n" );
    return 0;
}
