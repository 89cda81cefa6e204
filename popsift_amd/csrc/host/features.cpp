// features.cpp -- FeaturesHost / FeaturesDev / Feature::print
// (reference behaviour: features.cu:27-128, 306-330)
#include <cstdio>
#include "popsift/features.h"
#include "host_pool.h"
#include "popsift/sift_extremum.h"

#include "popsift_hip.h"
#include <cstddef>

#include <algorithm>
#include <cerrno>
#include <map>
#include <mutex>
#include <thread>
#include <string>
#include <unordered_map>
#include <cstring>
#include <cctype>
#include <cstdint>
#include <sched.h>
#include <utility>
#include <vector>
#include <cmath>
#include <cstdlib>
#include <iomanip>
#include <sstream>
#include <stdexcept>
#include <unistd.h>

namespace popsift {

namespace {
[[noreturn]] void fatal( const char* file, int line, const std::string& msg )
{
    std::ostringstream o;
    o << file << ":" << line << std::endl << "    " << msg;
    throw std::runtime_error( o.str() );
}
void* page_alloc( size_t bytes )
{
    void* p = nullptr;
    const size_t page = (size_t)sysconf( _SC_PAGESIZE );
    const int err = posix_memalign( &p, page, bytes ? bytes : page );
    if( err != 0 ) { errno = err; return nullptr; }
    return p;
}
} // namespace

FeaturesBase::FeaturesBase( ) : _num_ext( 0 ), _num_ori( 0 ) { }
FeaturesBase::~FeaturesBase( ) = default;

// ---- buffer pools (host_pool.h) -------------------------------------------------------------------
namespace pool {
namespace {
const int MAX_POOLS = 33;                       // devices 0..31, and one pool for "no device named"

// pinned bytes a pool may keep on its free list (POPSIFT_POOL_FREE_MB, default 2048): the list is bounded by BYTES,
// sized for `jobs outstanding x (image + result)` of a replica with head-room, not by a buffer count -- a count of 32
// made a replica with 24 jobs outstanding (~40 live buffers) hipHostFree / hipHostMalloc its surplus on every
// drain / refill burst
size_t free_limit()
{
    static const size_t lim = []{ const char* e = getenv( "POPSIFT_POOL_FREE_MB" ); const long v = e ? atol( e ) : 2048; return (size_t)( v < 0 ? 0 : v ) << 20; }();
    return lim;
}

// "0-3,8,10-11\n" -> the listed CPUs that the process may run on.  No strtok: several workers, the pool's helper threads
// and the caller of enqueue() parse at the same moment during warm-up, and strtok keeps process-global state.
int parse_cpulist( const char* s, const cpu_set_t& allowed, cpu_set_t* want )
{
    CPU_ZERO( want );
    int n = 0;
    while( *s != 0 ) {
        while( *s == ',' || *s == '\n' || *s == ' ' ) s++;
        if( *s == 0 ) break;
        char* end = nullptr;
        long a = strtol( s, &end, 10 );
        if( end == s ) { while( *s != 0 && *s != ',' ) s++; continue; }     // not a number: skip the token
        long b = a;
        s = end;
        if( *s == '-' ) { b = strtol( s + 1, &end, 10 ); if( end == s + 1 ) b = a; s = end; }
        while( *s != 0 && *s != ',' ) s++;
        for( long c = a < 0 ? 0 : a; c <= b && c < CPU_SETSIZE; c++ )
            if( CPU_ISSET( (int)c, &allowed ) ) { CPU_SET( (int)c, want ); n++; }
    }
    return n;
}

// CPUs local to each device's PCIe root, read and parsed ONCE per device (sysfs does not change under us)
struct DeviceCpus { std::once_flag once; bool valid = false; cpu_set_t set; };
DeviceCpus& device_cpus( int device )
{
    static DeviceCpus* tab = new DeviceCpus[MAX_POOLS];
    DeviceCpus& d = tab[ ( device >= 0 && device < MAX_POOLS - 1 ) ? device : MAX_POOLS - 1 ];
    if( device < 0 || device >= MAX_POOLS - 1 ) return d;           // never valid
    std::call_once( d.once, [&d, device]{
        const char* e = getenv( "POPSIFT_NUMA_PIN" );
        if( e != nullptr && e[0] == '0' ) return;
        char bus[64];
        if( psx_device_pci( device, bus, sizeof(bus) ) != PSX_OK || bus[0] == 0 ) return;
        for( char* c = bus; *c; c++ ) *c = (char)tolower( *c );
        FILE* f = fopen( ( std::string( "/sys/bus/pci/devices/" ) + bus + "/local_cpulist" ).c_str(), "r" );
        if( f == nullptr ) return;
        char line[4096] = { 0 };
        const bool got = fgets( line, sizeof(line), f ) != nullptr;
        fclose( f );
        // the PROCESS's mask (its main thread's: what a launcher such as taskset / numactl / bench.py's pinning set), not the
        // calling thread's: the first caller may be a worker that is already bound to another device's socket, and its narrow
        // mask would truncate -- or empty -- this device's set for the rest of the process
        cpu_set_t allowed;
        if( !got || sched_getaffinity( getpid(), sizeof(allowed), &allowed ) != 0 ) return;
        d.valid = parse_cpulist( line, allowed, &d.set ) > 0;
    } );
    return d;
}
bool multi_node_host() { static const bool m = access( "/sys/devices/system/node/node1", F_OK ) == 0; return m; }

void forget_pinned( void* p );      // drops the buffer from the pointer -> device registry (it is about to be freed)

struct Pool
{
    std::mutex                            m;
    std::multimap<size_t, void*>          free_list;        // by capacity: the smallest adequate buffer in O(log n)
    const bool                            pinned;
    const int                             device;          // -1: none
    size_t                                in_use = 0;      // bytes handed out
    size_t                                free_bytes = 0;  // bytes on the free list
    Stats                                 st;
    Pool( bool p, int d ) : pinned( p ), device( d ) { }

    // Where the pages of a pinned buffer land: on the NUMA node the HIP runtime picks for the calling thread -- by its CPU
    // affinity or by its current device, depending on the runtime.  The caller of enqueue() runs anywhere, so on a
    // multi-socket host a pool miss allocates from a short-lived helper thread that is bound to the CPUs of the device's
    // PCIe root AND has made the device current (psx_host_alloc_near): socket-1 GPUs then DMA to socket-1 memory under
    // either rule.  Only pool misses pay for it (warm-up).
    void* alloc_pinned( size_t c )
    {
        void* p = nullptr;
        DeviceCpus& dc = device_cpus( device );
        // single-node host (or CPUs unknown): placement does not matter, and the CALLER's current device must not change
        if( !multi_node_host() || !dc.valid ) { if( psx_host_alloc( c, &p ) != PSX_OK ) return nullptr; return p; }
        const int dev = device;
        const cpu_set_t* set = &dc.set;
        std::thread t( [&p, c, dev, set]{ (void)sched_setaffinity( 0, sizeof(cpu_set_t), set ); if( psx_host_alloc_near( dev, c, &p ) != PSX_OK ) p = nullptr; } );
        t.join();
        return p;
    }

    void* get( size_t bytes, size_t* cap )
    {
        if( bytes == 0 ) bytes = 1;
        {
            std::lock_guard<std::mutex> g( m );
            auto it = free_list.lower_bound( bytes );
            if( it != free_list.end() && it->first <= 4 * bytes + ( 4u << 20 ) ) {
                void* p = it->second; *cap = it->first;
                free_list.erase( it );
                in_use += *cap; free_bytes -= *cap; st.hits++;
                return p;
            }
        }
        const size_t mb = (size_t)1 << 20;
        const size_t c = ( ( bytes + bytes / 4 + mb - 1 ) / mb ) * mb;       // 25 % slack, whole megabytes
        void* p = nullptr;
        if( pinned ) { p = alloc_pinned( c ); if( p == nullptr ) return nullptr; }
        else         { if( posix_memalign( &p, 4096, c ) != 0 ) return nullptr; }
        *cap = c;
        { std::lock_guard<std::mutex> g( m ); in_use += c; st.allocs++; }
        return p;
    }
    void put( void* p, size_t cap )
    {
        if( p == nullptr ) return;
        {
            std::lock_guard<std::mutex> g( m );
            in_use -= std::min( in_use, cap );
            if( free_bytes + cap <= free_limit() ) { free_list.emplace( cap, p ); free_bytes += cap; return; }
            st.frees++;
        }
        if( pinned ) { forget_pinned( p ); psx_host_free( p ); } else free( p );      // only beyond the byte bound: never in a steady stream
    }
    Stats stats()
    {
        std::lock_guard<std::mutex> g( m );
        Stats s = st; s.free_bytes = free_bytes; s.in_use = in_use; s.free_buffers = (long)free_list.size();
        return s;
    }
};

Pool& plain()  { static Pool* p = new Pool( false, -1 ); return *p; }     // never destroyed: objects may outlive main()
// one pinned pool per device: replicas on different devices share neither a mutex nor buffers (a buffer allocated
// next to GPU 0 is never handed to GPU 5)
Pool& pinned( int device )
{
    static Pool** pools = []{ Pool** a = new Pool*[MAX_POOLS]; for( int i = 0; i < MAX_POOLS; i++ ) a[i] = new Pool( true, i < MAX_POOLS - 1 ? i : -1 ); return a; }();
    return *pools[ ( device >= 0 && device < MAX_POOLS - 1 ) ? device : MAX_POOLS - 1 ];
}

// which pool a live pinned buffer belongs to: objects (SiftJob, FeaturesHost) outlive the thread that got the buffer and
// do not carry a device; 16 shards, each a tiny critical section
struct Registry
{
    std::mutex m[16];
    std::unordered_map<void*, int> map[16];
    static int shard( void* p ) { return (int)( ( (uintptr_t)p >> 12 ) & 15 ); }
    void set( void* p, int dev ) { const int s = shard( p ); std::lock_guard<std::mutex> g( m[s] ); map[s][p] = dev; }
    int  get( void* p )          { const int s = shard( p ); std::lock_guard<std::mutex> g( m[s] ); auto it = map[s].find( p ); return it == map[s].end() ? -1 : it->second; }
    void erase( void* p )        { const int s = shard( p ); std::lock_guard<std::mutex> g( m[s] ); map[s].erase( p ); }
};
Registry& registry() { static Registry* r = new Registry; return *r; }
void forget_pinned( void* p ) { registry().erase( p ); }
thread_local int t_device = -1;
} // namespace

bool  pin_thread_to_device_cpus( int device )
{
    DeviceCpus& dc = device_cpus( device );
    return dc.valid && sched_setaffinity( 0, sizeof(cpu_set_t), &dc.set ) == 0;
}
void  set_thread_device( int device )         { t_device = device; }
int   thread_device( )                        { return t_device; }
void* get_plain( size_t bytes, size_t* cap )  { return plain().get( bytes, cap ); }
void  put_plain( void* p, size_t cap )        { plain().put( p, cap ); }
void* get_pinned( size_t bytes, size_t* cap )
{
    const int dev = t_device;
    void* p = pinned( dev ).get( bytes, cap );
    if( p != nullptr ) registry().set( p, dev );
    return p;
}
void  put_pinned( void* p, size_t cap )       { if( p != nullptr ) pinned( registry().get( p ) ).put( p, cap ); }
size_t pinned_in_use( )
{
    // of the calling thread's device: the limit is a per-replica allowance
    return pinned( t_device ).stats().in_use;
}
Stats pinned_stats( int device )
{
    if( device >= 0 ) return pinned( device ).stats();
    Stats sum;
    for( int i = 0; i < MAX_POOLS; i++ ) {
        const Stats s = pinned( i < MAX_POOLS - 1 ? i : -1 ).stats();
        sum.allocs += s.allocs; sum.frees += s.frees; sum.hits += s.hits; sum.free_bytes += s.free_bytes; sum.in_use += s.in_use; sum.free_buffers += s.free_buffers;
    }
    return sum;
}
} // namespace pool

FeaturesHost::FeaturesHost( ) : _ext( nullptr ), _ori( nullptr ), _ext_cap( 0 ), _ori_cap( 0 ), _bytes( false ) { }

FeaturesHost::FeaturesHost( int num_ext, int num_ori ) : _ext( nullptr ), _ori( nullptr ), _ext_cap( 0 ), _ori_cap( 0 ), _bytes( false )
{
    reset( num_ext, num_ori );
}

FeaturesHost::~FeaturesHost( )
{
    release();
}

void FeaturesHost::release( )
{
    if( _ext_cap ) pool::put_plain( _ext, _ext_cap ); else free( _ext );
    if( _ori_cap ) pool::put_pinned( _ori, _ori_cap ); else free( _ori );
    _ext = nullptr; _ori = nullptr; _ext_cap = _ori_cap = 0;
    _bytes = false;
    _desc_idx.clear();
}

void FeaturesHost::adoptBytes( int num_ext, int num_ori, Feature* ext, size_t ext_cap, unsigned char* bytes, size_t bytes_cap,
                               std::vector<int>&& desc_idx )
{
    release();
    _ext = ext; _ext_cap = ext_cap;
    _ori = reinterpret_cast<Descriptor*>( bytes ); _ori_cap = bytes_cap;
    _bytes = true;
    _desc_idx = std::move( desc_idx );
    setFeatureCount( num_ext );
    setDescriptorCount( num_ori );
}

void FeaturesHost::resetBytes( int num_ext, int num_ori )
{
    release();
    _ext = (Feature*)page_alloc( (size_t)num_ext * sizeof(Feature) );
    _ori = (Descriptor*)page_alloc( (size_t)num_ori * 128 );
    if( _ext == nullptr || _ori == nullptr ) {
        std::ostringstream ss;
        ss << "Runtime error:" << std::endl
           << "    Failed to (re)allocate memory for downloading " << num_ext << " features and " << num_ori << " byte descriptors";
        fatal( __FILE__, __LINE__, ss.str() );
    }
    _bytes = true;
    _desc_idx.assign( (size_t)num_ext * ORIENTATION_MAX_COUNT, -1 );
    setFeatureCount( num_ext );
    setDescriptorCount( num_ori );
}

int FeaturesHost::descriptorIndex( int feature, int ori ) const
{
    if( feature < 0 || feature >= size() || ori < 0 || ori >= ORIENTATION_MAX_COUNT ) return -1;
    if( _bytes ) return _desc_idx[(size_t)feature * ORIENTATION_MAX_COUNT + ori];
    const Descriptor* d = _ext[feature].desc[ori];
    return d ? (int)( d - _ori ) : -1;
}

const unsigned char* FeaturesHost::descriptorBytes( int feature, int ori ) const
{
    if( !_bytes ) return nullptr;
    const int j = descriptorIndex( feature, ori );
    if( j < 0 || j >= getDescriptorCount() ) return nullptr;
    return reinterpret_cast<const unsigned char*>( _ori ) + (size_t)j * 128;
}

void FeaturesHost::adopt( int num_ext, int num_ori, Feature* ext, size_t ext_cap, Descriptor* ori, size_t ori_cap )
{
    release();
    _ext = ext; _ext_cap = ext_cap;
    _ori = ori; _ori_cap = ori_cap;
    setFeatureCount( num_ext );
    setDescriptorCount( num_ori );
}

void FeaturesHost::reset( int num_ext, int num_ori )
{
    release();

    _ext = (Feature*)page_alloc( (size_t)num_ext * sizeof(Feature) );
    if( _ext == nullptr ) {
        std::ostringstream ss;
        ss << "Runtime error:" << std::endl
           << "    Failed to (re)allocate memory for downloading " << num_ext << " features";
        fatal( __FILE__, __LINE__, ss.str() );
    }
    _ori = (Descriptor*)page_alloc( (size_t)num_ori * sizeof(Descriptor) );
    if( _ori == nullptr ) {
        std::ostringstream ss;
        ss << "Runtime error:" << std::endl
           << "    Failed to (re)allocate memory for downloading " << num_ori << " descriptors";
        fatal( __FILE__, __LINE__, ss.str() );
    }
    setFeatureCount( num_ext );
    setDescriptorCount( num_ori );
}

void FeaturesHost::pin( )   { }
void FeaturesHost::unpin( ) { }

void FeaturesHost::print( std::ostream& ostr, bool write_as_uchar ) const
{
    if( !_bytes ) {
        for( int i = 0; i < size(); i++ ) _ext[i].print( ostr, write_as_uchar );
        return;
    }
    // byte result: the usual line with the bytes as integers (what --write-as-uchar prints for values <= 255)
    for( int i = 0; i < size(); i++ ) {
        const Feature& f = _ext[i];
        const float sigval = 1.0f / ( f.sigma * f.sigma );
        for( int ori = 0; ori < f.num_ori; ori++ ) {
            ostr << f.xpos << " " << f.ypos << " " << sigval << " 0 " << sigval << " ";
            const unsigned char* b = descriptorBytes( i, ori );
            if( b != nullptr )
                for( int k = 0; k < 128; k++ ) ostr << (int)b[k] << " ";
            ostr << std::endl;
        }
    }
}

std::ostream& operator<<( std::ostream& ostr, const FeaturesHost& feature )
{
    feature.print( ostr, false );
    return ostr;
}

// output-features.txt line format (features.cu:310-330): x y 1/s^2 0 1/s^2 d0..d127
void Feature::print( std::ostream& ostr, bool write_as_uchar ) const
{
    const float sigval = 1.0f / ( sigma * sigma );
    for( int ori = 0; ori < num_ori; ori++ ) {
        ostr << xpos << " " << ypos << " " << sigval << " 0 " << sigval << " ";
        if( desc[ori] == nullptr ) {
            // a byte result (Config::ByteDescriptors) has no float descriptors: FeaturesHost::print writes its bytes
        } else if( write_as_uchar ) {
            for( int i = 0; i < 128; i++ ) ostr << roundf( desc[ori]->features[i] ) << " ";
        } else {
            ostr << std::setprecision(3);
            for( int i = 0; i < 128; i++ ) ostr << desc[ori]->features[i] << " ";
            ostr << std::setprecision(6);
        }
        ostr << std::endl;
    }
}

std::ostream& operator<<( std::ostream& ostr, const Feature& feature )
{
    feature.print( ostr, false );
    return ostr;
}

// FeaturesDev hands out device arrays of popsift::Feature; the C-ABI fills them as psx_feature_dev
static_assert( sizeof(Feature) == sizeof(psx_feature_dev), "popsift::Feature and psx_feature_dev must have the same layout" );
static_assert( offsetof(Feature, desc) == offsetof(psx_feature_dev, desc), "popsift::Feature::desc offset" );
static_assert( offsetof(Feature, orientation) == offsetof(psx_feature_dev, orientation), "popsift::Feature::orientation offset" );

FeaturesDev::FeaturesDev( ) : _ext( nullptr ), _ori( nullptr ), _rev( nullptr ), _device( 0 ) { }

FeaturesDev::FeaturesDev( int num_ext, int num_ori ) : _ext( nullptr ), _ori( nullptr ), _rev( nullptr ), _device( 0 )
{
    reset( num_ext, num_ori );
}

FeaturesDev::~FeaturesDev( )
{
    psx_dev_free( _device, _ext );
    psx_dev_free( _device, _ori );
    psx_dev_free( _device, _rev );
}

void FeaturesDev::reset( int num_ext, int num_ori )
{
    psx_dev_free( _device, _ext ); _ext = nullptr;
    psx_dev_free( _device, _ori ); _ori = nullptr;
    psx_dev_free( _device, _rev ); _rev = nullptr;
    void *e = nullptr, *o = nullptr, *r = nullptr;
    if( psx_dev_alloc( _device, (size_t)num_ext * sizeof(Feature), &e ) != PSX_OK ||
        psx_dev_alloc( _device, (size_t)num_ori * sizeof(Descriptor), &o ) != PSX_OK ||
        psx_dev_alloc( _device, (size_t)num_ori * sizeof(int), &r ) != PSX_OK )
        fatal( __FILE__, __LINE__, "Runtime error:\n    Failed to allocate device memory for features" );
    _ext = (Feature*)e; _ori = (Descriptor*)o; _rev = (int*)r;
    setFeatureCount( num_ext );
    setDescriptorCount( num_ori );
}

// FeaturesDev::match (features.cu:270-304): the reference computes the match matrix on the device and
// prints one line per left descriptor from a device printf (show_distance, features.cu:227-268); same
// lines here, printed by the host from the arrays psx_match returns.
void FeaturesDev::match( FeaturesDev* other )
{
    if( other == nullptr ) fatal( __FILE__, __LINE__, "FeaturesDev::match: null argument" );
    const int l_len = getDescriptorCount();
    const int r_len = other->getDescriptorCount();
    if( l_len <= 0 ) return;
    std::vector<int>   mm( 3 * (size_t)l_len );
    std::vector<float> dd( 2 * (size_t)l_len );
    std::vector<int>   l_fem( l_len ), r_fem( r_len > 0 ? r_len : 1 );
    if( psx_match( _device, (const float*)_ori, l_len, (const float*)other->_ori, r_len, mm.data(), dd.data() ) != PSX_OK ||
        psx_dev_read( _device, l_fem.data(), _rev, (size_t)l_len * sizeof(int) ) != PSX_OK ||
        ( r_len > 0 && psx_dev_read( other->_device, r_fem.data(), other->_rev, (size_t)r_len * sizeof(int) ) != PSX_OK ) )
        fatal( __FILE__, __LINE__, "FeaturesDev::match failed" );
    for( int i = 0; i < l_len; i++ )
    {
        const int m1 = mm[3*i], m2 = mm[3*i+1];
        printf( "%s feat %4d [%4d] matches feat %4d [%4d] ( 2nd feat %4d [%4d] ) dist %.3f vs %.3f\n",
                mm[3*i+2] ? "accept" : "reject",
                l_fem[i], i,
                r_len > 0 ? r_fem[m1] : 0, m1,
                r_len > 0 ? r_fem[m2] : 0, m2,
                dd[2*i], dd[2*i+1] );
    }
}

// FeaturesDev::matchBytes: both descriptor sets quantised on the device with the byte rule, then psx_match_u8 (exact:
// the reference's result on the bytes, bit for bit); same lines as match(), the integer distances printed alike
void FeaturesDev::matchBytes( FeaturesDev* other )
{
    if( other == nullptr ) fatal( __FILE__, __LINE__, "FeaturesDev::matchBytes: null argument" );
    const int l_len = getDescriptorCount();
    const int r_len = other->getDescriptorCount();
    if( l_len <= 0 ) return;
    std::vector<int> mm( 3 * (size_t)l_len ), dd( 2 * (size_t)l_len );
    std::vector<int> l_fem( l_len ), r_fem( r_len > 0 ? r_len : 1 );
    void *lb = nullptr, *rb = nullptr;
    bool ok = psx_dev_alloc( _device, (size_t)l_len * 128, &lb ) == PSX_OK &&
              psx_dev_alloc( _device, (size_t)( r_len > 0 ? r_len : 1 ) * 128, &rb ) == PSX_OK &&
              psx_quantize_desc( _device, (const float*)_ori, l_len, (unsigned char*)lb ) == PSX_OK &&
              psx_quantize_desc( _device, (const float*)other->_ori, r_len, (unsigned char*)rb ) == PSX_OK &&
              psx_match_u8( _device, (const unsigned char*)lb, l_len, (const unsigned char*)rb, r_len, mm.data(), dd.data() ) == PSX_OK &&
              psx_dev_read( _device, l_fem.data(), _rev, (size_t)l_len * sizeof(int) ) == PSX_OK &&
              ( r_len <= 0 || psx_dev_read( other->_device, r_fem.data(), other->_rev, (size_t)r_len * sizeof(int) ) == PSX_OK );
    psx_dev_free( _device, lb );
    psx_dev_free( _device, rb );
    if( !ok ) fatal( __FILE__, __LINE__, "FeaturesDev::matchBytes failed" );
    for( int i = 0; i < l_len; i++ )
    {
        const int m1 = mm[3*i], m2 = mm[3*i+1];
        const float d1 = dd[2*i] == INT32_MAX ? INFINITY : (float)dd[2*i];
        const float d2 = dd[2*i+1] == INT32_MAX ? INFINITY : (float)dd[2*i+1];
        printf( "%s feat %4d [%4d] matches feat %4d [%4d] ( 2nd feat %4d [%4d] ) dist %.3f vs %.3f\n",
                mm[3*i+2] ? "accept" : "reject",
                l_fem[i], i,
                r_len > 0 ? r_fem[m1] : 0, m1,
                r_len > 0 ? r_fem[m2] : 0, m2,
                d1, d2 );
    }
}

// FeaturesDev::matchPairs / matchPairsGuided: psx_match_pairs* / psx_match_pairs_guided* on the two descriptor arrays; the
// pair list (16 bytes per pair) and the two reverse maps come back, nothing per descriptor.  guide == nullptr: unguided.
static std::vector<Match> match_pairs_impl( const char* who, int device, int other_device,
                                            Feature* l_ext, Descriptor* l_ori, int* l_rev, int l_len,
                                            Feature* r_ext, Descriptor* r_ori, int* r_rev, int r_len,
                                            const MatchGuide* guide, const MatchOptions& opts )
{
    std::vector<Match> out;
    psx_guide pg;
    if( guide != nullptr ) {
        pg.kind = (int)guide->kind;
        for( int k = 0; k < 9; k++ ) pg.m[k] = guide->m[k];
        pg.tol = guide->tol;
        // refused here, before any device is touched (and for empty sides too): what psx_match_pairs_guided refuses
        bool ok = ( pg.kind == PSX_GUIDE_HOMOGRAPHY || pg.kind == PSX_GUIDE_EPIPOLAR ) && std::isfinite( pg.tol ) && pg.tol >= 0.0f;
        for( int k = 0; k < 9; k++ ) ok = ok && std::isfinite( pg.m[k] );
        if( !ok ) fatal( __FILE__, __LINE__, std::string( who ) + ": invalid guide (kind 1 or 2, finite entries, finite tolerance >= 0)" );
    }
    if( l_len <= 0 || r_len <= 0 ) return out;
    psx_match_opts po;
    po.ratio = opts.ratio;
    po.flags = opts.mutual ? PSX_PAIRS_MUTUAL : 0;
    int count = 0;
    std::vector<psx_match_pair>    pf;
    std::vector<psx_match_pair_u8> pb;
    int rc = PSX_OK;
    void *lb = nullptr, *rb = nullptr, *lxy = nullptr, *rxy = nullptr;
    if( guide != nullptr ) {
        rc = psx_dev_alloc( device, (size_t)l_len * 2 * sizeof(float), &lxy );
        if( rc == PSX_OK ) rc = psx_dev_alloc( device, (size_t)r_len * 2 * sizeof(float), &rxy );
        if( rc == PSX_OK ) rc = psx_desc_positions( device, (const psx_feature_dev*)l_ext, l_rev, l_len, (float*)lxy );
        if( rc == PSX_OK ) rc = psx_desc_positions( device, (const psx_feature_dev*)r_ext, r_rev, r_len, (float*)rxy );
    }
    if( opts.bytes ) {
        pb.resize( l_len );
        if( rc == PSX_OK ) rc = psx_dev_alloc( device, (size_t)l_len * 128, &lb );
        if( rc == PSX_OK ) rc = psx_dev_alloc( device, (size_t)r_len * 128, &rb );
        if( rc == PSX_OK ) rc = psx_quantize_desc( device, (const float*)l_ori, l_len, (unsigned char*)lb );
        if( rc == PSX_OK ) rc = psx_quantize_desc( device, (const float*)r_ori, r_len, (unsigned char*)rb );
        if( rc == PSX_OK && guide == nullptr )
            rc = psx_match_pairs_u8( device, (const unsigned char*)lb, l_len, (const unsigned char*)rb, r_len, &po, pb.data(), l_len, &count );
        else if( rc == PSX_OK )
            rc = psx_match_pairs_guided_u8( device, (const unsigned char*)lb, (const float*)lxy, l_len, (const unsigned char*)rb, (const float*)rxy, r_len,
                                            &pg, &po, pb.data(), l_len, &count );
    } else {
        pf.resize( l_len );
        if( rc == PSX_OK && guide == nullptr )
            rc = psx_match_pairs( device, (const float*)l_ori, l_len, (const float*)r_ori, r_len, &po, pf.data(), l_len, &count );
        else if( rc == PSX_OK )
            rc = psx_match_pairs_guided( device, (const float*)l_ori, (const float*)lxy, l_len, (const float*)r_ori, (const float*)rxy, r_len,
                                         &pg, &po, pf.data(), l_len, &count );
    }
    psx_dev_free( device, lb );
    psx_dev_free( device, rb );
    psx_dev_free( device, lxy );
    psx_dev_free( device, rxy );
    if( rc != PSX_OK ) {
        std::ostringstream ss;
        ss << who << " failed (" << rc << ( rc == PSX_ERR_INVALID ? ": invalid options" : "" ) << ")";
        fatal( __FILE__, __LINE__, ss.str() );
    }
    std::vector<int> l_fem( l_len ), r_fem( r_len );
    if( psx_dev_read( device, l_fem.data(), l_rev, (size_t)l_len * sizeof(int) ) != PSX_OK ||
        psx_dev_read( other_device, r_fem.data(), r_rev, (size_t)r_len * sizeof(int) ) != PSX_OK )
        fatal( __FILE__, __LINE__, std::string( who ) + ": reading the reverse maps failed" );
    out.resize( count );
    for( int k = 0; k < count; k++ ) {
        Match& m = out[k];
        if( opts.bytes ) {
            m.left_descriptor = pb[k].left; m.right_descriptor = pb[k].right;
            m.distance        = pb[k].d1 == INT32_MAX ? INFINITY : (float)pb[k].d1;
            m.second_distance = pb[k].d2 == INT32_MAX ? INFINITY : (float)pb[k].d2;
        } else {
            m.left_descriptor = pf[k].left; m.right_descriptor = pf[k].right;
            m.distance = pf[k].d1; m.second_distance = pf[k].d2;
        }
        m.left_feature  = l_fem[m.left_descriptor];
        m.right_feature = r_fem[m.right_descriptor];
    }
    return out;
}

std::vector<Match> FeaturesDev::matchPairs( FeaturesDev* other, const MatchOptions& opts )
{
    if( other == nullptr ) fatal( __FILE__, __LINE__, "FeaturesDev::matchPairs: null argument" );
    if( other->_device != _device ) {
        std::ostringstream ss;
        ss << "FeaturesDev::matchPairs: the two objects live on different devices (" << _device << " and " << other->_device << ")";
        fatal( __FILE__, __LINE__, ss.str() );
    }
    return match_pairs_impl( "FeaturesDev::matchPairs", _device, other->_device, _ext, _ori, _rev, getDescriptorCount(),
                             other->_ext, other->_ori, other->_rev, other->getDescriptorCount(), nullptr, opts );
}

std::vector<Match> FeaturesDev::matchPairsGuided( FeaturesDev* other, const MatchGuide& guide, const MatchOptions& opts )
{
    if( other == nullptr ) fatal( __FILE__, __LINE__, "FeaturesDev::matchPairsGuided: null argument" );
    if( other->_device != _device ) {
        std::ostringstream ss;
        ss << "FeaturesDev::matchPairsGuided: the two objects live on different devices (" << _device << " and " << other->_device << ")";
        fatal( __FILE__, __LINE__, ss.str() );
    }
    return match_pairs_impl( "FeaturesDev::matchPairsGuided", _device, other->_device, _ext, _ori, _rev, getDescriptorCount(),
                             other->_ext, other->_ori, other->_rev, other->getDescriptorCount(), &guide, opts );
}

// FeaturesDev::matchPairsMany: psx_match_pairs_many_u8 on this object's bytes and every other object's -- each side
// quantised once, ONE matching call for all of them; the concatenated list is cut at the per-set counts and mapped through
// the reverse maps as matchPairs does
std::vector<std::vector<Match>> FeaturesDev::matchPairsMany( const std::vector<FeaturesDev*>& others, const MatchOptions& opts )
{
    const char* who = "FeaturesDev::matchPairsMany";
    for( FeaturesDev* o : others ) {
        if( o == nullptr ) fatal( __FILE__, __LINE__, std::string( who ) + ": null argument" );
        if( o->_device != _device ) {
            std::ostringstream ss;
            ss << who << ": the objects live on different devices (" << _device << " and " << o->_device << ")";
            fatal( __FILE__, __LINE__, ss.str() );
        }
    }
    if( !opts.bytes ) fatal( __FILE__, __LINE__, std::string( who ) + ": the one-to-many form is byte-only (set MatchOptions::bytes)" );
    const int K = (int)others.size();
    const int l_len = getDescriptorCount();
    std::vector<std::vector<Match>> out( others.size() );
    bool any = false;
    for( FeaturesDev* o : others ) any = any || o->getDescriptorCount() > 0;
    if( l_len <= 0 || !any ) return out;
    psx_match_opts po;
    po.ratio = opts.ratio;
    po.flags = opts.mutual ? PSX_PAIRS_MUTUAL : 0;
    std::vector<void*> bufs( (size_t)K + 1, nullptr );
    std::vector<const unsigned char*> ptrs( K, nullptr );
    std::vector<int> lens( K, 0 ), counts( K, 0 );
    int rc = psx_dev_alloc( _device, (size_t)l_len * 128, &bufs[K] );
    if( rc == PSX_OK ) rc = psx_quantize_desc( _device, (const float*)_ori, l_len, (unsigned char*)bufs[K] );
    for( int k = 0; k < K && rc == PSX_OK; k++ ) {
        const int r_len = others[k]->getDescriptorCount();
        if( r_len <= 0 ) continue;
        lens[k] = r_len;
        rc = psx_dev_alloc( _device, (size_t)r_len * 128, &bufs[k] );
        if( rc == PSX_OK ) rc = psx_quantize_desc( _device, (const float*)others[k]->_ori, r_len, (unsigned char*)bufs[k] );
        ptrs[k] = (const unsigned char*)bufs[k];
    }
    // at most l_len pairs per set exist (a product above INT_MAX is the call's to refuse)
    const long long room = (long long)K * l_len;
    std::vector<psx_match_pair_u8> pb( (size_t)( room < INT32_MAX ? room : INT32_MAX ) );
    int count = 0;
    if( rc == PSX_OK )
        rc = psx_match_pairs_many_u8( _device, (const unsigned char*)bufs[K], l_len, ptrs.data(), lens.data(), K, &po,
                                      pb.data(), (int)pb.size(), counts.data(), &count );
    for( void* b : bufs ) psx_dev_free( _device, b );
    if( rc != PSX_OK ) {
        std::ostringstream ss;
        ss << who << " failed (" << rc << ( rc == PSX_ERR_INVALID ? ": invalid options" : "" ) << ")";
        fatal( __FILE__, __LINE__, ss.str() );
    }
    std::vector<int> l_fem( l_len );
    if( psx_dev_read( _device, l_fem.data(), _rev, (size_t)l_len * sizeof(int) ) != PSX_OK )
        fatal( __FILE__, __LINE__, std::string( who ) + ": reading the reverse maps failed" );
    size_t at = 0;
    for( int k = 0; k < K; k++ ) {
        if( counts[k] <= 0 ) continue;
        std::vector<int> r_fem( lens[k] );
        if( psx_dev_read( _device, r_fem.data(), others[k]->_rev, (size_t)lens[k] * sizeof(int) ) != PSX_OK )
            fatal( __FILE__, __LINE__, std::string( who ) + ": reading the reverse maps failed" );
        out[k].resize( counts[k] );
        for( int q = 0; q < counts[k]; q++, at++ ) {
            Match& m = out[k][q];
            m.left_descriptor = pb[at].left; m.right_descriptor = pb[at].right;
            m.distance        = pb[at].d1 == INT32_MAX ? INFINITY : (float)pb[at].d1;
            m.second_distance = pb[at].d2 == INT32_MAX ? INFINITY : (float)pb[at].d2;
            m.left_feature  = l_fem[m.left_descriptor];
            m.right_feature = r_fem[m.right_descriptor];
        }
    }
    return out;
}

// FeaturesDev::matchPairsGraph: psx_match_pairs_graph_u8 on the bytes of every view an edge names -- each quantised once
// for the whole call, ONE matching call for all edges; the concatenated list is cut at the per-edge counts and mapped
// through the two views' reverse maps as matchPairs does
std::vector<std::vector<Match>> FeaturesDev::matchPairsGraph( const std::vector<FeaturesDev*>& views, const std::vector<std::pair<int,int>>& edges,
                                                              const MatchOptions& opts )
{
    const char* who = "FeaturesDev::matchPairsGraph";
    const int N = (int)views.size(), E = (int)edges.size();
    std::vector<char> named( views.size(), 0 );
    for( const std::pair<int,int>& e : edges ) {
        if( e.first < 0 || e.first >= N || e.second < 0 || e.second >= N ) {
            std::ostringstream ss;
            ss << who << ": edge (" << e.first << ", " << e.second << ") out of range (" << N << " views)";
            fatal( __FILE__, __LINE__, ss.str() );
        }
        named[e.first] = named[e.second] = 1;
    }
    int device = -1;
    for( int v = 0; v < N; v++ ) {
        if( !named[v] ) continue;
        if( views[v] == nullptr ) fatal( __FILE__, __LINE__, std::string( who ) + ": null argument" );
        if( device < 0 ) device = views[v]->_device;
        if( views[v]->_device != device ) {
            std::ostringstream ss;
            ss << who << ": the objects live on different devices (" << device << " and " << views[v]->_device << ")";
            fatal( __FILE__, __LINE__, ss.str() );
        }
    }
    if( !opts.bytes ) fatal( __FILE__, __LINE__, std::string( who ) + ": the edge-list form is byte-only (set MatchOptions::bytes)" );
    std::vector<std::vector<Match>> out( edges.size() );
    std::vector<int> lens( views.size(), 0 );
    for( int v = 0; v < N; v++ ) if( named[v] && views[v]->getDescriptorCount() > 0 ) lens[v] = views[v]->getDescriptorCount();
    long long room = 0;                                      // at most lens[left] pairs per edge exist
    std::vector<char> used( views.size(), 0 );               // named by an edge with two non-empty sides: only these are quantised
    for( const std::pair<int,int>& e : edges )
        if( lens[e.first] > 0 && lens[e.second] > 0 ) { room += lens[e.first]; used[e.first] = used[e.second] = 1; }
    if( room == 0 ) return out;
    psx_match_opts po;
    po.ratio = opts.ratio;
    po.flags = opts.mutual ? PSX_PAIRS_MUTUAL : 0;
    std::vector<void*> bufs( views.size(), nullptr );
    std::vector<const unsigned char*> ptrs( views.size(), nullptr );
    int rc = PSX_OK;
    for( int v = 0; v < N && rc == PSX_OK; v++ ) {
        if( !used[v] ) { lens[v] = 0; continue; }            // a view no live edge names is an empty set to the call
        rc = psx_dev_alloc( device, (size_t)lens[v] * 128, &bufs[v] );
        if( rc == PSX_OK ) rc = psx_quantize_desc( device, (const float*)views[v]->_ori, lens[v], (unsigned char*)bufs[v] );
        ptrs[v] = (const unsigned char*)bufs[v];
    }
    std::vector<psx_view_edge> pe( edges.size() );
    for( int e = 0; e < E; e++ ) { pe[e].left = edges[e].first; pe[e].right = edges[e].second; }
    std::vector<psx_match_pair_u8> pb( (size_t)( room < INT32_MAX ? room : INT32_MAX ) );
    std::vector<int> counts( edges.size(), 0 );
    int count = 0;
    if( rc == PSX_OK )
        rc = psx_match_pairs_graph_u8( device, ptrs.data(), lens.data(), N, pe.data(), E, &po, pb.data(), (int)pb.size(), counts.data(), &count );
    for( void* b : bufs ) psx_dev_free( device, b );
    if( rc != PSX_OK ) {
        std::ostringstream ss;
        ss << who << " failed (" << rc << ( rc == PSX_ERR_INVALID ? ": invalid options" : "" ) << ")";
        fatal( __FILE__, __LINE__, ss.str() );
    }
    std::vector<std::vector<int>> fem( views.size() );       // every used view's reverse map, read once
    for( int v = 0; v < N; v++ ) {
        if( !used[v] ) continue;
        fem[v].resize( lens[v] );
        if( psx_dev_read( device, fem[v].data(), views[v]->_rev, (size_t)lens[v] * sizeof(int) ) != PSX_OK )
            fatal( __FILE__, __LINE__, std::string( who ) + ": reading the reverse maps failed" );
    }
    size_t at = 0;
    for( int e = 0; e < E; e++ ) {
        if( counts[e] <= 0 ) continue;
        const std::vector<int>& l_fem = fem[pe[e].left];
        const std::vector<int>& r_fem = fem[pe[e].right];
        out[e].resize( counts[e] );
        for( int q = 0; q < counts[e]; q++, at++ ) {
            Match& m = out[e][q];
            m.left_descriptor = pb[at].left; m.right_descriptor = pb[at].right;
            m.distance        = pb[at].d1 == INT32_MAX ? INFINITY : (float)pb[at].d1;
            m.second_distance = pb[at].d2 == INT32_MAX ? INFINITY : (float)pb[at].d2;
            m.left_feature  = l_fem[m.left_descriptor];
            m.right_feature = r_fem[m.right_descriptor];
        }
    }
    return out;
}

// FeaturesDev::matchPairsManyFloat: psx_match_pairs_many on the objects' own float descriptors -- nothing is quantised,
// nothing is copied, ONE matching call for all of them; the concatenated list is cut at the per-set counts and mapped
// through the reverse maps as matchPairs does
std::vector<std::vector<Match>> FeaturesDev::matchPairsManyFloat( const std::vector<FeaturesDev*>& others, const MatchOptions& opts )
{
    const char* who = "FeaturesDev::matchPairsManyFloat";
    for( FeaturesDev* o : others ) {
        if( o == nullptr ) fatal( __FILE__, __LINE__, std::string( who ) + ": null argument" );
        if( o->_device != _device ) {
            std::ostringstream ss;
            ss << who << ": the objects live on different devices (" << _device << " and " << o->_device << ")";
            fatal( __FILE__, __LINE__, ss.str() );
        }
    }
    if( opts.bytes ) fatal( __FILE__, __LINE__, std::string( who ) + ": float descriptors only (use matchPairsMany for MatchOptions::bytes)" );
    const int K = (int)others.size();
    const int l_len = getDescriptorCount();
    std::vector<std::vector<Match>> out( others.size() );
    bool any = false;
    for( FeaturesDev* o : others ) any = any || o->getDescriptorCount() > 0;
    if( l_len <= 0 || !any ) return out;
    psx_match_opts po;
    po.ratio = opts.ratio;
    po.flags = opts.mutual ? PSX_PAIRS_MUTUAL : 0;
    std::vector<const float*> ptrs( K, nullptr );
    std::vector<int> lens( K, 0 ), counts( K, 0 );
    for( int k = 0; k < K; k++ ) {
        const int r_len = others[k]->getDescriptorCount();
        if( r_len <= 0 ) continue;
        lens[k] = r_len;
        ptrs[k] = (const float*)others[k]->_ori;
    }
    // at most l_len pairs per set exist (a product above INT_MAX is the call's to refuse)
    const long long room = (long long)K * l_len;
    std::vector<psx_match_pair> pf( (size_t)( room < INT32_MAX ? room : INT32_MAX ) );
    int count = 0;
    const int rc = psx_match_pairs_many( _device, (const float*)_ori, l_len, ptrs.data(), lens.data(), K, &po,
                                         pf.data(), (int)pf.size(), counts.data(), &count );
    if( rc != PSX_OK ) {
        std::ostringstream ss;
        ss << who << " failed (" << rc << ( rc == PSX_ERR_INVALID ? ": invalid options" : "" ) << ")";
        fatal( __FILE__, __LINE__, ss.str() );
    }
    std::vector<int> l_fem( l_len );
    if( psx_dev_read( _device, l_fem.data(), _rev, (size_t)l_len * sizeof(int) ) != PSX_OK )
        fatal( __FILE__, __LINE__, std::string( who ) + ": reading the reverse maps failed" );
    size_t at = 0;
    for( int k = 0; k < K; k++ ) {
        if( counts[k] <= 0 ) continue;
        std::vector<int> r_fem( lens[k] );
        if( psx_dev_read( _device, r_fem.data(), others[k]->_rev, (size_t)lens[k] * sizeof(int) ) != PSX_OK )
            fatal( __FILE__, __LINE__, std::string( who ) + ": reading the reverse maps failed" );
        out[k].resize( counts[k] );
        for( int q = 0; q < counts[k]; q++, at++ ) {
            Match& m = out[k][q];
            m.left_descriptor = pf[at].left; m.right_descriptor = pf[at].right;
            m.distance = pf[at].d1; m.second_distance = pf[at].d2;
            m.left_feature  = l_fem[m.left_descriptor];
            m.right_feature = r_fem[m.right_descriptor];
        }
    }
    return out;
}

// FeaturesDev::matchPairsGuidedMany: psx_match_pairs_guided_many_u8 on this object's bytes and positions and every other
// object's that is neither empty nor skipped -- each side quantised and its positions gathered once, ONE matching call for
// all of them; the concatenated list is cut at the per-set counts and mapped through the reverse maps as matchPairs does
std::vector<std::vector<Match>> FeaturesDev::matchPairsGuidedMany( const std::vector<FeaturesDev*>& others, const std::vector<MatchGuide>& guides,
                                                                   const MatchOptions& opts )
{
    const char* who = "FeaturesDev::matchPairsGuidedMany";
    for( FeaturesDev* o : others ) {
        if( o == nullptr ) fatal( __FILE__, __LINE__, std::string( who ) + ": null argument" );
        if( o->_device != _device ) {
            std::ostringstream ss;
            ss << who << ": the objects live on different devices (" << _device << " and " << o->_device << ")";
            fatal( __FILE__, __LINE__, ss.str() );
        }
    }
    if( !opts.bytes ) fatal( __FILE__, __LINE__, std::string( who ) + ": the one-to-many form is byte-only (set MatchOptions::bytes)" );
    if( guides.size() != others.size() ) {
        std::ostringstream ss;
        ss << who << ": " << others.size() << " objects but " << guides.size() << " guides";
        fatal( __FILE__, __LINE__, ss.str() );
    }
    const int K = (int)others.size();
    std::vector<psx_guide> pg( others.size() );
    for( int k = 0; k < K; k++ ) {
        pg[k].kind = (int)guides[k].kind;
        for( int q = 0; q < 9; q++ ) pg[k].m[q] = guides[k].m[q];
        pg[k].tol = guides[k].tol;
        if( pg[k].kind == PSX_GUIDE_NONE ) continue;
        // refused here, before any device is touched (and for empty sides too): what the call refuses
        bool ok = ( pg[k].kind == PSX_GUIDE_HOMOGRAPHY || pg[k].kind == PSX_GUIDE_EPIPOLAR ) && std::isfinite( pg[k].tol ) && pg[k].tol >= 0.0f;
        for( int q = 0; q < 9; q++ ) ok = ok && std::isfinite( pg[k].m[q] );
        if( !ok ) fatal( __FILE__, __LINE__, std::string( who ) + ": invalid guide (kind 0, 1 or 2, finite entries, finite tolerance >= 0)" );
    }
    const int l_len = getDescriptorCount();
    std::vector<std::vector<Match>> out( others.size() );
    std::vector<int> lens( K, 0 ), counts( K, 0 );
    bool any = false;
    for( int k = 0; k < K; k++ ) {
        if( pg[k].kind != PSX_GUIDE_NONE && others[k]->getDescriptorCount() > 0 ) lens[k] = others[k]->getDescriptorCount();
        any = any || lens[k] > 0;
    }
    if( l_len <= 0 || !any ) return out;
    psx_match_opts po;
    po.ratio = opts.ratio;
    po.flags = opts.mutual ? PSX_PAIRS_MUTUAL : 0;
    // descriptors of set k at [k], its positions at [K + 1 + k]; this object's at [K] and [2 K + 1]
    std::vector<void*> bufs( 2 * (size_t)K + 2, nullptr );
    std::vector<const unsigned char*> ptrs( K, nullptr );
    std::vector<const float*> xys( K, nullptr );
    int rc = psx_dev_alloc( _device, (size_t)l_len * 128, &bufs[K] );
    if( rc == PSX_OK ) rc = psx_dev_alloc( _device, (size_t)l_len * 2 * sizeof(float), &bufs[2 * K + 1] );
    if( rc == PSX_OK ) rc = psx_quantize_desc( _device, (const float*)_ori, l_len, (unsigned char*)bufs[K] );
    if( rc == PSX_OK ) rc = psx_desc_positions( _device, (const psx_feature_dev*)_ext, _rev, l_len, (float*)bufs[2 * K + 1] );
    for( int k = 0; k < K && rc == PSX_OK; k++ ) {
        const int r_len = lens[k];
        if( r_len <= 0 ) continue;
        rc = psx_dev_alloc( _device, (size_t)r_len * 128, &bufs[k] );
        if( rc == PSX_OK ) rc = psx_dev_alloc( _device, (size_t)r_len * 2 * sizeof(float), &bufs[K + 1 + k] );
        if( rc == PSX_OK ) rc = psx_quantize_desc( _device, (const float*)others[k]->_ori, r_len, (unsigned char*)bufs[k] );
        if( rc == PSX_OK ) rc = psx_desc_positions( _device, (const psx_feature_dev*)others[k]->_ext, others[k]->_rev, r_len, (float*)bufs[K + 1 + k] );
        ptrs[k] = (const unsigned char*)bufs[k];
        xys[k] = (const float*)bufs[K + 1 + k];
    }
    // at most l_len pairs per set exist (a product above INT_MAX is the call's to refuse)
    const long long room = (long long)K * l_len;
    std::vector<psx_match_pair_u8> pb( (size_t)( room < INT32_MAX ? room : INT32_MAX ) );
    int count = 0;
    if( rc == PSX_OK )
        rc = psx_match_pairs_guided_many_u8( _device, (const unsigned char*)bufs[K], (const float*)bufs[2 * K + 1], l_len, ptrs.data(), xys.data(),
                                             lens.data(), K, pg.data(), &po, pb.data(), (int)pb.size(), counts.data(), &count );
    for( void* b : bufs ) psx_dev_free( _device, b );
    if( rc != PSX_OK ) {
        std::ostringstream ss;
        ss << who << " failed (" << rc << ( rc == PSX_ERR_INVALID ? ": invalid options" : "" ) << ")";
        fatal( __FILE__, __LINE__, ss.str() );
    }
    std::vector<int> l_fem( l_len );
    if( psx_dev_read( _device, l_fem.data(), _rev, (size_t)l_len * sizeof(int) ) != PSX_OK )
        fatal( __FILE__, __LINE__, std::string( who ) + ": reading the reverse maps failed" );
    size_t at = 0;
    for( int k = 0; k < K; k++ ) {
        if( counts[k] <= 0 ) continue;
        std::vector<int> r_fem( lens[k] );
        if( psx_dev_read( _device, r_fem.data(), others[k]->_rev, (size_t)lens[k] * sizeof(int) ) != PSX_OK )
            fatal( __FILE__, __LINE__, std::string( who ) + ": reading the reverse maps failed" );
        out[k].resize( counts[k] );
        for( int q = 0; q < counts[k]; q++, at++ ) {
            Match& m = out[k][q];
            m.left_descriptor = pb[at].left; m.right_descriptor = pb[at].right;
            m.distance        = pb[at].d1 == INT32_MAX ? INFINITY : (float)pb[at].d1;
            m.second_distance = pb[at].d2 == INT32_MAX ? INFINITY : (float)pb[at].d2;
            m.left_feature  = l_fem[m.left_descriptor];
            m.right_feature = r_fem[m.right_descriptor];
        }
    }
    return out;
}

HomographyEstimate FeaturesDev::estimateHomography( FeaturesDev* other, const std::vector<Match>& matches, const RansacOptions& opts )
{
    return estimate( "FeaturesDev::estimateHomography", ModelHomography, other, matches, opts );
}

FundamentalEstimate FeaturesDev::estimateFundamental( FeaturesDev* other, const std::vector<Match>& matches, const RansacOptions& opts )
{
    return estimate( "FeaturesDev::estimateFundamental", ModelFundamental, other, matches, opts );
}

HomographyEstimate FeaturesDev::estimateAffine( FeaturesDev* other, const std::vector<Match>& matches, const RansacOptions& opts )
{
    return estimate( "FeaturesDev::estimateAffine", ModelAffine, other, matches, opts );
}

HomographyEstimate FeaturesDev::estimateSimilarity( FeaturesDev* other, const std::vector<Match>& matches, const RansacOptions& opts )
{
    return estimate( "FeaturesDev::estimateSimilarity", ModelSimilarity, other, matches, opts );
}

// what differs between the models of estimate() and estimateMany(), in the order of FeaturesDev::RansacModel
namespace {
typedef int (*RansacOneFn)( int, const void*, int, const float*, int, const float*, int, const psx_ransac_opts*, psx_ransac_result*, void*, int, int*,
                            float*, int* );
typedef int (*RansacManyFn)( int, const void*, const int*, int, const float*, int, const float* const*, const int*, const psx_ransac_opts*,
                             psx_ransac_result*, void*, int, int*, float*, int* );
const struct { int min_pairs; RansacOneFn one; RansacManyFn many; } ransac_models[4] = {
    { 4, psx_ransac_homography,  psx_ransac_homography_many },
    { 8, psx_ransac_fundamental, psx_ransac_fundamental_many },
    { 3, psx_ransac_affine,      psx_ransac_affine_many },
    { 2, psx_ransac_similarity,  psx_ransac_similarity_many },
};
}

HomographyEstimate FeaturesDev::estimate( const char* who, RansacModel model, FeaturesDev* other, const std::vector<Match>& matches,
                                          const RansacOptions& opts )
{
    if( other == nullptr ) fatal( __FILE__, __LINE__, std::string( who ) + ": null argument" );
    if( other->_device != _device ) {
        std::ostringstream ss;
        ss << who << ": the two objects live on different devices (" << _device << " and " << other->_device << ")";
        fatal( __FILE__, __LINE__, ss.str() );
    }
    // refused here, before any device is touched: what the psx_ransac_* calls refuse
    if( !( std::isfinite( opts.tol ) && opts.tol >= 0.0f ) || opts.hypotheses < 1 || opts.hypotheses > 65536 )
        fatal( __FILE__, __LINE__, std::string( who ) + ": invalid options (finite tolerance >= 0, 1 to 65536 hypotheses)" );
    HomographyEstimate est;
    est.guide.kind = model == ModelFundamental ? MatchGuide::Epipolar : MatchGuide::Homography;
    for( int k = 0; k < 9; k++ ) est.guide.m[k] = 0.0f;
    est.guide.tol = opts.tol;
    est.best = -1; est.sample_inliers = 0; est.refit_kept = false;
    const int n = (int)matches.size();
    const int l_len = getDescriptorCount(), r_len = other->getDescriptorCount();
    if( n < ransac_models[model].min_pairs ) return est;
    // the record is copied whole: its distance slots carry the index of the match
    std::vector<psx_match_pair_u8> rec( n ), inl( n );
    for( int k = 0; k < n; k++ ) { rec[k].left = matches[k].left_descriptor; rec[k].right = matches[k].right_descriptor; rec[k].d1 = k; rec[k].d2 = 0; }
    psx_ransac_opts po;
    po.tol = opts.tol; po.hypotheses = opts.hypotheses; po.seed = opts.seed; po.flags = opts.refit ? PSX_RANSAC_REFIT : 0;
    psx_ransac_result res;
    int count = 0;
    void *lxy = nullptr, *rxy = nullptr;
    int rc = ( l_len > 0 && r_len > 0 ) ? PSX_OK : PSX_ERR_INVALID;
    if( rc == PSX_OK ) rc = psx_dev_alloc( _device, (size_t)l_len * 2 * sizeof(float), &lxy );
    if( rc == PSX_OK ) rc = psx_dev_alloc( _device, (size_t)r_len * 2 * sizeof(float), &rxy );
    if( rc == PSX_OK ) rc = psx_desc_positions( _device, (const psx_feature_dev*)_ext, _rev, l_len, (float*)lxy );
    if( rc == PSX_OK ) rc = psx_desc_positions( _device, (const psx_feature_dev*)other->_ext, other->_rev, r_len, (float*)rxy );
    if( rc == PSX_OK ) rc = ransac_models[model].one( _device, rec.data(), n, (const float*)lxy, l_len, (const float*)rxy, r_len, &po, &res,
                                                      inl.data(), n, &count, nullptr, nullptr );
    psx_dev_free( _device, lxy );
    psx_dev_free( _device, rxy );
    if( rc != PSX_OK ) {
        std::ostringstream ss;
        ss << who << " failed (" << rc << ( rc == PSX_ERR_INVALID ? ": invalid options or a descriptor index outside its object" : "" ) << ")";
        fatal( __FILE__, __LINE__, ss.str() );
    }
    for( int k = 0; k < 9; k++ ) est.guide.m[k] = res.m[k];
    est.best = res.best; est.sample_inliers = res.sample_inliers; est.refit_kept = res.refit_kept != 0;
    est.inliers.reserve( count );
    for( int k = 0; k < count; k++ ) est.inliers.push_back( matches[inl[k].d1] );
    return est;
}

std::vector<HomographyEstimate> FeaturesDev::estimateHomographyMany( const std::vector<FeaturesDev*>& others,
                                                                     const std::vector<std::vector<Match>>& matches, const RansacOptions& opts )
{
    return estimateMany( "FeaturesDev::estimateHomographyMany", ModelHomography, others, matches, opts );
}

std::vector<FundamentalEstimate> FeaturesDev::estimateFundamentalMany( const std::vector<FeaturesDev*>& others,
                                                                       const std::vector<std::vector<Match>>& matches, const RansacOptions& opts )
{
    return estimateMany( "FeaturesDev::estimateFundamentalMany", ModelFundamental, others, matches, opts );
}

std::vector<HomographyEstimate> FeaturesDev::estimateAffineMany( const std::vector<FeaturesDev*>& others,
                                                                 const std::vector<std::vector<Match>>& matches, const RansacOptions& opts )
{
    return estimateMany( "FeaturesDev::estimateAffineMany", ModelAffine, others, matches, opts );
}

std::vector<HomographyEstimate> FeaturesDev::estimateSimilarityMany( const std::vector<FeaturesDev*>& others,
                                                                     const std::vector<std::vector<Match>>& matches, const RansacOptions& opts )
{
    return estimateMany( "FeaturesDev::estimateSimilarityMany", ModelSimilarity, others, matches, opts );
}

// psx_ransac_homography_many / _fundamental_many / _affine_many / _similarity_many on the lists matchPairsMany returned: the lists that can have
// a model go behind one another into ONE call (a shorter list is "no model" without a device, as estimate() has it), the
// left positions are gathered once, every other object's once
std::vector<HomographyEstimate> FeaturesDev::estimateMany( const char* who, RansacModel model, const std::vector<FeaturesDev*>& others,
                                                           const std::vector<std::vector<Match>>& matches, const RansacOptions& opts )
{
    if( others.size() != matches.size() ) {
        std::ostringstream ss;
        ss << who << ": " << others.size() << " objects but " << matches.size() << " match lists";
        fatal( __FILE__, __LINE__, ss.str() );
    }
    for( FeaturesDev* o : others ) {
        if( o == nullptr ) fatal( __FILE__, __LINE__, std::string( who ) + ": null argument" );
        if( o->_device != _device ) {
            std::ostringstream ss;
            ss << who << ": the objects live on different devices (" << _device << " and " << o->_device << ")";
            fatal( __FILE__, __LINE__, ss.str() );
        }
    }
    if( !( std::isfinite( opts.tol ) && opts.tol >= 0.0f ) || opts.hypotheses < 1 || opts.hypotheses > 65536 )
        fatal( __FILE__, __LINE__, std::string( who ) + ": invalid options (finite tolerance >= 0, 1 to 65536 hypotheses)" );
    const int K = (int)others.size();
    const int min_pairs = ransac_models[model].min_pairs;
    HomographyEstimate none;
    none.guide.kind = model == ModelFundamental ? MatchGuide::Epipolar : MatchGuide::Homography;
    for( int k = 0; k < 9; k++ ) none.guide.m[k] = 0.0f;
    none.guide.tol = opts.tol;
    none.best = -1; none.sample_inliers = 0; none.refit_kept = false;
    std::vector<HomographyEstimate> out( others.size(), none );
    std::vector<int> counts( K, 0 ), lens( K, 0 );
    size_t total = 0;
    for( int k = 0; k < K; k++ )
        if( (int)matches[k].size() >= min_pairs ) { counts[k] = (int)matches[k].size(); total += matches[k].size(); }
    if( total == 0 ) return out;
    // the record is copied whole: its distance slots carry the index of the match within its list
    std::vector<psx_match_pair_u8> rec( total ), inl( total );
    size_t at = 0;
    for( int k = 0; k < K; k++ )
        for( int q = 0; q < counts[k]; q++, at++ ) {
            rec[at].left = matches[k][q].left_descriptor; rec[at].right = matches[k][q].right_descriptor; rec[at].d1 = q; rec[at].d2 = 0;
        }
    psx_ransac_opts po;
    po.tol = opts.tol; po.hypotheses = opts.hypotheses; po.seed = opts.seed; po.flags = opts.refit ? PSX_RANSAC_REFIT : 0;
    std::vector<psx_ransac_result> res( K );
    std::vector<void*> bufs( (size_t)K + 1, nullptr );
    std::vector<const float*> rxys( K, nullptr );
    const int l_len = getDescriptorCount();
    int count = 0;
    int rc = l_len > 0 ? PSX_OK : PSX_ERR_INVALID;
    if( rc == PSX_OK ) rc = psx_dev_alloc( _device, (size_t)l_len * 2 * sizeof(float), &bufs[K] );
    if( rc == PSX_OK ) rc = psx_desc_positions( _device, (const psx_feature_dev*)_ext, _rev, l_len, (float*)bufs[K] );
    for( int k = 0; k < K && rc == PSX_OK; k++ ) {
        const int r_len = others[k]->getDescriptorCount();
        if( counts[k] == 0 ) continue;
        if( r_len <= 0 ) { rc = PSX_ERR_INVALID; break; }
        lens[k] = r_len;
        rc = psx_dev_alloc( _device, (size_t)r_len * 2 * sizeof(float), &bufs[k] );
        if( rc == PSX_OK ) rc = psx_desc_positions( _device, (const psx_feature_dev*)others[k]->_ext, others[k]->_rev, r_len, (float*)bufs[k] );
        rxys[k] = (const float*)bufs[k];
    }
    if( rc == PSX_OK )
        rc = ransac_models[model].many( _device, rec.data(), counts.data(), K, (const float*)bufs[K], l_len, rxys.data(), lens.data(), &po, res.data(),
                                        inl.data(), (int)total, &count, nullptr, nullptr );
    for( void* b : bufs ) psx_dev_free( _device, b );
    if( rc != PSX_OK ) {
        std::ostringstream ss;
        ss << who << " failed (" << rc << ( rc == PSX_ERR_INVALID ? ": invalid options or a descriptor index outside its object" : "" ) << ")";
        fatal( __FILE__, __LINE__, ss.str() );
    }
    at = 0;
    for( int k = 0; k < K; k++ ) {
        if( counts[k] == 0 ) continue;
        HomographyEstimate& est = out[k];
        for( int j = 0; j < 9; j++ ) est.guide.m[j] = res[k].m[j];
        est.best = res[k].best; est.sample_inliers = res[k].sample_inliers; est.refit_kept = res[k].refit_kept != 0;
        est.inliers.reserve( res[k].inliers );
        for( int q = 0; q < res[k].inliers; q++, at++ ) est.inliers.push_back( matches[k][inl[at].d1] );
    }
    return out;
}

namespace {
typedef int (*RansacGraphFn)( int, const void*, const int*, const psx_view_edge*, int, const float* const*, const int*, int, const psx_ransac_opts*,
                              psx_ransac_result*, void*, int, int*, float*, int* );
const RansacGraphFn ransac_graph_models[4] = { psx_ransac_homography_graph, psx_ransac_fundamental_graph, psx_ransac_affine_graph,
                                               psx_ransac_similarity_graph };

// what the edge-list forms refuse about their views and edges, as matchPairsGraph does: an edge index outside `views`, a
// null view that an edge names, named views on different devices.  Returns the device of the named views (-1: no edge).
int graph_views_device( const char* who, const std::vector<FeaturesDev*>& views, const std::vector<std::pair<int,int>>& edges,
                        int (*device_of)( FeaturesDev* ) )
{
    const int N = (int)views.size();
    std::vector<char> named( views.size(), 0 );
    for( const std::pair<int,int>& e : edges ) {
        if( e.first < 0 || e.first >= N || e.second < 0 || e.second >= N ) {
            std::ostringstream ss;
            ss << who << ": edge (" << e.first << ", " << e.second << ") out of range (" << N << " views)";
            fatal( __FILE__, __LINE__, ss.str() );
        }
        named[e.first] = named[e.second] = 1;
    }
    int device = -1;
    for( int v = 0; v < N; v++ ) {
        if( !named[v] ) continue;
        if( views[v] == nullptr ) fatal( __FILE__, __LINE__, std::string( who ) + ": null argument" );
        if( device < 0 ) device = device_of( views[v] );
        if( device_of( views[v] ) != device ) {
            std::ostringstream ss;
            ss << who << ": the objects live on different devices (" << device << " and " << device_of( views[v] ) << ")";
            fatal( __FILE__, __LINE__, ss.str() );
        }
    }
    return device;
}
}

std::vector<HomographyEstimate> FeaturesDev::estimateHomographyGraph( const std::vector<FeaturesDev*>& views, const std::vector<std::pair<int,int>>& edges,
                                                                      const std::vector<std::vector<Match>>& matches, const RansacOptions& opts )
{
    return estimateGraph( "FeaturesDev::estimateHomographyGraph", ModelHomography, views, edges, matches, opts );
}

std::vector<FundamentalEstimate> FeaturesDev::estimateFundamentalGraph( const std::vector<FeaturesDev*>& views, const std::vector<std::pair<int,int>>& edges,
                                                                        const std::vector<std::vector<Match>>& matches, const RansacOptions& opts )
{
    return estimateGraph( "FeaturesDev::estimateFundamentalGraph", ModelFundamental, views, edges, matches, opts );
}

std::vector<HomographyEstimate> FeaturesDev::estimateAffineGraph( const std::vector<FeaturesDev*>& views, const std::vector<std::pair<int,int>>& edges,
                                                                  const std::vector<std::vector<Match>>& matches, const RansacOptions& opts )
{
    return estimateGraph( "FeaturesDev::estimateAffineGraph", ModelAffine, views, edges, matches, opts );
}

std::vector<HomographyEstimate> FeaturesDev::estimateSimilarityGraph( const std::vector<FeaturesDev*>& views, const std::vector<std::pair<int,int>>& edges,
                                                                      const std::vector<std::vector<Match>>& matches, const RansacOptions& opts )
{
    return estimateGraph( "FeaturesDev::estimateSimilarityGraph", ModelSimilarity, views, edges, matches, opts );
}

// psx_ransac_homography_graph / _fundamental_graph / _affine_graph / _similarity_graph on the lists matchPairsGraph returned:
// the lists that can have a model go behind one another into ONE call (a shorter list is "no model" without a device, as
// estimate() has it), the positions of every view such an edge names are gathered once
std::vector<HomographyEstimate> FeaturesDev::estimateGraph( const char* who, RansacModel model, const std::vector<FeaturesDev*>& views,
                                                            const std::vector<std::pair<int,int>>& edges,
                                                            const std::vector<std::vector<Match>>& matches, const RansacOptions& opts )
{
    if( edges.size() != matches.size() ) {
        std::ostringstream ss;
        ss << who << ": " << edges.size() << " edges but " << matches.size() << " match lists";
        fatal( __FILE__, __LINE__, ss.str() );
    }
    const int device = graph_views_device( who, views, edges, []( FeaturesDev* f ) { return f->_device; } );
    if( !( std::isfinite( opts.tol ) && opts.tol >= 0.0f ) || opts.hypotheses < 1 || opts.hypotheses > 65536 )
        fatal( __FILE__, __LINE__, std::string( who ) + ": invalid options (finite tolerance >= 0, 1 to 65536 hypotheses)" );
    const int N = (int)views.size(), E = (int)edges.size();
    const int min_pairs = ransac_models[model].min_pairs;
    HomographyEstimate none;
    none.guide.kind = model == ModelFundamental ? MatchGuide::Epipolar : MatchGuide::Homography;
    for( int k = 0; k < 9; k++ ) none.guide.m[k] = 0.0f;
    none.guide.tol = opts.tol;
    none.best = -1; none.sample_inliers = 0; none.refit_kept = false;
    std::vector<HomographyEstimate> out( edges.size(), none );
    std::vector<int> counts( edges.size(), 0 ), lens( views.size(), 0 );
    std::vector<char> used( views.size(), 0 );               // named by an edge that has a model to estimate
    size_t total = 0;
    for( int e = 0; e < E; e++ )
        if( (int)matches[e].size() >= min_pairs ) {
            counts[e] = (int)matches[e].size(); total += matches[e].size();
            used[edges[e].first] = used[edges[e].second] = 1;
        }
    if( total == 0 ) return out;
    // the record is copied whole: its distance slots carry the index of the match within its list
    std::vector<psx_match_pair_u8> rec( total ), inl( total );
    size_t at = 0;
    for( int e = 0; e < E; e++ )
        for( int q = 0; q < counts[e]; q++, at++ ) {
            rec[at].left = matches[e][q].left_descriptor; rec[at].right = matches[e][q].right_descriptor; rec[at].d1 = q; rec[at].d2 = 0;
        }
    psx_ransac_opts po;
    po.tol = opts.tol; po.hypotheses = opts.hypotheses; po.seed = opts.seed; po.flags = opts.refit ? PSX_RANSAC_REFIT : 0;
    std::vector<psx_view_edge> pe( edges.size() );
    for( int e = 0; e < E; e++ ) { pe[e].left = edges[e].first; pe[e].right = edges[e].second; }
    std::vector<psx_ransac_result> res( edges.size() );
    std::vector<void*> bufs( views.size(), nullptr );
    std::vector<const float*> xys( views.size(), nullptr );
    int count = 0;
    int rc = PSX_OK;
    for( int v = 0; v < N && rc == PSX_OK; v++ ) {
        if( !used[v] ) continue;
        const int len = views[v]->getDescriptorCount();
        if( len <= 0 ) { rc = PSX_ERR_INVALID; break; }
        lens[v] = len;
        rc = psx_dev_alloc( device, (size_t)len * 2 * sizeof(float), &bufs[v] );
        if( rc == PSX_OK ) rc = psx_desc_positions( device, (const psx_feature_dev*)views[v]->_ext, views[v]->_rev, len, (float*)bufs[v] );
        xys[v] = (const float*)bufs[v];
    }
    if( rc == PSX_OK )
        rc = ransac_graph_models[model]( device, rec.data(), counts.data(), pe.data(), E, xys.data(), lens.data(), N, &po, res.data(), inl.data(),
                                         (int)total, &count, nullptr, nullptr );
    for( void* b : bufs ) psx_dev_free( device, b );
    if( rc != PSX_OK ) {
        std::ostringstream ss;
        ss << who << " failed (" << rc << ( rc == PSX_ERR_INVALID ? ": invalid options or a descriptor index outside its object" : "" ) << ")";
        fatal( __FILE__, __LINE__, ss.str() );
    }
    at = 0;
    for( int e = 0; e < E; e++ ) {
        if( counts[e] == 0 ) continue;
        HomographyEstimate& est = out[e];
        for( int j = 0; j < 9; j++ ) est.guide.m[j] = res[e].m[j];
        est.best = res[e].best; est.sample_inliers = res[e].sample_inliers; est.refit_kept = res[e].refit_kept != 0;
        est.inliers.reserve( res[e].inliers );
        for( int q = 0; q < res[e].inliers; q++, at++ ) est.inliers.push_back( matches[e][inl[at].d1] );
    }
    return out;
}

// FeaturesDev::buildTracks: psx_tracks_graph on the descriptor indices of the lists, at the capacities no result can exceed
Tracks FeaturesDev::buildTracks( const std::vector<FeaturesDev*>& views, const std::vector<std::pair<int,int>>& edges,
                                 const std::vector<std::vector<Match>>& matches, const TrackOptions& opts )
{
    const char* who = "FeaturesDev::buildTracks";
    if( edges.size() != matches.size() ) {
        std::ostringstream ss;
        ss << who << ": " << edges.size() << " edges but " << matches.size() << " match lists";
        fatal( __FILE__, __LINE__, ss.str() );
    }
    int device = graph_views_device( who, views, edges, []( FeaturesDev* f ) { return f->_device; } );
    if( opts.min_views < 2 ) fatal( __FILE__, __LINE__, std::string( who ) + ": invalid options (min_views >= 2)" );
    if( device < 0 ) device = 0;                             // no edge: the call touches no device
    const int N = (int)views.size(), E = (int)edges.size();
    std::vector<int> counts( edges.size(), 0 ), lens( views.size(), 0 );
    Tracks out;
    out.view_offsets.assign( views.size() + 1, 0 );
    for( int v = 0; v < N; v++ ) {
        lens[v] = views[v] != nullptr ? views[v]->getDescriptorCount() : 0;
        out.view_offsets[v + 1] = out.view_offsets[v] + lens[v];
    }
    const int M = out.view_offsets[N];
    size_t total = 0;
    for( int e = 0; e < E; e++ ) { counts[e] = (int)matches[e].size(); total += matches[e].size(); }
    std::vector<psx_match_pair_u8> rec( total );
    size_t at = 0;
    for( int e = 0; e < E; e++ )
        for( const Match& m : matches[e] ) {
            rec[at].left = m.left_descriptor; rec[at].right = m.right_descriptor; rec[at].d1 = 0; rec[at].d2 = 0;
            at++;
        }
    std::vector<psx_view_edge> pe( edges.size() );
    for( int e = 0; e < E; e++ ) { pe[e].left = edges[e].first; pe[e].right = edges[e].second; }
    psx_track_opts po;
    po.min_views = opts.min_views; po.flags = opts.keep_conflicts ? PSX_TRACKS_KEEP_CONFLICTS : 0;
    std::vector<psx_track_member> mem( (size_t)M );
    out.labels.assign( (size_t)M, -1 );
    out.starts.assign( (size_t)M / 2 + 1, 0 );
    psx_tracks_info info;
    const int rc = psx_tracks_graph( device, rec.data(), counts.data(), pe.data(), E, lens.data(), N, &po, out.labels.data(), out.starts.data(),
                                     M / 2, mem.data(), M, &info );
    if( rc != PSX_OK ) {
        std::ostringstream ss;
        ss << who << " failed (" << rc << ( rc == PSX_ERR_INVALID ? ": a descriptor index outside its object" : "" ) << ")";
        fatal( __FILE__, __LINE__, ss.str() );
    }
    out.starts.resize( (size_t)info.tracks + 1 );
    out.members.resize( (size_t)info.members );
    for( int i = 0; i < info.members; i++ ) { out.members[i].view = mem[i].view; out.members[i].descriptor = mem[i].row; }
    out.n_tracks = info.tracks; out.n_members = info.members; out.components = info.components; out.conflicts = info.conflicts;
    out.too_few_views = info.too_few_views; out.joined_records = info.joined_records;
    return out;
}

// FeaturesDev::matchPairsGuidedGraph: psx_match_pairs_guided_graph_u8 on the bytes and positions of every view that an edge
// names which is neither skipped nor has an empty side -- each quantised and its positions gathered once, ONE matching
// call for all edges; the concatenated list is cut at the per-edge counts and mapped through the two views' reverse maps
std::vector<std::vector<Match>> FeaturesDev::matchPairsGuidedGraph( const std::vector<FeaturesDev*>& views, const std::vector<std::pair<int,int>>& edges,
                                                                    const std::vector<MatchGuide>& guides, const MatchOptions& opts )
{
    const char* who = "FeaturesDev::matchPairsGuidedGraph";
    const int device = graph_views_device( who, views, edges, []( FeaturesDev* f ) { return f->_device; } );
    if( !opts.bytes ) fatal( __FILE__, __LINE__, std::string( who ) + ": the edge-list form is byte-only (set MatchOptions::bytes)" );
    if( guides.size() != edges.size() ) {
        std::ostringstream ss;
        ss << who << ": " << edges.size() << " edges but " << guides.size() << " guides";
        fatal( __FILE__, __LINE__, ss.str() );
    }
    const int N = (int)views.size(), E = (int)edges.size();
    std::vector<psx_guide> pg( edges.size() );
    for( int e = 0; e < E; e++ ) {
        pg[e].kind = (int)guides[e].kind;
        for( int q = 0; q < 9; q++ ) pg[e].m[q] = guides[e].m[q];
        pg[e].tol = guides[e].tol;
        if( pg[e].kind == PSX_GUIDE_NONE ) continue;
        // refused here, before any device is touched (and for empty sides too): what the call refuses
        bool ok = ( pg[e].kind == PSX_GUIDE_HOMOGRAPHY || pg[e].kind == PSX_GUIDE_EPIPOLAR ) && std::isfinite( pg[e].tol ) && pg[e].tol >= 0.0f;
        for( int q = 0; q < 9; q++ ) ok = ok && std::isfinite( pg[e].m[q] );
        if( !ok ) fatal( __FILE__, __LINE__, std::string( who ) + ": invalid guide (kind 0, 1 or 2, finite entries, finite tolerance >= 0)" );
    }
    std::vector<std::vector<Match>> out( edges.size() );
    std::vector<int> lens( views.size(), 0 );
    std::vector<char> used( views.size(), 0 );               // named by an edge that is not skipped and has two non-empty sides
    long long room = 0;                                      // at most lens[left] pairs per edge exist
    for( int e = 0; e < E; e++ ) {
        const int l = edges[e].first, r = edges[e].second;
        if( pg[e].kind == PSX_GUIDE_NONE || views[l]->getDescriptorCount() <= 0 || views[r]->getDescriptorCount() <= 0 ) continue;
        room += views[l]->getDescriptorCount();
        used[l] = used[r] = 1;
    }
    if( room == 0 ) return out;
    psx_match_opts po;
    po.ratio = opts.ratio;
    po.flags = opts.mutual ? PSX_PAIRS_MUTUAL : 0;
    // descriptors of view v at [v], its positions at [N + v]
    std::vector<void*> bufs( 2 * views.size(), nullptr );
    std::vector<const unsigned char*> ptrs( views.size(), nullptr );
    std::vector<const float*> xys( views.size(), nullptr );
    int rc = PSX_OK;
    for( int v = 0; v < N && rc == PSX_OK; v++ ) {
        if( !used[v] ) continue;                             // a view no live edge names is an empty set to the call
        const int len = lens[v] = views[v]->getDescriptorCount();
        rc = psx_dev_alloc( device, (size_t)len * 128, &bufs[v] );
        if( rc == PSX_OK ) rc = psx_dev_alloc( device, (size_t)len * 2 * sizeof(float), &bufs[N + v] );
        if( rc == PSX_OK ) rc = psx_quantize_desc( device, (const float*)views[v]->_ori, len, (unsigned char*)bufs[v] );
        if( rc == PSX_OK ) rc = psx_desc_positions( device, (const psx_feature_dev*)views[v]->_ext, views[v]->_rev, len, (float*)bufs[N + v] );
        ptrs[v] = (const unsigned char*)bufs[v];
        xys[v] = (const float*)bufs[N + v];
    }
    std::vector<psx_view_edge> pe( edges.size() );
    for( int e = 0; e < E; e++ ) { pe[e].left = edges[e].first; pe[e].right = edges[e].second; }
    std::vector<psx_match_pair_u8> pb( (size_t)( room < INT32_MAX ? room : INT32_MAX ) );
    std::vector<int> counts( edges.size(), 0 );
    int count = 0;
    if( rc == PSX_OK )
        rc = psx_match_pairs_guided_graph_u8( device, ptrs.data(), xys.data(), lens.data(), N, pe.data(), E, pg.data(), &po, pb.data(),
                                              (int)pb.size(), counts.data(), &count );
    for( void* b : bufs ) psx_dev_free( device, b );
    if( rc != PSX_OK ) {
        std::ostringstream ss;
        ss << who << " failed (" << rc << ( rc == PSX_ERR_INVALID ? ": invalid options" : "" ) << ")";
        fatal( __FILE__, __LINE__, ss.str() );
    }
    std::vector<std::vector<int>> fem( views.size() );       // every used view's reverse map, read once
    for( int v = 0; v < N; v++ ) {
        if( !used[v] ) continue;
        fem[v].resize( lens[v] );
        if( psx_dev_read( device, fem[v].data(), views[v]->_rev, (size_t)lens[v] * sizeof(int) ) != PSX_OK )
            fatal( __FILE__, __LINE__, std::string( who ) + ": reading the reverse maps failed" );
    }
    size_t at = 0;
    for( int e = 0; e < E; e++ ) {
        if( counts[e] <= 0 ) continue;
        const std::vector<int>& l_fem = fem[pe[e].left];
        const std::vector<int>& r_fem = fem[pe[e].right];
        out[e].resize( counts[e] );
        for( int q = 0; q < counts[e]; q++, at++ ) {
            Match& m = out[e][q];
            m.left_descriptor = pb[at].left; m.right_descriptor = pb[at].right;
            m.distance        = pb[at].d1 == INT32_MAX ? INFINITY : (float)pb[at].d1;
            m.second_distance = pb[at].d2 == INT32_MAX ? INFINITY : (float)pb[at].d2;
            m.left_feature  = l_fem[m.left_descriptor];
            m.right_feature = r_fem[m.right_descriptor];
        }
    }
    return out;
}

// ---- the float forms of the edge-list calls and of the batched guided calls -------------------------------------------------
namespace {

// the guides as the library takes them; refuses, before any device is touched (and for empty sides too), what the calls refuse
std::vector<psx_guide> float_guides( const char* who, const std::vector<MatchGuide>& guides )
{
    std::vector<psx_guide> pg( guides.size() );
    for( size_t e = 0; e < guides.size(); e++ ) {
        pg[e].kind = (int)guides[e].kind;
        for( int q = 0; q < 9; q++ ) pg[e].m[q] = guides[e].m[q];
        pg[e].tol = guides[e].tol;
        if( pg[e].kind == PSX_GUIDE_NONE ) continue;
        bool ok = ( pg[e].kind == PSX_GUIDE_HOMOGRAPHY || pg[e].kind == PSX_GUIDE_EPIPOLAR ) && std::isfinite( pg[e].tol ) && pg[e].tol >= 0.0f;
        for( int q = 0; q < 9; q++ ) ok = ok && std::isfinite( pg[e].m[q] );
        if( !ok ) fatal( __FILE__, __LINE__, std::string( who ) + ": invalid guide (kind 0, 1 or 2, finite entries, finite tolerance >= 0)" );
    }
    return pg;
}

// the concatenated float records of an edge-list call, cut at the per-edge counts and mapped through the two views'
// reverse maps (fem[v]: view v's, read by the caller for every view a counted edge names)
std::vector<std::vector<Match>> float_lists( const std::vector<psx_match_pair>& pf, const std::vector<int>& counts, const std::vector<psx_view_edge>& pe,
                                             const std::vector<std::vector<int>>& fem )
{
    std::vector<std::vector<Match>> out( counts.size() );
    size_t at = 0;
    for( size_t e = 0; e < counts.size(); e++ ) {
        if( counts[e] <= 0 ) continue;
        const std::vector<int>& l_fem = fem[pe[e].left];
        const std::vector<int>& r_fem = fem[pe[e].right];
        out[e].resize( counts[e] );
        for( int q = 0; q < counts[e]; q++, at++ ) {
            Match& m = out[e][q];
            m.left_descriptor = pf[at].left; m.right_descriptor = pf[at].right;
            m.distance = pf[at].d1; m.second_distance = pf[at].d2;
            m.left_feature  = l_fem[m.left_descriptor];
            m.right_feature = r_fem[m.right_descriptor];
        }
    }
    return out;
}

}

// Both edge-list float forms: psx_match_pairs_graph (guides == nullptr) or psx_match_pairs_guided_graph on the views' own
// float descriptors -- nothing is quantised, no descriptor is copied; the guided form gathers every used view's positions once
std::vector<std::vector<Match>> FeaturesDev::matchGraphFloat( const char* who, const std::vector<FeaturesDev*>& views,
                                                              const std::vector<std::pair<int,int>>& edges, const std::vector<MatchGuide>* guides,
                                                              const MatchOptions& opts )
{
    const int device = graph_views_device( who, views, edges, []( FeaturesDev* f ) { return f->_device; } );
    if( opts.bytes ) fatal( __FILE__, __LINE__, std::string( who ) + ": float descriptors only (use the byte form for MatchOptions::bytes)" );
    if( guides && guides->size() != edges.size() ) {
        std::ostringstream ss;
        ss << who << ": " << edges.size() << " edges but " << guides->size() << " guides";
        fatal( __FILE__, __LINE__, ss.str() );
    }
    const int N = (int)views.size(), E = (int)edges.size();
    std::vector<psx_guide> pg;
    if( guides ) pg = float_guides( who, *guides );
    std::vector<std::vector<Match>> out( edges.size() );
    std::vector<int> lens( views.size(), 0 );
    std::vector<char> used( views.size(), 0 );               // named by an edge that is not skipped and has two non-empty sides
    long long room = 0;                                      // at most lens[left] pairs per edge exist
    for( int e = 0; e < E; e++ ) {
        const int l = edges[e].first, r = edges[e].second;
        if( ( guides && pg[e].kind == PSX_GUIDE_NONE ) || views[l]->getDescriptorCount() <= 0 || views[r]->getDescriptorCount() <= 0 ) continue;
        room += views[l]->getDescriptorCount();
        used[l] = used[r] = 1;
    }
    if( room == 0 ) return out;
    psx_match_opts po;
    po.ratio = opts.ratio;
    po.flags = opts.mutual ? PSX_PAIRS_MUTUAL : 0;
    std::vector<void*> bufs( views.size(), nullptr );        // the guided form: view v's positions
    std::vector<const float*> ptrs( views.size(), nullptr ), xys( views.size(), nullptr );
    int rc = PSX_OK;
    for( int v = 0; v < N && rc == PSX_OK; v++ ) {
        if( !used[v] ) continue;                             // a view no live edge names is an empty set to the call
        const int len = lens[v] = views[v]->getDescriptorCount();
        ptrs[v] = (const float*)views[v]->_ori;
        if( !guides ) continue;
        rc = psx_dev_alloc( device, (size_t)len * 2 * sizeof(float), &bufs[v] );
        if( rc == PSX_OK ) rc = psx_desc_positions( device, (const psx_feature_dev*)views[v]->_ext, views[v]->_rev, len, (float*)bufs[v] );
        xys[v] = (const float*)bufs[v];
    }
    std::vector<psx_view_edge> pe( edges.size() );
    for( int e = 0; e < E; e++ ) { pe[e].left = edges[e].first; pe[e].right = edges[e].second; }
    std::vector<psx_match_pair> pf( (size_t)( room < INT32_MAX ? room : INT32_MAX ) );
    std::vector<int> counts( edges.size(), 0 );
    int count = 0;
    if( rc == PSX_OK )
        rc = guides ? psx_match_pairs_guided_graph( device, ptrs.data(), xys.data(), lens.data(), N, pe.data(), E, pg.data(), &po, pf.data(),
                                                    (int)pf.size(), counts.data(), &count )
                    : psx_match_pairs_graph( device, ptrs.data(), lens.data(), N, pe.data(), E, &po, pf.data(), (int)pf.size(), counts.data(), &count );
    for( void* b : bufs ) psx_dev_free( device, b );
    if( rc != PSX_OK ) {
        std::ostringstream ss;
        ss << who << " failed (" << rc << ( rc == PSX_ERR_INVALID ? ": invalid options" : "" ) << ")";
        fatal( __FILE__, __LINE__, ss.str() );
    }
    std::vector<std::vector<int>> fem( views.size() );       // every used view's reverse map, read once
    for( int v = 0; v < N; v++ ) {
        if( !used[v] ) continue;
        fem[v].resize( lens[v] );
        if( psx_dev_read( device, fem[v].data(), views[v]->_rev, (size_t)lens[v] * sizeof(int) ) != PSX_OK )
            fatal( __FILE__, __LINE__, std::string( who ) + ": reading the reverse maps failed" );
    }
    return float_lists( pf, counts, pe, fem );
}

std::vector<std::vector<Match>> FeaturesDev::matchPairsGraphFloat( const std::vector<FeaturesDev*>& views, const std::vector<std::pair<int,int>>& edges,
                                                                   const MatchOptions& opts )
{
    return matchGraphFloat( "FeaturesDev::matchPairsGraphFloat", views, edges, nullptr, opts );
}

std::vector<std::vector<Match>> FeaturesDev::matchPairsGuidedGraphFloat( const std::vector<FeaturesDev*>& views,
                                                                         const std::vector<std::pair<int,int>>& edges,
                                                                         const std::vector<MatchGuide>& guides, const MatchOptions& opts )
{
    return matchGraphFloat( "FeaturesDev::matchPairsGuidedGraphFloat", views, edges, &guides, opts );
}

// FeaturesDev::matchPairsGuidedManyFloat: psx_match_pairs_guided_many on this object's float descriptors and every other
// object's that is neither empty nor skipped -- no quantisation, no descriptor copies, every side's positions gathered once
std::vector<std::vector<Match>> FeaturesDev::matchPairsGuidedManyFloat( const std::vector<FeaturesDev*>& others, const std::vector<MatchGuide>& guides,
                                                                        const MatchOptions& opts )
{
    const char* who = "FeaturesDev::matchPairsGuidedManyFloat";
    for( FeaturesDev* o : others ) {
        if( o == nullptr ) fatal( __FILE__, __LINE__, std::string( who ) + ": null argument" );
        if( o->_device != _device ) {
            std::ostringstream ss;
            ss << who << ": the objects live on different devices (" << _device << " and " << o->_device << ")";
            fatal( __FILE__, __LINE__, ss.str() );
        }
    }
    if( opts.bytes ) fatal( __FILE__, __LINE__, std::string( who ) + ": float descriptors only (use matchPairsGuidedMany for MatchOptions::bytes)" );
    if( guides.size() != others.size() ) {
        std::ostringstream ss;
        ss << who << ": " << others.size() << " objects but " << guides.size() << " guides";
        fatal( __FILE__, __LINE__, ss.str() );
    }
    const int K = (int)others.size();
    const std::vector<psx_guide> pg = float_guides( who, guides );
    const int l_len = getDescriptorCount();
    std::vector<std::vector<Match>> out( others.size() );
    std::vector<int> lens( K, 0 ), counts( K, 0 );
    bool any = false;
    for( int k = 0; k < K; k++ ) {
        if( pg[k].kind != PSX_GUIDE_NONE && others[k]->getDescriptorCount() > 0 ) lens[k] = others[k]->getDescriptorCount();
        any = any || lens[k] > 0;
    }
    if( l_len <= 0 || !any ) return out;
    psx_match_opts po;
    po.ratio = opts.ratio;
    po.flags = opts.mutual ? PSX_PAIRS_MUTUAL : 0;
    // the positions of set k at [k], this object's at [K]
    std::vector<void*> bufs( (size_t)K + 1, nullptr );
    std::vector<const float*> ptrs( K, nullptr ), xys( K, nullptr );
    int rc = psx_dev_alloc( _device, (size_t)l_len * 2 * sizeof(float), &bufs[K] );
    if( rc == PSX_OK ) rc = psx_desc_positions( _device, (const psx_feature_dev*)_ext, _rev, l_len, (float*)bufs[K] );
    for( int k = 0; k < K && rc == PSX_OK; k++ ) {
        const int r_len = lens[k];
        if( r_len <= 0 ) continue;
        rc = psx_dev_alloc( _device, (size_t)r_len * 2 * sizeof(float), &bufs[k] );
        if( rc == PSX_OK ) rc = psx_desc_positions( _device, (const psx_feature_dev*)others[k]->_ext, others[k]->_rev, r_len, (float*)bufs[k] );
        ptrs[k] = (const float*)others[k]->_ori;
        xys[k] = (const float*)bufs[k];
    }
    // at most l_len pairs per set exist (a product above INT_MAX is the call's to refuse)
    const long long room = (long long)K * l_len;
    std::vector<psx_match_pair> pf( (size_t)( room < INT32_MAX ? room : INT32_MAX ) );
    int count = 0;
    if( rc == PSX_OK )
        rc = psx_match_pairs_guided_many( _device, (const float*)_ori, (const float*)bufs[K], l_len, ptrs.data(), xys.data(), lens.data(), K,
                                          pg.data(), &po, pf.data(), (int)pf.size(), counts.data(), &count );
    for( void* b : bufs ) psx_dev_free( _device, b );
    if( rc != PSX_OK ) {
        std::ostringstream ss;
        ss << who << " failed (" << rc << ( rc == PSX_ERR_INVALID ? ": invalid options" : "" ) << ")";
        fatal( __FILE__, __LINE__, ss.str() );
    }
    // the star as an edge list over [others..., this]: set k is edge (K, k)
    std::vector<std::vector<int>> fem( (size_t)K + 1 );
    std::vector<psx_view_edge> pe( K );
    bool pairs = false;
    for( int k = 0; k < K; k++ ) {
        pe[k].left = K; pe[k].right = k;
        if( counts[k] <= 0 ) continue;
        pairs = true;
        fem[k].resize( lens[k] );
        if( psx_dev_read( _device, fem[k].data(), others[k]->_rev, (size_t)lens[k] * sizeof(int) ) != PSX_OK )
            fatal( __FILE__, __LINE__, std::string( who ) + ": reading the reverse maps failed" );
    }
    if( pairs ) {
        fem[K].resize( l_len );
        if( psx_dev_read( _device, fem[K].data(), _rev, (size_t)l_len * sizeof(int) ) != PSX_OK )
            fatal( __FILE__, __LINE__, std::string( who ) + ": reading the reverse maps failed" );
    }
    return float_lists( pf, counts, pe, fem );
}

} // namespace popsift
