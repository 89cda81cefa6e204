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

// ---- the matching, RANSAC and track wrappers: their host steps, each stated once --------------------------------------------
// Every form is VIEWS + EDGE LIST.  An edge-list call brings both; a star (this object against `others`) is
// views = [others..., this] with edges[k] = (K, k); one pair is the star of one.  One path serves them all: check (the
// number of guides or match lists, then edges and views, then the options, then the guides), find the views that live
// edges name, prepare those views' inputs in owned device buffers, make the ONE call of the form -- single, _many or
// _graph --, cut the records that come back at the per-edge counts.
namespace {

typedef std::vector<FeaturesDev*>       Views;
typedef std::vector<std::pair<int,int>> Edges;
typedef std::vector<std::vector<Match>> Lists;
enum Form { OnePair, Star, EdgeList };      // which entry point makes the final call: the single one, _many or _graph

Views star_views( FeaturesDev* centre, const Views& others ) { Views v( others ); v.push_back( centre ); return v; }
Edges star_edges( size_t K ) { Edges e( K ); for( size_t k = 0; k < K; k++ ) e[k] = std::make_pair( (int)K, (int)k ); return e; }
std::vector<const std::vector<Match>*> pointers( const Lists& lists )
{
    std::vector<const std::vector<Match>*> p;
    for( const std::vector<Match>& l : lists ) p.push_back( &l );
    return p;
}

[[noreturn]] void failed( const char* who, int rc, const char* invalid_means )
{
    std::ostringstream ss;
    ss << who << " failed (" << rc << ( rc == PSX_ERR_INVALID ? invalid_means : "" ) << ")";
    fatal( __FILE__, __LINE__, ss.str() );
}

// ---- options as the library takes them; what the calls would refuse is refused here, before any device is touched
psx_match_opts to_psx( const MatchOptions& o )
{
    psx_match_opts po;
    po.ratio = o.ratio;
    po.flags = o.mutual ? PSX_PAIRS_MUTUAL : 0;
    return po;
}
psx_ransac_opts to_psx( const char* who, const RansacOptions& o )
{
    if( !( std::isfinite( o.tol ) && o.tol >= 0.0f ) || o.hypotheses < 1 || o.hypotheses > 65536 )
        fatal( __FILE__, __LINE__, std::string( who ) + ": invalid options (finite tolerance >= 0, 1 to 65536 hypotheses)" );
    psx_ransac_opts po;
    po.tol = o.tol; po.hypotheses = o.hypotheses; po.seed = o.seed; po.flags = o.refit ? PSX_RANSAC_REFIT : 0;
    return po;
}
// batched: kind None is a set / an edge to skip, and is not looked at further
psx_guide to_psx( const char* who, const MatchGuide& g, bool batched )
{
    psx_guide pg;
    pg.kind = (int)g.kind;
    for( int k = 0; k < 9; k++ ) pg.m[k] = g.m[k];
    pg.tol = g.tol;
    if( batched && pg.kind == PSX_GUIDE_NONE ) return pg;
    bool ok = ( pg.kind == PSX_GUIDE_HOMOGRAPHY || pg.kind == PSX_GUIDE_EPIPOLAR ) && std::isfinite( pg.tol ) && pg.tol >= 0.0f;
    for( int k = 0; k < 9; k++ ) ok = ok && std::isfinite( pg.m[k] );
    if( !ok ) fatal( __FILE__, __LINE__, std::string( who ) + ": invalid guide (kind " + ( batched ? "0, 1 or 2" : "1 or 2" )
                                         + ", finite entries, finite tolerance >= 0)" );
    return pg;
}
std::vector<psx_view_edge> to_psx( const Edges& edges )
{
    std::vector<psx_view_edge> pe( edges.size() );
    for( size_t e = 0; e < edges.size(); e++ ) { pe[e].left = edges[e].first; pe[e].right = edges[e].second; }
    return pe;
}

// ---- the temporary device buffers of one wrapper call: freed when the call leaves, by return or by throw
class DevBufs
{
    const int          _device;
    std::vector<void*> _bufs;
public:
    explicit DevBufs( int device ) : _device( device ) { }
    DevBufs( const DevBufs& ) = delete;
    DevBufs& operator=( const DevBufs& ) = delete;
    ~DevBufs( ) { for( void* b : _bufs ) psx_dev_free( _device, b ); }
    int device( ) const { return _device; }
    int alloc( size_t bytes, void** out )
    {
        _bufs.reserve( _bufs.size() + 1 );       // before the allocation: nothing can throw between it and its registration
        const int rc = psx_dev_alloc( _device, bytes, out );
        if( rc == PSX_OK ) _bufs.push_back( *out );
        return rc;
    }
};

// ---- per-view inputs: a view's descriptors as the matcher of D reads them -- quantised into an owned buffer, or its own floats
int descriptors_of( DevBufs& bufs, FeaturesDev* f, int len, const unsigned char** out )
{
    void* b = nullptr;
    int rc = bufs.alloc( (size_t)len * 128, &b );
    if( rc == PSX_OK ) rc = psx_quantize_desc( bufs.device(), (const float*)f->getDescriptors(), len, (unsigned char*)b );
    *out = (const unsigned char*)b;
    return rc;
}
int descriptors_of( DevBufs&, FeaturesDev* f, int, const float** out ) { *out = (const float*)f->getDescriptors(); return PSX_OK; }

// what the call needs of every used view, at the view's index: its length, its descriptors (ptrs == nullptr: none) and, where
// asked for, the positions of its descriptors.  A view that is not used stays an empty set to the call and costs nothing.
template<class D>
int prepare( const Views& views, const std::vector<char>& used, bool positions, DevBufs& bufs, std::vector<const D*>* ptrs,
             std::vector<const float*>& xys, std::vector<int>& lens )
{
    int rc = PSX_OK;
    for( size_t v = 0; v < views.size() && rc == PSX_OK; v++ ) {
        if( !used[v] ) continue;
        const int len = views[v]->getDescriptorCount();
        if( len <= 0 ) return PSX_ERR_INVALID;       // a match list on an empty object (no live edge of a matching call names one)
        lens[v] = len;
        if( ptrs ) rc = descriptors_of( bufs, views[v], len, &(*ptrs)[v] );
        if( !positions ) continue;
        void* xy = nullptr;
        if( rc == PSX_OK ) rc = bufs.alloc( (size_t)len * 2 * sizeof(float), &xy );
        if( rc == PSX_OK ) rc = psx_desc_positions( bufs.device(), (const psx_feature_dev*)views[v]->getFeatures(), views[v]->getReverseMap(), len, (float*)xy );
        xys[v] = (const float*)xy;
    }
    return rc;
}

// a view's reverse map (descriptor -> feature) on the host
bool read_reverse_map( int device, FeaturesDev* f, std::vector<int>& fem )
{
    fem.resize( f->getDescriptorCount() > 0 ? f->getDescriptorCount() : 0 );
    return fem.empty() || psx_dev_read( device, fem.data(), f->getReverseMap(), fem.size() * sizeof(int) ) == PSX_OK;
}

// ---- lists out: a record as a Match (the feature indices follow from the reverse maps); byte distances convert exactly
float byte_distance( int d ) { return d == INT32_MAX ? INFINITY : (float)d; }
void to_match( const psx_match_pair& p, Match& m )    { m.left_descriptor = p.left; m.right_descriptor = p.right; m.distance = p.d1; m.second_distance = p.d2; }
void to_match( const psx_match_pair_u8& p, Match& m ) { m.left_descriptor = p.left; m.right_descriptor = p.right;
                                                        m.distance = byte_distance( p.d1 ); m.second_distance = byte_distance( p.d2 ); }

// the concatenated records of a call, cut at the per-edge counts and mapped through the two views' reverse maps; the map
// of every view that an edge with pairs names is read once
template<class P>
Lists lists_out( const char* who, int device, const Views& views, const Edges& edges, const std::vector<int>& counts, const std::vector<P>& pairs )
{
    Lists out( edges.size() );
    std::vector<std::vector<int>> fem( views.size() );
    size_t at = 0;
    for( size_t e = 0; e < edges.size(); e++ ) {
        if( counts[e] <= 0 ) continue;
        const int side[2] = { edges[e].first, edges[e].second };
        for( int v : side )
            if( fem[v].empty() && !read_reverse_map( device, views[v], fem[v] ) )
                fatal( __FILE__, __LINE__, std::string( who ) + ": reading the reverse maps failed" );
        out[e].resize( counts[e] );
        for( int q = 0; q < counts[e]; q++, at++ ) {
            Match& m = out[e][q];
            to_match( pairs[at], m );
            m.left_feature  = fem[side[0]][m.left_descriptor];
            m.right_feature = fem[side[1]][m.right_descriptor];
        }
    }
    return out;
}

// ---- the entry points of the two descriptor formats, by form
template<class D, class P> struct MatchFns
{
    int (*one)( int, const D*, int, const D*, int, const psx_match_opts*, P*, int, int* );
    int (*one_guided)( int, const D*, const float*, int, const D*, const float*, int, const psx_guide*, const psx_match_opts*, P*, int, int* );
    int (*many)( int, const D*, int, const D* const*, const int*, int, const psx_match_opts*, P*, int, int*, int* );
    int (*many_guided)( int, const D*, const float*, int, const D* const*, const float* const*, const int*, int, const psx_guide*,
                        const psx_match_opts*, P*, int, int*, int* );
    int (*graph)( int, const D* const*, const int*, int, const psx_view_edge*, int, const psx_match_opts*, P*, int, int*, int* );
    int (*graph_guided)( int, const D* const*, const float* const*, const int*, int, const psx_view_edge*, int, const psx_guide*,
                         const psx_match_opts*, P*, int, int*, int* );
};
const MatchFns<unsigned char, psx_match_pair_u8> byte_fns = { psx_match_pairs_u8, psx_match_pairs_guided_u8, psx_match_pairs_many_u8,
    psx_match_pairs_guided_many_u8, psx_match_pairs_graph_u8, psx_match_pairs_guided_graph_u8 };
const MatchFns<float, psx_match_pair> float_fns = { psx_match_pairs, psx_match_pairs_guided, psx_match_pairs_many,
    psx_match_pairs_guided_many, psx_match_pairs_graph, psx_match_pairs_guided_graph };

// Every matching wrapper, after the views are checked: the guides, the live edges (not skipped by a guide of kind None, two
// non-empty sides) and the views they name -- only these are quantised or gathered --, then ONE call.  A star and one pair
// pass their centre (the last view) as the left side and the views before it as the right sets.
template<class D, class P>
Lists match_lists( const MatchFns<D, P>& fn, const char* who, Form form, int device, const Views& views, const Edges& edges,
                   const std::vector<MatchGuide>* guides, const MatchOptions& opts )
{
    const int N = (int)views.size(), E = (int)edges.size(), C = N - 1;
    std::vector<psx_guide> pg;
    if( guides ) for( const MatchGuide& g : *guides ) pg.push_back( to_psx( who, g, form != OnePair ) );
    std::vector<char> used( views.size(), 0 );
    long long room = 0;                                      // at most lens[left] pairs per edge exist
    for( int e = 0; e < E; e++ ) {
        const int l = edges[e].first, r = edges[e].second;
        if( ( guides && pg[e].kind == PSX_GUIDE_NONE ) || views[l]->getDescriptorCount() <= 0 || views[r]->getDescriptorCount() <= 0 ) continue;
        room += views[l]->getDescriptorCount();
        used[l] = used[r] = 1;
    }
    if( room == 0 ) return Lists( edges.size() );
    // a star leaves room for every set (a product above INT_MAX is the call's to refuse)
    if( form != EdgeList ) room = (long long)E * views[C]->getDescriptorCount();
    const psx_match_opts po = to_psx( opts );
    const std::vector<psx_view_edge> pe = to_psx( edges );
    std::vector<const D*> ptrs( views.size(), nullptr );
    std::vector<const float*> xys( views.size(), nullptr );
    std::vector<int> lens( views.size(), 0 ), counts( edges.size(), 0 );
    std::vector<P> pairs( (size_t)( room < INT32_MAX ? room : INT32_MAX ) );
    const int capacity = (int)pairs.size();
    int count = 0;
    int rc;
    {
        DevBufs bufs( device );
        rc = prepare( views, used, guides != nullptr, bufs, &ptrs, xys, lens );
        if( rc != PSX_OK ) { }                               // a view could not be prepared: the call is not made
        else if( form == OnePair ) {
            rc = guides ? fn.one_guided( device, ptrs[C], xys[C], lens[C], ptrs[0], xys[0], lens[0], pg.data(), &po, pairs.data(), capacity, &count )
                        : fn.one( device, ptrs[C], lens[C], ptrs[0], lens[0], &po, pairs.data(), capacity, &count );
            counts[0] = count;
        }
        else if( form == Star )
            rc = guides ? fn.many_guided( device, ptrs[C], xys[C], lens[C], ptrs.data(), xys.data(), lens.data(), E, pg.data(), &po, pairs.data(),
                                          capacity, counts.data(), &count )
                        : fn.many( device, ptrs[C], lens[C], ptrs.data(), lens.data(), E, &po, pairs.data(), capacity, counts.data(), &count );
        else
            rc = guides ? fn.graph_guided( device, ptrs.data(), xys.data(), lens.data(), N, pe.data(), E, pg.data(), &po, pairs.data(), capacity,
                                           counts.data(), &count )
                        : fn.graph( device, ptrs.data(), lens.data(), N, pe.data(), E, &po, pairs.data(), capacity, counts.data(), &count );
    }
    if( rc != PSX_OK ) failed( who, rc, ": invalid options" );
    return lists_out( who, device, views, edges, counts, pairs );
}

// ---- RANSAC: what differs between the models, in the order of FeaturesDev::RansacModel
typedef int (*RansacOneFn)( int, const void*, int, const float*, int, const float*, int, const psx_ransac_opts*, psx_ransac_result*, void*, int, int*,
                            float*, int* );
typedef int (*RansacManyFn)( int, const void*, const int*, int, const float*, int, const float* const*, const int*, const psx_ransac_opts*,
                             psx_ransac_result*, void*, int, int*, float*, int* );
typedef int (*RansacGraphFn)( int, const void*, const int*, const psx_view_edge*, int, const float* const*, const int*, int, const psx_ransac_opts*,
                              psx_ransac_result*, void*, int, int*, float*, int* );
const struct { int min_pairs; MatchGuide::Kind guide; RansacOneFn one; RansacManyFn many; RansacGraphFn graph; } ransac_models[4] = {
    { 4, MatchGuide::Homography, psx_ransac_homography,  psx_ransac_homography_many,  psx_ransac_homography_graph },
    { 8, MatchGuide::Epipolar,   psx_ransac_fundamental, psx_ransac_fundamental_many, psx_ransac_fundamental_graph },
    { 3, MatchGuide::Homography, psx_ransac_affine,      psx_ransac_affine_many,      psx_ransac_affine_graph },
    { 2, MatchGuide::Homography, psx_ransac_similarity,  psx_ransac_similarity_many,  psx_ransac_similarity_graph },
};

// the lists with a count behind one another as the library's records; the record is copied whole, so with `index` its
// distance slots carry the index of the match within its list
std::vector<psx_match_pair_u8> pack_records( const std::vector<const std::vector<Match>*>& lists, const std::vector<int>& counts, bool index )
{
    size_t total = 0;
    for( int c : counts ) total += c;
    std::vector<psx_match_pair_u8> rec( total );
    size_t at = 0;
    for( size_t e = 0; e < lists.size(); e++ )
        for( int q = 0; q < counts[e]; q++, at++ ) {
            const Match& m = (*lists[e])[q];
            rec[at].left = m.left_descriptor; rec[at].right = m.right_descriptor; rec[at].d1 = index ? q : 0; rec[at].d2 = 0;
        }
    return rec;
}

// Every estimate*, after the views are checked: the lists that can have a model go behind one another into ONE call (a
// shorter list is "no model" without a device), the positions of every view such an edge names are gathered once
std::vector<HomographyEstimate> estimate_lists( const char* who, int model, Form form, int device, const Views& views, const Edges& edges,
                                                const std::vector<const std::vector<Match>*>& lists, const RansacOptions& opts )
{
    const psx_ransac_opts po = to_psx( who, opts );
    const int N = (int)views.size(), E = (int)edges.size(), C = N - 1;
    HomographyEstimate none;
    none.guide.kind = ransac_models[model].guide;
    for( int k = 0; k < 9; k++ ) none.guide.m[k] = 0.0f;
    none.guide.tol = opts.tol;
    none.best = -1; none.sample_inliers = 0; none.refit_kept = false;
    std::vector<HomographyEstimate> out( edges.size(), none );
    std::vector<int> counts( edges.size(), 0 );
    std::vector<char> used( views.size(), 0 );               // named by an edge that has a model to estimate
    for( int e = 0; e < E; e++ )
        if( (int)lists[e]->size() >= ransac_models[model].min_pairs ) {
            counts[e] = (int)lists[e]->size();
            used[edges[e].first] = used[edges[e].second] = 1;
        }
    const std::vector<psx_match_pair_u8> rec = pack_records( lists, counts, true );
    if( rec.empty() ) return out;
    std::vector<psx_match_pair_u8> inl( rec.size() );
    const std::vector<psx_view_edge> pe = to_psx( edges );
    std::vector<psx_ransac_result> res( edges.size() );
    std::vector<const float*> xys( views.size(), nullptr );
    std::vector<int> lens( views.size(), 0 );
    const int capacity = (int)inl.size();
    int count = 0;
    int rc;
    {
        DevBufs bufs( device );
        rc = prepare<float>( views, used, true, bufs, nullptr, xys, lens );
        if( rc != PSX_OK ) { }                               // a view could not be prepared: the call is not made
        else if( form == OnePair )
            rc = ransac_models[model].one( device, rec.data(), counts[0], xys[C], lens[C], xys[0], lens[0], &po, res.data(), inl.data(), capacity, &count,
                                           nullptr, nullptr );
        else if( form == Star )
            rc = ransac_models[model].many( device, rec.data(), counts.data(), E, xys[C], lens[C], xys.data(), lens.data(), &po, res.data(), inl.data(),
                                            capacity, &count, nullptr, nullptr );
        else
            rc = ransac_models[model].graph( device, rec.data(), counts.data(), pe.data(), E, xys.data(), lens.data(), N, &po, res.data(), inl.data(),
                                             capacity, &count, nullptr, nullptr );
    }
    if( rc != PSX_OK ) failed( who, rc, ": invalid options or a descriptor index outside its object" );
    size_t at = 0;
    for( int e = 0; e < E; e++ ) {
        if( counts[e] == 0 ) continue;
        HomographyEstimate& est = out[e];
        for( int j = 0; j < 9; j++ ) est.guide.m[j] = res[e].m[j];
        est.best = res[e].best; est.sample_inliers = res[e].sample_inliers; est.refit_kept = res[e].refit_kept != 0;
        est.inliers.reserve( res[e].inliers );
        for( int q = 0; q < res[e].inliers; q++, at++ ) est.inliers.push_back( (*lists[e])[inl[at].d1] );
    }
    return out;
}

// ---- match() and matchBytes(): one line per left descriptor, as the reference's show_distance prints them (features.cu:227-268)
bool print_matches( int l_device, FeaturesDev* l, int r_device, FeaturesDev* r, const std::vector<int>& mm, const std::vector<float>& dd )
{
    std::vector<int> l_fem, r_fem;
    if( !read_reverse_map( l_device, l, l_fem ) || !read_reverse_map( r_device, r, r_fem ) ) return false;
    for( int i = 0; i < (int)l_fem.size(); i++ )
    {
        const int m1 = mm[3*i], m2 = mm[3*i+1];
        printf( "%s feat %4d [%4d] matches feat %4d [%4d] ( 2nd feat %4d [%4d] ) dist %.3f vs %.3f\n",
                mm[3*i+2] ? "accept" : "reject",
                l_fem[i], i,
                r_fem.empty() ? 0 : r_fem[m1], m1,
                r_fem.empty() ? 0 : r_fem[m2], m2,
                dd[2*i], dd[2*i+1] );
    }
    return true;
}

} // namespace

// What every form refuses about its views and edges, in this order: a number of guides / match lists (`given`) other than
// one per edge, an edge index outside `views`, a null view that an edge names, named views on different devices.  Returns
// the device of the named views: a star's or a pair's is its centre's, an edge list without edges has none (-1).
int FeaturesDev::checkViews( const char* who, int form, const std::vector<FeaturesDev*>& views, const std::vector<std::pair<int,int>>& edges,
                             size_t given, const char* what )
{
    if( given != edges.size() ) {
        std::ostringstream ss;
        ss << who << ": " << edges.size() << ( form == EdgeList ? " edges but " : " objects but " ) << given << " " << what;
        fatal( __FILE__, __LINE__, ss.str() );
    }
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
    int device = form == EdgeList ? -1 : views.back()->_device;
    for( int v = 0; v < N; v++ ) {
        if( !named[v] ) continue;
        if( views[v] == nullptr ) fatal( __FILE__, __LINE__, std::string( who ) + ": null argument" );
        if( device < 0 ) device = views[v]->_device;
        if( views[v]->_device != device ) {
            std::ostringstream ss;
            ss << who << ": the " << ( form == OnePair ? "two " : "" ) << "objects live on different devices (" << device << " and " << views[v]->_device << ")";
            fatal( __FILE__, __LINE__, ss.str() );
        }
    }
    return device;
}

// Every matching wrapper: the checks in their one order, then the path of the descriptor format.  wrong_format: what to
// say when the form does not take opts.bytes as it is (nullptr: it does).
std::vector<std::vector<Match>> FeaturesDev::matchLists( const char* who, int form, const std::vector<FeaturesDev*>& views,
                                                         const std::vector<std::pair<int,int>>& edges, const std::vector<MatchGuide>* guides,
                                                         const MatchOptions& opts, const char* wrong_format )
{
    const int device = checkViews( who, form, views, edges, guides ? guides->size() : edges.size(), "guides" );
    if( wrong_format ) fatal( __FILE__, __LINE__, std::string( who ) + wrong_format );
    return opts.bytes ? match_lists( byte_fns, who, (Form)form, device, views, edges, guides, opts )
                      : match_lists( float_fns, who, (Form)form, device, views, edges, guides, opts );
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
    if( psx_match( _device, (const float*)_ori, l_len, (const float*)other->_ori, r_len, mm.data(), dd.data() ) != PSX_OK ||
        !print_matches( _device, this, other->_device, other, mm, dd ) )
        fatal( __FILE__, __LINE__, "FeaturesDev::match failed" );
}

// FeaturesDev::matchBytes: both descriptor sets quantised on the device with the byte rule, then psx_match_u8 (exact:
// the reference's result on the bytes, bit for bit); same lines as match(), the integer distances printed alike
void FeaturesDev::matchBytes( FeaturesDev* other )
{
    if( other == nullptr ) fatal( __FILE__, __LINE__, "FeaturesDev::matchBytes: null argument" );
    const int l_len = getDescriptorCount();
    const int r_len = other->getDescriptorCount();
    if( l_len <= 0 ) return;
    std::vector<int> mm( 3 * (size_t)l_len ), di( 2 * (size_t)l_len );
    std::vector<float> dd( 2 * (size_t)l_len );
    DevBufs bufs( _device );
    void *lb = nullptr, *rb = nullptr;
    const bool ok = bufs.alloc( (size_t)l_len * 128, &lb ) == PSX_OK &&
                    bufs.alloc( (size_t)( r_len > 0 ? r_len : 1 ) * 128, &rb ) == PSX_OK &&
                    psx_quantize_desc( _device, (const float*)_ori, l_len, (unsigned char*)lb ) == PSX_OK &&
                    psx_quantize_desc( _device, (const float*)other->_ori, r_len, (unsigned char*)rb ) == PSX_OK &&
                    psx_match_u8( _device, (const unsigned char*)lb, l_len, (const unsigned char*)rb, r_len, mm.data(), di.data() ) == PSX_OK;
    for( size_t i = 0; i < di.size(); i++ ) dd[i] = byte_distance( di[i] );
    if( !ok || !print_matches( _device, this, other->_device, other, mm, dd ) ) fatal( __FILE__, __LINE__, "FeaturesDev::matchBytes failed" );
}

// ---- matching: each public form names its views, its edges and what it takes
std::vector<Match> FeaturesDev::matchPairs( FeaturesDev* other, const MatchOptions& opts )
{
    return matchLists( "FeaturesDev::matchPairs", OnePair, star_views( this, Views( 1, other ) ), star_edges( 1 ), nullptr, opts, nullptr )[0];
}

std::vector<Match> FeaturesDev::matchPairsGuided( FeaturesDev* other, const MatchGuide& guide, const MatchOptions& opts )
{
    const std::vector<MatchGuide> guides( 1, guide );
    return matchLists( "FeaturesDev::matchPairsGuided", OnePair, star_views( this, Views( 1, other ) ), star_edges( 1 ), &guides, opts, nullptr )[0];
}

std::vector<std::vector<Match>> FeaturesDev::matchPairsMany( const std::vector<FeaturesDev*>& others, const MatchOptions& opts )
{
    return matchLists( "FeaturesDev::matchPairsMany", Star, star_views( this, others ), star_edges( others.size() ), nullptr, opts,
                       opts.bytes ? nullptr : ": the one-to-many form is byte-only (set MatchOptions::bytes)" );
}

std::vector<std::vector<Match>> FeaturesDev::matchPairsManyFloat( const std::vector<FeaturesDev*>& others, const MatchOptions& opts )
{
    return matchLists( "FeaturesDev::matchPairsManyFloat", Star, star_views( this, others ), star_edges( others.size() ), nullptr, opts,
                       opts.bytes ? ": float descriptors only (use matchPairsMany for MatchOptions::bytes)" : nullptr );
}

std::vector<std::vector<Match>> FeaturesDev::matchPairsGuidedMany( const std::vector<FeaturesDev*>& others, const std::vector<MatchGuide>& guides,
                                                                   const MatchOptions& opts )
{
    return matchLists( "FeaturesDev::matchPairsGuidedMany", Star, star_views( this, others ), star_edges( others.size() ), &guides, opts,
                       opts.bytes ? nullptr : ": the one-to-many form is byte-only (set MatchOptions::bytes)" );
}

std::vector<std::vector<Match>> FeaturesDev::matchPairsGuidedManyFloat( const std::vector<FeaturesDev*>& others, const std::vector<MatchGuide>& guides,
                                                                        const MatchOptions& opts )
{
    return matchLists( "FeaturesDev::matchPairsGuidedManyFloat", Star, star_views( this, others ), star_edges( others.size() ), &guides, opts,
                       opts.bytes ? ": float descriptors only (use matchPairsGuidedMany for MatchOptions::bytes)" : nullptr );
}

std::vector<std::vector<Match>> FeaturesDev::matchPairsGraph( const std::vector<FeaturesDev*>& views, const std::vector<std::pair<int,int>>& edges,
                                                              const MatchOptions& opts )
{
    return matchLists( "FeaturesDev::matchPairsGraph", EdgeList, views, edges, nullptr, opts,
                       opts.bytes ? nullptr : ": the edge-list form is byte-only (set MatchOptions::bytes)" );
}

std::vector<std::vector<Match>> FeaturesDev::matchPairsGraphFloat( const std::vector<FeaturesDev*>& views, const std::vector<std::pair<int,int>>& edges,
                                                                   const MatchOptions& opts )
{
    return matchLists( "FeaturesDev::matchPairsGraphFloat", EdgeList, views, edges, nullptr, opts,
                       opts.bytes ? ": float descriptors only (use the byte form for MatchOptions::bytes)" : nullptr );
}

std::vector<std::vector<Match>> FeaturesDev::matchPairsGuidedGraph( const std::vector<FeaturesDev*>& views, const std::vector<std::pair<int,int>>& edges,
                                                                    const std::vector<MatchGuide>& guides, const MatchOptions& opts )
{
    return matchLists( "FeaturesDev::matchPairsGuidedGraph", EdgeList, views, edges, &guides, opts,
                       opts.bytes ? nullptr : ": the edge-list form is byte-only (set MatchOptions::bytes)" );
}

std::vector<std::vector<Match>> FeaturesDev::matchPairsGuidedGraphFloat( const std::vector<FeaturesDev*>& views,
                                                                         const std::vector<std::pair<int,int>>& edges,
                                                                         const std::vector<MatchGuide>& guides, const MatchOptions& opts )
{
    return matchLists( "FeaturesDev::matchPairsGuidedGraphFloat", EdgeList, views, edges, &guides, opts,
                       opts.bytes ? ": float descriptors only (use the byte form for MatchOptions::bytes)" : nullptr );
}

// ---- RANSAC: three forms, four models each
HomographyEstimate FeaturesDev::estimate( const char* who, RansacModel model, FeaturesDev* other, const std::vector<Match>& matches,
                                          const RansacOptions& opts )
{
    const Views views = star_views( this, Views( 1, other ) );
    const Edges edges = star_edges( 1 );
    const int device = checkViews( who, OnePair, views, edges, 1, "match lists" );
    return estimate_lists( who, model, OnePair, device, views, edges, std::vector<const std::vector<Match>*>( 1, &matches ), opts )[0];
}

std::vector<HomographyEstimate> FeaturesDev::estimateMany( const char* who, RansacModel model, const std::vector<FeaturesDev*>& others,
                                                           const std::vector<std::vector<Match>>& matches, const RansacOptions& opts )
{
    const Views views = star_views( this, others );
    const Edges edges = star_edges( others.size() );
    const int device = checkViews( who, Star, views, edges, matches.size(), "match lists" );
    return estimate_lists( who, model, Star, device, views, edges, pointers( matches ), opts );
}

std::vector<HomographyEstimate> FeaturesDev::estimateGraph( const char* who, RansacModel model, const std::vector<FeaturesDev*>& views,
                                                            const std::vector<std::pair<int,int>>& edges,
                                                            const std::vector<std::vector<Match>>& matches, const RansacOptions& opts )
{
    const int device = checkViews( who, EdgeList, views, edges, matches.size(), "match lists" );
    return estimate_lists( who, model, EdgeList, device, views, edges, pointers( matches ), opts );
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

// FeaturesDev::buildTracks: psx_tracks_graph on the descriptor indices of the lists, at the capacities no result can exceed
Tracks FeaturesDev::buildTracks( const std::vector<FeaturesDev*>& views, const std::vector<std::pair<int,int>>& edges,
                                 const std::vector<std::vector<Match>>& matches, const TrackOptions& opts )
{
    const char* who = "FeaturesDev::buildTracks";
    int device = checkViews( who, EdgeList, views, edges, matches.size(), "match lists" );
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
    for( int e = 0; e < E; e++ ) counts[e] = (int)matches[e].size();
    const std::vector<psx_match_pair_u8> rec = pack_records( pointers( matches ), counts, false );
    const std::vector<psx_view_edge> pe = to_psx( edges );
    psx_track_opts po;
    po.min_views = opts.min_views; po.flags = opts.keep_conflicts ? PSX_TRACKS_KEEP_CONFLICTS : 0;
    std::vector<psx_track_member> mem( (size_t)M );
    out.labels.assign( (size_t)M, -1 );
    out.starts.assign( (size_t)M / 2 + 1, 0 );
    psx_tracks_info info;
    const int rc = psx_tracks_graph( device, rec.data(), counts.data(), pe.data(), E, lens.data(), N, &po, out.labels.data(), out.starts.data(),
                                     M / 2, mem.data(), M, &info );
    if( rc != PSX_OK ) failed( who, rc, ": a descriptor index outside its object" );
    out.starts.resize( (size_t)info.tracks + 1 );
    out.members.resize( (size_t)info.members );
    for( int i = 0; i < info.members; i++ ) { out.members[i].view = mem[i].view; out.members[i].descriptor = mem[i].row; }
    out.n_tracks = info.tracks; out.n_members = info.members; out.components = info.components; out.conflicts = info.conflicts;
    out.too_few_views = info.too_few_views; out.joined_records = info.joined_records;
    return out;
}

} // namespace popsift
