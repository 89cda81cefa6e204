// CPU test of byte descriptors in the C++ host API (no GPU needed): Config::DescriptorFormat default and setter,
// a default FeaturesHost (no byte view), Feature::print on a feature without float descriptors, and a byte-mode
// PopSift without a usable device: the job is fulfilled and get() fails loudly (or, with a device, returns bytes).
#include <popsift/popsift.h>
#include <popsift/features.h>
#include <popsift/sift_conf.h>

#include <cstdio>
#include <sstream>
#include <stdexcept>
#include <vector>

static int fails = 0;
#define CHECK(c) do { if(!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); fails++; } } while(0)

int main()
{
    popsift::Config c;
    CHECK( c.getDescriptorFormat() == popsift::Config::FloatDescriptors );
    c.setDescriptorFormat( popsift::Config::ByteDescriptors );
    CHECK( c.getDescriptorFormat() == popsift::Config::ByteDescriptors );
    c.setDescriptorFormat( popsift::Config::FloatDescriptors );
    CHECK( c.getDescriptorFormat() == popsift::Config::FloatDescriptors );
    popsift::Config b; b.setDescriptorFormat( popsift::Config::ByteDescriptors );
    popsift::Config copy = b;
    CHECK( copy.getDescriptorFormat() == popsift::Config::ByteDescriptors );

    {
        popsift::FeaturesHost f( 2, 3 );
        CHECK( !f.hasByteDescriptors() && f.getDescriptorBytes() == nullptr && f.descriptorBytes( 0, 0 ) == nullptr );
        CHECK( f.getDescriptors() != nullptr );
        popsift::Feature& k = f.getFeatures()[0];
        k.xpos = 1.5f; k.ypos = 2.5f; k.sigma = 2.0f; k.num_ori = 1; k.desc[0] = nullptr;
        std::ostringstream o; k.print( o, true );             // must not dereference the null descriptor
        CHECK( o.str().find( "1.5 2.5 0.25 0 0.25 " ) == 0 );
    }

    {
        PopSift ps( b, popsift::Config::ExtractingMode, PopSift::ByteImages );
        std::vector<unsigned char> img( 64 * 48, 100 );
        SiftJob* job = ps.enqueue( 64, 48, img.data() );
        CHECK( job != nullptr );
        bool got_error = false, got_bytes = false;
        try {
            popsift::FeaturesHost* f = job->get();
            got_bytes = ( f != nullptr && f->hasByteDescriptors() && f->getDescriptors() == nullptr );
            delete f;
        } catch( const std::runtime_error& ) {
            got_error = true;
        }
        CHECK( got_error || got_bytes );
        delete job;
        ps.uninit();
    }
    std::printf( "%s\n", fails ? "FAILED" : "ALL OK" );
    return fails ? 1 : 0;
}
