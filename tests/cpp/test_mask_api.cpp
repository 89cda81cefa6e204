// Test of the detection-mask overloads of the C++ host API: PopSift::enqueue( w, h, image, popsift::Mask ) for byte and
// float images and the matching SiftJob constructors compile and stay unambiguous beside the plain and the keypoint
// overloads (nullptr and literal arguments), the job owns a copy of the plane, "no mask" is a null Mask, and a mask of
// another size is refused with a runtime_error at enqueue -- before a device is touched (this runs without a GPU).
// With POPSIFT_TEST_EXPECT_GPU set (the -m gpu test): an all-zero mask yields an EMPTY result, an all-ones mask the
// unmasked counts, and a job without a mask behind a masked one on the same (single) context runs unmasked.
#include <popsift/popsift.h>
#include <popsift/features.h>
#include <popsift/sift_conf.h>
#include <popsift_c.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static int fails = 0;
#define CHECK(c) do { if(!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); fails++; } } while(0)

template <class F> static std::string runtime_error_of( F f )
{
    try { f(); } catch( const std::runtime_error& e ) { return std::string( "E:" ) + e.what(); } catch( ... ) { return ""; }
    return "";
}

// 0: the job failed with a runtime_error, 1: it delivered a result
static int outcome( SiftJob* job, int* ne, int* no )
{
    int rc = 0;
    try {
        popsift::FeaturesHost* f = job->get();
        if( f != nullptr ) { rc = 1; *ne = f->getFeatureCount(); *no = f->getDescriptorCount(); delete f; }
    } catch( const std::runtime_error& ) { rc = 0; }
    delete job;
    return rc;
}

int main()
{
    const bool gpu = std::getenv( "POPSIFT_TEST_EXPECT_GPU" ) != nullptr;
    const int w = 160, h = 120;
    std::vector<unsigned char> img( (size_t)w * h );
    for( int y = 0; y < h; y++ ) for( int x = 0; x < w; x++ )
        img[(size_t)y * w + x] = (unsigned char)( 128 + 100 * ( ( ( x / 9 ) + ( y / 7 ) ) & 1 ) - ( x * y ) % 23 );
    std::vector<float> fimg( img.size() );
    for( size_t i = 0; i < img.size(); i++ ) fimg[i] = img[i] / 256.0f;
    std::vector<unsigned char> ones( img.size(), 3 ), zeros( img.size(), 0 );

    {   // the job owns a copy of the plane; a null Mask is "no mask"
        std::vector<unsigned char> tmp = ones;
        SiftJob j( w, h, img.data(), popsift::Mask{ tmp.data(), w, h } );
        tmp[5] = 0;
        CHECK( j.hasMask() && j.getMask() != tmp.data() && j.getMask()[5] == 3 && !j.hasKeypoints() );
        SiftJob none( w, h, fimg.data(), popsift::Mask{ nullptr, 0, 0 } );
        CHECK( !none.hasMask() && none.isFloat() );
        SiftJob plain( w, h, img.data() );
        CHECK( !plain.hasMask() );
        SiftJob kp( w, h, img.data(), nullptr, 0 );             // still the keypoint constructor
        CHECK( kp.hasKeypoints() && !kp.hasMask() );
        CHECK( !runtime_error_of( [&]{ SiftJob bad( w, h, img.data(), popsift::Mask{ ones.data(), w - 1, h } ); } ).empty() );
    }

    popsift::Config cfg;
    cfg.setOctaves( 3 );
    {
        PopSift ps( cfg, popsift::Config::ExtractingMode, PopSift::ByteImages );
        // a mask of the wrong size, a null plane with a size, a mask on the wrong image type: refused at enqueue
        const std::string e1 = runtime_error_of( [&]{ ps.enqueue( w, h, img.data(), popsift::Mask{ ones.data(), w, h + 1 } ); } );
        CHECK( e1.find( "160 x 121" ) != std::string::npos && e1.find( "160 x 120" ) != std::string::npos );
        CHECK( !runtime_error_of( [&]{ ps.enqueue( w, h, img.data(), { ones.data(), h, w } ); } ).empty() );
        CHECK( !runtime_error_of( [&]{ ps.enqueue( w, h, img.data(), { nullptr, w, h } ); } ).empty() );
        CHECK( !runtime_error_of( [&]{ ps.enqueue( w, h, fimg.data(), { ones.data(), w, h } ); } ).empty() );
        // unambiguous overload set: literal arguments and nullptr
        int ne = -1, no = -1, ne1 = -1, no1 = -1;
        SiftJob* jm = ps.enqueue( w, h, img.data(), { ones.data(), w, h } );          // Mask from a braced list
        SiftJob* jk = ps.enqueue( w, h, img.data(), nullptr, 0 );                     // the keypoint overload
        SiftJob* jn = ps.enqueue( w, h, img.data(), popsift::Mask{ nullptr, 0, 0 } ); // no mask
        SiftJob* jp = ps.enqueue( w, h, img.data() );
        CHECK( jm && jk && jn && jp );
        CHECK( jm->hasMask() && !jk->hasMask() && jk->hasKeypoints() && !jn->hasMask() && !jp->hasMask() );
        int got = outcome( jm, &ne1, &no1 );
        if( gpu ) CHECK( got == 1 && ne1 > 0 && no1 >= ne1 );
        got = outcome( jk, &ne, &no );
        if( gpu ) CHECK( got == 1 && ne == 0 && no == 0 );
        got = outcome( jn, &ne, &no );
        if( gpu ) CHECK( got == 1 && ne == ne1 && no == no1 );
        got = outcome( jp, &ne, &no );
        if( gpu ) CHECK( got == 1 && ne == ne1 && no == no1 );
        // an all-zero mask: an empty result, no error; the job behind it (same context with POPSIFT_PIPE_DEPTH=1) is unmasked
        SiftJob* jz = ps.enqueue( w, h, img.data(), popsift::Mask{ zeros.data(), w, h } );
        SiftJob* ja = ps.enqueue( w, h, img.data() );
        got = outcome( jz, &ne, &no );
        if( gpu ) CHECK( got == 1 && ne == 0 && no == 0 );
        got = outcome( ja, &ne, &no );
        if( gpu ) CHECK( got == 1 && ne == ne1 && no == no1 );
        ps.uninit();
    }
    {
        PopSift ps( cfg, popsift::Config::MatchingMode, PopSift::FloatImages );
        CHECK( !runtime_error_of( [&]{ ps.enqueue( w, h, img.data(), { ones.data(), w, h } ); } ).empty() );
        SiftJob* j = ps.enqueue( w, h, fimg.data(), { zeros.data(), w, h } );
        CHECK( j != nullptr && j->hasMask() );
        bool ok = false, err = false;
        try {
            popsift::FeaturesDev* d = j->getDev();
            ok = d != nullptr;
            if( gpu ) CHECK( d != nullptr && d->getFeatureCount() == 0 && d->getDescriptorCount() == 0 );   // the mask applies
            delete d;
        } catch( const std::runtime_error& ) { err = true; }
        CHECK( ok || err );
        if( gpu ) CHECK( ok );
        delete j;
        ps.uninit();
    }
    // the flat C binding: NULL for a NULL handle, NULL (with a message) for a mask of another size
    CHECK( popsift_c_enqueue_u8_mask( nullptr, w, h, img.data(), ones.data(), w, h ) == nullptr );
    CHECK( popsift_c_enqueue_f32_mask( nullptr, w, h, fimg.data(), ones.data(), w, h ) == nullptr );
    {
        popsift_c_handle* hd = popsift_c_create( nullptr, 0, 0 );
        CHECK( hd != nullptr );
        if( hd ) {
            CHECK( popsift_c_enqueue_u8_mask( hd, w, h, img.data(), ones.data(), w + 2, h ) == nullptr );
            CHECK( std::strstr( popsift_c_last_error(), "162 x 120" ) != nullptr );
            popsift_c_destroy( hd );
        }
    }
    std::printf( "%s\n", fails ? "FAILED" : "ALL OK" );
    return fails ? 1 : 0;
}
