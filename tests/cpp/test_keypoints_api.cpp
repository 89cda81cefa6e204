// Test of the keypoint overloads of the C++ host API: popsift::Keypoint mirrors psx_keypoint (40 bytes), the four
// PopSift::enqueue( ..., kps, n ) / SiftJob constructors compile and deep-copy the list, the image mode check holds,
// a job is always fulfilled.  With POPSIFT_TEST_EXPECT_GPU set (the -m gpu test): a null or zero-length list yields an
// EMPTY result, not an error; a real list yields its descriptors and FeaturesHost::getSourceIndices().
#include <popsift/popsift.h>
#include <popsift/features.h>
#include <popsift/sift_conf.h>
#include <popsift_hip.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

static int fails = 0;
#define CHECK(c) do { if(!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); fails++; } } while(0)

static_assert( sizeof(psx_keypoint) == 40, "psx_keypoint is 40 bytes" );
static_assert( sizeof(popsift::Keypoint) == sizeof(psx_keypoint), "popsift::Keypoint mirrors psx_keypoint" );
static_assert( (int)popsift::KeypointAuto == PSX_KP_AUTO, "KeypointAuto" );

template <class F> static bool throws_runtime_error( F f )
{
    try { f(); } catch( const std::runtime_error& ) { return true; } catch( ... ) { return false; }
    return false;
}

// 0: the job failed with a runtime_error, 1: it delivered a result (counts in *ne / *no / *nsrc)
static int outcome( SiftJob* job, int* ne, int* no, std::vector<int>* src )
{
    int rc = 0;
    try {
        popsift::FeaturesHost* f = job->get();
        if( f != nullptr ) {
            rc = 1;
            *ne = f->getFeatureCount(); *no = f->getDescriptorCount(); *src = f->getSourceIndices();
            delete f;
        }
    } catch( const std::runtime_error& ) { rc = 0; }
    delete job;
    return rc;
}

int main()
{
    const bool gpu = std::getenv( "POPSIFT_TEST_EXPECT_GPU" ) != nullptr;
    const int w = 96, h = 80;
    std::vector<unsigned char> img( (size_t)w * h );
    for( int y = 0; y < h; y++ ) for( int x = 0; x < w; x++ ) img[(size_t)y * w + x] = (unsigned char)( ( x * 7 + y * 13 + ( x * y ) % 31 ) & 255 );
    std::vector<float> fimg( img.size() );
    for( size_t i = 0; i < img.size(); i++ ) fimg[i] = img[i] / 256.0f;

    std::vector<popsift::Keypoint> kps( 3 );
    for( int i = 0; i < 3; i++ ) {
        popsift::Keypoint& k = kps[i];
        k.xpos = 30.0f + 10.0f * i; k.ypos = 40.0f; k.sigma = 2.5f;
        k.octave = popsift::KeypointAuto; k.lpos = 0; k.num_ori = i == 2 ? 1 : 0;
        for( int q = 0; q < ORIENTATION_MAX_COUNT; q++ ) k.orientation[q] = 0.0f;
    }
    kps[1].xpos = -5.0f;                                      // outside the image: dropped by the acceptance rule

    {   // the job owns a copy of the list
        std::vector<popsift::Keypoint> tmp = kps;
        SiftJob j( w, h, img.data(), tmp.data(), (int)tmp.size() );
        tmp[0].xpos = 999.0f;
        CHECK( j.hasKeypoints() && j.getKeypoints().size() == 3 && j.getKeypoints()[0].xpos == 30.0f );
        SiftJob none( w, h, fimg.data(), nullptr, 0 );
        CHECK( none.hasKeypoints() && none.getKeypoints().empty() && none.isFloat() );
        SiftJob plain( w, h, img.data() );
        CHECK( !plain.hasKeypoints() );
    }

    popsift::Config cfg;
    cfg.setOctaves( 3 );
    {
        PopSift ps( cfg, popsift::Config::ExtractingMode, PopSift::ByteImages );
        CHECK( throws_runtime_error( [&]{ ps.enqueue( w, h, fimg.data(), kps.data(), 3 ); } ) );
        int ne = -1, no = -1; std::vector<int> src;
        // null list, zero-length list: empty result
        SiftJob* j0 = ps.enqueue( w, h, img.data(), nullptr, 0 );
        CHECK( j0 != nullptr );
        int got = outcome( j0, &ne, &no, &src );
        if( gpu ) CHECK( got == 1 && ne == 0 && no == 0 && src.empty() );
        SiftJob* j1 = ps.enqueue( w, h, img.data(), kps.data(), 0 );
        CHECK( j1 != nullptr );
        got = outcome( j1, &ne, &no, &src );
        if( gpu ) CHECK( got == 1 && ne == 0 && no == 0 && src.empty() );
        // a real list: records 0 and 2 survive, in caller order
        SiftJob* j2 = ps.enqueue( w, h, img.data(), kps.data(), 3 );
        CHECK( j2 != nullptr );
        got = outcome( j2, &ne, &no, &src );
        if( gpu ) CHECK( got == 1 && ne == 2 && no >= 2 && src.size() == 2 && src[0] == 0 && src[1] == 2 );
        // the detector path is untouched: no source indices
        SiftJob* j3 = ps.enqueue( w, h, img.data() );
        CHECK( j3 != nullptr );
        got = outcome( j3, &ne, &no, &src );
        if( gpu ) CHECK( got == 1 && src.empty() );
        ps.uninit();
    }
    {
        PopSift ps( cfg, popsift::Config::MatchingMode, PopSift::FloatImages );
        CHECK( throws_runtime_error( [&]{ ps.enqueue( w, h, img.data(), kps.data(), 3 ); } ) );
        SiftJob* j = ps.enqueue( w, h, fimg.data(), kps.data(), 3 );
        CHECK( j != nullptr );
        bool ok = false, err = false;
        try {
            popsift::FeaturesDev* d = j->getDev();
            ok = d != nullptr;
            if( gpu ) CHECK( d != nullptr && d->getFeatureCount() == 2 && d->getDescriptorCount() >= 2 );
            delete d;
        } catch( const std::runtime_error& ) { err = true; }
        CHECK( ok || err );
        if( gpu ) CHECK( ok );
        delete j;
        ps.uninit();
    }
    std::printf( "%s\n", fails ? "FAILED" : "ALL OK" );
    return fails ? 1 : 0;
}
