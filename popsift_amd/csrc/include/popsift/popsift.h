// popsift/popsift.h -- PopSift / SiftJob, the public extraction API.
//
// Same public surface as the reference (popsift.h:44-317): SiftJob and PopSift live in the
// global namespace, enqueue() deep-copies the image and returns a heap SiftJob*, get() blocks on
// a single-shot future and returns a heap FeaturesHost* the caller deletes.
//
// Implementation differs (MI355X-first): no HIP/CUDA type appears in this header; a PopSift
// owns POPSIFT_PIPE_DEPTH (default 8) worker threads, each with its own extraction context of the
// C-ABI (include/popsift_hip.h: pyramid + HIP stream).  A worker takes the next job from the queue,
// uploads, queues the whole kernel chain, sleeps until its frame is done and fulfils the job, so
// several frames overlap on the GPU.  The reference runs 2 threads over 3 queues with one pyramid
// and synchronises the whole device four times per image (popsift.cpp:293-344).
#pragma once

#include "common/sync_queue.h"
#include "common/device_prop.h"
#include "sift_conf.h"
#include "sift_config.h"
#include "sift_extremum.h"

#include <cstddef>
#include <exception>
#include <future>
#include <memory>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

namespace popsift
{
    class FeaturesBase;
    class FeaturesHost;
    class FeaturesDev;

    /// A caller-supplied keypoint: the fields of psx_keypoint (include/popsift_hip.h), in input-image units as a
    /// Feature reports them.  octave = KeypointAuto lets the library place the keypoint by its sigma; num_ori = 0 lets
    /// it assign the orientations, 1..4 adopts orientation[] verbatim.
    enum { KeypointAuto = -1 };
    struct Keypoint
    {
        float xpos;
        float ypos;
        float sigma;
        int   octave;
        int   lpos;
        int   num_ori;
        float orientation[ORIENTATION_MAX_COUNT];
    };

    /// A detection mask: a tight w x h plane of bytes, the size of the image it goes with; non-zero = keypoints
    /// allowed here (psx_set_mask, include/popsift_hip.h; INTEGRATION.md "Detection mask").  data = nullptr (with
    /// w = h = 0) means "no mask".  The plane is deep-copied at enqueue.
    struct Mask
    {
        const unsigned char* data;
        int w;
        int h;
    };
} // namespace popsift

class SiftJob
{
    std::promise<popsift::FeaturesBase*> _p;
    std::future <popsift::FeaturesBase*> _f;
    int                 _w;
    int                 _h;
    unsigned char*      _imageData;
    size_t              _pinned_cap;   ///< > 0: _imageData is pinned, GPU-mapped pool memory (direct DMA source)
    bool                _is_float;
    std::exception_ptr  _err;
    bool                _has_kps = false;          ///< describe _kps instead of running the detector
    std::vector<popsift::Keypoint> _kps;           ///< deep copy of the caller's keypoints
    unsigned char*      _mask = nullptr;           ///< deep copy of the caller's detection mask (_w x _h bytes), or null
    size_t              _mask_pinned_cap = 0;      ///< > 0: _mask is pinned pool memory

public:
    /// byte image, value range 0..255
    SiftJob( int w, int h, const unsigned char* imageData );
    /// float image, value range [0..1[
    SiftJob( int w, int h, const float* imageData );
    /// the same with caller-supplied keypoints (deep-copied; kps may be null when n is 0)
    SiftJob( int w, int h, const unsigned char* imageData, const popsift::Keypoint* kps, int n );
    SiftJob( int w, int h, const float* imageData, const popsift::Keypoint* kps, int n );
    /// the detector with a detection mask (deep-copied; mask.data null: no mask; its size must be the image's)
    SiftJob( int w, int h, const unsigned char* imageData, const popsift::Mask& mask );
    SiftJob( int w, int h, const float* imageData, const popsift::Mask& mask );
    ~SiftJob( );

    /// deprecated alias of getHost()
    popsift::FeaturesHost* get();
    popsift::FeaturesBase* getBase();
    popsift::FeaturesHost* getHost();
    popsift::FeaturesDev*  getDev();

    /// fulfil the promise (internal)
    void setFeatures( popsift::FeaturesBase* f );
    void setError( std::exception_ptr ptr );

    // internal accessors used by the dispatcher
    int  getWidth() const  { return _w; }
    int  getHeight() const { return _h; }
    bool isFloat() const   { return _is_float; }
    const unsigned char* getData() const { return _imageData; }
    bool isPinned() const  { return _pinned_cap != 0; }
    bool hasKeypoints() const { return _has_kps; }
    const std::vector<popsift::Keypoint>& getKeypoints() const { return _kps; }
    bool hasMask() const { return _mask != nullptr; }
    const unsigned char* getMask() const { return _mask; }
};

class PopSift
{
public:
    enum ImageMode
    {
        ByteImages,   ///< byte image, value range 0..255
        FloatImages   ///< float image, value range [0..1[
    };

    enum AllocTest
    {
        Ok,
        ImageExceedsLinearTextureLimit,
        ImageExceedsLayeredSurfaceLimit
    };

public:
    PopSift() = delete;
    PopSift(const PopSift&) = delete;

    explicit PopSift( ImageMode imode = ByteImages, int device = 0 );
    explicit PopSift( const popsift::Config&          config,
                      popsift::Config::ProcessingMode mode = popsift::Config::ExtractingMode,
                      ImageMode imode = ByteImages, int device = 0 );
    ~PopSift();

public:
    /// provide the configuration; refused (returns false) once extraction has started
    bool configure( const popsift::Config& config, bool force = false );

    void uninit( );

    /// always Ok on this backend unless the pyramid cannot be addressed (no texture limits on gfx950)
    AllocTest testTextureFit( int width, int height );
    std::string testTextureFitErrorString( AllocTest err, int w, int h );

    SiftJob* enqueue( int w, int h, const unsigned char* imageData );
    SiftJob* enqueue( int w, int h, const float* imageData );
    /// Describe the caller's keypoints instead of running the detector (orientations are assigned where a record
    /// brings none).  A null or zero-length list yields an empty result.  FeaturesHost::getSourceIndices() maps the
    /// features back to the records.
    SiftJob* enqueue( int w, int h, const unsigned char* imageData, const popsift::Keypoint* kps, int n );
    SiftJob* enqueue( int w, int h, const float* imageData, const popsift::Keypoint* kps, int n );
    /// Run the detector under a detection mask: only keypoints whose reported position falls on a non-zero mask pixel
    /// are found (they take no slot, orientation or descriptor work otherwise).  mask.data = nullptr: no mask.  A mask
    /// whose size is not the image's is refused with a std::runtime_error before a device is touched.  A job without a
    /// mask runs unmasked, whatever the job before it on the same context carried.
    SiftJob* enqueue( int w, int h, const unsigned char* imageData, const popsift::Mask& mask );
    SiftJob* enqueue( int w, int h, const float* imageData, const popsift::Mask& mask );

    /// deprecated
    inline void uninit( int /*pipe*/ ) { uninit(); }
    /// deprecated
    inline bool init( int /*pipe*/, int w, int h ) { _last_init_w = w; _last_init_h = h; return true; }
    /// deprecated
    inline popsift::FeaturesBase* execute( int /*pipe*/, const unsigned char* imageData )
    {
        SiftJob* j = enqueue( _last_init_w, _last_init_h, imageData );
        if( !j ) return nullptr;
        popsift::FeaturesBase* f = j->getBase();
        delete j;
        return f;
    }

private:
    struct Impl;
    void start();
    void dispatchLoop();
    void resolveOctaves( int w, int h );
    SiftJob* enqueueChecked( int w, int h, const void* imageData, bool is_float, const popsift::Keypoint* kps, int n );
    SiftJob* enqueueMasked( int w, int h, const void* imageData, bool is_float, const popsift::Mask& mask );

    std::unique_ptr<Impl> _impl;
    popsift::Config _config;
    popsift::Config::ProcessingMode _proc_mode;
    int             _last_init_w{};
    int             _last_init_h{};
    ImageMode       _image_mode;
    int             _device;
    bool            _isInit{true};
    popsift::cuda::device_prop_t _device_properties;
};
