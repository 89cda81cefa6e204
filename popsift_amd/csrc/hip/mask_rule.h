// mask_rule.h -- the detection mask's one rule (psx_set_mask, include/popsift_hip.h).
//
// ONE inline function, compiled for the host (psx_mask_keep) and for the device (refine() in extrema.hip): the two cannot
// drift apart.  A mask is a tight w x h plane of bytes, the size of the INPUT image; non-zero = keypoints allowed here.
// A position (xpos, ypos) in input-image units -- what psx_feature reports -- is kept iff mask[yi * w + xi] != 0 with
//     xi = clamp((int)floorf(xpos + 0.5f), 0, w - 1),   yi = clamp((int)floorf(ypos + 0.5f), 0, h - 1).
// The detector applies it to a refined extremum at octave coordinates (xn, yn) as (xn * s, yn * s) with
// s = ldexpf(1, octave - up_fac), the scale write_feature (orient_desc.hip) applies: a power of two, so xn * s is bit for
// bit the xpos the feature record reports later and a caller can restate the rule on the records alone.  The clamp is
// needed: with upscaling a reported position reaches w - 0.5.  Float32 arithmetic only, no transcendental function:
// host and device agree bit for bit (the sum xpos + 0.5f is rounded to float32 before the floor on both).
#pragma once

#include <math.h>
#include <stddef.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PSX_MASK_HD __host__ __device__
#else
#define PSX_MASK_HD
#endif

// The mask in force for a launch, passed to the kernels BY VALUE (the parameter block is uploaded at psx_resize, the
// mask changes per frame); data == nullptr: no mask, and the launch takes the kernels' unmasked instantiation.
struct PsxMask {
    const unsigned char* data;
    int w, h;
};

// pixel index of one coordinate: floor(v + 0.5) clamped to [0, n - 1]; the clamp is done on the float so that the
// conversion to int is defined for every input (NaN lands on 0)
PSX_MASK_HD inline int psx_mask_pixel(float v, int n)
{
    const float f = floorf(v + 0.5f);
    if (!(f > 0.0f)) return 0;
    if (f >= (float)(n - 1)) return n - 1;
    return (int)f;
}

// the scale from octave coordinates to input-image units
PSX_MASK_HD inline float psx_mask_scale(int octave, int up_fac) { return ldexpf(1.0f, octave - up_fac); }

// true: a keypoint reported at (xpos, ypos) is allowed
PSX_MASK_HD inline bool psx_mask_allows(const unsigned char* mask, int w, int h, float xpos, float ypos)
{
    const int xi = psx_mask_pixel(xpos, w);
    const int yi = psx_mask_pixel(ypos, h);
    return mask[(size_t)yi * (size_t)w + (size_t)xi] != 0;
}
