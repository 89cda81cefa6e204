// kp_place.h -- placement and acceptance of caller-supplied keypoints (psx_keypoint, include/popsift_hip.h).
//
// ONE inline function, compiled for the host (psx_place_keypoints) and for the device (k_kp_classify / k_kp_scatter in
// keypoints.hip): the two cannot drift apart.  The rule compares against tables only -- no transcendental function, so
// host and device agree bit for bit:
//   * units: octave units = image units / ldexpf(1, octave - up), the exact inverse of write_feature (orient_desc.hip);
//   * automatic placement (octave == PSX_KP_AUTO): s = sigma * 2^up; o = 0; while o < num_octaves - 1 and
//     s >= b[levels]: s *= 0.5, o++; lpos = 0 if s < b[0], else 1 + the number of b[1] .. b[levels - 1] that are <= s.
//     b_l = sigma0 * 2^((l + 0.5) / levels): [b_0, b_levels) spans exactly a factor of two, so the octaves tile the
//     scale axis without overlap, and a detector keypoint of level 1 .. levels (sigma0 * 2^(sn / levels) with
//     |sn - lpos| <= 0.5) comes back to its own (octave, lpos);
//   * acceptance: finite position and sigma, sigma > 0, num_ori in 0..4, finite given orientations, an explicit octave
//     inside [0, num_octaves), lpos inside [0, L - 1], the octave-unit position inside [0, w_o - 1] x [0, h_o - 1]
//     (the detector's own rule, extrema.hip refine_point) and the octave-unit sigma inside
//     [sigma0, sigma0 * sigma_k^(L - 1)], the range the detector can emit.
#pragma once

#include <float.h>
#include <math.h>

#include "popsift_hip.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PSX_KP_HD __host__ __device__
#else
#define PSX_KP_HD
#endif

// What the rule needs to know of a configuration and an image size; passed to the kernels by value.
struct PsxKpGeom {
    int   num_octaves;
    int   levels;
    int   L;                              // levels + 3
    int   up;                             // int(upscale_factor)
    int   max_extrema;
    float sigma_min, sigma_max;           // sigma0 and (float)(sigma0 * 2^((L - 1) / levels)), octave units
    float bounds[PSX_GAUSS_LEVELS];       // b_0 .. b_levels
    int   w[PSX_MAX_OCTAVES], h[PSX_MAX_OCTAVES];
};

struct PsxKpPlaced {
    int   octave, lpos;
    float xpos, ypos, sigma;              // octave units
};

PSX_KP_HD inline bool psx_kp_finite(float v) { return fabsf(v) <= FLT_MAX; }      // false for NaN and +-inf

// true: the record is accepted and *out says where it lands
PSX_KP_HD inline bool psx_kp_place(const PsxKpGeom& g, const psx_keypoint& k, PsxKpPlaced* out)
{
    if (!psx_kp_finite(k.xpos) || !psx_kp_finite(k.ypos) || !psx_kp_finite(k.sigma) || !(k.sigma > 0.0f)) return false;
    if (k.num_ori < 0 || k.num_ori > PSX_ORI_MAX) return false;
    for (int q = 0; q < PSX_ORI_MAX; q++)
        if (q < k.num_ori && !psx_kp_finite(k.orientation[q])) return false;

    int o, lpos;
    if (k.octave == PSX_KP_AUTO) {
        float s = ldexpf(k.sigma, g.up);
        o = 0;
        while (o < g.num_octaves - 1 && s >= g.bounds[g.levels]) { s *= 0.5f; o++; }
        lpos = 0;
        if (!(s < g.bounds[0])) {
            lpos = 1;
            for (int l = 1; l < g.levels; l++) lpos += (g.bounds[l] <= s) ? 1 : 0;
        }
    } else {
        o = k.octave;
        lpos = k.lpos;
        if (o < 0 || o >= g.num_octaves) return false;
    }
    if (lpos < 0 || lpos > g.L - 1) return false;

    const float unit = ldexpf(1.0f, o - g.up);
    const float x = k.xpos / unit, y = k.ypos / unit, s = k.sigma / unit;
    if (x < 0.0f || x > (float)g.w[o] - 1.0f || y < 0.0f || y > (float)g.h[o] - 1.0f) return false;
    if (s < g.sigma_min || s > g.sigma_max) return false;
    out->octave = o; out->lpos = lpos;
    out->xpos = x; out->ypos = y; out->sigma = s;
    return true;
}
