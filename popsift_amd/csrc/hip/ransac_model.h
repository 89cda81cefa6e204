// ransac_model.h -- what the two RANSAC translation units (ransac.hip: one pair list; ransac_many.hip: many lists in one
// call) share besides the rule headers: the traits of a model kind, the float4 -> correspondence conversion and the order
// of the arg-max.  Internal to the HIP library.
#pragma once

#include <hip/hip_runtime.h>

#include "fundamental_rule.h"

// What differs between the two estimators, by the kind of guide the model is (PSX_GUIDE_HOMOGRAPHY: ransac_rule.h;
// PSX_GUIDE_EPIPOLAR: fundamental_rule.h): the sample size, which models may score, the serial fit of the refit.
template <int KIND> struct RModel;
template <> struct RModel<PSX_GUIDE_HOMOGRAPHY> {
    static constexpr int MIN = 4;
    static __host__ __device__ __forceinline__ bool usable(const float* m) { return psx_ransac_model_finite(m); }
    static void fit(const psx_ransac_pt* pt, int n, float* m) { psx_homography_fit_rule<0>(pt, n, m); }
};
template <> struct RModel<PSX_GUIDE_EPIPOLAR> {
    static constexpr int MIN = PSX_FUND_MIN;
    static __host__ __device__ __forceinline__ bool usable(const float* m) { return psx_fund_model_usable(m); }
    static void fit(const psx_ransac_pt* pt, int n, float* m) { psx_fundamental_fit_rule<0>(pt, n, m); }
};

__device__ __forceinline__ psx_ransac_pt r_pt(const float4& v) { psx_ransac_pt p = {v.x, v.y, v.z, v.w}; return p; }

// the arg-max order: count descending, index ascending
__device__ __forceinline__ void r_better(int& bc, int& bh, int c, int h)
{
    if (c > bc || (c == bc && h < bh)) { bc = c; bh = h; }
}
