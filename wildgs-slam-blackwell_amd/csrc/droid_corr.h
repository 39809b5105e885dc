// What the correlation lookups of droid.hip (corr_index) and droid_altcorr.hip
// (altcorr) share: the element conversions and the rule for a lookup centre.
#pragma once

#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

namespace wgsr {

constexpr int kCorrMaxRadius = 6;
// floor of a centre that cannot be looked up: no tap of its window, at any
// radius <= kCorrMaxRadius, lands in a plane, and int arithmetic around it
// (+- radius, - another centre's floor) cannot overflow
constexpr int kCorrFar = -(1 << 29);

__device__ __forceinline__ float to_f32(float v) { return v; }
__device__ __forceinline__ float to_f32(__half v) { return __half2float(v); }
template <class T> __device__ __forceinline__ T from_f32(float v);
template <> __device__ __forceinline__ float from_f32<float>(float v) { return v; }
template <> __device__ __forceinline__ __half from_f32<__half>(float v) { return __float2half_rn(v); }

struct CorrCentre {
  int fx, fy;    // floor of the lookup centre
  float dx, dy;  // its fractional part
  float cx, cy;  // 1 - dx, 1 - dy (altcorr's weights; corr_index forms 1.f - dx itself)
};

// 1 - (v - fl) for fl = floorf(v), d = v - fl as rounded.  For a small
// negative v (say -0.003) d is rounded to 2^-24 absolute and 1.f - d would
// carry that as a relative error of 1e-5; (fl + 1) - v is exact there and
// within one rounding everywhere.  d == 0: v is an integer (every float of
// 2^23 or more is, and there fl + 1 need not be exact).
__device__ __forceinline__ float corr_complement(float v, float fl, float d) {
  return d == 0.f ? 1.f : (fl + 1.f) - v;
}

// A centre that is not finite, or too far away for int arithmetic, is moved to
// where no tap can land: the whole window is zero.  The floor is compared as a
// float, before it becomes an int.
__device__ __forceinline__ CorrCentre corr_centre(float x0, float y0) {
  const float flx = floorf(x0), fly = floorf(y0);
  const bool ok = fabsf(flx) < 1e8f && fabsf(fly) < 1e8f;  // (false for NaN)
  CorrCentre c;
  c.fx = ok ? (int)flx : kCorrFar;
  c.fy = ok ? (int)fly : kCorrFar;
  c.dx = ok ? x0 - flx : 0.f;
  c.dy = ok ? y0 - fly : 0.f;
  c.cx = ok ? corr_complement(x0, flx, c.dx) : 1.f;
  c.cy = ok ? corr_complement(y0, fly, c.dy) : 1.f;
  return c;
}

}  // namespace wgsr
