// Rigid-transform helpers of the droid_backends kernels (droid.hip,
// droid_ba.hip).  Conventions: see droid.hip.
#pragma once

#include "wgsr_common.h"

namespace wgsr {

constexpr float kMinDepth = 0.25f;  // DROID's MIN_DEPTH

struct Pose {  // a rigid transform: unit quaternion (x, y, z, w) and translation
  float qx, qy, qz, qw, tx, ty, tz;
};

// R(q) v - v as DROID states the rotation (exact for a unit quaternion):
// w s + u x s with s = 2 (u x v), q = (u, w)
__device__ __forceinline__ f3 rot_delta(const Pose& p, f3 v) {
  const f3 u = mk3(p.qx, p.qy, p.qz);
  const f3 s = scl3(2.f, cross3(u, v));
  return add3(scl3(p.qw, s), cross3(u, s));
}
__device__ __forceinline__ f3 rotate(const Pose& p, f3 v) { return add3(v, rot_delta(p, v)); }

__device__ __forceinline__ Pose load_pose(const float* __restrict__ poses, int64_t i) {
  const float* p = poses + 7 * i;
  return Pose{p[3], p[4], p[5], p[6], p[0], p[1], p[2]};
}

// the transform that takes frame a's camera coordinates to frame b's.  The
// quaternion product is evaluated without FMA contraction: for a == b its
// vector part then cancels exactly (a frame is at distance 0 from itself).
__device__ __forceinline__ Pose relative_pose(const Pose& a, const Pose& b) {
#pragma clang fp contract(off)
  Pose r;
  // q_b * conj(q_a)
  const float cx = -a.qx, cy = -a.qy, cz = -a.qz, cw = a.qw;
  r.qw = b.qw * cw - b.qx * cx - b.qy * cy - b.qz * cz;
  r.qx = b.qw * cx + b.qx * cw + b.qy * cz - b.qz * cy;
  r.qy = b.qw * cy - b.qx * cz + b.qy * cw + b.qz * cx;
  r.qz = b.qw * cz + b.qx * cy - b.qy * cx + b.qz * cw;
  r.tx = r.ty = r.tz = 0.f;
  const f3 rt = rotate(r, mk3(a.tx, a.ty, a.tz));
  r.tx = b.tx - rt.x; r.ty = b.ty - rt.y; r.tz = b.tz - rt.z;
  return r;
}

}  // namespace wgsr
