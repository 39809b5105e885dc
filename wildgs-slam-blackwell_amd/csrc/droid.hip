// droid_backends for gfx950: the tracker-side ops that feed the mapper
// (frame_distance, depth_filter, iproj) and the per-iteration correlation
// lookup (corr_index_forward / corr_index_backward).  ba is droid_ba.hip,
// altcorr droid_altcorr.hip; projmap is not built (python/droid_backends
// raises for it).
//
// Conventions (DROID-SLAM's): poses [num, 7] = (tx, ty, tz, qx, qy, qz, qw),
// world to camera; disps [num, ht, wd]; intrinsics (fx, fy, cx, cy).  Pixel
// (u = column, v = row) with disparity d is the homogeneous point
// X = ((u - cx) / fx, (v - cy) / fy, 1, d); the transform i -> j is
// q_ij = q_j conj(q_i), t_ij = t_j - R(q_ij) t_i, and X maps to
// Y = (R(q_ij) X_xyz + d t_ij, d).
//
// frame_distance: one workgroup per pair.  The relative pose is uniform per
//   pair: one lane per direction computes it into LDS.  The four per-lane
//   partials (two flow sums, two valid counts) are summed by wave butterflies
//   and a four-wave LDS step; thread 0 writes the pair's result (no atomics).
//   With `bidirectional` the same workgroup evaluates j -> i too and writes
//   0.5 (d_ij + d_ji): one launch for DepthVideo.distance's two.
// depth_filter: one lane per pixel loops over the six neighbour frames with
//   the count in a register; six lanes compute the six relative poses of the
//   workgroup's frame.  One store per pixel, so the output needs no zero fill.
// corr_index: a workgroup owns 64 consecutive (y, x) positions of one volume.
//   Forward: each wave gathers its positions' (2r+2)^2 windows (a window row is
//   contiguous in the plane) into LDS as fp32, then lane <-> position and the
//   (2r+1)^2 outputs leave as coalesced rows of corr[n, i, j, :, :].
//   Backward: corr_grad comes in by the same coalesced rows (lane <->
//   position) into LDS, then one wave per position writes that position's
//   whole [h2, w2] plane in order -- 16-byte stores when the planes allow --
//   so every element, zeros included, is written exactly once (no atomics, no
//   memset by the caller).
#include <math.h>

#include <hip/hip_fp16.h>

#include "wgsr_common.h"
#include "wgsr_internal.h"
#include "droid_corr.h"
#include "droid_pose.h"

namespace wgsr {

namespace {

// ---------------------------------------------------------------------------
// frame_distance
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_frame_distance(const float* __restrict__ poses,
                                                        const float* __restrict__ disps,
                                                        const float* __restrict__ intrinsics, int num, int ht, int wd,
                                                        const int64_t* __restrict__ ii,
                                                        const int64_t* __restrict__ jj, float beta, int ndir,
                                                        float* __restrict__ dist) {
  __shared__ Pose s_rel[2];
  __shared__ float s_sum[2][4];
  __shared__ uint32_t s_cnt[2][4];
  const int t = threadIdx.x, w = t >> 6, lane = t & 63;
  const int64_t fi = ii[blockIdx.x], fj = jj[blockIdx.x];
  // (block-uniform) an index outside [0, num) reads nothing
  if (fi < 0 || fi >= num || fj < 0 || fj >= num) {
    if (t == 0) dist[blockIdx.x] = __builtin_nanf("");
    return;
  }
  if (t < ndir) {
    const Pose a = load_pose(poses, t == 0 ? fi : fj), b = load_pose(poses, t == 0 ? fj : fi);
    s_rel[t] = relative_pose(a, b);
  }
  __syncthreads();
  const float fx = intrinsics[0], fy = intrinsics[1], cx = intrinsics[2], cy = intrinsics[3];
  const float ifx = 1.f / fx, ify = 1.f / fy;
  const int total = ht * wd;
  float result = 0.f;
  for (int dir = 0; dir < ndir; ++dir) {
    const Pose T = s_rel[dir];
    const float* __restrict__ dsp = disps + (size_t)(dir == 0 ? fi : fj) * total;
    float sumA = 0.f, sumB = 0.f;
    uint32_t cntA = 0, cntB = 0;
    for (int k = t; k < total; k += 256) {
      const int row = k / wd, col = k - row * wd;
      const float u = (float)col, v = (float)row, d = dsp[k];
      const f3 X = mk3((u - cx) * ifx, (v - cy) * ify, 1.f);
      // M = Y - X; the flow fx Y0 / Y2 + cx - u is fx (M0 - X0 M2) / Y2 (X2 = 1):
      // no cancellation against u, so a small motion keeps its precision
      {  // rotation and translation
        const f3 D = rot_delta(T, X);
        const float M0 = D.x + d * T.tx, M1 = D.y + d * T.ty, M2 = D.z + d * T.tz;
        const float Y2 = 1.f + M2, iz = __builtin_amdgcn_rcpf(Y2);
        const float du = fx * (M0 - X.x * M2) * iz, dv = fy * (M1 - X.y * M2) * iz;
        const bool ok = Y2 > kMinDepth;
        sumA += ok ? __builtin_amdgcn_sqrtf(du * du + dv * dv) : 0.f;
        cntA += ok ? 1u : 0u;
      }
      {  // translation only
        const float M2 = d * T.tz;
        const float Y2 = 1.f + M2, iz = __builtin_amdgcn_rcpf(Y2);
        const float du = fx * (d * T.tx - X.x * M2) * iz, dv = fy * (d * T.ty - X.y * M2) * iz;
        const bool ok = Y2 > kMinDepth;
        sumB += ok ? __builtin_amdgcn_sqrtf(du * du + dv * dv) : 0.f;
        cntB += ok ? 1u : 0u;
      }
    }
    sumA = wave_sum(sumA);
    sumB = wave_sum(sumB);
    cntA = wave_sum_u32(cntA);
    cntB = wave_sum_u32(cntB);
    __syncthreads();  // (the previous direction's reads are done)
    if (lane == 0) { s_sum[0][w] = sumA; s_sum[1][w] = sumB; s_cnt[0][w] = cntA; s_cnt[1][w] = cntB; }
    __syncthreads();
    if (t == 0) {
      const float a = (s_sum[0][0] + s_sum[0][1]) + (s_sum[0][2] + s_sum[0][3]);
      const float b = (s_sum[1][0] + s_sum[1][1]) + (s_sum[1][2] + s_sum[1][3]);
      const uint32_t na = s_cnt[0][0] + s_cnt[0][1] + s_cnt[0][2] + s_cnt[0][3];
      const uint32_t nb = s_cnt[1][0] + s_cnt[1][1] + s_cnt[1][2] + s_cnt[1][3];
      const float valid = beta * (float)na + (1.f - beta) * (float)nb;
      const float accum = beta * a + (1.f - beta) * b;
      const float dd = (valid / ((float)total + 1e-8f) < 0.75f) ? 1000.f : accum / valid;
      result += dd;
    }
  }
  if (t == 0) dist[blockIdx.x] = ndir == 2 ? 0.5f * result : result;
}

// ---------------------------------------------------------------------------
// depth_filter
// ---------------------------------------------------------------------------
constexpr int kNeigh = 6;
constexpr int kFilterPix = 1024;  // pixels per workgroup (4 per thread)

__global__ __launch_bounds__(256) void k_depth_filter(const float* __restrict__ poses,
                                                      const float* __restrict__ disps,
                                                      const float* __restrict__ intrinsics, int num, int ht, int wd,
                                                      const int64_t* __restrict__ inds,
                                                      const float* __restrict__ thresh,
                                                      float* __restrict__ count) {
  __shared__ Pose s_rel[kNeigh];
  __shared__ int s_jx[kNeigh];
  const int t = threadIdx.x, b = blockIdx.y;
  const int total = ht * wd;
  const int64_t ix = inds[b];
  float* __restrict__ out = count + (size_t)b * total;
  const int k0 = blockIdx.x * kFilterPix;
  if (ix < 0 || ix >= num) {  // (block-uniform) reads nothing
    for (int k = k0 + t; k < min(k0 + kFilterPix, total); k += 256) out[k] = __builtin_nanf("");
    return;
  }
  if (t < kNeigh) {
    // the reference's neighbour rule: ix-1, ix-2, ix-3, ix+3, ix+4, ix+5
    const int64_t jx = t < 3 ? ix - t - 1 : ix + t;
    const bool in = jx >= 0 && jx < num;
    s_jx[t] = in ? (int)jx : -1;
    if (in) s_rel[t] = relative_pose(load_pose(poses, ix), load_pose(poses, jx));
  }
  __syncthreads();
  const float fx = intrinsics[0], fy = intrinsics[1], cx = intrinsics[2], cy = intrinsics[3];
  const float th = thresh[b];
  const float* __restrict__ dsp = disps + (size_t)ix * total;
  const float umax = (float)(wd - 1), vmax = (float)(ht - 1);
  for (int k = k0 + t; k < min(k0 + kFilterPix, total); k += 256) {
    const int row = k / wd, col = k - row * wd;
    const float d = dsp[k];
    const f3 X = mk3(((float)col - cx) / fx, ((float)row - cy) / fy, 1.f);
    int c = 0;
#pragma unroll
    for (int ng = 0; ng < kNeigh; ++ng) {
      const int jx = s_jx[ng];
      if (jx < 0) continue;  // (block-uniform)
      const Pose T = s_rel[ng];
      const f3 R = rotate(T, X);
      const float Y0 = R.x + d * T.tx, Y1 = R.y + d * T.ty, Y2 = R.z + d * T.tz;
      const float uj = fx * (Y0 / Y2) + cx, vj = fy * (Y1 / Y2) + cy;
      // 0 <= floor(uj) < wd - 1 and 0 <= floor(vj) < ht - 1 (false for NaN)
      if (uj >= 0.f && uj < umax && vj >= 0.f && vj < vmax) {
        const int u0 = (int)uj, v0 = (int)vj;  // (non-negative: truncation is floor)
        const float* __restrict__ q = disps + (size_t)jx * total + v0 * wd + u0;
        const float zj = 1.f / (d / Y2);
        const bool hit = fabsf(zj - 1.f / q[0]) < th || fabsf(zj - 1.f / q[1]) < th ||
                         fabsf(zj - 1.f / q[wd]) < th || fabsf(zj - 1.f / q[wd + 1]) < th;
        c += hit ? 1 : 0;
      }
    }
    out[k] = (float)c;
  }
}

// ---------------------------------------------------------------------------
// iproj
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_iproj(const float* __restrict__ poses, const float* __restrict__ disps,
                                               const float* __restrict__ intrinsics, int ht, int wd,
                                               float* __restrict__ points) {
  __shared__ Pose s_pose;
  const int t = threadIdx.x, f = blockIdx.y;
  const int total = ht * wd;
  if (t == 0) s_pose = load_pose(poses, f);
  __syncthreads();
  const int k = blockIdx.x * 256 + t;
  if (k >= total) return;
  const Pose T = s_pose;
  const float fx = intrinsics[0], fy = intrinsics[1], cx = intrinsics[2], cy = intrinsics[3];
  const int row = k / wd, col = k - row * wd;
  const float d = disps[(size_t)f * total + k];
  const f3 R = rotate(T, mk3(((float)col - cx) / fx, ((float)row - cy) / fy, 1.f));
  float* __restrict__ o = points + 3 * ((size_t)f * total + k);
  o[0] = (R.x + d * T.tx) / d;
  o[1] = (R.y + d * T.ty) / d;
  o[2] = (R.z + d * T.tz) / d;
}

// ---------------------------------------------------------------------------
// corr_index
// ---------------------------------------------------------------------------
constexpr int kCorrPos = 64;  // positions per workgroup (lane <-> position)

struct CorrPosLds {
  int fx[kCorrPos], fy[kCorrPos];    // floor of the lookup centre
  float dx[kCorrPos], dy[kCorrPos];  // its fractional part
};

// the lookup centre of the workgroup's position `pos` (thread pos < 64), by
// corr_centre's rule (droid_corr.h): a centre that is not finite, or too far
// away for int arithmetic, gives an all-zero window.
__device__ __forceinline__ void corr_load_centre(CorrPosLds& L, const float* __restrict__ coords, size_t n, int HW,
                                                 int p, int pos) {
  float x0 = 0.f, y0 = 0.f;
  if (p < HW) {
    x0 = coords[(2 * n) * HW + p];
    y0 = coords[(2 * n + 1) * HW + p];
  }
  const CorrCentre c = corr_centre(x0, y0);
  L.fx[pos] = c.fx;
  L.fy[pos] = c.fy;
  L.dx[pos] = c.dx;
  L.dy[pos] = c.dy;
}

// dynamic LDS: kCorrPos rows of `stride` floats
template <class T>
__global__ __launch_bounds__(256) void k_corr_index_fwd(const T* __restrict__ volume,
                                                        const float* __restrict__ coords, int HW, int h2, int w2,
                                                        int r, int groups, T* __restrict__ corr) {
  extern __shared__ float s_win[];
  __shared__ CorrPosLds L;
  const int t = threadIdx.x, w = t >> 6, lane = t & 63;
  const size_t n = blockIdx.x / groups;
  const int p0 = (int)(blockIdx.x % groups) * kCorrPos;
  const int S = 2 * r + 2, rd = 2 * r + 1, taps = S * S, stride = taps | 1;
  if (t < kCorrPos) corr_load_centre(L, coords, n, HW, p0 + t, t);
  __syncthreads();
  // gather: wave w takes positions w, w + 4, ...; tap index = row * S + column
  const size_t plane = (size_t)h2 * w2;
  for (int pos = w; pos < kCorrPos; pos += 4) {
    const int p = p0 + pos;
    if (p >= HW) break;
    const T* __restrict__ src = volume + (n * HW + p) * plane;
    const int bx = L.fx[pos] - r, by = L.fy[pos] - r;
    for (int k = lane; k < taps; k += 64) {
      const int ty = k / S, tx = k - ty * S;
      const int y1 = by + ty, x1 = bx + tx;
      float v = 0.f;
      if (y1 >= 0 && y1 < h2 && x1 >= 0 && x1 < w2) v = to_f32(src[(size_t)y1 * w2 + x1]);
      s_win[pos * stride + k] = v;
    }
  }
  __syncthreads();
  const int p = p0 + lane;
  if (p >= HW) return;
  const float dx = L.dx[lane], dy = L.dy[lane];
  const float w00 = (1.f - dx) * (1.f - dy), w10 = dx * (1.f - dy), w01 = (1.f - dx) * dy, w11 = dx * dy;
  const float* __restrict__ win = s_win + lane * stride;
  for (int o = w; o < rd * rd; o += 4) {
    const int i = o / rd, j = o - i * rd;  // i along x, j along y
    const float* __restrict__ q = win + j * S + i;
    const float v = w00 * q[0] + w10 * q[1] + w01 * q[S] + w11 * q[S + 1];
    corr[(n * rd * rd + o) * HW + p] = from_f32<T>(v);
  }
}

// d / d volume[y1][x1] of one position, from its staged corr_grad row
__device__ __forceinline__ float corr_tap_grad(const float* __restrict__ cg, int rd, int ix, int jy, float w00,
                                               float w10, float w01, float w11) {
  float g = 0.f;
  if (ix < rd && jy < rd) g += w00 * cg[ix * rd + jy];
  if (ix > 0 && jy < rd) g += w10 * cg[(ix - 1) * rd + jy];
  if (ix < rd && jy > 0) g += w01 * cg[ix * rd + jy - 1];
  if (ix > 0 && jy > 0) g += w11 * cg[(ix - 1) * rd + jy - 1];
  return g;
}

// VEC elements per store (VEC * sizeof(T) = 16 bytes, or 1): the host picks
// the vector form only when w2 % VEC == 0 and the planes are 16-byte aligned
template <class T, int VEC>
__global__ __launch_bounds__(256) void k_corr_index_bwd(const float* __restrict__ coords,
                                                        const T* __restrict__ corr_grad, int HW, int h2, int w2,
                                                        int r, int groups, T* __restrict__ volume_grad) {
  extern __shared__ float s_cg[];  // kCorrPos rows of rd * rd floats (odd stride)
  __shared__ CorrPosLds L;
  const int t = threadIdx.x, w = t >> 6, lane = t & 63;
  const size_t n = blockIdx.x / groups;
  const int p0 = (int)(blockIdx.x % groups) * kCorrPos;
  const int S = 2 * r + 2, rd = 2 * r + 1, nout = rd * rd;
  if (t < kCorrPos) corr_load_centre(L, coords, n, HW, p0 + t, t);
  {
    const int p = p0 + lane;
    if (p < HW)
      for (int o = w; o < nout; o += 4) s_cg[lane * nout + o] = to_f32(corr_grad[(n * nout + o) * HW + p]);
  }
  __syncthreads();
  const int plane = h2 * w2;
  for (int pos = w; pos < kCorrPos; pos += 4) {
    const int p = p0 + pos;
    if (p >= HW) break;
    T* __restrict__ dst = volume_grad + (n * HW + p) * (size_t)plane;
    const float* __restrict__ cg = s_cg + pos * nout;
    const int bx = L.fx[pos] - r, by = L.fy[pos] - r;
    const float dx = L.dx[pos], dy = L.dy[pos];
    const float w00 = (1.f - dx) * (1.f - dy), w10 = dx * (1.f - dy), w01 = (1.f - dx) * dy, w11 = dx * dy;
    for (int e = lane * VEC; e < plane; e += 64 * VEC) {
      const int y1 = e / w2, x1 = e - y1 * w2;
      const int jy = y1 - by;
      T v[VEC];
#pragma unroll
      for (int k = 0; k < VEC; ++k) v[k] = from_f32<T>(0.f);
      if (jy >= 0 && jy < S && x1 + VEC > bx && x1 < bx + S) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
          const int ix = x1 + k - bx;
          if (ix >= 0 && ix < S) v[k] = from_f32<T>(corr_tap_grad(cg, rd, ix, jy, w00, w10, w01, w11));
        }
      }
      if constexpr (VEC == 1) {
        dst[e] = v[0];
      } else {
        static_assert(VEC * sizeof(T) == 16, "one 16-byte store");
        uint4 pk;
        __builtin_memcpy(&pk, v, 16);
        *reinterpret_cast<uint4*>(dst + e) = pk;
      }
    }
  }
}

bool frames_ok(int num, int ht, int wd) {
  return num > 0 && ht > 0 && wd > 0 && (int64_t)ht * wd < (int64_t(1) << 30);
}

template <class T>
hipError_t launch_corr_fwd(const void* volume, const float* coords, int n, int HW, int h2, int w2, int r, void* corr,
                           hipStream_t s) {
  const int groups = (HW + kCorrPos - 1) / kCorrPos, S = 2 * r + 2;
  const size_t lds = sizeof(float) * kCorrPos * (size_t)((S * S) | 1);
  hipLaunchKernelGGL(k_corr_index_fwd<T>, dim3((unsigned)(n * groups)), dim3(256), lds, s, (const T*)volume, coords,
                     HW, h2, w2, r, groups, (T*)corr);
  return hipGetLastError();
}

template <class T>
hipError_t launch_corr_bwd(const float* coords, const void* corr_grad, int n, int HW, int h2, int w2, int r,
                           void* volume_grad, hipStream_t s) {
  const int groups = (HW + kCorrPos - 1) / kCorrPos, rd = 2 * r + 1;
  const size_t lds = sizeof(float) * kCorrPos * (size_t)(rd * rd);
  constexpr int kVec = 16 / (int)sizeof(T);
  const bool vec = w2 % kVec == 0 && (reinterpret_cast<uintptr_t>(volume_grad) & 15) == 0;
  const dim3 grid((unsigned)(n * groups));
  if (vec)
    hipLaunchKernelGGL((k_corr_index_bwd<T, kVec>), grid, dim3(256), lds, s, coords, (const T*)corr_grad, HW, h2, w2,
                       r, groups, (T*)volume_grad);
  else
    hipLaunchKernelGGL((k_corr_index_bwd<T, 1>), grid, dim3(256), lds, s, coords, (const T*)corr_grad, HW, h2, w2, r,
                       groups, (T*)volume_grad);
  return hipGetLastError();
}

// shared argument checks of the two lookups; 0 or an error code
int corr_args_ok(const char* who, int dtype, int n, int h1, int w1, int h2, int w2, int r) {
  if (dtype != WGSR_DTYPE_F32 && dtype != WGSR_DTYPE_F16)
    return set_error(WGSR_EINVAL, "%s: the volume must be float32 or float16 (tag %d)", who, dtype);
  if (n < 0 || h1 <= 0 || w1 <= 0 || h2 <= 0 || w2 <= 0)
    return set_error(WGSR_EINVAL, "%s: bad shape n=%d h1=%d w1=%d h2=%d w2=%d", who, n, h1, w1, h2, w2);
  if (r < 0 || r > kCorrMaxRadius)
    return set_error(WGSR_EINVAL, "%s: radius %d outside [0, %d]", who, r, kCorrMaxRadius);
  const int64_t HW = (int64_t)h1 * w1, groups = (HW + kCorrPos - 1) / kCorrPos;
  if (HW >= (int64_t(1) << 30) || (int64_t)h2 * w2 >= (int64_t(1) << 30) || (int64_t)n * groups >= (int64_t(1) << 31))
    return set_error(WGSR_EINVAL, "%s: shape too large n=%d h1=%d w1=%d h2=%d w2=%d", who, n, h1, w1, h2, w2);
  return WGSR_OK;
}

}  // namespace

}  // namespace wgsr

using namespace wgsr;

extern "C" {

int wgsr_droid_frame_distance(const float* poses, const float* disps, const float* intrinsics, int num, int ht,
                              int wd, const int64_t* ii, const int64_t* jj, int n, float beta, int bidirectional,
                              float* dist, void* stream) {
  if (n < 0 || !frames_ok(num, ht, wd))
    return set_error(WGSR_EINVAL, "wgsr_droid_frame_distance: bad shape num=%d ht=%d wd=%d n=%d", num, ht, wd, n);
  if (n == 0) return WGSR_OK;
  if (!poses || !disps || !intrinsics || !ii || !jj || !dist)
    return set_error(WGSR_EINVAL, "wgsr_droid_frame_distance: null pointer");
  hipLaunchKernelGGL(k_frame_distance, dim3((unsigned)n), dim3(256), 0, (hipStream_t)stream, poses, disps, intrinsics,
                     num, ht, wd, ii, jj, beta, bidirectional ? 2 : 1, dist);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? WGSR_OK : set_error(WGSR_EHIP, "wgsr_droid_frame_distance: %s", hipGetErrorString(e));
}

int wgsr_droid_depth_filter(const float* poses, const float* disps, const float* intrinsics, int num, int ht, int wd,
                            const int64_t* inds, const float* thresh, int m, float* count, void* stream) {
  if (m < 0 || m > 65535 || !frames_ok(num, ht, wd))
    return set_error(WGSR_EINVAL, "wgsr_droid_depth_filter: bad shape num=%d ht=%d wd=%d m=%d", num, ht, wd, m);
  if (m == 0) return WGSR_OK;
  if (!poses || !disps || !intrinsics || !inds || !thresh || !count)
    return set_error(WGSR_EINVAL, "wgsr_droid_depth_filter: null pointer");
  const unsigned gx = (unsigned)((ht * wd + kFilterPix - 1) / kFilterPix);
  hipLaunchKernelGGL(k_depth_filter, dim3(gx, (unsigned)m), dim3(256), 0, (hipStream_t)stream, poses, disps,
                     intrinsics, num, ht, wd, inds, thresh, count);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? WGSR_OK : set_error(WGSR_EHIP, "wgsr_droid_depth_filter: %s", hipGetErrorString(e));
}

int wgsr_droid_iproj(const float* poses, const float* disps, const float* intrinsics, int num, int ht, int wd,
                     float* points, void* stream) {
  if (num < 0 || num > 65535 || (num > 0 && !frames_ok(num, ht, wd)))
    return set_error(WGSR_EINVAL, "wgsr_droid_iproj: bad shape num=%d ht=%d wd=%d", num, ht, wd);
  if (num == 0) return WGSR_OK;
  if (!poses || !disps || !intrinsics || !points) return set_error(WGSR_EINVAL, "wgsr_droid_iproj: null pointer");
  hipLaunchKernelGGL(k_iproj, dim3((unsigned)((ht * wd + 255) / 256), (unsigned)num), dim3(256), 0,
                     (hipStream_t)stream, poses, disps, intrinsics, ht, wd, points);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? WGSR_OK : set_error(WGSR_EHIP, "wgsr_droid_iproj: %s", hipGetErrorString(e));
}

int wgsr_droid_corr_index_forward(const void* volume, const float* coords, int dtype, int n, int h1, int w1, int h2,
                                  int w2, int radius, void* corr, void* stream) {
  if (const int c = corr_args_ok("wgsr_droid_corr_index_forward", dtype, n, h1, w1, h2, w2, radius)) return c;
  if (n == 0) return WGSR_OK;
  if (!volume || !coords || !corr) return set_error(WGSR_EINVAL, "wgsr_droid_corr_index_forward: null pointer");
  const hipError_t e = dtype == WGSR_DTYPE_F16
                           ? launch_corr_fwd<__half>(volume, coords, n, h1 * w1, h2, w2, radius, corr,
                                                     (hipStream_t)stream)
                           : launch_corr_fwd<float>(volume, coords, n, h1 * w1, h2, w2, radius, corr,
                                                    (hipStream_t)stream);
  return e == hipSuccess ? WGSR_OK : set_error(WGSR_EHIP, "wgsr_droid_corr_index_forward: %s", hipGetErrorString(e));
}

int wgsr_droid_corr_index_backward(const float* coords, const void* corr_grad, int dtype, int n, int h1, int w1,
                                   int h2, int w2, int radius, void* volume_grad, void* stream) {
  if (const int c = corr_args_ok("wgsr_droid_corr_index_backward", dtype, n, h1, w1, h2, w2, radius)) return c;
  if (n == 0) return WGSR_OK;
  if (!coords || !corr_grad || !volume_grad)
    return set_error(WGSR_EINVAL, "wgsr_droid_corr_index_backward: null pointer");
  const hipError_t e = dtype == WGSR_DTYPE_F16
                           ? launch_corr_bwd<__half>(coords, corr_grad, n, h1 * w1, h2, w2, radius, volume_grad,
                                                     (hipStream_t)stream)
                           : launch_corr_bwd<float>(coords, corr_grad, n, h1 * w1, h2, w2, radius, volume_grad,
                                                    (hipStream_t)stream);
  return e == hipSuccess ? WGSR_OK : set_error(WGSR_EHIP, "wgsr_droid_corr_index_backward: %s", hipGetErrorString(e));
}

}  // extern "C"
