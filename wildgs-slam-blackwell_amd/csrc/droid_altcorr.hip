// droid_backends.altcorr_forward / altcorr_backward for gfx950: the on-the-fly
// correlation lookup of FactorGraph.update_lowmem (corr.py AltCorrBlock).
//
// For a pixel (y, x) of map fmap1[fi] and a lookup centre (x0, y0), the
// (2r+2)^2 integer positions around the centre ("taps") each get the dot
// product of the pixel's C-channel feature with fmap2[fj]'s feature there
// (zero outside the plane), and the (2r+1)^2 outputs are the bilinear blends
// of four neighbouring taps: corr_index_forward of the all-pairs volume,
// without the volume.
//
// Forward: a workgroup (256 threads) owns an 8 x 8 tile of pixels of one
//   (b, n).  Neighbouring pixels' windows overlap, so the workgroup covers the
//   bounding box of the tile's in-plane taps with 16 x 16 rectangles of fmap2
//   positions (a smooth flow puts all of the tile's 15 x 15 taps at r = 3 in
//   one or two; a rough flow takes more, and costs in proportion) and thread
//   <-> rectangle position, wave <-> four rectangle rows.  The pixels' features
//   of a 32-channel pass are staged in LDS as fp32 once.  Then, per rectangle,
//   a wave finds by ballot (lane <-> pixel) the pixels whose window meets its
//   rows -- none: nothing is loaded -- loads each lane's position's 32 channels
//   with 16-byte loads into registers, and for every such pixel does 32 FMAs
//   (LDS broadcast operand x register), no cross-lane reduction; a lane whose
//   position is one of the pixel's taps adds the pass's dot product into the
//   pixel's tap table in LDS.  Each (pixel, tap) has one owner and one order
//   of addition (passes in channel order): no atomics, no barrier inside a
//   pass, bit-reproducible, and any coordinates take the same path.  Last,
//   lane <-> pixel blends the table into the outputs; every output element is
//   written.
// Backward (fp32; never on the inference path): a workgroup per pixel, lane
//   <-> channel, wave <-> tap.  The tap gradients of one (pixel, n) go through
//   LDS; fmap1_grad is summed in registers and written once, fmap2_grad is
//   scattered with the hardware fp32 atomic add.
#include <limits.h>
#include <math.h>

#include "wgsr_common.h"
#include "wgsr_internal.h"
#include "droid_corr.h"

namespace wgsr {

namespace {

constexpr int kTile = 8;              // the pixel tile is kTile x kTile
constexpr int kPix = kTile * kTile;   // = 64: lane <-> pixel in the set-up and the blend
constexpr int kRect = 16;             // the fmap2 rectangle is kRect x kRect: thread <-> position
constexpr int kChunk = 32;            // channels per pass
static_assert(kRect * kRect == 256 && kPix == 64, "one position per thread, one pixel per lane");

struct AltPixLds {
  int fx[kPix], fy[kPix];    // floor of the lookup centre (kCorrFar: no tap in the plane, or no such pixel)
  float dx[kPix], dy[kPix];  // its fractional part
  float cx[kPix], cy[kPix];  // 1 - dx, 1 - dy (corr_complement)
  int x0, x1, y0, y1;        // the tile's taps in the plane lie in [x0, x1) x [y0, y1)
};

__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = min(v, __shfl_xor(v, m));
  return v;
}

// dynamic LDS (16-byte aligned): the pixels' features of the current pass
// [kPix][kChunk], then the tap table [kPix][(2r+2)^2 | 1]
template <class TI, class TO, int VEC>
__global__ __launch_bounds__(256) void k_altcorr_fwd(const TI* __restrict__ fmap1, const TI* __restrict__ fmap2,
                                                     const float* __restrict__ coords,
                                                     const int64_t* __restrict__ ii, const int64_t* __restrict__ jj,
                                                     int F1, int F2, int N, int h1, int w1, int h2, int w2, int C,
                                                     int r, float scale, int tiles_x, int tiles,
                                                     TO* __restrict__ corr, int64_t stride_b, int64_t stride_n,
                                                     int chan_off) {
  extern __shared__ float4 s_dyn[];
  __shared__ AltPixLds L;
  const int t = threadIdx.x, w = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63;
  const int S = 2 * r + 2, rd = 2 * r + 1, SS = S * S, stride = SS | 1;
  float* __restrict__ s_f1 = reinterpret_cast<float*>(s_dyn);
  float* __restrict__ s_dot = s_f1 + kPix * kChunk;
  const int tile = (int)(blockIdx.x % (unsigned)tiles), bn = (int)(blockIdx.x / (unsigned)tiles);
  const int b = bn / N, n = bn - b * N;
  const int x0 = (tile % tiles_x) * kTile, y0 = (tile / tiles_x) * kTile;
  const int HW = h1 * w1;
  const int64_t fi = ii ? ii[b] : (int64_t)b, fj = jj ? jj[b] : (int64_t)b;
  TO* __restrict__ out = corr + (size_t)b * stride_b + (size_t)n * stride_n + (size_t)chan_off * HW;
  // (block-uniform) a map index outside its range reads nothing
  if (fi < 0 || fi >= F1 || fj < 0 || fj >= F2) {
    for (int idx = t; idx < kPix * rd * rd; idx += 256) {
      const int p = idx & 63, o = idx >> 6, y = y0 + (p >> 3), x = x0 + (p & 7);
      if (y < h1 && x < w1) out[(size_t)o * HW + y * w1 + x] = from_f32<TO>(__builtin_nanf(""));
    }
    return;
  }
  if (t < kPix) {  // (wave 0, whole)
    const int y = y0 + (t >> 3), x = x0 + (t & 7);
    CorrCentre c = {kCorrFar, kCorrFar, 0.f, 0.f, 1.f, 1.f};
    if (y < h1 && x < w1) {
      const float* __restrict__ q = coords + 2 * ((size_t)bn * HW + y * w1 + x);
      c = corr_centre(q[0] * scale, q[1] * scale);
    }
    // the window's part in the plane; a pixel without one takes no part
    const int lx = max(c.fx - r, 0), hx = min(c.fx - r + S, w2), ly = max(c.fy - r, 0), hy = min(c.fy - r + S, h2);
    const bool has = lx < hx && ly < hy;
    L.fx[t] = has ? c.fx : kCorrFar;
    L.fy[t] = has ? c.fy : kCorrFar;
    L.dx[t] = c.dx;
    L.dy[t] = c.dy;
    L.cx[t] = c.cx;
    L.cy[t] = c.cy;
    const int bx0 = wave_min(has ? lx : INT_MAX), by0 = wave_min(has ? ly : INT_MAX);
    const int bx1 = -wave_min(has ? -hx : INT_MAX), by1 = -wave_min(has ? -hy : INT_MAX);
    if (t == 0) {
      const bool any = bx0 != INT_MAX;
      L.x0 = any ? bx0 : 0;
      L.x1 = any ? bx1 : 0;
      L.y0 = any ? by0 : 0;
      L.y1 = any ? by1 : 0;
    }
  }
  for (int i = t; i < kPix * stride; i += 256) s_dot[i] = 0.f;
  __syncthreads();
  const int rx = t & (kRect - 1), ry = t >> 4;
  const int myfx = L.fx[lane], myfy = L.fy[lane];  // lane <-> pixel
  const int bx0 = __builtin_amdgcn_readfirstlane(L.x0), bx1 = __builtin_amdgcn_readfirstlane(L.x1);
  const int by0 = __builtin_amdgcn_readfirstlane(L.y0), by1 = __builtin_amdgcn_readfirstlane(L.y1);
  const TI* __restrict__ f1 = fmap1 + (size_t)fi * HW * C;
  const TI* __restrict__ f2 = fmap2 + (size_t)fj * h2 * w2 * C;

  for (int c0 = 0; c0 < C; c0 += kChunk) {
    __syncthreads();  // the last pass's reads of s_f1 are done
    for (int e = t; e < kPix * kChunk; e += 256) {
      const int p = e >> 5, c = e & (kChunk - 1), y = y0 + (p >> 3), x = x0 + (p & 7);
      s_f1[e] = (y < h1 && x < w1) ? to_f32(f1[(size_t)(y * w1 + x) * C + c0 + c]) : 0.f;
    }
    __syncthreads();
    // the rectangles that tile the taps' bounding box; no barrier in here:
    // a (pixel, tap) entry of the table has one owner
    for (int oy = by0; oy < by1; oy += kRect) {
      for (int ox = bx0; ox < bx1; ox += kRect) {
        // the pixels whose window meets this wave's rows [oy + 4 w, + 4) of the rectangle
        const int wy = oy + 4 * w;
        const bool hit = myfx != kCorrFar && myfx - r < ox + kRect && myfx - r + S > ox && myfy - r < wy + 4 &&
                         myfy - r + S > wy;
        unsigned long long mask = __ballot(hit);
        if (mask == 0) continue;  // (wave-uniform)
        const int ax = ox + rx, ay = oy + ry;
        const bool inplane = ax < w2 && ay < h2;
        const TI* __restrict__ f2p = inplane ? f2 + ((size_t)ay * w2 + ax) * C + c0 : f2;
        float v[kChunk];
        if constexpr (VEC == 1) {
#pragma unroll
          for (int c = 0; c < kChunk; ++c) v[c] = inplane ? to_f32(f2p[c]) : 0.f;
        } else {
          static_assert(VEC * sizeof(TI) == 16, "one 16-byte load");
#pragma unroll
          for (int i = 0; i < kChunk / VEC; ++i) {
            uint4 pk = make_uint4(0, 0, 0, 0);
            if (inplane) pk = reinterpret_cast<const uint4*>(f2p)[i];
            TI e[VEC];
            __builtin_memcpy(e, &pk, 16);
#pragma unroll
            for (int k = 0; k < VEC; ++k) v[i * VEC + k] = to_f32(e[k]);
          }
        }
        while (mask) {
          const int p = __builtin_ctzll(mask);
          mask &= mask - 1;
          const float4* __restrict__ a = reinterpret_cast<const float4*>(s_f1 + p * kChunk);
          float dot = 0.f;
#pragma unroll
          for (int c = 0; c < kChunk / 4; ++c) {
            const float4 f = a[c];  // (one address per wave: a broadcast read)
            dot = fmaf(f.x, v[4 * c], dot);
            dot = fmaf(f.y, v[4 * c + 1], dot);
            dot = fmaf(f.z, v[4 * c + 2], dot);
            dot = fmaf(f.w, v[4 * c + 3], dot);
          }
          const int kx = ax - (__builtin_amdgcn_readlane(myfx, p) - r), ky = ay - (__builtin_amdgcn_readlane(myfy, p) - r);
          if (inplane && kx >= 0 && kx < S && ky >= 0 && ky < S) s_dot[p * stride + ky * S + kx] += dot;
        }
      }
    }
  }
  __syncthreads();

  // blend: lane <-> pixel, output o = iy + rd * ix
  {
    const int p = lane, y = y0 + (p >> 3), x = x0 + (p & 7);
    if (y >= h1 || x >= w1) return;
    const float dx = L.dx[p], dy = L.dy[p], cx = L.cx[p], cy = L.cy[p];
    const float w00 = cx * cy, w10 = dx * cy, w01 = cx * dy, w11 = dx * dy;
    const float* __restrict__ win = s_dot + p * stride;
    TO* __restrict__ o_px = out + y * w1 + x;
    for (int o = w; o < rd * rd; o += 4) {
      const int ix = o / rd, iy = o - ix * rd;
      const float* __restrict__ q = win + iy * S + ix;
      const float val = w00 * q[0] + w10 * q[1] + w01 * q[S] + w11 * q[S + 1];
      o_px[(size_t)o * HW] = from_f32<TO>(val);
    }
  }
}

// one workgroup per pixel (b, y, x); see the head of the file
__global__ __launch_bounds__(256) void k_altcorr_bwd(const float* __restrict__ fmap1,
                                                     const float* __restrict__ fmap2,
                                                     const float* __restrict__ coords,
                                                     const float* __restrict__ corr_grad, int N, int HW, int h2,
                                                     int w2, int C, int r, float* __restrict__ fmap1_grad,
                                                     float* __restrict__ fmap2_grad) {
  __shared__ float s_g[(2 * kCorrMaxRadius + 2) * (2 * kCorrMaxRadius + 2)];
  __shared__ float s_red[4][64];
  const int t = threadIdx.x, w = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63;
  const int S = 2 * r + 2, rd = 2 * r + 1, SS = S * S;
  const size_t b = blockIdx.x / (unsigned)HW;
  const int pix = (int)(blockIdx.x % (unsigned)HW);
  const size_t px = b * HW + pix;
  const float* __restrict__ f2 = fmap2 + b * h2 * w2 * C;
  float* __restrict__ g2 = fmap2_grad + b * h2 * w2 * C;
  for (int cb = 0; cb < C; cb += 64) {
    const int c = cb + lane;
    const bool cin = c < C;
    const float a1 = cin ? fmap1[px * C + c] : 0.f;
    float acc = 0.f;
    for (int n = 0; n < N; ++n) {
      const size_t en = (b * N + n) * HW + pix;
      const CorrCentre ctr = corr_centre(coords[2 * en], coords[2 * en + 1]);
      __syncthreads();  // the last entry's readers of s_g are done
      if (t < SS) {
        // d / d tap (kx, ky): the four outputs that blend it
        const int ky = t / S, kx = t - ky * S;
        const float dx = ctr.dx, dy = ctr.dy, cx = ctr.cx, cy = ctr.cy;
        const float* __restrict__ cg = corr_grad + ((b * N + n) * rd * rd) * HW + pix;
        float g = 0.f;
        if (kx < rd && ky < rd) g += cx * cy * cg[(size_t)(kx * rd + ky) * HW];
        if (kx > 0 && ky < rd) g += dx * cy * cg[(size_t)((kx - 1) * rd + ky) * HW];
        if (kx < rd && ky > 0) g += cx * dy * cg[(size_t)(kx * rd + ky - 1) * HW];
        if (kx > 0 && ky > 0) g += dx * dy * cg[(size_t)((kx - 1) * rd + ky - 1) * HW];
        s_g[t] = g;
      }
      __syncthreads();
      for (int k = w; k < SS; k += 4) {
        const int ky = k / S, kx = k - ky * S;
        const int ax = ctr.fx - r + kx, ay = ctr.fy - r + ky;
        if (ax < 0 || ax >= w2 || ay < 0 || ay >= h2 || !cin) continue;
        const size_t off = ((size_t)ay * w2 + ax) * C + c;
        const float g = s_g[k];
        acc = fmaf(g, f2[off], acc);
        atomicAdd(g2 + off, g * a1);
      }
    }
    __syncthreads();  // (s_red's readers of the last channel block are done)
    s_red[w][lane] = acc;
    __syncthreads();
    if (w == 0 && cin) fmap1_grad[px * C + c] = (s_red[0][lane] + s_red[1][lane]) + (s_red[2][lane] + s_red[3][lane]);
  }
}

template <class TI, class TO>
hipError_t launch_altcorr_fwd(const void* fmap1, const void* fmap2, const float* coords, const int64_t* ii,
                              const int64_t* jj, int F1, int F2, int B, int N, int h1, int w1, int h2, int w2, int C,
                              int r, float scale, void* corr, int64_t stride_b, int64_t stride_n, int chan_off,
                              hipStream_t s) {
  const int tiles_x = (w1 + kTile - 1) / kTile, tiles = tiles_x * ((h1 + kTile - 1) / kTile), S = 2 * r + 2;
  const size_t lds = sizeof(float) * (kPix * (size_t)((S * S) | 1) + kPix * kChunk);
  const dim3 grid((unsigned)((size_t)B * N * tiles));
  constexpr int kVec = 16 / (int)sizeof(TI);
  // (C is a multiple of 32, so every feature row is as aligned as the base)
  if ((reinterpret_cast<uintptr_t>(fmap2) & 15) == 0)
    hipLaunchKernelGGL((k_altcorr_fwd<TI, TO, kVec>), grid, dim3(256), lds, s, (const TI*)fmap1, (const TI*)fmap2,
                       coords, ii, jj, F1, F2, N, h1, w1, h2, w2, C, r, scale, tiles_x, tiles, (TO*)corr, stride_b,
                       stride_n, chan_off);
  else
    hipLaunchKernelGGL((k_altcorr_fwd<TI, TO, 1>), grid, dim3(256), lds, s, (const TI*)fmap1, (const TI*)fmap2,
                       coords, ii, jj, F1, F2, N, h1, w1, h2, w2, C, r, scale, tiles_x, tiles, (TO*)corr, stride_b,
                       stride_n, chan_off);
  return hipGetLastError();
}

// the checks the two entry points share; 0 or an error code
int altcorr_args_ok(const char* who, int B, int N, int h1, int w1, int h2, int w2, int C, int r) {
  if (B < 0 || N < 0 || h1 <= 0 || w1 <= 0 || h2 <= 0 || w2 <= 0)
    return set_error(WGSR_EINVAL, "%s: bad shape b=%d n=%d h1=%d w1=%d h2=%d w2=%d", who, B, N, h1, w1, h2, w2);
  if (C <= 0 || C % kChunk != 0)
    return set_error(WGSR_EINVAL, "%s: the channel count %d must be a positive multiple of %d", who, C, kChunk);
  if (r < 0 || r > kCorrMaxRadius)
    return set_error(WGSR_EINVAL, "%s: radius %d outside [0, %d]", who, r, kCorrMaxRadius);
  const int64_t HW = (int64_t)h1 * w1, tiles = (int64_t)((w1 + kTile - 1) / kTile) * ((h1 + kTile - 1) / kTile);
  if (HW >= (int64_t(1) << 30) || (int64_t)h2 * w2 >= (int64_t(1) << 30) ||
      (int64_t)B * N * tiles >= (int64_t(1) << 31) || (int64_t)B * HW >= (int64_t(1) << 31))
    return set_error(WGSR_EINVAL, "%s: shape too large b=%d n=%d h1=%d w1=%d h2=%d w2=%d", who, B, N, h1, w1, h2, w2);
  return WGSR_OK;
}

}  // namespace

}  // namespace wgsr

using namespace wgsr;

extern "C" {

int wgsr_droid_altcorr_forward(const void* fmap1, const void* fmap2, const float* coords, const int64_t* ii,
                               const int64_t* jj, int dtype, int corr_dtype, int f1, int f2, int b, int n, int h1,
                               int w1, int h2, int w2, int c, int radius, float coord_scale, void* corr,
                               int64_t corr_stride_b, int64_t corr_stride_n, int channel_offset, void* stream) {
  const char* who = "wgsr_droid_altcorr_forward";
  if (dtype != WGSR_DTYPE_F32 && dtype != WGSR_DTYPE_F16)
    return set_error(WGSR_EINVAL, "%s: the maps must be float32 or float16 (tag %d)", who, dtype);
  if (corr_dtype != WGSR_DTYPE_F32 && !(corr_dtype == WGSR_DTYPE_F16 && dtype == WGSR_DTYPE_F16))
    return set_error(WGSR_EINVAL, "%s: corr must be float32, or float16 with float16 maps (tag %d)", who, corr_dtype);
  if (const int e = altcorr_args_ok(who, b, n, h1, w1, h2, w2, c, radius)) return e;
  if (f1 <= 0 || f2 <= 0 || (!ii && b > f1) || (!jj && b > f2))
    return set_error(WGSR_EINVAL, "%s: %d entries need more than f1=%d / f2=%d maps without an index array", who, b,
                     f1, f2);
  int ex = 0;
  if (!(coord_scale > 0.f) || !isfinite(coord_scale) || frexpf(coord_scale, &ex) != 0.5f)
    return set_error(WGSR_EINVAL, "%s: coord_scale %g is not a power of two", who, (double)coord_scale);
  const int rd = 2 * radius + 1;
  if (channel_offset < 0 || corr_stride_n < ((int64_t)channel_offset + rd * rd) * h1 * w1 ||
      corr_stride_b < (int64_t)n * corr_stride_n)
    return set_error(WGSR_EINVAL, "%s: corr strides (%lld, %lld) too small for channel offset %d", who,
                     (long long)corr_stride_b, (long long)corr_stride_n, channel_offset);
  if (b == 0 || n == 0) return WGSR_OK;
  if (!fmap1 || !fmap2 || !coords || !corr) return set_error(WGSR_EINVAL, "%s: null pointer", who);
  hipError_t e;
  if (dtype == WGSR_DTYPE_F32)
    e = launch_altcorr_fwd<float, float>(fmap1, fmap2, coords, ii, jj, f1, f2, b, n, h1, w1, h2, w2, c, radius,
                                         coord_scale, corr, corr_stride_b, corr_stride_n, channel_offset,
                                         (hipStream_t)stream);
  else if (corr_dtype == WGSR_DTYPE_F16)
    e = launch_altcorr_fwd<__half, __half>(fmap1, fmap2, coords, ii, jj, f1, f2, b, n, h1, w1, h2, w2, c, radius,
                                           coord_scale, corr, corr_stride_b, corr_stride_n, channel_offset,
                                           (hipStream_t)stream);
  else
    e = launch_altcorr_fwd<__half, float>(fmap1, fmap2, coords, ii, jj, f1, f2, b, n, h1, w1, h2, w2, c, radius,
                                          coord_scale, corr, corr_stride_b, corr_stride_n, channel_offset,
                                          (hipStream_t)stream);
  return e == hipSuccess ? WGSR_OK : set_error(WGSR_EHIP, "%s: %s", who, hipGetErrorString(e));
}

int wgsr_droid_altcorr_backward(const float* fmap1, const float* fmap2, const float* coords, const float* corr_grad,
                                int b, int n, int h1, int w1, int h2, int w2, int c, int radius, float* fmap1_grad,
                                float* fmap2_grad, float* coords_grad, void* stream) {
  const char* who = "wgsr_droid_altcorr_backward";
  if (const int e = altcorr_args_ok(who, b, n, h1, w1, h2, w2, c, radius)) return e;
  if (b == 0) return WGSR_OK;
  if (!fmap1 || !fmap2 || !fmap1_grad || !fmap2_grad || (n > 0 && (!coords || !corr_grad)))
    return set_error(WGSR_EINVAL, "%s: null pointer", who);
  hipStream_t s = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(fmap2_grad, 0, sizeof(float) * (size_t)b * h2 * w2 * c, s);
  if (e == hipSuccess && coords_grad && n > 0)
    e = hipMemsetAsync(coords_grad, 0, sizeof(float) * 2 * (size_t)b * n * h1 * w1, s);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_altcorr_bwd, dim3((unsigned)((size_t)b * h1 * w1)), dim3(256), 0, s, fmap1, fmap2, coords,
                       corr_grad, n, h1 * w1, h2, w2, c, radius, fmap1_grad, fmap2_grad);
    e = hipGetLastError();
  }
  return e == hipSuccess ? WGSR_OK : set_error(WGSR_EHIP, "%s: %s", who, hipGetErrorString(e));
}

}  // extern "C"
