// The all-pairs correlation pyramid of the tracker's frontend and motion filter
// (corr.py CorrBlock; wgsr.frontend.CorrBlock) for gfx950: the volume and its
// pooled levels built by one launch into the slots of a store, and the lookup
// of every level by one launch through the slot table.
//
// A slot holds one edge's levels back to back: level i is [H, W, H >> i,
// W >> i] fp16, each level starting on a 16-byte boundary (CorrSlotLayout).
//
// Build (k_corrvol_build): fmap1, fmap2 [n, C, H, W] fp16, channel-major, so a
//   pixel's C features are HW elements apart.  A workgroup (8 waves) owns
//   kM = 32 pixels of frame 1 against one band of 8 full-width rows of frame 2:
//   the band is 8 W consecutive frame-2 positions, so a level-0 row of the
//   tile is one contiguous run in memory, and the band holds whole aligned
//   8 x 8 patches, so every pooled level of the tile comes from the tile alone.
//   The maps are copied as they lie ([channel][pixel]) into LDS; the transposed
//   read ds_read_b64_tr_b16 hands lane <-> pixel its 8 channels of a 32-channel
//   step (both operands go through the same read, so they agree on the order
//   of the channels inside a step).  v_mfma_f32_16x16x32_f16 takes 16 frame-2
//   positions as rows and 16 frame-1 pixels as columns: a lane then holds four
//   consecutive frame-2 positions of one frame-1 pixel, scales the fp32 sums by
//   1/16 (exact: the reference divides both maps by 4), rounds once to fp16 and
//   puts them as one 8-byte write into the tile image in LDS.  After the band's
//   last pass the image goes to level 0 with 16-byte stores, and thread <->
//   (frame-1 pixel, 8 x 8 patch) averages the stored fp16 values 2 x 2, rounds,
//   and averages what it rounded again: levels 1 .. 3 as the reference pools
//   them (from the values it stored, not from the fp32 sums), with the odd
//   trailing row or column dropped.  No plane is read back from memory.
// Lookup (k_corrvol_lookup): k_corr_index_fwd of droid.hip, applied to level i
//   of the edge's slot at coords 2^-i, for every level in the one launch
//   (workgroup <-> 64 positions of one level of one edge).  It reads coords as
//   [n, H, W, 2] and writes level i's window into channels [i (2r+1)^2, (i+1)
//   (2r+1)^2) of [n, L (2r+1)^2, H, W]; same centre rule (droid_corr.h), same
//   weight and sum expressions: bit-identical to the per-level calls.
#include <math.h>

#include "wgsr_common.h"
#include "wgsr_internal.h"
#include "droid_corr.h"

namespace wgsr {

namespace {

constexpr int kCvMaxLevels = 4;  // an 8-row band holds whole 2^(L-1) patches up to L = 4
constexpr int kCvBand = 8;       // rows of frame 2 per workgroup
constexpr int kCvM = 32;         // pixels of frame 1 per workgroup
constexpr int kCvThreads = 512;  // 8 waves
constexpr int kCvN = 128;        // positions of frame 2 per pass (16 per wave)
constexpr int kCvK = 32;         // channels per MFMA step
// LDS row strides in fp16 elements.  A transposed read's 32-lane half takes 8
// rows x 32 bytes: with rows 288 bytes apart (72 dwords = 8 x an odd number)
// they fall on all 64 banks once.  The fmap1 image keeps the smallest stride
// that holds its 32 pixels with 16-byte rows (some of its reads are 2-way):
// at C = 128 and W = 64 the three images then take 78.5 KiB, two workgroups
// per CU.
constexpr int kCvStride1 = 40;   // fmap1 image: [C][32 pixels]
constexpr int kCvStride2 = 144;  // fmap2 image: [C][128 positions]
constexpr size_t kCvMaxLds = 160 * 1024;

struct CorrSlotLayout {
  int64_t off[kCvMaxLevels];  // first element of level i in a slot
  int64_t elems;              // elements per slot (a multiple of 8)
};

CorrSlotLayout slot_layout(int h, int w, int levels) {
  CorrSlotLayout lay = {};
  int64_t at = 0;
  for (int i = 0; i < levels; ++i) {
    lay.off[i] = at;
    at += (int64_t)h * w * (h >> i) * (w >> i);
    at = (at + 7) & ~int64_t(7);
  }
  lay.elems = at;
  return lay;
}

typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// Copy `cols` (a multiple of 8) positions [p0, p0 + cols) of each of the C
// channel rows of one map (src [C][HW]) into img [C][stride]; positions at or
// past `pend` are zero.  VEC: 16-byte moves (HW, p0 and pend multiples of 8,
// src 16-byte aligned).
template <bool VEC>
__device__ __forceinline__ void cv_stage(const __half* __restrict__ src, int HW, int C, int p0, int pend, int cols,
                                         __half* __restrict__ img, int stride, int t) {
  if constexpr (VEC) {
    const int per = cols >> 3;
    for (int u = t; u < C * per; u += kCvThreads) {
      const int k = u / per, c = (u - k * per) << 3;
      uint4 v = make_uint4(0, 0, 0, 0);
      if (p0 + c < pend) v = *reinterpret_cast<const uint4*>(src + (size_t)k * HW + p0 + c);
      *reinterpret_cast<uint4*>(img + k * stride + c) = v;
    }
  } else {
    for (int u = t; u < C * cols; u += kCvThreads) {
      const int k = u / cols, c = u - k * cols;
      img[k * stride + c] = p0 + c < pend ? src[(size_t)k * HW + p0 + c] : __float2half_rn(0.f);
    }
  }
}

// The MFMA operand of 16 pixels (columns c0 .. c0 + 15 of a [channel][pixel]
// image) for channels k0 .. k0 + 31: lane <-> pixel lane & 15, channels
// k0 + 8 (lane >> 4) + 0 .. 7.  Every lane of the wave must be active.
__device__ __forceinline__ f16x8 cv_frag(const __half* img, int stride, int c0, int k0, int lane) {
  const int g = lane >> 4, i = lane & 15, q = i >> 2, p = i & 3;
  const __half* a = img + (k0 + 8 * g + q) * stride + c0 + 4 * p;
  typedef __attribute__((address_space(3))) s16x4* lds_ptr;
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)(a));
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)(a + 4 * stride));
  return __builtin_bit_cast(f16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}

__device__ __forceinline__ float cv_pool(float a, float b, float c, float d) {
  // the mean of four stored fp16 values, rounded to fp16 (kept as its fp32 value)
  return __half2float(__float2half_rn(((a + b) + (c + d)) * 0.25f));
}

// dynamic LDS (16-byte aligned): fmap1 image [C][kCvStride1], fmap2 image
// [C][kCvStride2], tile image [kCvM][tstride]
template <bool VEC>
__global__ __launch_bounds__(kCvThreads) void k_corrvol_build(const __half* __restrict__ fmap1,
                                                       const __half* __restrict__ fmap2, int C, int H, int W,
                                                       int levels, CorrSlotLayout lay, __half* __restrict__ store,
                                                       int capacity, const int* __restrict__ slots, int tstride) {
  extern __shared__ uint4 s_cv[];
  const int t = threadIdx.x, w = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63;
  const int HW = H * W;
  const int e = blockIdx.z, band = blockIdx.y, m0 = blockIdx.x * kCvM;
  const int slot = slots[e];
  if (slot < 0 || slot >= capacity) return;  // (block-uniform) nothing is written outside the store
  __half* __restrict__ s_f1 = reinterpret_cast<__half*>(s_cv);
  __half* __restrict__ s_f2 = s_f1 + C * kCvStride1;
  __half* __restrict__ s_t = s_f2 + C * kCvStride2;
  const int rows = min(kCvBand, H - band * kCvBand);  // rows of frame 2 in this band
  const int q0 = band * kCvBand * W, ncols = rows * W;  // its positions [q0, q0 + ncols)
  const __half* __restrict__ f1 = fmap1 + (size_t)e * C * HW;
  const __half* __restrict__ f2 = fmap2 + (size_t)e * C * HW;

  cv_stage<VEC>(f1, HW, C, m0, HW, kCvM, s_f1, kCvStride1, t);
  // With 16-byte moves and C <= 256 a thread's share of a pass (at most kCvPre
  // moves) is loaded into registers one pass ahead, so that its latency runs
  // beside the MFMAs of the pass before.
  constexpr int kCvPre = 8, kPer = kCvN >> 3;
  const bool ahead = VEC && C * kPer <= kCvPre * kCvThreads;
  uint4 pre[kCvPre];
  auto fetch = [&](int n0) {
#pragma unroll
    for (int i = 0; i < kCvPre; ++i) {
      const int u = t + i * kCvThreads, k = u / kPer, c = (u - k * kPer) << 3;
      pre[i] = make_uint4(0, 0, 0, 0);
      if (u < C * kPer && n0 + c < ncols) pre[i] = *reinterpret_cast<const uint4*>(f2 + (size_t)k * HW + q0 + n0 + c);
    }
  };
  if (ahead) fetch(0);
  for (int n0 = 0; n0 < ncols; n0 += kCvN) {
    __syncthreads();  // the last pass's reads of s_f2 are done
    if (ahead) {
#pragma unroll
      for (int i = 0; i < kCvPre; ++i) {
        const int u = t + i * kCvThreads, k = u / kPer, c = (u - k * kPer) << 3;
        if (u < C * kPer) *reinterpret_cast<uint4*>(s_f2 + k * kCvStride2 + c) = pre[i];
      }
    } else {
      cv_stage<VEC>(f2, HW, C, q0 + n0, q0 + ncols, kCvN, s_f2, kCvStride2, t);
    }
    __syncthreads();
    if (ahead && n0 + kCvN < ncols) fetch(n0 + kCvN);
    f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    for (int k0 = 0; k0 < C; k0 += kCvK) {
      const f16x8 a = cv_frag(s_f2, kCvStride2, 16 * w, k0, lane);
#pragma unroll
      for (int h = 0; h < 2; ++h)
        acc[h] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, cv_frag(s_f1, kCvStride1, 16 * h, k0, lane), acc[h], 0, 0,
                                                         0);
    }
    // D: row (frame-2 position) 4 (lane >> 4) + i in register i, column (frame-1 pixel) lane & 15
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      __half v[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = __float2half_rn(acc[h][i] * 0.0625f);
      uint2 pk;
      __builtin_memcpy(&pk, v, 8);
      *reinterpret_cast<uint2*>(s_t + (16 * h + (lane & 15)) * tstride + n0 + 16 * w + 4 * (lane >> 4)) = pk;
    }
  }
  __syncthreads();

  __half* __restrict__ vol = store + (size_t)slot * lay.elems;
  const int mrows = min(kCvM, HW - m0);  // frame-1 pixels of this tile
  // level 0: row m of the image is positions [q0, q0 + ncols) of pixel m0 + m
  if constexpr (VEC) {
    const int per = ncols >> 3;
    for (int u = t; u < mrows * per; u += kCvThreads) {
      const int m = u / per, c = (u - m * per) << 3;
      *reinterpret_cast<uint4*>(vol + (size_t)(m0 + m) * HW + q0 + c) =
          *reinterpret_cast<const uint4*>(s_t + m * tstride + c);
    }
  } else {
    for (int u = t; u < mrows * ncols; u += kCvThreads) {
      const int m = u / ncols, c = u - m * ncols;
      vol[(size_t)(m0 + m) * HW + q0 + c] = s_t[m * tstride + c];
    }
  }
  if (levels < 2) return;

  // pooled levels: thread <-> (pixel m, patch px): the band's rows x columns 8 px .. 8 px + 7
  const int patches = (W + 7) >> 3;
  for (int u = t; u < mrows * patches; u += kCvThreads) {
    const int m = u / patches, px = u - m * patches, x0 = px << 3;
    const __half* __restrict__ src = s_t + m * tstride + x0;
    float l0[8][8];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      if constexpr (VEC) {  // (W a multiple of 8: whole rows of the patch, 16-byte aligned)
        uint4 pk = make_uint4(0, 0, 0, 0);
        if (r < rows) pk = *reinterpret_cast<const uint4*>(src + r * W);
        __half hv[8];
        __builtin_memcpy(hv, &pk, 16);
#pragma unroll
        for (int c = 0; c < 8; ++c) l0[r][c] = __half2float(hv[c]);
      } else {
#pragma unroll
        for (int c = 0; c < 8; ++c) l0[r][c] = (r < rows && x0 + c < W) ? __half2float(src[r * W + c]) : 0.f;
      }
    }
    const size_t p1 = (size_t)(m0 + m);
    float l1[4][4];
    {
      const int h1 = H >> 1, w1 = W >> 1, y1 = band * 4, x1 = px * 4;
      __half* __restrict__ dst = vol + lay.off[1] + p1 * h1 * w1;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          l1[j][i] = cv_pool(l0[2 * j][2 * i], l0[2 * j][2 * i + 1], l0[2 * j + 1][2 * i], l0[2 * j + 1][2 * i + 1]);
        if (y1 + j >= h1) continue;
        if constexpr (VEC) {  // (w1 a multiple of 4: 8-byte aligned whole rows)
          __half hv[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) hv[i] = __float2half_rn(l1[j][i]);
          uint2 pk;
          __builtin_memcpy(&pk, hv, 8);
          *reinterpret_cast<uint2*>(dst + (size_t)(y1 + j) * w1 + x1) = pk;
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (x1 + i < w1) dst[(size_t)(y1 + j) * w1 + x1 + i] = __float2half_rn(l1[j][i]);
        }
      }
    }
    if (levels < 3) continue;
    float l2[2][2];
    {
      const int h2 = H >> 2, w2 = W >> 2, y2 = band * 2, x2 = px * 2;
      __half* __restrict__ dst = vol + lay.off[2] + p1 * h2 * w2;
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          l2[j][i] = cv_pool(l1[2 * j][2 * i], l1[2 * j][2 * i + 1], l1[2 * j + 1][2 * i], l1[2 * j + 1][2 * i + 1]);
          if (y2 + j < h2 && x2 + i < w2) dst[(size_t)(y2 + j) * w2 + x2 + i] = __float2half_rn(l2[j][i]);
        }
    }
    if (levels < 4) continue;
    {
      const int h3 = H >> 3, w3 = W >> 3;
      if (band < h3 && px < w3)
        vol[lay.off[3] + p1 * h3 * w3 + (size_t)band * w3 + px] =
            __float2half_rn(cv_pool(l2[0][0], l2[0][1], l2[1][0], l2[1][1]));
    }
  }
}

constexpr int kCvPos = 64;  // positions per workgroup (lane <-> position), as k_corr_index_fwd

struct CvPosLds {
  int fx[kCvPos], fy[kCvPos];
  float dx[kCvPos], dy[kCvPos];
};

// dynamic LDS: kCvPos rows of `stride` floats.  Workgroup <-> (edge, level, 64 positions).
__global__ __launch_bounds__(256) void k_corrvol_lookup(const __half* __restrict__ store, CorrSlotLayout lay,
                                                        int capacity, const int* __restrict__ slots,
                                                        const float* __restrict__ coords, int H, int W, int levels,
                                                        int r, int groups, __half* __restrict__ corr) {
  extern __shared__ float s_win[];
  __shared__ CvPosLds L;
  const int t = threadIdx.x, w = t >> 6, lane = t & 63;
  const int HW = H * W;
  const unsigned per_edge = (unsigned)(groups * levels);
  const size_t n = blockIdx.x / per_edge;
  const int rem = (int)(blockIdx.x % per_edge), level = rem / groups;
  const int p0 = (rem - level * groups) * kCvPos;
  const int h2 = H >> level, w2 = W >> level;
  const int S = 2 * r + 2, rd = 2 * r + 1, taps = S * S, stride = taps | 1;
  const int slot = slots[n];
  const bool held = slot >= 0 && slot < capacity;  // (block-uniform) else nothing is read: NaN
  if (t < kCvPos) {
    const int p = p0 + t;
    float x0 = 0.f, y0 = 0.f;
    if (p < HW) {
      const float scale = 1.f / (float)(1 << level);
      x0 = coords[2 * (n * HW + p)] * scale;
      y0 = coords[2 * (n * HW + p) + 1] * scale;
    }
    const CorrCentre c = corr_centre(x0, y0);
    L.fx[t] = c.fx;
    L.fy[t] = c.fy;
    L.dx[t] = c.dx;
    L.dy[t] = c.dy;
  }
  __syncthreads();
  // gather: wave w takes positions w, w + 4, ...; tap index = row * S + column
  const size_t plane = (size_t)h2 * w2;
  const __half* __restrict__ volume = store + (held ? (size_t)slot * lay.elems + lay.off[level] : 0);
  for (int pos = w; pos < kCvPos; pos += 4) {
    const int p = p0 + pos;
    if (p >= HW) break;
    const __half* __restrict__ src = volume + (size_t)p * plane;
    const int bx = L.fx[pos] - r, by = L.fy[pos] - r;
    for (int k = lane; k < taps; k += 64) {
      const int ty = k / S, tx = k - ty * S;
      const int y1 = by + ty, x1 = bx + tx;
      float v = 0.f;
      if (!held) v = __builtin_nanf("");
      else if (y1 >= 0 && y1 < h2 && x1 >= 0 && x1 < w2) v = to_f32(src[(size_t)y1 * w2 + x1]);
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
    corr[((n * levels + level) * rd * rd + o) * HW + p] = from_f32<__half>(v);
  }
}

// the checks the entry points share; 0 or an error code
int corrvol_args_ok(const char* who, int dtype, int n, int h, int w, int levels) {
  if (dtype == WGSR_DTYPE_F32)
    return set_error(WGSR_EINVAL, "%s: float32 volumes (WGSR_DTYPE_F32) are not built; only WGSR_DTYPE_F16", who);
  if (dtype != WGSR_DTYPE_F16) return set_error(WGSR_EINVAL, "%s: unknown dtype tag %d", who, dtype);
  if (levels < 1 || levels > kCvMaxLevels)
    return set_error(WGSR_EINVAL, "%s: %d levels outside [1, %d]", who, levels, kCvMaxLevels);
  if (n < 0 || n > 65535 || h <= 0 || w <= 0 || (int64_t)h * w >= (int64_t(1) << 20))
    return set_error(WGSR_EINVAL, "%s: bad shape n=%d h=%d w=%d", who, n, h, w);
  if ((h >> (levels - 1)) == 0 || (w >> (levels - 1)) == 0)
    return set_error(WGSR_EINVAL, "%s: h=%d, w=%d must each be at least %d for %d levels", who, h, w,
                     1 << (levels - 1), levels);
  return WGSR_OK;
}

}  // namespace

}  // namespace wgsr

using namespace wgsr;

extern "C" {

int64_t wgsr_droid_corr_slot_bytes(int h, int w, int levels) {
  if (corrvol_args_ok("wgsr_droid_corr_slot_bytes", WGSR_DTYPE_F16, 0, h, w, levels) != WGSR_OK) return -1;
  return slot_layout(h, w, levels).elems * (int64_t)sizeof(__half);
}

int wgsr_droid_corr_build(const void* fmap1, const void* fmap2, int dtype, int n, int c, int h, int w, int levels,
                          void* store, int capacity, const int32_t* slots, void* stream) {
  const char* who = "wgsr_droid_corr_build";
  if (const int e = corrvol_args_ok(who, dtype, n, h, w, levels)) return e;
  if (c <= 0 || c % kCvK != 0)
    return set_error(WGSR_EINVAL, "%s: the channel count %d must be a positive multiple of %d", who, c, kCvK);
  if (capacity < 0) return set_error(WGSR_EINVAL, "%s: capacity %d", who, capacity);
  const int tstride = (kCvBand * w + kCvN - 1) / kCvN * kCvN + 8;
  const size_t lds = sizeof(__half) * ((size_t)c * (kCvStride1 + kCvStride2) + (size_t)kCvM * tstride);
  if (lds > kCvMaxLds)
    return set_error(WGSR_EINVAL, "%s: c=%d, w=%d need %zu bytes of LDS per workgroup (at most %zu)", who, c, w, lds,
                     kCvMaxLds);
  if (n == 0) return WGSR_OK;
  if (!fmap1 || !fmap2 || !store || !slots) return set_error(WGSR_EINVAL, "%s: null pointer", who);
  if (reinterpret_cast<uintptr_t>(store) & 15) return set_error(WGSR_EINVAL, "%s: the store must be 16-byte aligned", who);
  const CorrSlotLayout lay = slot_layout(h, w, levels);
  const int HW = h * w;
  const dim3 grid((unsigned)((HW + kCvM - 1) / kCvM), (unsigned)((h + kCvBand - 1) / kCvBand), (unsigned)n);
  hipStream_t s = (hipStream_t)stream;
  const bool vec = w % 8 == 0 && ((reinterpret_cast<uintptr_t>(fmap1) | reinterpret_cast<uintptr_t>(fmap2)) & 15) == 0;
  const void* fn = vec ? (const void*)k_corrvol_build<true> : (const void*)k_corrvol_build<false>;
  // more than 64 KiB of dynamic LDS has to be asked for, once per kernel and
  // device (asked for the largest size, so a later shape needs no second call)
  hipError_t e = hipSuccess;
  if (lds > 64 * 1024) {
    static unsigned long long asked[2];
    int device = 0;
    e = hipGetDevice(&device);
    if (e == hipSuccess && (device >= 64 || !(asked[vec] >> device & 1))) {
      e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kCvMaxLds);
      if (e == hipSuccess && device < 64) asked[vec] |= 1ull << device;
    }
  }
  if (e == hipSuccess) {
    if (vec)
      hipLaunchKernelGGL(k_corrvol_build<true>, grid, dim3(kCvThreads), lds, s, (const __half*)fmap1, (const __half*)fmap2, c,
                         h, w, levels, lay, (__half*)store, capacity, slots, tstride);
    else
      hipLaunchKernelGGL(k_corrvol_build<false>, grid, dim3(kCvThreads), lds, s, (const __half*)fmap1, (const __half*)fmap2,
                         c, h, w, levels, lay, (__half*)store, capacity, slots, tstride);
    e = hipGetLastError();
  }
  return e == hipSuccess ? WGSR_OK : set_error(WGSR_EHIP, "%s: %s", who, hipGetErrorString(e));
}

int wgsr_droid_corr_lookup(const void* store, int capacity, const int32_t* slots, const float* coords, int dtype,
                           int n, int h, int w, int levels, int radius, void* corr, void* stream) {
  const char* who = "wgsr_droid_corr_lookup";
  if (const int e = corrvol_args_ok(who, dtype, n, h, w, levels)) return e;
  if (radius < 0 || radius > kCorrMaxRadius)
    return set_error(WGSR_EINVAL, "%s: radius %d outside [0, %d]", who, radius, kCorrMaxRadius);
  if (capacity < 0) return set_error(WGSR_EINVAL, "%s: capacity %d", who, capacity);
  const int HW = h * w, groups = (HW + kCvPos - 1) / kCvPos, S = 2 * radius + 2;
  if ((int64_t)n * groups * levels >= (int64_t(1) << 31))
    return set_error(WGSR_EINVAL, "%s: shape too large n=%d h=%d w=%d", who, n, h, w);
  if (n == 0) return WGSR_OK;
  if (!store || !slots || !coords || !corr) return set_error(WGSR_EINVAL, "%s: null pointer", who);
  const size_t lds = sizeof(float) * kCvPos * (size_t)((S * S) | 1);
  hipLaunchKernelGGL(k_corrvol_lookup, dim3((unsigned)((size_t)n * groups * levels)), dim3(256), lds,
                     (hipStream_t)stream, (const __half*)store, slot_layout(h, w, levels), capacity, slots, coords, h,
                     w, levels, radius, groups, (__half*)corr);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? WGSR_OK : set_error(WGSR_EHIP, "%s: %s", who, hipGetErrorString(e));
}

}  // extern "C"
