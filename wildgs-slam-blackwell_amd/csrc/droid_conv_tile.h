// What the fp16 MFMA 3 x 3 convolutions of droid_conv3x3.hip (k_conv3x3) and
// droid_gru.hip (k_gru_conv) share: the tile, its staging into LDS, the tap x
// K-step loop over packed weight fragments, the index validation and the host
// checks.  The one place in the kernels that knows the staged layout and the
// fragment layout (wgsr.frontend.pack_conv3x3_wide and include/wgsr.h are the
// other two parties).
//
// Tile.  A workgroup of four waves owns 16 x TY pixels (x by y) of one map.  It
// stages the 18 x (TY + 2) pixels of the tile with its halo, up to 128 channels
// at a time, into LDS, zeros outside the image, transposed on the way in:
// [pixel][channel] with 272 bytes per pixel, so that the B operand of a lane
// (pixel lane & 15 of a tile row, 8 consecutive channels) is one ds_read_b128
// at any tap offset.  (A transposed read of the image as it lies, the idiom of
// droid_upsample.hip, needs its four pixels per lane 8-byte aligned, which the
// taps' shifts by one pixel break.)  272 bytes = 68 dwords puts the 16 pixels
// of a 16-lane group on 16 different 4-dword slots of the 64 banks; the
// 16-lane groups of ds_read_b128 take lanes of two channel groups, whose slots
// are one apart, so two of the four groups meet one 2-way conflict: no stride
// of this layout avoids it (a set of 8 slots is never closed under a shift).
// The writes (ds_write_b128, 8 contiguous lanes = 8 consecutive pixels) are
// conflict-free.
//
// Packed weights (the layout is part of the ABI, include/wgsr.h): with KS =
// C_in / 32 K-steps and R = ceil(C_out / 16) row blocks, element
//   ((((rb 9 + tap) KS + ks) 64 + lane) 8 + j)
// = W[16 rb + (lane & 15)][32 ks + 8 (lane >> 4) + j][tap / 3][tap % 3],
// zero for rows >= C_out: fragment (rb, tap, ks) is the A operand of the wave
// as it lies, 16 contiguous bytes per lane, 1 KiB per wave, read from memory
// (the weights stay in L2: 288 KiB per 128 output rows of 128 channels).
#pragma once

#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include "wgsr_common.h"
#include "wgsr_internal.h"

namespace wgsr {

namespace {

constexpr int kCtC = 128;                             // channels a staged pixel has room for
constexpr int kCtTX = 16;                             // pixels of a tile row
constexpr int kCtHX = kCtTX + 2;                      // with the halo
constexpr int kCtStride = kCtC + 8;                   // halfs per staged pixel: 272 bytes
constexpr int kCtFrag = 64 * 8;                       // halfs of one weight fragment
// dynamic LDS (16-byte aligned) of `pixels` staged pixels: [pixels][kCtStride] fp16, then the validation word
constexpr size_t ct_lds(int pixels) { return sizeof(__half) * (size_t)pixels * kCtStride + 16; }
constexpr int ct_halo(int ty) { return kCtHX * (ty + 2); }  // staged pixels of a tile of ty rows

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// `nch` channels of the tile (x0, y0) of one entry with its halo into s_x[pixel][channel]; zero outside the image.
// Thread <-> (pixel, 8 channels): 8 loads that the wave's lanes continue along x, one 16-byte write.
template <int TY>
__device__ __forceinline__ void ct_stage(__half* __restrict__ s_x, const __half* __restrict__ src, int nch, int x0,
                                         int y0, int ht, int wd, int t) {
  constexpr int HP = ct_halo(TY);
  const size_t HW = (size_t)ht * wd;
  for (int u = t; u < HP * (nch / 8); u += 256) {
    const int cg = u / HP, hp = u - cg * HP;
    const int ry = hp / kCtHX, rx = hp - ry * kCtHX;
    const int y = y0 - 1 + ry, x = x0 - 1 + rx;
    union {
      uint4 v;
      __half h[8];
    } p;
    p.v = make_uint4(0, 0, 0, 0);
    if (y >= 0 && y < ht && x >= 0 && x < wd) {
      const __half* __restrict__ s = src + (size_t)(8 * cg) * HW + (size_t)y * wd + x;
#pragma unroll
      for (int j = 0; j < 8; ++j) p.h[j] = s[(size_t)j * HW];
    }
    *reinterpret_cast<uint4*>(s_x + hp * kCtStride + 8 * cg) = p.v;
  }
}

// One K-step of one tap: RBW weight fragments (rbs halfs apart) and CBW B fragments (one per tile row), then
// RBW x CBW v_mfma_f32_16x16x32_f16.  PS: halfs per staged pixel; HX: staged pixels per row; SY: staged rows per
// tile row (the stride of the convolution; droid_basic_encoder.hip): the defaults are the tile described above.
template <int RBW, int CBW, int PS = kCtStride, int HX = kCtHX, int SY = 1>
__device__ __forceinline__ void ct_kstep(f32x4 (&acc)[RBW][CBW], const __half* xrow, const __half* wtap, size_t rbs,
                                         int ks) {
  f16x8 af[RBW], bf[CBW];
#pragma unroll
  for (int rb = 0; rb < RBW; ++rb) af[rb] = *reinterpret_cast<const f16x8*>(wtap + rb * rbs + (size_t)ks * kCtFrag);
#pragma unroll
  for (int cb = 0; cb < CBW; ++cb) bf[cb] = *reinterpret_cast<const f16x8*>(xrow + cb * SY * HX * PS + 32 * ks);
#pragma unroll
  for (int rb = 0; rb < RBW; ++rb)
#pragma unroll
    for (int cb = 0; cb < CBW; ++cb)
      acc[rb][cb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[rb], bf[cb], acc[rb][cb], 0, 0, 0);
}

// acc += the 9 taps x the K-steps of the staged channels.  xlane: the lane's pixel of its first tile row in the
// staged tile at tap (0, 0), channels 8 (lane >> 4) ..; wlane: the lane's 8 halfs of fragment (first row block,
// tap 0, K-step 0); rbs: halfs between two row blocks; ksteps: K-steps per (row block, tap) of the packed
// weights; ks0: the K-step of staged channel 0.  NKS > 0: that many K-steps, unrolled (nks unused); NKS == 0: nks
// K-steps at run time, an even number, the loop kept rolled outside a pair.
template <int RBW, int CBW, int NKS, int PS = kCtStride, int HX = kCtHX, int SY = 1>
__device__ __forceinline__ void ct_taps(f32x4 (&acc)[RBW][CBW], const __half* xlane, const __half* wlane, size_t rbs,
                                        int ksteps, int ks0, int nks) {
#pragma unroll 1
  for (int tap = 0; tap < 9; ++tap) {
    const int ky = tap / 3, kx = tap - 3 * ky;
    const __half* xrow = xlane + (ky * HX + kx) * PS;
    const __half* wtap = wlane + (size_t)(tap * ksteps + ks0) * kCtFrag;
    if constexpr (NKS > 0) {
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks) ct_kstep<RBW, CBW, PS, HX, SY>(acc, xrow, wtap, rbs, ks);
    } else {
#pragma unroll 1
      for (int k2 = 0; k2 < nks; k2 += 2) {
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) ct_kstep<RBW, CBW, PS, HX, SY>(acc, xrow, wtap, rbs, k2 + kk);
      }
    }
  }
}

// ix (null: nothing to check) against [0, limit): every workgroup scans, the first writes the status word (0 or
// `bit`); true: return before writing.  s_bad: one word of LDS.
__device__ __forceinline__ bool ct_bad_ix(uint32_t* s_bad, const int64_t* __restrict__ ix, int n, int limit,
                                          uint32_t bit, uint32_t* status, bool first, int t) {
  if (t == 0) *s_bad = 0u;
  __syncthreads();
  uint32_t bad = 0u;
  if (ix)
    for (int e = t; e < n; e += 256) {
      const int64_t v = ix[e];
      if (v < 0 || v >= limit) bad = bit;
    }
  if (bad) atomicOr(s_bad, bad);  // (LDS)
  __syncthreads();
  const uint32_t st = *s_bad;
  if (first && t == 0) *status = st;
  return st != 0u;
}

int ct_err(const char* who, hipError_t e) {
  return e == hipSuccess ? WGSR_OK : set_error(WGSR_EHIP, "%s: %s", who, hipGetErrorString(e));
}

// `need` bytes of dynamic LDS against the device's limit per workgroup, asked once per call (a host query: no
// synchronisation).
int ct_lds_ok(const char* who, size_t need) {
  int dev = 0, limit = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e == hipSuccess) e = hipDeviceGetAttribute(&limit, hipDeviceAttributeMaxSharedMemoryPerBlock, dev);
  if (e != hipSuccess) return ct_err(who, e);
  if (need > (size_t)limit)
    return set_error(WGSR_EINVAL, "%s: the tile needs %zu bytes of LDS, the device gives a workgroup %d", who, need,
                     limit);
  return WGSR_OK;
}

// the shape every entry point takes: at most 65535 maps (grid.y) of ht x wd < 2^20 pixels (include/wgsr.h)
int ct_shape_ok(const char* who, int batch, int ht, int wd) {
  if (batch < 0 || batch > 65535 || ht <= 0 || wd <= 0 || (int64_t)ht * wd >= (int64_t(1) << 20))
    return set_error(WGSR_EINVAL, "%s: bad shape: %d maps of %d x %d", who, batch, ht, wd);
  return WGSR_OK;
}

}  // namespace

}  // namespace wgsr
