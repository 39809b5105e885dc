// The two encoders in front of the ConvGRU in the tracker's update operator
// (UpdateModule.corr_encoder / .flow_encoder, droid_net.py:88-100, 136-137) for
// gfx950: wgsr_droid_corr_encoder, wgsr_droid_flow_encoder.
//
//   corr  [n, 196, ht, wd] fp16 -> Conv2d(196, 128, 1 x 1) ReLU, Conv2d(128, 128, 3 x 3) ReLU -> [n, 128, ht, wd]
//   flow  [n, 4, ht, wd]        -> Conv2d(4, 128, 7 x 7, pad 3) ReLU, Conv2d(128, 64, 3 x 3) ReLU -> [n, 64, ht, wd]
//
// One kernel, k_encoder, two phases, the hidden layer never in memory.  A
// workgroup of four waves owns the 16 x 8 tile of droid_conv_tile.h.
//
// Phase A.  hidden = fp16(ReLU(first layer + bias)) on the 18 x 10 pixels of the
// tile with its halo, 128 channels, by v_mfma_f32_16x16x32_f16: rows = hidden
// channels (8 row blocks), columns = halo pixels (180, rounded to 12 blocks of
// 16), K = 196 products padded to 224 (7 K-steps) in both encoders.  Wave <->
// 4 row blocks x 6 pixel blocks: 24 accumulators (96 registers), per K-step 4
// weight fragments from memory and 6 B fragments from LDS.  The D fragment
// gives a lane 4 consecutive channels of one pixel: one 8-byte write into the
// staged tile s_h[pixel][kCtStride], the layout ct_taps convolves.  A halo
// pixel outside the image is written as zeros -- the second convolution pads the
// hidden layer, not the input -- and the 12 columns past pixel 179 read pixel
// 179 again (finite, real data) and are not written.
//
//   corr: K index = the channel.  The map is staged 64 channels at a time as
//         s_c[pixel][72] (144 bytes per pixel: 16 pixels on 16 different
//         4-dword slots), chunks of 64, 64, 64 and 32 channels; channels 196 ..
//         223 are staged as zeros and never read from memory (the last 8-channel
//         group reads its 4 real channels only).  27 KB beside the 49 KB hidden
//         tile: two workgroups per CU, each hiding the other's staging.
//   flow: K index = 32 ky + 4 kx + ci, kx = 7 the zero-weight pad: one K-step is
//         one kernel row, and a lane's 8 halfs are the 4 channels of two
//         adjacent pixels.  The (18 + 6) x (10 + 6) input pixels of the tile are
//         staged once as s_f[row][25][4] (8 bytes per pixel, one extra column
//         for kx = 7, zeros outside the image), fp32 input rounded to fp16
//         (round to nearest even) on the way in: autocast's cast.
//
// Phase B.  ct_taps over s_h with the second layer's packed weights
// (pack_conv3x3, KS = 4), wave <-> RBW row blocks x 4 tile rows as k_conv3x3's
// big form (RBW = 4 for 128 rows, 2 for 64), epilogue fp16(ReLU(acc + bias)).
//
// First-layer weights (include/wgsr.h; wgsr.frontend.pack_conv1x1_196 /
// pack_conv7x7_4): 8 x 7 x 64 x 8 fp16, fragment (rb, ks) the A operand as it lies,
//   corr: W[16 rb + (lane & 15)][32 ks + 8 (lane >> 4) + j], zero past channel 195
//   flow: W[16 rb + (lane & 15)][j & 3][ks][2 (lane >> 4) + (j >> 2)], zero at kx = 7
// with an fp32 bias [128].
#include <hip/hip_fp16.h>

#include "droid_conv_tile.h"

namespace wgsr {

namespace {

constexpr int kEnTY = 8;                              // rows of the tile
constexpr int kEnHP = ct_halo(kEnTY);                 // 180 hidden pixels
constexpr int kEnPB = (kEnHP + 15) / 16;              // 12 pixel blocks
constexpr int kEnKS = 7;                              // K-steps of a first layer
constexpr int kEnCorrC = 196;                         // channels of corr
constexpr int kEnChunk = 64;                          // channels of corr staged at a time
constexpr int kEnCS = kEnChunk + 8;                   // halfs per staged pixel of a chunk
constexpr int kEnFW = kCtHX + 6 + 1;                  // staged flow pixels per row: 7 x 7 halo and the kx = 7 column
constexpr int kEnFH = kEnTY + 2 + 6;                  // rows
constexpr int kEnCvKS = kCtC / 32;                    // K-steps per tap of the second layer
constexpr size_t kEnHidBytes = ct_lds(kEnHP);         // the hidden tile (and ct_lds's spare word)
constexpr size_t kEnCorrLds = kEnHidBytes + sizeof(__half) * kEnHP * kEnCS;
constexpr size_t kEnFlowLds = kEnHidBytes + sizeof(__half) * kEnFH * kEnFW * 4;

enum { kEnCorr = 0, kEnFlow = 1 };

struct EncArgs {
  const void* in;         // corr [n, 196, ht, wd] fp16; flow [n, 4, ht, wd] fp32 or fp16
  int in_f32;             // flow: the input is fp32
  const __half* w1;       // [8][7][64][8]
  const float* b1;        // [128]
  const __half* w2;       // pack_conv3x3
  const float* b2;        // [c_out]
  __half* out;            // [n, c_out, ht, wd]
  int ht, wd, tiles_x;
};

// channels c0 .. c0 + 8 ncg - 1 of the halo tile into s_c[pixel][kEnCS]; zeros outside the image and past channel 195
__device__ __forceinline__ void en_stage_corr(__half* __restrict__ s_c, const __half* __restrict__ src, int c0, int ncg,
                                              int x0, int y0, int ht, int wd, int t) {
  const size_t HW = (size_t)ht * wd;
  for (int u = t; u < kEnHP * ncg; u += 256) {
    const int cg = u / kEnHP, hp = u - cg * kEnHP;
    const int ry = hp / kCtHX, rx = hp - ry * kCtHX;
    const int y = y0 - 1 + ry, x = x0 - 1 + rx;
    const int c = c0 + 8 * cg;
    union {
      uint4 v;
      __half h[8];
    } p;
    p.v = make_uint4(0, 0, 0, 0);
    if (y >= 0 && y < ht && x >= 0 && x < wd && c < kEnCorrC) {
      const __half* __restrict__ s = src + (size_t)c * HW + (size_t)y * wd + x;
      if (c + 8 <= kEnCorrC) {
#pragma unroll
        for (int j = 0; j < 8; ++j) p.h[j] = s[(size_t)j * HW];
      } else {  // the last group: channels 192 .. 195
#pragma unroll
        for (int j = 0; j < kEnCorrC % 8; ++j) p.h[j] = s[(size_t)j * HW];
      }
    }
    *reinterpret_cast<uint4*>(s_c + hp * kEnCS + 8 * cg) = p.v;
  }
}

// the (10 + 6) x (18 + 6 + 1) input pixels around the tile into s_f[row][kEnFW][4]; zeros outside the image
template <typename T>
__device__ __forceinline__ void en_stage_flow(__half* __restrict__ s_f, const T* __restrict__ src, int x0, int y0,
                                              int ht, int wd, int t) {
  const size_t HW = (size_t)ht * wd;
  for (int u = t; u < kEnFH * kEnFW; u += 256) {
    const int ry = u / kEnFW, rx = u - ry * kEnFW;
    const int y = y0 - 4 + ry, x = x0 - 4 + rx;
    union {
      uint2 v;
      __half h[4];
    } p;
    p.v = make_uint2(0, 0);
    if (y >= 0 && y < ht && x >= 0 && x < wd) {
      const T* __restrict__ s = src + (size_t)y * wd + x;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if constexpr (sizeof(T) == 4)
          p.h[j] = __float2half_rn(s[(size_t)j * HW]);
        else
          p.h[j] = s[(size_t)j * HW];
      }
    }
    *reinterpret_cast<uint2*>(s_f + 4 * u) = p.v;
  }
}

// dynamic LDS: the hidden tile, then the staged input.  grid (tiles, entries), 256 threads, two workgroups per CU.
template <int ENC, int RBW>
__global__ __launch_bounds__(256, 2) void k_encoder(const EncArgs a) {
  extern __shared__ uint4 s_en[];
  __half* __restrict__ s_h = reinterpret_cast<__half*>(s_en);
  __half* __restrict__ s_in = reinterpret_cast<__half*>(reinterpret_cast<char*>(s_en) + kEnHidBytes);
  const int t = threadIdx.x, lane = t & 63, wv = __builtin_amdgcn_readfirstlane(t >> 6);
  const int i = lane & 15, g = lane >> 4;
  const int b = blockIdx.y;
  const int ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
  const int x0 = tx * kCtTX, y0 = ty * kEnTY;
  const int ht = a.ht, wd = a.wd;
  const size_t HW = (size_t)ht * wd;

  {  // ---- phase A: wave <-> row blocks 4 wc .. + 3, pixel blocks 6 wp .. + 5
    constexpr int RA = 4, PA = 6;
    static_assert(2 * RA * 16 == kCtC && 2 * PA == kEnPB, "four waves cover the hidden tile");
    const int wc = wv & 1, wp = wv >> 1;
    f32x4 acc[RA][PA];
#pragma unroll
    for (int rb = 0; rb < RA; ++rb)
#pragma unroll
      for (int pb = 0; pb < PA; ++pb) acc[rb][pb] = f32x4{0.f, 0.f, 0.f, 0.f};
    const __half* __restrict__ wfrag = a.w1 + (size_t)(RA * wc) * kEnKS * kCtFrag + 8 * lane;
    int hpix[PA];  // the lane's hidden pixel of each block, the padding columns on pixel 179
#pragma unroll
    for (int pb = 0; pb < PA; ++pb) hpix[pb] = min(16 * (PA * wp + pb) + i, kEnHP - 1);

    if constexpr (ENC == kEnCorr) {
      const __half* __restrict__ src = reinterpret_cast<const __half*>(a.in) + (size_t)b * kEnCorrC * HW;
#pragma unroll 1
      for (int c0 = 0; c0 < 32 * kEnKS; c0 += kEnChunk) {
        const int nks = min(kEnChunk, 32 * kEnKS - c0) / 32;
        if (c0) __syncthreads();  // every wave is done with the chunk before
        en_stage_corr(s_in, src, c0, 4 * nks, x0, y0, ht, wd, t);
        __syncthreads();
#pragma unroll 1
        for (int ks = 0; ks < nks; ++ks) {
          f16x8 af[RA], bf[PA];
#pragma unroll
          for (int rb = 0; rb < RA; ++rb)
            af[rb] = *reinterpret_cast<const f16x8*>(wfrag + (size_t)(rb * kEnKS + c0 / 32 + ks) * kCtFrag);
#pragma unroll
          for (int pb = 0; pb < PA; ++pb)
            bf[pb] = *reinterpret_cast<const f16x8*>(s_in + hpix[pb] * kEnCS + 32 * ks + 8 * g);
#pragma unroll
          for (int rb = 0; rb < RA; ++rb)
#pragma unroll
            for (int pb = 0; pb < PA; ++pb)
              acc[rb][pb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[rb], bf[pb], acc[rb][pb], 0, 0, 0);
        }
      }
    } else {
      if (a.in_f32)
        en_stage_flow(s_in, reinterpret_cast<const float*>(a.in) + (size_t)b * 4 * HW, x0, y0, ht, wd, t);
      else
        en_stage_flow(s_in, reinterpret_cast<const __half*>(a.in) + (size_t)b * 4 * HW, x0, y0, ht, wd, t);
      __syncthreads();
      int foff[PA];  // hidden pixel (ry, rx) at tap (0, kx = 2 g): staged pixel (ry, rx + 2 g)
#pragma unroll
      for (int pb = 0; pb < PA; ++pb) {
        const int ry = hpix[pb] / kCtHX, rx = hpix[pb] - ry * kCtHX;
        foff[pb] = 4 * (ry * kEnFW + rx + 2 * g);
      }
#pragma unroll 1
      for (int ks = 0; ks < kEnKS; ++ks) {  // kernel row ky = ks
        f16x8 af[RA], bf[PA];
#pragma unroll
        for (int rb = 0; rb < RA; ++rb)
          af[rb] = *reinterpret_cast<const f16x8*>(wfrag + (size_t)(rb * kEnKS + ks) * kCtFrag);
#pragma unroll
        for (int pb = 0; pb < PA; ++pb) {
          union {
            uint2 v[2];  // (8-byte aligned: two reads)
            f16x8 f;
          } q;
          const uint2* p = reinterpret_cast<const uint2*>(s_in + foff[pb] + 4 * ks * kEnFW);
          q.v[0] = p[0], q.v[1] = p[1];
          bf[pb] = q.f;
        }
#pragma unroll
        for (int rb = 0; rb < RA; ++rb)
#pragma unroll
          for (int pb = 0; pb < PA; ++pb)
            acc[rb][pb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[rb], bf[pb], acc[rb][pb], 0, 0, 0);
      }
    }
    // D: row (hidden channel of the block) 4 g + r in register r, column (pixel of the block) i
#pragma unroll
    for (int pb = 0; pb < PA; ++pb) {
      const int hp = 16 * (PA * wp + pb) + i;
      if (hp >= kEnHP) continue;  // (a padding column)
      const int ry = hp / kCtHX, rx = hp - ry * kCtHX;
      const int y = y0 - 1 + ry, x = x0 - 1 + rx;
      const bool inside = y >= 0 && y < ht && x >= 0 && x < wd;
#pragma unroll
      for (int rb = 0; rb < RA; ++rb) {
        const int ch = 16 * (RA * wc + rb) + 4 * g;
        const float4 bias = *reinterpret_cast<const float4*>(a.b1 + ch);
        union {
          uint2 v;
          __half h[4];
        } p;
        p.v = make_uint2(0, 0);
        if (inside) {
          p.h[0] = __float2half_rn(fmaxf(acc[rb][pb][0] + bias.x, 0.f));
          p.h[1] = __float2half_rn(fmaxf(acc[rb][pb][1] + bias.y, 0.f));
          p.h[2] = __float2half_rn(fmaxf(acc[rb][pb][2] + bias.z, 0.f));
          p.h[3] = __float2half_rn(fmaxf(acc[rb][pb][3] + bias.w, 0.f));
        }
        *reinterpret_cast<uint2*>(s_h + hp * kCtStride + ch) = p.v;
      }
    }
  }
  __syncthreads();

  // ---- phase B: the 3 x 3 convolution of the hidden tile; wave <-> RBW row blocks x 4 tile rows
  constexpr int CBW = 4;
  const int wp = wv & 1, wc = wv >> 1;
  const int rb0 = wc * RBW;
  const __half* xlane = s_h + (wp * CBW * kCtHX + i) * kCtStride + 8 * g;
  const __half* __restrict__ wfrag = a.w2 + (size_t)rb0 * 9 * kEnCvKS * kCtFrag + 8 * lane;
  f32x4 acc[RBW][CBW];
#pragma unroll
  for (int rb = 0; rb < RBW; ++rb)
#pragma unroll
    for (int cb = 0; cb < CBW; ++cb) acc[rb][cb] = f32x4{0.f, 0.f, 0.f, 0.f};
  ct_taps<RBW, CBW, kEnCvKS>(acc, xlane, wfrag, (size_t)9 * kEnCvKS * kCtFrag, kEnCvKS, 0, kEnCvKS);
  constexpr int c_out = 16 * 2 * RBW;
  const int x = x0 + i;
  __half* __restrict__ out = a.out + (size_t)b * c_out * HW;
#pragma unroll
  for (int rb = 0; rb < RBW; ++rb) {
    const int co = 16 * (rb0 + rb) + 4 * g;
    const float4 bias = *reinterpret_cast<const float4*>(a.b2 + co);
    const float bs[4] = {bias.x, bias.y, bias.z, bias.w};
#pragma unroll
    for (int cb = 0; cb < CBW; ++cb) {
      const int y = y0 + wp * CBW + cb;
      if (y >= ht || x >= wd) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r)
        out[((size_t)(co + r) * ht + y) * wd + x] = __float2half_rn(fmaxf(acc[rb][cb][r] + bs[r], 0.f));
    }
  }
}

int en_aligned(const char* who, const void* w1, const void* b1, const void* w2, const void* b2) {
  if (!w1 || !b1 || !w2 || !b2) return set_error(WGSR_EINVAL, "%s: null pointer", who);
  if ((reinterpret_cast<uintptr_t>(w1) | reinterpret_cast<uintptr_t>(b1) | reinterpret_cast<uintptr_t>(w2) |
       reinterpret_cast<uintptr_t>(b2)) & 15)
    return set_error(WGSR_EINVAL, "%s: packed weights and biases must be 16-byte aligned", who);
  return WGSR_OK;
}

template <int ENC, int RBW>
int en_launch(const char* who, EncArgs a, int n, size_t lds, hipStream_t s) {
  a.tiles_x = (a.wd + kCtTX - 1) / kCtTX;
  const dim3 grid((unsigned)(a.tiles_x * ((a.ht + kEnTY - 1) / kEnTY)), (unsigned)n);
  // more than 64 KiB of dynamic LDS has to be asked for, once per kernel and device (as droid_corrvol.hip does)
  if (lds > 64 * 1024) {
    static unsigned long long asked;
    int device = 0;
    hipError_t e = hipGetDevice(&device);
    if (e == hipSuccess && (device >= 64 || !(asked >> device & 1))) {
      e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_encoder<ENC, RBW>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      if (e == hipSuccess && device < 64) asked |= 1ull << device;
    }
    if (e != hipSuccess) return ct_err(who, e);
  }
  hipLaunchKernelGGL((k_encoder<ENC, RBW>), grid, dim3(256), lds, s, a);
  return ct_err(who, hipGetLastError());
}

}  // namespace

}  // namespace wgsr

using namespace wgsr;

extern "C" {

int wgsr_droid_corr_encoder(const void* corr, const void* w1, const float* b1, const void* w2, const float* b2,
                            void* out, int n, int ht, int wd, void* stream) {
  const char* who = "wgsr_droid_corr_encoder";
  if (const int e = ct_shape_ok(who, n, ht, wd)) return e;
  if (n == 0) return WGSR_OK;
  if (!corr || !out) return set_error(WGSR_EINVAL, "%s: null pointer", who);
  if (const int e = en_aligned(who, w1, b1, w2, b2)) return e;
  if (const int e = ct_lds_ok(who, kEnCorrLds)) return e;
  EncArgs a = {};
  a.in = corr, a.w1 = (const __half*)w1, a.b1 = b1, a.w2 = (const __half*)w2, a.b2 = b2, a.out = (__half*)out;
  a.ht = ht, a.wd = wd;
  return en_launch<kEnCorr, 4>(who, a, n, kEnCorrLds, (hipStream_t)stream);
}

int wgsr_droid_flow_encoder(const void* flow, int flow_dtype, const void* w1, const float* b1, const void* w2,
                            const float* b2, void* out, int n, int ht, int wd, void* stream) {
  const char* who = "wgsr_droid_flow_encoder";
  if (const int e = ct_shape_ok(who, n, ht, wd)) return e;
  if (flow_dtype != WGSR_DTYPE_F32 && flow_dtype != WGSR_DTYPE_F16)
    return set_error(WGSR_EINVAL, "%s: flow_dtype = %d is neither WGSR_DTYPE_F32 nor WGSR_DTYPE_F16", who, flow_dtype);
  if (n == 0) return WGSR_OK;
  if (!flow || !out) return set_error(WGSR_EINVAL, "%s: null pointer", who);
  if (const int e = en_aligned(who, w1, b1, w2, b2)) return e;
  if (const int e = ct_lds_ok(who, kEnFlowLds)) return e;
  EncArgs a = {};
  a.in = flow, a.in_f32 = flow_dtype == WGSR_DTYPE_F32;
  a.w1 = (const __half*)w1, a.b1 = b1, a.w2 = (const __half*)w2, a.b2 = b2, a.out = (__half*)out;
  a.ht = ht, a.wd = wd;
  return en_launch<kEnFlow, 2>(who, a, n, kEnFlowLds, (hipStream_t)stream);
}

}  // extern "C"
