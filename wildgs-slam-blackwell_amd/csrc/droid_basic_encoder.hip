// The tracker's feature and context encoders (DroidNet.fnet / .cnet, the
// BasicEncoder of extractor.py:75-141) for gfx950, launch by launch:
// wgsr_droid_be_stem, wgsr_droid_be_conv, wgsr_droid_be_stats
// (wgsr.frontend.feature_encoder / context_encoder chain them).
//
//   stem    Conv 7 x 7 stride 2, 3 -> 32; N; ReLU
//   layer1  2 x block(32 -> 32), layer2  block(32 -> 64, stride 2), block(64 -> 64),
//   layer3  block(64 -> 128, stride 2), block(128 -> 128);  head  Conv 1 x 1, 128 -> out
//   block(x) = ReLU(x' + ReLU(N(conv2(ReLU(N(conv1(x))))))), x' = N(Conv 1 x 1 stride 2 (x)) at stride 2, else x
//   N = InstanceNorm2d without parameters (fnet) or the identity (cnet)
//
// Normalise on read.  A convolution writes its raw output R = fp16(acc + bias)
// and, for fnet, per-wave partial statistics of the values as stored; a tiny
// launch (k_be_stats) merges them into (mean, rstd) per (frame, channel).  The
// consumer applies N, the ReLU and the residual sum while it stages its tile:
//   A  ReLU(N(R))          B  ReLU(P + ReLU(N(R)))          C  ReLU(N(Rd) + ReLU(N(R)))
// evaluated in fp32 and rounded to fp16 once; a staged pixel outside the map is
// zero (the convolution pads the activated map).  A launch that stages B or C
// can write the interior of its staged tile, the same bits, as the block output
// X that a later launch reads as P.  No launch only normalises, activates or adds.
//
// k_be_conv.  The tile of droid_conv_tile.h: 16 x TY output pixels, four waves,
// the staged pixels [pixel][C_in + 8] fp16.  Stride 1: TY = 8, 18 x 10 staged
// pixels, a wave owns two tile rows.  Stride 2: TY = 4, 33 x 9 staged pixels
// (origin 2 x0 - 1), a wave owns one row; C_in + 8 halfs per pixel keeps the
// largest tile (C_in = 64: 42768 bytes) under 64 KiB.  A wave walks the output
// rows in chunks of RBW row blocks: rows3 rows of a 3 x 3 convolution
// (pack_conv3x3_wide), then rows1 rows of a 1 x 1 convolution (pack_conv1x1)
// that reads the centre tap of the same staged tile only -- at stride 2 that is
// the block's downsample (input pixel (2 y, 2 x)), at stride 1 the head.
//
// k_be_stem.  K index 21 ky + 3 kx + ci, 147 products padded to 160 = 5 K-steps.
// The (2 16 + 5) x (2 8 + 5) input pixels of a tile are staged as
// s_img[row][3 x + ci] (112 halfs per row), so that the 21 products of a kernel
// row are contiguous; a lane gathers the 8 halfs of its B operand from them.
// With mean / std the kernel stages fp16((x - mean_c) / std_c), the division in
// fp32; zero outside the image, after the normalisation.
//
// Statistics.  A wave reduces the in-image pixels of its rows (at most 32) to
// (count, mean, M2) per channel in two passes over its registers, lanes summed
// in a fixed butterfly; k_be_stats merges a (frame, channel)'s partials with
// Chan's formula, lane l the partials l, l + 64, .. in order, then the 64 lanes
// in a fixed tree: no atomics, two runs give the same bits, and a frame does not
// see the others.
#include <hip/hip_fp16.h>

#include "droid_conv_tile.h"

namespace wgsr {

namespace {

constexpr int kBeStemKS = 5;                          // K-steps of the stem
constexpr int kBeStemK = 147;                         // its products
constexpr int kBeStemTY = 8;
constexpr int kBeImgW = 2 * kCtTX + 5;                // staged image pixels per row
constexpr int kBeImgH = 2 * kBeStemTY + 5;
constexpr int kBeImgRow = 112;                        // halfs per staged image row (3 x 37 = 111)
constexpr int kBeStemRows = 32;
constexpr float kBeEps = 1e-5f;

enum { kBeRaw = 0, kBeCnet = 1 };

constexpr int be_ty(int stride) { return stride == 1 ? 8 : 4; }

struct BeOut {
  const float* bias;      // [rows]
  __half* out;            // [n, rows, ho, wo]; cnet head: net [n, 128, ho, wo]
  __half* out2;           // cnet head: inp [n, 128, ho, wo]
  float* part;            // [n, rows, parts, 3] or null
  int rows, ho, wo, parts;
};

struct BeArgs {
  const __half* r;        // raw map [.., C_in, hi, wi], r_fs halfs between frames
  const float* st;        // its (mean, rstd) [.., C_in, 2], st_fs floats between frames; null: N is the identity
  const __half* p;        // the second term (P or Rd) or null
  const float* pst;       // Rd's statistics; null: the term is taken as it lies
  size_t r_fs, st_fs, p_fs, pst_fs;
  __half* side;           // X [n, C_in, hi, wi] or null
  const __half* w3;       // rows3 rows, pack_conv3x3_wide
  const __half* w1;       // rows1 rows, pack_conv1x1
  int rows3, rows1;
  int hi, wi, tiles_x;
  BeOut o;
};

struct StemArgs {
  const void* img;        // [n, 3, H, W]
  const float* mean;      // [3] or null
  const float* sd;        // [3]: the standard deviations
  const __half* w;        // [2][5][64][8]
  int H, W, tiles_x;
  BeOut o;
};

__device__ __forceinline__ float be_sum16(float v) {  // over the 16 lanes of a group, the same bits in each
#pragma unroll
  for (int m = 1; m < 16; m <<= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// acc + bias of RBW row blocks (from rb0) x CBW tile rows (from y0w) of the wave -> the output and the wave's partial
// statistics (index pi).  D: row 4 g + r in register r, column i.
template <int RBW, int CBW, int EPI>
__device__ __forceinline__ void be_store(const f32x4 (&acc)[RBW][CBW], const BeOut& o, int b, int rb0, int x0, int y0w,
                                         int pi, int lane) {
  const int i = lane & 15, g = lane >> 4;
  const int x = x0 + i;
  const size_t HW = (size_t)o.ho * o.wo;
  const int nx = min(kCtTX, o.wo - x0), ny = max(0, min(CBW, o.ho - y0w));
  const float cnt = (float)(nx * ny);
#pragma unroll
  for (int rb = 0; rb < RBW; ++rb) {
    const int ch = 16 * (rb0 + rb) + 4 * g;
    const float4 bias = *reinterpret_cast<const float4*>(o.bias + ch);
    const float bs[4] = {bias.x, bias.y, bias.z, bias.w};
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float v[CBW];
#pragma unroll
      for (int cb = 0; cb < CBW; ++cb) {
        const int y = y0w + cb;
        const bool ok = y < o.ho && x < o.wo;
        const float a = acc[rb][cb][r] + bs[r];
        __half h;
        if constexpr (EPI == kBeCnet) {
          const int c = ch + r;
          h = __float2half_rn(c < 128 ? tanhf(a) : fmaxf(a, 0.f));
          if (ok) (c < 128 ? o.out : o.out2)[((size_t)b * 128 + (c & 127)) * HW + (size_t)y * o.wo + x] = h;
        } else {
          h = __float2half_rn(a);
          if (ok) o.out[((size_t)b * o.rows + ch + r) * HW + (size_t)y * o.wo + x] = h;
        }
        v[cb] = ok ? __half2float(h) : 0.f;
      }
      if constexpr (EPI == kBeRaw) {
        if (o.part) {  // (uniform)
          float s = 0.f;
#pragma unroll
          for (int cb = 0; cb < CBW; ++cb) s += v[cb];
          s = be_sum16(s);
          const float mean = cnt > 0.f ? s / cnt : 0.f;
          float q = 0.f;
#pragma unroll
          for (int cb = 0; cb < CBW; ++cb) {
            const float d = v[cb] - mean;
            if (y0w + cb < o.ho && x < o.wo) q += d * d;
          }
          q = be_sum16(q);
          if (i == 0) {
            float* dst = o.part + (((size_t)b * o.rows + ch + r) * o.parts + pi) * 3;
            dst[0] = cnt, dst[1] = mean, dst[2] = q;
          }
        }
      }
    }
  }
}

// The tile (x0, y0) of output pixels: its SY 16 + (3 - SY) by SY TY + (3 - SY) input pixels from (SY x0 - 1, SY y0 -
// 1), form A, B or C of the sources, into s_x[pixel][CIN + 8]; zero outside the map.  Thread <-> (pixel, 8 channels).
template <int CIN, int SY>
__device__ __forceinline__ void be_stage(__half* __restrict__ s_x, const BeArgs& a, int b, int x0, int y0, int t) {
  constexpr int TY = be_ty(SY), PS = CIN + 8;
  constexpr int HX = SY * kCtTX + 3 - SY, HY = SY * TY + 3 - SY, HP = HX * HY;
  const int hi = a.hi, wi = a.wi;
  const size_t HW = (size_t)hi * wi;
  const __half* __restrict__ r = a.r + (size_t)b * a.r_fs;
  const float* __restrict__ st = a.st ? a.st + (size_t)b * a.st_fs : nullptr;
  const __half* __restrict__ p = a.p ? a.p + (size_t)b * a.p_fs : nullptr;
  const float* __restrict__ pst = a.pst ? a.pst + (size_t)b * a.pst_fs : nullptr;
  __half* __restrict__ side = a.side ? a.side + (size_t)b * CIN * HW : nullptr;
  for (int u = t; u < HP * (CIN / 8); u += 256) {
    const int cg = u / HP, hp = u - cg * HP;
    const int ry = hp / HX, rx = hp - ry * HX;
    const int y = SY * y0 - 1 + ry, x = SY * x0 - 1 + rx;
    union {
      uint4 v;
      __half h[8];
    } q;
    q.v = make_uint4(0, 0, 0, 0);
    if (y >= 0 && y < hi && x >= 0 && x < wi) {
      const size_t base = (size_t)(8 * cg) * HW + (size_t)y * wi + x;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float v = __half2float(r[base + (size_t)j * HW]);
        if (st) v = (v - st[2 * (8 * cg + j)]) * st[2 * (8 * cg + j) + 1];
        v = fmaxf(v, 0.f);
        if (p) {
          float w = __half2float(p[base + (size_t)j * HW]);
          if (pst) w = (w - pst[2 * (8 * cg + j)]) * pst[2 * (8 * cg + j) + 1];
          v = fmaxf(w + v, 0.f);
        }
        q.h[j] = __float2half_rn(v);
      }
      if constexpr (SY == 1) {
        if (side && ry >= 1 && ry <= TY && rx >= 1 && rx <= kCtTX) {
#pragma unroll
          for (int j = 0; j < 8; ++j) side[base + (size_t)j * HW] = q.h[j];
        }
      }
    }
    *reinterpret_cast<uint4*>(s_x + hp * PS + 8 * cg) = q.v;
  }
}

// dynamic LDS: the staged tile.  grid (tiles, frames), 256 threads.
template <int CIN, int SY, int EPI>
__global__ __launch_bounds__(256) void k_be_conv(const BeArgs a) {
  constexpr int TY = be_ty(SY), CBW = TY / 4, PS = CIN + 8, HX = SY * kCtTX + 3 - SY, NKS = CIN / 32;
  constexpr int RBW = CIN == 32 ? 2 : 4;
  extern __shared__ uint4 s_be[];
  __half* __restrict__ s_x = reinterpret_cast<__half*>(s_be);
  const int t = threadIdx.x, lane = t & 63, wv = __builtin_amdgcn_readfirstlane(t >> 6);
  const int i = lane & 15, g = lane >> 4;
  const int b = blockIdx.y;
  const int ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
  const int x0 = tx * kCtTX, y0 = ty * TY;
  be_stage<CIN, SY>(s_x, a, b, x0, y0, t);
  __syncthreads();
  // the lane's pixel of the wave's first row at tap (0, 0), channels 8 g ..
  const __half* xlane = s_x + (SY * wv * CBW * HX + SY * i) * PS + 8 * g;
  const int nrb3 = a.rows3 / 16, nrb = nrb3 + a.rows1 / 16;
  const int pi = 4 * (int)blockIdx.x + wv;
#pragma unroll 1
  for (int rb0 = 0; rb0 < nrb; rb0 += RBW) {
    f32x4 acc[RBW][CBW];
#pragma unroll
    for (int rb = 0; rb < RBW; ++rb)
#pragma unroll
      for (int cb = 0; cb < CBW; ++cb) acc[rb][cb] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (rb0 < nrb3) {
      ct_taps<RBW, CBW, NKS, PS, HX, SY>(acc, xlane, a.w3 + (size_t)rb0 * 9 * NKS * kCtFrag + 8 * lane,
                                         (size_t)9 * NKS * kCtFrag, NKS, 0, NKS);
    } else {  // the centre tap only
      const __half* wtap = a.w1 + (size_t)(rb0 - nrb3) * NKS * kCtFrag + 8 * lane;
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks)
        ct_kstep<RBW, CBW, PS, HX, SY>(acc, xlane + (HX + 1) * PS, wtap, (size_t)NKS * kCtFrag, ks);
    }
    be_store<RBW, CBW, EPI>(acc, a.o, b, rb0, x0, y0 + wv * CBW, pi, lane);
  }
}

// grid (tiles, frames), 256 threads; T: the image's type
template <typename T>
__global__ __launch_bounds__(256) void k_be_stem(const StemArgs a) {
  constexpr int RBW = kBeStemRows / 16, CBW = kBeStemTY / 4;
  __shared__ __align__(16) __half s_img[kBeImgH * kBeImgRow];
  const int t = threadIdx.x, lane = t & 63, wv = __builtin_amdgcn_readfirstlane(t >> 6);
  const int i = lane & 15, g = lane >> 4;
  const int b = blockIdx.y;
  const int ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
  const int x0 = tx * kCtTX, y0 = ty * kBeStemTY;
  const size_t HW = (size_t)a.H * a.W;
  const T* __restrict__ src = reinterpret_cast<const T*>(a.img) + (size_t)b * 3 * HW;
  for (int u = t; u < kBeImgH * kBeImgW; u += 256) {
    const int ry = u / kBeImgW, rx = u - ry * kBeImgW;
    const int y = 2 * y0 - 3 + ry, x = 2 * x0 - 3 + rx;
    const bool inside = y >= 0 && y < a.H && x >= 0 && x < a.W;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      __half h = __float2half_rn(0.f);
      if (inside) {
        float v;
        if constexpr (sizeof(T) == 4)
          v = src[(size_t)c * HW + (size_t)y * a.W + x];
        else
          v = __half2float(src[(size_t)c * HW + (size_t)y * a.W + x]);
        if (a.mean) v = (v - a.mean[c]) / a.sd[c];
        h = __float2half_rn(v);
      }
      s_img[ry * kBeImgRow + 3 * rx + c] = h;
    }
  }
  __syncthreads();
  f32x4 acc[RBW][CBW];
#pragma unroll
  for (int rb = 0; rb < RBW; ++rb)
#pragma unroll
    for (int cb = 0; cb < CBW; ++cb) acc[rb][cb] = f32x4{0.f, 0.f, 0.f, 0.f};
  // output pixel (row, i) at product k = 21 ky + 3 kx + ci: staged (2 row + ky, 3 (2 i + kx) + ci)
  const __half* xlane = s_img + 2 * wv * CBW * kBeImgRow + 6 * i;
  const __half* __restrict__ wfrag = a.w + 8 * lane;
#pragma unroll
  for (int ks = 0; ks < kBeStemKS; ++ks) {
    f16x8 af[RBW], bf[CBW];
#pragma unroll
    for (int rb = 0; rb < RBW; ++rb)
      af[rb] = *reinterpret_cast<const f16x8*>(wfrag + (size_t)(rb * kBeStemKS + ks) * kCtFrag);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int k = min(32 * ks + 8 * g + j, kBeStemK - 1);  // (the weights past product 146 are zero)
      const int off = (k / 21) * kBeImgRow + k % 21;
#pragma unroll
      for (int cb = 0; cb < CBW; ++cb) bf[cb][j] = reinterpret_cast<const _Float16*>(xlane)[2 * cb * kBeImgRow + off];
    }
#pragma unroll
    for (int rb = 0; rb < RBW; ++rb)
#pragma unroll
      for (int cb = 0; cb < CBW; ++cb)
        acc[rb][cb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[rb], bf[cb], acc[rb][cb], 0, 0, 0);
  }
  be_store<RBW, CBW, kBeRaw>(acc, a.o, b, 0, x0, y0 + wv * CBW, 4 * (int)blockIdx.x + wv, lane);
}

// Chan's merge of (nb, mb, qb) into (n, m, q); an empty side leaves the other as it is
__device__ __forceinline__ void be_merge(float& n, float& m, float& q, float nb, float mb, float qb) {
  if (nb == 0.f) return;
  if (n == 0.f) {
    n = nb, m = mb, q = qb;
    return;
  }
  const float tot = n + nb, d = mb - m;
  m = m + d * (nb / tot);
  q = q + qb + d * d * (n * nb / tot);
  n = tot;
}

// grid (rows, frames), 64 threads: the partials of one (frame, channel) -> (mean, rstd)
__global__ __launch_bounds__(64) void k_be_stats(const float* __restrict__ part, float* __restrict__ stats, int rows,
                                                 int parts) {
  const int lane = threadIdx.x;
  const size_t e = (size_t)blockIdx.y * rows + blockIdx.x;
  const float* __restrict__ src = part + e * parts * 3;
  float n = 0.f, m = 0.f, q = 0.f;
  for (int p = lane; p < parts; p += 64) be_merge(n, m, q, src[3 * p], src[3 * p + 1], src[3 * p + 2]);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const float nb = __shfl_down(n, off, 64), mb = __shfl_down(m, off, 64), qb = __shfl_down(q, off, 64);
    if (lane + off < 64) be_merge(n, m, q, nb, mb, qb);
  }
  if (lane == 0) {
    stats[2 * e] = m;
    stats[2 * e + 1] = 1.f / sqrtf(q / n + kBeEps);
  }
}

int be_parts(int ho, int wo, int stride) {
  return 4 * ((wo + kCtTX - 1) / kCtTX) * ((ho + be_ty(stride) - 1) / be_ty(stride));
}

bool be_misaligned(const void* p) { return reinterpret_cast<uintptr_t>(p) & 15; }

template <int CIN, int SY, int EPI>
int be_launch(const char* who, BeArgs a, int n, hipStream_t s) {
  constexpr int TY = be_ty(SY);
  constexpr size_t lds = sizeof(__half) * (SY * kCtTX + 3 - SY) * (SY * TY + 3 - SY) * (CIN + 8);
  static_assert(lds <= 64 * 1024, "the staged tile fits the LDS a workgroup has without asking");
  if (const int e = ct_lds_ok(who, lds)) return e;
  a.tiles_x = (a.o.wo + kCtTX - 1) / kCtTX;
  const dim3 grid((unsigned)(a.tiles_x * ((a.o.ho + TY - 1) / TY)), (unsigned)n);
  hipLaunchKernelGGL((k_be_conv<CIN, SY, EPI>), grid, dim3(256), lds, s, a);
  return ct_err(who, hipGetLastError());
}

}  // namespace

}  // namespace wgsr

using namespace wgsr;

extern "C" {

int wgsr_droid_be_parts(int ho, int wo, int stride) {
  if (ho <= 0 || wo <= 0 || (stride != 1 && stride != 2)) return 0;
  return be_parts(ho, wo, stride);
}

int wgsr_droid_be_stem(const void* image, int image_dtype, const float* mean, const float* std_dev, const void* w,
                       const float* bias, void* out, float* part, int n, int H, int W, void* stream) {
  const char* who = "wgsr_droid_be_stem";
  if (H <= 0 || W <= 0) return set_error(WGSR_EINVAL, "%s: bad shape: %d x %d", who, H, W);
  const int ho = (H + 1) / 2, wo = (W + 1) / 2;
  if (const int e = ct_shape_ok(who, n, ho, wo)) return e;
  if (image_dtype != WGSR_DTYPE_F32 && image_dtype != WGSR_DTYPE_F16)
    return set_error(WGSR_EINVAL, "%s: image_dtype = %d is neither WGSR_DTYPE_F32 nor WGSR_DTYPE_F16", who,
                     image_dtype);
  if (n == 0) return WGSR_OK;
  if (!image || !w || !bias || !out || (mean != nullptr) != (std_dev != nullptr))
    return set_error(WGSR_EINVAL, "%s: null pointer (mean and std come together)", who);
  if (be_misaligned(w) || be_misaligned(bias))
    return set_error(WGSR_EINVAL, "%s: packed weights and biases must be 16-byte aligned", who);
  StemArgs a = {};
  a.img = image, a.mean = mean, a.sd = std_dev, a.w = (const __half*)w, a.H = H, a.W = W;
  a.tiles_x = (wo + kCtTX - 1) / kCtTX;
  a.o.bias = bias, a.o.out = (__half*)out, a.o.part = part, a.o.rows = kBeStemRows, a.o.ho = ho, a.o.wo = wo;
  a.o.parts = be_parts(ho, wo, 1);
  const dim3 grid((unsigned)(a.o.parts / 4), (unsigned)n);
  if (image_dtype == WGSR_DTYPE_F32)
    hipLaunchKernelGGL(k_be_stem<float>, grid, dim3(256), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(k_be_stem<__half>, grid, dim3(256), 0, (hipStream_t)stream, a);
  return ct_err(who, hipGetLastError());
}

int wgsr_droid_be_conv(const void* r, int64_t r_frame, const float* r_stats, int64_t r_stats_frame, const void* p,
                       int64_t p_frame, const float* p_stats, int64_t p_stats_frame, void* side, int c_in,
                       int stride, const void* w3, int rows3, const void* w1, int rows1, const float* bias,
                       int epilogue, void* out, void* out2, float* part, int n, int hi, int wi, void* stream) {
  const char* who = "wgsr_droid_be_conv";
  if (const int e = ct_shape_ok(who, n, hi, wi)) return e;
  const bool s2 = stride == 2;
  if (!((c_in == 32 || c_in == 64 || (c_in == 128 && !s2)) && (stride == 1 || s2)))
    return set_error(WGSR_EINVAL, "%s: c_in = %d at stride %d is not built (32, 64 and, at stride 1, 128)", who, c_in,
                     stride);
  const int chunk = c_in == 32 ? 32 : 64;
  if (rows3 < 0 || rows1 < 0 || rows3 + rows1 == 0 || rows3 % chunk || rows1 % chunk)
    return set_error(WGSR_EINVAL, "%s: rows3 = %d and rows1 = %d must be multiples of %d, one of them positive", who,
                     rows3, rows1, chunk);
  if (epilogue != kBeRaw && !(epilogue == kBeCnet && c_in == 128 && rows3 == 0 && rows1 == 256 && out2 && !part))
    return set_error(WGSR_EINVAL, "%s: epilogue %d: the split head is 256 rows of a 1 x 1 on 128 channels into two "
                     "tensors, without statistics", who, epilogue);
  if (n == 0) return WGSR_OK;
  if (!r || !out || !bias || (rows3 && !w3) || (rows1 && !w1) || (p_stats && !p))
    return set_error(WGSR_EINVAL, "%s: null pointer", who);
  if (side && s2) return set_error(WGSR_EINVAL, "%s: a side output needs stride 1", who);
  if (be_misaligned(w3) || be_misaligned(w1) || be_misaligned(bias))
    return set_error(WGSR_EINVAL, "%s: packed weights and biases must be 16-byte aligned", who);
  if (r_frame < 0 || r_stats_frame < 0 || p_frame < 0 || p_stats_frame < 0)
    return set_error(WGSR_EINVAL, "%s: negative frame stride", who);
  BeArgs a = {};
  a.r = (const __half*)r, a.st = r_stats, a.p = (const __half*)p, a.pst = p_stats;
  a.r_fs = (size_t)r_frame, a.st_fs = (size_t)r_stats_frame, a.p_fs = (size_t)p_frame, a.pst_fs = (size_t)p_stats_frame;
  a.side = (__half*)side, a.w3 = (const __half*)w3, a.w1 = (const __half*)w1, a.rows3 = rows3, a.rows1 = rows1;
  a.hi = hi, a.wi = wi;
  a.o.bias = bias, a.o.out = (__half*)out, a.o.out2 = (__half*)out2, a.o.part = part, a.o.rows = rows3 + rows1;
  a.o.ho = s2 ? (hi + 1) / 2 : hi, a.o.wo = s2 ? (wi + 1) / 2 : wi;
  a.o.parts = be_parts(a.o.ho, a.o.wo, stride);
  hipStream_t s = (hipStream_t)stream;
  if (epilogue == kBeCnet) return be_launch<128, 1, kBeCnet>(who, a, n, s);
  if (c_in == 32) return s2 ? be_launch<32, 2, kBeRaw>(who, a, n, s) : be_launch<32, 1, kBeRaw>(who, a, n, s);
  if (c_in == 64) return s2 ? be_launch<64, 2, kBeRaw>(who, a, n, s) : be_launch<64, 1, kBeRaw>(who, a, n, s);
  return be_launch<128, 1, kBeRaw>(who, a, n, s);
}

int wgsr_droid_be_stats(const float* part, float* stats, int n, int rows, int parts, void* stream) {
  const char* who = "wgsr_droid_be_stats";
  if (n < 0 || n > 65535 || rows <= 0 || parts <= 0)
    return set_error(WGSR_EINVAL, "%s: bad shape: %d frames of %d rows, %d partials", who, n, rows, parts);
  if (n == 0) return WGSR_OK;
  if (!part || !stats) return set_error(WGSR_EINVAL, "%s: null pointer", who);
  hipLaunchKernelGGL(k_be_stats, dim3((unsigned)rows, (unsigned)n), dim3(64), 0, (hipStream_t)stream, part, stats, rows,
                     parts);
  return ct_err(who, hipGetLastError());
}

}  // extern "C"
