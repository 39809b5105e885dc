// Convex upsampling of the tracker's disparities (cvx_upsample, droid_net.py:
// 23-37; DepthVideo.upsample, depth_video.py:179-183; wgsr.frontend.upsample)
// for gfx950, with and without the mask head computed in the launch.
//
// With pad the zero-padded coarse map [ht, wd, dim] of an entry,
//   up[8y+a, 8x+b, c] = sum_k softmax_k(mask[64k + 8a + b, y, x]) pad[y + k/3 - 1, x + k%3 - 1, c],
// k = 0..8.  Both kernels form the nine logits of one (pixel, a, b) as fp32
// values in registers and hand them to the same two functions (up_softmax,
// up_sum): the maximum is subtracted, e_k = exp(m_k - max) and their sum s are
// fp32, and the output is (sum_k e_k d_k) (1 / s) with explicit fmas in k
// order.  The weights are never rounded to fp16 and never reach memory.
//
// k_cvx_upsample (the mask given, [n, 576, ht, wd] fp16 or fp32): workgroup
//   <-> 64 consecutive pixels of one entry, thread <-> (pixel, a): lane <->
//   pixel makes each of the 72 loads of a thread one contiguous run per wave,
//   and the 8 dim results of a thread are 32 dim contiguous bytes of output row
//   8y + a that the next lane continues: float4 stores.
// k_upmask_upsample (the head fused in, dim = 1): logits [576, 32 pixels] =
//   weight [576, C] x feat [C, 32 pixels] by v_mfma_f32_16x16x32_f16 with the
//   channels as rows.  The feature tile is copied as it lies ([channel]
//   [pixel]) into LDS and read with ds_read_b64_tr_b16 (the idiom of
//   droid_corrvol.hip's cv_frag); a weight fragment is 16 contiguous bytes of
//   a weight row, read straight from memory (the weights stay in L2: 147 KB at
//   C = 128 per 32 pixels).  Channel 64k + 8a + b lies in the 16-channel tile
//   t = 4k + (8a + b) / 16, so wave q accumulates the nine tiles q, q + 4, ..,
//   q + 32: register i of lane l of tile 4k + q is the logit of neighbour k,
//   a = 2q + (l >> 5), b = 4 ((l >> 4) & 1) + i, pixel l & 15.  The nine
//   logits of a (pixel, a, b) are thus the same register of nine accumulators
//   of one lane, which adds the bias, rounds to fp16 (the value the
//   convolution hands on under autocast) and ends with four consecutive b: one
//   16-byte store.
//
// Index validation: every workgroup scans src_index / out_index (n entries)
// and returns before it writes when one is out of range, so a refused call
// leaves the output untouched; workgroup (0, 0) writes the status word.
#include <math.h>

#include "wgsr_common.h"
#include "wgsr_internal.h"
#include "droid_corr.h"

namespace wgsr {

namespace {

constexpr int kUpPix = 64;       // pixels per workgroup of k_cvx_upsample (lane <-> pixel)
constexpr int kUpMaskCh = 576;   // 9 neighbours x 8 x 8 sub-positions
constexpr int kUpMaxDim = 4;
constexpr int kUpK = 32;         // channels per MFMA step
constexpr int kUpMaxC = 512;
// The fused kernel's tile is 32 pixels: two accumulator groups of nine tiles
// per wave (72 accumulator registers, 130 in all) leave room for three
// workgroups per CU, so one workgroup's softmax runs beside another's MFMAs;
// every workgroup reads all of the weights from L2.  The launch bound names two
// waves per SIMD so that everything is allocated in the 256 architectural
// registers: left to a budget of 512 the compiler put the accumulators in
// AGPRs, rotated the loop through copies between the two files and gave MFMAs
// a srcC that partly overlapped their destination; with more than one wave on
// a SIMD a few 16-pixel groups per launch then came out wrong
// (tests/test_gpu_upsample.py::test_fused_head_with_every_cu_busy).
constexpr int kUpFPix = 32;
// feature image [C][kUpStride] fp16: 16-byte rows; 24 dwords = 8 x an odd
// number, so the rows q and q + 4 of a transposed read fall on different
// banks (rows q and q + 8 of a 32-lane half share theirs: 2-way)
constexpr int kUpStride = 48;

typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

struct UpWeights {
  float e[9];
  float inv;
};

__device__ __forceinline__ UpWeights up_softmax(const float (&m)[9]) {
  float mx = m[0];
#pragma unroll
  for (int k = 1; k < 9; ++k) mx = fmaxf(mx, m[k]);
  UpWeights w;
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    // exp(x), x <= 0, as v_exp_f32 of x log2(e): with a = -x log2(e) the rounded
    // product and constant put a relative error of about a 2^-24 on a weight
    // of 2^-a of the largest: under 2^-24 of the sum at every a (a 2^-a <=
    // 0.54), where libm's expf costs five times the instructions
    w.e[k] = __builtin_amdgcn_exp2f((m[k] - mx) * 1.44269504088896341f);
    s += w.e[k];
  }
  w.inv = 1.f / s;
  return w;
}

__device__ __forceinline__ float up_sum(const UpWeights& w, const float (&d)[9]) {
  float acc = w.e[0] * d[0];
#pragma unroll
  for (int k = 1; k < 9; ++k) acc = fmaf(w.e[k], d[k], acc);
  return acc * w.inv;
}

// The nine neighbours of pixel (y, x) of channel c of one frame [ht, wd, dim]; zero outside.
__device__ __forceinline__ void up_neighbours(const float* __restrict__ frame, int ht, int wd, int dim, int y, int x,
                                              int c, float (&d)[9]) {
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const int yy = y + k / 3 - 1, xx = x + k % 3 - 1;
    d[k] = (yy >= 0 && yy < ht && xx >= 0 && xx < wd) ? frame[((size_t)yy * wd + xx) * dim + c] : 0.f;
  }
}

// Every thread of the workgroup calls this.  True when every index lies in its
// range; `first` (workgroup-uniform): this workgroup writes the status word.
__device__ __forceinline__ bool up_indices_ok(const int64_t* __restrict__ src_index,
                                              const int64_t* __restrict__ out_index, int n, int n_src, int n_out,
                                              uint32_t* __restrict__ status, bool first, uint32_t* s_bad) {
  if (threadIdx.x == 0) *s_bad = 0u;
  __syncthreads();
  uint32_t bad = 0u;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    if (src_index) {
      const int64_t v = src_index[i];
      if (v < 0 || v >= n_src) bad |= WGSR_UPSAMPLE_BAD_SRC;
    }
    if (out_index) {
      const int64_t v = out_index[i];
      if (v < 0 || v >= n_out) bad |= WGSR_UPSAMPLE_BAD_OUT;
    }
  }
  if (bad) atomicOr(s_bad, bad);  // (LDS)
  __syncthreads();
  const uint32_t st = *s_bad;
  if (first && threadIdx.x == 0) *status = st;
  return st == 0u;
}

template <class M, int DIM>
__global__ __launch_bounds__(8 * kUpPix) void k_cvx_upsample(const float* __restrict__ data,
                                                            const int64_t* __restrict__ src_index,
                                                            const M* __restrict__ mask, float* __restrict__ out,
                                                            const int64_t* __restrict__ out_index, int n, int n_src,
                                                            int n_out, int ht, int wd, uint32_t* __restrict__ status) {
  __shared__ uint32_t s_bad;
  const int e = blockIdx.y;
  if (!up_indices_ok(src_index, out_index, n, n_src, n_out, status, blockIdx.x == 0 && e == 0, &s_bad)) return;
  const int HW = ht * wd;
  const int p = blockIdx.x * kUpPix + (threadIdx.x & 63), a = threadIdx.x >> 6;
  if (p >= HW) return;
  const int y = p / wd, x = p - y * wd;
  const size_t fi = src_index ? (size_t)src_index[e] : (size_t)e;
  const size_t fo = out_index ? (size_t)out_index[e] : (size_t)e;
  float d[DIM][9];
#pragma unroll
  for (int c = 0; c < DIM; ++c) up_neighbours(data + fi * HW * DIM, ht, wd, DIM, y, x, c, d[c]);
  const M* __restrict__ mp = mask + ((size_t)e * kUpMaskCh + 8 * a) * HW + p;
  float m[8][9];
#pragma unroll
  for (int b = 0; b < 8; ++b)
#pragma unroll
    for (int k = 0; k < 9; ++k) m[b][k] = to_f32(mp[(size_t)(64 * k + b) * HW]);
  float r[8 * DIM];
#pragma unroll
  for (int b = 0; b < 8; ++b) {
    const UpWeights w = up_softmax(m[b]);
#pragma unroll
    for (int c = 0; c < DIM; ++c) r[b * DIM + c] = up_sum(w, d[c]);
  }
  // row 8y + a of the frame, columns 8x .. 8x + 7: 8 DIM floats, 32 DIM bytes from a 32-byte boundary
  float4* __restrict__ o = reinterpret_cast<float4*>(out + (fo * 64 * HW + ((size_t)(8 * y + a) * 8 * wd + 8 * x)) * DIM);
#pragma unroll
  for (int v = 0; v < 2 * DIM; ++v) o[v] = make_float4(r[4 * v], r[4 * v + 1], r[4 * v + 2], r[4 * v + 3]);
}

// The MFMA operand of 16 pixels (columns c0 .. c0 + 15 of the [channel][pixel]
// image) for channels k0 .. k0 + 31: lane <-> pixel lane & 15, channels
// k0 + 8 (lane >> 4) + 0 .. 7.  Every lane of the wave must be active.
__device__ __forceinline__ f16x8 up_frag(const __half* img, int c0, int k0, int lane) {
  const int g = lane >> 4, i = lane & 15, q = i >> 2, p = i & 3;
  const __half* a = img + (k0 + 8 * g + q) * kUpStride + c0 + 4 * p;
  typedef __attribute__((address_space(3))) s16x4* lds_ptr;
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)(a));
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)(a + 4 * kUpStride));
  return __builtin_bit_cast(f16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}

// dynamic LDS (16-byte aligned): the feature image [C][kUpStride] fp16, then the validation word.
// VEC: 16-byte moves into the image (HW a multiple of 8, feat 16-byte aligned).
template <bool VEC>
__global__ __launch_bounds__(256, 2) void k_upmask_upsample(const __half* __restrict__ feat,
                                                         const __half* __restrict__ weight,
                                                         const float* __restrict__ bias, int C,
                                                         const float* __restrict__ disps,
                                                         const int64_t* __restrict__ src_index,
                                                         float* __restrict__ out,
                                                         const int64_t* __restrict__ out_index, int n, int n_src,
                                                         int n_out, int ht, int wd, uint32_t* __restrict__ status) {
  extern __shared__ uint4 s_up[];
  __half* __restrict__ s_f = reinterpret_cast<__half*>(s_up);
  uint32_t* s_bad = reinterpret_cast<uint32_t*>(s_f + C * kUpStride);
  const int e = blockIdx.y;
  if (!up_indices_ok(src_index, out_index, n, n_src, n_out, status, blockIdx.x == 0 && e == 0, s_bad)) return;
  const int t = threadIdx.x, q = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63;
  const int HW = ht * wd, p0 = blockIdx.x * kUpFPix;
  const __half* __restrict__ f = feat + (size_t)e * C * HW;
  // the tile's pixels [p0, p0 + 32) of every channel; zero at and past HW
  if constexpr (VEC) {
    for (int u = t; u < C * (kUpFPix / 8); u += 256) {
      const int k = u >> 2, c = (u & 3) << 3;
      uint4 v = make_uint4(0, 0, 0, 0);
      if (p0 + c < HW) v = *reinterpret_cast<const uint4*>(f + (size_t)k * HW + p0 + c);
      *reinterpret_cast<uint4*>(s_f + k * kUpStride + c) = v;
    }
  } else {
    for (int u = t; u < C * kUpFPix; u += 256) {
      const int k = u >> 5, c = u & 31;
      s_f[k * kUpStride + c] = p0 + c < HW ? f[(size_t)k * HW + p0 + c] : __float2half_rn(0.f);
    }
  }
  __syncthreads();

  // acc[g][k]: pixels 16 g .. 16 g + 15 (columns) x the 16 channels of tile 4 k + q (rows)
  f32x4 acc[kUpFPix / 16][9];
#pragma unroll
  for (int g = 0; g < kUpFPix / 16; ++g)
#pragma unroll
    for (int k = 0; k < 9; ++k) acc[g][k] = f32x4{0.f, 0.f, 0.f, 0.f};
  // this lane's 8 channels of row 16 (4 k + q) + (lane & 15) of the weights
  const __half* __restrict__ wrow = weight + (size_t)(16 * q + (lane & 15)) * C + 8 * (lane >> 4);
  for (int k0 = 0; k0 < C; k0 += kUpK) {
    f16x8 wf[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) wf[k] = *reinterpret_cast<const f16x8*>(wrow + (size_t)64 * k * C + k0);
#pragma unroll
    for (int g = 0; g < kUpFPix / 16; ++g) {
      const f16x8 ff = up_frag(s_f, 16 * g, k0, lane);
#pragma unroll
      for (int k = 0; k < 9; ++k) acc[g][k] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[k], ff, acc[g][k], 0, 0, 0);
    }
  }

  // D: row (channel of the tile) 4 (lane >> 4) + i in register i, column (pixel) lane & 15
  const int sub = 16 * q + 4 * (lane >> 4);  // 8 a + b of register 0
  const int a = sub >> 3, b0 = sub & 7;
  float4 bs[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) bs[k] = *reinterpret_cast<const float4*>(bias + 64 * k + sub);
  const size_t fi = src_index ? (size_t)src_index[e] : (size_t)e;
  const size_t fo = out_index ? (size_t)out_index[e] : (size_t)e;
#pragma unroll
  for (int g = 0; g < kUpFPix / 16; ++g) {
    const int p = p0 + 16 * g + (lane & 15);
    if (p >= HW) continue;
    const int y = p / wd, x = p - y * wd;
    float d[9];
    up_neighbours(disps + fi * HW, ht, wd, 1, y, x, 0, d);
    float r[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float m[9];
#pragma unroll
      for (int k = 0; k < 9; ++k) {
        const float bk = i == 0 ? bs[k].x : i == 1 ? bs[k].y : i == 2 ? bs[k].z : bs[k].w;
        m[k] = __half2float(__float2half_rn(acc[g][k][i] + bk));
      }
      r[i] = up_sum(up_softmax(m), d);
    }
    *reinterpret_cast<float4*>(out + fo * 64 * HW + (size_t)(8 * y + a) * 8 * wd + 8 * x + b0) =
        make_float4(r[0], r[1], r[2], r[3]);
  }
}

// the checks the entry points share; 0 or an error code
int upsample_args_ok(const char* who, const void* src, const int64_t* src_index, const float* out,
                     const int64_t* out_index, int n, int n_src, int n_out, int ht, int wd, const uint32_t* status) {
  if (n < 0 || n > 65535 || n_src < 0 || n_out < 0 || ht <= 0 || wd <= 0 || (int64_t)ht * wd >= (int64_t(1) << 20))
    return set_error(WGSR_EINVAL, "%s: bad shape n=%d n_src=%d n_out=%d ht=%d wd=%d", who, n, n_src, n_out, ht, wd);
  if (!src_index && n > n_src)
    return set_error(WGSR_EINVAL, "%s: n=%d entries but n_src=%d frames and no src_index", who, n, n_src);
  if (!out_index && n > n_out)
    return set_error(WGSR_EINVAL, "%s: n=%d entries but n_out=%d frames and no out_index", who, n, n_out);
  if (!status) return set_error(WGSR_EINVAL, "%s: null status", who);
  if (n == 0) return WGSR_OK;
  if (!src || !out) return set_error(WGSR_EINVAL, "%s: null pointer", who);
  if (reinterpret_cast<uintptr_t>(out) & 15) return set_error(WGSR_EINVAL, "%s: out must be 16-byte aligned", who);
  return WGSR_OK;
}

template <class M>
void launch_cvx(int dim, dim3 grid, hipStream_t s, const float* data, const int64_t* src_index, const void* mask,
                float* out, const int64_t* out_index, int n, int n_src, int n_out, int ht, int wd, uint32_t* status) {
  const dim3 block(8 * kUpPix);
  const M* m = (const M*)mask;
  switch (dim) {
    case 1: hipLaunchKernelGGL((k_cvx_upsample<M, 1>), grid, block, 0, s, data, src_index, m, out, out_index, n, n_src, n_out, ht, wd, status); break;
    case 2: hipLaunchKernelGGL((k_cvx_upsample<M, 2>), grid, block, 0, s, data, src_index, m, out, out_index, n, n_src, n_out, ht, wd, status); break;
    case 3: hipLaunchKernelGGL((k_cvx_upsample<M, 3>), grid, block, 0, s, data, src_index, m, out, out_index, n, n_src, n_out, ht, wd, status); break;
    default: hipLaunchKernelGGL((k_cvx_upsample<M, 4>), grid, block, 0, s, data, src_index, m, out, out_index, n, n_src, n_out, ht, wd, status); break;
  }
}

}  // namespace

}  // namespace wgsr

using namespace wgsr;

extern "C" {

int wgsr_droid_cvx_upsample(const float* data, const int64_t* src_index, const void* mask, int mask_dtype, float* out,
                            const int64_t* out_index, int n, int n_src, int n_out, int ht, int wd, int dim,
                            uint32_t* status, void* stream) {
  const char* who = "wgsr_droid_cvx_upsample";
  if (mask_dtype != WGSR_DTYPE_F32 && mask_dtype != WGSR_DTYPE_F16)
    return set_error(WGSR_EINVAL, "%s: unknown mask dtype tag %d", who, mask_dtype);
  if (dim < 1 || dim > kUpMaxDim) return set_error(WGSR_EINVAL, "%s: dim %d outside [1, %d]", who, dim, kUpMaxDim);
  if (const int e = upsample_args_ok(who, data, src_index, out, out_index, n, n_src, n_out, ht, wd, status)) return e;
  hipStream_t s = (hipStream_t)stream;
  if (n == 0) {  // (no launch: the status word still has to say so)
    const hipError_t e = hipMemsetAsync(status, 0, sizeof(uint32_t), s);
    return e == hipSuccess ? WGSR_OK : set_error(WGSR_EHIP, "%s: %s", who, hipGetErrorString(e));
  }
  if (!mask) return set_error(WGSR_EINVAL, "%s: null pointer", who);
  const dim3 grid((unsigned)((ht * wd + kUpPix - 1) / kUpPix), (unsigned)n);
  if (mask_dtype == WGSR_DTYPE_F16)
    launch_cvx<__half>(dim, grid, s, data, src_index, mask, out, out_index, n, n_src, n_out, ht, wd, status);
  else
    launch_cvx<float>(dim, grid, s, data, src_index, mask, out, out_index, n, n_src, n_out, ht, wd, status);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? WGSR_OK : set_error(WGSR_EHIP, "%s: %s", who, hipGetErrorString(e));
}

int wgsr_droid_upmask_upsample(const void* feat, const void* weight, const float* bias, int C, const float* disps,
                               const int64_t* src_index, float* out, const int64_t* out_index, int n, int n_src,
                               int n_out, int ht, int wd, uint32_t* status, void* stream) {
  const char* who = "wgsr_droid_upmask_upsample";
  if (C <= 0 || C % kUpK != 0 || C > kUpMaxC)
    return set_error(WGSR_EINVAL, "%s: the channel count C=%d must be a multiple of %d in [%d, %d]", who, C, kUpK, kUpK,
                     kUpMaxC);
  if (const int e = upsample_args_ok(who, disps, src_index, out, out_index, n, n_src, n_out, ht, wd, status)) return e;
  hipStream_t s = (hipStream_t)stream;
  if (n == 0) {
    const hipError_t e = hipMemsetAsync(status, 0, sizeof(uint32_t), s);
    return e == hipSuccess ? WGSR_OK : set_error(WGSR_EHIP, "%s: %s", who, hipGetErrorString(e));
  }
  if (!feat || !weight || !bias) return set_error(WGSR_EINVAL, "%s: null pointer", who);
  if ((reinterpret_cast<uintptr_t>(weight) | reinterpret_cast<uintptr_t>(bias)) & 15)
    return set_error(WGSR_EINVAL, "%s: weight and bias must be 16-byte aligned", who);
  const int HW = ht * wd;
  const dim3 grid((unsigned)((HW + kUpFPix - 1) / kUpFPix), (unsigned)n);
  const size_t lds = sizeof(__half) * (size_t)C * kUpStride + 16;
  const __half* f = (const __half*)feat;
  const __half* w = (const __half*)weight;
  if (HW % 8 == 0 && (reinterpret_cast<uintptr_t>(feat) & 15) == 0)
    hipLaunchKernelGGL(k_upmask_upsample<true>, grid, dim3(256), lds, s, f, w, bias, C, disps, src_index, out,
                       out_index, n, n_src, n_out, ht, wd, status);
  else
    hipLaunchKernelGGL(k_upmask_upsample<false>, grid, dim3(256), lds, s, f, w, bias, C, disps, src_index, out,
                       out_index, n, n_src, n_out, ht, wd, status);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? WGSR_OK : set_error(WGSR_EHIP, "%s: %s", who, hipGetErrorString(e));
}

}  // extern "C"
