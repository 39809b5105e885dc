// The 3 x 3 convolutions after the ConvGRU in the tracker's update operator
// (UpdateModule.delta / .weight, droid_net.py:102-115, 141-145; GraphAgg.forward
// up to eta and the features of upmask, droid_net.py:65-77) for gfx950:
// wgsr_droid_conv3x3_relu, wgsr_droid_update_heads, wgsr_droid_graph_agg.
//
// One implicit-GEMM kernel, k_conv3x3: padding 1, stride 1, C_in = 128, input
// [n, 128, ht, wd] fp16 as the reference hands it around (NCHW),
//   D[co, pixel] = sum_{tap, ci} W[co, ci, tap] X[ci, pixel + tap],
// by v_mfma_f32_16x16x32_f16 with the output channels as rows (A = weights,
// B = input, fp32 accumulation), fp32 bias, the epilogue in fp32.  The tile of
// 16 x TY pixels, its staging into LDS, the packed weights (here KS = 4) and
// the tap x K-step loop are those of droid_conv_tile.h; TY = 8 (4 for the
// group mean, below), all 128 channels staged at once.
//
//   big  (RBW = 4, CBW = 4): wave <-> 4 row blocks (64 output channels) x 4 tile
//        rows; the workgroup covers 128 output channels per pass and loops
//        over passes of 128 (the heads' 256-row hidden layer: two passes over
//        one staged tile).  16 MFMAs per 4 weight + 4 LDS fragments.
//   head (RBW = 1, CBW = 2): C_out in {1, 2} padded to one 16-row block; wave
//        <-> 2 tile rows.  15/16 (7/8) of the block's rows are padding.
//   mean (RBW = 2, CBW = 4, TY = 4): wave <-> 2 row blocks x the 4 tile rows.  A
//        workgroup of the group mean works through its group's edges one after
//        the other, so the launch has only groups x tiles workgroups: with 16 x
//        8 tiles 12 frames of 48 x 64 are 288 workgroups on 256 CUs, one per CU
//        and a second round for 32 of them; 16 x 4 tiles make 576 that are all
//        resident (29 KB of LDS, 122 VGPRs) and hide each other's staging:
//        measured 541 -> 225 us per graph_agg call at 96 edges.
//
// Epilogues (compile time):
//   kRelu16  fp16(ReLU(conv + bias)) -> [n, C_out, ht, wd]
//   kMean16  workgroup <-> (group, tile): the edges e with ix[e] == group in
//            ascending e, each staged and convolved in turn, ReLU(conv + bias)
//            added in fp32 to the lane's own sums, x 1 / count, one rounding ->
//            [G, C_out, ht, wd] fp16.  No atomics: the sum of a (group, pixel,
//            channel) is formed by one lane in a fixed order.  An empty group
//            writes zeros.  The edge list is the scan of ix itself (n 8-byte
//            loads per edge visit, against 1152 x 128 MACs per pixel).
//   kHead32  act(conv + bias), act = identity | sigmoid | 0.01 softplus
//            (threshold 20), fp32, channels last [n, ht, wd, C_out]; not
//            rounded to fp16, which is more exact than autocast.
//
// The bias is fp32 [16 R], zero past C_out.
//
// Index validation (graph_agg): every workgroup of every launch scans ix and
// returns before it writes when an entry is outside [0, G); workgroup (0, 0)
// writes the status word.
#include <hip/hip_fp16.h>
#include <math.h>

#include "droid_conv_tile.h"

namespace wgsr {

namespace {

constexpr int kCvCin = kCtC;                          // C_in: the whole tile is staged at once
constexpr int kCvKS = kCvCin / 32;                    // K-steps per (row block, tap)
constexpr int kCvFragsPerRb = 9 * kCvKS;              // taps x K-steps

enum { kRelu16 = 0, kMean16 = 1, kHead32 = 2 };
enum { kActNone = 0, kActSigmoid = 1, kActEta = 2 };

struct ConvArgs {
  const __half* in;       // [batch, >= 128 channels, ht, wd]: channel 0 of entry 0
  int64_t in_bstride;     // halfs between two entries
  const __half* w;        // packed
  const float* b;         // [c_out_pad]
  int c_out, c_out_pad;
  void* out;
  const int64_t* ix;      // [n], validated against [0, G) when status is given; kMean16: the group of each edge
  int n, G;
  int ht, wd, tiles_x;
  uint32_t* status;       // null: no validation
};

template <int ACT>
__device__ __forceinline__ float cv_act(float v) {
  if constexpr (ACT == kActSigmoid) return 1.f / (1.f + expf(-v));
  if constexpr (ACT == kActEta) return 0.01f * (v > 20.f ? v : log1pf(expf(v)));
  return v;
}

// dynamic LDS: ct_lds(ct_halo(TY)), the staged tile and the validation word.
// grid (tiles, entries or groups), 256 threads.  Two waves per SIMD: everything in the 256
// architectural registers (droid_upsample.hip on why).
template <int RBW, int CBW, int TY, int EPI, int ACT>
__global__ __launch_bounds__(256, 2) void k_conv3x3(const ConvArgs a) {
  extern __shared__ uint4 s_cv[];
  __half* __restrict__ s_x = reinterpret_cast<__half*>(s_cv);
  uint32_t* s_bad = reinterpret_cast<uint32_t*>(s_x + ct_halo(TY) * kCtStride);
  const int t = threadIdx.x, lane = t & 63, wv = __builtin_amdgcn_readfirstlane(t >> 6);
  if (a.status &&
      ct_bad_ix(s_bad, a.ix, a.n, a.G, WGSR_GRAPH_AGG_BAD_IX, a.status, blockIdx.x == 0 && blockIdx.y == 0, t))
    return;
  constexpr int WP = TY / CBW;     // waves along the tile's rows
  constexpr int WC = 4 / WP;       // waves along the output channels
  constexpr int PASS_RB = RBW * WC;
  static_assert(WP * WC == 4 && WP * CBW == TY, "four waves cover the tile");
  const int wp = wv % WP, wc = wv / WP;
  const int i = lane & 15, g = lane >> 4;
  const int b = blockIdx.y;
  const int ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
  const int x0 = tx * kCtTX, y0 = ty * TY;
  const int ht = a.ht, wd = a.wd;
  const int x = x0 + i;
  // pixel (tile row wp CBW, column i) at tap (0, 0), channels 8 g ..
  const __half* xlane = s_x + (wp * CBW * kCtHX + i) * kCtStride + 8 * g;

  if constexpr (EPI != kMean16) {
    ct_stage<TY>(s_x, a.in + (size_t)b * a.in_bstride, kCvCin, x0, y0, ht, wd, t);
    __syncthreads();
  }
  const int passes = a.c_out_pad / (16 * PASS_RB);
  for (int ps = 0; ps < passes; ++ps) {
    const int rb0 = ps * PASS_RB + wc * RBW;  // this wave's first row block
    float4 bias[RBW];
#pragma unroll
    for (int rb = 0; rb < RBW; ++rb) bias[rb] = *reinterpret_cast<const float4*>(a.b + 16 * (rb0 + rb) + 4 * g);
    const __half* __restrict__ wfrag = a.w + (size_t)rb0 * kCvFragsPerRb * kCtFrag + 8 * lane;

    f32x4 sum[RBW][CBW];
    int count = 0;
    if constexpr (EPI == kMean16) {
#pragma unroll
      for (int rb = 0; rb < RBW; ++rb)
#pragma unroll
        for (int cb = 0; cb < CBW; ++cb) sum[rb][cb] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const int e_begin = EPI == kMean16 ? 0 : b, e_end = EPI == kMean16 ? a.n : b + 1;
    for (int e = e_begin; e < e_end; ++e) {
      if constexpr (EPI == kMean16) {
        if (a.ix[e] != (int64_t)b) continue;  // (workgroup-uniform)
        ++count;
        __syncthreads();  // every wave is done with the edge staged before
        ct_stage<TY>(s_x, a.in + (size_t)e * a.in_bstride, kCvCin, x0, y0, ht, wd, t);
        __syncthreads();
      }
      f32x4 acc[RBW][CBW];
#pragma unroll
      for (int rb = 0; rb < RBW; ++rb)
#pragma unroll
        for (int cb = 0; cb < CBW; ++cb) acc[rb][cb] = f32x4{0.f, 0.f, 0.f, 0.f};
      ct_taps<RBW, CBW, kCvKS>(acc, xlane, wfrag, (size_t)kCvFragsPerRb * kCtFrag, kCvKS, 0, kCvKS);
      // D: row (output channel of the block) 4 g + r in register r, column (pixel of the tile row) i
      if constexpr (EPI == kMean16) {
#pragma unroll
        for (int rb = 0; rb < RBW; ++rb)
#pragma unroll
          for (int cb = 0; cb < CBW; ++cb) {
            sum[rb][cb][0] += fmaxf(acc[rb][cb][0] + bias[rb].x, 0.f);
            sum[rb][cb][1] += fmaxf(acc[rb][cb][1] + bias[rb].y, 0.f);
            sum[rb][cb][2] += fmaxf(acc[rb][cb][2] + bias[rb].z, 0.f);
            sum[rb][cb][3] += fmaxf(acc[rb][cb][3] + bias[rb].w, 0.f);
          }
      } else if constexpr (EPI == kRelu16) {
        __half* __restrict__ out = reinterpret_cast<__half*>(a.out);
#pragma unroll
        for (int cb = 0; cb < CBW; ++cb) {
          const int y = y0 + wp * CBW + cb;
          if (y >= ht || x >= wd) continue;
#pragma unroll
          for (int rb = 0; rb < RBW; ++rb) {
            const float bs[4] = {bias[rb].x, bias[rb].y, bias[rb].z, bias[rb].w};
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int co = 16 * (rb0 + rb) + 4 * g + r;
              if (co < a.c_out)
                out[(((size_t)b * a.c_out + co) * ht + y) * wd + x] = __float2half_rn(fmaxf(acc[rb][cb][r] + bs[r], 0.f));
            }
          }
        }
      } else {
        static_assert(EPI != kHead32 || (RBW == 1 && WC == 1), "a head is one row block");
        float* __restrict__ out = reinterpret_cast<float*>(a.out);
        const float bs[4] = {bias[0].x, bias[0].y, bias[0].z, bias[0].w};
#pragma unroll
        for (int cb = 0; cb < CBW; ++cb) {
          const int y = y0 + wp * CBW + cb;
          if (y >= ht || x >= wd || g != 0) continue;  // rows 0 .. 3 of the block are lanes 0 .. 15
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (r < a.c_out) out[(((size_t)b * ht + y) * wd + x) * a.c_out + r] = cv_act<ACT>(acc[0][cb][r] + bs[r]);
        }
      }
    }
    if constexpr (EPI == kMean16) {
      __half* __restrict__ out = reinterpret_cast<__half*>(a.out);
      const float inv = count ? 1.f / (float)count : 0.f;
#pragma unroll
      for (int cb = 0; cb < CBW; ++cb) {
        const int y = y0 + wp * CBW + cb;
        if (y >= ht || x >= wd) continue;
#pragma unroll
        for (int rb = 0; rb < RBW; ++rb)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int co = 16 * (rb0 + rb) + 4 * g + r;
            if (co < a.c_out)
              out[(((size_t)b * a.c_out + co) * ht + y) * wd + x] = __float2half_rn(sum[rb][cb][r] * inv);
          }
      }
    }
  }
}

constexpr size_t kCvLds = ct_lds(ct_halo(8));  // the largest tile

int cv_aligned(const char* who, const void* w, const void* b) {
  if (!w || !b) return set_error(WGSR_EINVAL, "%s: null pointer", who);
  if ((reinterpret_cast<uintptr_t>(w) | reinterpret_cast<uintptr_t>(b)) & 15)
    return set_error(WGSR_EINVAL, "%s: packed weights and bias must be 16-byte aligned", who);
  return WGSR_OK;
}

// One launch over `batch` maps (or groups); the arguments have been checked.
template <int RBW, int CBW, int TY, int EPI, int ACT>
int cv_launch(const char* who, ConvArgs a, int batch, hipStream_t s) {
  a.tiles_x = (a.wd + kCtTX - 1) / kCtTX;
  a.c_out_pad = (a.c_out + 15) / 16 * 16;
  constexpr int pass_rows = 16 * RBW * (4 / (TY / CBW));
  if (a.c_out_pad % pass_rows != 0)
    return set_error(WGSR_EINVAL, "%s: %d output rows are no multiple of %d", who, a.c_out_pad, pass_rows);
  const dim3 grid((unsigned)(a.tiles_x * ((a.ht + TY - 1) / TY)), (unsigned)batch);
  hipLaunchKernelGGL((k_conv3x3<RBW, CBW, TY, EPI, ACT>), grid, dim3(256), ct_lds(ct_halo(TY)), s, a);
  return ct_err(who, hipGetLastError());
}

}  // namespace

}  // namespace wgsr

using namespace wgsr;

extern "C" {

int wgsr_droid_conv3x3_relu(const void* x, const void* w_packed, const float* b_packed, int c_out, void* out, int n,
                            int ht, int wd, void* stream) {
  const char* who = "wgsr_droid_conv3x3_relu";
  if (const int e = ct_shape_ok(who, n, ht, wd)) return e;
  if (c_out <= 0 || c_out % 128 != 0)
    return set_error(WGSR_EINVAL, "%s: C_out = %d must be a positive multiple of 128", who, c_out);
  if (n == 0) return WGSR_OK;
  if (!x || !out) return set_error(WGSR_EINVAL, "%s: null pointer", who);
  if (const int e = cv_aligned(who, w_packed, b_packed)) return e;
  if (const int e = ct_lds_ok(who, kCvLds)) return e;
  ConvArgs a = {};
  a.in = (const __half*)x, a.in_bstride = (int64_t)kCvCin * ht * wd;
  a.w = (const __half*)w_packed, a.b = b_packed, a.c_out = c_out, a.out = out;
  a.n = n, a.ht = ht, a.wd = wd;
  return cv_launch<4, 4, 8, kRelu16, kActNone>(who, a, n, (hipStream_t)stream);
}

int wgsr_droid_update_heads(const void* net, const void* hidden_w, const float* hidden_b, const void* delta_w,
                            const float* delta_b, const void* weight_w, const float* weight_b, void* hidden,
                            float* delta, float* weight, int n, int ht, int wd, void* stream) {
  const char* who = "wgsr_droid_update_heads";
  if (const int e = ct_shape_ok(who, n, ht, wd)) return e;
  if (n == 0) return WGSR_OK;
  if (!net || !hidden || !delta || !weight) return set_error(WGSR_EINVAL, "%s: null pointer", who);
  if (const int e = cv_aligned(who, hidden_w, hidden_b)) return e;
  if (const int e = cv_aligned(who, delta_w, delta_b)) return e;
  if (const int e = cv_aligned(who, weight_w, weight_b)) return e;
  if (const int e = ct_lds_ok(who, kCvLds)) return e;
  hipStream_t s = (hipStream_t)stream;
  const int64_t HW = (int64_t)ht * wd;
  ConvArgs a = {};
  a.n = n, a.ht = ht, a.wd = wd;
  // both hidden layers in one launch: rows 0 .. 127 delta.0, rows 128 .. 255 weight.0
  a.in = (const __half*)net, a.in_bstride = kCvCin * HW;
  a.w = (const __half*)hidden_w, a.b = hidden_b, a.c_out = 2 * kCvCin, a.out = hidden;
  if (const int e = cv_launch<4, 4, 8, kRelu16, kActNone>(who, a, n, s)) return e;
  a.in_bstride = 2 * kCvCin * HW, a.c_out = 2;
  a.in = (const __half*)hidden, a.w = (const __half*)delta_w, a.b = delta_b, a.out = delta;
  if (const int e = cv_launch<1, 2, 8, kHead32, kActNone>(who, a, n, s)) return e;
  a.in = (const __half*)hidden + kCvCin * HW, a.w = (const __half*)weight_w, a.b = weight_b, a.out = weight;
  return cv_launch<1, 2, 8, kHead32, kActSigmoid>(who, a, n, s);
}

int wgsr_droid_graph_agg(const void* net, const int64_t* ix, int n, int G, const void* conv1_w, const float* conv1_b,
                         const void* conv2_w, const float* conv2_b, const void* eta_w, const float* eta_b,
                         void* mean, void* feat, float* eta, int ht, int wd, uint32_t* status, void* stream) {
  const char* who = "wgsr_droid_graph_agg";
  if (const int e = ct_shape_ok(who, n, ht, wd)) return e;
  if (const int e = ct_shape_ok(who, G, ht, wd)) return e;
  if (!status) return set_error(WGSR_EINVAL, "%s: null status", who);
  hipStream_t s = (hipStream_t)stream;
  if (G == 0) {  // (no launch: the status word still has to say so)
    if (n) return set_error(WGSR_EINVAL, "%s: n=%d edges but G=0 groups", who, n);
    return ct_err(who, hipMemsetAsync(status, 0, sizeof(uint32_t), s));
  }
  if ((n && (!net || !ix)) || !mean || !feat || !eta) return set_error(WGSR_EINVAL, "%s: null pointer", who);
  if (const int e = cv_aligned(who, conv1_w, conv1_b)) return e;
  if (const int e = cv_aligned(who, conv2_w, conv2_b)) return e;
  if (const int e = cv_aligned(who, eta_w, eta_b)) return e;
  if (const int e = ct_lds_ok(who, kCvLds)) return e;
  const int64_t HW = (int64_t)ht * wd;
  ConvArgs a = {};
  a.ix = ix, a.n = n, a.G = G, a.ht = ht, a.wd = wd, a.status = status;
  a.in_bstride = kCvCin * HW, a.c_out = kCvCin;
  a.in = (const __half*)net, a.w = (const __half*)conv1_w, a.b = conv1_b, a.out = mean;
  if (const int e = cv_launch<2, 4, 4, kMean16, kActNone>(who, a, G, s)) return e;
  a.in = (const __half*)mean, a.w = (const __half*)conv2_w, a.b = conv2_b, a.out = feat;
  if (const int e = cv_launch<4, 4, 8, kRelu16, kActNone>(who, a, G, s)) return e;
  a.in = (const __half*)feat, a.w = (const __half*)eta_w, a.b = eta_b, a.c_out = 1, a.out = eta;
  return cv_launch<1, 2, 8, kHead32, kActEta>(who, a, G, s);
}

}  // extern "C"
