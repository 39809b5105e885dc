// The ConvGRU of the tracker's update operator (gru.py:34-48, called at
// droid_net.py:138 as self.gru(net, inp, corr, flow)) for gfx950: wgsr_droid_gru.
//
//   glo  = mean over the pixels of an edge of sigmoid(w(net)) * net        [n, 128]
//   z    = sigmoid(convz([net, inp, corr, flow])     + convz_glo(glo))
//   r    = sigmoid(convr([net, inp, corr, flow])     + convr_glo(glo))
//   q    = tanh   (convq([r * net, inp, corr, flow]) + convq_glo(glo))
//   net' = (1 - z) * net + z * q
//
// Four launches.  fp32 everywhere inside a launch; exactly three fp16
// rounding points, the activations that go to memory: z, rnet = r * net, net'.
//
// k_gru_glo_part, workgroup <-> (chunk of 128 pixels, edge).  The 1 x 1
// convolution w by v_mfma_f32_16x16x32_f16 on the chunk staged [pixel][channel]
// (the layout of k_conv3x3), sigmoid(. + bias) x net (net from the staged
// chunk) summed in fp32 by the lane over its 8 pixel blocks, the 16 lanes of a
// row reduced by four xor-shuffles: the chunk's sums, fp32 [n, chunks, 128] in
// the caller's scratch.  (One workgroup per edge was the first form: 393 216
// sigmoids on 256 lanes, about a quarter of a millisecond per call whatever
// the number of edges; measured, DESIGN.md.)
// k_gru_glo_finish, one workgroup per edge: the chunks' sums added in ascending
// order, x 1 / HW, then thread <-> output of the three 128 x 128 products:
// gbias[e, 128 k + co] = b_k[co] + (W_k_glo glo[e])[co] + b_k_glo[co], fp32, the
// bias the two convolution launches add.  No atomics, a fixed order: an
// edge's result does not depend on the other edges of the call.
//
// k_gru_conv, the wide-K form of k_conv3x3 (droid_conv3x3.hip) on the 16 x 8
// tile, the staging and the tap x K-step loop of droid_conv_tile.h: wave <-> 4
// row blocks x 4 tile rows, 128 output rows per workgroup; blockIdx.z is the
// pass of 128 rows (zr: two, convz over convr; q: one).  The K loop runs over
// up to four sources, each (pointer, 64 or 128 channels, entry stride, optional
// index array): one source is one chunk, staged into the same LDS buffer after
// the chunk before it has been consumed, the accumulators kept across chunks.
// The concatenated tensor is never written.  Chunks are not double-buffered
// and weight fragments not staged in LDS: two workgroups per CU (49 KB each)
// hide each other's staging, as in k_conv3x3.
//
// Epilogues: zr pass 0  z    = fp16(sigmoid(acc + gbias))           -> [n, 128, ht, wd]
//            zr pass 1  rnet = fp16(sigmoid(acc + gbias) * net)     -> [n, 128, ht, wd]
//            q          net' = fp16((1 - z) net + z tanh(acc + gbias)), z and net read at the output element.
// sigmoid(v) = 1 / (1 + expf(-v)); tanh(v) = 1 - 2 / (1 + expf(2 v)) (exact
// limits at both ends: expf -> inf gives 1, expf -> 0 gives -1).
//
// Packed weights (wgsr.frontend.pack_conv3x3_wide): the layout of
// droid_conv_tile.h with KS = C_in / 32 = 14.
//
// Index validation (inp through inp_ix): every workgroup of every launch scans
// inp_ix and returns before it writes when an entry is outside [0, F);
// workgroup (0, 0, 0) writes the status word.
#include <hip/hip_fp16.h>
#include <math.h>

#include "droid_conv_tile.h"

namespace wgsr {

namespace {

constexpr int kGrC = kCtC;                            // channels of net, and output rows of one pass
constexpr int kGrTY = 8;                              // rows of the tile
constexpr int kGrGates = 3 * kGrC;                    // columns of gbias
constexpr int kGrGloPix = 128;                        // pixels of a chunk of k_gru_glo
// halfs of glo_w: w packed as one tap (8 row blocks x 4 K-steps), then conv{z,r,q}_glo [384][128]
constexpr int kGrGloPacked = 8 * 4 * kCtFrag;
constexpr size_t kGrConvLds = ct_lds(ct_halo(kGrTY));
constexpr size_t kGrGloLds = ct_lds(kGrGloPix);

enum { kZR = 0, kQ = 1 };

struct GruSrc {
  const __half* p;        // channel 0 of entry 0
  int64_t bstride;        // halfs between two entries
  const int64_t* ix;      // null: entry e of the source belongs to edge e
  int ch;                 // 64 or 128; 0: no such source
};

struct GruArgs {
  GruSrc src[4];
  const __half* w;        // packed, ksteps K-steps per (row block, tap)
  int ksteps;
  const float* gbias;     // [n, 384]
  int gb0;                // the column of gbias of row 0 of pass 0
  const __half* net;      // [n, 128, ht, wd]: the epilogues' net
  const __half* z;        // kQ: [n, 128, ht, wd]
  __half* out0;           // kZR: z; kQ: net'
  __half* out1;           // kZR: rnet
  const int64_t* inp_ix;  // [n] or null, validated against [0, F)
  int n, F;
  int ht, wd, tiles_x;
  uint32_t* status;
};

struct GloArgs {
  const __half* net;      // [n, 128, ht, wd]
  const __half* w;        // glo_w
  const float* b;         // glo_b: w's bias [128], conv{z,r,q}'s [384], conv{z,r,q}_glo's [384]
  float* gbias;           // [n, 384]
  float* part;            // [n, chunks, 128]: the chunks' sums
  const int64_t* inp_ix;
  int n, F, HW, chunks;
  uint32_t* status;
};

__device__ __forceinline__ float gr_sigmoid(float v) { return 1.f / (1.f + expf(-v)); }
__device__ __forceinline__ float gr_tanh(float v) { return 1.f - 2.f / (1.f + expf(2.f * v)); }

// grid (chunks of 128 pixels, n), 256 threads.  dynamic LDS: the staged chunk [128 pixels][kCtStride] fp16, the
// validation word.  part[e][chunk][co] = sum over the chunk's pixels of sigmoid(w(net) + bias) x net.
__global__ __launch_bounds__(256, 2) void k_gru_glo_part(const GloArgs a) {
  extern __shared__ uint4 s_gr[];
  __half* __restrict__ s_x = reinterpret_cast<__half*>(s_gr);
  uint32_t* s_bad = reinterpret_cast<uint32_t*>(s_x + kGrGloPix * kCtStride);
  const int t = threadIdx.x, lane = t & 63, wv = __builtin_amdgcn_readfirstlane(t >> 6);
  if (ct_bad_ix(s_bad, a.inp_ix, a.n, a.F, WGSR_GRU_BAD_IX, a.status, blockIdx.x == 0 && blockIdx.y == 0, t)) return;
  const int i = lane & 15, g = lane >> 4;
  const int e = blockIdx.y, HW = a.HW, p0 = blockIdx.x * kGrGloPix;
  const __half* __restrict__ net = a.net + (size_t)e * kGrC * HW;
  // wave <-> row blocks 2 wv, 2 wv + 1 (32 output channels) x the 8 pixel blocks of the chunk
  const __half* __restrict__ wfrag = a.w + (size_t)(2 * wv) * 4 * kCtFrag + 8 * lane;
  // thread <-> (pixel, 8 channels): 8 loads that the wave's lanes continue along the pixels, one 16-byte write
  for (int u = t; u < kGrGloPix * (kGrC / 8); u += 256) {
    const int cg = u / kGrGloPix, px = u - cg * kGrGloPix;
    union {
      uint4 v;
      __half h[8];
    } q;
    q.v = make_uint4(0, 0, 0, 0);
    if (p0 + px < HW) {
      const __half* __restrict__ s = net + (size_t)(8 * cg) * HW + p0 + px;
#pragma unroll
      for (int j = 0; j < 8; ++j) q.h[j] = s[(size_t)j * HW];
    }
    *reinterpret_cast<uint4*>(s_x + px * kCtStride + 8 * cg) = q.v;
  }
  __syncthreads();
  f32x4 acc[2][8];
#pragma unroll
  for (int rb = 0; rb < 2; ++rb)
#pragma unroll
    for (int cb = 0; cb < 8; ++cb) acc[rb][cb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    f16x8 af[2];
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) af[rb] = *reinterpret_cast<const f16x8*>(wfrag + (size_t)(4 * rb + ks) * kCtFrag);
#pragma unroll
    for (int cb = 0; cb < 8; ++cb) {
      const f16x8 bf = *reinterpret_cast<const f16x8*>(s_x + (16 * cb + i) * kCtStride + 32 * ks + 8 * g);
#pragma unroll
      for (int rb = 0; rb < 2; ++rb)
        acc[rb][cb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[rb], bf, acc[rb][cb], 0, 0, 0);
    }
  }
  // D: row (output channel of the block) 4 g + r in register r, column (pixel of the block) i.  A pixel
  // past HW was staged as zeros: its term sigmoid(bias) x 0 adds nothing.
#pragma unroll
  for (int rb = 0; rb < 2; ++rb) {
    const float4 b4 = *reinterpret_cast<const float4*>(a.b + 16 * (2 * wv + rb) + 4 * g);
    const float bs[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int co = 16 * (2 * wv + rb) + 4 * g + r;
      float v = 0.f;
#pragma unroll
      for (int cb = 0; cb < 8; ++cb)
        v += gr_sigmoid(acc[rb][cb][r] + bs[r]) * __half2float(s_x[(16 * cb + i) * kCtStride + co]);
#pragma unroll
      for (int m = 8; m >= 1; m >>= 1) v += __shfl_xor(v, m);
      if (i == 0) a.part[((size_t)e * gridDim.x + blockIdx.x) * kGrC + co] = v;
    }
  }
}

// grid (n), 256 threads.  glo = (the chunks' sums in ascending order) x 1 / HW, then thread <-> output of the
// three 128 x 128 products.
__global__ __launch_bounds__(256) void k_gru_glo_finish(const GloArgs a) {
  __shared__ float s_glo[kGrC];
  __shared__ uint32_t s_bad;
  const int t = threadIdx.x;
  if (ct_bad_ix(&s_bad, a.inp_ix, a.n, a.F, WGSR_GRU_BAD_IX, a.status, blockIdx.x == 0, t)) return;
  const int e = blockIdx.x;
  if (t < kGrC) {
    const float* __restrict__ part = a.part + (size_t)e * a.chunks * kGrC + t;
    float v = 0.f;
    for (int c = 0; c < a.chunks; ++c) v += part[(size_t)c * kGrC];
    s_glo[t] = v * (1.f / (float)a.HW);
  }
  __syncthreads();
  const __half* __restrict__ wg = a.w + kGrGloPacked;
  for (int o = t; o < kGrGates; o += 256) {
    const uint4* __restrict__ row = reinterpret_cast<const uint4*>(wg + (size_t)o * kGrC);
    float dot = 0.f;
    for (int c8 = 0; c8 < kGrC / 8; ++c8) {
      union {
        uint4 v;
        __half h[8];
      } q;
      q.v = row[c8];
#pragma unroll
      for (int j = 0; j < 8; ++j) dot = fmaf(__half2float(q.h[j]), s_glo[8 * c8 + j], dot);
    }
    a.gbias[(size_t)e * kGrGates + o] = a.b[kGrC + o] + dot + a.b[kGrC + kGrGates + o];
  }
}

// grid (tiles, n, passes of 128 rows), 256 threads.  dynamic LDS: the staged chunk, the validation word.
// Two waves per SIMD: everything in the 256 architectural registers (droid_upsample.hip on why).
template <int EPI>
__global__ __launch_bounds__(256, 2) void k_gru_conv(const GruArgs a) {
  extern __shared__ uint4 s_gr[];
  __half* __restrict__ s_x = reinterpret_cast<__half*>(s_gr);
  uint32_t* s_bad = reinterpret_cast<uint32_t*>(s_x + ct_halo(kGrTY) * kCtStride);
  const int t = threadIdx.x, lane = t & 63, wv = __builtin_amdgcn_readfirstlane(t >> 6);
  if (ct_bad_ix(s_bad, a.inp_ix, a.n, a.F, WGSR_GRU_BAD_IX, a.status,
                blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0, t))
    return;
  const int wp = wv & 1, wc = wv >> 1;  // wave <-> tile rows 4 wp .. 4 wp + 3, row blocks 4 wc .. 4 wc + 3 of the pass
  const int i = lane & 15, g = lane >> 4;
  const int b = blockIdx.y, pass = blockIdx.z;
  const int ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
  const int x0 = tx * kCtTX, y0 = ty * kGrTY;
  const int ht = a.ht, wd = a.wd;
  const int x = x0 + i;
  const int ksteps = a.ksteps;
  const __half* __restrict__ wfrag = a.w + (size_t)(8 * pass + 4 * wc) * 9 * ksteps * kCtFrag + 8 * lane;
  const size_t rbs = (size_t)9 * ksteps * kCtFrag;  // halfs between two row blocks
  // pixel (tile row 4 wp, column i) at tap (0, 0), channels 8 g ..
  const __half* xlane = s_x + (4 * wp * kCtHX + i) * kCtStride + 8 * g;

  f32x4 acc[4][4];
#pragma unroll
  for (int rb = 0; rb < 4; ++rb)
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) acc[rb][cb] = f32x4{0.f, 0.f, 0.f, 0.f};
  int ks0 = 0;  // K-steps of the sources before this one
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int nch = a.src[s].ch;
    if (nch == 0) continue;  // (workgroup-uniform)
    const int64_t se = a.src[s].ix ? a.src[s].ix[b] : (int64_t)b;
    if (s) __syncthreads();  // every wave is done with the chunk staged before
    ct_stage<kGrTY>(s_x, a.src[s].p + (size_t)se * a.src[s].bstride, nch, x0, y0, ht, wd, t);
    __syncthreads();
    const int nks = nch >> 5;  // 2 or 4
    ct_taps<4, 4, 0>(acc, xlane, wfrag, rbs, ksteps, ks0, nks);
    ks0 += nks;
  }
  // D: row (output channel of the block) 4 g + r in register r, column (pixel of the tile row) i
  const float* __restrict__ gb = a.gbias + (size_t)b * kGrGates + a.gb0 + kGrC * pass;
#pragma unroll
  for (int rb = 0; rb < 4; ++rb) {
    const int co0 = 16 * (4 * wc + rb) + 4 * g;
    const float4 b4 = *reinterpret_cast<const float4*>(gb + co0);
    const float bs[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) {
      const int y = y0 + 4 * wp + cb;
      if (y >= ht || x >= wd) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const size_t at = (((size_t)b * kGrC + co0 + r) * ht + y) * wd + x;
        const float v = acc[rb][cb][r] + bs[r];
        if constexpr (EPI == kZR) {
          if (pass == 0)
            a.out0[at] = __float2half_rn(gr_sigmoid(v));
          else
            a.out1[at] = __float2half_rn(gr_sigmoid(v) * __half2float(a.net[at]));
        } else {
          const float z = __half2float(a.z[at]), h = __half2float(a.net[at]);
          a.out0[at] = __float2half_rn((1.f - z) * h + z * gr_tanh(v));
        }
      }
    }
  }
}

struct GrRange {
  const char* name;
  uintptr_t lo, hi;
};

}  // namespace

}  // namespace wgsr

using namespace wgsr;

extern "C" {

int wgsr_droid_gru(const void* net, const void* inp, const int64_t* inp_ix, int inp_frames, const void* corr,
                   const void* flow, const void* glo_w, const float* glo_b, const void* zr_w, const void* q_w,
                   float* gbias, float* glo_part, void* z, void* rnet, void* out, int n, int ht, int wd,
                   uint32_t* status, void* stream) {
  const char* who = "wgsr_droid_gru";
  if (const int e = ct_shape_ok(who, n, ht, wd)) return e;
  if (inp_ix && (inp_frames <= 0 || inp_frames > 65535))
    return set_error(WGSR_EINVAL, "%s: inp_ix with %d frames of inp", who, inp_frames);
  if (!status) return set_error(WGSR_EINVAL, "%s: null status", who);
  hipStream_t s = (hipStream_t)stream;
  if (n == 0) return ct_err(who, hipMemsetAsync(status, 0, sizeof(uint32_t), s));
  if (!net || !inp || !corr || !flow || !gbias || !glo_part || !z || !rnet || !out || !glo_w || !glo_b || !zr_w || !q_w)
    return set_error(WGSR_EINVAL, "%s: null pointer", who);
  if ((reinterpret_cast<uintptr_t>(glo_w) | reinterpret_cast<uintptr_t>(glo_b) | reinterpret_cast<uintptr_t>(zr_w) |
       reinterpret_cast<uintptr_t>(q_w) | reinterpret_cast<uintptr_t>(gbias)) & 15)
    return set_error(WGSR_EINVAL, "%s: packed weights, biases and gbias must be 16-byte aligned", who);
  if (const int e = ct_lds_ok(who, kGrConvLds > kGrGloLds ? kGrConvLds : kGrGloLds)) return e;
  const int64_t HW = (int64_t)ht * wd;
  const uintptr_t map = (uintptr_t)(2 * kGrC * HW);  // bytes of one entry of 128 channels
  const auto range = [](const char* name, const void* p, uintptr_t bytes) {
    return GrRange{name, reinterpret_cast<uintptr_t>(p), reinterpret_cast<uintptr_t>(p) + bytes};
  };
  const int chunks = (int)((HW + kGrGloPix - 1) / kGrGloPix);
  constexpr int NW = 5;
  const GrRange wr[NW] = {range("out", out, n * map), range("z", z, n * map), range("rnet", rnet, n * map),
                          range("gbias", gbias, (uintptr_t)n * kGrGates * sizeof(float)),
                          range("glo_part", glo_part, (uintptr_t)n * chunks * kGrC * sizeof(float))};
  const GrRange rd[4] = {range("net", net, n * map), range("inp", inp, (inp_ix ? inp_frames : n) * map),
                         range("corr", corr, n * map), range("flow", flow, n * map / 2)};
  for (int i = 0; i < NW; ++i) {
    for (int j = 0; j < 4; ++j)
      if (wr[i].lo < rd[j].hi && rd[j].lo < wr[i].hi)
        return set_error(WGSR_EINVAL, "%s: %s overlaps %s", who, wr[i].name, rd[j].name);
    for (int j = i + 1; j < NW; ++j)
      if (wr[i].lo < wr[j].hi && wr[j].lo < wr[i].hi)
        return set_error(WGSR_EINVAL, "%s: %s overlaps %s", who, wr[i].name, wr[j].name);
  }

  GloArgs ga = {};
  ga.net = (const __half*)net, ga.w = (const __half*)glo_w, ga.b = glo_b, ga.gbias = gbias;
  ga.part = glo_part, ga.chunks = chunks;
  ga.inp_ix = inp_ix, ga.n = n, ga.F = inp_frames, ga.HW = (int)HW, ga.status = status;
  hipLaunchKernelGGL(k_gru_glo_part, dim3((unsigned)chunks, (unsigned)n), dim3(256), kGrGloLds, s, ga);
  if (const int e = ct_err(who, hipGetLastError())) return e;
  hipLaunchKernelGGL(k_gru_glo_finish, dim3((unsigned)n), dim3(256), 0, s, ga);
  if (const int e = ct_err(who, hipGetLastError())) return e;

  GruArgs a = {};
  a.src[0] = {(const __half*)net, kGrC * HW, nullptr, kGrC};
  a.src[1] = {(const __half*)inp, kGrC * HW, inp_ix, kGrC};
  a.src[2] = {(const __half*)corr, kGrC * HW, nullptr, kGrC};
  a.src[3] = {(const __half*)flow, kGrC / 2 * HW, nullptr, kGrC / 2};
  a.ksteps = (3 * kGrC + kGrC / 2) / 32;
  a.gbias = gbias, a.net = (const __half*)net;
  a.inp_ix = inp_ix, a.n = n, a.F = inp_frames, a.ht = ht, a.wd = wd, a.status = status;
  a.tiles_x = (wd + kCtTX - 1) / kCtTX;
  const unsigned tiles = (unsigned)(a.tiles_x * ((ht + kGrTY - 1) / kGrTY));
  a.w = (const __half*)zr_w, a.gb0 = 0, a.out0 = (__half*)z, a.out1 = (__half*)rnet;
  hipLaunchKernelGGL(k_gru_conv<kZR>, dim3(tiles, (unsigned)n, 2), dim3(256), kGrConvLds, s, a);
  if (const int e = ct_err(who, hipGetLastError())) return e;
  a.src[0].p = (const __half*)rnet;
  a.w = (const __half*)q_w, a.gb0 = 2 * kGrC, a.z = (const __half*)z, a.out0 = (__half*)out, a.out1 = nullptr;
  hipLaunchKernelGGL(k_gru_conv<kQ>, dim3(tiles, (unsigned)n, 1), dim3(256), kGrConvLds, s, a);
  return ct_err(who, hipGetLastError());
}

}  // extern "C"
