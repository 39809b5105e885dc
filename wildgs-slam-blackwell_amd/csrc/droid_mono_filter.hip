// wgsr.frontend.filter_mono_depth: the tracker's DINO-consistency filter of the
// metric depth prior (DepthVideo.filter_high_err_mono_depth, depth_video.py:
// 281-349) for gfx950.
//
// For every reference frame j of a keyframe idx, every pixel of j is carried
// into idx with j's metric disparity; it is a candidate for the pixel it
// rounds to when the DINO features of the two pixels have a cosine above a
// threshold.  Per (j, target) the candidate with the largest source index
// wins, its disparity is compared with idx's own, and the target counts it as
// accurate or inaccurate; the mask of idx is cleared where fewer than two
// frames agree and at least one disagrees.
//
// The reference upsamples each frame's [hd, wd, C] DINO map bilinearly to H x
// W (C = 384: 300 MB a frame at 384 x 512) and gathers it.  Here no
// full-resolution map exists.  A bilinear sample is a combination of four
// cell vectors, so
//   <f_j(p), f_i(q)> = sum over 4 x 4 (cell of p, cell of q) of
//                      w_p w_q G_j[cell_p][cell_q],  G_j = F_j F_idx^T
//   |f(p)|^2         = sum over the 2 x 2 cells of p, twice, of w w' S[c][c'],
//                      S = F F^T (10 distinct entries by symmetry)
// which is the same polynomial in the same fp32 inputs as the reference's
// blend-then-dot, summed in another order.
//
//   k_mf_zero        zeroes the winner words (a kernel, so that a captured
//                    call holds no memset node)
//   k_mf_gram        G_j (n_ref of them, n x n, n = hd wd) and S of every
//                    frame (n_ref + 1; only the tiles within wd + 1 cells of
//                    the diagonal, at or above it, are computed or read), in
//                    fp32 on v_mfma_f32_16x16x4_f32: a 64 x 64 tile per
//                    workgroup, 2 x 2 MFMA tiles per wave (four independent
//                    accumulators), K in chunks of 32 through LDS.  An LDS row
//                    is 33 floats and lane quarter h reads k = 16 (h & 1) + 8
//                    (h >> 1) + m at step m -- a sum may take its k in any
//                    order -- so the 32 lanes of a half read 32 banks.
//   k_mf_candidates  one thread per (j, source pixel): geometry, rounding, 16
//                    + 10 + 10 Gram reads, and on a match one 64-bit atomicMax
//                    of ((source index + 1) << 32) | bits(d) into the winner
//                    word of (j, target).  d > 0, so the word orders by source
//                    index alone and the result does not depend on arrival.
//   k_mf_decide      one thread per target pixel: walks its n_ref winner
//                    words, counts, clears the mask byte.
//
// Index validation: every kernel tests the entries of jj it uses against [0,
// num) and does nothing for a bad one; k_mf_decide scans all of jj, writes the
// status word and returns before it writes when any is bad, so a refused call
// leaves the mask (and the counts) untouched.
#include <math.h>

#include <algorithm>

#include "wgsr_common.h"
#include "wgsr_internal.h"
#include "droid_pose.h"

namespace wgsr {

namespace {

constexpr int kMfTile = 64;     // Gram rows and columns per workgroup
constexpr int kMfK = 32;        // channels per LDS chunk
constexpr int kMfLd = 33;       // floats per LDS row
constexpr int kMfThreads = 256;
constexpr float kMfMinZ = 0.1f;   // 0.5 MIN_DEPTH of the reference's proj
constexpr float kMfNormEps = 1e-12f;  // F.normalize's eps
constexpr int kMfDownScale = 8;   // DepthVideo.down_scale

typedef float f32x4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(kMfThreads) void k_mf_zero(ulonglong2* __restrict__ w, size_t pairs) {
  const size_t stride = (size_t)gridDim.x * kMfThreads;
  for (size_t i = (size_t)blockIdx.x * kMfThreads + threadIdx.x; i < pairs; i += stride) w[i] = make_ulonglong2(0, 0);
}

// the frame of reference k (k == n_ref: the keyframe) among the feature maps
__device__ __forceinline__ int64_t mf_feat_frame(int packed, int k, int n_ref, int64_t frame) {
  return packed ? (k == n_ref ? 0 : k + 1) : frame;
}

// gram[b], b < n_ref: F_jj[b] F_idx^T; n_ref <= b < 2 n_ref: F F^T of jj[b - n_ref]; b == 2 n_ref: of idx
__global__ __launch_bounds__(kMfThreads) void k_mf_gram(const float* __restrict__ feats, int packed,
                                                        const int64_t* __restrict__ jj, int n_ref, int idx, int num,
                                                        int n, int C, int band, float* __restrict__ gram) {
  __shared__ float sA[kMfTile * kMfLd];
  __shared__ float sB[kMfTile * kMfLd];
  const int b = blockIdx.z, row0 = blockIdx.y * kMfTile, col0 = blockIdx.x * kMfTile;
  const bool self = b >= n_ref;
  // a frame's own Gram matrix is read at [c][c'] with c <= c' <= c + band only
  if (self && (col0 + kMfTile - 1 < row0 || col0 > row0 + kMfTile - 1 + band)) return;
  const int ka = b < n_ref ? b : b - n_ref;  // the reference of the A operand (n_ref: the keyframe)
  int64_t fa = idx;
  if (ka < n_ref) {
    fa = jj[ka];
    if (fa < 0 || fa >= num) return;
  }
  const float* A = feats + (size_t)mf_feat_frame(packed, ka, n_ref, fa) * n * C;
  const float* B = self ? A : feats + (size_t)mf_feat_frame(packed, n_ref, n_ref, idx) * n * C;

  const int t = threadIdx.x, w = t >> 6, lane = t & 63, lr = lane & 15, kh = lane >> 4;
  const int wr = w >> 1, wc = w & 1;
  const int kq = 16 * (kh & 1) + 8 * (kh >> 1);
  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int k0 = 0; k0 < C; k0 += kMfK) {
    float4 va[2], vb[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int s = t + kMfThreads * i, r = s >> 3, k = k0 + 4 * (s & 7);
      // rows past n: a valid row, never stored; channels past C: zero (C % 4 == 0)
      const size_t ra = (size_t)min(row0 + r, n - 1) * C, rb = (size_t)min(col0 + r, n - 1) * C;
      va[i] = k < C ? *reinterpret_cast<const float4*>(A + ra + k) : make_float4(0.f, 0.f, 0.f, 0.f);
      vb[i] = k < C ? *reinterpret_cast<const float4*>(B + rb + k) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    __syncthreads();  // the last chunk has been read
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int s = t + kMfThreads * i, o = (s >> 3) * kMfLd + 4 * (s & 7);
      sA[o] = va[i].x; sA[o + 1] = va[i].y; sA[o + 2] = va[i].z; sA[o + 3] = va[i].w;
      sB[o] = vb[i].x; sB[o + 1] = vb[i].y; sB[o + 2] = vb[i].z; sB[o + 3] = vb[i].w;
    }
    __syncthreads();
    const float* pa = sA + (32 * wr + lr) * kMfLd + kq;
    const float* pb = sB + (32 * wc + lr) * kMfLd + kq;
#pragma unroll
    for (int m = 0; m < 8; ++m) {
      const float a0 = pa[m], a1 = pa[16 * kMfLd + m], b0 = pb[m], b1 = pb[16 * kMfLd + m];
      acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc[1][1], 0, 0, 0);
    }
  }
  // D: column lane & 15 (the B row), rows 4 (lane >> 4) + q (the A rows)
  float* G = gram + (size_t)b * n * n;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int col = col0 + 32 * wc + 16 * j + lr;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int row = row0 + 32 * wr + 16 * i + 4 * kh + q;
        if (row < n && col < n) G[(size_t)row * n + col] = acc[i][j][q];
      }
    }
}

// F.interpolate(mode='bilinear', align_corners=False) from `in` cells to `out`
// pixels along one axis: the two cells of pixel `dst` and the weight of the second
__device__ __forceinline__ void mf_axis(int dst, float scale, int in, int& i0, int& i1, float& l1) {
  float src = scale * ((float)dst + 0.5f) - 0.5f;
  src = src < 0.f ? 0.f : src;
  i0 = min((int)src, in - 1);
  i1 = min(i0 + 1, in - 1);
  l1 = fminf(fmaxf(src - (float)i0, 0.f), 1.f);
}

struct MfBlend {  // the four cells (ascending linear index) and weights of a pixel's bilinear sample
  int c[4];
  float w[4];
};

__device__ __forceinline__ MfBlend mf_blend(int x, int y, float sx, float sy, int hd, int wd) {
  int x0, x1, y0, y1;
  float lx, ly;
  mf_axis(x, sx, wd, x0, x1, lx);
  mf_axis(y, sy, hd, y0, y1, ly);
  MfBlend r;
  r.c[0] = y0 * wd + x0; r.c[1] = y0 * wd + x1; r.c[2] = y1 * wd + x0; r.c[3] = y1 * wd + x1;
  r.w[0] = (1.f - ly) * (1.f - lx); r.w[1] = (1.f - ly) * lx; r.w[2] = ly * (1.f - lx); r.w[3] = ly * lx;
  return r;
}

// |sample|^2 from the frame's own (symmetric) Gram matrix, read at [c][c']
// with c <= c' <= c + wd + 1 only
__device__ __forceinline__ float mf_norm2(const float* __restrict__ S, int n, const MfBlend& p) {
  float s = 0.f;
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    s = fmaf(p.w[a] * p.w[a], S[(size_t)p.c[a] * n + p.c[a]], s);
#pragma unroll
    for (int b = a + 1; b < 4; ++b) {
      // (at a clamped border cell 1 can follow cell 2)
      const int lo = min(p.c[a], p.c[b]), hi = max(p.c[a], p.c[b]);
      s = fmaf(2.f * p.w[a] * p.w[b], S[(size_t)lo * n + hi], s);
    }
  }
  return fmaxf(s, 0.f);
}

__global__ __launch_bounds__(kMfThreads) void k_mf_candidates(
    const float* __restrict__ poses, const float* __restrict__ disps, const float* __restrict__ intrinsics,
    const int64_t* __restrict__ jj, int n_ref, int idx, int num, int H, int W, int hd, int wd, float sim_thresh,
    const float* __restrict__ gram, unsigned long long* __restrict__ winner) {
  const int k = blockIdx.y;
  const int64_t j = jj[k];
  if (j < 0 || j >= num) return;
  const int HW = H * W, p = blockIdx.x * kMfThreads + threadIdx.x;
  if (p >= HW) return;
  const int y = p / W, x = p - y * W;
  const float fx = intrinsics[0] * kMfDownScale, fy = intrinsics[1] * kMfDownScale;
  const float cx = intrinsics[2] * kMfDownScale, cy = intrinsics[3] * kMfDownScale;
  const float D = disps[(size_t)j * HW + p];
  const Pose rel = relative_pose(load_pose(poses, j), load_pose(poses, idx));
  const f3 r = rotate(rel, mk3(((float)x - cx) / fx, ((float)y - cy) / fy, 1.f));
  const float X = r.x + rel.tx * D, Y = r.y + rel.ty * D;
  float Z = r.z + rel.tz * D;
  if (Z < kMfMinZ) Z = 1.f;  // (the reference's proj: such a point stays a candidate)
  const float iz = 1.f / Z;
  const float u = fx * (X * iz) + cx, v = fy * (Y * iz) + cy, d = D * iz;
  const float tu = rintf(u), tv = rintf(v);  // round half to even, as torch.round
  // compared as floats: a huge or non-finite coordinate is simply invalid
  if (!(tu >= 0.f && tu < (float)W && tv >= 0.f && tv < (float)H && d > 0.f)) return;
  const int tx = (int)tu, ty = (int)tv;

  const float sx = (float)wd / (float)W, sy = (float)hd / (float)H;
  const int n = hd * wd;
  const MfBlend bs = mf_blend(x, y, sx, sy, hd, wd), bt = mf_blend(tx, ty, sx, sy, hd, wd);
  const size_t nn = (size_t)n * n;
  const float* G = gram + (size_t)k * nn;
  float dot = 0.f;
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const float* row = G + (size_t)bs.c[a] * n;
    float s = 0.f;
#pragma unroll
    for (int b = 0; b < 4; ++b) s = fmaf(bt.w[b], row[bt.c[b]], s);
    dot = fmaf(bs.w[a], s, dot);
  }
  const float ns = sqrtf(mf_norm2(gram + (size_t)(n_ref + k) * nn, n, bs));
  const float nt = sqrtf(mf_norm2(gram + (size_t)(2 * n_ref) * nn, n, bt));
  const float cosine = dot / (fmaxf(ns, kMfNormEps) * fmaxf(nt, kMfNormEps));
  if (!(cosine > sim_thresh)) return;
  const unsigned long long word = ((unsigned long long)(p + 1) << 32) | __float_as_uint(d);
  atomicMax(winner + (size_t)k * HW + (size_t)ty * W + tx, word);
}

__global__ __launch_bounds__(kMfThreads) void k_mf_decide(const float* __restrict__ disps,
                                                          const int64_t* __restrict__ jj, int n_ref, int idx, int num,
                                                          int HW, float err_thresh,
                                                          const unsigned long long* __restrict__ winner,
                                                          uint8_t* __restrict__ mask, int32_t* __restrict__ accurate,
                                                          int32_t* __restrict__ inaccurate,
                                                          uint32_t* __restrict__ status) {
  int bad = 0;
  for (int e = threadIdx.x; e < n_ref; e += kMfThreads) bad |= (jj[e] < 0 || jj[e] >= num) ? 1 : 0;
  bad = __syncthreads_or(bad);
  if (blockIdx.x == 0 && threadIdx.x == 0) *status = bad ? WGSR_MONO_FILTER_BAD_JJ : 0u;
  if (bad) return;
  const int p = blockIdx.x * kMfThreads + threadIdx.x;
  if (p >= HW) return;
  const float Di = disps[(size_t)idx * HW + p];
  const float inv_i = 1.f / Di;  // (a zero disparity: inf, an inaccurate count)
  int acc = 0, inacc = 0;
  for (int k = 0; k < n_ref; ++k) {
    const unsigned long long word = winner[(size_t)k * HW + p];
    if (!word) continue;
    const float w = __uint_as_float((uint32_t)word);
    const float err = fabsf(1.f / w - inv_i) * w;
    if (err < err_thresh) ++acc; else ++inacc;
  }
  if (accurate) accurate[p] = acc;
  if (inaccurate) inaccurate[p] = inacc;
  if (acc <= 1 && inacc > 0 && Di > 0.f) mask[(size_t)idx * HW + p] = 0;
}

inline int64_t mf_align(int64_t b) { return (b + 255) & ~(int64_t)255; }

// nullptr, or why the sizes are refused
const char* mf_sizes_bad(int n_ref, int H, int W, int hd, int wd) {
  if (n_ref < 0 || n_ref > 32767) return "n_ref outside [0, 32767]";
  if (H < 1 || W < 1 || (int64_t)H * W >= ((int64_t)1 << 31) - kMfThreads) return "H x W outside [1, 2^31 - 256)";
  if (hd < 1 || wd < 1 || hd > H || wd > W || (int64_t)hd * wd > (1 << 20)) return "hd x wd outside [1, H] x [1, W] or over 2^20 cells";
  return nullptr;
}

}  // namespace

}  // namespace wgsr

using namespace wgsr;

extern "C" {

int64_t wgsr_droid_mono_filter_workspace_bytes(int n_ref, int H, int W, int hd, int wd) {
  if (const char* why = mf_sizes_bad(n_ref, H, W, hd, wd)) {
    set_error(WGSR_EINVAL, "wgsr_droid_mono_filter_workspace_bytes: %s", why);
    return -1;
  }
  const int64_t n = (int64_t)hd * wd;
  return mf_align((int64_t)n_ref * H * W * 8) + mf_align((2 * (int64_t)n_ref + 1) * n * n * 4);
}

int wgsr_droid_mono_filter(const float* poses, const float* disps_up, uint8_t* mask_up, const float* intrinsics,
                           const float* feats, int feats_packed, const int64_t* jj, int n_ref, int idx, int num,
                           int H, int W, int hd, int wd, int C, float sim_thresh, float err_thresh,
                           int32_t* accurate, int32_t* inaccurate, void* workspace, int64_t workspace_bytes,
                           uint32_t* status, void* stream) {
  const char* who = "wgsr_droid_mono_filter";
  if (const char* why = mf_sizes_bad(n_ref, H, W, hd, wd)) return set_error(WGSR_EINVAL, "%s: %s", who, why);
  if (num < 1 || idx < 0 || idx >= num) return set_error(WGSR_EINVAL, "%s: idx=%d outside [0, %d)", who, idx, num);
  if (C < 4 || C % 4 != 0) return set_error(WGSR_EINVAL, "%s: the channel count C=%d must be a positive multiple of 4", who, C);
  if (!poses || !disps_up || !mask_up || !intrinsics || !status || (n_ref && (!feats || !jj || !workspace)))
    return set_error(WGSR_EINVAL, "%s: null pointer", who);
  if (reinterpret_cast<uintptr_t>(feats) & 15) return set_error(WGSR_EINVAL, "%s: feats must be 16-byte aligned", who);
  if (reinterpret_cast<uintptr_t>(workspace) & 15)
    return set_error(WGSR_EINVAL, "%s: workspace must be 16-byte aligned", who);
  const int64_t need = wgsr_droid_mono_filter_workspace_bytes(n_ref, H, W, hd, wd);
  if (n_ref && workspace_bytes < need)
    return set_error(WGSR_EINVAL, "%s: workspace of %lld bytes, %lld needed", who, (long long)workspace_bytes,
                     (long long)need);
  hipStream_t s = (hipStream_t)stream;
  const int HW = H * W, n = hd * wd;
  unsigned long long* winner = static_cast<unsigned long long*>(workspace);
  float* gram = reinterpret_cast<float*>(static_cast<char*>(workspace) + mf_align((int64_t)n_ref * HW * 8));
  const unsigned pix_blocks = (unsigned)((HW + kMfThreads - 1) / kMfThreads);
  if (n_ref) {
    const size_t pairs = ((size_t)n_ref * HW + 1) / 2;  // (the winner block is padded to 256 bytes)
    const unsigned zb = (unsigned)std::min<size_t>((pairs + kMfThreads - 1) / kMfThreads, 2048);
    hipLaunchKernelGGL(k_mf_zero, dim3(zb), dim3(kMfThreads), 0, s, reinterpret_cast<ulonglong2*>(winner), pairs);
    const unsigned tiles = (unsigned)((n + kMfTile - 1) / kMfTile);
    hipLaunchKernelGGL(k_mf_gram, dim3(tiles, tiles, (unsigned)(2 * n_ref + 1)), dim3(kMfThreads), 0, s, feats,
                       feats_packed, jj, n_ref, idx, num, n, C, wd + 1, gram);
    hipLaunchKernelGGL(k_mf_candidates, dim3(pix_blocks, (unsigned)n_ref), dim3(kMfThreads), 0, s, poses, disps_up,
                       intrinsics, jj, n_ref, idx, num, H, W, hd, wd, sim_thresh, gram, winner);
  }
  hipLaunchKernelGGL(k_mf_decide, dim3(pix_blocks), dim3(kMfThreads), 0, s, disps_up, jj, n_ref, idx, num, HW,
                     err_thresh, winner, mask_up, accurate, inaccurate, status);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? WGSR_OK : set_error(WGSR_EHIP, "%s: %s", who, hipGetErrorString(e));
}

}  // extern "C"
