// droid_backends.ba for gfx950: DROID-SLAM's dense bundle adjustment, every
// Gauss-Newton iteration wholly on the device (no host round trip, no
// atomics: two calls on the same inputs give the same bits).
//
// Conventions: droid.hip's.  N edges (ii[e], jj[e]); frames [t0, t1) have free
// poses (P = t1 - t0); kx = sorted({t0..t1-1} u set(ii)) are the K frames
// whose disparities are variables ("slots"); HW = ht * wd.
//
// One call:  k_ba_setup  (one workgroup) validates the indices into the status
//   word, numbers the slots (frame -> slot by a block scan of a presence
//   flag) and groups the edges by source slot (CSR, edges ascending).
// One iteration:
//   k_ba_edge    one workgroup per edge: relative pose, per pixel the residual
//                and the Jacobians (fp32); writes E_i, E_j [6, HW], C, b_z [HW]
//                and the edge's 12 x 12 pose Hessian and two gradients (fp32
//                per lane over HW / 256 pixels, fp64 across lanes).
//   k_ba_frame   one lane per (slot, pixel): C_k, w_k, Q_k = 1 / C_k and the
//                slot's own coupling Ei[k] = sum of its edges' E_i.
//   k_ba_reduce  one workgroup per block (a <= b) of the reduced system: the
//                owner sums the pose Hessian blocks of the edges between a
//                and b and subtracts the Schur term S_ab = sum over slots k,
//                couplings c1 of k to a, c2 of k to b of E_c1 diag(Q_k) E_c2^T
//                (fp32 products, fp64 sums), damps the diagonal and writes
//                the block and its mirror; (a, a) also writes g_a = a_a - s_a.
//   k_ba_solve_* one workgroup: fp64 Cholesky and the two triangular solves
//                (factor in LDS while 6P <= kCholLds, else blocked through
//                global memory); a failed pivot gives dx = 0.
//   k_ba_update  one lane per (slot, pixel): dz and disps += dz.
//   k_ba_retract one lane per free pose: the SE(3) retraction.
// Every kernel after k_ba_setup returns at once when the status word is set.
#include <math.h>

#include "wgsr_common.h"
#include "wgsr_internal.h"
#include "droid_pose.h"

namespace wgsr {

namespace {

constexpr int kBaThreads = 256;
constexpr int kCholLds = 84;    // largest 6P factored in LDS (84 * 84 doubles = 56448 bytes)
constexpr int kCholBlock = 32;  // block width of the global-memory path
constexpr float kBaAlpha = 0.05f;
constexpr int kHess = 78;       // lower triangle of the 12 x 12 edge Hessian
constexpr int kEdgeSums = kHess + 12;

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, kWave);
  return v;
}

// exclusive prefix of one int per thread over the workgroup (256 threads);
// *total = the sum.  s_scan: 256 ints.
__device__ __forceinline__ int block_excl_scan(int v, int* s_scan, int* total) {
  const int t = threadIdx.x;
  __syncthreads();
  s_scan[t] = v;
  __syncthreads();
  for (int off = 1; off < kBaThreads; off <<= 1) {
    const int add = t >= off ? s_scan[t - off] : 0;
    __syncthreads();
    s_scan[t] += add;
    __syncthreads();
  }
  *total = s_scan[kBaThreads - 1];
  return s_scan[t] - v;
}

// ---------------------------------------------------------------------------
// setup: validation, slots, edges by source slot
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kBaThreads) void k_ba_setup(const int64_t* __restrict__ ii,
                                                         const int64_t* __restrict__ jj, int N, int num, int K,
                                                         int t0, int t1, int* __restrict__ slot,
                                                         int* __restrict__ kx, int* __restrict__ estart,
                                                         int* __restrict__ elist, int* __restrict__ ejj,
                                                         uint32_t* __restrict__ status) {
  __shared__ int s_scan[kBaThreads];
  __shared__ uint32_t s_status;
  const int t = threadIdx.x;
  if (t == 0) s_status = 0u;
  for (int f = t; f < num; f += kBaThreads) slot[f] = (f >= t0 && f < t1) ? 1 : 0;
  __syncthreads();
  for (int e = t; e < N; e += kBaThreads) {
    const int64_t i = ii[e], j = jj[e];
    uint32_t bad = 0u;
    if (i < 0 || i >= num || j < 0 || j >= num) bad |= WGSR_BA_BAD_INDEX;
    if (j >= t1) bad |= WGSR_BA_BAD_JJ;
    if (bad) atomicOr(&s_status, bad);
    if (i >= 0 && i < num) slot[i] = 1;  // (every writer stores the same value)
  }
  __syncthreads();
  // frame -> slot: each thread numbers a contiguous chunk of frames
  const int chunk = (num + kBaThreads - 1) / kBaThreads;
  const int f0 = min(t * chunk, num), f1 = min(f0 + chunk, num);
  int cnt = 0, total = 0;
  for (int f = f0; f < f1; ++f) cnt += slot[f];
  int at = block_excl_scan(cnt, s_scan, &total);
  for (int f = f0; f < f1; ++f) {
    if (slot[f]) {
      if (at < K) kx[at] = f;
      slot[f] = at++;
    } else {
      slot[f] = -1;
    }
  }
  if (t == 0 && total != K) s_status |= WGSR_BA_BAD_K;
  __syncthreads();
  const uint32_t st = s_status;
  if (t == 0) *status = st;
  if (st) return;
  // edges by source slot, ascending within a slot: count, scan, fill
  const int kchunk = (K + kBaThreads - 1) / kBaThreads;
  const int k0 = min(t * kchunk, K), k1 = min(k0 + kchunk, K);
  cnt = 0;
  for (int k = k0; k < k1; ++k) {
    const int64_t f = kx[k];
    for (int e = 0; e < N; ++e) cnt += ii[e] == f ? 1 : 0;
  }
  at = block_excl_scan(cnt, s_scan, &total);
  for (int k = k0; k < k1; ++k) {
    const int64_t f = kx[k];
    estart[k] = at;
    for (int e = 0; e < N; ++e)
      if (ii[e] == f) {
        elist[at] = e;
        ejj[at++] = (int)jj[e];  // the coupling's pose, in list order
      }
  }
  if (t == 0) estart[K] = total;  // (= N: every ii is a slot)
}

// ---------------------------------------------------------------------------
// edge linearisation
// ---------------------------------------------------------------------------
// minus the transposed adjoint of T applied to the 6-vector (a, b):
// -(R^T a, R^T (b + a x t))
__device__ __forceinline__ void neg_adj_t(const Pose& Tinv, f3 tr, const float* __restrict__ Jj,
                                          float* __restrict__ Ji) {
  const f3 a = mk3(Jj[0], Jj[1], Jj[2]), b = mk3(Jj[3], Jj[4], Jj[5]);
  const f3 ra = rotate(Tinv, a), rb = rotate(Tinv, add3(b, cross3(a, tr)));
  Ji[0] = -ra.x; Ji[1] = -ra.y; Ji[2] = -ra.z;
  Ji[3] = -rb.x; Ji[4] = -rb.y; Ji[5] = -rb.z;
}

// one residual row: J = (J_i, J_j), weight wp (0 on a stereo edge), residual r
__device__ __forceinline__ void edge_row(float wp, float r, float Jz, const float (&J)[12], float (&h)[kHess],
                                         float (&v)[12], float (&ei)[6], float (&ej)[6]) {
  float wJ[12];
#pragma unroll
  for (int n = 0; n < 12; ++n) wJ[n] = wp * J[n];
  int l = 0;
#pragma unroll
  for (int n = 0; n < 12; ++n) {
#pragma unroll
    for (int m = 0; m <= n; ++m) h[l++] += wJ[n] * J[m];
  }
#pragma unroll
  for (int n = 0; n < 12; ++n) v[n] += wJ[n] * r;
#pragma unroll
  for (int n = 0; n < 6; ++n) {
    ei[n] += wJ[n] * Jz;
    ej[n] += wJ[6 + n] * Jz;
  }
}

__global__ __launch_bounds__(kBaThreads) void k_ba_edge(
    const uint32_t* __restrict__ status, const float* __restrict__ poses, const float* __restrict__ disps,
    const float* __restrict__ intrinsics, const float* __restrict__ targets, const float* __restrict__ weights,
    const int64_t* __restrict__ ii, const int64_t* __restrict__ jj, int ht, int wd, int store,
    float* __restrict__ Ei, float* __restrict__ Ej, float* __restrict__ Ce, float* __restrict__ bz,
    double* __restrict__ Hf, double* __restrict__ vf) {
  if (*status) return;
  __shared__ Pose s_T;
  __shared__ double s_red[4][kEdgeSums];
  const int t = threadIdx.x, wv_ = t >> 6, lane = t & 63;
  const size_t e = blockIdx.x;
  const int64_t fi = ii[e], fj = jj[e];
  const bool stereo = fi == fj;
  if (t == 0) {
    // a stereo edge: the fixed baseline
    s_T = stereo ? Pose{0.f, 0.f, 0.f, 1.f, -0.1f, 0.f, 0.f}
                 : relative_pose(load_pose(poses, fi), load_pose(poses, fj));
  }
  __syncthreads();
  const Pose T = s_T;
  const Pose Tinv = Pose{-T.qx, -T.qy, -T.qz, T.qw, 0.f, 0.f, 0.f};
  const f3 tr = mk3(T.tx, T.ty, T.tz);
  const float fx = intrinsics[0], fy = intrinsics[1], cx = intrinsics[2], cy = intrinsics[3];
  const int HW = ht * wd;
  const float* __restrict__ dsp = disps + (size_t)fi * HW;
  const float* __restrict__ tg = targets + e * 2 * HW;
  const float* __restrict__ wg = weights + e * 2 * HW;
  float h[kHess], v[12];
#pragma unroll
  for (int l = 0; l < kHess; ++l) h[l] = 0.f;
#pragma unroll
  for (int n = 0; n < 12; ++n) v[n] = 0.f;
  for (int k = t; k < HW; k += kBaThreads) {
    const int row = k / wd, col = k - row * wd;
    const float hd = dsp[k];
    const f3 R = rotate(T, mk3(((float)col - cx) / fx, ((float)row - cy) / fy, 1.f));
    const float x = R.x + hd * T.tx, y = R.y + hd * T.ty, z = R.z + hd * T.tz;
    const bool ok = z >= kMinDepth;  // (false for NaN)
    const float d = ok ? 1.f / z : 0.f, d2 = d * d;
    const float wu = ok ? 0.001f * wg[k] : 0.f, wv = ok ? 0.001f * wg[HW + k] : 0.f;
    const float ru = tg[k] - (fx * d * x + cx), rv = tg[HW + k] - (fy * d * y + cy);
    float J[12], ei[6], ej[6];
#pragma unroll
    for (int n = 0; n < 6; ++n) ei[n] = ej[n] = 0.f;
    // the u row
    J[6] = fx * (hd * d);
    J[7] = 0.f;
    J[8] = fx * (-x * hd * d2);
    J[9] = fx * (-x * y * d2);
    J[10] = fx * (1.f + x * x * d2);
    J[11] = fx * (-y * d);
    const float Jzu = fx * (T.tx * d - T.tz * (x * d2));
    neg_adj_t(Tinv, tr, J + 6, J);
    edge_row(stereo ? 0.f : wu, ru, Jzu, J, h, v, ei, ej);
    // the v row
    J[6] = 0.f;
    J[7] = fy * (hd * d);
    J[8] = fy * (-y * hd * d2);
    J[9] = fy * (-1.f - y * y * d2);
    J[10] = fy * (x * y * d2);
    J[11] = fy * (x * d);
    const float Jzv = fy * (T.ty * d - T.tz * (y * d2));
    neg_adj_t(Tinv, tr, J + 6, J);
    edge_row(stereo ? 0.f : wv, rv, Jzv, J, h, v, ei, ej);
    if (store) {
      Ce[e * HW + k] = wu * Jzu * Jzu + wv * Jzv * Jzv;
      bz[e * HW + k] = wu * ru * Jzu + wv * rv * Jzv;
#pragma unroll
      for (int n = 0; n < 6; ++n) {
        Ei[(e * 6 + n) * HW + k] = ei[n];
        Ej[(e * 6 + n) * HW + k] = ej[n];
      }
    }
  }
  // fp64 across lanes: wave butterflies, then the four waves in a fixed order
#pragma unroll
  for (int l = 0; l < kHess; ++l) {
    const double s = wave_sum_f64((double)h[l]);
    if (lane == 0) s_red[wv_][l] = s;
  }
#pragma unroll
  for (int n = 0; n < 12; ++n) {
    const double s = wave_sum_f64((double)v[n]);
    if (lane == 0) s_red[wv_][kHess + n] = s;
  }
  __syncthreads();
  if (t < kEdgeSums) {
    const double s = (s_red[0][t] + s_red[1][t]) + (s_red[2][t] + s_red[3][t]);
    if (t < kHess) {
      int n = 0;
      while ((n + 1) * (n + 2) / 2 <= t) ++n;  // t = n (n + 1) / 2 + m, m <= n
      const int m = t - n * (n + 1) / 2;
      Hf[e * 144 + n * 12 + m] = s;
      Hf[e * 144 + m * 12 + n] = s;
    } else {
      vf[e * 12 + (t - kHess)] = s;
    }
  }
}

// ---------------------------------------------------------------------------
// per-slot depth block
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kBaThreads) void k_ba_frame(
    const uint32_t* __restrict__ status, const int* __restrict__ kx, const int* __restrict__ estart,
    const int* __restrict__ elist, const float* __restrict__ disps, const float* __restrict__ disps_sens,
    const float* __restrict__ eta, int t0, int t1, int HW, const float* __restrict__ Ce,
    const float* __restrict__ bz, const float* __restrict__ Ei, float* __restrict__ C, float* __restrict__ w,
    float* __restrict__ Q, float* __restrict__ EiSum) {
  if (*status) return;
  const size_t k = blockIdx.y;
  const int p = blockIdx.x * kBaThreads + threadIdx.x;
  if (p >= HW) return;
  const int f = kx[k];
  const bool free_pose = f >= t0 && f < t1;
  float c = 0.f, b = 0.f, es[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int q = estart[k]; q < estart[k + 1]; ++q) {
    const size_t e = elist[q];
    c += Ce[e * HW + p];
    b += bz[e * HW + p];
    if (free_pose) {
#pragma unroll
      for (int n = 0; n < 6; ++n) es[n] += Ei[(e * 6 + n) * HW + p];
    }
  }
  const float s = disps_sens[(size_t)f * HW + p], dd = disps[(size_t)f * HW + p];
  if (s > 0.f) {  // a sensor disparity: the prior replaces eta
    c += kBaAlpha;
    b -= kBaAlpha * (dd - s);
  } else {
    c += eta[k * HW + p];
  }
  C[k * HW + p] = c;
  w[k * HW + p] = b;
  Q[k * HW + p] = 1.f / c;
#pragma unroll
  for (int n = 0; n < 6; ++n) EiSum[(k * 6 + n) * HW + p] = es[n];
}

// ---------------------------------------------------------------------------
// reduced system: one workgroup per block (a <= b)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kBaThreads) void k_ba_reduce(
    const uint32_t* __restrict__ status, const int* __restrict__ slot, const int* __restrict__ kx,
    const int* __restrict__ estart, const int* __restrict__ elist, const int* __restrict__ ejj, int N, int K,
    int t0, int P, int HW, int schur, const double* __restrict__ Hf, const double* __restrict__ vf,
    const float* __restrict__ Ej, const float* __restrict__ EiSum, const float* __restrict__ Q,
    const float* __restrict__ w, float lm, float ep, double* __restrict__ H, double* __restrict__ g) {
  if (*status) return;
  const int a = blockIdx.y, b = blockIdx.x;
  if (a > b) return;
  __shared__ double s_red[4][42];
  __shared__ double s_S[42];
  const int t = threadIdx.x, wv_ = t >> 6, lane = t & 63;
  const int fa = t0 + a, fb = t0 + b;
  double acc[36], sacc[6];
#pragma unroll
  for (int l = 0; l < 36; ++l) acc[l] = 0.0;
#pragma unroll
  for (int n = 0; n < 6; ++n) sacc[n] = 0.0;
  if (schur) {
    for (int k = 0; k < K; ++k) {  // (all of this control flow is workgroup-uniform)
      const int f = kx[k], e0 = estart[k], deg = estart[k + 1] - e0;
      const float* __restrict__ Qk = Q + (size_t)k * HW;
      const float* __restrict__ wk = w + (size_t)k * HW;
      // coupling -1 is the slot's own pose (present when f is free: f == fa says so)
      for (int c1 = -1; c1 < deg; ++c1) {
        const float* __restrict__ E1;
        if (c1 < 0) {
          if (f != fa) continue;
          E1 = EiSum + (size_t)k * 6 * HW;
        } else {
          if (ejj[e0 + c1] != fa) continue;
          E1 = Ej + (size_t)elist[e0 + c1] * 6 * HW;
        }
        if (a == b) {
          for (int p = t; p < HW; p += kBaThreads) {
            const float qw = Qk[p] * wk[p];
#pragma unroll
            for (int n = 0; n < 6; ++n) sacc[n] += (double)(E1[(size_t)n * HW + p] * qw);
          }
        }
        for (int c2 = -1; c2 < deg; ++c2) {
          const float* __restrict__ E2;
          if (c2 < 0) {
            if (f != fb) continue;
            E2 = EiSum + (size_t)k * 6 * HW;
          } else {
            if (ejj[e0 + c2] != fb) continue;
            E2 = Ej + (size_t)elist[e0 + c2] * 6 * HW;
          }
          for (int p = t; p < HW; p += kBaThreads) {
            const float q = Qk[p];
            float x1[6], x2[6];
#pragma unroll
            for (int n = 0; n < 6; ++n) {
              x1[n] = E1[(size_t)n * HW + p] * q;
              x2[n] = E2[(size_t)n * HW + p];
            }
#pragma unroll
            for (int n = 0; n < 6; ++n) {
#pragma unroll
              for (int m = 0; m < 6; ++m) acc[n * 6 + m] += (double)(x1[n] * x2[m]);
            }
          }
        }
      }
    }
#pragma unroll
    for (int l = 0; l < 36; ++l) {
      const double s = wave_sum_f64(acc[l]);
      if (lane == 0) s_red[wv_][l] = s;
    }
#pragma unroll
    for (int n = 0; n < 6; ++n) {
      const double s = wave_sum_f64(sacc[n]);
      if (lane == 0) s_red[wv_][36 + n] = s;
    }
  }
  __syncthreads();
  if (t < 42) s_S[t] = schur ? (s_red[0][t] + s_red[1][t]) + (s_red[2][t] + s_red[3][t]) : 0.0;
  __syncthreads();
  if (t >= 42) return;
  const int ld = 6 * P;
  const int qa0 = estart[slot[fa]], qa1 = estart[slot[fa] + 1];  // (a free frame always has a slot)
  if (t < 36) {
    int n = t / 6, m = t - n * 6;
    const bool mirror = a == b && n < m;  // a diagonal block is symmetric: computed once
    if (mirror) { const int q = n; n = m; m = q; }
    // the pose blocks of the edges between a and b, from the lists of the two
    // source frames (a stereo edge, ejj == its source, has no pose terms)
    double s = 0.0;
    if (a != b) {
      for (int q = qa0; q < qa1; ++q)  // a -> b: rows i, columns j
        if (ejj[q] == fb) s += Hf[(size_t)elist[q] * 144 + n * 12 + 6 + m];
      for (int q = estart[slot[fb]]; q < estart[slot[fb] + 1]; ++q)  // b -> a: rows j, columns i
        if (ejj[q] == fa) s += Hf[(size_t)elist[q] * 144 + (6 + n) * 12 + m];
    } else {
      for (int q = qa0; q < qa1; ++q)  // a is the source
        if (ejj[q] != fa) s += Hf[(size_t)elist[q] * 144 + n * 12 + m];
      for (int q = 0; q < N; ++q)  // a is the target
        if (ejj[q] == fa && (q < qa0 || q >= qa1)) s += Hf[(size_t)elist[q] * 144 + (6 + n) * 12 + 6 + m];
    }
    s -= s_S[n * 6 + m];
    if (a == b && n == m) s = s + ((double)ep + (double)lm * s);
    if (mirror) { const int q = n; n = m; m = q; }
    H[(size_t)(6 * a + n) * ld + 6 * b + m] = s;
    if (a != b) H[(size_t)(6 * b + m) * ld + 6 * a + n] = s;
  } else if (a == b) {
    const int n = t - 36;
    double s = 0.0;
    for (int q = qa0; q < qa1; ++q)
      if (ejj[q] != fa) s += vf[(size_t)elist[q] * 12 + n];
    for (int q = 0; q < N; ++q)
      if (ejj[q] == fa && (q < qa0 || q >= qa1)) s += vf[(size_t)elist[q] * 12 + 6 + n];
    g[6 * a + n] = s - s_S[36 + n];
  }
}

// ---------------------------------------------------------------------------
// fp64 Cholesky solve in one workgroup
// ---------------------------------------------------------------------------
// in-place lower Cholesky of the nb x nb matrix s (LDS, row stride ld) by the
// whole workgroup, one barrier per column: step j reads only column j (left
// unscaled: L_ij L_cj = s_ij s_cj / d) and writes columns > j, and scales
// column j - 1, which nobody reads any more.  false (workgroup-uniform) on a
// pivot that is not a positive finite number.
__device__ __forceinline__ bool chol_lds(double* s, int ld, int nb) {
  const int t = threadIdx.x, ty = t >> 4, tx = t & 15;
  double prev = 1.0;  // the square root of the previous pivot
  for (int j = 0; j < nb; ++j) {
    __syncthreads();
    const double d = s[j * ld + j];
    if (!(d > 0.0) || !(d < INFINITY)) return false;
    if (j > 0)
      for (int i = j - 1 + t; i < nb; i += kBaThreads) s[i * ld + j - 1] = i == j - 1 ? prev : s[i * ld + j - 1] / prev;
    const double inv = 1.0 / d;
    for (int i = j + 1 + ty; i < nb; i += 16) {
      const double lij = s[i * ld + j] * inv;
      for (int c = j + 1 + tx; c <= i; c += 16) s[i * ld + c] -= lij * s[c * ld + j];
    }
    prev = sqrt(d);
  }
  __syncthreads();
  if (t == 0) s[(nb - 1) * ld + nb - 1] = prev;
  __syncthreads();
  return true;
}

// the whole system in LDS (n <= kCholLds)
__global__ __launch_bounds__(kBaThreads) void k_ba_solve_lds(const uint32_t* __restrict__ status,
                                                             const double* __restrict__ H,
                                                             const double* __restrict__ g, int n,
                                                             float* __restrict__ dx, float* __restrict__ dx_out) {
  if (*status) return;
  __shared__ double s_L[kCholLds * kCholLds];
  __shared__ double s_y[kCholLds], s_x[kCholLds];
  const int t = threadIdx.x;
  for (int idx = t; idx < n * n; idx += kBaThreads) s_L[idx] = H[idx];
  for (int i = t; i < n; i += kBaThreads) s_y[i] = g[i];
  const bool ok = chol_lds(s_L, n, n);
  if (ok) {
    // one barrier per step: step j reads entry j (final since step j - 1) and
    // writes entries beyond it; the results go to the other array
    for (int j = 0; j < n; ++j) {  // L y = g: s_y -> s_x
      __syncthreads();
      const double yj = s_y[j] / s_L[j * n + j];
      if (t == 0) s_x[j] = yj;
      for (int i = j + 1 + t; i < n; i += kBaThreads) s_y[i] -= s_L[i * n + j] * yj;
    }
    for (int j = n - 1; j >= 0; --j) {  // L^T x = y: s_x -> s_y
      __syncthreads();
      const double xj = s_x[j] / s_L[j * n + j];
      if (t == 0) s_y[j] = xj;
      for (int i = t; i < j; i += kBaThreads) s_x[i] -= s_L[j * n + i] * xj;
    }
    __syncthreads();
  }
  for (int i = t; i < n; i += kBaThreads) {
    const float v = ok ? (float)s_y[i] : 0.f;
    dx[i] = v;
    if (dx_out != dx) dx_out[i] = v;
  }
}

// blocked through global memory: L [n, n] (a copy of H; its lower triangle
// becomes the factor) and y [n] are scratch.  Right-looking: the kCholBlock-wide diagonal block is factored in
// LDS, the panel below it solved one row per lane (the row in registers), and
// the trailing triangle updated in 64 x 64 tiles whose two panel pieces are
// staged in LDS (a 4 x 4 register tile per lane).
__global__ __launch_bounds__(kBaThreads) void k_ba_solve_global(const uint32_t* __restrict__ status,
                                                                const double* __restrict__ H,
                                                                const double* __restrict__ g, int n,
                                                                double* __restrict__ L, double* __restrict__ y,
                                                                float* __restrict__ dx,
                                                                float* __restrict__ dx_out) {
  if (*status) return;
  constexpr int B = kCholBlock, LD = kCholBlock + 1, T = 64;
  __shared__ double s_D[B * LD];
  __shared__ double s_A[T * LD], s_B[T * LD];
  __shared__ double s_x[B];
  const int t = threadIdx.x, ty = t >> 4, tx = t & 15;
  for (size_t idx = t; idx < (size_t)n * n; idx += kBaThreads) L[idx] = H[idx];
  for (int i = t; i < n; i += kBaThreads) y[i] = g[i];
  __syncthreads();
  bool ok = true;
  for (int j0 = 0; j0 < n; j0 += B) {
    const int nb = min(B, n - j0), r0 = j0 + nb;
    for (int idx = t; idx < nb * nb; idx += kBaThreads) {
      const int i = idx / nb, c = idx - i * nb;
      if (c <= i) s_D[i * LD + c] = L[(size_t)(j0 + i) * n + j0 + c];
    }
    ok = chol_lds(s_D, LD, nb);
    if (!ok) break;
    for (int idx = t; idx < nb * nb; idx += kBaThreads) {
      const int i = idx / nb, c = idx - i * nb;
      if (c <= i) L[(size_t)(j0 + i) * n + j0 + c] = s_D[i * LD + c];
    }
    if (r0 >= n) break;  // (the last block; every other block is B wide)
    // the panel below: row i of L_panel = A_panel L_D^-T
    for (int i = r0 + t; i < n; i += kBaThreads) {
      double* __restrict__ row = L + (size_t)i * n + j0;
      double r[B];
#pragma unroll
      for (int c = 0; c < B; ++c) r[c] = row[c];
#pragma unroll
      for (int c = 0; c < B; ++c) {
        asm volatile("" ::: "memory");  // (keeps the LDS reads of row c here: hoisted, all 528 spill)
        double acc = r[c];
#pragma unroll
        for (int k = 0; k < c; ++k) acc -= r[k] * s_D[c * LD + k];
        r[c] = acc / s_D[c * LD + c];
      }
#pragma unroll
      for (int c = 0; c < B; ++c) row[c] = r[c];
    }
    // the trailing lower triangle -= panel panel^T, tile by tile
    const int nt = (n - r0 + T - 1) / T;
    for (int ti = 0; ti < nt; ++ti) {
      for (int tc = 0; tc <= ti; ++tc) {
        const int I0 = r0 + T * ti, C0 = r0 + T * tc;
        __syncthreads();  // (the panel is written; the last tile's LDS reads are done)
        for (int idx = t; idx < T * B; idx += kBaThreads) {
          const int r = idx / B, k = idx - r * B;
          s_A[r * LD + k] = I0 + r < n ? L[(size_t)(I0 + r) * n + j0 + k] : 0.0;
          s_B[r * LD + k] = C0 + r < n ? L[(size_t)(C0 + r) * n + j0 + k] : 0.0;
        }
        __syncthreads();
        double acc[4][4];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int b = 0; b < 4; ++b) acc[a][b] = 0.0;
        for (int k = 0; k < B; ++k) {
          double va[4], vb[4];
#pragma unroll
          for (int a = 0; a < 4; ++a) {
            va[a] = s_A[(ty + 16 * a) * LD + k];
            vb[a] = s_B[(tx + 16 * a) * LD + k];
          }
#pragma unroll
          for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) acc[a][b] += va[a] * vb[b];
        }
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int b = 0; b < 4; ++b) {
            const int i = I0 + ty + 16 * a, c = C0 + tx + 16 * b;
            if (i < n && c <= i) L[(size_t)i * n + c] -= acc[a][b];
          }
      }
    }
    __syncthreads();
  }
  if (ok) {
    // L y = g, block by block: the diagonal block (staged in LDS) by wave 0,
    // lane i holding row i's value; then every row below takes the block's
    // part away
    for (int j0 = 0; j0 < n; j0 += B) {
      const int nb = min(B, n - j0), r0 = j0 + nb;
      __syncthreads();
      for (int idx = t; idx < nb * nb; idx += kBaThreads) {
        const int i = idx / nb, c = idx - i * nb;
        if (c <= i) s_D[i * LD + c] = L[(size_t)(j0 + i) * n + j0 + c];
      }
      __syncthreads();
      if (t < kWave) {
        double r = t < nb ? y[j0 + t] : 0.0;
        for (int c = 0; c < nb; ++c) {
          const double v = __shfl(r, c, kWave) / s_D[c * LD + c];
          if (t == c) r = v;
          else if (t > c && t < nb) r -= s_D[t * LD + c] * v;
        }
        if (t < nb) { s_x[t] = r; y[j0 + t] = r; }
      }
      __syncthreads();
      for (int i = r0 + t; i < n; i += kBaThreads) {
        const double* __restrict__ row = L + (size_t)i * n + j0;
        double acc = 0.0;
        for (int k = 0; k < nb; ++k) acc += row[k] * s_x[k];
        y[i] -= acc;
      }
    }
    // L^T x = y, from the last block up
    for (int j0 = ((n - 1) / B) * B; j0 >= 0; j0 -= B) {
      const int nb = min(B, n - j0);
      __syncthreads();
      for (int idx = t; idx < nb * nb; idx += kBaThreads) {
        const int i = idx / nb, c = idx - i * nb;
        if (c <= i) s_D[i * LD + c] = L[(size_t)(j0 + i) * n + j0 + c];
      }
      __syncthreads();
      if (t < kWave) {
        double r = t < nb ? y[j0 + t] : 0.0;
        for (int c = nb - 1; c >= 0; --c) {
          const double v = __shfl(r, c, kWave) / s_D[c * LD + c];
          if (t == c) r = v;
          else if (t < c) r -= s_D[c * LD + t] * v;
        }
        if (t < nb) { s_x[t] = r; y[j0 + t] = r; }
      }
      __syncthreads();
      for (int i = t; i < j0; i += kBaThreads) {
        double acc = 0.0;
        for (int k = 0; k < nb; ++k) acc += L[(size_t)(j0 + k) * n + i] * s_x[k];
        y[i] -= acc;
      }
    }
    __syncthreads();
  }
  for (int i = t; i < n; i += kBaThreads) {
    const float v = ok ? (float)y[i] : 0.f;
    dx[i] = v;
    if (dx_out != dx) dx_out[i] = v;
  }
}

// ---------------------------------------------------------------------------
// back-substitution and the two retractions
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kBaThreads) void k_ba_update(
    const uint32_t* __restrict__ status, const int* __restrict__ kx, const int* __restrict__ estart,
    const int* __restrict__ elist, const int64_t* __restrict__ jj, int t0, int P, int HW,
    const float* __restrict__ Ej, const float* __restrict__ EiSum, const float* __restrict__ Q,
    const float* __restrict__ w, const float* __restrict__ dx, float* __restrict__ dz,
    float* __restrict__ disps) {
  if (*status) return;
  const size_t k = blockIdx.y;
  const int p = blockIdx.x * kBaThreads + threadIdx.x;
  if (p >= HW) return;
  const int f = kx[k];
  float s = 0.f;
  // a coupling whose pose is t0 itself (index 0) is left out, as in the
  // reference (the recorded quirk of the back-substitution)
  {
    const int64_t ix = (int64_t)f - t0;
    if (ix > 0 && ix < P) {
#pragma unroll
      for (int n = 0; n < 6; ++n) s += EiSum[(k * 6 + n) * HW + p] * dx[ix * 6 + n];
    }
  }
  for (int q = estart[k]; q < estart[k + 1]; ++q) {
    const size_t e = elist[q];
    const int64_t ix = jj[e] - t0;
    if (ix > 0 && ix < P) {
#pragma unroll
      for (int n = 0; n < 6; ++n) s += Ej[(e * 6 + n) * HW + p] * dx[ix * 6 + n];
    }
  }
  const float step = Q[k * HW + p] * (w[k * HW + p] - s);
  dz[k * HW + p] = step;
  disps[(size_t)f * HW + p] += step;
}

// poses[t0 + i] <- exp(dx[i]) poses[t0 + i]
__global__ __launch_bounds__(kBaThreads) void k_ba_retract(const uint32_t* __restrict__ status,
                                                           float* __restrict__ poses, const float* __restrict__ dx,
                                                           int t0, int P) {
  if (*status) return;
  const int i = blockIdx.x * kBaThreads + threadIdx.x;
  if (i >= P) return;
  const float* xi = dx + 6 * (size_t)i;
  const f3 tau = mk3(xi[0], xi[1], xi[2]), phi = mk3(xi[3], xi[4], xi[5]);
  const float th2 = dot3(phi, phi), th = sqrtf(th2);
  float imag, real;
  if (th2 < 1e-8f) {
    imag = 0.5f - (1.f / 48.f) * th2 + (1.f / 3840.f) * th2 * th2;
    real = 1.f - (1.f / 8.f) * th2 + (1.f / 384.f) * th2 * th2;
  } else {
    imag = sinf(0.5f * th) / th;
    real = cosf(0.5f * th);
  }
  const Pose dq = Pose{imag * phi.x, imag * phi.y, imag * phi.z, real, 0.f, 0.f, 0.f};
  f3 dt = tau;
  if (th > 1e-4f) {  // V(phi) tau
    const f3 c1 = cross3(phi, tau), c2 = cross3(phi, c1);
    dt = add3(dt, add3(scl3((1.f - cosf(th)) / th2, c1), scl3((th - sinf(th)) / (th * th2), c2)));
  }
  float* p = poses + 7 * (size_t)(t0 + i);
  const Pose q = load_pose(p, 0);
  const f3 t1 = add3(rotate(dq, mk3(q.tx, q.ty, q.tz)), dt);
  p[0] = t1.x; p[1] = t1.y; p[2] = t1.z;
  p[3] = dq.qw * q.qx + dq.qx * q.qw + dq.qy * q.qz - dq.qz * q.qy;
  p[4] = dq.qw * q.qy + dq.qy * q.qw + dq.qz * q.qx - dq.qx * q.qz;
  p[5] = dq.qw * q.qz + dq.qz * q.qw + dq.qx * q.qy - dq.qy * q.qx;
  p[6] = dq.qw * q.qw - dq.qx * q.qx - dq.qy * q.qy - dq.qz * q.qz;
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
struct BaDims {
  int num, ht, wd, N, t0, t1, K;
};

const char* ba_dims_error(const BaDims& d) {
  if (d.num <= 0 || d.ht <= 0 || d.wd <= 0 || (int64_t)d.ht * d.wd >= (int64_t(1) << 30)) return "bad frame shape";
  if (d.N <= 0) return "no edges";
  if (d.t0 < 0 || d.t1 <= d.t0 || d.t1 > d.num) return "need 0 <= t0 < t1 <= num";
  if (d.K < d.t1 - d.t0 || d.K > d.num) return "eta must have between t1 - t0 and num rows";
  if (d.K > 65535 || d.t1 - d.t0 > 65535) return "more than 65535 frames";
  return nullptr;
}

struct BaLayout {  // byte offsets into the workspace
  size_t slot, kx, estart, elist, ejj, Hf, vf, H, g, L, y, dx, Ei, Ej, Ce, bz, C, w, Q, EiSum, total;
};

BaLayout ba_layout(const BaDims& d) {
  BaLayout o;
  size_t at = 0;
  auto take = [&](size_t bytes) {
    const size_t here = at;
    at += (bytes + 255) & ~size_t(255);
    return here;
  };
  const size_t HW = (size_t)d.ht * d.wd, N = d.N, K = d.K, n = 6 * (size_t)(d.t1 - d.t0);
  o.slot = take(4 * (size_t)d.num);
  o.kx = take(4 * K);
  o.estart = take(4 * (K + 1));
  o.elist = take(4 * N);
  o.ejj = take(4 * N);
  o.Hf = take(8 * 144 * N);
  o.vf = take(8 * 12 * N);
  o.H = take(8 * n * n);
  o.g = take(8 * n);
  o.L = take(n > (size_t)kCholLds ? 8 * n * n : 0);
  o.y = take(8 * n);
  o.dx = take(4 * n);
  o.Ei = take(4 * 6 * HW * N);
  o.Ej = take(4 * 6 * HW * N);
  o.Ce = take(4 * HW * N);
  o.bz = take(4 * HW * N);
  o.C = take(4 * HW * K);
  o.w = take(4 * HW * K);
  o.Q = take(4 * HW * K);
  o.EiSum = take(4 * 6 * HW * K);
  o.total = at;
  return o;
}

struct BaArgs {
  float* poses;
  float* disps;
  const float *intrinsics, *disps_sens, *targets, *weights, *eta;
  const int64_t *ii, *jj;
  BaDims d;
  float lm, ep;
  bool motion_only;
  uint32_t* status;
  hipStream_t s;
};

// wgsr_droid_ba_stage_events: five events recorded around the stages of every
// iteration this thread launches (null: off)
thread_local hipEvent_t* g_stage_events = nullptr;
void stage_mark(int k, hipStream_t s) {
  if (g_stage_events) (void)hipEventRecord(g_stage_events[k], s);
}

template <class T> T* ws_ptr(void* ws, size_t off) { return reinterpret_cast<T*>(static_cast<char*>(ws) + off); }

hipError_t ba_setup(const BaArgs& a, void* ws, const BaLayout& o) {
  hipLaunchKernelGGL(k_ba_setup, dim3(1), dim3(kBaThreads), 0, a.s, a.ii, a.jj, a.d.N, a.d.num, a.d.K, a.d.t0,
                     a.d.t1, ws_ptr<int>(ws, o.slot), ws_ptr<int>(ws, o.kx), ws_ptr<int>(ws, o.estart), ws_ptr<int>(ws, o.elist),
                     ws_ptr<int>(ws, o.ejj), a.status);
  return hipGetLastError();
}

// one linearisation and solve: H, g (and C, w unless motion_only) into the
// given buffers, dx into the workspace and into dx_out
hipError_t ba_linearise_solve(const BaArgs& a, void* ws, const BaLayout& o, double* H, double* g, float* C, float* w,
                              float* dx_out) {
  const BaDims& d = a.d;
  const int HW = d.ht * d.wd, P = d.t1 - d.t0, n = 6 * P, schur = a.motion_only ? 0 : 1;
  const unsigned px = (unsigned)((HW + kBaThreads - 1) / kBaThreads);
  const int *kx = ws_ptr<int>(ws, o.kx), *estart = ws_ptr<int>(ws, o.estart), *elist = ws_ptr<int>(ws, o.elist);
  stage_mark(0, a.s);
  hipLaunchKernelGGL(k_ba_edge, dim3((unsigned)d.N), dim3(kBaThreads), 0, a.s, a.status, a.poses, a.disps,
                     a.intrinsics, a.targets, a.weights, a.ii, a.jj, d.ht, d.wd, schur, ws_ptr<float>(ws, o.Ei),
                     ws_ptr<float>(ws, o.Ej), ws_ptr<float>(ws, o.Ce), ws_ptr<float>(ws, o.bz), ws_ptr<double>(ws, o.Hf),
                     ws_ptr<double>(ws, o.vf));
  if (schur)
    hipLaunchKernelGGL(k_ba_frame, dim3(px, (unsigned)d.K), dim3(kBaThreads), 0, a.s, a.status, kx, estart, elist,
                       a.disps, a.disps_sens, a.eta, d.t0, d.t1, HW, ws_ptr<float>(ws, o.Ce), ws_ptr<float>(ws, o.bz),
                       ws_ptr<float>(ws, o.Ei), C, w, ws_ptr<float>(ws, o.Q), ws_ptr<float>(ws, o.EiSum));
  stage_mark(1, a.s);
  hipLaunchKernelGGL(k_ba_reduce, dim3((unsigned)P, (unsigned)P), dim3(kBaThreads), 0, a.s, a.status,
                     ws_ptr<int>(ws, o.slot), kx, estart, elist, ws_ptr<int>(ws, o.ejj), d.N, d.K, d.t0, P, HW, schur, ws_ptr<double>(ws, o.Hf), ws_ptr<double>(ws, o.vf),
                     ws_ptr<float>(ws, o.Ej), ws_ptr<float>(ws, o.EiSum), ws_ptr<float>(ws, o.Q), w, a.lm, a.ep, H, g);
  stage_mark(2, a.s);
  float* dx = ws_ptr<float>(ws, o.dx);
  if (n <= kCholLds)
    hipLaunchKernelGGL(k_ba_solve_lds, dim3(1), dim3(kBaThreads), 0, a.s, a.status, H, g, n, dx, dx_out);
  else
    hipLaunchKernelGGL(k_ba_solve_global, dim3(1), dim3(kBaThreads), 0, a.s, a.status, H, g, n,
                       ws_ptr<double>(ws, o.L), ws_ptr<double>(ws, o.y), dx, dx_out);
  stage_mark(3, a.s);
  return hipGetLastError();
}

int ba_check(const char* who, const BaArgs& a, const void* ws, int64_t ws_bytes, BaLayout* o) {
  if (const char* msg = ba_dims_error(a.d))
    return set_error(WGSR_EINVAL, "%s: %s (num=%d ht=%d wd=%d n_edges=%d t0=%d t1=%d K=%d)", who, msg, a.d.num,
                     a.d.ht, a.d.wd, a.d.N, a.d.t0, a.d.t1, a.d.K);
  if (!a.poses || !a.disps || !a.intrinsics || !a.disps_sens || !a.targets || !a.weights || !a.eta || !a.ii ||
      !a.jj || !a.status || !ws)
    return set_error(WGSR_EINVAL, "%s: null pointer", who);
  *o = ba_layout(a.d);
  if (ws_bytes < 0 || (uint64_t)ws_bytes < o->total)
    return set_error(WGSR_EINVAL, "%s: workspace of %lld bytes, need %llu", who, (long long)ws_bytes,
                     (unsigned long long)o->total);
  if (reinterpret_cast<uintptr_t>(ws) & 7) return set_error(WGSR_EINVAL, "%s: workspace must be 8-byte aligned", who);
  return WGSR_OK;
}

}  // namespace

}  // namespace wgsr

using namespace wgsr;

extern "C" {

int64_t wgsr_droid_ba_workspace_bytes(int num, int ht, int wd, int n_edges, int t0, int t1, int K) {
  const BaDims d{num, ht, wd, n_edges, t0, t1, K};
  if (const char* msg = ba_dims_error(d)) {
    set_error(WGSR_EINVAL, "wgsr_droid_ba_workspace_bytes: %s (num=%d ht=%d wd=%d n_edges=%d t0=%d t1=%d K=%d)", msg,
              num, ht, wd, n_edges, t0, t1, K);
    return -1;
  }
  return (int64_t)ba_layout(d).total;
}

void wgsr_droid_ba_stage_events(void** events) { g_stage_events = reinterpret_cast<hipEvent_t*>(events); }

int wgsr_droid_ba(float* poses, float* disps, const float* intrinsics, const float* disps_sens,
                  const float* targets, const float* weights, const float* eta, const int64_t* ii,
                  const int64_t* jj, int num, int ht, int wd, int n_edges, int K, int t0, int t1, int iterations,
                  float lm, float ep, int motion_only, int depth_only, void* workspace, int64_t workspace_bytes,
                  float* dx, float* dz, uint32_t* status, void* stream) {
  const char* who = "wgsr_droid_ba";
  const BaArgs a{poses, disps, intrinsics, disps_sens, targets, weights, eta, ii, jj,
                 BaDims{num, ht, wd, n_edges, t0, t1, K}, lm, ep, motion_only != 0, status, (hipStream_t)stream};
  BaLayout o;
  if (const int c = ba_check(who, a, workspace, workspace_bytes, &o)) return c;
  if (iterations < 0) return set_error(WGSR_EINVAL, "%s: iterations=%d", who, iterations);
  if (!dx || (!a.motion_only && !dz)) return set_error(WGSR_EINVAL, "%s: null output", who);
  hipError_t e = ba_setup(a, workspace, o);
  const int HW = ht * wd, P = t1 - t0;
  const unsigned px = (unsigned)((HW + kBaThreads - 1) / kBaThreads);
  for (int it = 0; it < iterations && e == hipSuccess; ++it) {
    e = ba_linearise_solve(a, workspace, o, ws_ptr<double>(workspace, o.H), ws_ptr<double>(workspace, o.g),
                           ws_ptr<float>(workspace, o.C), ws_ptr<float>(workspace, o.w), dx);
    if (e != hipSuccess) break;
    if (!a.motion_only)
      hipLaunchKernelGGL(k_ba_update, dim3(px, (unsigned)K), dim3(kBaThreads), 0, a.s, status,
                         ws_ptr<int>(workspace, o.kx), ws_ptr<int>(workspace, o.estart), ws_ptr<int>(workspace, o.elist), jj, t0,
                         P, HW, ws_ptr<float>(workspace, o.Ej), ws_ptr<float>(workspace, o.EiSum),
                         ws_ptr<float>(workspace, o.Q), ws_ptr<float>(workspace, o.w), ws_ptr<float>(workspace, o.dx), dz,
                         disps);
    if (a.motion_only || !depth_only)
      hipLaunchKernelGGL(k_ba_retract, dim3((unsigned)((P + kBaThreads - 1) / kBaThreads)), dim3(kBaThreads), 0, a.s,
                         status, poses, ws_ptr<float>(workspace, o.dx), t0, P);
    stage_mark(4, a.s);
    e = hipGetLastError();
  }
  return e == hipSuccess ? WGSR_OK : set_error(WGSR_EHIP, "%s: %s", who, hipGetErrorString(e));
}

int wgsr_droid_ba_system(const float* poses, const float* disps, const float* intrinsics, const float* disps_sens,
                         const float* targets, const float* weights, const float* eta, const int64_t* ii,
                         const int64_t* jj, int num, int ht, int wd, int n_edges, int K, int t0, int t1, float lm,
                         float ep, int motion_only, void* workspace, int64_t workspace_bytes, double* H, double* g,
                         float* C, float* w, float* dx, uint32_t* status, void* stream) {
  const char* who = "wgsr_droid_ba_system";
  const BaArgs a{const_cast<float*>(poses), const_cast<float*>(disps), intrinsics, disps_sens, targets, weights, eta,
                 ii, jj, BaDims{num, ht, wd, n_edges, t0, t1, K}, lm, ep, motion_only != 0, status,
                 (hipStream_t)stream};
  BaLayout o;
  if (const int c = ba_check(who, a, workspace, workspace_bytes, &o)) return c;
  if (!H || !g || !dx || (!a.motion_only && (!C || !w))) return set_error(WGSR_EINVAL, "%s: null output", who);
  if ((reinterpret_cast<uintptr_t>(H) | reinterpret_cast<uintptr_t>(g)) & 7)
    return set_error(WGSR_EINVAL, "%s: H and g must be 8-byte aligned", who);
  hipError_t e = ba_setup(a, workspace, o);
  if (e == hipSuccess) e = ba_linearise_solve(a, workspace, o, H, g, C, w, dx);
  return e == hipSuccess ? WGSR_OK : set_error(WGSR_EHIP, "%s: %s", who, hipGetErrorString(e));
}

}  // extern "C"
