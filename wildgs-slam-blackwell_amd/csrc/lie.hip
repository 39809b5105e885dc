// lietorch's SE3 for gfx950: the group operations behind python/lietorch, and
// the fused reprojection of the tracker's update loop
// (projective_ops.projective_transform; wgsr.frontend.reproject).
//
// Conventions: a group element is 7 floats (tx, ty, tz, qx, qy, qz, qw), the
// layout droid_pose.h::load_pose reads; a tangent vector is 6 floats (tau,
// phi), translation part first.  fp32 only, inference only.
//
// Group kernels: one lane per output element.  An operand is (pointer,
// inner): output element e reads operand element e / inner, so a pose
// broadcast over trailing dimensions (G[:, :, None, None] * X) is never
// materialised.  A quaternion is never renormalised.
//   exp   q = (a phi, cos(theta / 2)), t = tau + b phi x tau + c phi x (phi x tau)
//         with a = sin(theta / 2) / theta, b = (1 - cos theta) / theta^2 = 2 a^2
//         (no cancellation), c = (theta - sin theta) / theta^3; a and c by their
//         series below theta = 0.25 (next term < 1e-12).
//   log   q -> -q when qw < 0; phi = s qv with s = 2 atan2(|qv|, qw) / |qv|
//         (series below |qv| = 1e-4); tau = t - phi x t / 2 + d phi x (phi x t),
//         d = (1 - (theta / 2) cot(theta / 2)) / theta^2 with cot(theta / 2) =
//         qw / |qv| (series below theta = 0.25).
//
// k_reproject: one workgroup owns 256 consecutive pixels of one edge.  Thread
//   0 forms the edge's transform G_ij = G_j G_i^-1 (or the fixed stereo
//   transform when i == j) once, as a rotation matrix and a translation in
//   LDS next to the two frames' intrinsics.  A lane reads its pixel's
//   disparity (coalesced) and writes coords as one 8-byte store (three 4-byte
//   stores with the depth slot), valid as 4 bytes and, with Jacobians, Jz as
//   one 8-byte store.  Jj and Ji are 48 bytes per pixel: each wave stages its
//   64 blocks in LDS and writes them back as three 16-byte stores per lane to
//   consecutive addresses (1 KiB per instruction; written straight from the
//   lanes, an instruction would touch a third of each of 24 lines).  An edge
//   whose index is outside [0, num) reads nothing and gets NaN.
#include <math.h>

#include "wgsr_common.h"
#include "wgsr_internal.h"
#include "droid_pose.h"

namespace wgsr {

namespace {

constexpr float kSeriesTheta = 0.25f;  // a, c, d by series below this angle
constexpr float kLogSmall = 1e-4f;     // atan2(n, w) / n by series below this |qv|
constexpr float kReprojMinDepth = 0.2f;  // projective_ops.MIN_DEPTH (not droid_pose.h's kMinDepth)

__device__ __forceinline__ void store_pose(float* __restrict__ o, const Pose& p) {
  o[0] = p.tx; o[1] = p.ty; o[2] = p.tz; o[3] = p.qx; o[4] = p.qy; o[5] = p.qz; o[6] = p.qw;
}

__device__ __forceinline__ Pose se3_exp(const float* __restrict__ xi) {
  const f3 tau = mk3(xi[0], xi[1], xi[2]), phi = mk3(xi[3], xi[4], xi[5]);
  const float th2 = dot3(phi, phi), th = sqrtf(th2);
  float a, c;
  if (th < kSeriesTheta) {
    a = 0.5f + th2 * (-1.f / 48.f + th2 * (1.f / 3840.f + th2 * (-1.f / 645120.f)));
    c = 1.f / 6.f + th2 * (-1.f / 120.f + th2 * (1.f / 5040.f + th2 * (-1.f / 362880.f)));
  } else {
    a = sinf(0.5f * th) / th;
    c = (th - sinf(th)) / (th2 * th);
  }
  const float b = 2.f * a * a;
  const f3 w1 = cross3(phi, tau), w2 = cross3(phi, w1);
  Pose r;
  r.qx = a * phi.x; r.qy = a * phi.y; r.qz = a * phi.z; r.qw = cosf(0.5f * th);
  r.tx = tau.x + (b * w1.x + c * w2.x);
  r.ty = tau.y + (b * w1.y + c * w2.y);
  r.tz = tau.z + (b * w1.z + c * w2.z);
  return r;
}

__device__ __forceinline__ void se3_log(const Pose& p, float* __restrict__ o) {
  const float sg = p.qw < 0.f ? -1.f : 1.f;
  const f3 u = mk3(sg * p.qx, sg * p.qy, sg * p.qz);
  const float w = sg * p.qw;
  const float n2 = dot3(u, u), n = sqrtf(n2);
  float s;
  if (n < kLogSmall) {
    s = (2.f / w) * (1.f - n2 / (w * w) / 3.f);
  } else {
    s = 2.f * atan2f(n, w) / n;
  }
  const f3 phi = scl3(s, u);
  const float th = s * n, th2 = th * th;
  float d;
  if (th < kSeriesTheta) {
    d = 1.f / 12.f + th2 * (1.f / 720.f + th2 * (1.f / 30240.f + th2 * (1.f / 1209600.f)));
  } else {
    d = (1.f - 0.5f * th * w / n) / th2;
  }
  const f3 t = mk3(p.tx, p.ty, p.tz);
  const f3 w1 = cross3(phi, t), w2 = cross3(phi, w1);
  o[0] = t.x + (d * w2.x - 0.5f * w1.x);
  o[1] = t.y + (d * w2.y - 0.5f * w1.y);
  o[2] = t.z + (d * w2.z - 0.5f * w1.z);
  o[3] = phi.x; o[4] = phi.y; o[5] = phi.z;
}

__device__ __forceinline__ Pose se3_conj(const Pose& p) {  // rotation part inverted, translation kept
  Pose r = p;
  r.qx = -p.qx; r.qy = -p.qy; r.qz = -p.qz;
  return r;
}

__device__ __forceinline__ Pose se3_inv(const Pose& p) {
  Pose r = se3_conj(p);
  const f3 t = rotate(r, mk3(p.tx, p.ty, p.tz));
  r.tx = -t.x; r.ty = -t.y; r.tz = -t.z;
  return r;
}

__device__ __forceinline__ Pose se3_mul(const Pose& a, const Pose& b) {
  const f3 av = mk3(a.qx, a.qy, a.qz), bv = mk3(b.qx, b.qy, b.qz);
  const f3 cr = cross3(av, bv);
  Pose r;
  r.qw = a.qw * b.qw - dot3(av, bv);
  r.qx = a.qw * bv.x + b.qw * av.x + cr.x;
  r.qy = a.qw * bv.y + b.qw * av.y + cr.y;
  r.qz = a.qw * bv.z + b.qw * av.z + cr.z;
  const f3 t = rotate(a, mk3(b.tx, b.ty, b.tz));
  r.tx = a.tx + t.x; r.ty = a.ty + t.y; r.tz = a.tz + t.z;
  return r;
}

// the rotation matrix of q (row-major 3 x 3), the polynomial of rotate()
__device__ __forceinline__ void quat_matrix(const Pose& p, float* __restrict__ R) {
  const float x = p.qx, y = p.qy, z = p.qz, w = p.qw;
  R[0] = 1.f - 2.f * (y * y + z * z); R[1] = 2.f * (x * y - w * z); R[2] = 2.f * (x * z + w * y);
  R[3] = 2.f * (x * y + w * z); R[4] = 1.f - 2.f * (x * x + z * z); R[5] = 2.f * (y * z - w * x);
  R[6] = 2.f * (x * z - w * y); R[7] = 2.f * (y * z + w * x); R[8] = 1.f - 2.f * (x * x + y * y);
}

enum LieOp {
  kExp = WGSR_LIE_EXP, kLog = WGSR_LIE_LOG, kInv = WGSR_LIE_INV, kMul = WGSR_LIE_MUL, kAct3 = WGSR_LIE_ACT3,
  kAct4 = WGSR_LIE_ACT4, kMatrix = WGSR_LIE_MATRIX, kAdj = WGSR_LIE_ADJ, kAdjT = WGSR_LIE_ADJT,
  kRetr = WGSR_LIE_RETR
};

// floats per element of the operands and of the result (0: no second operand)
__host__ __device__ constexpr int lie_dim_a(int op) { return op == kExp ? 6 : 7; }
__host__ __device__ constexpr int lie_dim_b(int op) {
  return op == kMul ? 7 : op == kAct3 ? 3 : op == kAct4 ? 4 : (op == kAdj || op == kAdjT || op == kRetr) ? 6 : 0;
}
__host__ __device__ constexpr int lie_dim_out(int op) {
  return op == kLog ? 6 : op == kAct3 ? 3 : op == kAct4 ? 4 : op == kMatrix ? 16 : (op == kAdj || op == kAdjT) ? 6 : 7;
}

template <int OP>
__global__ __launch_bounds__(256) void k_lie_se3(const float* __restrict__ a, int64_t inner_a,
                                                 const float* __restrict__ b, int64_t inner_b,
                                                 float* __restrict__ out, int64_t n) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  const int64_t ea = inner_a == 1 ? e : e / inner_a;
  float* __restrict__ o = out + lie_dim_out(OP) * e;
  if constexpr (OP == kExp) {
    store_pose(o, se3_exp(a + 6 * ea));
    return;
  } else {
    const Pose X = load_pose(a, ea);
    const float* __restrict__ pb = nullptr;
    if constexpr (lie_dim_b(OP) != 0) pb = b + lie_dim_b(OP) * (inner_b == 1 ? e : e / inner_b);
    if constexpr (OP == kLog) {
      se3_log(X, o);
    } else if constexpr (OP == kInv) {
      store_pose(o, se3_inv(X));
    } else if constexpr (OP == kMul) {
      store_pose(o, se3_mul(X, load_pose(pb, 0)));
    } else if constexpr (OP == kAct3) {
      const f3 r = rotate(X, mk3(pb[0], pb[1], pb[2]));
      o[0] = r.x + X.tx; o[1] = r.y + X.ty; o[2] = r.z + X.tz;
    } else if constexpr (OP == kAct4) {
      const f3 r = rotate(X, mk3(pb[0], pb[1], pb[2]));
      const float w = pb[3];
      o[0] = r.x + w * X.tx; o[1] = r.y + w * X.ty; o[2] = r.z + w * X.tz; o[3] = w;
    } else if constexpr (OP == kMatrix) {
      float R[9];
      quat_matrix(X, R);
      o[0] = R[0]; o[1] = R[1]; o[2] = R[2]; o[3] = X.tx;
      o[4] = R[3]; o[5] = R[4]; o[6] = R[5]; o[7] = X.ty;
      o[8] = R[6]; o[9] = R[7]; o[10] = R[8]; o[11] = X.tz;
      o[12] = 0.f; o[13] = 0.f; o[14] = 0.f; o[15] = 1.f;
    } else if constexpr (OP == kAdj) {  // (R tau + t x R phi, R phi)
      const f3 rt = rotate(X, mk3(pb[0], pb[1], pb[2])), rp = rotate(X, mk3(pb[3], pb[4], pb[5]));
      const f3 c = cross3(mk3(X.tx, X.ty, X.tz), rp);
      o[0] = rt.x + c.x; o[1] = rt.y + c.y; o[2] = rt.z + c.z; o[3] = rp.x; o[4] = rp.y; o[5] = rp.z;
    } else if constexpr (OP == kAdjT) {  // (R^T tau, R^T (phi - t x tau))
      const Pose Xc = se3_conj(X);
      const f3 tau = mk3(pb[0], pb[1], pb[2]);
      const f3 c = cross3(mk3(X.tx, X.ty, X.tz), tau);
      const f3 rt = rotate(Xc, tau), rp = rotate(Xc, mk3(pb[3] - c.x, pb[4] - c.y, pb[5] - c.z));
      o[0] = rt.x; o[1] = rt.y; o[2] = rt.z; o[3] = rp.x; o[4] = rp.y; o[5] = rp.z;
    } else {  // kRetr: exp(a) X
      static_assert(OP == kRetr, "unknown op");
      store_pose(o, se3_mul(se3_exp(pb), X));
    }
  }
}

template <int OP>
hipError_t launch_lie(const float* a, int64_t inner_a, const float* b, int64_t inner_b, float* out, int64_t n,
                      hipStream_t s) {
  hipLaunchKernelGGL(k_lie_se3<OP>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a, inner_a, b, inner_b, out,
                     n);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// reprojection
// ---------------------------------------------------------------------------
struct ReprojEdge {
  float R[9], t[3];  // G_ij
  float Ki[4], Kj[4];  // (fx, fy, cx, cy) of frames i and j
};

template <bool JAC, bool DEPTH>
__global__ __launch_bounds__(256) void k_reproject(const float* __restrict__ poses, const float* __restrict__ disps,
                                                   const float* __restrict__ intrinsics, int intr_stride, int num,
                                                   int ht, int wd, const int64_t* __restrict__ ii,
                                                   const int64_t* __restrict__ jj, int groups,
                                                   float* __restrict__ coords, float* __restrict__ valid,
                                                   float* __restrict__ Ji, float* __restrict__ Jj,
                                                   float* __restrict__ Jz) {
  __shared__ ReprojEdge s_e;
  const int t = threadIdx.x;
  const int e = blockIdx.x / groups;
  const int k = (int)(blockIdx.x - (unsigned)e * groups) * 256 + t;
  const int total = ht * wd;
  const int64_t fi = ii[e], fj = jj[e];
  const bool bad = fi < 0 || fi >= num || fj < 0 || fj >= num;  // (block-uniform)
  if (t == 0 && !bad) {
    Pose G;
    if (fi == fj) {  // the fixed stereo baseline
      G = Pose{0.f, 0.f, 0.f, 1.f, -0.1f, 0.f, 0.f};
    } else {
      G = se3_mul(load_pose(poses, fj), se3_inv(load_pose(poses, fi)));
    }
    quat_matrix(G, s_e.R);
    s_e.t[0] = G.tx; s_e.t[1] = G.ty; s_e.t[2] = G.tz;
    for (int c = 0; c < 4; ++c) {
      s_e.Ki[c] = intrinsics[fi * intr_stride + c];
      s_e.Kj[c] = intrinsics[fj * intr_stride + c];
    }
  }
  __syncthreads();
  const bool live = k < total;  // (a lane past the last pixel computes on d = 1 and stores nothing)
  const size_t px = (size_t)e * total + k;
  constexpr int CD = DEPTH ? 3 : 2;
  if (bad) {
    if (!live) return;
    const float nan = __builtin_nanf("");
    for (int c = 0; c < CD; ++c) coords[CD * px + c] = nan;
    valid[px] = nan;
    if constexpr (JAC) {
      for (int c = 0; c < 12; ++c) { Ji[12 * px + c] = nan; Jj[12 * px + c] = nan; }
      Jz[2 * px] = nan; Jz[2 * px + 1] = nan;
    }
    return;
  }
  if constexpr (!JAC) {
    if (!live) return;
  }
  const int row = k / wd, col = k - row * wd;
  const float d = live ? disps[(size_t)fi * total + k] : 1.f;
  const float* __restrict__ R = s_e.R;
  const float tx = s_e.t[0], ty = s_e.t[1], tz = s_e.t[2];
  const float X0 = ((float)col - s_e.Ki[2]) / s_e.Ki[0], Y0 = ((float)row - s_e.Ki[3]) / s_e.Ki[1];
  const float X = (R[0] * X0 + R[1] * Y0 + R[2]) + d * tx;
  const float Y = (R[3] * X0 + R[4] * Y0 + R[5]) + d * ty;
  const float Z = (R[6] * X0 + R[7] * Y0 + R[8]) + d * tz;
  const float fx = s_e.Kj[0], fy = s_e.Kj[1], cx = s_e.Kj[2], cy = s_e.Kj[3];
  const float Zp = Z < 0.5f * kReprojMinDepth ? 1.f : Z;
  const float dz = 1.f / Zp;
  const float x = fx * (X * dz) + cx, y = fy * (Y * dz) + cy;
  if (live) {
    if constexpr (DEPTH) {
      coords[3 * px] = x; coords[3 * px + 1] = y; coords[3 * px + 2] = d * dz;
    } else {
      reinterpret_cast<float2*>(coords)[px] = make_float2(x, y);
    }
    valid[px] = (Z > kReprojMinDepth && 1.f > kReprojMinDepth) ? 1.f : 0.f;
  }
  if constexpr (JAC) {
    const float p00 = fx * dz, p02 = -fx * X * dz * dz, p11 = fy * dz, p12 = -fy * Y * dz * dz;
    __shared__ float4 s_stage[2][4][192];  // [Jj | Ji][wave][64 pixels x 3]
    // Jj = Jp Ja, rows (tau, phi)
    const float a0 = p00 * d, a1 = 0.f, a2 = p02 * d, a3 = p02 * Y, a4 = p00 * Z - p02 * X, a5 = -p00 * Y;
    const float b0 = 0.f, b1 = p11 * d, b2 = p12 * d, b3 = p12 * Y - p11 * Z, b4 = -p12 * X, b5 = p11 * X;
    // a pixel's 2 x 6 block is 48 bytes: the wave's 64 blocks go through LDS
    // so that each store instruction writes 1 KiB of consecutive addresses
    float4* __restrict__ sj = s_stage[0][t >> 6], * __restrict__ si = s_stage[1][t >> 6];
    const int lane = t & 63;
    sj[3 * lane] = make_float4(a0, a1, a2, a3);
    sj[3 * lane + 1] = make_float4(a4, a5, b0, b1);
    sj[3 * lane + 2] = make_float4(b2, b3, b4, b5);
    // Ji = -adjT_Gij(row) = -(R^T tau, R^T (phi - t x tau))
    float r[2][6];
    const float rows[2][6] = {{a0, a1, a2, a3, a4, a5}, {b0, b1, b2, b3, b4, b5}};
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const float u0 = rows[q][0], u1 = rows[q][1], u2 = rows[q][2];
      const float v0 = rows[q][3] - (ty * u2 - tz * u1), v1 = rows[q][4] - (tz * u0 - tx * u2),
                  v2 = rows[q][5] - (tx * u1 - ty * u0);
      r[q][0] = -(R[0] * u0 + R[3] * u1 + R[6] * u2);
      r[q][1] = -(R[1] * u0 + R[4] * u1 + R[7] * u2);
      r[q][2] = -(R[2] * u0 + R[5] * u1 + R[8] * u2);
      r[q][3] = -(R[0] * v0 + R[3] * v1 + R[6] * v2);
      r[q][4] = -(R[1] * v0 + R[4] * v1 + R[7] * v2);
      r[q][5] = -(R[2] * v0 + R[5] * v1 + R[8] * v2);
    }
    si[3 * lane] = make_float4(r[0][0], r[0][1], r[0][2], r[0][3]);
    si[3 * lane + 1] = make_float4(r[0][4], r[0][5], r[1][0], r[1][1]);
    si[3 * lane + 2] = make_float4(r[1][2], r[1][3], r[1][4], r[1][5]);
    if (live) reinterpret_cast<float2*>(Jz)[px] = make_float2(p00 * tx + p02 * tz, p11 * ty + p12 * tz);
    __syncthreads();
    // the wave's first pixel and how many of its 64 exist (<= 0: none)
    const int k0 = k - lane, nv4 = 3 * min(64, total - k0);
    float4* __restrict__ oj = reinterpret_cast<float4*>(Jj) + 3 * ((size_t)e * total + k0);
    float4* __restrict__ oi = reinterpret_cast<float4*>(Ji) + 3 * ((size_t)e * total + k0);
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const int v = q * 64 + lane;
      if (v < nv4) { oj[v] = sj[v]; oi[v] = si[v]; }
    }
  }
}

}  // namespace

}  // namespace wgsr

using namespace wgsr;

extern "C" {

int wgsr_lie_se3(int op, const float* a, int64_t inner_a, const float* b, int64_t inner_b, float* out, int64_t n,
                 void* stream) {
  if (op < WGSR_LIE_EXP || op > WGSR_LIE_RETR) return set_error(WGSR_EINVAL, "wgsr_lie_se3: unknown op %d", op);
  const bool two = lie_dim_b(op) != 0;
  if (n < 0 || inner_a < 1 || (two && inner_b < 1) || n >= (int64_t(1) << 31) * 256)
    return set_error(WGSR_EINVAL, "wgsr_lie_se3: bad size n=%lld inner_a=%lld inner_b=%lld", (long long)n,
                     (long long)inner_a, (long long)inner_b);
  if (n == 0) return WGSR_OK;
  if (!a || !out || (two && !b)) return set_error(WGSR_EINVAL, "wgsr_lie_se3: null pointer");
  hipStream_t s = (hipStream_t)stream;
  hipError_t e = hipSuccess;
  switch (op) {
    case WGSR_LIE_EXP: e = launch_lie<kExp>(a, inner_a, b, inner_b, out, n, s); break;
    case WGSR_LIE_LOG: e = launch_lie<kLog>(a, inner_a, b, inner_b, out, n, s); break;
    case WGSR_LIE_INV: e = launch_lie<kInv>(a, inner_a, b, inner_b, out, n, s); break;
    case WGSR_LIE_MUL: e = launch_lie<kMul>(a, inner_a, b, inner_b, out, n, s); break;
    case WGSR_LIE_ACT3: e = launch_lie<kAct3>(a, inner_a, b, inner_b, out, n, s); break;
    case WGSR_LIE_ACT4: e = launch_lie<kAct4>(a, inner_a, b, inner_b, out, n, s); break;
    case WGSR_LIE_MATRIX: e = launch_lie<kMatrix>(a, inner_a, b, inner_b, out, n, s); break;
    case WGSR_LIE_ADJ: e = launch_lie<kAdj>(a, inner_a, b, inner_b, out, n, s); break;
    case WGSR_LIE_ADJT: e = launch_lie<kAdjT>(a, inner_a, b, inner_b, out, n, s); break;
    default: e = launch_lie<kRetr>(a, inner_a, b, inner_b, out, n, s); break;
  }
  return e == hipSuccess ? WGSR_OK : set_error(WGSR_EHIP, "wgsr_lie_se3: %s", hipGetErrorString(e));
}

int wgsr_droid_reproject(const float* poses, const float* disps, const float* intrinsics, int per_frame_intrinsics,
                         int num, int ht, int wd, const int64_t* ii, const int64_t* jj, int n, int flags,
                         float* coords, float* valid, float* Ji, float* Jj, float* Jz, void* stream) {
  const int64_t total = (int64_t)ht * wd, groups = (total + 255) / 256;
  if (n < 0 || num <= 0 || ht <= 0 || wd <= 0 || total >= (int64_t(1) << 30) || n * groups >= (int64_t(1) << 31))
    return set_error(WGSR_EINVAL, "wgsr_droid_reproject: bad shape num=%d ht=%d wd=%d n=%d", num, ht, wd, n);
  if (flags & ~(WGSR_REPROJECT_JACOBIAN | WGSR_REPROJECT_DEPTH))
    return set_error(WGSR_EINVAL, "wgsr_droid_reproject: unknown flags %d", flags);
  const bool jac = flags & WGSR_REPROJECT_JACOBIAN, depth = flags & WGSR_REPROJECT_DEPTH;
  if (n == 0) return WGSR_OK;
  if (!poses || !disps || !intrinsics || !ii || !jj || !coords || !valid)
    return set_error(WGSR_EINVAL, "wgsr_droid_reproject: null pointer");
  if (jac ? (!Ji || !Jj || !Jz) : (Ji || Jj || Jz))
    return set_error(WGSR_EINVAL, "wgsr_droid_reproject: Ji, Jj, Jz must be given with the Jacobian flag and null "
                                  "without it");
  auto misaligned = [](const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; };
  if ((!depth && misaligned(coords, 8)) || (jac && (misaligned(Ji, 16) || misaligned(Jj, 16) || misaligned(Jz, 8))))
    return set_error(WGSR_EINVAL, "wgsr_droid_reproject: coords and Jz must be 8-byte, Ji and Jj 16-byte aligned");
  const dim3 grid((unsigned)(n * groups));
  const int st = per_frame_intrinsics ? 4 : 0;
  hipStream_t s = (hipStream_t)stream;
#define WGSR_REPROJECT_LAUNCH(J, D)                                                                              \
  hipLaunchKernelGGL((k_reproject<J, D>), grid, dim3(256), 0, s, poses, disps, intrinsics, st, num, ht, wd, ii, jj, \
                     (int)groups, coords, valid, Ji, Jj, Jz)
  if (jac && depth) WGSR_REPROJECT_LAUNCH(true, true);
  else if (jac) WGSR_REPROJECT_LAUNCH(true, false);
  else if (depth) WGSR_REPROJECT_LAUNCH(false, true);
  else WGSR_REPROJECT_LAUNCH(false, false);
#undef WGSR_REPROJECT_LAUNCH
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? WGSR_OK : set_error(WGSR_EHIP, "wgsr_droid_reproject: %s", hipGetErrorString(e));
}

}  // extern "C"
