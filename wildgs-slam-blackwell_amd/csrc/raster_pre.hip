// Rasteriser forward, first stage: preprocess -- one
// lane per Gaussian: cull, cov3D -> EWA cov2D -> conic, radius + tile
// rectangle, SH -> RGB; writes a 48-byte splat record per Gaussian (the only
// thing the tile loops read).  Then, in stream order: the dual scan and the
// bin sort (sort.hip), the pair expansion between them (raster_lists.hip), the
// per-bin depth sort that emits the tile lists (raster_bin_sort.hip), the
// render (raster_render_fwd.hip).  Sorting by depth and stably by tile yields
// exactly upstream's (tile << 32 | depth) order, ties by Gaussian index, while
// the N-sized sort only moves bin ids.
// Also here: the capacity-mode count reduction (k_cap_counts) and
// wgsr_mark_visible's kernel (k_mark_visible).
#include <algorithm>

#include "raster_sh.h"
#include "wgsr_common.h"
#include "wgsr_internal.h"

namespace wgsr {

namespace {

// SH -> RGB (upstream computeColorFromSH forward), clamp flags in bits 0..2.
// Every product and sum is written here, under contract(off) (the local
// lambdas included): no multiply-add of the colour can be fused, whatever the
// inlining context, so every preprocess kernel rounds the colour alike.
__device__ __forceinline__ f3 sh_to_rgb(int deg, const float* sh, f3 dir, uint32_t& clamp_bits) {
#pragma clang fp contract(off)
  auto term = [](float c, const float* v) -> f3 { return {c * v[0], c * v[1], c * v[2]}; };
  auto plus = [](f3 a, f3 b) -> f3 { return {a.x + b.x, a.y + b.y, a.z + b.z}; };
  auto minus = [](f3 a, f3 b) -> f3 { return {a.x - b.x, a.y - b.y, a.z - b.z}; };
  f3 r = term(SH_C0, sh);
  if (deg > 0) {
    const float x = dir.x, y = dir.y, z = dir.z;
    r = minus(plus(minus(r, term(SH_C1 * y, sh + 3)), term(SH_C1 * z, sh + 6)), term(SH_C1 * x, sh + 9));
    if (deg > 1) {
      const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
      r = plus(r, term(SH_C2[0] * xy, sh + 12));
      r = plus(r, term(SH_C2[1] * yz, sh + 15));
      r = plus(r, term(SH_C2[2] * (2.f * zz - xx - yy), sh + 18));
      r = plus(r, term(SH_C2[3] * xz, sh + 21));
      r = plus(r, term(SH_C2[4] * (xx - yy), sh + 24));
      if (deg > 2) {
        r = plus(r, term(SH_C3[0] * y * (3.f * xx - yy), sh + 27));
        r = plus(r, term(SH_C3[1] * xy * z, sh + 30));
        r = plus(r, term(SH_C3[2] * y * (4.f * zz - xx - yy), sh + 33));
        r = plus(r, term(SH_C3[3] * z * (2.f * zz - 3.f * xx - 3.f * yy), sh + 36));
        r = plus(r, term(SH_C3[4] * x * (4.f * zz - xx - yy), sh + 39));
        r = plus(r, term(SH_C3[5] * z * (xx - yy), sh + 42));
        r = plus(r, term(SH_C3[6] * x * (xx - 3.f * yy), sh + 45));
      }
    }
  }
  r = plus(r, f3{0.5f, 0.5f, 0.5f});
  clamp_bits = (r.x < 0 ? 1u : 0u) | (r.y < 0 ? 2u : 0u) | (r.z < 0 ? 4u : 0u);
  return mk3(fmaxf(r.x, 0.f), fmaxf(r.y, 0.f), fmaxf(r.z, 0.f));
}

// One Gaussian of k_preprocess2; returns (rect area, exact list length, bins
// touched), 0 if culled.  The per-Gaussian words every Gaussian gets (radius,
// list length, tb, depth key) are returned in `w` (radius, cnt, tb, key) and
// stored once by the caller; the splat record, rect, row table and clamp bits
// only for visible Gaussians.
// finish: null -- the record is stored whole here, its colour read from
// `colors` (black without), no clamp bits.  Non-null -- the caller finishes
// the record: it gets the geometry half (A, B) in finish[0..1] and stores it
// with the colour and the clamp bits once it has evaluated them.
__device__ __forceinline__ uint3 preprocess_one(
    const float* __restrict__ colors, const float* __restrict__ cov_pre, float scale_mod, int W, int H, int gx,
    int gy, int prefiltered, float4* __restrict__ splat, ListRec* __restrict__ lrec,
    uint32_t* __restrict__ clamped, uint32_t* __restrict__ err_flag, int bshift, int i, const Cam& c, const f3 p,
    const f3 sc, const float4 q, const float o, uint4& w, uint2& rcw, float4* finish) {
#pragma clang fp contract(off)
  w = make_uint4(0u, 0u, 0u, 0xFFFFFFFFu);  // culled: radius 0, no list, key sorts last
  rcw = make_uint2(0u, 0u);

  const float4 hom = xform44(c.proj, p);
  const float pw = 1.0f / (hom.w + 0.0000001f);
  const f3 pproj = mk3(hom.x * pw, hom.y * pw, hom.z * pw);
  const f3 pv = xform43(c.view, p);
  if (pv.z <= kNearZ) {
    if (prefiltered) atomicOr(err_flag, 1u);
    return make_uint3(0u, 0u, 0u);
  }
  float cv[6];
  if (cov_pre) {
#pragma unroll
    for (int k = 0; k < 6; ++k) cv[k] = cov_pre[6 * (size_t)i + k];
  } else {
    cov3d_from(sc, scale_mod, q, cv);
  }
  float S[3][3];
  sym3(cv, S);
  float T[2][3];
  f3 tc;
  float xm, ym;
  ewa_T(c, pv, T, tc, xm, ym);
  float a, b, cc;
  cov2d(T, S, a, b, cc);
  const float det = a * cc - b * b;
  if (det == 0.0f) return make_uint3(0u, 0u, 0u);
  const float det_inv = 1.f / det;
  const float mid = 0.5f * (a + cc);
  const float l1 = mid + sqrtf(fmaxf(0.1f, mid * mid - det));
  const float l2 = mid - sqrtf(fmaxf(0.1f, mid * mid - det));
  const float my_radius = ceilf(3.f * sqrtf(fmaxf(l1, l2)));
  const float px = ndc2pix(pproj.x, W), py = ndc2pix(pproj.y, H);
  const int r = (int)my_radius;
  const int x0 = min(gx, max(0, (int)((px - r) / kTile)));
  const int y0 = min(gy, max(0, (int)((py - r) / kTile)));
  const int x1 = min(gx, max(0, (int)((px + r + kTile - 1) / kTile)));
  const int y1 = min(gy, max(0, (int)((py + r + kTile - 1) / kTile)));
  if ((x1 - x0) * (y1 - y0) == 0) return make_uint3(0u, 0u, 0u);

  f3 rgb{};  // (black unless colours are given)
  if (colors) rgb = mk3(colors[3 * i], colors[3 * i + 1], colors[3 * i + 2]);
  // Reach of the splat: o G >= 1/255  <=>  d^T conic d <= lim = 2 ln(255 o)
  // (G = exp(-d^T conic d / 2) <= 1, so lim < 0 means "reaches no pixel").
  // The render loops test each entry's ellipse against a wave's pixel
  // rectangle and skip entries that cannot reach it (pure culling).
  const float lim = (o >= kMinAlpha) ? 2.f * logf(255.f * o) : -1.f;
  // record: A = (mean x, mean y, conic xx, conic yy), B = (conic xy, opacity,
  // lim, 0), C = (r, g, b, depth) -- pairs laid out for packed math
  const float4 A = make_float4(px, py, kConicSq * (cc * det_inv), kConicSq * (a * det_inv));
  const float4 B = make_float4(kConicXY * (-b * det_inv), o, lim, 0.f);
  if (finish) {
    finish[0] = A;
    finish[1] = B;
  } else {
    splat[3 * (size_t)i + 0] = A;
    splat[3 * (size_t)i + 1] = B;
    splat[3 * (size_t)i + 2] = make_float4(rgb.x, rgb.y, rgb.z, pv.z);
  }
  rcw = make_uint2((uint32_t)x0 | ((uint32_t)y0 << 16), (uint32_t)x1 | ((uint32_t)y1 << 16));
  // exact tile list length (row_span); upstream's num_rendered counts the rect
  const Reach rr = reach_of(A, B);
  uint32_t cnt = 0;
  uint4 tab = make_uint4(0u, 0u, 0u, 0u);
  for (int ty = y0; ty < y1; ++ty) {
    int xa;
    const uint32_t len = (uint32_t)row_span(rr, ty, x0, x1, xa);
    const int k = ty - y0;
    if (k < 4) {
      tab.x |= len << (8 * k);
      tab.z |= (uint32_t)(xa - x0) << (8 * k);
    } else if (k < kRowTab) {
      tab.y |= len << (8 * (k - 4));
      tab.w |= (uint32_t)(xa - x0) << (8 * (k - 4));
    }
    cnt += len;
  }
  lrec[i].tab = tab;
  if (!finish) clamped[i] = 0u;
  // bins of the rect (exact lists are per tile; a bin list holds every
  // Gaussian whose rect meets the bin, and the render waves cull the rest)
  const uint32_t nb = cnt == 0 ? 0u
                               : (uint32_t)((((x1 - 1) >> bshift) - (x0 >> bshift) + 1) *
                                            (((y1 - 1) >> bshift) - (y0 >> bshift) + 1));
  // tb: both < 2^16 (bin_shift() requires <= 65535 tiles); the key: pv.z > 0.2 > 0,
  // so float bits sort like the floats
  w = make_uint4((uint32_t)r, cnt, cnt | (nb << 16), __float_as_uint(pv.z));
  return make_uint3((uint32_t)((x1 - x0) * (y1 - y0)), cnt, nb);
}

// A preprocess wave's pair counts (upstream's num_rendered, exact pairs, bin
// pairs) and visible depth-key range into the counter block: one atomic per
// wave each, all five into the wave's own 64-byte record (CountSlot, one
// memory-side segment).  The wave sums / maxima are
// DPP row reductions + four readlanes (SGPR results, no LDS round trips);
// per-lane rect areas of 2^26 or more (images beyond ~17 Gpixel) take the
// 64-bit shuffle path.  (1M / 1080p / SH3: k_preprocess2 98.3-99.0 -> 78.5-79.6
// us against five arrays of 64 words, where 8 or 16 slots shared a segment.)
__device__ __forceinline__ void wave_pair_counts(const uint3 ac, uint32_t khi, uint32_t knlo,
                                                 CountSlot* __restrict__ slots) {
  CountSlot* __restrict__ rec = slots + blockIdx.x % kCountSlots;
  unsigned long long area, cnt, nbin;
  if (wave_any(ac.x >= (1u << 26))) {
    area = ac.x;
    cnt = ac.y;
    nbin = ac.z;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      area += __shfl_xor(area, off, 64);
      cnt += __shfl_xor(cnt, off, 64);
      nbin += __shfl_xor(nbin, off, 64);
    }
  } else {  // (list and bin counts never exceed the rect area)
    area = wave_total_u32(ac.x);
    cnt = wave_total_u32(ac.y);
    nbin = wave_total_u32(ac.z);
  }
  const uint32_t kh = wave_maximum_u32(khi), kn = wave_maximum_u32(knlo);
  if (threadIdx.x % 64 == 0) {
    atomicAdd(&rec->rect, area);
    atomicAdd(&rec->list, cnt);
    atomicAdd(&rec->bin, nbin);
    // the depth sort's key range (DepthKeyPlan): max key, max complement
    if (kh) atomicMax(&rec->key_hi, kh);
    if (kn) atomicMax(&rec->key_nlo, kn);
  }
}

constexpr int kPreWave = 64;

// ---- k_preprocess2: geometry first, then the visible rows' SH slab ----------
// One wave of 64 Gaussians per workgroup, in three steps:
//   1. the wave loads its parameters (one round trip for all four arrays) and
//      runs the projection / covariance / rectangle / row-table work; the
//      per-Gaussian words and the list record are stored, the splat record's
//      geometry half (A, B) stays in registers when SH colours follow;
//   2. the visible rows queue their evaluated SH coefficients as LDS-DMA
//      loads (global_load_lds: no VGPR holds them in flight) in a chunk-major
//      layout [chunk][lane] (chunk = 4 floats when rows are 16-byte aligned,
//      else 1), so that each lane then reads its own row conflict-free.
//      Culled rows read no SH (17 % of the bench scene's rows; 1M / 1080p /
//      SH3: 103.6 -> 102.3 us against a slab queued with the parameters for
//      every row);
//   3. after the slab wait the visible rows evaluate their colour and store
//      the whole 48-byte record in three back-to-back stores.  (With A, B
//      stored before the wait and the colour after it, many of the record's
//      lines had left the L2 in between and went to HBM twice: WRITE_SIZE at
//      1M 129.3 -> 98.0 MB per dispatch, 200k 29.9 -> 27.8 us.)
// With colours given (or no SH) step 1 stores the whole record and 2, 3 drop out.
// Other measured alternatives, all bit-identical and slower: SH coefficients
// in VGPRs (150 vs 103 us), a coalesced row-major slab (107.2-112 vs
// 101.1-102.5, also with XOR-swizzled LDS rows; a 16-row-group slab
// 103.7-108.0 vs 101.1-102.0), one memory round trip per wave (106.7 vs
// 103.4), records staged through LDS for contiguous stores (115.8 vs 106.7).
template <int kD, int kCh>
__device__ __forceinline__ f3 sh_rgb_lds(const float* __restrict__ s_sh, int lane, f3 dir, uint32_t& cbits) {
  constexpr int K = (kD + 1) * (kD + 1), NF = 3 * K, NCH = (NF + kCh - 1) / kCh;
  float sh[NCH * kCh];
#pragma unroll
  for (int k = 0; k < NCH; ++k) {
    if constexpr (kCh >= 4) {
      const float4 v = reinterpret_cast<const float4*>(s_sh)[k * 64 + lane];
      sh[4 * k] = v.x;
      sh[4 * k + 1] = v.y;
      sh[4 * k + 2] = v.z;
      sh[4 * k + 3] = v.w;
    } else {
      sh[k] = s_sh[k * 64 + lane];
    }
  }
  return sh_to_rgb(kD, sh, dir, cbits);
}

// kCh: floats per slab chunk (4 or 1); kD: the evaluated SH degree (-1: no
// slab -- colours given, or no SH), a template parameter so that the slab is a
// compile-time number of loads.  (D is not read -- kD stands for it -- but
// stays in the parameter list, which is the kernel's launch interface.)
template <int kCh, int kD>
__global__ __launch_bounds__(kPreWave) void k_preprocess2(
    int P, int D, int M, const float* __restrict__ means, const float* __restrict__ scales,
    const float* __restrict__ rots, const float* __restrict__ opac, const float* __restrict__ shs,
    const float* __restrict__ colors, const float* __restrict__ cov_pre, float scale_mod,
    const float* __restrict__ viewm, const float* __restrict__ projm, const float* __restrict__ campos_p, int W,
    int H, float tanx, float tany, int gx, int gy, int prefiltered, float4* __restrict__ splat,
    ListRec* __restrict__ lrec, uint32_t* __restrict__ clamped,
    uint32_t* __restrict__ dkey, int32_t* __restrict__ radii, int32_t* __restrict__ n_touched,
    uint32_t* __restrict__ err_flag, CountSlot* __restrict__ slots, int bshift,
    uint32_t* __restrict__ tb, uint8_t* __restrict__ gflag, const ZeroJob zero, uint32_t* __restrict__ meta) {
  extern __shared__ float s_sh[];  // nch x 64 x kCh floats (chunk-major)
  const int lane = threadIdx.x;
  const int i0 = blockIdx.x * kPreWave, i = i0 + lane;
  constexpr bool sh_on = kD >= 0;
  // the parameters first, in one basic block (clamped rows; with cov_pre the
  // scale / rotation loads read its first words and are discarded)
  const int ic = min(i, P - 1);
  const int ir = cov_pre ? 0 : ic;
  const float* __restrict__ sp = cov_pre ? cov_pre : scales;
  const float* __restrict__ rp = cov_pre ? cov_pre : rots;
  const f3 pl = mk3(means[3 * ic], means[3 * ic + 1], means[3 * ic + 2]);
  const f3 sl = mk3(sp[3 * ir], sp[3 * ir + 1], sp[3 * ir + 2]);
  const float4 ql = make_float4(rp[4 * ir], rp[4 * ir + 1], rp[4 * ir + 2], rp[4 * ir + 3]);
  const float ol = opac[ic];
  // an opaque use of every parameter: the four loads share one round trip
  // (none sinks into the branch below)
  asm volatile("" ::"v"(pl.x), "v"(pl.y), "v"(pl.z), "v"(sl.x), "v"(sl.y), "v"(sl.z), "v"(ql.x), "v"(ql.y),
               "v"(ql.z), "v"(ql.w), "v"(ol));
  auto load_slab = [&]() {  // (step 2; called by the visible rows)
    using lds_t = __attribute__((address_space(3))) void*;
    constexpr int kNch = (3 * ((kD < 0 ? 0 : kD) + 1) * ((kD < 0 ? 0 : kD) + 1) + kCh - 1) / kCh;
    const float* src = shs + (size_t)ic * (3 * M);
#pragma unroll
    for (int k = 0; k < kNch; ++k) {
      if constexpr (kCh == 4)
        __builtin_amdgcn_global_load_lds((const void*)(src + 4 * k), (lds_t)(s_sh + 256 * k), 16, 0, 0);
      else
        __builtin_amdgcn_global_load_lds((const void*)(src + k), (lds_t)(s_sh + 64 * k), 4, 0, 0);
    }
  };
  const f3 p = i < P ? pl : mk3(0.f, 0.f, 1.f);
  const float o = i < P ? ol : 0.f;
  const f3 sc = cov_pre ? mk3(1.f, 1.f, 1.f) : sl;
  const float4 q = cov_pre ? make_float4(1.f, 0.f, 0.f, 0.f) : ql;
  Cam c;
  load_cam(c, viewm, projm, W, H, tanx, tany);
  uint3 ac = make_uint3(0u, 0u, 0u);
  uint32_t khi = 0u, knlo = 0u;
  uint4 w = make_uint4(0u, 0u, 0u, 0xFFFFFFFFu);
  float4 ab[2];  // SH colours: the record's geometry half, stored with the colour below
  if (i < P) {
    uint2 rcw;
    ac = preprocess_one(colors, cov_pre, scale_mod, W, H, gx, gy, prefiltered, splat, lrec, clamped, err_flag, bshift,
                        i, c, p, sc, q, o, w, rcw, sh_on ? ab : nullptr);
    radii[i] = (int32_t)w.x;
    lrec[i].w = make_uint4(rcw.x, rcw.y, w.z, w.y);
    if (bshift) tb[i] = w.z;
    dkey[i] = w.w;
    if (w.w != 0xFFFFFFFFu) {
      khi = w.w;
      knlo = ~w.w;
    }
    n_touched[i] = 0;
    gflag[i] = 0;
  }
  if constexpr (sh_on) {
    if (i < P && w.x != 0u) load_slab();  // (visible rows only: culled rows read no SH)
    __builtin_amdgcn_s_waitcnt(0);  // the slab has landed (one wave per workgroup)
    __syncthreads();
    if (i < P && w.x != 0u) {  // visible: the colour record
#pragma clang fp contract(off)
      f3 dir = sub3(p, mk3(campos_p[0], campos_p[1], campos_p[2]));
      const float len = sqrtf(dot3(dir, dir));
      dir = mk3(dir.x / len, dir.y / len, dir.z / len);
      uint32_t cbits = 0;
      const f3 rgb = sh_rgb_lds<(kD < 0 ? 0 : kD), kCh>(s_sh, lane, dir, cbits);
      splat[3 * (size_t)i + 0] = ab[0];
      splat[3 * (size_t)i + 1] = ab[1];
      splat[3 * (size_t)i + 2] = make_float4(rgb.x, rgb.y, rgb.z, __uint_as_float(w.w));
      clamped[i] = cbits;
    }
  }
  wave_pair_counts(ac, khi, knlo, slots);
  zero_share(zero, blockIdx.x, gridDim.x, lane, kPreWave);
  if (blockIdx.x == 0 && lane == 0) {
    meta[1] = 0u;  // no capacity overflow (ImageLayout::meta)
    meta[2] = 0u;  // slots not (yet) known to follow the index order (k_duplicate_bins)
  }
}

__global__ __launch_bounds__(256) void k_mark_visible(int P, const float* __restrict__ means,
                                                      const float* __restrict__ viewm, uint8_t* __restrict__ present) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= P) return;
  const f3 p = mk3(means[3 * i], means[3 * i + 1], means[3 * i + 2]);
  const f3 pv = xform43(viewm, p);
  present[i] = pv.z > kNearZ ? 1 : 0;
}

}  // namespace

// Capacity-mode forward: the counter block's partial pair counts (upstream's
// rect pairs, exact pairs, bin pairs of the kCountSlots records) -> counts[0..2]
// (saturating u32), the bin-pair count clamped to the buffers (counts[4], what
// the sort reads as its key count) and the overflow flag (counts[3] and the
// image buffer's meta[1], which makes the render backward a no-op).

__global__ __launch_bounds__(64) void k_cap_counts(const CountSlot* __restrict__ slots,
                                                   uint64_t cap_rect, uint64_t cap_bin, uint32_t* __restrict__ counts,
                                                   uint32_t* __restrict__ meta) {
  const int t = threadIdx.x;
  const CountTotals tot = count_slots_reduce(slots, t);
  const unsigned long long r = tot.rect, e = tot.list, b = tot.bin;
  if (t == 0) {
    const uint32_t ovf = (r > cap_rect || b > cap_bin) ? 1u : 0u;
    counts[0] = (uint32_t)min(r, 0xFFFFFFFFull);
    counts[1] = (uint32_t)min(e, 0xFFFFFFFFull);
    counts[2] = (uint32_t)min(b, 0xFFFFFFFFull);
    counts[3] = ovf;
    counts[4] = (uint32_t)min(b, (unsigned long long)cap_bin);
    meta[1] = ovf;
  }
}

hipError_t launch_cap_counts(const CountSlot* slots, uint64_t cap_rect, uint64_t cap_bin, uint32_t* counts,
                             uint32_t* meta, hipStream_t s) {
  hipLaunchKernelGGL(k_cap_counts, dim3(1), dim3(64), 0, s, slots, cap_rect, cap_bin, counts, meta);
  return hipGetLastError();
}

hipError_t launch_preprocess(const wgsr_raster_args& a, void* geom, int32_t* radii, int32_t* n_touched,
                             uint32_t* err_flag, CountSlot* slots, int bshift, const ZeroJob& zero,
                             hipStream_t s, uint32_t* meta) {
  if (a.P == 0) return hipSuccess;
  const GeomLayout L(a.P);
  const int gx = (a.W + kTile - 1) / kTile, gy = (a.H + kTile - 1) / kTile;
  const bool sh_on = a.shs && !a.colors;
  const bool ch4 = sh_on && (a.M * 3) % 4 == 0 && (reinterpret_cast<uintptr_t>(a.shs) & 15) == 0;
  const int nf = 3 * (a.D + 1) * (a.D + 1);
  const int kch = ch4 ? 4 : 1;
  const size_t lds2 = sh_on ? sizeof(float) * 64 * (size_t)(((nf + kch - 1) / kch) * kch) : 0;
  using PreKernel = decltype(&k_preprocess2<1, -1>);
  static constexpr PreKernel kPre[2][4] = {{k_preprocess2<1, 0>, k_preprocess2<1, 1>, k_preprocess2<1, 2>,
                                            k_preprocess2<1, 3>},
                                           {k_preprocess2<4, 0>, k_preprocess2<4, 1>, k_preprocess2<4, 2>,
                                            k_preprocess2<4, 3>}};
  const PreKernel kern = sh_on ? kPre[ch4 ? 1 : 0][std::min(std::max(a.D, 0), 3)] : k_preprocess2<1, -1>;
  hipLaunchKernelGGL(kern, dim3((a.P + kPreWave - 1) / kPreWave), dim3(kPreWave),
                     lds2, s, a.P, a.D, a.M, a.means3D, a.scales, a.rotations, a.opacities, a.shs, a.colors,
                     a.cov3D_precomp, a.scale_modifier, a.viewmatrix, a.projmatrix, a.campos, a.W, a.H, a.tan_fovx,
                     a.tan_fovy, gx, gy, a.prefiltered, at<float4>(geom, L.splat), at<ListRec>(geom, L.lrec),
                     at<uint32_t>(geom, L.clamped), at<uint32_t>(geom, L.dkey), radii, n_touched, err_flag, slots,
                     bshift, at<uint32_t>(geom, L.tb), at<uint8_t>(geom, L.gflag), zero, meta);
  return hipGetLastError();
}

hipError_t launch_mark_visible(int P, const float* means3D, const float* view, uint8_t* present, hipStream_t s) {
  if (P == 0) return hipSuccess;
  hipLaunchKernelGGL(k_mark_visible, dim3((P + 255) / 256), dim3(256), 0, s, P, means3D, view, present);
  return hipGetLastError();
}

}  // namespace wgsr
