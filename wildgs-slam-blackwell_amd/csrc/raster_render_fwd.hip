// Render forward: one 16x16 tile per workgroup of four
// waves, wave w blending the 8x8 quadrant w front to back, one pixel per lane.
// k_render_fwd_dec (the default) lets every wave fetch and stop on its own;
// k_render_fwd1 (WGSR_FWD_DEC=0) streams the records through shared LDS with
// one barrier per batch.  Bit-identical outputs.
#include <stdlib.h>

#include <type_traits>

#include "wgsr_common.h"
#include "wgsr_internal.h"

namespace wgsr {

namespace {

// Splat records arrive 64 at a time through LDS; wave 0 loads the next
// batch's records into registers while the current batch is blended (ids two
// ahead).
constexpr int kFwdBatch = 64;

// Entry-pair blend: the batch's entries that (one 8x8-quadrant wave's)
// survive the wave's culling are first compacted into the wave's own LDS area
// with two consecutive survivors interleaved per field (sQ: {x1, x2, y1, y2},
// {A.z1, A.z2, A.w1, A.w2}, {B.x1, B.x2, o1, o2}), so that one ds_read_b128
// hands two entries' operands to packed-FP32 math: the power, exp2 argument
// and opacity product of BOTH entries cost one v_pk_* instruction each (the
// forward's own operation sequence per lane, so alpha is bitwise that of
// the backward's recomputation).  Only the
// transmittance recurrence, the compares and the colour accumulation stay
// per entry.  n_touched increments are staged per compact slot.
// wave 0 streams the next batch's records into a second LDS buffer with
// global_load_lds instead of holding them in registers (every wave of the
// kernel would allocate those VGPRs)
struct FwdPairRec {   // two consecutive survivors (one LDS address per pair)
  float4 q[3];       // {x, x', y, y'}, {A.z, A.z', A.w, A.w'}, {B.x, B.x', o, o'}
  float4 c[2];       // colour (c0, c1, c2, depth) of each
  uint32_t n[2];     // contributor numbers
  uint32_t pad[2];
};
struct FwdPairLds {
  FwdPairRec p[kFwdBatch / 2];
  uint32_t touch[kFwdBatch];  // n_touched increment per compact slot
};

template <bool kTouch>
__device__ __forceinline__ void fwd_blend_one(float a, float pw, const float4& C, uint32_t cn, uint32_t* touch_slot,
                                              float& T, v2f& c01, v2f& c2d, uint32_t& last, uint64_t& dm,
                                              uint64_t valid) {
  const float test_T = fmaf(-T, a, T);  // T (1 - alpha)
  const uint64_t live = wave_ballot(pw <= 0.0f) & wave_ballot(a >= kMinAlpha) & ~dm & valid;
  const uint64_t low = wave_ballot(test_T < kMinT);
  const uint64_t blend = live & ~low;
  const bool bl = __builtin_amdgcn_inverse_ballot_w64(blend);
  const float wgt = bl ? a * T : 0.f;
  c01 += wgt * v2f{C.x, C.y};
  c2d += wgt * v2f{C.z, C.w};
  uint32_t tot = 0;
  if (kTouch) tot = (uint32_t)__popcll(blend & wave_ballot(test_T > 0.5f));
  T = bl ? test_T : T;
  last = bl ? cn : last;
  dm |= live & low;
  if (kTouch) *touch_slot = tot;
}

template <bool kTouch>
__device__ __forceinline__ void fwd_blend_pairs(int n, const FwdPairLds& L, uint32_t* touch, v2f pxy, float& T,
                                                v2f& c01, v2f& c2d, uint32_t& last, uint64_t& dm) {
  for (int i = 0; i < n && dm != ~0ull; i += 2) {
    const FwdPairRec& R = L.p[i >> 1];
    const float4 q0 = R.q[0], q1 = R.q[1], q2 = R.q[2];
    const float4 C1 = R.c[0], C2 = R.c[1];
    const uint2 cn = *reinterpret_cast<const uint2*>(&R.n[0]);
    const v2f DX = v2f{q0.x, q0.y} - v2f{pxy.x, pxy.x}, DY = v2f{q0.z, q0.w} - v2f{pxy.y, pxy.y};
    // splat_power per lane: fma(dx, fma(B.x, dy, A.z dx), (A.w dy) dy)
    const v2f tz = v2f{q1.x, q1.y} * DX, tw = v2f{q1.z, q1.w} * DY;
    const v2f PW = pfma(DX, pfma(v2f{q2.x, q2.y}, DY, tz), tw * DY);
    const v2f ag = v2f{q2.z, q2.w} * v2f{__builtin_amdgcn_exp2f(PW.x), __builtin_amdgcn_exp2f(PW.y)};
    const float a1 = fminf(kMaxAlpha, ag.x), a2 = fminf(kMaxAlpha, ag.y);
    fwd_blend_one<kTouch>(a1, PW.x, C1, cn.x, touch + i, T, c01, c2d, last, dm, ~0ull);
    // (an odd survivor count leaves the last pair's second half unused)
    fwd_blend_one<kTouch>(a2, PW.y, C2, cn.y, touch + i + 1, T, c01, c2d, last, dm, i + 1 < n ? ~0ull : 0ull);
  }
}

// cull the staged batch against the wave's pixel box, compact the survivors
// into L, blend them front to back in pairs, flush n_touched
// after(): called once the survivors are compacted (the LDS-DMA of the next
// batch is queued there, behind every LDS write of this batch)
template <class F>
__device__ __forceinline__ void fwd_blend_batch_pairs(int cnt, uint32_t cbase, const float4* sA, const float4* sB,
                                                      const float4* sC, const uint32_t* sG, FwdPairLds& L, int wx0,
                                                      int wx1, int wy0, int wy1, v2f pxy, int lane,
                                                      int32_t* __restrict__ n_touched, float& T, v2f& c01, v2f& c2d,
                                                      uint32_t& last, uint64_t& dm, uint32_t* fl_gid,
                                                      uint32_t* fl_tv, const float4* pre, uint32_t pre_gid, F after) {
  // (pre: this lane's records, read by the caller before it queued an LDS DMA)
  const float4 A = pre ? pre[0] : sA[lane], B = pre ? pre[1] : sB[lane];
  const bool mine = lane < cnt && ellipse_hits(A, B, wx0, wx1, wy0, wy1);
  const uint64_t todo = wave_ballot(mine);
  const int n = __popcll(todo);
  const uint32_t k = lanes_below(todo);
  // (uniform) a batch whose wave has no pixel left with T > 0.5 runs the entry
  // loop without the n_touched bookkeeping: T only falls, so none of its
  // entries can touch a pixel (one compare, two moves, one LDS store fewer)
  const bool touch = (wave_ballot(T > 0.5f) & ~dm) != 0;
  if (mine) {
    FwdPairRec& R = L.p[k >> 1];
    float* q = &R.q[0].x + (k & 1);
    q[0] = A.x; q[2] = A.y; q[4] = A.z; q[6] = A.w; q[8] = B.x; q[10] = B.y;
    R.c[k & 1] = pre ? pre[2] : sC[lane];
    R.n[k & 1] = cbase + (uint32_t)lane;
  }
  if (touch) L.touch[lane] = 0;
  if (lane == 63 && (n & 1)) {  // the unused half of an odd last pair: finite operands
    FwdPairRec& R = L.p[n >> 1];
    float* q = &R.q[0].x + 1;
    q[0] = 0.f; q[2] = 0.f; q[4] = 0.f; q[6] = 0.f; q[8] = 0.f; q[10] = 0.f;
    R.c[1] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  // (a wave's own LDS accesses complete in order; the wave barrier -- no
  // instruction -- keeps the compiler from moving the cross-lane reads below
  // above these writes)
  __builtin_amdgcn_wave_barrier();
  after();
  if (touch) {
    fwd_blend_pairs<true>(n, L, L.touch, pxy, T, c01, c2d, last, dm);
    const uint32_t tv = mine ? L.touch[k] : 0u;
    if (fl_tv) {  // the caller issues the atomic later
      *fl_gid = pre_gid;
      *fl_tv = tv;
    } else if (tv != 0) {
      atomicAdd(&n_touched[sG[lane]], (int)tv);
    }
  } else {
    fwd_blend_pairs<false>(n, L, L.touch, pxy, T, c01, c2d, last, dm);
  }
  __builtin_amdgcn_wave_barrier();  // (the next batch's compaction writes stay behind these reads)
}

// One 16x16 tile per workgroup of 4 waves; wave w owns the 8x8 quadrant w,
// one pixel per lane.  Every per-pixel predicate (done, live, low, blend) is
// an explicit SGPR lane mask combined by scalar ops: the per-entry update is
// ~22 VALU instructions (power 6, exp2, alpha 2, four compares, T update,
// weight, two packed accumulates, three selects).  Also writes each
// quadrant's deepest contributor (tile_m4), the backward's per-tile work.
__global__ __launch_bounds__(256) void k_render_fwd1(
    const uint2* __restrict__ ranges, const uint32_t* __restrict__ order, const uint32_t* __restrict__ point_g,
    const float4* __restrict__ splat, int W, int H, int gx, int ntiles, const float* __restrict__ bg,
    float* __restrict__ out_color, float* __restrict__ out_depth, float* __restrict__ out_opac,
    float* __restrict__ final_T, uint32_t* __restrict__ n_contrib, int32_t* __restrict__ n_touched,
    uint32_t* __restrict__ tile_m4) {
  // two batch buffers as separate objects, so that the compiler can tell the
  // LDS-DMA into one from the reads of the other (no vmcnt wait before them)
  __shared__ float4 sA_0[kFwdBatch], sB_0[kFwdBatch], sC_0[kFwdBatch];
  __shared__ float4 sA_1[kFwdBatch], sB_1[kFwdBatch], sC_1[kFwdBatch];
  __shared__ uint32_t sG_0[kFwdBatch], sG_1[kFwdBatch];
  __shared__ uint32_t sDone[2][4];  // per batch parity: wave w has no pixel left
  __shared__ FwdPairLds sPair[4];  // per wave: the batch's surviving entries, compacted
  const uint32_t slot = xcd_remap(blockIdx.x, (uint32_t)ntiles);
  const uint32_t tile = order ? order[slot] : slot;  // null: xcd_remap's order as it is
  const int t = threadIdx.x, w = t >> 6, lane = t & 63;
  const int tx0 = (int)(tile % gx) * kTile, ty0 = (int)(tile / gx) * kTile;
  int ox, oy;
  tile_pixel<1>(w, lane, 0, ox, oy);
  const int px = tx0 + ox, py = ty0 + oy;
  const v2f pxy{(float)px, (float)py};
  // per-pixel predicates live in SGPR lane masks (a ballot of a compound
  // predicate would be materialised through VGPRs): dm = finished pixels
  uint64_t dm = wave_ballot(!(px < W && py < H));
  const uint2 range = ranges[tile];
  int wx0, wx1, wy0, wy1;
  wave_box<1>(w, tx0, ty0, wx0, wx1, wy0, wy1);
  float T = 1.f;
  v2f c01{0.f, 0.f}, c2d{0.f, 0.f};  // (colour 0, colour 1), (colour 2, depth)
  uint32_t last = 0;

  // prefetch pipeline (wave 0): batch b+1's records stream straight into the
  // other LDS buffer (global_load_lds_dwordx4, no VGPRs held), ids of b+2 in
  // registers.  ONE barrier per batch, which waits for LDS only: wave 0's
  // vmcnt wait before it finds every load a batch old, and the n_touched
  // atomics of a batch are issued right after the next batch's barrier, so
  // no wave ever waits for an atomic.  Loads past the list re-read its last
  // entry (valid; culled by lane < cnt), so they need no branch.
  const uint32_t last_i = range.y > range.x ? range.y - 1 : range.x;
  auto fetch = [&](uint32_t g, float4* dA, float4* dB, float4* dC) {
    const float4* src = splat + 3 * (size_t)g;
    __builtin_amdgcn_global_load_lds((const void*)src, (__attribute__((address_space(3))) void*)dA, 16, 0, 0);
    __builtin_amdgcn_global_load_lds((const void*)(src + 1), (__attribute__((address_space(3))) void*)dB, 16, 0, 0);
    __builtin_amdgcn_global_load_lds((const void*)(src + 2), (__attribute__((address_space(3))) void*)dC, 16, 0, 0);
  };
  uint32_t gcur = 0, gnext = 0;
  if (w == 0 && range.x < range.y) {
    gcur = point_g[min(range.x + t, last_i)];
    fetch(gcur, sA_0, sB_0, sC_0);
    if (range.x + kFwdBatch < range.y) gnext = point_g[min(range.x + kFwdBatch + t, last_i)];
  }
  uint32_t fl_gid = 0, fl_tv = 0;  // this lane's n_touched increment of the previous batch
  // one batch: read buffer (cA..cG), DMA target (nA..nC) as restrict
  // parameters, so that the compiler's LDS-DMA wait tracking sees that the
  // reads cannot alias the DMA in flight
  auto body = [&](uint32_t b0, uint32_t* __restrict__ done, float4* __restrict__ cA, float4* __restrict__ cB,
                  float4* __restrict__ cC, uint32_t* __restrict__ cG, float4* __restrict__ nA_,
                  float4* __restrict__ nB_, float4* __restrict__ nC_) -> bool {
    if (w == 0) {
      cG[t] = gcur;
      __builtin_amdgcn_s_waitcnt(0);  // this batch's records have landed
    }
    if (lane == 0) done[w] = dm == ~0ull ? 1u : 0u;
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");  // (every wave is done with the other buffer)
    const uint4 dn = *reinterpret_cast<const uint4*>(done);
    // this lane's entry, read before the DMA is queued: the compiler would
    // otherwise wait for the DMA before reading the other buffer
    const float4 pre[3] = {cA[lane], cB[lane], cC[lane]};
    const uint32_t gme = cG[lane];
    // wave 0 queues the next batch's DMA after this batch's LDS writes (the
    // compiler orders LDS writes behind a DMA in flight), its id loads, then
    // the previous batch's n_touched atomics (a wait the compiler places for
    // the loads then never covers an atomic)
    bool queued = false;
    auto queue_next = [&]() {
      if (queued) return;
      queued = true;
      if (w == 0 && b0 + kFwdBatch < range.y) {
        gcur = gnext;
        fetch(gcur, nA_, nB_, nC_);
        if (b0 + 2 * kFwdBatch < range.y) gnext = point_g[min(b0 + 2 * kFwdBatch + t, last_i)];
      }
      if (fl_tv != 0) atomicAdd(&n_touched[fl_gid], (int)fl_tv);
      fl_tv = 0;
    };
    if (dn.x & dn.y & dn.z & dn.w) return false;
    if (dm != ~0ull) {
      const int cnt = (int)min((uint32_t)kFwdBatch, range.y - b0);
      fwd_blend_batch_pairs(cnt, b0 - range.x + 1, cA, cB, cC, cG, sPair[w], wx0, wx1, wy0, wy1, pxy, lane, n_touched,
                            T, c01, c2d, last, dm, &fl_gid, &fl_tv, pre, gme, queue_next);
    }
    queue_next();  // (a finished wave: keeps the barriers and the pipeline)
    return true;
  };
  auto step = [&](auto par, uint32_t b0) -> bool {
    if constexpr (decltype(par)::value == 0)
      return body(b0, sDone[0], sA_0, sB_0, sC_0, sG_0, sA_1, sB_1, sC_1);
    else
      return body(b0, sDone[1], sA_1, sB_1, sC_1, sG_1, sA_0, sB_0, sC_0);
  };
  for (uint32_t b0 = range.x; b0 < range.y; b0 += 2 * kFwdBatch) {
    if (!step(std::integral_constant<int, 0>{}, b0)) break;
    if (b0 + kFwdBatch >= range.y || !step(std::integral_constant<int, 1>{}, b0 + kFwdBatch)) break;
  }
  if (fl_tv != 0) atomicAdd(&n_touched[fl_gid], (int)fl_tv);
  {  // this quadrant's deepest contributor: tile_m4[4 tile + w] (no barrier)
    uint32_t mx = last;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, off, 64));
    if (lane == 0) tile_m4[4 * tile + w] = mx;
  }
  if (!(px < W && py < H)) return;
  const size_t HW = (size_t)H * W;
  const size_t pid = (size_t)py * W + px;
  final_T[pid] = T;
  n_contrib[pid] = last;
  out_color[pid] = c01.x + T * bg[0];
  out_color[HW + pid] = c01.y + T * bg[1];
  out_color[2 * HW + pid] = c2d.x + T * bg[2];
  out_depth[pid] = c2d.y;
  out_opac[pid] = 1.f - T;
}

// k_render_fwd1 with the quadrant waves decoupled (the default;
// WGSR_FWD_DEC=0 keeps k_render_fwd1): every wave prefetches its own batch
// records into registers one batch ahead (lane j entry j) instead of wave 0
// streaming them into shared LDS behind a barrier per batch, and stops as
// soon as its own 64 pixels are done -- no wave waits for its tile's
// slowest quadrant.  Same blend per pixel in the same order, n_touched as
// integer atomics: bit-identical outputs.
#ifndef WGSR_FWD_DEC
#define WGSR_FWD_DEC 1
#endif
// diagnostic build: per quadrant wave of k_render_fwd_dec -- [0] waves, [1]
// batches, [2] entries in them, [3] survivors of the culling, [4] pair
// iterations (survivor pairs), [5] batches with the n_touched bookkeeping,
// [6] waves that stopped with every pixel done (wgsr_debug_fwd_stats)
#ifndef WGSR_FWD_STATS
#define WGSR_FWD_STATS 0
#endif
#if WGSR_FWD_STATS
__device__ unsigned long long g_fwd_stats[8];
#endif
__global__ __launch_bounds__(256) void k_render_fwd_dec(
    const uint2* __restrict__ ranges, const uint32_t* __restrict__ order, const uint32_t* __restrict__ point_g,
    const float4* __restrict__ splat, int W, int H, int gx, int ntiles, const float* __restrict__ bg,
    float* __restrict__ out_color, float* __restrict__ out_depth, float* __restrict__ out_opac,
    float* __restrict__ final_T, uint32_t* __restrict__ n_contrib, int32_t* __restrict__ n_touched,
    uint32_t* __restrict__ tile_m4) {
  __shared__ FwdPairLds sPair[4];  // per wave: the batch's surviving entries, compacted
  const uint32_t slot = xcd_remap(blockIdx.x, (uint32_t)ntiles);
  const uint32_t tile = order ? order[slot] : slot;
  const int t = threadIdx.x, w = t >> 6, lane = t & 63;
  const int tx0 = (int)(tile % gx) * kTile, ty0 = (int)(tile / gx) * kTile;
  int ox, oy;
  tile_pixel<1>(w, lane, 0, ox, oy);
  const int px = tx0 + ox, py = ty0 + oy;
  const v2f pxy{(float)px, (float)py};
  uint64_t dm = wave_ballot(!(px < W && py < H));
  const uint2 range = ranges[tile];
  int wx0, wx1, wy0, wy1;
  wave_box<1>(w, tx0, ty0, wx0, wx1, wy0, wy1);
  float T = 1.f;
  v2f c01{0.f, 0.f}, c2d{0.f, 0.f};
  uint32_t last = 0;
  (void)t;
  const uint32_t last_i = range.y > range.x ? range.y - 1 : range.x;
  uint32_t gcur = 0, gnext = 0;
  float4 nA = make_float4(0, 0, 0, 0), nB = nA, nC = nA;
  if (range.x < range.y) {
    gcur = point_g[min(range.x + lane, last_i)];
    nA = splat[3 * (size_t)gcur];
    nB = splat[3 * (size_t)gcur + 1];
    nC = splat[3 * (size_t)gcur + 2];
    if (range.x + kFwdBatch < range.y) gnext = point_g[min(range.x + kFwdBatch + lane, last_i)];
  }
  uint32_t fl_gid = 0, fl_tv = 0;  // this lane's n_touched increment of the previous batch
#if WGSR_FWD_STATS
  uint32_t st_b = 0, st_e = 0, st_s = 0, st_p = 0, st_t = 0;
#endif
  for (uint32_t b0 = range.x; b0 < range.y && dm != ~0ull; b0 += kFwdBatch) {  // (wave-uniform)
    const float4 pre[3] = {nA, nB, nC};
    const uint32_t gme = gcur;
    if (b0 + kFwdBatch < range.y) {  // the next batch's records, the one after's ids
      gcur = gnext;
      nA = splat[3 * (size_t)gcur];
      nB = splat[3 * (size_t)gcur + 1];
      nC = splat[3 * (size_t)gcur + 2];
      if (b0 + 2 * kFwdBatch < range.y) gnext = point_g[min(b0 + 2 * kFwdBatch + lane, last_i)];
    }
    const int cnt = (int)min((uint32_t)kFwdBatch, range.y - b0);
    // cull against the wave's pixel box, compact the survivors in pairs, blend
    // (fwd_blend_batch_pairs on register-held records)
    FwdPairLds& L = sPair[w];
    const bool mine = lane < cnt && ellipse_hits(pre[0], pre[1], wx0, wx1, wy0, wy1);
    const uint64_t todo = wave_ballot(mine);
    const int n = __popcll(todo);
    const uint32_t k = lanes_below(todo);
    const bool touch = (wave_ballot(T > 0.5f) & ~dm) != 0;  // (uniform)
    if (mine) {
      FwdPairRec& R = L.p[k >> 1];
      float* q = &R.q[0].x + (k & 1);
      q[0] = pre[0].x; q[2] = pre[0].y; q[4] = pre[0].z; q[6] = pre[0].w; q[8] = pre[1].x; q[10] = pre[1].y;
      R.c[k & 1] = pre[2];
      R.n[k & 1] = b0 - range.x + 1 + (uint32_t)lane;
    }
    if (touch) L.touch[lane] = 0;
    if (lane == 63 && (n & 1)) {  // the unused half of an odd last pair: finite operands
      FwdPairRec& R = L.p[n >> 1];
      float* q = &R.q[0].x + 1;
      q[0] = 0.f; q[2] = 0.f; q[4] = 0.f; q[6] = 0.f; q[8] = 0.f; q[10] = 0.f;
      R.c[1] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
#if WGSR_FWD_STATS
    ++st_b;
    st_e += (uint32_t)cnt;
    st_s += (uint32_t)n;
    st_p += (uint32_t)((n + 1) / 2);
    st_t += touch ? 1u : 0u;
#endif
    // cross-lane LDS traffic of one wave: ordered by the hardware, and kept in
    // program order by the (instruction-free) wave barriers here and below
    __builtin_amdgcn_wave_barrier();
    if (fl_tv != 0) atomicAdd(&n_touched[fl_gid], (int)fl_tv);  // the previous batch's
    fl_tv = 0;
    if (touch) {
      fwd_blend_pairs<true>(n, L, L.touch, pxy, T, c01, c2d, last, dm);
      fl_gid = gme;
      fl_tv = mine ? L.touch[k] : 0u;
    } else {
      fwd_blend_pairs<false>(n, L, L.touch, pxy, T, c01, c2d, last, dm);
    }
    __builtin_amdgcn_wave_barrier();
  }
  if (fl_tv != 0) atomicAdd(&n_touched[fl_gid], (int)fl_tv);
#if WGSR_FWD_STATS
  if (lane == 0) {
    atomicAdd(&g_fwd_stats[0], 1ull);
    atomicAdd(&g_fwd_stats[1], (unsigned long long)st_b);
    atomicAdd(&g_fwd_stats[2], (unsigned long long)st_e);
    atomicAdd(&g_fwd_stats[3], (unsigned long long)st_s);
    atomicAdd(&g_fwd_stats[4], (unsigned long long)st_p);
    atomicAdd(&g_fwd_stats[5], (unsigned long long)st_t);
    atomicAdd(&g_fwd_stats[6], dm == ~0ull ? 1ull : 0ull);
  }
#endif
  {  // this quadrant's deepest contributor: tile_m4[4 tile + w]
    uint32_t mx = last;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, off, 64));
    if (lane == 0) tile_m4[4 * tile + w] = mx;
  }
  if (!(px < W && py < H)) return;
  const size_t HW = (size_t)H * W;
  const size_t pid = (size_t)py * W + px;
  final_T[pid] = T;
  n_contrib[pid] = last;
  out_color[pid] = c01.x + T * bg[0];
  out_color[HW + pid] = c01.y + T * bg[1];
  out_color[2 * HW + pid] = c2d.x + T * bg[2];
  out_depth[pid] = c2d.y;
  out_opac[pid] = 1.f - T;
}

}  // namespace

hipError_t launch_render_fwd(const wgsr_raster_args& a, const uint2* ranges, const uint32_t* point_g, const void* geom, float* out_color, float* out_depth,
                             float* out_opacity, float* final_T, uint32_t* n_contrib, int32_t* n_touched,
                             uint32_t* tile_m, hipStream_t s) {
  const GeomLayout L(a.P);
  const int gx = (a.W + kTile - 1) / kTile, gy = (a.H + kTile - 1) / kTile;
  const int nt = gx * gy;
  const char* dec = getenv("WGSR_FWD_DEC");  // (read per launch: tests compare the two)
  auto kern = (dec ? atoi(dec) != 0 : WGSR_FWD_DEC != 0) ? k_render_fwd_dec : k_render_fwd1;
  hipLaunchKernelGGL(kern, dim3(nt), dim3(256), 0, s, ranges, nullptr, point_g,
                     at<float4>(geom, L.splat), a.W, a.H, gx, nt, a.bg, out_color, out_depth, out_opacity, final_T,
                     n_contrib, n_touched, tile_m);
  return hipGetLastError();
}

}  // namespace wgsr

#if WGSR_FWD_STATS
// diagnostic build only: read and clear the forward's per-wave census
extern "C" int wgsr_debug_fwd_stats(unsigned long long* out) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(wgsr::g_fwd_stats), sizeof(unsigned long long) * 8) != hipSuccess)
    return 1;
  unsigned long long z[8] = {};
  return hipMemcpyToSymbol(HIP_SYMBOL(wgsr::g_fwd_stats), z, sizeof(z)) != hipSuccess;
}
#endif
