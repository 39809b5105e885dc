// Rasteriser tile lists: what lies between the
// preprocess records and the render kernels, the sorts aside (sort.hip,
// raster_bin_sort.hip).  k_duplicate_bins / k_duplicate expand the Gaussians
// into pairs, k_bin_bounds finds each bin in the sorted pairs, k_expand_bins
// (global depth-sort schedule) and k_ranges cut per-tile lists and ranges,
// k_tile_order writes the render backward's launch order during the forward.
// Also here: k_check_tile_lists (wgsr_check_tile_lists) and k_zero_u32.
#include <algorithm>

#include "wgsr_common.h"
#include "wgsr_internal.h"

namespace wgsr {

namespace {

// Expand the exact tile lists (row_span) of depth ranks [r0, r0 + 64) (one
// wave) into pairs: lane <-> pair, so the writes are contiguous.
__global__ __launch_bounds__(256) void k_duplicate(uint32_t P, int gx, const uint32_t* __restrict__ offs,
                                                   const uint32_t* __restrict__ sorted_g,
                                                   const ListRec* __restrict__ lrec,
                                                   const float4* __restrict__ splat, uint32_t* __restrict__ keys,
                                                   uint32_t* __restrict__ slot_g, uint8_t* __restrict__ pflag) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t r0 = (blockIdx.x * blockDim.x + threadIdx.x) - lane;
  if (r0 >= P) return;
  const uint32_t r = r0 + lane;
  const uint32_t my_off = offs[min(r, P)];
  const uint32_t start = offs[r0];
  const uint32_t end = offs[min(r0 + 64, P)];
  uint32_t g = 0, rlo = 0, rhi = 0;
  uint4 tab = make_uint4(0u, 0u, 0u, 0u);
  bool tall = false;  // rows beyond the row table (or a rect too wide for it)
  if (r < P) {
    g = sorted_g[r];
    if (offs[r + 1] > my_off) {
      const uint4 lw = lrec[g].w;
      const ushort4 rc = lr_rect(lw);
      rlo = lw.x;
      rhi = lw.y;
      tab = lrec[g].tab;
      tall = rc.w - rc.y > kRowTab || !rowtab_ok(rc);
    }
  }
  // rare: some Gaussian of the wave needs spans beyond its row table
  const bool any_tall = wave_any(tall);
  Reach rr{};
  if (any_tall && tall) rr = reach_of(splat[3 * (size_t)g], splat[3 * (size_t)g + 1]);
  for (uint32_t base = start; base < end; base += 64) {
    const uint32_t k = base + lane;
    const uint32_t kk = min(k, end - 1);
    int lo = 0, hi = 64;
#pragma unroll
    for (int it = 0; it < 6; ++it) {
      const int mid = (lo + hi) >> 1;
      const uint32_t v = __shfl(my_off, mid, 64);
      if (v <= kk) lo = mid; else hi = mid;
    }
    const uint32_t local = kk - __shfl(my_off, lo, 64);
    const uint32_t gg = __shfl(g, lo, 64);
    const uint32_t a = __shfl(rlo, lo, 64), b = __shfl(rhi, lo, 64);
    const int x0 = (int)(a & 0xFFFF), y0 = (int)(a >> 16), x1 = (int)(b & 0xFFFF), y1 = (int)(b >> 16);
    const uint4 tb = make_uint4(__shfl(tab.x, lo, 64), __shfl(tab.y, lo, 64), __shfl(tab.z, lo, 64),
                                __shfl(tab.w, lo, 64));
    // walk the table rows to the one holding list entry `local`
    const bool use_tab = x1 - x0 <= 255;
    const int nt = use_tab ? min(y1 - y0, kRowTab) : 0;
    uint32_t acc = 0, tx = 0, ty = 0;
    bool found = false;
    for (int row = 0; row < nt; ++row) {
      const uint32_t len = rowtab_len(tb, row);
      if (!found && local < acc + len) {
        ty = (uint32_t)(y0 + row);
        tx = (uint32_t)x0 + rowtab_x(tb, row) + (local - acc);
        found = true;
      }
      if (!found) acc += len;
    }
    if (any_tall) {  // wave-uniform: the shuffles need every lane
      Reach rg;
      rg.mx = __shfl(rr.mx, lo, 64); rg.my = __shfl(rr.my, lo, 64); rg.ca = __shfl(rr.ca, lo, 64);
      rg.cb = __shfl(rr.cb, lo, 64); rg.L = __shfl(rr.L, lo, 64); rg.det = __shfl(rr.det, lo, 64);
      rg.ey = __shfl(rr.ey, lo, 64); rg.dya = __shfl(rr.dya, lo, 64); rg.ica = __shfl(rr.ica, lo, 64);
      rg.ok = __shfl(rr.ok, lo, 64);
      for (int row = y0 + nt; !found && row < y1; ++row) {
        int xa;
        const uint32_t len = (uint32_t)row_span(rg, row, x0, x1, xa);
        if (local < acc + len) {
          ty = (uint32_t)row;
          tx = (uint32_t)xa + (local - acc);
          found = true;
        }
        acc += len;
      }
    }
    if (k < end) {
      keys[k] = ty * (uint32_t)gx + tx;
      slot_g[k] = gg;
      pflag[k] = 0;  // the backward's "record written" flag of this slot
    }
  }
}

// Exact tile mask of the splat inside bin (bx, by): bit rr 2^s + c for the
// tile (bx 2^s + c, by 2^s + rr) of its exact list (the row table, or
// row_span past it: the same spans k_duplicate enumerates).
__device__ __forceinline__ uint32_t bin_mask(int bx, int by, int bshift, int x0, int y0, int x1, int y1,
                                             const uint4& tab, bool tall, const Reach& rg) {
  const int B = 1 << bshift;
  const bool use_tab = x1 - x0 <= 255;
  uint32_t mask = 0;
  for (int rr = 0; rr < B; ++rr) {
    const int ty = (by << bshift) + rr;
    if (ty < y0 || ty >= y1) continue;
    const int kr = ty - y0;
    int xa, len;
    if (!tall || (use_tab && kr < kRowTab)) {
      xa = x0 + (int)rowtab_x(tab, kr);
      len = (int)rowtab_len(tab, kr);
    } else {
      len = row_span(rg, ty, x0, x1, xa);
    }
    const int cl = max(xa, bx << bshift), ch = min(xa + len, (bx << bshift) + B);
    if (ch > cl) mask |= ((1u << (ch - cl)) - 1u) << (rr * B + (cl - (bx << bshift)));
  }
  return mask;
}

// Exact tile mask inside bin (bx, by) of a splat whose rect rows all sit in
// its row table (not `tall`): the bin's 2^S rows' spans come out of the
// table as one byte run (rows above the rect shift in zeros, rows below it
// are zero in the table), each row a bit field of the mask.
template <int S>
__device__ __forceinline__ uint32_t bin_mask_tab(int bx, int by, int x0, int y0, const uint4& tab) {
  constexpr int B = 1 << S;
  const int kr0 = (by << S) - y0;  // in [-(B - 1), kRowTab - 1]
  const uint64_t L64 = ((uint64_t)tab.y << 32) | tab.x, X64 = ((uint64_t)tab.w << 32) | tab.z;
  // branch-free: one of the two shifts is by zero
  const uint32_t sr = 8u * (uint32_t)max(kr0, 0), sl = 8u * (uint32_t)max(-kr0, 0);
  const uint32_t lens = (uint32_t)((L64 >> sr) << sl);
  const uint32_t xs = (uint32_t)((X64 >> sr) << sl);
  const int d0 = x0 - (bx << S);  // the rect's left edge relative to the bin's
  uint32_t mask = 0;
#pragma unroll
  for (int rr = 0; rr < B; ++rr) {
    // row rr covers bin columns [lo, hi) (clamped to the bin; len >= 0 so
    // hi >= lo, and an empty or outside row gives lo == hi)
    const int xa = d0 + (int)((xs >> (8 * rr)) & 0xFFu);
    const int xe = xa + (int)((lens >> (8 * rr)) & 0xFFu);
    const int lo = min(max(xa, 0), B), hi = min(max(xe, 0), B);  // (v_med3_i32)
    mask |= (((1u << hi) - 1u) ^ ((1u << lo) - 1u)) << (rr * B);
  }
  return mask;
}

// Sort bins, after the dual scan's block sums (packed_scan_blocks: bsum[b]
// = the sums of (exact list length, bins touched) over 256-rank block b in
// depth order, bsup their 16-block sums): each 256-thread workgroup sums the
// blocks before its own and finishes the scan for its
// ranks (thread <-> rank) -- slot_start[g], the backward's record slots, and
// the ranks' first bin pair -- zeroes the "record written" flags of its slots,
// and every wave expands its 64 ranks' bin rectangles into (key, Gaussian)
// pairs: lane <-> pair, contiguous writes.  key = bin id (low 16 bits: the
// sort's digits) | the Gaussian's exact tile list inside the bin as a
// 2^s x 2^s tile mask (bin_mask; high 16 bits, carried through the sort).  A
// Gaussian's pairs in row-major bin order (the stable sort by bin keeps the
// depth order inside each bin).
// A pair's owner (the rank whose rectangle it belongs to) is found without a
// search: each rank with bins writes its lane id at its first pair's place
// in a 64-entry LDS row, and an inclusive max-scan over the row (DPP) hands
// every pair its owner -- the last rank starting at or before it; the
// owner's record (rect, first pair, Gaussian, row table) is read
// from LDS where every rank staged it (three LDS reads per pair instead of a
// six-step shuffle search and ten shuffles).
constexpr int kDupScanThreads = kPackedScanTile;  // one rank per thread
template <int S>
__global__ __launch_bounds__(kDupScanThreads) void k_duplicate_bins(
    uint32_t P, int gbx, const ListRec* __restrict__ lrec, const uint32_t* __restrict__ sorted_g,
    const uint2* __restrict__ bsum, const uint2* __restrict__ bsup, const float4* __restrict__ splat,
    uint32_t* __restrict__ slot_start, uint8_t* __restrict__ pflag, uint32_t* __restrict__ keys,
    uint32_t* __restrict__ vals, const ZeroJob zero, uint32_t* __restrict__ meta, uint32_t cap_slots,
    uint32_t cap_pairs) {
  // (cap_slots / cap_pairs: the capacity-mode forward's buffer sizes -- writes
  // past them are dropped and the forward flags the overflow; ~0 otherwise)
  constexpr int NW = kDupScanThreads / 64;
  constexpr int bshift = S;
  __shared__ uint2 s_w[NW], s_p[NW];
  __shared__ uint4 s_ra[NW][64];    // per rank: rect lo | hi, first bin pair, Gaussian
  __shared__ uint4 s_rt[NW][64];    // per rank: row table
  __shared__ uint2 s_rw[NW][64];    // per rank: bin columns of the rect, their reciprocal (float bits)
  __shared__ uint32_t s_own[NW][64];
  const int t = threadIdx.x, w = t >> 6, lane = t & 63;
  const uint32_t r = blockIdx.x * kDupScanThreads + t;
  const bool in = r < P;
  // ranks in index order: Gaussian g's slots are [slot_start[g], slot_start[g + 1]) (ImageLayout::meta[2])
  if (blockIdx.x == 0 && t == 0) meta[2] = sorted_g ? 0u : 1u;
  // (unconditional loads of a clamped rank, the selects after: a load under
  // `in` would be waited for at its join.)
  const uint32_t rc = min(r, P - 1u);
  const uint32_t g0 = sorted_g ? sorted_g[rc] : rc;  // (null: index order)
  // the whole 32-byte list record in one round trip (row table + rect, tb,
  // list length: one cache line)
  uint4 lw = lrec[g0].w, tab = lrec[g0].tab;
  // the block prefix's inputs, issued behind the record loads (the scans
  // below wait for the records only; vmcnt counts in order): the earlier
  // superblocks' sums plus the earlier blocks of its own superblock
  uint2 pre = make_uint2(0u, 0u);
  {
    const uint32_t b = blockIdx.x, sb = b / kScanSupBlocks;
    for (uint32_t q = (uint32_t)t; q < sb; q += kDupScanThreads) {
      const uint2 x = bsup[(size_t)q * kScanSupStride];
      pre.x += x.x;
      pre.y += x.y;
    }
    if ((uint32_t)t < kScanSupBlocks && sb * kScanSupBlocks + t < b) {
      const uint2 x = bsum[sb * kScanSupBlocks + t];
      pre.x += x.x;
      pre.y += x.y;
    }
  }
  const uint32_t g = in ? g0 : 0u;
  if (!in) {
    lw = make_uint4(0u, 0u, 0u, 0u);
    tab = lw;
  }
  const uint32_t v = lw.z;
  const uint32_t cnt = v & 0xFFFFu, nb = v >> 16;
  uint32_t rlo = 0, rhi = 0;
  bool tall = false;
  if (nb) {
    const ushort4 rc = lr_rect(lw);
    rlo = lw.x;
    rhi = lw.y;  // exclusive
    tall = rc.w - rc.y > kRowTab || !rowtab_ok(rc);
  } else {
    tab = make_uint4(0u, 0u, 0u, 0u);
  }
  const uint32_t ic = wave_incl_scan(cnt), ib = wave_incl_scan(nb);
  if (lane == 63) s_w[w] = make_uint2(ic, ib);
  pre.x = wave_sum_u32(pre.x);
  pre.y = wave_sum_u32(pre.y);
  if (lane == 0) s_p[w] = pre;
  __syncthreads();
  uint2 wb = make_uint2(0u, 0u);  // this block's first slot / first bin pair
#pragma unroll
  for (int k = 0; k < NW; ++k) {
    wb.x += s_p[k].x;
    wb.y += s_p[k].y;
  }
#pragma unroll
  for (int k = 0; k < NW; ++k) {
    const uint2 x = s_w[k];
    if (k < w) { wb.x += x.x; wb.y += x.y; }
  }
  const uint2 wt = s_w[w];  // the wave's totals
  if (in) slot_start[g] = wb.x + ic - cnt;
  // the wave's slots are contiguous: dword stores for the aligned interior,
  // byte stores for the (< 4-byte) head and tail
  {
    const uint32_t f0 = wb.x, f1 = min(wb.x + wt.x, cap_slots);
    const uint32_t a0 = min((f0 + 3u) & ~3u, max(f1, f0)), a1 = max(f1 & ~3u, a0);
    if (lane < (int)(a0 - f0)) pflag[f0 + lane] = 0;
    if (lane < (int)(f1 - a1)) pflag[a1 + lane] = 0;
    uint32_t* pw = reinterpret_cast<uint32_t*>(pflag);
    for (uint32_t k = (a0 >> 2) + lane; k < (a1 >> 2); k += 64) pw[k] = 0u;
  }
  // scratch the bin sort needs zeroed (its superblock sums)
  zero_share(zero, blockIdx.x, gridDim.x, t, kDupScanThreads);
  if (wt.y == 0) return;  // wave-uniform; no barrier below
  const uint32_t my_off = wb.y + ib - nb;  // first bin pair of this rank
  const uint32_t start = wb.y, end = wb.y + wt.y;
  const bool any_tall = wave_any(tall);
  Reach rr{};
  if (any_tall && tall) rr = reach_of(splat[3 * (size_t)g], splat[3 * (size_t)g + 1]);
  // every rank's record, for its pairs' lanes
  s_ra[w][lane] = make_uint4(rlo, rhi, my_off, g);
  s_rt[w][lane] = tab;
  {  // the rect's bin-column count and its reciprocal, once per rank
    const int bw = (((int)(rhi & 0xFFFFu) - 1) >> bshift) - ((int)(rlo & 0xFFFFu) >> bshift) + 1;
    s_rw[w][lane] = make_uint2((uint32_t)bw, __float_as_uint(__builtin_amdgcn_rcpf((float)bw)));
  }
  uint32_t carry = 0;  // owner of the chunk's first pair (the first chunk: a rank starts there)
  for (uint32_t base = start; base < end; base += 64) {
    const uint32_t k = base + lane;
    const uint32_t kk = min(k, end - 1);
    // owner of pair kk: the highest lane with bins whose first pair is <= kk
    // (lanes without bins share their successor's offset: they do not write)
    s_own[w][lane] = lane == 0 ? carry : 0u;
    __builtin_amdgcn_wave_barrier();
    if (nb && my_off >= base && my_off < base + 64) s_own[w][my_off - base] = (uint32_t)lane;
    __builtin_amdgcn_wave_barrier();
    const uint32_t lo = wave_incl_max(s_own[w][lane]);
    carry = (uint32_t)__builtin_amdgcn_readlane((int)lo, 63);
    const uint4 ra = s_ra[w][lo];
    const uint32_t local = kk - ra.z;
    const uint32_t gg = ra.w;
    const int x0 = (int)(ra.x & 0xFFFFu), y0 = (int)(ra.x >> 16), x1 = (int)(ra.y & 0xFFFFu), y1 = (int)(ra.y >> 16);
    const uint4 tq = s_rt[w][lo];
    const uint2 rw = s_rw[w][lo];
    const int bx0 = x0 >> bshift, bw = (int)rw.x;
    // local / bw without the integer-division sequence: local < 2^16 (a
    // Gaussian's bins), so the float estimate is within one of the quotient
    int row = (int)((float)local * __uint_as_float(rw.y));
    int col = (int)local - row * bw;
    {  // (selects, not branches)
      const int dn = col < 0 ? 1 : 0, up = col >= bw ? 1 : 0;
      row += up - dn;
      col += (dn - up) * bw;
    }
    const int bx = bx0 + col, by = (y0 >> bshift) + row;
    uint32_t mask;
    if (!any_tall) {  // (wave-uniform) every owner's rows sit in its row table
      mask = bin_mask_tab<S>(bx, by, x0, y0, tq);
    } else {
      const bool tl = __shfl((int)tall, (int)lo, 64) != 0;
      Reach rg;  // (the shuffles need every lane)
      rg.mx = __shfl(rr.mx, lo, 64); rg.my = __shfl(rr.my, lo, 64); rg.ca = __shfl(rr.ca, lo, 64);
      rg.cb = __shfl(rr.cb, lo, 64); rg.L = __shfl(rr.L, lo, 64); rg.det = __shfl(rr.det, lo, 64);
      rg.ey = __shfl(rr.ey, lo, 64); rg.dya = __shfl(rr.dya, lo, 64); rg.ica = __shfl(rr.ica, lo, 64);
      rg.ok = __shfl(rr.ok, lo, 64);
      mask = tl ? bin_mask(bx, by, bshift, x0, y0, x1, y1, tq, true, rg) : bin_mask_tab<S>(bx, by, x0, y0, tq);
    }
    if (k < end && k < cap_pairs) {
      keys[k] = (uint32_t)(by * gbx + bx) | (mask << 16);
      vals[k] = gg;
    }
    __builtin_amdgcn_wave_barrier();  // (the next chunk's owner row is rewritten)
  }
}

// [start, end) of every bin in the bin-sorted keys (upstream's
// identifyTileRanges on bin ids): one thread per entry, bins with no entry
// keep the zero range written before the launch.
__global__ __launch_bounds__(256) void k_bin_bounds(const uint32_t* __restrict__ skeys, uint32_t NB,
                                                    uint2* __restrict__ bounds) {
  const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= NB) return;
  const uint32_t b = skeys[e] & 0xFFFFu;
  if (e == 0 || (skeys[e - 1] & 0xFFFFu) != b) bounds[b].x = e;
  if (e + 1 == NB || (skeys[e + 1] & 0xFFFFu) != b) bounds[b].y = e + 1;
}

// One workgroup per (bin, row of its tiles): the exact lists of the row's
// 2^s tiles, in depth order, out of the bin's sorted entries -- an entry
// belongs to tile c if bit c of its key's row mask is set; a block-wide
// stable compaction per tile (one ballot per wave, a cross-wave prefix)
// keeps the order, kExpThreads entries per step (the next step's keys and
// ids in flight).  Tile (r, c) of a bin whose entries sit at [lo, hi) writes
// at lists[2^2s lo + (r 2^s + c) (hi - lo) ...], a region as long as the
// bin's list: no count pass, no overlap.  (Measured at 1M/1080p: 256
// threads 44 us; one wave per row 73 us -- a bin's ~2000 entries then take
// ~35 dependent steps; 512 threads 55 us -- fewer workgroups in flight.)
constexpr int kExpThreads = 256;
__global__ __launch_bounds__(kExpThreads) void k_expand_bins(const uint32_t* __restrict__ skeys,
                                                             const uint32_t* __restrict__ sgid,
                                                             const uint2* __restrict__ bounds, int gx, int gy,
                                                             int bshift, int gbx, uint32_t* __restrict__ lists,
                                                             uint2* __restrict__ ranges,
                                                             uint32_t* __restrict__ tile_len,
                                                             uint32_t* __restrict__ meta) {
  constexpr int NW = kExpThreads / 64;
  const int t = threadIdx.x, w = t >> 6, lane = t & 63;
  if (blockIdx.x == 0 && t == 0) meta[0] = 1u;  // the lists are the sort-bin region
  const int B = 1 << bshift;
  // (an XCD-aware mapping -- the 2^s row workgroups of a bin on one XCD, so
  // that the bin comes from HBM once -- measured 31.5 vs 30.8 us: the rows'
  // re-reads already hit the last-level cache)
  const uint32_t bin = blockIdx.x >> bshift;
  const int r = (int)(blockIdx.x & (uint32_t)(B - 1));
  const int bx = (int)(bin % (uint32_t)gbx), by = (int)(bin / (uint32_t)gbx);
  const int ty = (by << bshift) + r;
  if (ty >= gy) return;  // block-uniform
  const uint2 bb = bounds[bin];
  const uint32_t lo = bb.x, hi = bb.y, len = hi - lo;
  const size_t base0 = ((size_t)lo << (2 * bshift)) + (size_t)(r << bshift) * len;
  const uint32_t shift = 16u + ((uint32_t)r << bshift), rmask = (1u << B) - 1u;
  uint32_t count[4] = {0u, 0u, 0u, 0u};
  // the step's per-wave counts of each tile as four 16-bit fields of one
  // 64-bit LDS word (<= 4 x 64 entries per field): each wave's cross-wave
  // prefix is three conditional 64-bit adds instead of 16 LDS reads and 32
  // adds; the words are double-buffered by step parity, so a step needs one
  // barrier (a wave rewrites a buffer only after the next step's barrier,
  // which every wave passes after reading it); stores through a uniform base
  // pointer with 32-bit offsets.  (Measured: 31.2 -> 28.5 us at 1M / 1080p
  // against per-wave LDS counts with two barriers per step; two entries per
  // thread per step: 35.5 us.)
  __shared__ unsigned long long s_wp[2][NW];
  uint32_t* const out0 = lists + base0;
  uint32_t key = lo + t < hi ? skeys[lo + t] : 0u, gid = lo + t < hi ? sgid[lo + t] : 0u;
  asm volatile("" ::"v"(key), "v"(gid));
  int par = 0;
  for (uint32_t e0 = lo; e0 < hi; e0 += kExpThreads, par ^= 1) {
    const uint32_t bits = (key >> shift) & rmask, my_gid = gid;
    const uint32_t e1 = e0 + kExpThreads + t;
    key = e1 < hi ? skeys[e1] : 0u;
    gid = e1 < hi ? sgid[e1] : 0u;
    uint64_t m[4];
    unsigned long long packed = 0ull;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      m[c] = wave_ballot(c < B && ((bits >> c) & 1u));
      packed |= (unsigned long long)__popcll(m[c]) << (16 * c);
    }
    if (lane == 0) s_wp[par][w] = packed;
    __syncthreads();
    unsigned long long off = 0ull, tot = 0ull;
#pragma unroll
    for (int k = 0; k < NW; ++k) {
      const unsigned long long v = s_wp[par][k];
      off += k < w ? v : 0ull;
      tot += v;
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (c >= B) break;
      if ((bits >> c) & 1u)
        out0[(uint32_t)c * len + count[c] + (uint32_t)((off >> (16 * c)) & 0xFFFFull) + lanes_below(m[c])] = my_gid;
      count[c] += (uint32_t)((tot >> (16 * c)) & 0xFFFFull);
    }
    asm volatile("" ::"v"(key), "v"(gid));
  }
  if (t < B) {
    const int tx = (bx << bshift) + t;
    if (tx < gx) {
      const uint32_t tile = (uint32_t)ty * (uint32_t)gx + (uint32_t)tx;
      const size_t b0 = base0 + (size_t)t * len;
      uint32_t c = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) c = k == t ? count[k] : c;
      ranges[tile] = make_uint2((uint32_t)b0, (uint32_t)b0 + c);
      tile_len[tile] = c;
    }
  }
}

// ---- tile ranges and the tiles' launch order ---------------------------------
// The render kernels take tile order[xcd_remap(blockIdx)]: blocks b with the
// same b % 8 run on one XCD (round-robin dispatch), and xcd_remap hands each
// XCD a contiguous chunk of tiles (a band of the image: splat records shared
// by neighbouring tiles stay in that XCD's L2).  Inside a chunk the tiles are
// ordered heaviest first (longest-processing-time list scheduling): with ~2
// waves per SIMD slot over the kernel, launch order decides the makespan
// (bench scene, backward: 68 % -> 91 % of the ideal in a list-scheduling
// simulation).  Order only changes scheduling, never a result.
constexpr int kOrderBuckets = 1024;

__device__ __forceinline__ void tile_chunk(uint32_t x, uint32_t nt, uint32_t& c0, uint32_t& c1) {
  const uint32_t q = nt / 8, r = nt % 8;
  c0 = x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q;
  c1 = c0 + (x < r ? q + 1 : q);
}

// Counting sort of the chunk's tiles by descending work bucket (one
// 1024-thread workgroup per chunk; positions inside a bucket come from LDS
// atomics, so ties may land in any order).
// work of a tile: the max of its quadrants' work[4 tile .. 4 tile + 3]
__device__ __forceinline__ uint32_t tile_work(const uint32_t* __restrict__ work, uint32_t tile) {
  const uint4 q = reinterpret_cast<const uint4*>(work)[tile];
  return max(max(q.x, q.y), max(q.z, q.w));
}

__device__ __forceinline__ void order_chunk(uint32_t c0, uint32_t c1, const uint32_t* __restrict__ work,
                                            uint32_t* __restrict__ order, uint32_t* s_cnt) {
  const int t = threadIdx.x;
  s_cnt[t] = 0;
  __syncthreads();
  auto bucket = [&](uint32_t tile) {
    return (uint32_t)(kOrderBuckets - 1) - min((uint32_t)(kOrderBuckets - 1), tile_work(work, tile));
  };
  for (uint32_t tile = c0 + t; tile < c1; tile += 1024) atomicAdd(&s_cnt[bucket(tile)], 1u);
  __syncthreads();
  // exclusive scan of the 1024 bucket counts (one per thread)
  __shared__ uint32_t s_w[16];
  const uint32_t v = s_cnt[t];
  uint32_t inc = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t o = __shfl_up(inc, off, 64);
    if ((t & 63) >= off) inc += o;
  }
  if ((t & 63) == 63) s_w[t >> 6] = inc;
  __syncthreads();
  uint32_t base = 0;
  for (int i = 0; i < (t >> 6); ++i) base += s_w[i];
  __syncthreads();
  s_cnt[t] = base + inc - v;
  __syncthreads();
  for (uint32_t tile = c0 + t; tile < c1; tile += 1024) order[c0 + atomicAdd(&s_cnt[bucket(tile)], 1u)] = tile;
}

// ranges[tile] = [first, end) of the tile's run in the sorted pair keys
// (binary search); len[tile] = its list length.
__global__ __launch_bounds__(256) void k_ranges(const uint32_t* __restrict__ keys, uint32_t N, int ntiles,
                                                uint2* __restrict__ ranges, uint32_t* __restrict__ len,
                                                uint32_t* __restrict__ meta) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t == 0) meta[0] = 0u;  // the lists are point_g
  if (t >= ntiles) return;
  auto lower = [&](uint32_t v) {
    uint32_t lo = 0, hi = N;
    while (lo < hi) {
      const uint32_t mid = (lo + hi) >> 1;
      if (keys[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
  };
  const uint2 r = make_uint2(lower((uint32_t)t), lower((uint32_t)t + 1));
  ranges[t] = r;
  len[t] = r.y - r.x;
}

// The backward's launch order by each tile's deepest contributor (its
// back-to-front walk length), written by the forward.
// One workgroup per XCD chunk.
__global__ __launch_bounds__(1024) void k_tile_order(const uint32_t* __restrict__ work, uint32_t ntiles,
                                                     uint32_t* __restrict__ order) {
  __shared__ uint32_t s_cnt[kOrderBuckets];
  uint32_t c0, c1;
  tile_chunk(blockIdx.x, ntiles, c0, c1);
  order_chunk(c0, c1, work, order, s_cnt);
}

}  // namespace

hipError_t launch_duplicate_bins(const wgsr_raster_args& a, void* geom, const uint32_t* depth_order, int bshift,
                                 uint8_t* pflag, uint32_t* keys, uint32_t* vals, const ZeroJob& zero,
                                 uint32_t* meta, hipStream_t s, uint32_t cap_slots, uint32_t cap_pairs) {
  if (a.P == 0) return hipSuccess;
  const GeomLayout L(a.P);
  const Bins B((a.W + kTile - 1) / kTile, (a.H + kTile - 1) / kTile, bshift);
  if (bshift < 1 || bshift > kMaxBinShift) return hipErrorInvalidValue;
  hipLaunchKernelGGL(bshift == 1 ? k_duplicate_bins<1> : k_duplicate_bins<2>,
                     dim3((a.P + kDupScanThreads - 1) / kDupScanThreads), dim3(kDupScanThreads), 0,
                     s, (uint32_t)a.P, B.bx, at<ListRec>(geom, L.lrec), depth_order, at<uint2>(geom, L.bsum),
                     at<uint2>(geom, L.bsup), at<float4>(geom, L.splat),
                     at<uint32_t>(geom, L.slot_start), pflag, keys, vals, zero, meta, cap_slots, cap_pairs);
  return hipGetLastError();
}

// every bin's [start, end) in the NB bin-sorted keys, unless a one-pass sort
// already wrote them (bounds_done)
hipError_t make_bin_bounds(const uint32_t* sorted_keys, uint32_t NB, int nbins, uint2* bounds, bool bounds_done,
                           hipStream_t s) {
  if (bounds_done) return hipSuccess;
  hipError_t e = hipMemsetAsync(bounds, 0, sizeof(uint2) * (size_t)nbins, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_bin_bounds, dim3((NB + 255) / 256), dim3(256), 0, s, sorted_keys, NB, bounds);
  return hipSuccess;
}

hipError_t launch_expand_bins(const wgsr_raster_args& a, const uint32_t* sorted_keys, const uint32_t* sorted_g,
                              uint32_t NB, int bshift, uint2* bounds, bool bounds_done, uint32_t* lists, uint2* ranges,
                              uint32_t* tile_len, uint32_t* meta, hipStream_t s) {
  const int gx = (a.W + kTile - 1) / kTile, gy = (a.H + kTile - 1) / kTile;
  const Bins B(gx, gy, bshift);
  hipError_t e = make_bin_bounds(sorted_keys, NB, B.n, bounds, bounds_done, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_expand_bins, dim3((uint32_t)B.n << bshift), dim3(kExpThreads), 0, s, sorted_keys, sorted_g, bounds, gx,
                     gy, bshift, B.bx, lists, ranges, tile_len, meta);
  return hipGetLastError();
}

hipError_t launch_duplicate(const wgsr_raster_args& a, const void* geom, const uint32_t* sorted_g, uint32_t P,
                            uint32_t* keys, uint32_t* slot_g, uint8_t* pflag, hipStream_t s) {
  if (P == 0) return hipSuccess;
  const GeomLayout L(P);
  const int gx = (a.W + kTile - 1) / kTile;
  hipLaunchKernelGGL(k_duplicate, dim3((P + 255) / 256), dim3(256), 0, s, P, gx, at<uint32_t>(geom, L.offs),
                     sorted_g, at<ListRec>(geom, L.lrec), at<float4>(geom, L.splat),
                     keys, slot_g, pflag);
  return hipGetLastError();
}

hipError_t launch_ranges(const uint32_t* sorted_keys, uint32_t N, int ntiles, uint2* ranges, uint32_t* len,
                         uint32_t* meta, hipStream_t s) {
  hipLaunchKernelGGL(k_ranges, dim3((ntiles + 255) / 256), dim3(256), 0, s, sorted_keys, N, ntiles, ranges, len, meta);
  return hipGetLastError();
}

hipError_t launch_tile_order(const uint32_t* work_quads, int ntiles, uint32_t* order, hipStream_t s) {
  // per-XCD chunks (one global LPT list measured 2 % slower)
  hipLaunchKernelGGL(k_tile_order, dim3(8), dim3(1024), 0, s, work_quads, (uint32_t)ntiles, order);
  return hipGetLastError();
}

// Consistency check of a forward's tile lists (wgsr_check_tile_lists): one
// wave per tile.  bad[0] += tiles whose [start, end) leaves the list region
// or disagrees with tile_len; bad[1] += listed ids >= P; bad[2] += pixels
// whose last contributor lies beyond their tile's list.  The entries of a
// tile with a bad range are not read.
__global__ __launch_bounds__(64) void k_check_tile_lists(const uint2* __restrict__ ranges,
                                                         const uint32_t* __restrict__ tile_len,
                                                         const uint32_t* __restrict__ meta,
                                                         const uint32_t* __restrict__ lists_exact,
                                                         const uint32_t* __restrict__ lists_bins, uint64_t n_exact,
                                                         uint64_t n_bins, uint32_t P, int W, int H, int gx,
                                                         const uint32_t* __restrict__ n_contrib,
                                                         uint32_t* __restrict__ bad) {
  const uint32_t tile = blockIdx.x;
  const int lane = threadIdx.x;
  const bool bins = meta[0] != 0u;
  const uint32_t* __restrict__ lists = bins ? lists_bins : lists_exact;
  const uint64_t region = bins ? n_bins : n_exact;
  const uint2 r = ranges[tile];
  const bool ok = r.x <= r.y && (uint64_t)r.y <= region && tile_len[tile] == r.y - r.x;
  if (!ok) {
    if (lane == 0) atomicAdd(&bad[0], 1u);
    return;
  }
  uint32_t nb = 0;
  for (uint32_t e = r.x + (uint32_t)lane; e < r.y; e += 64) nb += lists[e] >= P ? 1u : 0u;
  const int tx0 = (int)(tile % (uint32_t)gx) * kTile, ty0 = (int)(tile / (uint32_t)gx) * kTile;
  uint32_t np = 0;
  for (int q = lane; q < kTile * kTile; q += 64) {
    const int px = tx0 + (q % kTile), py = ty0 + (q / kTile);
    if (px < W && py < H) np += n_contrib[(size_t)py * W + px] > r.y - r.x ? 1u : 0u;
  }
  if (nb) atomicAdd(&bad[1], nb);
  if (np) atomicAdd(&bad[2], np);
}

// p[0..n) = 0 by a kernel: the capacity-mode forward zeroes its buffers with
// kernel nodes, not memset nodes.  A hipMemsetAsync captured into a HIP graph
// (a memset node) was measured NOT to have zeroed the counter block before
// k_preprocess accumulated into it on some replays -- the two-rank
// data-parallel loop on one GPU: a replayed forward of an unchanged map and
// camera reported N_rect >= 2^32 while the eager forward of the same state
// gave 8561, deterministically, and the kernel zeroing below fixed it.  Garbage
// counts make the bin sort take `cap` keys of which only the written ones are
// valid, so the per-bin sort then gathers depth keys through unwritten
// Gaussian ids: the out-of-bounds reads behind round 5's SIGABRT in the
// overflow-recovery test are consistent with it.
__global__ __launch_bounds__(256) void k_zero_u32(uint32_t* __restrict__ p, size_t n) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) p[i] = 0u;
}

hipError_t launch_zero_u32(uint32_t* p, size_t n, hipStream_t s) {
  if (n == 0) return hipSuccess;
  const size_t blocks = std::min<size_t>((n + 255) / 256, 1024);
  hipLaunchKernelGGL(k_zero_u32, dim3((uint32_t)blocks), dim3(256), 0, s, p, n);
  return hipGetLastError();
}

hipError_t launch_check_tile_lists(const wgsr_raster_args& a, int bshift, uint64_t num_rendered, const void* binning,
                                   const void* image, uint32_t* bad, hipStream_t s) {
  const int gx = (a.W + kTile - 1) / kTile, gy = (a.H + kTile - 1) / kTile;
  const ImageLayout IL(a.W, a.H);
  const BinLayout BL((size_t)num_rendered);
  hipLaunchKernelGGL(k_check_tile_lists, dim3((uint32_t)(gx * gy)), dim3(64), 0, s, at<uint2>(image, IL.ranges),
                     at<uint32_t>(image, IL.tile_len), at<uint32_t>(image, IL.meta), at<uint32_t>(binning, BL.point_g),
                     at<uint32_t>(binning, BL.total), num_rendered, num_rendered << (2 * bshift), (uint32_t)a.P, a.W,
                     a.H, gx, at<uint32_t>(image, IL.n_contrib), bad);
  return hipGetLastError();
}

}  // namespace wgsr
