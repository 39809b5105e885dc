// Per-bin depth sort of the rasteriser forward (the
// default schedule): one workgroup per sort bin orders the bin's entries by
// depth in LDS and emits the bin's per-tile lists, ranges and list lengths.
// k_argsort_small runs the same LDS passes on one small key array.
#include "wgsr_common.h"
#include "wgsr_internal.h"

namespace wgsr {

namespace {

// ---- per-bin depth sort (the default with sort bins) ---------------------------
// With the Gaussians duplicated in INDEX order (no global depth sort), the
// stable bin sort leaves every bin's entries in index order, one entry per
// Gaussian.  Sorting each bin stably by depth key then yields exactly the
// order a stable global depth sort leaves inside the bin: depth bits, ties by
// Gaussian index -- upstream's (tile | depth) key order with cub's stable tie
// order.  One 512-thread workgroup per bin: the bin's depth
// keys minus their minimum (R bits) are LSD-radix sorted in LDS, ceil(R / 9)
// stable passes of <= 9-bit digits, each entry's position in the bin riding
// along; the (key, Gaussian) pairs are then gathered in that order and cut
// into the bin's per-tile lists (BdsEmit below), at every bin shift.  A bin of
// more than kBdsCap entries runs the same passes chunk by chunk through global
// scratch (the region behind the lists).
// (The emit: each wave walks the sorted bin once for the tiles it owns,
// bds_emit_walk.  4 x 4-tile bins, 1M / 1080p: k_bin_depth_sort 39.5 -> 50.1
// us with k_expand_bins' 29.5 us and its launch gone, 0.7473 -> 0.7325 ms per
// step; 2 x 2-tile bins (100k 512 x 384, the online loop): 0.1672 -> 0.1665
// and 0.7223 -> 0.7199 ms.  The earlier lane <-> entry emit
// (a count pass, a prefix over the waves, a write pass) lost to k_expand_bins
// at 4 x 4 tiles (140.8 vs 131.3 us) and is gone.)
// (512 threads, up to 10 entries per lane in steps of one: 1024 threads with
// 1, 2, 4, 7 entries per lane measured 42-46 vs 33 us at 1M / 1080p)
constexpr int kBdsThreads = 512, kBdsWaves = kBdsThreads / 64, kBdsItems = 10;
constexpr int kBdsCap = kBdsThreads * kBdsItems;  // entries sorted in LDS
constexpr int kBdsMaxBits = 9, kBdsDigits = 1 << kBdsMaxBits;
static_assert(kBdsDigits <= kBdsThreads, "threads t < kBdsDigits own digit t");
__device__ __forceinline__ bool bds_owns_digit() { return (int)threadIdx.x < kBdsDigits; }

// Peer groups (the wave's lanes holding the same digit) from per-(wave,
// digit) 64-bit lane masks in LDS: one ds_or_b64 + one read per entry group
// instead of one ballot and a 64-bit select per digit bit.  A wave's LDS
// instructions complete in order, so every lane's OR lands before any lane's
// read, and every read before the clear behind it.
// The lane-mask table shares LDS with the staging buffer (a pass ranks with
// the table, then scatters into the buffer; the table is zeroed again before
// the next pass) -- 61 instead of 93 KB per 512-thread workgroup, two
// workgroups per CU: the 1M frame's 510 bins in one round.  (Peer groups by
// ballots: 73 vs 45.5 us at 1M, round 3.)
struct BdsLds {
  union {
    uint2 buf[kBdsCap];                                // (depth key, position in the bin)
    unsigned long long match[kBdsWaves][kBdsDigits];  // lane masks per digit (zero between uses)
  };
  uint32_t wcnt[kBdsWaves][kBdsDigits];   // per wave digit counts, then their prefix over waves
  uint32_t base[kBdsDigits];              // per digit: first slot
  uint32_t tmp[kBdsWaves];
  uint32_t rng[2][kBdsWaves];
  uint32_t ecnt[16];                      // emit: entries per tile of the bin, written by the tile's wave
};

// The bin's exact per-tile lists, emitted straight from the depth-sorted bin
// (what k_expand_bins does from a global copy of it): tile k = r 2^s + c of
// the bin gets, in depth order, every entry whose key has bit 16 + k set, at
// lists[2^2s lo + k n + ...] (n = the bin's length: no count pass, no
// overlap).  The walk is wave <-> tile: a chunk's sorted (tile mask, Gaussian)
// pairs are staged once into L.buf (free after the last pass), and after one
// barrier every wave walks the staged list 64 entries at a time for the
// tiles it owns -- per step one 64-bit LDS read shared by its tiles, and per
// tile a bit test, a ballot, a scalar popcount and one store at k n + running
// count + lanes below.  A wave owns its tiles' whole lists, so there is no
// count pass, no prefix over the waves and no barrier inside the walk; the
// running counts are wave-uniform and carry across the chunks of a big bin.
//   16 tiles (s = 2): wave w owns tiles w and w + 8.
//    4 tiles (s = 1): waves w and w + 4 share tile w: both walk the whole
//      chunk and count every hit (so both hold the tile's running count with
//      no exchange), w stores the first half of the 64-entry groups and w + 4
//      the second.  Counting a group is the read, the ballot and the popcount
//      -- a fraction of a storing step -- so all eight waves work and the
//      longest chain is half the stores of one wave per tile.
struct BdsEmit {
  uint32_t* __restrict__ lists;
  uint2* __restrict__ ranges;
  uint32_t* __restrict__ tile_len;
  uint32_t* __restrict__ meta;
  int gx, gy, bshift, gbx;
};

// TPW tiles per wave: 2 (16 tiles) or 1 (4 tiles, two waves per tile)
template <int TPW>
__device__ __forceinline__ void bds_emit_walk(BdsLds& L, uint32_t cnt, uint32_t* __restrict__ out, uint32_t n,
                                              uint32_t (&run)[2]) {
  static_assert(TPW == 1 || TPW == 2, "16 or 4 tiles over eight waves");
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // (an SGPR)
  const uint32_t groups = (cnt + 63u) >> 6;
  const uint32_t k0 = TPW == 2 ? w : (w & 3u);
  uint32_t g0 = 0u, g1 = groups;  // the groups whose hits this wave stores
  if (TPW == 1) {
    const uint32_t h = (groups + 1u) >> 1;
    if (w >> 2) g0 = h; else g1 = h;
  }
  // each tile's next free slot as a uniform pointer (advanced by scalar
  // popcounts): a store is that base plus a 32-bit lane offset
  uint32_t kbit[TPW];
  uint32_t* dst[TPW];
#pragma unroll
  for (int i = 0; i < TPW; ++i) {
    const uint32_t k = k0 + 8u * (uint32_t)i;
    kbit[i] = 1u << k;
    dst[i] = out + (size_t)k * n + run[i];
  }
  auto emit = [&](const uint2 e, uint32_t g) {
    const bool st = TPW == 2 || (g >= g0 && g < g1);  // wave-uniform
#pragma unroll
    for (int i = 0; i < TPW; ++i) {
      const bool bit = (e.x & kbit[i]) != 0u;
      const uint64_t b = wave_ballot(bit);
      if (st && bit) dst[i][lanes_below(b)] = e.y;
      dst[i] += __popcll(b);
    }
  };
  // two groups per trip, each group's read in flight over the other's stores
  // (the group past cnt is staged with zero masks)
  const uint2* src = L.buf + lane;
  uint2 ea = src[0], eb;
  uint32_t g = 0;
  for (; g + 1u < groups; g += 2u) {
    eb = src[(g + 1u) * 64u];
    emit(ea, g);
    if (g + 2u < groups) ea = src[(g + 2u) * 64u];
    emit(eb, g + 1u);
  }
  if (g < groups) emit(ea, g);
#pragma unroll
  for (int i = 0; i < TPW; ++i) {
    const uint32_t k = k0 + 8u * (uint32_t)i;
    run[i] = (uint32_t)(dst[i] - (out + (size_t)k * n));
    if (lane == 0u && (TPW == 2 || w < 4u)) L.ecnt[k] = run[i];  // (the last chunk's is the tile's length)
  }
}

// One chunk: wave w's lanes hold sorted positions (w JN + j) 64 + lane of it
// in m[j] (the tile mask, 0 past cnt) and g[j] (the Gaussian).  run: the
// wave's tiles' entries so far (zero before the bin's first chunk).
template <int JN>
__device__ __forceinline__ void bds_emit_chunk(BdsLds& L, const uint32_t (&m)[JN], const uint32_t (&g)[JN],
                                               uint32_t cnt, int NT, uint32_t* __restrict__ out, uint32_t n,
                                               uint32_t (&run)[2]) {
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int j = 0; j < JN; ++j)
    if ((uint32_t)(w * JN + j) * 64u < cnt)  // wave-uniform: whole groups, the last one zero-padded
      L.buf[(uint32_t)(w * JN + j) * 64u + (uint32_t)lane] = make_uint2(m[j], g[j]);
  __syncthreads();
  if (NT == 16)
    bds_emit_walk<2>(L, cnt, out, n, run);
  else
    bds_emit_walk<1>(L, cnt, out, n, run);
  __syncthreads();  // the buffer is restaged by the next chunk; ecnt is read by bds_emit_ranges
}

// the bin's ranges / list lengths (and the lists' location flag), after its last chunk
__device__ __forceinline__ void bds_emit_ranges(const BdsLds& L, const BdsEmit& E, uint32_t bin, uint32_t lo,
                                                uint32_t n) {
  const int t = threadIdx.x;
  const int B = 1 << E.bshift;
  if (bin == 0 && t == 0) E.meta[0] = 1u;  // the lists are the sort-bin region
  if (t < B * B) {
    const int r = t >> E.bshift, c = t & (B - 1);
    const int bx = (int)(bin % (uint32_t)E.gbx), by = (int)(bin / (uint32_t)E.gbx);
    const int tx = (bx << E.bshift) + c, ty = (by << E.bshift) + r;
    if (tx < E.gx && ty < E.gy) {
      const uint32_t tile = (uint32_t)ty * (uint32_t)E.gx + (uint32_t)tx;
      const uint32_t b0 = (lo << (2 * E.bshift)) + (uint32_t)t * n;
      const uint32_t c_t = n ? L.ecnt[t] : 0u;
      E.ranges[tile] = make_uint2(b0, b0 + c_t);
      E.tile_len[tile] = c_t;
    }
  }
}

__device__ __forceinline__ uint32_t bds_excl_scan(uint32_t v, uint32_t* s_tmp, uint32_t* total) {
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint32_t inc = wave_incl_scan(v);
  if (lane == 63) s_tmp[w] = inc;
  __syncthreads();
  uint32_t base = 0, tot = 0;
#pragma unroll
  for (int i = 0; i < kBdsWaves; ++i) {
    const uint32_t x = s_tmp[i];
    base += i < w ? x : 0u;
    tot += x;
  }
  __syncthreads();
  *total = tot;
  return base + inc - v;
}

// wave w owns the cn entries' slots [w pw, w pw + pw) (pw a multiple of 64,
// so all eight waves share the work), walked 64 at a time: ranks follow slot
// order (stable).  pk[j] packs the entry's position in the bin (bits 0-12),
// its digit (13-21) and its rank among the wave's entries of that digit
// (22-31, < 14 x 64); bds_rank fills bits 13-31.
constexpr int kBdsPosBits = 13, kBdsRankShift = kBdsPosBits + kBdsMaxBits;
static_assert(kBdsCap <= (1 << kBdsPosBits) && kBdsItems * 64 <= (1 << (32 - kBdsRankShift)), "pk packing");
__device__ __forceinline__ uint32_t bds_digit(uint32_t pk) { return (pk >> kBdsPosBits) & (kBdsDigits - 1); }
__device__ __forceinline__ uint32_t bds_pos(uint32_t pk) { return pk & ((1u << kBdsPosBits) - 1u); }
template <int JN>
__device__ __forceinline__ void bds_rank(BdsLds& L, uint32_t cn, uint32_t mn, int shift, int bits,
                                         const uint32_t (&k)[JN], uint32_t (&pk)[JN]) {
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint32_t mask = (1u << bits) - 1u;
#pragma unroll
  for (int j = 0; j < JN; ++j) {
    const uint32_t le = (uint32_t)(w * JN + j) * 64u + (uint32_t)lane;
    const bool valid = le < cn;
    const uint32_t d = ((k[j] - mn) >> shift) & mask;
    (void)bits;
    if (valid) atomicOr(&L.match[w][d], 1ull << lane);
    const uint64_t peers = valid ? L.match[w][d] : 0ull;
    if (valid) L.match[w][d] = 0ull;
    const int leader = __ffsll((unsigned long long)peers) - 1;
    uint32_t old = 0;
    if (valid && lane == leader) old = atomicAdd(&L.wcnt[w][d], (uint32_t)__popcll(peers));
    old = (uint32_t)__shfl((int)old, leader & 63, 64);
    const uint32_t rk = old + lanes_below(peers);
    pk[j] = (pk[j] & ((1u << kBdsPosBits) - 1u)) | (d << kBdsPosBits) | (rk << kBdsRankShift);
    __builtin_amdgcn_sched_barrier(0);  // one entry group at a time: few live registers
  }
}
__device__ __forceinline__ uint32_t bds_slot(const BdsLds& L, uint32_t pk) {
  const int w = threadIdx.x >> 6;
  const uint32_t d = bds_digit(pk);
  return L.base[d] + L.wcnt[w][d] + (pk >> kBdsRankShift);
}

// thread t (digit t): the waves' counts -> their exclusive prefix in place;
// returns the digit's total
__device__ __forceinline__ uint32_t bds_wave_prefix(BdsLds& L) {
  const int t = threadIdx.x;
  uint32_t run = 0;
  if (!bds_owns_digit()) return 0u;
#pragma unroll
  for (int q = 0; q < kBdsWaves; ++q) {
    const uint32_t x = L.wcnt[q][t];
    L.wcnt[q][t] = run;
    run += x;
  }
  return run;
}

// Scratch written by other waves of this workgroup in the previous pass: the
// workgroup barrier orders it (same CU, so the vector L1 is coherent for
// them; an agent-scope fence would write back and invalidate the whole L2).
__device__ __forceinline__ uint2 bds_load_scratch(const uint2* p) { return *p; }

// the bin's key range over the workgroup -> (min key, R = bits of the span)
__device__ __forceinline__ uint32_t bds_range(BdsLds& L, uint32_t mn, uint32_t mx, int& R) {
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    mn = min(mn, (uint32_t)__shfl_xor((int)mn, off, 64));
    mx = max(mx, (uint32_t)__shfl_xor((int)mx, off, 64));
  }
  if (lane == 0) {
    L.rng[0][w] = mn;
    L.rng[1][w] = mx;
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < kBdsWaves; ++q) {
    mn = min(mn, L.rng[0][q]);
    mx = max(mx, L.rng[1][q]);
  }
  const uint32_t span = mx - mn;
  R = span ? 32 - __clz((int)span) : 0;
  return mn;
}
__device__ __forceinline__ void bds_plan(int R, int& passes, int& pbits) {
  passes = (R + kBdsMaxBits - 1) / kBdsMaxBits;
  pbits = passes ? (R + passes - 1) / passes : 0;
}

// The LDS passes over n <= 64 JN x kBdsWaves entries: wave w owns slots
// [w JN 64, (w + 1) JN 64), JN entries per lane in registers, every pass
// ranked in LDS.  k[j]: the key of slot (w JN + j) 64 + lane (anything past
// n); on return bds_pos(pk[j]) is the input position of the entry sorted
// into that slot (anything past n).
template <int JN>
__device__ __forceinline__ void bds_passes(BdsLds& L, uint32_t (&k)[JN], uint32_t (&pk)[JN], uint32_t n) {
  const int t = threadIdx.x, w = t >> 6, lane = t & 63;
  uint32_t mn = 0xFFFFFFFFu, mx = 0u;
#pragma unroll
  for (int j = 0; j < JN; ++j) {
    const uint32_t le = (uint32_t)(w * JN + j) * 64u + (uint32_t)lane;
    pk[j] = le;
    k[j] = le < n ? k[j] : 0u;
    if (le < n) {
      mn = min(mn, k[j]);
      mx = max(mx, k[j]);
    }
  }
  int R, npass, pbits;
  mn = bds_range(L, mn, mx, R);
  bds_plan(R, npass, pbits);
  for (int p = 0; p < npass; ++p) {
    const int shift = p * pbits, bits = min(pbits, R - shift);
    bds_rank<JN>(L, n, mn, shift, bits, k, pk);
    __syncthreads();
    uint32_t all;
    const uint32_t ex = bds_excl_scan(bds_wave_prefix(L), L.tmp, &all);
    if (bds_owns_digit()) L.base[t] = ex;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < JN; ++j) {
      const uint32_t le = (uint32_t)(w * JN + j) * 64u + (uint32_t)lane;
      if (le < n) L.buf[bds_slot(L, pk[j])] = make_uint2(k[j], bds_pos(pk[j]));
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < JN; ++j) {
      const uint32_t le = (uint32_t)(w * JN + j) * 64u + (uint32_t)lane;
      if (le < n) {
        const uint2 kv = L.buf[le];
        k[j] = kv.x;
        pk[j] = kv.y;
      }
    }
#pragma unroll
    for (int q = 0; q < kBdsWaves; ++q)
      if (bds_owns_digit()) L.wcnt[q][t] = 0u;
    if (p + 1 < npass) {  // the next pass ranks with the table the buffer overwrote
      __syncthreads();
      for (int i = t; i < kBdsWaves * kBdsDigits; i += kBdsThreads) (&L.match[0][0])[i] = 0ull;
    }
    __syncthreads();
  }
}

// a bin of n <= 64 JN x kBdsWaves entries: its depth keys gathered through
// the Gaussian ids, the passes, then the per-tile lists straight from the
// sorted bin
template <int JN>
__device__ __forceinline__ void bds_small(BdsLds& L, const uint32_t* __restrict__ skeys,
                                          const uint32_t* __restrict__ sgid, const uint32_t* __restrict__ gdep,
                                          uint32_t lo, uint32_t n, const BdsEmit& EM) {
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  uint32_t k[JN], pk[JN];
  // (loads of clamped positions, all issued before any is used: a load under
  // `le < n` is waited for at its join, one round trip per j; the Gaussians'
  // depth keys through the bin's ids are two round trips)
#pragma unroll
  for (int j = 0; j < JN; ++j) k[j] = sgid[lo + min((uint32_t)(w * JN + j) * 64u + (uint32_t)lane, n - 1u)];
#pragma unroll
  for (int j = 0; j < JN; ++j) k[j] = gdep[k[j]];
  bds_passes<JN>(L, k, pk, n);
  uint32_t m[JN], g[JN];
  const uint32_t tmask = (1u << (1 << (2 * EM.bshift))) - 1u;
#pragma unroll
  for (int j = 0; j < JN; ++j) {
    const uint32_t le = (uint32_t)(w * JN + j) * 64u + (uint32_t)lane;
    const uint32_t q = le < n ? bds_pos(pk[j]) : 0u;  // (unconditional loads, as above)
    m[j] = skeys[lo + q];
    g[j] = sgid[lo + q];
  }
#pragma unroll
  for (int j = 0; j < JN; ++j) {
    const uint32_t le = (uint32_t)(w * JN + j) * 64u + (uint32_t)lane;
    m[j] = le < n ? (m[j] >> 16) & tmask : 0u;
    g[j] = le < n ? g[j] : 0u;
  }
  uint32_t run[2] = {0u, 0u};
  bds_emit_chunk<JN>(L, m, g, n, 1 << (2 * EM.bshift), EM.lists + ((size_t)lo << (2 * EM.bshift)), n, run);
}

// the same passes on keys loaded directly: perm[i] = the position of the i-th
// smallest key (k_argsort_small)
template <int JN>
__device__ __forceinline__ void bds_argsort(BdsLds& L, const uint32_t* __restrict__ keys, uint32_t n,
                                            uint32_t* __restrict__ perm) {
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  uint32_t k[JN], pk[JN];
  // (loads of clamped positions, all issued before any is used, as in bds_small)
#pragma unroll
  for (int j = 0; j < JN; ++j) k[j] = keys[min((uint32_t)(w * JN + j) * 64u + (uint32_t)lane, n - 1u)];
  bds_passes<JN>(L, k, pk, n);
#pragma unroll
  for (int j = 0; j < JN; ++j) {
    const uint32_t le = (uint32_t)(w * JN + j) * 64u + (uint32_t)lane;
    if (le < n) perm[le] = bds_pos(pk[j]);
  }
}

// the emit of a bin beyond the LDS tile: chunks of JN x kBdsThreads sorted
// positions, their bin positions from the final pass's scratch (fin; null:
// already in order), running per-tile counts across the chunks
template <int JN>
__device__ __forceinline__ void bds_emit_big(BdsLds& L, const uint32_t* __restrict__ skeys,
                                             const uint32_t* __restrict__ sgid, const uint2* fin, uint32_t lo,
                                             uint32_t n, const BdsEmit& E) {
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint32_t tmask = (1u << (1 << (2 * E.bshift))) - 1u;
  constexpr uint32_t kChunk = JN * kBdsThreads;
  uint32_t* out = E.lists + ((size_t)lo << (2 * E.bshift));
  uint32_t run[2] = {0u, 0u};
  for (uint32_t c0 = 0; c0 < n; c0 += kChunk) {
    const uint32_t cn = min(kChunk, n - c0);
    // (loads of clamped positions, every one issued before the first is used)
    uint32_t m[JN], g[JN];
#pragma unroll
    for (int j = 0; j < JN; ++j) g[j] = c0 + min((uint32_t)(w * JN + j) * 64u + (uint32_t)lane, cn - 1u);
    if (fin) {  // (uniform)
#pragma unroll
      for (int j = 0; j < JN; ++j) g[j] = bds_load_scratch(fin + g[j]).y;
    }
#pragma unroll
    for (int j = 0; j < JN; ++j) {
      m[j] = skeys[lo + g[j]];
      g[j] = sgid[lo + g[j]];
    }
#pragma unroll
    for (int j = 0; j < JN; ++j) {
      const uint32_t le = (uint32_t)(w * JN + j) * 64u + (uint32_t)lane;
      m[j] = le < cn ? (m[j] >> 16) & tmask : 0u;
      g[j] = le < cn ? g[j] : 0u;
    }
    bds_emit_chunk<JN>(L, m, g, cn, 1 << (2 * E.bshift), out, n, run);
  }
}

// a bin beyond the LDS tile: each pass counts its digits over the whole bin,
// then ranks kBdsCap-entry chunks in order with running digit bases, the
// (key, position) pairs ping-ponging through global scratch
__device__ __forceinline__ void bds_big(BdsLds& L, const uint32_t* __restrict__ skeys, const uint32_t* __restrict__ sgid,
                                     const uint32_t* __restrict__ gdep, uint32_t lo, uint32_t n, uint32_t NL,
                                     uint2* scratch, const BdsEmit& EM) {
  const int t = threadIdx.x, w = t >> 6, lane = t & 63;
  uint32_t mn = 0xFFFFFFFFu, mx = 0u;
  auto dep = [&](uint32_t e) { return gdep[sgid[lo + e]]; };
  for (uint32_t e = (uint32_t)t; e < n; e += kBdsThreads) {
    const uint32_t x = dep(e);
    mn = min(mn, x);
    mx = max(mx, x);
  }
  int R, passes, pbits;
  mn = bds_range(L, mn, mx, R);
  bds_plan(R, passes, pbits);
  constexpr int JN = 7;  // (chunks of half the LDS tile: fewer registers)
  if (passes == 0) {
    bds_emit_big<JN>(L, skeys, sgid, nullptr, lo, n, EM);
    return;
  }
  constexpr uint32_t kChunk = JN * kBdsThreads;
  uint2* bufA = scratch + lo;
  uint2* bufB = scratch + NL + lo;
  for (int p = 0; p < passes; ++p) {
    const int shift = p * pbits, bits = min(pbits, R - shift);
    const uint32_t mask = (1u << bits) - 1u;
    const uint2* src = (p & 1) ? bufA : bufB;  // pass p - 1's output
    uint2* dst = (p & 1) ? bufB : bufA;
    auto load = [&](uint32_t e) -> uint2 {
      return p == 0 ? make_uint2(dep(e), e) : bds_load_scratch(src + e);
    };
    if (bds_owns_digit()) L.base[t] = 0u;
    __syncthreads();
    for (uint32_t e = (uint32_t)t; e < n; e += kBdsThreads) atomicAdd(&L.base[((load(e).x - mn) >> shift) & mask], 1u);
    __syncthreads();
    {
      uint32_t all;
      const uint32_t c = bds_owns_digit() ? L.base[t] : 0u;
      const uint32_t ex = bds_excl_scan(c, L.tmp, &all);
      if (bds_owns_digit()) L.base[t] = ex;
    }
    __syncthreads();
    for (uint32_t c0 = 0; c0 < n; c0 += kChunk) {
      const uint32_t cn = min(kChunk, n - c0);
      uint32_t k[JN], pk[JN], pos[JN];  // (positions beyond the 13 bits of pk)
#pragma unroll
      for (int j = 0; j < JN; ++j) {
        const uint32_t le = (uint32_t)(w * JN + j) * 64u + (uint32_t)lane;
        k[j] = 0u;
        pos[j] = 0u;
        pk[j] = 0u;
        if (le < cn) {
          const uint2 kv = load(c0 + le);
          k[j] = kv.x;
          pos[j] = kv.y;
        }
      }
      bds_rank<JN>(L, cn, mn, shift, bits, k, pk);
      __syncthreads();
      const uint32_t tot = bds_wave_prefix(L);
      __syncthreads();
#pragma unroll
      for (int j = 0; j < JN; ++j) {
        const uint32_t le = (uint32_t)(w * JN + j) * 64u + (uint32_t)lane;
        if (le < cn) dst[bds_slot(L, pk[j])] = make_uint2(k[j], pos[j]);
      }
      __syncthreads();
      if (bds_owns_digit()) L.base[t] += tot;
#pragma unroll
      for (int q = 0; q < kBdsWaves; ++q)
        if (bds_owns_digit()) L.wcnt[q][t] = 0u;
      __syncthreads();
    }
    __syncthreads();
  }
  const uint2* fin = ((passes - 1) & 1) ? bufB : bufA;
  bds_emit_big<JN>(L, skeys, sgid, fin, lo, n, EM);
}

// the smallest JN that holds the bin, else the chunked passes
// (every step of JN: a bin's time is its busiest wave's chain of JN entry
// groups per pass, and a coarser JN leaves the last waves idle -- measured
// with 1024 threads: 4.7k entries at JN = 7 keep 11 of 16 waves busy, at
// JN = 5 all 15 it needs)
template <int JN = 1>
__device__ __forceinline__ void bds_sort_bin(BdsLds& L, const uint32_t* __restrict__ skeys,
                                             const uint32_t* __restrict__ sgid, const uint32_t* __restrict__ gdep,
                                             uint32_t lo, uint32_t n, uint32_t NL, uint2* scratch, const BdsEmit& EM) {
  if constexpr (JN > kBdsItems)
    bds_big(L, skeys, sgid, gdep, lo, n, NL, scratch, EM);
  else if (n <= (uint32_t)JN * kBdsThreads)
    bds_small<JN>(L, skeys, sgid, gdep, lo, n, EM);
  else
    bds_sort_bin<JN + 1>(L, skeys, sgid, gdep, lo, n, NL, scratch, EM);
}

__global__ __launch_bounds__(kBdsThreads) void k_bin_depth_sort(
    const uint32_t* __restrict__ skeys, const uint32_t* __restrict__ sgid, const uint2* __restrict__ bounds,
    const uint32_t* __restrict__ gdep, uint32_t NL, uint2* scratch, BdsEmit emit) {
  __shared__ BdsLds L;
  const int t = threadIdx.x;
  const uint32_t bin = blockIdx.x;
  const uint2 bb = bounds[bin];
  const uint32_t lo = bb.x, n = bb.y - bb.x;
  if (n == 0) {  // block-uniform
    bds_emit_ranges(L, emit, bin, lo, 0u);
    return;
  }
#pragma unroll
  for (int q = 0; q < kBdsWaves; ++q)
    if (bds_owns_digit()) L.wcnt[q][t] = 0u;  // (published by bds_range's barrier)
  for (int i = t; i < kBdsWaves * kBdsDigits; i += kBdsThreads) (&L.match[0][0])[i] = 0ull;
  bds_sort_bin(L, skeys, sgid, gdep, lo, n, NL, scratch, emit);
  bds_emit_ranges(L, emit, bin, lo, n);
}

// Stable argsort of n <= kBdsCap 32-bit keys in one workgroup: the per-bin
// depth sort's LDS passes on a single "bin" whose payload is the position
// (ties keep index order).  perm[i] = the index of the i-th smallest key.
__global__ __launch_bounds__(kBdsThreads) void k_argsort_small(const uint32_t* __restrict__ keys, uint32_t n,
                                                              uint32_t* __restrict__ perm) {
  __shared__ BdsLds L;
  const int t = threadIdx.x;
#pragma unroll
  for (int q = 0; q < kBdsWaves; ++q)
    if (bds_owns_digit()) L.wcnt[q][t] = 0u;
  for (int i = t; i < kBdsWaves * kBdsDigits; i += kBdsThreads) (&L.match[0][0])[i] = 0ull;
  if (n <= 2u * kBdsThreads)
    bds_argsort<2>(L, keys, n, perm);
  else if (n <= 4u * kBdsThreads)
    bds_argsort<4>(L, keys, n, perm);
  else
    bds_argsort<kBdsItems>(L, keys, n, perm);
}

}  // namespace

uint32_t argsort_small_max() { return (uint32_t)kBdsCap; }
hipError_t launch_argsort_small(const uint32_t* keys, uint32_t n, uint32_t* perm, hipStream_t s) {
  if (n == 0) return hipSuccess;
  if (n > (uint32_t)kBdsCap) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_argsort_small, dim3(1), dim3(kBdsThreads), 0, s, keys, n, perm);
  return hipGetLastError();
}

hipError_t launch_bin_depth_sort(const wgsr_raster_args& a, const uint32_t* sorted_keys, const uint32_t* sorted_g,
                                 uint32_t NB, int bshift, uint2* bounds, bool bounds_done, const uint32_t* gdepth,
                                 void* scratch, uint32_t* lists, uint2* ranges, uint32_t* tile_len, uint32_t* meta,
                                 hipStream_t s) {
  const int gx = (a.W + kTile - 1) / kTile, gy = (a.H + kTile - 1) / kTile;
  const Bins B(gx, gy, bshift);
  hipError_t e = make_bin_bounds(sorted_keys, NB, B.n, bounds, bounds_done, s);
  if (e != hipSuccess) return e;
  const BdsEmit emit{lists, ranges, tile_len, meta, gx, gy, bshift, B.bx};
  hipLaunchKernelGGL(k_bin_depth_sort, dim3((uint32_t)B.n), dim3(kBdsThreads), 0, s, sorted_keys, sorted_g, bounds,
                     gdepth, NB, static_cast<uint2*>(scratch), emit);
  return hipGetLastError();
}

}  // namespace wgsr
