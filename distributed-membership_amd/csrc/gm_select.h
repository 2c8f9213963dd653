// gm_select.h -- the wave-per-row rank-select helpers the pick (gm_pick.hip) and the column-shard
// draw (gm_draw.hip) share (internal to the SCALED kernels): the row's totals and chunk prefix from
// its band records, the resolution of a draw's rank to a column, the S2 outputs beyond the
// precomputed ones, and the 16-lanes-per-row helpers of gm_s_pick0 / gm_s_draw0.
#pragma once
#include "gm_device.h"
#include "gm_scaled.h"

// ------------------------------------------------------- wave-per-row helpers
// LDS per wave of the draw kernels: chunk prefix [chunks + 1] u32 (S_CHUNK(B) columns per
// chunk), the fallback generator's state [624] u32.
__host__ __device__ __forceinline__ int gm_draw_chunks(int wp, int band) { return wp / S_CHUNK(band); }  // rank-select chunks per row
__host__ __device__ __forceinline__ size_t gm_draw_lds_words(int wp, int band) {
  return (size_t)gm_draw_chunks(wp, band) + 1 + 624;
}

// Row r of this shard: numfailed (band counts), size and the chunk prefix
// pre[c] = present cells in chunks [0, c) (pre[nc] = size), from the chunk counts.
// the lane's first (band, row) record of row r (all of them when nb <= 64), as gm_row_totals reads it
__device__ __forceinline__ uint4 gm_row_rec0(const SState &s, int r, int lane) {
  const int perb = (s.nb + 63) >> 6, b0 = lane * perb;
  return b0 < s.nb ? s.brec[(size_t)b0 * s.n + r] : make_uint4(0u, 0u, 0u, 0u);
}

// pre0: the lane's first record, when the caller loaded it already (gm_row_rec0)
template <int B>
__device__ __forceinline__ void gm_row_totals(const SState &s, int r, int lane, uint32_t *pre, uint32_t &size,
                                              uint32_t &nfail, const uint4 *pre0 = nullptr) {
  constexpr int CPB = B / S_CHUNK(B);  // rank-select chunks per band
  const int nb = s.nb, perb = (nb + 63) >> 6;
  const int b0 = min(nb, lane * perb), b1 = min(nb, b0 + perb);
  uint32_t fs = 0, ps = 0;
  uint4 rec0 = make_uint4(0u, 0u, 0u, 0u);  // the lane's first (band, row) record (all of them when nb <= 64)
  for (int b = b0; b < b1; b++) {
    const uint4 rc = (b == b0 && pre0) ? *pre0 : s.brec[(size_t)b * s.n + r];
    if (b == b0) rec0 = rc;
    fs += S_BC_FAIL(rc.z);
    ps += S_BC_PRES(rc.z);
  }
  // wave sums / prefix on DPP (no LDS round trips): inclusive scans, totals from lane 63
  nfail = (uint32_t)__builtin_amdgcn_readlane(dpp_scan((int)fs), 63);
  const uint32_t x = (uint32_t)dpp_scan((int)ps);
  size = (uint32_t)__builtin_amdgcn_readlane((int)x, 63);
  if (pre) {
    uint32_t a = x - ps;
    for (int b = b0; b < b1; b++) {
      const uint2 pc = b == b0 ? make_uint2(rec0.x, rec0.y) : *(const uint2 *)&s.brec[(size_t)b * s.n + r];
      const uint64_t v = (uint64_t)pc.x | ((uint64_t)pc.y << 32);
#pragma unroll
      for (int c = 0; c < CPB; c++) {
        pre[b * CPB + c] = a;
        a += (uint32_t)(v >> (8 * c)) & 0xFFu;
      }
    }
    if (lane == 63) pre[nb * CPB] = a;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
}

// Freshness (age < TFAIL) of the escaped cell (r, col) of tick t, from its (band, row) list of
// tick t (rare: a draw landing on an escaped cell)
__device__ __forceinline__ bool esc_fresh(const SState &s, int r, int col) {
  const int b = col / s.band, c = col % s.band;
  const size_t slab = (size_t)b * s.n;
  const uint32_t w = s.brec[slab + r].w;
  // the pools of the tick just swept: its parity is that of the row's last written tick
  const EscList l = esc_list(s, s.wtick[r] & 1, slab, r, w);
  for (int i = 0; i < (int)S_EW_TOT(w); i++) {
    const uint32_t e = *l.at(i);
    if ((e & 0xFFFFu) == (uint32_t)c) return S_AGE(e >> 16) < GM_TFAIL;
  }
  return false;
}

// Resolve up to 8 draws at once, one per 8-lane group: group g holds shard-local rank
// ix_g (valid iff act) of a present entry of row r. The chunk-word prefix finds the
// 64- or 128-column chunk; its cell bytes (8 or 16 per lane) give the column. Returns, to
// every lane, the shard-local column of each draw (-1 if none) and whether it is fresh.
template <int B>
__device__ __forceinline__ void gm_resolve8(const SState &s, int r, const uint32_t *pre, bool act, uint32_t ix, int lane,
                                            int col[8], int fresh[8]) {
  constexpr int CH = S_CHUNK(B), CPL = CH / 8;  // chunk columns, cells per lane of the 8-lane group
  const int gl = lane & 7;
  int cnt = 0, base = 0;
  uint32_t en[CPL];
#pragma unroll
  for (int v = 0; v < CPL; v++) en[v] = 0;
  uint32_t q = 0;
  if (act) {
    int lo = 0, hi = s.wp / CH - 1;  // largest chunk with pre[c] <= ix (a non-empty one)
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (pre[mid] <= ix) lo = mid;
      else hi = mid - 1;
    }
    q = ix - pre[lo];
    const int col0 = lo * CH + gl * CPL;  // this lane's cells
    base = col0;
    const uint8_t *cp = s.table + ((size_t)(col0 / B) * s.n + r) * B + (col0 % B);
#pragma unroll
    for (int h = 0; h < CPL / 8; h++) {
      const uint2 t2 = *(const uint2 *)(cp + 8 * h);
#pragma unroll
      for (int v = 0; v < 8; v++) en[8 * h + v] = ((v < 4 ? t2.x : t2.y) >> (8 * (v & 3))) & 0xFFu;
    }
#pragma unroll
    for (int v = 0; v < CPL; v++) cnt += en[v] != 0;
  }
  int x = cnt;
#pragma unroll
  for (int o = 1; o < 8; o <<= 1) {
    const int y = __shfl_up(x, o, 64);
    if (gl >= o) x += y;
  }
  const int excl = x - cnt;
  int mycol = -1, myfresh = 0;
  bool holder = false;
  if (act && (int)q >= excl && (int)q < excl + cnt) {
    holder = true;
    int need = (int)q - excl;
#pragma unroll
    for (int v = 0; v < CPL; v++) {
      if (en[v] != 0) {
        if (need == 0) {
          mycol = base + v;
          // the table is as of tick t; an escaped cell's age is in its (band, row) escape list
          myfresh = s_is_esc(en[v]) ? esc_fresh(s, r, mycol) : S_AGE(s_widen(en[v])) < GM_TFAIL;
        }
        need--;
      }
    }
  }
  const uint64_t hm = __ballot(holder);
#pragma unroll
  for (int g = 0; g < 8; g++) {
    const uint32_t seg = (uint32_t)(hm >> (8 * g)) & 0xFFu;
    const int src = seg ? 8 * g + __builtin_ctz(seg) : 0;
    col[g] = seg ? __shfl(mycol, src, 64) : -1;
    fresh[g] = seg ? __shfl(myfresh, src, 64) : 0;
  }
}

// S2 outputs of a row beyond the precomputed ones: lane 0 runs the lazy generator
// (state in this wave's LDS), `skip` outputs consumed already; lane q < cnt gets output q.
__device__ __forceinline__ uint32_t gm_mt_batch(GmLazyMT &mt, uint32_t *mts, uint32_t seed, bool fresh_gen, int skip,
                                                int cnt, int lane) {
  if (lane == 0 && fresh_gen) {
    mt.seed(mts, seed);
    for (int i = 0; i < skip; i++) (void)mt.next();
  }
  uint32_t raw = 0;
  for (int q = 0; q < cnt; q++) {
    uint32_t o = 0;
    if (lane == 0) o = mt.next();
    o = __shfl(o, 0, 64);
    if (lane == q) raw = o;
  }
  return raw;
}

// 16 lanes per row (gm_s_pick0, gm_s_draw0): row16_scan is gm_device.h's, with dpp_scan
__device__ __forceinline__ int row16_bcast(int v, int g, int q) { return __shfl(v, 16 * g + q, 64); }
__device__ __forceinline__ uint32_t row16_bits(uint64_t bal, int g) { return (uint32_t)(bal >> (16 * g)) & 0xFFFFu; }

// launcher only another SCALED unit calls: the draw and delivery of a single-context tick
// (gm_s_pick0 then the rows it left, or gm_s_pick over every row; gm_pick.hip)
hipError_t gm_launch_pick(const SState &s, int t, hipStream_t st);
