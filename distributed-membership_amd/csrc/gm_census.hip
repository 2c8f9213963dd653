// gm_census.hip -- SCALED membership census (gm_census): what the cluster believes at tick T.
//
// A column reduction of the stored table over the live observers: per subject column one
// gm_census_rec (holders, stale entries, heartbeat / timestamp range and sums) and, over all of this
// context's columns, the joint histogram of (subject's crash flag, heartbeat lag, age). The table
// stays on the device; O(w) bytes plus the histogram go back (gm_host_read.hip gm_census). Nothing the
// tick kernels read is written: the reducer's only outputs are its own scratch.
//
// Every live row is relative to the same tick T (wtick[r] == T), so both passes accumulate in cell
// units (h, age) and convert once per column at the flush: hb = 2T - 255 + h - s_hbase(column),
// ts = T - age (gm_host_read.hip decode_scaled_row). A live row holding cells relative to another tick
// sets GM_CEN_ESTATE.
//
//   gm_c_bytes  the stored bytes. A workgroup takes one band and a run of rows; a lane owns 4
//               adjacent columns (one dword per row), GM_CEN_UNROLL rows in flight per lane. The per-column accumulators
//               stay in registers and are flushed once per workgroup. The histogram is counted in
//               LDS: a steady cluster puts almost every cell into a few dozen bins, so the bins are
//               replicated (8 copies, 2 on a join ramp whose lags need all 64 bins) and a lane adds
//               to copy lane % copies -- the copies of a bin are adjacent words, i.e. distinct banks.
//               Escape bytes hold no value; they are counted per row and compared with the row's
//               list word (the host decoder's check).
//   gm_c_esc    the escape lists of parity T & 1, 16 lanes per (band, row) list (its inline slot is
//               one 64-byte line), one entry per lane. Entries are aggregated per column in LDS over
//               the (band, row run) tile before anything global is touched: on a cold start every
//               cell is an entry (gm_scaled.h on the escape pool's single counter). The histogram
//               adds are combined per wave by value first (few distinct bins per wave).
//   gm_c_final  the scratch encodings of min / max -> -1 = none.
//
// Scratch encodings (the scratch is zeroed by a fill): a minimum v is kept as ~v under an unsigned
// max, a maximum as v + 1; 0 = no entry either way (gm_s_detect lets -1 lose an unsigned min; a
// zero fill cannot write that -1 next to counters that start at 0).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "gm_abi.h"
#include "gm_scaled.h"

#define GM_CEN_RUN_MAX 4096  // rows of one band per workgroup, at most
#define GM_CEN_RUN_MIN 256
#define GM_CEN_BMAX 1024     // widest band
#define GM_CEN_HWORDS 4096   // LDS words of gm_c_bytes' histogram copies
#define GM_CEN_UNROLL 8      // rows a lane has in flight
#define GM_CEN_ESTATE 1u     // status word: the stored state is inconsistent (-> GM_ESTATE)
#define GM_CEN_ROW_LIVE 1u   // row state: live, relative to T
#define GM_CEN_ROW_OFF 2u    // live, relative to another tick: may hold nothing

static_assert(GM_CENSUS_AGES == 32 && GM_CENSUS_LAGS == 64, "bin packing of the histograms");
static_assert(sizeof(gm_census_rec) == 40, "gm_census_rec layout");

// one column's share of a tile -> its record (cell units in, absolute values out); n > 0
__device__ __forceinline__ void cen_flush(gm_census_rec *d, uint32_t n, uint32_t stale, uint32_t hsum, uint32_t asum,
                                          uint32_t hmin, uint32_t hmax, uint32_t amin, uint32_t amax, int T,
                                          int hbase) {
  const int hb0 = 2 * T - 255 - hbase;
  atomicAdd(&d->holders, n);
  if (stale) atomicAdd(&d->stale, stale);
  atomicAdd((unsigned long long *)&d->hb_sum, (unsigned long long)((long long)n * hb0 + (long long)hsum));
  atomicAdd((unsigned long long *)&d->ts_sum, (unsigned long long)((long long)n * T - (long long)asum));
  atomicMax((unsigned int *)&d->hb_min, ~(uint32_t)(hb0 + (int)hmin));
  atomicMax((unsigned int *)&d->hb_max, (uint32_t)(hb0 + (int)hmax) + 1u);
  atomicMax((unsigned int *)&d->ts_min, ~(uint32_t)(T - (int)amax));
  atomicMax((unsigned int *)&d->ts_max, (uint32_t)(T - (int)amin) + 1u);
}

// Grid (ceil(n / rrun), nb). lagbits: lag bins kept in LDS = 1 << lagbits (4: a stored byte lags at
// most 14 ticks; 6 on a join ramp, whose columns add s_hbase / 2).
__global__ __launch_bounds__(256) void gm_c_bytes(SState s, gm_census_rec *rec, unsigned long long *hist,
                                                  uint32_t *status, int T, int rrun, int lagbits) {
  __shared__ uint32_t lh[GM_CEN_HWORDS];      // [class << lagbits | lag][age 0..15][copy]
  __shared__ uint32_t rowst[GM_CEN_RUN_MAX];  // row state << 30 | escape bytes of the row's slice
  const int tid = threadIdx.x;
  const int b = blockIdx.y, r0 = blockIdx.x * rrun, rows = min(rrun, s.n - r0);
  const int B = s.band, lpr = B >> 2, rs = 256 / lpr;  // lanes per row, rows per step
  const int cg = tid & (lpr - 1), sub = tid / lpr;
  const int colb = b * B + 4 * cg;  // shard-local column of this lane's first cell
  const size_t slab = (size_t)b * s.n;
  const int bins = 2 << (lagbits + 4), copies = GM_CEN_HWORDS / bins, copy = tid & (copies - 1);
  const int lagmax = (1 << lagbits) - 1;
  uint32_t cls[4], hbh[4];  // the subject's class, s_hbase / 2
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const int lc = colb + q;
    cls[q] = lc < s.w && s.failed[s.c0 + lc] != 0 ? 1u : 0u;
    hbh[q] = (uint32_t)s_hbase(s.ramp, s.c0 + lc) >> 1;
  }
  for (int i = tid; i < GM_CEN_HWORDS; i += 256) lh[i] = 0;
  for (int i = tid; i < rows; i += 256)
    rowst[i] = s.failed[r0 + i] ? 0u : (s.wtick[r0 + i] == T ? GM_CEN_ROW_LIVE : GM_CEN_ROW_OFF) << 30;
  __syncthreads();
  uint32_t cn[4] = {0, 0, 0, 0}, cst[4] = {0, 0, 0, 0}, chs[4] = {0, 0, 0, 0}, cas[4] = {0, 0, 0, 0};
  uint32_t chmin[4] = {15, 15, 15, 15}, chmax[4] = {0, 0, 0, 0}, camin[4] = {15, 15, 15, 15}, camax[4] = {0, 0, 0, 0};
  bool bad = false;
  const uint8_t *src = s.table + (slab + r0) * B + 4 * cg;
  for (int i0 = sub; i0 < rows; i0 += GM_CEN_UNROLL * rs) {
    uint32_t w[GM_CEN_UNROLL], st[GM_CEN_UNROLL];
#pragma unroll
    for (int u = 0; u < GM_CEN_UNROLL; u++) {  // crashed rows are skipped before their cells are loaded
      const int i = i0 + u * rs;
      st[u] = i < rows ? rowst[i] >> 30 : 0u;
      w[u] = st[u] ? __builtin_nontemporal_load((const uint32_t *)(src + (size_t)i * B)) : 0u;
    }
#pragma unroll
    for (int u = 0; u < GM_CEN_UNROLL; u++) {
      if (!w[u]) continue;
      if (st[u] != GM_CEN_ROW_LIVE) {  // cells relative to another tick in a live row
        bad = true;
        continue;
      }
      uint32_t nesc = 0;
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const uint32_t x = (w[u] >> (8 * q)) & 0xFFu;
        if (x >= 16) {  // h = 224 + 2 h4, age a (s_widen)
          const uint32_t h4 = x >> 4, a = x & 15u;
          cn[q]++;
          cst[q] += a >= GM_TFAIL;
          chs[q] += h4;
          cas[q] += a;
          chmin[q] = min(chmin[q], h4);
          chmax[q] = max(chmax[q], h4);
          camin[q] = min(camin[q], a);
          camax[q] = max(camax[q], a);
          const uint32_t lag = min(15u - h4 + hbh[q], (uint32_t)lagmax);  // (255 - h + hbase) >> 1
          atomicAdd(&lh[((((cls[q] << lagbits) | lag) << 4) | a) * copies + copy], 1u);
        } else if (x) {
          nesc++;
        }
      }
      if (nesc) atomicAdd(&rowst[i0 + u * rs], nesc);
    }
  }
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const int lc = colb + q;
    if (cn[q] && lc < s.w)
      cen_flush(rec + lc, cn[q], cst[q], 224u * cn[q] + 2u * chs[q], cas[q], 224u + 2u * chmin[q], 224u + 2u * chmax[q],
                camin[q], camax[q], T, 2 * (int)hbh[q]);
  }
  __syncthreads();
  // a live row's escape bytes against its list word, as the host decoder checks them
  for (int i = tid; i < rows; i += 256) {
    const uint32_t v = rowst[i];
    if ((v >> 30) == GM_CEN_ROW_LIVE && S_EW_TOT(s.brec[slab + r0 + i].w) != (v & 0x3FFFFFFFu)) bad = true;
  }
  if (bad) atomicOr(status, GM_CEN_ESTATE);
  for (int i = tid; i < bins; i += 256) {
    uint32_t v = 0;
    for (int k = 0; k < copies; k++) v += lh[i * copies + k];
    if (!v) continue;
    const int a = i & 15, lag = (i >> 4) & lagmax, c = i >> (4 + lagbits);
    atomicAdd(hist + ((size_t)c * GM_CENSUS_LAGS + lag) * GM_CENSUS_AGES + a, (unsigned long long)v);
  }
}

// Grid (ceil(n / rrun), nb): the escape lists of the tile's live rows.
__global__ __launch_bounds__(256) void gm_c_esc(SState s, gm_census_rec *rec, unsigned long long *hist,
                                                uint32_t *status, int T, int rrun) {
  __shared__ uint32_t lh[2 * GM_CENSUS_LAGS * GM_CENSUS_AGES];
  __shared__ uint32_t cns[GM_CEN_BMAX];  // per column of the band: entries | stale << 16 (rrun < 65536)
  __shared__ uint32_t chs[GM_CEN_BMAX], cas[GM_CEN_BMAX];
  __shared__ uint32_t chmin[GM_CEN_BMAX], chmax[GM_CEN_BMAX], camin[GM_CEN_BMAX], camax[GM_CEN_BMAX];
  const int tid = threadIdx.x;
  const int b = blockIdx.y, r0 = blockIdx.x * rrun, rows = min(rrun, s.n - r0);
  const int B = s.band, par = T & 1;
  const size_t slab = (size_t)b * s.n;
  uint32_t any = 0;
  for (int i = tid; i < rows; i += 256)
    if (!s.failed[r0 + i]) any |= S_EW_TOT(s.brec[slab + r0 + i].w);
  if (!__syncthreads_or(any != 0)) return;  // the steady tick: no list in these rows
  for (int i = tid; i < 2 * GM_CENSUS_LAGS * GM_CENSUS_AGES; i += 256) lh[i] = 0;
  for (int i = tid; i < B; i += 256) {
    cns[i] = chs[i] = cas[i] = chmax[i] = camax[i] = 0;
    chmin[i] = camin[i] = 0xFFFFFFFFu;
  }
  __syncthreads();
  bool bad = false;
  const int li = tid & 15;
  for (int i = tid >> 4; i < rows; i += 16) {
    const int r = r0 + i;
    if (s.failed[r]) continue;
    const uint32_t w = s.brec[slab + r].w;
    const int tot = (int)S_EW_TOT(w);
    if (!tot) continue;
    // the list's extent before anything of it is read (gm_c_bytes compares tot with the row's bytes)
    if (s.wtick[r] != T || tot > B || (tot > S_ESC_IN && S_EW_OFF(w) + (uint32_t)(tot - S_ESC_IN) > s.tesc_region)) {
      bad = true;
      continue;
    }
    const EscList l = esc_list(s, par, slab, r, w);
    const uint8_t *cells = s.table + (slab + r) * B;
    for (int j = li; j < tot; j += 16) {
      const uint32_t e = *l.at(j);
      const uint32_t col = e & 0xFFFFu, cell = e >> 16;
      if (col >= (uint32_t)B || !s_is_esc(cells[col])) {  // an entry for a cell that is no escape
        bad = true;
        continue;
      }
      const int lc = b * B + (int)col;
      if (!cell || lc >= s.w) continue;  // absent
      const uint32_t h = S_H(cell), a = S_AGE(cell);
      atomicAdd(&cns[col], 1u + ((a >= GM_TFAIL ? 1u : 0u) << 16));
      atomicAdd(&chs[col], h);
      atomicAdd(&cas[col], a);
      atomicMin(&chmin[col], h);
      atomicMax(&chmax[col], h);
      atomicMin(&camin[col], a);
      atomicMax(&camax[col], a);
      const uint32_t lag = min((255u - h + (uint32_t)s_hbase(s.ramp, s.c0 + lc)) >> 1, (uint32_t)(GM_CENSUS_LAGS - 1));
      const uint32_t bin = (((s.failed[s.c0 + lc] ? 1u : 0u) * GM_CENSUS_LAGS + lag) * GM_CENSUS_AGES) + a;
      // one add per distinct bin among the wave's active lanes
      for (bool done = false; !done;) {
        const uint32_t v = __builtin_amdgcn_readfirstlane(bin);
        const uint64_t m = __builtin_amdgcn_ballot_w64(bin == v);
        if (bin == v) {
          if ((tid & 63) == __builtin_ctzll(m)) atomicAdd(&lh[v], (uint32_t)__builtin_popcountll(m));
          done = true;
        }
      }
    }
  }
  if (bad) atomicOr(status, GM_CEN_ESTATE);
  __syncthreads();
  for (int col = tid; col < B; col += 256) {
    const uint32_t v = cns[col];
    const int lc = b * B + col;
    if (!v || lc >= s.w) continue;
    cen_flush(rec + lc, v & 0xFFFFu, v >> 16, chs[col], cas[col], chmin[col], chmax[col], camin[col], camax[col], T,
              s_hbase(s.ramp, s.c0 + lc));
  }
  for (int i = tid; i < 2 * GM_CENSUS_LAGS * GM_CENSUS_AGES; i += 256)
    if (lh[i]) atomicAdd(hist + i, (unsigned long long)lh[i]);
}

__global__ __launch_bounds__(256) void gm_c_final(gm_census_rec *rec, int w) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= w) return;
  gm_census_rec d = rec[j];
  d.hb_min = d.hb_min ? (int32_t)~(uint32_t)d.hb_min : -1;
  d.ts_min = d.ts_min ? (int32_t)~(uint32_t)d.ts_min : -1;
  d.hb_max -= 1;
  d.ts_max -= 1;
  rec[j] = d;
}

// rec [s.w], hist [2][GM_CENSUS_LAGS][GM_CENSUS_AGES] and status zeroed on st before
hipError_t gm_launch_census(const SState &s, gm_census_rec *rec, uint64_t *hist, uint32_t *status, int T,
                            hipStream_t st) {
  if (s.band < 64 || s.band > GM_CEN_BMAX || (s.band & (s.band - 1))) return hipErrorInvalidValue;
  // rows per workgroup: long runs (one flush per column and workgroup), yet about 1024 workgroups at scale
  const int64_t want = ((int64_t)s.n * s.nb + 1023) / 1024;
  const int rrun = (int)std::min<int64_t>(GM_CEN_RUN_MAX, std::max<int64_t>(GM_CEN_RUN_MIN, want));
  const dim3 grid((s.n + rrun - 1) / rrun, s.nb);
  hipLaunchKernelGGL(gm_c_bytes, grid, dim3(256), 0, st, s, rec, (unsigned long long *)hist, status, T, rrun,
                     s.ramp ? 6 : 4);
  hipLaunchKernelGGL(gm_c_esc, grid, dim3(256), 0, st, s, rec, (unsigned long long *)hist, status, T, rrun);
  hipLaunchKernelGGL(gm_c_final, dim3((s.w + 255) / 256), dim3(256), 0, st, rec, s.w);
  return hipGetLastError();
}
