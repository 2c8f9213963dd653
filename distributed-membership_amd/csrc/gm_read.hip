// gm_read.hip -- SCALED: table rows decoded on the device (gm_read_rows), the mirror of gm_load.hip's
// gm_l_encode: stored bytes plus the escape lists of the rows asked for -> absolute (hb, ts).
//
// The stored form is layout-dependent (gm_scaled.h: one byte per cell relative to wtick[r], escaped
// cells as entries of per-(band, row) lists, inline slot then striped pool); what a caller wants is
// not: hb / ts per column, -1 = absent (gm_host_read.hip decode_scaled_row). gm_read_table copies the
// whole stored state to the host and decodes there; here the rows [r0, r0 + rows) are decoded where
// they live, into a staging block `int32 hb[rows][w]` then `int32 ts[rows][w]` over the context's w
// real columns (padding columns are not written), and only that block crosses to the host.
//
//   gm_r_decode  gm_s_init's / gm_l_encode's work split -- one wave per (band, rows) unit, 16 cells per
//                lane, LPR = B / 16 lanes per row -- for every band width. Which 16 cells differs: the
//                kernel writes 8 B per byte it reads, so the mapping is chosen for the stores. Lane li
//                of a row holds the dwords li, LPR + li, 2 LPR + li, 3 LPR + li of the row's piece (four
//                4-byte loads, each contiguous over the row's lanes), i.e. four groups of 4 adjacent
//                columns, and writes each group's hb and ts as one 16-byte store: every store
//                instruction of a row's lanes covers one contiguous run of 16 LPR bytes (1 KiB per wave
//                at B = 1024). Where w is no multiple of 4 the rows are not 16-byte aligned and the
//                cells are stored one by one. Plain stores: the staging block is read back by the
//                copy engine at once, and non-temporal stores cost 5 - 8x the kernel's time here
//                (profiles/read_rows/README.md has the four variants measured).
//                Per cell: 0 -> (-1, -1); a byte -> s_widen; an escape code -> the cell's entry of the
//                (band, row) list; then hb = 2 wt - 255 + S_H(e) - s_hbase(column), ts = wt - S_AGE(e)
//                with wt = wtick[r] (a crashed row carries the tick it last ran).
//                Escape lists are read entry-parallel: the row's lanes park their cells in the wave's
//                LDS image of the row (column order, an escape byte as GM_RD_PENDING), one entry per
//                lane is scattered into it by its column, and the lanes take their cells back. A row
//                piece without an escape byte -- the steady state -- touches neither its record, the
//                lists nor LDS.
//                Nothing of a list is trusted before it is checked, as place_esc_list (gm_host_read.hip)
//                checks it on the host: the piece's count of escape bytes equals the
//                record's S_EW_TOT, the pool extent lies inside the stripe's region, every entry's
//                column is < B and names an escape byte -- one still open, so an entry naming a cell
//                twice, and with it the escape byte left without an entry (which the host decoder
//                would fill with a stale value), is caught as well. Otherwise GM_RD_ESTATE is set
//                in the status word (-> GM_ESTATE); a list whose extent is wrong is not read.
// The kernel writes the staging block and the status word only: nothing a tick reads.
#include <hip/hip_runtime.h>

#include "gm_abi.h"
#include "gm_scaled.h"

#define GM_RD_ESTATE 1u  // status word: a row's escape list disagrees with its cells (-> GM_ESTATE)
// LDS of one wave: its rows' 16-bit cells in column order (as the band kernel's)
#define GM_RD_WAVE_WORDS S_LDS_WAVE_WORDS
#define GM_RD_PENDING 0xFFFFu  // an escape byte whose entry has not arrived; no cell: h <= 255, age <= 31

// rows [r0, r0 + rows) of the table, lists of parity par; stage = hb [rows][s.w], ts [rows][s.w]
template <int B>
__global__ __launch_bounds__(256) void gm_r_decode(SState s, int par, int r0, int rows, int32_t *stage,
                                                   uint32_t *status) {
  constexpr int LPR = B / S_COLS_PER_LANE, RPW = 64 / LPR, Q = S_COLS_PER_LANE;
  const int U = (rows + RPW - 1) / RPW;
  const int ub = __builtin_amdgcn_readfirstlane((int)blockIdx.x * 4 + (int)(threadIdx.x >> 6));
  if (ub >= U) return;  // whole wave
  __shared__ __attribute__((aligned(16))) uint32_t lds_all[4 * GM_RD_WAVE_WORDS];  // escaped rows only
  uint32_t *lds = lds_all + (threadIdx.x >> 6) * GM_RD_WAVE_WORDS;
  const int lane = threadIdx.x & 63, sub = lane / LPR, li = lane % LPR;
  const int band = blockIdx.y, i = ub * RPW + sub;
  const bool valid = i < rows;  // row-uniform; the rows past the block stay in the wave (no cells, no escapes)
  const int r = r0 + i;
  const size_t slab = (size_t)band * s.n;
  // lane li of the row holds dwords li, LPR + li, 2 LPR + li, 3 LPR + li of the piece: cell q = 4 k + j is
  // column 4 (k LPR + li) + j, so each load and each store of the row's lanes is one contiguous run
  uint32_t tw[4] = {0u, 0u, 0u, 0u};
  if (valid) {
    const uint32_t *piece = (const uint32_t *)(s.table + (slab + (size_t)r) * B);
#pragma unroll
    for (int k = 0; k < 4; k++) tw[k] = __builtin_nontemporal_load(piece + k * LPR + li);
  }
  uint32_t cell[Q];  // the lane's 16-bit cells; GM_RD_PENDING: an escape byte whose entry has not arrived
  bool esc_any = false;
#pragma unroll
  for (int q = 0; q < Q; q++) {
    const uint32_t x = (tw[q >> 2] >> (8 * (q & 3))) & 0xFFu;
    const bool esc = s_is_esc(x);
    cell[q] = esc ? GM_RD_PENDING : s_widen(x);
    esc_any |= esc;
  }
  if (__builtin_amdgcn_ballot_w64(esc_any) != 0) {  // wave-uniform: some row of this wave has escapes
    int nesc = 0;
#pragma unroll
    for (int q = 0; q < Q; q++) nesc += cell[q] == GM_RD_PENDING;
    int k;  // escape bytes of the row's piece (row-uniform)
    row_scan<LPR>(nesc, li, lane, k);
    u32x2 *rowv = (u32x2 *)(lds + (lane - li) * 8);  // the row's B cells in column order, 4 per u32x2
    bool bad = false;
    if (k > 0) {
#pragma unroll
      for (int g = 0; g < 4; g++)
        rowv[g * LPR + li] = (u32x2){cell[4 * g] | cell[4 * g + 1] << 16, cell[4 * g + 2] | cell[4 * g + 3] << 16};
    }
    lds_wave_sync();
    if (k > 0) {
      const uint32_t word = s.brec[slab + (size_t)r].w;
      const int in = min(k, S_ESC_IN);
      // the list's extent before anything of it is read
      if ((int)S_EW_TOT(word) != k || S_EW_OFF(word) + (uint32_t)(k - in) > s.tesc_region) {
        bad = true;
      } else {
        const EscList l = esc_list(s, par, slab, r, word);
        uint16_t *row = (uint16_t *)rowv;
        for (int j = li; j < k; j += LPR) {  // one entry per lane
          const uint32_t e = *l.at(j);
          const uint32_t col = e & 0xFFFFu;
          if (col >= (uint32_t)B || row[col] != GM_RD_PENDING) {  // an entry for a cell that is no (open) escape
            bad = true;
            continue;
          }
          row[col] = (uint16_t)(e >> 16);
        }
      }
    }
    lds_wave_sync();
    if (k > 0) {
#pragma unroll
      for (int g = 0; g < 4; g++) {
        const u32x2 v = rowv[g * LPR + li];
        cell[4 * g] = v.x & 0xFFFFu;
        cell[4 * g + 1] = v.x >> 16;
        cell[4 * g + 2] = v.y & 0xFFFFu;
        cell[4 * g + 3] = v.y >> 16;
      }
#pragma unroll
      for (int q = 0; q < Q; q++) {
        if (cell[q] == GM_RD_PENDING) {  // an escape byte no entry named (k entries, one of them twice)
          bad = true;
          cell[q] = 0;
        }
      }
    }
    if (bad) atomicOr(status, GM_RD_ESTATE);
  }
  if (!valid) return;
  const int wt = s.wtick[r];
  int32_t *hrow = stage + (size_t)i * s.w, *trow = hrow + (size_t)rows * s.w;
#pragma unroll
  for (int g = 0; g < 4; g++) {
    const int jc = band * B + 4 * (g * LPR + li);  // shard-local column of the group's first cell
    if (jc >= s.w) continue;                       // padding columns are not written
    int32_t h[4], a[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const uint32_t e = cell[4 * g + j];
      h[j] = e == 0 ? -1 : 2 * wt - 255 + (int32_t)S_H(e) - s_hbase(s.ramp, s.c0 + jc + j);
      a[j] = e == 0 ? -1 : wt - (int32_t)S_AGE(e);
    }
    if ((s.w & 3) == 0) {  // rows are 16-byte aligned and jc + 4 <= w
      const i32x4 hv = {h[0], h[1], h[2], h[3]}, av = {a[0], a[1], a[2], a[3]};
      *(i32x4 *)(hrow + jc) = hv;
      *(i32x4 *)(trow + jc) = av;
    } else {
#pragma unroll
      for (int j = 0; j < 4; j++) {
        if (jc + j < s.w) {
          hrow[jc + j] = h[j];
          trow[jc + j] = a[j];
        }
      }
    }
  }
}

// ------------------------------------------------------------ launch wrapper
template <int B>
static void launch_decode_b(const SState &s, int par, int r0, int rows, int32_t *stage, uint32_t *status,
                            hipStream_t st) {
  constexpr int RPW = 64 / (B / S_COLS_PER_LANE);
  const dim3 nblk((((rows + RPW - 1) / RPW) + 3) / 4, s.nb);
  hipLaunchKernelGGL(gm_r_decode<B>, nblk, dim3(256), 0, st, s, par, r0, rows, stage, status);
}

// stage: int32 [2][rows][s.w] (16-byte aligned); status zeroed on st before; 0 < rows, r0 + rows <= s.n
hipError_t gm_launch_read_decode(const SState &s, int par, int r0, int rows, int32_t *stage, uint32_t *status,
                                 hipStream_t st) {
  if (rows <= 0 || r0 < 0 || r0 + (int64_t)rows > s.n) return hipErrorInvalidValue;
  return gm_band_dispatch(s.band, [&](auto b) {
    launch_decode_b<decltype(b)::value>(s, par, r0, rows, stage, status, st);
    return hipGetLastError();
  });
}
