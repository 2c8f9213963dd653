// gm_draw.hip -- the column-shard draw protocol: after the band kernels of the shard's columns,
// gm_s_xrows (the shard's per-row totals for the all-gather), gm_s_draw0 / gm_s_draw (every rank
// replays every pending row's S2 stream and resolves the draws landing in its own columns),
// gm_s_accept (the acceptance loop, identical on every rank) and gm_s_plist_sort (the pending rows
// of a bounded round, in the same order on every rank).
#include "gm_select.h"

#include <stdlib.h>

// ---------------------------------------------------------- column-sharded mode
// Phase A (gm_s_band, sharded): merge / sweep of this shard's columns; each row's
// shard totals (present, numfailed) accumulate into xcnt[rank] for the all-gather.

// gm_shard_stub (diagnostics): a draw landing in a peer's columns resolves to a fresh target spread
// evenly over the whole cluster -- rank ix of the row's `size` present entries stands for column
// ix * n / size. (Round 5 took column ix % n: the top ~1 % of the rows never received a list, their
// cells aged into escapes and removals, and the shard's band kernels grew ~25 % slower tick by tick.)
__device__ __forceinline__ int32_t stub_target(uint32_t ix, uint32_t size, int n) {
  return (int32_t)(((uint64_t)ix * (uint32_t)n / max(size, 1u)) << 1) | 1;
}
// rows in pending list l this tick: its append count, or 0 when the appends overflowed its
// capacity (gm_s_plist_sort: such a list is void on every rank)
__device__ __forceinline__ int plist_len(const SState &s, int l) {
  const uint32_t c = *s.plist_cnt[l];
  return c > (uint32_t)s.plist_cap[l] ? 0 : (int)c;
}

// Phase A': this shard's per-row totals (present, numfailed) for the all-gather, summed over the
// row's band records (thread per row of [r0, r1): a wave reads 1 KB per band, coalesced) -- not a
// device-scope atomic per (row, band) inside the band kernel. The ramp's self-append flag, set by
// the band kernel, is kept.
__global__ __launch_bounds__(256) void gm_s_xrows(SState s, int r0, int r1) {
  const int r = r0 + (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (r >= r1) return;
  uint32_t p = 0, f = 0;
  for (int b = 0; b < s.nb; b++) {
    const uint32_t z = s.brec[(size_t)b * s.n + r].z;
    p += S_BC_PRES(z);
    f += S_BC_FAIL(z);
  }
  int32_t *x = s.xcnt + S_XC(s, s.shard_rank, r);
  // the join ramp's self-append flag (set by the band kernel, in a slot zeroed before it) is kept;
  // without the ramp the slot is written whole, so the tick needs no fill of xcnt
  x[0] = (s.ramp ? (int32_t)((uint32_t)x[0] & S_XC_SELFAPP) : 0) | (int32_t)p;
  x[1] = (int32_t)f;
}

hipError_t gm_launch_xrows(const SState &s, int r0, int r1, hipStream_t st) {
  if (r1 > r0) hipLaunchKernelGGL(gm_s_xrows, dim3((r1 - r0 + 255) / 256), dim3(256), 0, st, s, r0, r1);
  return hipGetLastError();
}

// Phase B, round 0, four rows per wave (16 lanes per row: lane q of a row holds S2 output q, the
// counts of rank q, this shard's bands [q * perb, +perb)). Same results as gm_s_draw's round 0 with
// a fraction of its instructions: per row the 16 Lemire draws, the rank range of this shard's
// entries, a band prefix in LDS, and for each draw landing in this shard's columns a 16-ary search
// of the bands, the band record's 8 chunk counts and one 128-cell chunk read by the row's 16 lanes
// (8 bytes each, SWAR counts, a DPP prefix). Not for the join ramp (gm_s_draw handles it); needs
// G <= 16 ranks and B = 1024 (8 rank-select chunks per band).
template <int B>
__global__ __launch_bounds__(256) void gm_s_draw0(SState s, int t, int r0, int r1) {
  static_assert(B == 1024, "8 rank-select chunks of 128 columns per band");
  extern __shared__ __align__(16) uint32_t p_smem[];
  const int lane = threadIdx.x & 63, g = lane >> 4, q = lane & 15;
  const int slot = (int)(threadIdx.x >> 4);  // row slot of the workgroup (0..15)
  const int r = r0 + (int)blockIdx.x * 16 + slot;
  const bool valid = r < r1;
  const int rc = valid ? r : r1 - 1;
  const int G = s.shard_count, nb = s.nb, perb = (nb + 15) >> 4, par = t & 1;
  uint32_t *bpre = p_smem + (size_t)slot * (nb + 1);  // band prefix of this shard's present cells
  // every load of the row at once
  const int failed = s.failed[rc], kin = s.inbox_cnt[par][rc];
  const uint32_t raw = s.mtraw[(size_t)rc * S_MT_RAW + q];
  const int xp = q < G ? s.xcnt[S_XC(s, q, rc)] & S_XC_COUNT : 0;
  const int xf = q < G ? s.xcnt[S_XC(s, q, rc) + 1] : 0;
  uint32_t bsum = 0;
  for (int k = 0; k < perb; k++) {
    const int b = q * perb + k;
    if (b < nb) bsum += S_BC_PRES(s.brec[(size_t)b * s.n + rc].z);
  }
  // row sums over the 16 lanes: size, numfailed, this shard's rank range [own_lo, own_lo + own_cnt)
  const int xpi = row16_scan(xp), xfi = row16_scan(xf), bi = row16_scan((int)bsum);
  const uint32_t size = (uint32_t)row16_bcast(xpi, g, 15);
  const int nf = row16_bcast(xfi, g, 15);
  const uint32_t own_lo = s.shard_rank > 0 ? (uint32_t)row16_bcast(xpi, g, s.shard_rank - 1) : 0u;
  const uint32_t own_cnt = (uint32_t)row16_bcast(xp, g, s.shard_rank);
  const int numpot = (int)size - 1 - nf;
  const bool live = valid && !failed;
  const bool pend = live && numpot > 0;
  if (valid && q == 0) {
    int32_t *acc = s.acc + (size_t)r * 8;
    acc[0] = 0;
    acc[6] = numpot;
    acc[7] = (int)size;
    s.pending[r] = pend;
    int32_t *stat = s.rowstat + (size_t)r * 4;
    stat[0] = live ? kin : 0;  // lists delivered this tick; consumed by gm_s_band, the append target of tick t+2
    stat[1] = live ? (int)size : 0;
    stat[2] = live ? nf : 0;
    stat[3] = 0;
    s.inbox_cnt[par][r] = 0;
  }
  // band prefix (exclusive) of this shard's row, in LDS
  {
    uint32_t a = (uint32_t)bi - bsum;
    for (int k = 0; k < perb; k++) {
      const int b = q * perb + k;
      if (b < nb) {
        bpre[b] = a;
        a += S_BC_PRES(s.brec[(size_t)b * s.n + rc].z);
      }
    }
    if (q == 15) bpre[nb] = (uint32_t)bi;
  }
  // Lemire on output q (uniform_int_distribution, MP1Node.cpp:466): rejection threshold 2^32 mod size
  const uint32_t sz = pend ? size : 1u;
  const uint32_t thr = (0u - sz) % sz;
  const uint64_t prod = (uint64_t)raw * sz;
  const bool ok = pend && (uint32_t)prod >= thr;
  const uint32_t ix = (uint32_t)(prod >> 32);
  const bool mine = ok && ix >= own_lo && ix < own_lo + own_cnt;
  int32_t *st = s.status + (size_t)rc * S_MT_RAW;  // round 0: D = the 16 precomputed outputs
  if (pend && !mine) st[q] = ok ? (s.stub ? stub_target(ix, size, s.n) : -1) : -2;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  uint32_t mm = row16_bits(__ballot(mine), g);  // this row's draws to resolve here
  const uint64_t any = __ballot(mm != 0);
  if (!any) return;
  const int me = r;
  int32_t myst = -1;  // status of this lane's draw (output q), when it lands in this shard's columns
  // up to DB of the row's draws per pass (a row has ~16/G in this shard's columns): their band
  // searches, then their band records' loads, then their chunk loads, each batch in flight together
  constexpr int DB = 4;
  while (__ballot(mm != 0)) {
    bool act[DB];
    int dj[DB], band[DB];
    uint32_t rem[DB];
#pragma unroll
    for (int j = 0; j < DB; j++) {
      act[j] = mm != 0;
      dj[j] = act[j] ? __builtin_ctz(mm) : 0;
      mm &= mm - 1;
      const uint32_t x = (uint32_t)row16_bcast((int)ix, g, dj[j]) - own_lo;  // rank among this shard's entries
      // 16-ary search: the band b with bpre[b] <= x < bpre[b + 1]
      int lo = 0, span = nb;
      while (__ballot(act[j] && span > 1)) {
        const int step = (span + 15) >> 4;
        const int idx = lo + q * step;
        const bool le = act[j] && q * step < span && bpre[idx] <= x;
        const int c = __builtin_popcount(row16_bits(__ballot(le), g));
        if (act[j] && span > 1) {
          lo += (max(c, 1) - 1) * step;
          span = min(step, span - (max(c, 1) - 1) * step);
        }
      }
      band[j] = lo;
      rem[j] = act[j] ? x - bpre[lo] : 0u;  // rank inside the band
    }
    // the band records' 8 chunk counts, then the chunks (128 cells: 8 bytes per lane of the row)
    uint4 rec[DB];
#pragma unroll
    for (int j = 0; j < DB; j++)
      rec[j] = act[j] ? s.brec[(size_t)band[j] * s.n + rc] : make_uint4(0u, 0u, 0u, 0u);
    int ch[DB];
    uint2 w[DB];
#pragma unroll
    for (int j = 0; j < DB; j++) {
      const uint64_t cc = (uint64_t)rec[j].x | ((uint64_t)rec[j].y << 32);
      ch[j] = 0;
#pragma unroll
      for (int k = 0; k < 7; k++) {
        const uint32_t c8 = (uint32_t)(cc >> (8 * ch[j])) & 0xFFu;
        if (rem[j] >= c8 && ch[j] == k) {
          rem[j] -= c8;
          ch[j]++;
        }
      }
      w[j] = make_uint2(0u, 0u);
      if (act[j]) w[j] = *(const uint2 *)(s.table + ((size_t)band[j] * s.n + rc) * B + ch[j] * 128 + q * 8);
    }
#pragma unroll
    for (int j = 0; j < DB; j++) {
      // present (non-zero) bytes of the lane's 8 cells
      auto nzb = [](uint32_t v) { return (v | (v >> 1) | (v >> 2) | (v >> 3) | (v >> 4) | (v >> 5) | (v >> 6) | (v >> 7)) & 0x01010101u; };
      const uint32_t m0 = nzb(w[j].x), m1 = nzb(w[j].y);
      const int cnt = __builtin_popcount(m0) + __builtin_popcount(m1);
      const int incl = row16_scan(cnt);
      const int excl = incl - cnt;
      const bool holder = act[j] && (int)rem[j] >= excl && (int)rem[j] < incl;
      int32_t val = -1;
      if (holder) {  // the (rem - excl)-th present cell of its 8
        int need = (int)rem[j] - excl, pos = 0;
        uint32_t byte = 0;
#pragma unroll
        for (int v = 0; v < 8; v++) {
          const uint32_t bv = ((v < 4 ? w[j].x : w[j].y) >> (8 * (v & 3))) & 0xFFu;
          if (bv != 0) {
            if (need == 0) { pos = v; byte = bv; }
            need--;
          }
        }
        const int col = band[j] * B + ch[j] * 128 + q * 8 + pos;  // shard-local column
        const bool fresh = s_is_esc(byte) ? esc_fresh(s, rc, col) : S_AGE(s_widen(byte)) < GM_TFAIL;
        val = ((s.c0 + col) << 1) | (int32_t)(fresh && s.c0 + col != me);
      }
      // lane d of the row takes draw d's status from its holder; a draw no lane holds (the record's
      // counts and the cells disagree) keeps -1, which the acceptance reports as GM_ERR_DRAWS if it
      // reaches it -- never an older tick's value left in the reused status buffer
      const uint32_t hm = row16_bits(__ballot(holder), g);
      const int32_t v = row16_bcast(val, g, hm ? __builtin_ctz(hm) : 0);
      if (act[j] && q == dj[j]) myst = hm ? v : -1;
    }
  }
  if (mine) st[q] = myst;
}

hipError_t gm_launch_draw0(const SState &s, int t, int r0, int r1, hipStream_t st) {
  if (r1 <= r0) return hipSuccess;
  const size_t smem = sizeof(uint32_t) * 16 * (size_t)(s.nb + 1);
  hipLaunchKernelGGL(gm_s_draw0<1024>, dim3((r1 - r0 + 15) / 16), dim3(256), smem, st, s, t, r0, r1);
  return hipGetLastError();
}
// true when gm_s_draw0 applies: B = 1024, no join ramp, <= 16 ranks, the band prefix fits LDS
bool gm_draw0_ok(const SState &s) {
  return s.band == 1024 && !s.ramp && s.shard_count <= 16 && sizeof(uint32_t) * 16 * (size_t)(s.nb + 1) <= 65536;
}

// Phase B: every rank replays every pending row's S2 stream (round 0: outputs
// [0, 16) from gm_s_mtgen; round q >= 1: [16 + 64(q-1), 16 + 64q) from the lazy
// generator) and resolves the draws whose rank lands in its own columns.
// status[r][d] = -2 for an output Lemire rejects (same on every rank),
// (global column << 1) | fresh on the owning rank, -1 elsewhere (MAX-allreduced).
template <int B>
__global__ __launch_bounds__(256) void gm_s_draw(SState s, int t, int round, int D, int listed, int r0, int r1) {
  extern __shared__ __align__(16) uint32_t p_smem[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  // listed: the rows still pending after round 0, in ascending order (gm_s_plist_sort);
  // their statuses go to status1 by list position. Unlisted: rows [r0, r1) (a row chunk)
  const int i = (listed ? 0 : r0) + (int)blockIdx.x * 4 + wave;
  if (listed && i >= plist_len(s, listed)) return;
  const int r = listed ? s.plist[listed][i] : i;
  if (r >= (listed ? s.n : r1)) return;
  // round 0 has no lazy generator state (gm_launch_draw sizes its LDS to the chunk prefix)
  uint32_t *pre = p_smem + wave * (round == 0 ? (size_t)gm_draw_chunks(s.wp, B) + 1 : gm_draw_lds_words(s.wp, B));
  uint32_t *mts = pre + gm_draw_chunks(s.wp, B) + 1;
  const int G = s.shard_count;
  int32_t *acc = s.acc + (size_t)r * 8;
  // round 0: every load of the row issues at once -- crash flag, delivered-list count, the ranks'
  // counts, the 16 S2 outputs and this shard's first band record (for the chunk prefix; ~88 % of the
  // rows resolve a draw here) -- one memory round trip before the chunk search, not four
  uint32_t raw0 = 0;
  uint4 rec0 = make_uint4(0u, 0u, 0u, 0u);
  if (round == 0) {
    const int par = t & 1;
    int failed = s.failed[r], kin = s.inbox_cnt[par][r];
    int size = 0, nf = 0;
    bool selfapp = false;
    raw0 = lane < S_MT_RAW ? s.mtraw[(size_t)r * S_MT_RAW + lane] : 0u;
    rec0 = gm_row_rec0(s, r, lane);
    for (int g = 0; g < G; g++) {
      const int pr = s.xcnt[S_XC(s, g, r)];
      size += pr & S_XC_COUNT;
      selfapp |= (pr & S_XC_SELFAPP) != 0;
      nf += s.xcnt[S_XC(s, g, r) + 1];
    }
    asm volatile("" : "+v"(raw0), "+v"(rec0.x), "+v"(rec0.y), "+v"(rec0.z), "+v"(rec0.w));
    const bool live = !failed && s_ingroup(s.ramp, s.intro_until, r, t);  // else untouched
    if (lane == 0) {  // lists delivered this tick; consumed by gm_s_band, the append target of tick t+2
      s.rowstat[(size_t)r * 4] = live ? kin : 0;
      s.inbox_cnt[par][r] = 0;
    }
    if (selfapp && lane == 0) {
      // join ramp: row r appended its own entry (updateMyPos found no larger id in its start
      // group, gm_s_band); the reference appends only if no larger id is present at all --
      // the shards above the group must hold nothing of the row (present, or removed this tick)
      for (int g = 0; g < G; g++) {
        const int c0g = (int)((int64_t)s.n * g / G);
        if (c0g > (r | 3) && ((s.xcnt[S_XC(s, g, r)] & S_XC_COUNT) || s.xcnt[S_XC(s, g, r) + 1]))
          atomicOr(s.err, GM_ERR_SELF);
      }
    }
    const int numpot = size - 1 - nf;
    int nj = 0, jn[4] = {0, 0, 0, 0};
    if (s.ramp && r == 0 && live)  // gossipnodes = newNodes first (MP1Node.cpp:458): this tick's joiners, ascending id
      for (int c = max(1, 4 * (t - 1)); c < min(s.n, 4 * t); c++) jn[nj++] = c;
    const bool pend = live && numpot > 0 && nj < min(GM_FANOUT, numpot);
    if (lane == 0) {
      acc[0] = nj;
      for (int q = 0; q < 4; q++) acc[1 + q] = jn[q];
      acc[6] = numpot;
      acc[7] = size;
      s.pending[r] = pend;
      int32_t *stat = s.rowstat + (size_t)r * 4;
      stat[1] = live ? size : 0;
      stat[2] = live ? nf : 0;
      stat[3] = live && !pend ? nj : 0;
      if (live && !pend && nj) {  // the joiners alone (no draws): enqueue now, like gm_s_accept
        int32_t *cnt_out = s.inbox_cnt[(t & 1) ^ 1];
        for (int q = 0; q < nj; q++) {
          s.targets[(size_t)r * GM_FANOUT + q] = jn[q];
          const int slot = atomicAdd(&cnt_out[jn[q]], 1);
          if (slot < s.kcap) s.inbox[(t & 1) ^ 1][(size_t)jn[q] * S_KMAX + slot] = r;
          else atomicOr(s.err, GM_ERR_INBOX);
        }
      }
    }
    if (!pend) return;
  } else if (!s.pending[r]) {
    return;
  }
  // the round of this row's draws: the launch's for a bounded round over a pending list;
  // the row's own (pending[r] = its next round) in the host-driven loop, where rows that a
  // bounded round could not take continue from where they stopped
  const int rr = (round == 0 || listed) ? round : s.pending[r];
  const uint32_t size = (uint32_t)acc[7];
  uint32_t own_lo = 0;
  for (int g = 0; g < s.shard_rank; g++) own_lo += (uint32_t)s.xcnt[S_XC(s, g, r)] & S_XC_COUNT;
  const uint32_t own_cnt = (uint32_t)s.xcnt[S_XC(s, s.shard_rank, r)] & S_XC_COUNT;
  // "me" (myPos's id, MP1Node.cpp:459-460,470) is the row's own column, or in the join ramp
  // the quirk's target column; only the rank owning it knows it (mecol is -1 elsewhere), and
  // only that rank resolves a draw there: it reports "me" as not fresh, which the acceptance
  // skips the same way
  const int me = s.ramp ? s.mecol[r] : r;
  bool have_pre = false;  // this shard's chunk prefix of the row, built on first use
  const uint32_t thr = (0u - size) % size;
  GmLazyMT mt;
  int32_t *st = listed ? s.statusl[listed] + (size_t)i * D : s.status + (size_t)r * D;
  for (int d0 = 0; d0 < D; d0 += 64) {
    const int cnt = min(64, D - d0);
    uint32_t raw = 0;
    if (round == 0) {
      raw = raw0;  // D = 16: the one batch
    } else {  // round q >= 1 continues after 16 + 64 (q - 1) outputs (round 2 of the bounded tick: after 80)
      raw = gm_mt_batch(mt, mts, gm_rd_seed(s.rd_seed, t, r + 1), d0 == 0, S_MT_RAW + 64 * (rr - 1) + d0, cnt,
                        lane);
    }
    const uint64_t prod = (uint64_t)raw * size;
    const bool ok = lane < cnt && (uint32_t)prod >= thr;
    const uint32_t ix = (uint32_t)(prod >> 32);
    const bool mine = ok && ix >= own_lo && ix < own_lo + own_cnt;
    int32_t val = ok ? (s.stub ? stub_target(ix, size, s.n) : -1) : -2;
    uint64_t m = __ballot(mine);
    if (m && !have_pre) {
      uint32_t osz, onf;
      gm_row_totals<B>(s, r, lane, pre, osz, onf, round == 0 ? &rec0 : nullptr);
      have_pre = true;
    }
    while (m) {
      const int grp = lane >> 3;
      int myd = 0, c8 = 0, d[8];
#pragma unroll
      for (int i = 0; i < 8; i++) {
        d[i] = m ? __builtin_ctzll(m) : 64;
        if (m) {
          if (grp == i) myd = d[i];
          m &= m - 1;
          c8++;
        }
      }
      const uint32_t myix = __shfl(ix, myd, 64) - own_lo;
      int col[8], fr[8];
      gm_resolve8<B>(s, r, pre, grp < c8, myix, lane, col, fr);
#pragma unroll
      for (int i = 0; i < 8; i++)
        if (i < c8 && lane == d[i]) val = col[i] < 0 ? -1 : (((s.c0 + col[i]) << 1) | (fr[i] && s.c0 + col[i] != me));
    }
    if (lane < cnt) st[d0 + lane] = val;
  }
  if (rr > 0 && !listed && lane == 0) s.pending[r] = rr + 1;
}

// Phase C: with every draw resolved (MAX-allreduced status), run the acceptance loop
// of MP1Node.cpp:466-489 (skip me, skip stale, skip duplicates) identically on every
// rank; finished rows enqueue themselves into their targets' inboxes for tick t+1.
// mode 0: every row, statuses by row; rows left pending are counted (npending, host loop).
// mode 1: every row, and rows left pending are also appended to plist (bounded rounds).
// mode 2: the plist rows, statuses by list position; a row still pending sets GM_ERR_DRAWS.
// in_list 0: every row, statuses by row; 1 / 2: the rows of pending list 1 / 2, statuses by
// list position. Rows left pending go to: out -1 -> GM_ERR_DRAWS (bounded rounds exhausted),
// 0 -> the npending count (host-driven loop), 1 / 2 -> pending list 1 / 2 (next bounded round).
__global__ __launch_bounds__(256) void gm_s_accept(SState s, int t, int D, int in_list, int out, int r0, int r1) {
  const int i = (in_list ? 0 : r0) + (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (in_list && i >= plist_len(s, in_list)) return;
  const int r = in_list ? s.plist[in_list][i] : i;
  if (r >= (in_list ? s.n : r1) || !s.pending[r]) return;
  int32_t *acc = s.acc + (size_t)r * 8;
  // the row's accumulator (8 ints) and, in round 0 (D = 16), its 16 statuses by vector loads, all
  // in flight together: the draw loop below then runs on registers, not one load round trip per
  // draw (each row's words are its own 32 B / 64 B)
  const int4 a0 = ((const int4 *)acc)[0], a1 = ((const int4 *)acc)[1];
  int n = a0.x;
  const int numpot = a1.z;
  int g[GM_FANOUT] = {a0.y, a0.z, a0.w, a1.x, a1.y};
  static_assert(GM_FANOUT == 5, "acc = {n, g[0..4], numpot, size}");
  const int32_t *st = in_list ? s.statusl[in_list] + (size_t)i * D : s.status + (size_t)r * D;
  bool done = n >= GM_FANOUT || n >= numpot;
  auto take = [&](int32_t v) {  // one draw of MP1Node.cpp:466-489, in draw order
    if (done || v == -2) return;  // output rejected by Lemire: not a draw
    if (v < 0) {                  // a draw no shard resolved
      atomicOr(s.err, GM_ERR_DRAWS);
      done = true;
      return;
    }
    const int c = v >> 1;
    if (c == r) return;     // "me"
    if (!(v & 1)) return;   // age >= TFAIL
    bool dup = false;
#pragma unroll
    for (int q = 0; q < GM_FANOUT; q++) dup |= q < n && g[q] == c;
    if (!dup) {
#pragma unroll
      for (int q = 0; q < GM_FANOUT; q++)
        if (q == n) g[q] = c;
      n++;
    }
    done = n >= GM_FANOUT || n >= numpot;
  };
  if (D == 16) {
    int4 v4[4];
#pragma unroll
    for (int q = 0; q < 4; q++) v4[q] = ((const int4 *)st)[q];
#pragma unroll
    for (int q = 0; q < 4; q++) {
      take(v4[q].x);
      take(v4[q].y);
      take(v4[q].z);
      take(v4[q].w);
    }
  } else {
    for (int d = 0; d < D && !done; d++) take(st[d]);
  }
  for (int q = 0; q < n; q++) acc[1 + q] = g[q];
  acc[0] = n;
  if (!done) {
    // pending[r] = the row's next round: host-driven rounds q >= 1 draw S2 outputs
    // [16 + 64(q-1), 16 + 64q), so bounded round 1 = host round 1 and bounded round 2 (outputs
    // [80, 336)) = host rounds 2..5. A row no bounded round takes (its list is full, or it is
    // still short after round 2) is counted in npending; the host finishes it with the
    // host-driven rounds before anything reads the tick (draw_settle, gm_host_shard.hip)
    if (out == 0) {
      atomicAdd(s.npending, 1);  // gm_s_draw advanced pending[r]
    } else if (out > 0) {
      s.pending[r] = out;
      const uint32_t slot = atomicAdd(s.plist_cnt[out], 1u);
      if (slot < (uint32_t)s.plist_cap[out]) s.plist[out][slot] = r;
      else atomicAdd(s.npending, 1);
    } else {
      s.pending[r] = 1 + (GM_D_MORE_ROUND + GM_D_LAST_ROUND) / 64;
      atomicAdd(s.npending, 1);
    }
    return;
  }
  s.pending[r] = 0;
  const int par = t & 1;
  int32_t *cnt_out = s.inbox_cnt[par ^ 1];
  int slot[GM_FANOUT];
#pragma unroll
  for (int q = 0; q < GM_FANOUT; q++)  // the row's appends in flight together, then their stores
    if (q < n) slot[q] = atomicAdd(&cnt_out[g[q]], 1);
#pragma unroll
  for (int q = 0; q < GM_FANOUT; q++) {
    if (q >= n) continue;
    s.targets[(size_t)r * GM_FANOUT + q] = g[q];
    if (slot[q] < s.kcap) s.inbox[par ^ 1][(size_t)g[q] * S_KMAX + slot[q]] = r;
    else atomicOr(s.err, GM_ERR_INBOX);
  }
  s.rowstat[(size_t)r * 4 + 3] = n;
}

// rows [r0, r1) (unlisted) or the pending list `listed`. Round 0 draws only the 16 precomputed
// outputs: no lazy generator, so its waves take the chunk prefix's LDS alone.
hipError_t gm_launch_draw(const SState &s, int t, int round, int D, int listed, hipStream_t st, int r0, int r1) {
  if (r1 < 0) r1 = s.n;
  if (round == 0 && !listed && D == S_MT_RAW && gm_draw0_ok(s) && !(getenv("GM_DRAW0") && !atoi(getenv("GM_DRAW0"))))
    return gm_launch_draw0(s, t, r0, r1, st);  // four rows per wave
  const size_t words = round == 0 ? (size_t)gm_draw_chunks(s.wp, s.band) + 1 : gm_draw_lds_words(s.wp, s.band);
  const size_t smem = sizeof(uint32_t) * 4 * words;
  const int rows = listed ? s.plist_cap[listed] : r1 - r0;
  if (rows <= 0) return hipSuccess;
  const dim3 grid((rows + 3) / 4), blk(256);
  return gm_band_dispatch(s.band, [&](auto b) {
    hipLaunchKernelGGL(gm_s_draw<decltype(b)::value>, grid, blk, smem, st, s, t, round, D, listed, r0, r1);
    return hipGetLastError();
  });
}

hipError_t gm_launch_accept(const SState &s, int t, int D, int in_list, int out, hipStream_t st, int r0, int r1) {
  if (r1 < 0) r1 = s.n;
  const int rows = in_list ? s.plist_cap[in_list] : r1 - r0;
  if (rows <= 0) return hipSuccess;
  hipLaunchKernelGGL(gm_s_accept, dim3((rows + 255) / 256), dim3(256), 0, st, s, t, D, in_list, out, r0, r1);
  return hipGetLastError();
}

// The pending rows of round 0 in ascending order: the list order (= status1 rows) must be
// the same on every rank, whatever order the atomics appended them in. A list that overflowed
// holds a subset that depends on that order, so it is void (plist_len 0) and all of its rows go
// to the host-driven rounds (every rank counts the same total, acceptance being identical).
__global__ __launch_bounds__(1024) void gm_s_plist_sort(SState s, int l) {
  __shared__ int32_t v[S_PLIST_CAP];
  int32_t *list = s.plist[l];
  if (*s.plist_cnt[l] > (uint32_t)s.plist_cap[l]) {  // the appends past cap were counted already
    if (threadIdx.x == 0) atomicAdd(s.npending, s.plist_cap[l]);
    return;
  }
  const int cnt = (int)*s.plist_cnt[l];
  if (cnt <= 1) return;
  int m = 1;
  while (m < cnt) m <<= 1;
  for (int k = threadIdx.x; k < m; k += blockDim.x) v[k] = k < cnt ? list[k] : 0x7FFFFFFF;
  __syncthreads();
  for (int size = 2; size <= m; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int k = threadIdx.x; k < m; k += blockDim.x) {
        const int o = k ^ stride;
        if (o > k) {
          const bool up = (k & size) == 0;
          const int a = v[k], b = v[o];
          if ((a > b) == up) {
            v[k] = b;
            v[o] = a;
          }
        }
      }
      __syncthreads();
    }
  for (int k = threadIdx.x; k < cnt; k += blockDim.x) list[k] = v[k];
}

hipError_t gm_launch_plist_sort(const SState &s, int l, hipStream_t st) {
  hipLaunchKernelGGL(gm_s_plist_sort, dim3(1), dim3(1024), 0, st, s, l);
  return hipGetLastError();
}

// the single-context pick: one compile unit with the kernels above (see the file's header)
#include "gm_pick.hip"
