// gm_load.hip -- SCALED: load a cluster state into a context (gm_load_begin / gm_load_rows /
// gm_load_commit, the inverse of gm_read_table / gm_read_nodes / gm_read_targets).
//
// The state between two ticks is layout-independent -- every row's (hb, ts) per column, the
// heartbeat counters, the crash flags, the last tick's gossip targets, the next tick t (oracle/
// ref_cpu.c oc_load_scaled) -- and the stored form is not: cell bytes relative to wtick[r],
// per-(band, row) escape lists in striped pools, payload nibble planes with escape slots, 16-byte
// band records, inboxes (gm_scaled.h). Loading is therefore an encode pass on the device:
//
//   gm_l_check   wave per staged row: the pairs are well formed (both or neither of hb / ts
//                negative, ts <= t - 1), and the row's BASE TICK is chosen: t - 1 when every entry
//                of the row fits the 16-bit cell relative to it (age <= 31, h in [lag_hmin, 255]) --
//                every row that ran tick t - 1 does -- else the newest ts of the row: a row that
//                crashed long ago keeps entries that only fit relative to the tick it last ran.
//                (A crashed row is never re-based again, so any base its entries fit decodes to the
//                same (hb, ts); a live row must be relative to t - 1, which gm_l_nodes verifies.)
//                Entries that fit neither way are GM_ERANGE (the GM_ERR_LAG case), a heartbeat
//                ahead of its row's base tick GM_EINVAL.
//   gm_l_encode  gm_s_init's lane mapping -- one wave per (band, rows) unit, 16 cells per lane -- over
//                the staged block: S_CELL(255 - (2w - hb), w - ts) per cell, then the band kernel's own
//                store side (gm_scaled.h sweep_cells / payload_escapes / unit_stores): the stored
//                bytes, the escape list of parity (t - 1) & 1 named by the record's .w, and, for rows
//                whose base tick is t - 1, the payload plane of tick t - 1 (the fresh entries: what
//                the row put on the wire, oc_load_scaled's snaps) with its escape slots. Record
//                counts are 0 = "no count kept" (the fast path then compares the cells), no events.
//   gm_l_nodes   thread per row, check then write: crash flags 0 / 1, counts 0..5, targets in [0, n);
//                a live row's own entry as the self bump left it ({heartbeat - 1, t - 1}; the cold
//                start's {0, 0} at t = 1) and its base tick t - 1; a crashed row that still has
//                targets ran tick t - 1. Then hbctr, failed, targets, rowstat's count word.
//   gm_l_inbox   thread per row: the row appends itself to the inboxes of its counts[r] targets in the
//                parity tick t reads, one atomic per delivery (gm_s_pick's delivery); a receiver past
//                the inbox capacity is GM_ERANGE.
#include <hip/hip_runtime.h>

#include "gm_abi.h"
#include "gm_scaled.h"

// staged block rows [0, cnt) = table rows [r0, r0 + cnt); hb / ts [cnt][s.w]. base[i]: the row's base
// tick; own[2r], own[2r + 1]: row r's own entry where this context holds column r (checked at commit)
__global__ __launch_bounds__(256) void gm_l_check(SState s, int t, int r0, int cnt, const int32_t *hb,
                                                  const int32_t *ts, int32_t *base, int32_t *own, uint32_t *status) {
  const int i = __builtin_amdgcn_readfirstlane((int)blockIdx.x * 4 + (int)(threadIdx.x >> 6));
  if (i >= cnt) return;  // whole wave
  const int lane = threadIdx.x & 63;
  const int32_t *hr = hb + (size_t)i * s.w, *tr = ts + (size_t)i * s.w;
  uint32_t bad = 0;
  int mints = 0x7FFFFFFF, maxts = -1, minhb = 0x7FFFFFFF, maxhb = -1;
  for (int j = lane; j < s.w; j += 64) {
    const int h = hr[j], a = tr[j];
    if ((h < 0) != (a < 0) || a > t - 1) bad |= GM_LD_EINVAL;
    if (h >= 0 && a >= 0) {
      mints = min(mints, a);
      maxts = max(maxts, a);
      minhb = min(minhb, h);
      maxhb = max(maxhb, h);
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    bad |= (uint32_t)__shfl_xor((int)bad, o, 64);
    mints = min(mints, __shfl_xor(mints, o, 64));
    maxts = max(maxts, __shfl_xor(maxts, o, 64));
    minhb = min(minhb, __shfl_xor(minhb, o, 64));
    maxhb = max(maxhb, __shfl_xor(maxhb, o, 64));
  }
  if (lane != 0) return;
  const int r = r0 + i;
  int w = t - 1;
  if (maxts >= 0 && !bad) {
    // relative to w: age = w - ts <= 31 and h = 255 - (2w - hb) in [lag_hmin, 255] for every entry
    auto fits = [&](int b) { return b - mints <= 31 && 255 - 2 * b + minhb >= s.lag_hmin; };
    if (!fits(w)) w = maxts;
    if (!fits(w)) bad |= GM_LD_ERANGE;
    if (maxhb > 2 * w) bad |= GM_LD_EINVAL;  // a heartbeat ahead of the tick the row was written at
  }
  base[i] = w;
  if (r >= s.c0 && r < s.c0 + s.w) {
    own[2 * r] = hr[r - s.c0];
    own[2 * r + 1] = tr[r - s.c0];
  }
  if (bad) atomicOr(status, bad);
}

template <int B>
__global__ __launch_bounds__(256) void gm_l_encode(SState s, int t, int r0, int cnt, const int32_t *hb,
                                                   const int32_t *ts, const int32_t *base) {
  constexpr int LPR = B / S_COLS_PER_LANE, RPW = 64 / LPR, Q = S_COLS_PER_LANE;
  const int U = (cnt + RPW - 1) / RPW;
  const int ub = __builtin_amdgcn_readfirstlane((int)blockIdx.x * 4 + (int)(threadIdx.x >> 6));
  if (ub >= U) return;  // whole wave
  __shared__ uint32_t lds_all[4 * S_LDS_WAVE_WORDS];  // escaped rows only (esc_park / esc_emit)
  uint32_t *lds = lds_all + (threadIdx.x >> 6) * S_LDS_WAVE_WORDS;
  const int lane = threadIdx.x & 63, sub = lane / LPR, li = lane % LPR;
  const int band = blockIdx.y, i = ub * RPW + sub;
  if (i >= cnt) return;  // row-uniform: the helpers below need the row's own lanes only
  const int r = r0 + i;
  const int w = base[i];
  const bool sent = w == t - 1;  // the row ran tick t - 1: its fresh entries are that tick's payload
  const int32_t *hr = hb + (size_t)i * s.w, *tr = ts + (size_t)i * s.w;
  uint32_t cv[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int q = 0; q < Q; q++) {
    const int j = band * B + li * Q + q;  // shard-local column; padding absent
    uint32_t e = 0;
    if (j < s.w) {
      const int h = hr[j];
      if (h >= 0) e = S_CELL((uint32_t)(255 - (2 * w - h)), (uint32_t)(w - tr[j])) & 0xFFFFu;
    }
    cv[q >> 1] |= e << (16 * (q & 1));
  }
  u16x2 mm[8];
#pragma unroll
  for (int k = 0; k < 8; k++) mm[k] = pk(cv[k]);
  // the band kernel's store side, as of tick t - 1 (unit_finish after its sweep)
  u16x2 np2 = (u16x2)(0), nf2 = (u16x2)(0), badv = (u16x2)(0), nmx = (u16x2)(0), amax = (u16x2)(0);
  u16x2 nwv[2] = {(u16x2)(0), (u16x2)(0)};
  uint32_t cw[8], bw[4];
  sweep_cells(mm, np2, nf2, badv, nmx, amax, nwv, cw, bw);
  const bool esc_st = unpk(badv) != 0;
  const bool esc_row = row_any<LPR>(esc_st, sub);
  uint32_t em = 0;
  if (esc_row && esc_st) {
    em = esc_mask16(bw[0], bw[1], bw[2], bw[3]);
    esc_park(lds, lane, cw);
  }
  const int par = (t - 1) & 1;
  const size_t slab = (size_t)band * s.n;
  const bool pesc = sent && __builtin_elementwise_max(nmx.x, nmx.y) == S_NIB_ESC;
  if (row_any<LPR>(pesc, sub)) payload_escapes<LPR>(s, par, slab, r, li, lane, sub, pesc, cw);
  UnitIn<B> in;
  in.band = band;
  in.r = r;
  const uint32_t eb = unit_stores<B>(s, t - 1, in, bw, sent ? unpk(nwv[0]) : 0u, sent ? unpk(nwv[1]) : 0u, esc_row,
                                     em, lds);
  if (li == 0) {
    s.brec[slab + r] = make_uint4(0u, 0u, 0u, eb);
    if (band == 0) s.wtick[r] = w;  // (unit_stores stamped t - 1: this lane's later store stands)
  }
}

// write = 0: every check, nothing written but the status word; write = 1 (after a clean check): the
// node arrays, the targets and rowstat's count word
__global__ __launch_bounds__(256) void gm_l_nodes(SState s, int t, const int32_t *heartbeat, const int32_t *failed,
                                                  const int32_t *targets, const int32_t *counts, const int32_t *own,
                                                  uint32_t *status, int write) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= s.n) return;
  const int f = failed[r], k = counts[r], hbc = heartbeat[r];
  if (!write) {
    uint32_t bad = 0;
    if (f != 0 && f != 1) bad |= GM_LD_EINVAL;
    if (k < 0 || k > GM_FANOUT) bad |= GM_LD_EINVAL;
    for (int q = 0; q < min(max(k, 0), GM_FANOUT); q++) {
      const int d = targets[(size_t)r * GM_FANOUT + q];
      if (d < 0 || d >= s.n) bad |= GM_LD_EINVAL;
    }
    const bool ran = s.wtick[r] == t - 1;
    if (f == 0) {
      // what the converged tick kernels assume of a live row: its own entry present (GM_ERR_SELF
      // otherwise) as the last self bump left it, so the next bump's heartbeat hbctr + 1 follows it
      if (r >= s.c0 && r < s.c0 + s.w) {
        const int oh = own[2 * r], ot = own[2 * r + 1];
        const bool cold = t == 1 && oh == 0 && ot == 0 && hbc == 0;
        if (!cold && !(ot == t - 1 && oh == hbc - 1)) bad |= GM_LD_EINVAL;
      }
      if (!bad && !ran) bad |= GM_LD_ERANGE;  // an entry that does not fit relative to t - 1
    } else if (k > 0 && !ran) {
      bad |= GM_LD_EINVAL;  // a row that did not run tick t - 1 sent nothing
    }
    if (bad) atomicOr(status, bad);
    return;
  }
  s.hbctr[r] = hbc;
  s.failed[r] = f;
#pragma unroll
  for (int q = 0; q < GM_FANOUT; q++) s.targets[(size_t)r * GM_FANOUT + q] = q < k ? targets[(size_t)r * GM_FANOUT + q] : 0;
  *(int4 *)(s.rowstat + (size_t)r * 4) = make_int4(0, 0, 0, k);
}

// the sends of tick t - 1, delivered at tick t (inbox_cnt of both parities zeroed before)
__global__ __launch_bounds__(256) void gm_l_inbox(SState s, int t, uint32_t *status) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= s.n) return;
  const int par = t & 1;
  const int k = s.rowstat[(size_t)r * 4 + 3];
  for (int q = 0; q < k; q++) {
    const int dst = s.targets[(size_t)r * GM_FANOUT + q];
    const int slot = atomicAdd(&s.inbox_cnt[par][dst], 1);
    if (slot < s.kcap) s.inbox[par][(size_t)dst * S_KMAX + slot] = r;
    else atomicOr(status, GM_LD_ERANGE);
  }
}

// ------------------------------------------------------------ launch wrappers
hipError_t gm_launch_load_check(const SState &s, int t, int r0, int cnt, const int32_t *hb, const int32_t *ts,
                                int32_t *base, int32_t *own, uint32_t *status, hipStream_t st) {
  hipLaunchKernelGGL(gm_l_check, dim3((cnt + 3) / 4), dim3(256), 0, st, s, t, r0, cnt, hb, ts, base, own, status);
  return hipGetLastError();
}

template <int B>
static void launch_encode_b(const SState &s, int t, int r0, int cnt, const int32_t *hb, const int32_t *ts,
                            const int32_t *base, hipStream_t st) {
  constexpr int RPW = 64 / (B / S_COLS_PER_LANE);
  const dim3 nblk((((cnt + RPW - 1) / RPW) + 3) / 4, s.nb);
  hipLaunchKernelGGL(gm_l_encode<B>, nblk, dim3(256), 0, st, s, t, r0, cnt, hb, ts, base);
}

hipError_t gm_launch_load_encode(const SState &s, int t, int r0, int cnt, const int32_t *hb, const int32_t *ts,
                                 const int32_t *base, hipStream_t st) {
  return gm_band_dispatch(s.band, [&](auto b) {
    launch_encode_b<decltype(b)::value>(s, t, r0, cnt, hb, ts, base, st);
    return hipGetLastError();
  });
}

hipError_t gm_launch_load_nodes(const SState &s, int t, const int32_t *heartbeat, const int32_t *failed,
                                const int32_t *targets, const int32_t *counts, const int32_t *own, uint32_t *status,
                                int write, hipStream_t st) {
  hipLaunchKernelGGL(gm_l_nodes, dim3((s.n + 255) / 256), dim3(256), 0, st, s, t, heartbeat, failed, targets, counts,
                     own, status, write);
  return hipGetLastError();
}

hipError_t gm_launch_load_inbox(const SState &s, int t, uint32_t *status, hipStream_t st) {
  hipLaunchKernelGGL(gm_l_inbox, dim3((s.n + 255) / 256), dim3(256), 0, st, s, t, status);
  return hipGetLastError();
}
