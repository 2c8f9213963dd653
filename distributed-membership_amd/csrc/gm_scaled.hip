// gm_scaled.hip -- SCALED-mode tick: the HBM-bound full-membership hot path.
//
// One globaltime tick (Application::mp1Run for every node, Application.cpp:121-164)
// is three launches on the context stream:
//
//   gm_s_mtgen  thread per row: the first S_MT_RAW outputs of the row's S2 stream
//               (the mt19937 that nodeLoopOps seeds per call, MP1Node.cpp:450-452),
//               computed from 397+16 init words kept in registers.
//   gm_s_band   the merge / heartbeat / sweep pass over the N x W table, in COLUMN
//               BANDS: one wave per (band, 64 rows) streams the band's slice of its rows,
//               max-merges the slices of the gossip payloads delivered to each row
//               (updatelistCallBack, MP1Node.cpp:259-301), bumps the row's own entry
//               (MP1Node.cpp:409-415), runs the TFAIL/TREMOVE sweep (MP1Node.cpp:
//               426-444), writes the row slice back and the row's payload slice for
//               tick t+1 (the fresh entries' heartbeats, sendMemberList MP1Node.cpp:
//               360-395), and records per-(row, band) counts and events. Workgroups
//               are numbered band-major, so the chip sweeps one band of every row at a
//               time: a sender's payload slice is read by its ~5 receivers while that
//               band's payload slices (N x band x 2 B) are resident in the 256 MiB
//               Infinity Cache -- HBM sees each payload byte once instead of once per
//               delivery (band width sized so one band's traffic fits the cache).
//   gm_s_pick   wave per row: row totals from the band counts, the gossip-target draw
//               on the post-sweep list (MP1Node.cpp:449-489: Lemire over the S2
//               outputs, "memberlist[ix]" = rank-select over band prefix counts and one
//               table slice, skip me / stale / duplicates), and delivery: the row
//               appends itself to its targets' inboxes for tick t+1 (counting sort by
//               destination in place of EmulNet's buffer scan, EmulNet.cpp:144-177).
//
// Column-sharded ticks (multi-GPU) run gm_s_mtgen + gm_s_band on the shard's columns
// (which also accumulates the shard's per-row counts), exchange the counts, then
// gm_s_draw / gm_s_accept rounds.
//
// The kernels by unit:
//   gm_scaled.hip     this file: gm_s_mtgen, gm_s_init, the msgcount kernels, gm_launch_tick
//   gm_band.hip       gm_s_band, gm_s_band_listed, gm_s_selfcheck and the band launcher
//   gm_band_fast.hip  gm_s_band_fast (B = 1024) and its tunables, compiled as part of gm_band.hip;
//                     gm_band.h is what the two share
//   gm_draw.hip       gm_s_xrows, gm_s_draw0, gm_s_draw, gm_s_accept, gm_s_plist_sort
//   gm_pick.hip       gm_s_pick, gm_s_pick0, compiled as part of gm_draw.hip
//   gm_select.h       the rank-select helpers the pick and the draw share
#include "gm_band.h"
#include "gm_device.h"
#include "gm_scaled.h"
#include "gm_select.h"

#include <algorithm>

// ------------------------------------------------------------------ gm_s_mtgen
// Also zeroes the tick's counters (no fill launch of their own each tick): the event spill ring's
// count and the striped event totals (the last tick's records stay readable until here), and the
// fused draw's fallback-row count (gm_s_pick0 runs after the band kernels). Grid: max(n, 1 + S_EV_STRIPES).
// zero_draw (the pipelined column-shard tick): also the draw rounds' counters -- the pending lists'
// append counts and the rows left to the host-driven rounds (three fill launches a tick before)
__global__ __launch_bounds__(256) void gm_s_mtgen(SState s, int t, int zero_draw) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r < 1 + S_EV_STRIPES) s.ev_spill_cnt[r] = 0;
  if (r == 0 && s.pk_cnt) *s.pk_cnt = 0;
  if (zero_draw && r == 0) {
    *s.plist_cnt[1] = 0;
    *s.plist_cnt[2] = 0;
    *s.npending = 0;
  }
  if (r >= s.n) return;
  uint32_t out[S_MT_RAW];
  gm_mt_first16(gm_rd_seed(s.rd_seed, t, r + 1), out);
  uint4 *dst = (uint4 *)(s.mtraw + (size_t)r * S_MT_RAW);
#pragma unroll
  for (int k = 0; k < S_MT_RAW / 4; k++) dst[k] = make_uint4(out[4 * k], out[4 * k + 1], out[4 * k + 2], out[4 * k + 3]);
}

// the per-tick work before the band kernels: event counters, the S2 precompute
hipError_t gm_launch_tick_prologue(const SState &s, int t, hipStream_t st, bool zero_draw) {
  // the event records of a tick (per-(row, band) slots + spill ring) stay readable until the next
  // tick: gm_s_mtgen zeroes their counters
  hipLaunchKernelGGL(gm_s_mtgen, dim3((std::max(s.n, 1 + S_EV_STRIPES) + 255) / 256), dim3(256), 0, st, s, t,
                     zero_draw ? 1 : 0);
  return hipGetLastError();
}

// ------------------------------------------------------------ gm_s_msgcount
// msgcount analogue of tick t (gm_msgcount_record), in two phases:
//   gm_s_mcfresh (after gm_s_band, wave per row): fresh = the row's non-zero payload nibbles of
//     this tick in this context's columns (the entries it sends, MP1Node.cpp:372-375);
//     column shards SUM-allreduce it (and the DROP band kernel's per-row kept counts), so
//     every rank holds the whole row's counts;
//   gm_s_mcount (after the targets are final, thread per row): sent = fresh x targets;
//     received = the entries of the delivered lists -- the senders' fresh counts of tick t-1,
//     or on loss ticks the kept entries counted by the DROP band kernel.
__device__ __forceinline__ uint32_t nz_nibbles(uint32_t x) {
  return (uint32_t)__builtin_popcount((x | (x >> 1) | (x >> 2) | (x >> 3)) & 0x11111111u);
}
template <int B>
__global__ __launch_bounds__(256) void gm_s_mcfresh(SState s, int t) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= s.n) return;  // whole wave
  const int par = t & 1, half = B / 2, tot = s.nb * half;
  uint32_t f = 0;
  for (int off = lane * 16; off < tot; off += 64 * 16) {  // 16-byte pieces never straddle a band
    const int b = off / half, o = off % half;
    const uint4 v = *(const uint4 *)(s.msg + ((size_t)b * s.n + r) * B + par * half + o);
    f += nz_nibbles(v.x) + nz_nibbles(v.y) + nz_nibbles(v.z) + nz_nibbles(v.w);
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) f += __shfl_xor(f, o, 64);
  if (lane == 0) s.mc_fresh[(size_t)par * s.n + r] = f;
}

__global__ __launch_bounds__(256) void gm_s_mcount(SState s, int t, int dropped) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= s.n) return;
  const int par = t & 1;
  const int32_t *stat = s.rowstat + (size_t)r * 4;
  uint32_t recv = 0;
  if (dropped) {
    recv = s.mc_rdrop[r];
    s.mc_rdrop[r] = 0;
  } else {
    const int k = min(stat[0], S_KMAX);  // 0 for rows not merged this tick
    for (int q = 0; q < k; q++) recv += s.mc_fresh[(size_t)(par ^ 1) * s.n + s.inbox[par][(size_t)r * S_KMAX + q]];
  }
  s.mc_sent[(size_t)t * s.n + r] = (uint32_t)stat[3] * s.mc_fresh[(size_t)par * s.n + r];
  s.mc_recv[(size_t)t * s.n + r] = recv;
}

// phase 0: fresh counts (gm_s_mcfresh); phase 1: sent / received (gm_s_mcount)
hipError_t gm_launch_msgcount(const SState &s, int t, bool dropped, int phase, hipStream_t st) {
  if (phase == 1) {
    hipLaunchKernelGGL(gm_s_mcount, dim3((s.n + 255) / 256), dim3(256), 0, st, s, t, dropped ? 1 : 0);
    return hipGetLastError();
  }
  const dim3 g((s.n + 3) / 4), bk(256);
  return gm_band_dispatch(s.band, [&](auto b) {
    hipLaunchKernelGGL(gm_s_mcfresh<decltype(b)::value>, g, bk, 0, st, s, t);
    return hipGetLastError();
  });
}

// SCALED initial state (gm_config.init_mode): every observer holds every subject.
// Cold: {hb 0, ts 0}. Warm at t0: own entry {2*t0-1, t0}; others {2*(t0-1-a)-1,
// t0-a}, a = splitmix64(seed ^ r<<32 ^ c) % 4 -- values as if the cluster had been
// gossiping, so the first ticks carry no mass-staleness transient. Padding absent.
// Cells are encoded relative to tick t0 (S_CELL: h = 255 - (2*t0 - hb), age = t0 - ts).
// Join ramp (warm = 2): nobody in any list but the introducer's own entry {hb 0, ts 0}
// (nodeStart of node 0 at tick 0, MP1Node.cpp:126-140); state as of tick 0.
// The band kernel's lane mapping (one wave per (band, rows) unit, 16 cells per lane), so the
// escaped cells (a cold start escapes them all: odd h) form the same per-(band, row) lists
// in the pool of tick t0 that gm_s_band writes, and every record's .w names its list.
template <int B>
__global__ __launch_bounds__(256) void gm_s_init(SState s, int warm, int t0, uint64_t seed) {
  constexpr int LPR = B / S_COLS_PER_LANE, RPW = 64 / LPR, Q = S_COLS_PER_LANE;
  const int U = (s.n + RPW - 1) / RPW;
  const int ub = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
  if (ub >= U) return;  // whole wave
  const int lane = threadIdx.x & 63, li = lane % LPR;
  const int band = blockIdx.y, r = ub * RPW + lane / LPR;
  const bool row = r < s.n;
  uint32_t cw[8] = {0, 0, 0, 0, 0, 0, 0, 0}, bw[4] = {0, 0, 0, 0};
  if (row) {
#pragma unroll
    for (int q = 0; q < Q; q++) {
      const int j = band * B + li * Q + q;  // shard-local column
      uint32_t e = 0;                       // absent
      if (j < s.w && warm == 2) {
        if (r == 0 && s.c0 + j == 0) e = S_CELL(255u, 0u);
      } else if (j < s.w) {
        const int c = s.c0 + j;
        if (!warm) e = S_CELL(255u, 0u);  // hb 0 = 2*t0 at t0 = 0
        else if (c == r) e = S_CELL(254u, 0u);
        else {
          const int a = (int)((gm_mix64(seed ^ ((uint64_t)(uint32_t)r << 32) ^ (uint64_t)(uint32_t)c) >> 40) % 4);
          e = S_CELL((uint32_t)(252 - 2 * a), (uint32_t)a);
        }
      }
      cw[q >> 1] |= e << (16 * (q & 1));
      bw[q >> 2] |= s_narrow(e) << (8 * (q & 3));
    }
  }
  const uint32_t em = esc_mask16(bw[0], bw[1], bw[2], bw[3]);
  int etot;
  const int eoff = row_scan<LPR>(__builtin_popcount(em), li, lane, etot);
  const int par = t0 & 1;  // the state is "as of tick t0": tick t0 + 1 reads this pool
  const size_t slab = (size_t)band * s.n;
  const uint32_t base = row_alloc<LPR>(s, par, slab, min(r, s.n - 1), etot, li, lane);
  __shared__ uint32_t lds_all[4 * S_LDS_WAVE_WORDS];
  uint32_t *lds = lds_all + (threadIdx.x >> 6) * S_LDS_WAVE_WORDS;
  if (em) esc_park(lds, lane, cw);
  if (base != 0) esc_emit(lds, lane, esc_list(s, par, slab, r, base), eoff, em, li * Q, etot <= S_ESC_IN, s.err, s.lag_hmin);
  if (!row) return;
  *(u32x4 *)(s.table + (slab + r) * B + li * Q) = (u32x4){bw[0], bw[1], bw[2], bw[3]};
  if (li == 0) {
    s.brec[slab + r] = make_uint4(0u, 0u, 0u, base);
    if (band == 0) {
      s.hbctr[r] = warm == 1 ? 2 * t0 : 0;
      s.wtick[r] = t0;
    }
  }
}

template <int B>
static hipError_t launch_init_b(const SState &s, int warm, int t0, uint64_t seed, hipStream_t st) {
  constexpr int RPW = 64 / (B / S_COLS_PER_LANE);
  const dim3 nblk((((s.n + RPW - 1) / RPW) + 3) / 4, s.nb);
  hipLaunchKernelGGL(gm_s_init<B>, nblk, dim3(256), 0, st, s, warm, t0, seed);
  return hipGetLastError();
}

hipError_t gm_launch_init(const SState &s, int warm, int t0, uint64_t seed, hipStream_t st) {
  return gm_band_dispatch(s.band,
                          [&](auto b) { return launch_init_b<decltype(b)::value>(s, warm, t0, seed, st); });
}

// ------------------------------------------------------------------ gm_launch_tick
// One single-context tick: the prologue, the band kernels of every row, the join ramp's check of
// its self appends, then the pick. k0 / k1 (optional) bracket the band kernels.
hipError_t gm_launch_tick(const SState &s, int t, int drop_pct, hipStream_t st, hipEvent_t k0, hipEvent_t k1,
                          bool pick) {
  hipError_t e = gm_launch_tick_prologue(s, t, st, false);
  if (k0) (void)hipEventRecord(k0, st);
  const hipError_t eb = gm_launch_band_rows(s, t, drop_pct, 0, s.n, st);
  if (e == hipSuccess) e = eb;
  if (k1) (void)hipEventRecord(k1, st);
  if (s.ramp) gm_launch_selfcheck(s, st);
  const hipError_t ep = pick ? gm_launch_pick(s, t, st) : hipGetLastError();
  return e == hipSuccess ? ep : e;
}
