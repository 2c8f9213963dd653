// gm_host_scaled.hip -- SCALED host side: sizing and allocation of the SCALED kernels' state (gm_scaled.h), and the
// tick of a single context (a column shard's tick is gm_host_shard.hip's).
#include "gm_host.h"

using namespace gmh;

// Band width of the SCALED tick: the largest of 512/256/128/64 columns (dividing
// the padded row) whose per-band traffic -- N rows x band x (2 B cell read + 2 B
// write + 1 B payload write + 1 B payload read) -- stays within ~210 MB, so a band's
// payload slab stays resident in the 256 MiB Infinity Cache across its ~5 readers
// per sender slice (gm_band.h). gm_config.band / env GM_BAND override.
static int pick_band(const gm_ctx *c, int n, int wp) {
  int b = c->cfg.band;
  if (!b && getenv("GM_BAND")) b = atoi(getenv("GM_BAND"));
  if (b) return (b == 64 || b == 128 || b == 256 || b == 512 || b == 1024) && wp % b == 0 ? b : -1;
  // Measured (profiles/r02/): the widest band wins -- one row per wave at B = 1024 (no
  // max over two rows' list counts, half the per-(row, band) bookkeeping per cell), and a
  // payload gather stays whole lines; B = 128 gathers half a line per row. gm_s_band at
  // N = 65,536: 4.98 ms (B = 1024), 5.43 (512), 7.42 (128); the S-B shard (N = 262,144,
  // G = 8): 11.0 / 12.0 / 15.0 ms. Per-band traffic up to ~1.4 GB still keeps the gathered
  // payload slab (n x B/2 bytes) on-die.
  const double budget = 1.4e9;
  for (int cand : {1024, 512, 256, 128})
    if (wp % cand == 0 && 5.0 * n * cand <= budget) return cand;
  return 64;
}

int gmh::create_scaled(gm_ctx *c) {
  const int n = c->n;
  const int G = c->cfg.shard_count > 0 ? c->cfg.shard_count : 1;
  const int rank = c->cfg.shard_rank;
  if (rank < 0 || rank >= G || G > n) return GM_EINVAL;
  SState &s = c->s;
  s.n = n;
  s.shard_rank = rank;
  s.shard_count = G;
  // one forced shard (diagnostics/tests): the sharded tick + RCCL with a single rank
  s.sharded = G > 1 || (getenv("GM_FORCE_SHARD") && atoi(getenv("GM_FORCE_SHARD")) == 1);
  // contiguous, balanced subject-column ranges whose boundaries are multiples of 4 (when n >= 8G):
  // a start group of the join ramp (ids 4g..4g+3, gm_s_band's updateMyPos quirk) never straddles two
  // shards, and the keyed loss's 4-column hash groups are whole on every shard
  auto col0 = [n, G](int g) {
    if (g >= G) return n;
    return n >= 8 * G ? 4 * (int)((int64_t)n * g / (4 * G)) : (int)((int64_t)n * g / G);
  };
  s.c0 = col0(rank);
  s.w = col0(rank + 1) - s.c0;
  s.wp = (s.w + S_ROW_ALIGN - 1) / S_ROW_ALIGN * S_ROW_ALIGN;
  s.band = pick_band(c, n, s.wp);
  if (s.band < 0) return GM_EINVAL;
  s.nb = s.wp / s.band;
  if ((size_t)n * s.band * 2 >= (1ull << 31)) return GM_EUNSUPPORTED;  // 32-bit buffer offsets per band slab
  s.evs = s.band / 32;
  // draw kernels' LDS: 4 waves x (chunk prefix + lazy MT state); N = 262,144 on one GPU: 42 KB
  if (sizeof(uint32_t) * 4 * ((size_t)(s.wp / S_CHUNK(s.band)) + 1 + 624) > 65536) return GM_EUNSUPPORTED;
  s.rd_seed = c->cfg.rd_seed;
  s.drop_seed = c->cfg.drop_seed;
  const size_t cells = (size_t)n * s.wp;
  TRY(dalloc(c, &s.table, cells));   // stored cell bytes
  s.kcap = inbox_cap(S_KMAX);
  s.lag_hmin = 3;  // h <= 2: the next re-base would wrap (lag > 125 ticks)
  if (getenv("GM_LAG_CAP")) {  // diagnostics (tests): fail at a lag > L ticks (h = 254 - 2 lag), L >= 15
    const int L = atoi(getenv("GM_LAG_CAP"));
    if (L < 15 || L > 125) return GM_EINVAL;
    s.lag_hmin = 254 - 2 * L;
  }
  c->shard_sync = getenv("GM_SHARD_SYNC") ? (atoi(getenv("GM_SHARD_SYNC")) ? 1 : 0) : -1;
  if (getenv("GM_DIAG_ZERO_ROW")) c->diag_zero_row = atoi(getenv("GM_DIAG_ZERO_ROW"));
  TRY(dalloc(c, &s.msg, cells));        // nibbles: 2 parities x band/2 bytes per (band, row)
  // Escape storage (gm_scaled.h), one set per tick parity: a 16-cell inline slot per (band, row)
  // list (1/32 B per cell at B = 1024) and the pools. The pools are DENSE-equivalent (every
  // list's whole slice fits its stripe's region: no run can overflow them) when that fits the
  // memory budget -- a quarter of the device's free HBM at create, split over the shard count
  // (G column shards of one cluster may share a device: the loopback tests) -- or always up
  // to 2^31 cells. S-A (N = 65,536): 43 GB of dense pools, so a crash of half the cluster (the
  // reference's multifailure schedule, Application.cpp:188-195) escapes every cell it needs.
  // Beyond the budget the pools take what it holds, at least 1/64 of the cells and 1/16 of the
  // payload lanes -- a warm cluster escapes only a crashed node's entries in the ticks before
  // their removal (~10 per list at a 1 % crash: inline) -- and an overflow fails loudly
  // (GM_ERR_ESC -> GM_ERANGE). GM_ESC_CAP (cells; diagnostics, tests) lowers the table pool.
  // Striped: >= 64 (band, row) lists per stripe (up to 1024 stripes), more stripes while a
  // stripe's region exceeds what the list word's offset field addresses (S_EW_REGION_MAX).
  const size_t lists = (size_t)n * s.nb;
  int S = 1024;
  while (S > 1 && lists / S < 64) S >>= 1;
  auto grow = [&](size_t per_stripe_cells_total) {  // stripes so that one region fits the offset field
    while ((per_stripe_cells_total + S - 1) / S > S_EW_REGION_MAX) S <<= 1;
  };
  const size_t dense_t = ((lists + 1023) / 1024) * 1024 * s.band;  // table-pool entries, dense (rounded per stripe)
  const size_t dense_p = dense_t / 16;                              // payload-pool 16-byte slots, dense
  const double dense_bytes = 2.0 * ((double)dense_t * 4 + (double)dense_p * 16);
  size_t free_b = 0, total_b = 0;
  HIPCHECK(hipMemGetInfo(&free_b, &total_b));
  // the free HBM is split over the contexts of this cluster on this device: every shard on one
  // device (loopback) unless the caller says each has its own GPU (device_share = 1, RCCL ranks)
  const int gdev = c->cfg.device_share > 0 ? std::min(c->cfg.device_share, G) : G;
  double budget = (double)free_b / 4 / gdev;
  if (getenv("GM_ESC_BUDGET_GB")) budget = atof(getenv("GM_ESC_BUDGET_GB")) * 1e9;  // diagnostics (tests)
  const bool dense = cells <= (1ull << 31) || dense_bytes <= budget;
  size_t tcells, pslots;
  if (dense) {
    while (((lists + S - 1) / S) * s.band > S_EW_REGION_MAX) S <<= 1;  // the list word's offset field
    const size_t per = (lists + S - 1) / S;  // lists per stripe (at most)
    tcells = per * s.band * S;
    pslots = per * (s.band / 16) * S;
  } else {
    // the table pool takes the fraction f of its dense size and the payload pool min(1, 4f) of its
    // dense count (cells / 16 slots), so at least 1/16 of the payload lanes at the floor f = 1/64
    // (a / 256 here gave 1/256); both parities together fit the budget:
    // 8 f cells + 2 min(1, 4f) cells bytes
    const double cb = (double)cells;
    double f = budget / (16.0 * cb);
    if (f > 0.25) f = (budget - 2.0 * cb) / (8.0 * cb);
    f = std::min(1.0, std::max(1.0 / 64, f));
    tcells = std::max<size_t>((size_t)(cb * f), 4 * (size_t)s.band * S);
    pslots = std::max<size_t>((size_t)(cb * std::min(1.0, 4 * f) / 16), 4 * (size_t)(s.band / 16) * S);
    grow(tcells);
  }
  s.esc_dense = dense ? 1 : 0;
  s.esc_stripes = S;
  size_t treg = std::min<size_t>((tcells + S - 1) / S, S_EW_REGION_MAX);
  size_t preg = std::min<size_t>((pslots + S - 1) / S, 0xFFFFFFF0ull / S);
  if (getenv("GM_ESC_CAP")) treg = std::max<size_t>(1, std::min<size_t>(atol(getenv("GM_ESC_CAP")) / S, treg));
  s.tesc_region = (uint32_t)treg;
  s.pesc_region = (uint32_t)preg;
  s.tesc_cap = treg * S;
  s.pesc_cap = (uint32_t)(preg * S);
  for (int p = 0; p < 2; p++) {
    TRY(dalloc(c, &s.tesc_in[p], lists * S_ESC_IN));
    TRY(dalloc(c, &s.tesc[p], s.tesc_cap));
    TRY(dalloc(c, &s.pesc[p], (size_t)s.pesc_cap * 16));
    TRY(dalloc(c, &s.pesc_rec[p], (size_t)n * s.nb));
  }
  TRY(dalloc(c, &s.tesc_cnt, 2 * (size_t)S));
  TRY(dalloc(c, &s.pesc_cnt, 2 * (size_t)S));
  HIPCHECK(ctx_memset(c, s.tesc_cnt, 0, 2 * S * sizeof(unsigned long long)));
  HIPCHECK(ctx_memset(c, s.pesc_cnt, 0, 2 * S * sizeof(unsigned long long)));
  for (int p = 0; p < 2; p++) {
    TRY(dalloc(c, &s.inbox_cnt[p], n));
    TRY(dalloc(c, &s.inbox[p], (size_t)n * S_KMAX));
  }
  TRY(dalloc(c, &s.hbctr, n));
  TRY(dalloc(c, &s.wtick, n));
  TRY(dalloc(c, &s.failed, n));
  TRY(dalloc(c, &s.brec, (size_t)n * s.nb));
  // the band kernel's fast path (B = 1024; gm_s_band_fast) and the list of units it hands back
  // (at most every unit of a tick). GM_BAND_FAST=0 (diagnostics, A/B against the general path:
  // tests/test_gpu_band_fast.py) leaves it off.
  s.fb_cnt = nullptr;
  s.fb_list = nullptr;
  if (s.band == 1024 && !(getenv("GM_BAND_FAST") && atoi(getenv("GM_BAND_FAST")) == 0)) {
    TRY(dalloc(c, &s.fb_cnt, 2));
    HIPCHECK(ctx_memset(c, s.fb_cnt, 0, 2 * sizeof(uint32_t)));
    TRY(dalloc(c, &s.fb_list, (size_t)n * s.nb));
  }
  // gm_s_pick0 (single context, B = 1024) and the list of rows it leaves to gm_s_pick
  s.pk_list = nullptr;
  s.pk_cnt = nullptr;
  // gm_s_pick0's LDS: per row of the workgroup's 16, the band prefix (nb + 1 words) and the bands'
  // chunk counts (nb x 8 bytes)
  if (s.band == 1024 && !s.sharded && 16 * (sizeof(uint32_t) * (size_t)(s.nb + 1) + sizeof(uint2) * (size_t)s.nb) <= 65536 &&
      !(getenv("GM_PICK0") && atoi(getenv("GM_PICK0")) == 0)) {
    TRY(dalloc(c, &s.pk_list, n));
    TRY(dalloc(c, &s.pk_cnt, 1));
  }
  TRY(dalloc(c, &s.ev_band, (size_t)n * s.nb * s.evs));
  {  // event spill ring (records past a (row, band)'s E slots): up to every cell of the shard, within a
     // 1/32 share of the free HBM (the loopback shards of one device split it); at least 2^24 records.
     // A half-cluster crash at S-A removes ~550 M entries in its peak tick (~420 M past the slots).
    HIPCHECK(hipMemGetInfo(&free_b, &total_b));
    const size_t want = std::min<size_t>((size_t)n * s.wp, free_b / 32 / gdev / sizeof(uint64_t));
    s.ev_spill_cap = (uint32_t)std::min<size_t>(std::max<size_t>(want, 1u << 24), 1ull << 31);
  }
  TRY(dalloc(c, &s.ev_spill, s.ev_spill_cap));
  TRY(dalloc(c, &s.ev_spill_cnt, 1 + S_EV_STRIPES));
  TRY(dalloc(c, &s.evcum, (size_t)n * s.nb));
  TRY(dalloc(c, &s.mtraw, (size_t)n * S_MT_RAW));
  TRY(dalloc(c, &s.rowstat, (size_t)n * 4));
  TRY(dalloc(c, &s.targets, (size_t)n * GM_FANOUT));
  TRY(dalloc(c, &s.err, 1));
  // converged start (cold or warm, gm_config.init_mode); padding columns absent
  const bool warm = c->cfg.init_mode == 1;
  const int t0 = warm ? c->cfg.init_t0 : 0;
  // join ramp (init_mode 2); with keyed drops a joiner can miss its own entry and take
  // updateMyPos's quirk path (MP1Node.cpp:316), handled in gm_s_band within the row's start
  // group (ids 4g..4g+3): column shards never split a group (col0 above)
  const bool ramp = c->cfg.init_mode == 2;
  if (c->cfg.init_mode < 0 || c->cfg.init_mode > 2 || (warm && (t0 < 5 || t0 > GM_T_LIMIT / 2))) return GM_EINVAL;
  if (ramp)
    for (int g = 1; g < G; g++)
      if (col0(g) % 4 != 0) return GM_EUNSUPPORTED;  // n < 8G only
  s.ramp = ramp ? 1 : 0;
  s.intro_until = 0x7FFFFFFF;
  if (ramp) {
    TRY(dalloc(c, &s.mecol, n));
    HIPCHECK(ctx_memset(c, s.mecol, 0xFF, sizeof(int32_t) * n));  // -1: written by the rank owning the row's column
    TRY(dalloc(c, &s.selfadd, S_SELFADD_CAP));
    TRY(dalloc(c, &s.selfadd_cnt, 1));
    HIPCHECK(ctx_memset(c, s.selfadd_cnt, 0, sizeof(uint32_t)));
  }
  HIPCHECK(ctx_memset(c, s.msg, 0, sizeof(uint8_t) * cells));
  for (int p = 0; p < 2; p++) HIPCHECK(ctx_memset(c, s.inbox_cnt[p], 0, sizeof(int32_t) * n));
  HIPCHECK(ctx_memset(c, s.failed, 0, sizeof(int32_t) * n));
  HIPCHECK(ctx_memset(c, s.err, 0, sizeof(uint32_t)));
  HIPCHECK(gm_launch_init(s, ramp ? 2 : warm ? 1 : 0, t0, c->cfg.init_seed, c->stream));  // table, records, pool
  HIPCHECK(hipStreamSynchronize(c->stream));
  uint32_t ierr = 0;
  HIPCHECK(ctx_memcpy(c, &ierr, s.err, sizeof ierr, hipMemcpyDeviceToHost));
  if (ierr) {  // a cold start escapes every cell: beyond the dense-pool size it does not fit
    snprintf(g_errbuf, sizeof g_errbuf, "initial state overflows the escape pool (%zu cells)", s.tesc_cap);
    return GM_ERANGE;
  }
  HIPCHECK(ctx_memset(c, s.ev_spill_cnt, 0, (1 + S_EV_STRIPES) * sizeof(uint32_t)));
  HIPCHECK(ctx_memset(c, s.evcum, 0, sizeof(uint64_t) * (size_t)n * s.nb));
  HIPCHECK(ctx_memset(c, s.rowstat, 0, sizeof(int32_t) * n * 4));
  if (s.sharded) {
    TRY(dalloc(c, &s.acc, (size_t)n * 8));
    TRY(dalloc(c, &s.pending, n));
    // npending, then the pending lists' append counts (plist_cnt[1], [2]): one word block, so the tick's
    // end reads the first two back in one copy
    TRY(dalloc(c, &s.npending, 4));
    s.plist_cnt[1] = (uint32_t *)(s.npending + 1);
    s.plist_cnt[2] = (uint32_t *)(s.npending + 2);
    c->dmax = 64;
    // the exchange's row chunks (tick_sharded pipelines band -> all-gather -> draw -> MAX-allreduce ->
    // acceptance chunk by chunk): 2^xlog rows each (>= 64: a multiple of every band width's rows per
    // unit), K = GM_SCHUNKS chunks, by default 2 (one-box A/B, profiles/r05/ab5: stub shard 7.64 vs 7.76 ms
    // at 4, G = 8 loopback 7.58 vs 7.79 ms per shard-tick)
    {
      int K = getenv("GM_SCHUNKS") ? atoi(getenv("GM_SCHUNKS")) : 2;
      if (K < 1 || K > 64) return GM_EINVAL;
      s.xlog = 6;
      while (((int64_t)1 << s.xlog) * K < n) s.xlog++;
      s.xk = (int)((n + (1 << s.xlog) - 1) >> s.xlog);
    }
    TRY(dalloc(c, &s.xcnt, (size_t)s.xk * G * ((size_t)1 << s.xlog) * 2));
    TRY(dalloc(c, &s.status, (size_t)n * c->dmax));
    // bounded rounds (tick_sharded): round 0 takes every row's first 16 S2 outputs, round 1
    // the next 64 for up to plist_cap rows left pending -- no host round trip per tick
    s.plist_cap[1] = std::min(S_PLIST_CAP, std::max(std::min(n, 1024), n / 16));  // round 1: 64 more outputs
    s.plist_cap[2] = 256;                                             // round 2: 256 more outputs
    if (getenv("GM_PLIST_CAP"))  // diagnostics (tests): smaller lists, so rows overflow to the host-driven rounds
      for (int l = 1; l <= 2; l++) s.plist_cap[l] = std::max(1, std::min(s.plist_cap[l], atoi(getenv("GM_PLIST_CAP"))));
    if (hipHostMalloc(&c->draw_left_h, 2 * sizeof(int32_t), hipHostMallocDefault) != hipSuccess) return GM_ENOMEM;
    c->draw_left_h[0] = c->draw_left_h[1] = 0;
    HIPCHECK(hipEventCreateWithFlags(&c->draw_ev, hipEventDisableTiming));
    for (int l = 1; l <= 2; l++) {
      TRY(dalloc(c, &s.plist[l], s.plist_cap[l]));
      TRY(dalloc(c, &s.statusl[l], (size_t)s.plist_cap[l] * (l == 1 ? GM_D_MORE : GM_D_LAST)));
    }
    HIPCHECK(ctx_memset(c, s.pending, 0, sizeof(int32_t) * n));
    HIPCHECK(ctx_memset(c, s.xcnt, 0, xcnt_bytes(s)));
    TRY(exchange_create(c, s.xk));  // the pipelined exchange
  }
  c->t = t0 + 1;  // the converged table is the state "as of tick t0"
  return GM_OK;
}

void gmh::destroy_scaled(gm_ctx *c) {
  if (c->draw_left_h) (void)hipHostFree(c->draw_left_h);
  if (c->draw_ev) (void)hipEventDestroy(c->draw_ev);
}

// Join ramp: nodeStart of this tick's starters clears bFailed (MP1Node.cpp:108)
int gmh::ramp_starters(gm_ctx *c, hipStream_t st) {
  if (!c->s.ramp) return GM_OK;
  const int j0 = 4 * c->t, j1 = std::min(c->n, 4 * c->t + 4);
  for (int j = j0; j < j1; j++)
    if (c->failed_h[j]) {
      c->failed_h[j] = 0;
      c->fail_t[j] = 0x7FFFFFFF;
      c->nfailed--;
      HIPCHECK(hipMemcpyAsync(c->s.failed + j, c->failed_h.data() + j, sizeof(int32_t), hipMemcpyHostToDevice, st));
    }
  return GM_OK;
}

// SCALED detection recorder: fold tick t's records into the per-subject records and the timeline
// (gm_s_detect), on the stream that ran the tick's band kernels -- after them, and before the next
// tick's prologue zeroes the record counters. Nothing is launched while recording is off.
int gmh::detect_tick(gm_ctx *c, int t, hipStream_t st) {
  if (t >= c->det.tmax) return GM_OK;  // det.tmax 0: off
  HIPCHECK(gm_launch_detect(c->s, c->det.rec, c->det.tl, t, st));
  return GM_OK;
}

int gmh::tick_scaled(gm_ctx *c) {
  if (c->t > GM_T_LIMIT) return GM_ERANGE;
  if (c->s.sharded) return tick_sharded(&c, 1);
  TRY(ramp_starters(c, c->stream));
  const bool drop = drop_tick(c, c->t);
  hipEvent_t k0 = nullptr, k1 = nullptr;
  if (c->timing) TRY(timing_slot(c, &k0, &k1, c->stream));
  HIPCHECK(gm_launch_tick(c->s, c->t, drop ? c->cfg.drop_pct : -1, c->stream, k0, k1, true));
  TRY(detect_tick(c, c->t, c->stream));
  TRY(digest_tick(c, c->t, c->stream));  // while recording: the state the tick leaves, digested
  if (c->s.mc_sent && c->t < c->s.mc_tmax) {
    HIPCHECK(gm_launch_msgcount(c->s, c->t, drop, 0, c->stream));
    HIPCHECK(gm_launch_msgcount(c->s, c->t, drop, 1, c->stream));
  }
  if (c->timing) {
    HIPCHECK(hipEventRecord(c->e1, c->stream));
    c->timed_ticks++;
  }
  return GM_OK;
}
