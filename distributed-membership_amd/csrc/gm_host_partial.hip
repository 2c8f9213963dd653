// gm_host_partial.hip -- PARTIAL host side: the state of gm_partial.hip's kernels, the row shards'
// block capacities and exchange, and the tick of a context or of a loopback group of row shards.
#include <cmath>

#include "gm_host.h"

using namespace gmh;

// PARTIAL: V-entry views (scenario S-C), warm start at init_t0 (oracle op_create).
// shard_count = G > 1: row shard `shard_rank` owns nodes [n*g/G, n*(g+1)/G) and
// exchanges the lists its nodes send to other shards every tick (gm_tick with RCCL
// attached: all-to-all of record counts + two all-to-allv; gm_partial_loopback for
// G contexts on one device).
int gmh::create_partial(gm_ctx *c) {
  const int n = c->n;
  PState &p = c->p;
  p.n = n;
  p.V = c->cfg.view ? c->cfg.view : 32;
  // the per-wave LDS table holds the own list + P_KP delivered lists at <= 0.55 load
  if (p.V < 2 || p.V > 32 || p.V > n) return GM_EUNSUPPORTED;
  const int t0 = c->cfg.init_t0;
  if (c->cfg.init_mode != 1 || t0 < 5 || t0 > GM_T_LIMIT / 2) return GM_EINVAL;
  if (n > (1 << 25) - 1) return GM_EUNSUPPORTED;  // ids live in 25 bits of the LDS table words and wire entries
  const int G = c->cfg.shard_count > 0 ? c->cfg.shard_count : 1;
  const int rank = c->cfg.shard_rank;
  if (rank < 0 || rank >= G || G > n || G > 256) return GM_EINVAL;
  p.G = G;
  p.rank = rank;
  p.n0 = (int)((int64_t)n * rank / G);
  p.nloc = (int)((int64_t)n * (rank + 1) / G) - p.n0;
  p.rows = G > 1 ? p.nloc : n;  // own rows; received lists stay in recv_list (wire format)
  const int nl = p.nloc, R = n - nl;
  p.rd_seed = c->cfg.rd_seed;
  p.view_seed = c->cfg.view_seed;
  p.drop_seed = c->cfg.drop_seed;
  p.drop_pct = -1;
  TRY(dalloc(c, &p.lists, (size_t)2 * p.rows * p.V));
  for (int q = 0; q < 2; q++) {
    TRY(dalloc(c, &p.inbox[q], (size_t)nl * P_KMAX));
    HIPCHECK(ctx_memset(c, p.inbox[q], 0, sizeof(int32_t) * nl * P_KMAX));  // the counts (slot 0) start at 0
    if (G > 1) TRY(dalloc(c, &p.rsrc[q], R));
    if (G == 1) p.rsrc[q] = nullptr;
  }
  TRY(dalloc(c, &p.hbctr, nl));
  TRY(dalloc(c, &p.failed, nl));
  TRY(dalloc(c, &p.ev, (size_t)nl * 2 * p.V));
  TRY(dalloc(c, &p.ev_cnt, nl));
  TRY(dalloc(c, &p.ev_jm, nl));
  TRY(dalloc(c, &p.rowstat, (size_t)nl * 4));
  TRY(dalloc(c, &p.targets, (size_t)nl * GM_FANOUT));
  TRY(dalloc(c, &p.big, nl));
  TRY(dalloc(c, &p.huge, nl));
  TRY(dalloc(c, &p.err, 1));
  TRY(dalloc(c, &c->ph.mtraw, (size_t)nl * 16 * 2));
  {  // the S2 prefetch for tick t+1 runs beside tick t's kernels: at the lowest stream priority it
     // takes the CUs the tick leaves idle instead of competing for them (GM_SIDE_PRIO=0: default)
    int lo = 0, hi = 0;
    HIPCHECK(hipDeviceGetStreamPriorityRange(&lo, &hi));
    const bool low = !(getenv("GM_SIDE_PRIO") && !atoi(getenv("GM_SIDE_PRIO")));
    HIPCHECK(hipStreamCreateWithPriority(&c->ph.side, hipStreamNonBlocking, low ? lo : 0));
  }
  for (int q = 0; q < 2; q++) {
    HIPCHECK(hipEventCreateWithFlags(&c->ph.tickev[q], hipEventDisableTiming));
    HIPCHECK(hipEventCreateWithFlags(&c->ph.mtev[q], hipEventDisableTiming));
  }
  c->ph.sharded = G > 1 || (getenv("GM_FORCE_SHARD") && atoi(getenv("GM_FORCE_SHARD")) == 1);
  // row shards pipeline their exchange over K chunks of their nodes (GM_CHUNKS, default 4)
  p.nchunk = c->ph.sharded ? (getenv("GM_CHUNKS") ? atoi(getenv("GM_CHUNKS")) : 4) : 1;
  p.kcap = inbox_cap(P_KMAX - 1);
  if (p.nchunk < 1 || p.nchunk > 64) return GM_EINVAL;
  TRY(dalloc(c, &p.big_cnt, p.nchunk));
  TRY(dalloc(c, &p.huge_cnt, p.nchunk));
  if (c->ph.sharded) {
    TRY(exchange_create(c, p.nchunk));
    TRY(dalloc(c, &p.pk_hdr, (size_t)G * nl * 8));
    TRY(dalloc(c, &p.pk_list, (size_t)G * nl * p.V));
    HIPCHECK(ctx_memset(c, p.pk_hdr, 0xFF, sizeof(int32_t) * G * nl * 8));
    TRY(dalloc(c, &p.pk_cnt, (size_t)p.nchunk * G));
    TRY(dalloc(c, &p.pk_cap, (size_t)p.nchunk * G));
    p.xcap_frac = getenv("GM_XCHG_CAP_FRAC") ? (float)atof(getenv("GM_XCHG_CAP_FRAC")) : 0.f;
    if (p.xcap_frac < 0.f || p.xcap_frac > 1.f) return GM_EINVAL;
    TRY(dalloc(c, &p.recv_hdr, (size_t)std::max(R, 1) * 8));
    for (int q = 0; q < 2; q++) TRY(dalloc(c, &p.recv_list[q], (size_t)std::max(R, 1) * p.V));
    std::vector<int32_t> b(G + 1);
    for (int g = 0; g <= G; g++) b[g] = (int32_t)((int64_t)n * g / G);
    TRY(dalloc(c, &p.shard_n0, G + 1));
    HIPCHECK(ctx_memcpy(c, p.shard_n0, b.data(), sizeof(int32_t) * (G + 1), hipMemcpyHostToDevice));
    TRY(partial_caps(c));
  }
  HIPCHECK(ctx_memset(c, p.lists, 0, sizeof(uint64_t) * 2 * p.rows * p.V));
  HIPCHECK(ctx_memset(c, p.failed, 0, sizeof(int32_t) * nl));
  HIPCHECK(ctx_memset(c, p.ev_cnt, 0, sizeof(int32_t) * nl));
  HIPCHECK(ctx_memset(c, p.ev_jm, 0, sizeof(uint32_t) * nl));
  HIPCHECK(ctx_memset(c, p.rowstat, 0, sizeof(int32_t) * nl * 4));
  HIPCHECK(ctx_memset(c, p.err, 0, sizeof(uint32_t)));
  HIPCHECK(gm_launch_partial_init(p, t0, c->cfg.init_seed, c->stream));
  HIPCHECK(hipStreamSynchronize(c->stream));
  c->t = t0 + 1;
  return GM_OK;
}

void gmh::destroy_partial(gm_ctx *c) {
  if (c->ph.side) {
    (void)hipStreamSynchronize(c->ph.side);
    (void)hipStreamDestroy(c->ph.side);
  }
  for (int q = 0; q < 2; q++) {
    if (c->ph.tickev[q]) (void)hipEventDestroy(c->ph.tickev[q]);
    if (c->ph.mtev[q]) (void)hipEventDestroy(c->ph.mtev[q]);
  }
}

// ------------------------------------------------------------ PARTIAL row shards
// After chunk c's local kernels of tick t, gm_p_pack (on the comm stream) builds the records the
// chunk's nodes address to each other shard q -- from their targets and their final lists of the
// tick, no record written by the node kernels -- packed to the front of block (q, r0_c), whose
// capacity every rank knows (xcap). The exchange sends the blocks with two all-to-allv -- headers,
// then lists (wire format) into recv_list[t&1], where tick t+1 reads its senders' lists -- and
// gm_p_unpack appends each received record whose stamp is t to its targets' inboxes (rows of a block
// past its records keep older stamps), while later chunks compute. No host round trip.
// Capacity of a packed block (gm_p_pack): the records one chunk of `rows` senders addresses to
// shard q. A sender's five targets are drawn from its view; with a fraction f_q of the view's
// entries on shard q it addresses q with probability 1 - (1 - f_q)^5, so the block's record count is
// a sum of Bernoullis whose mean is at most rows * (1 - (1 - E f_q)^5) (the map is concave) and
// whose variance is at most the binomial's. E f_q: views follow the live nodes once the crashed
// ones are swept out, and hold the static shares before -- so f_q = max(n_q / n, live_q / live) (a
// crashed shard keeps its static share; ADVICE r4: a contiguous half-cluster crash, the
// reference's multifailure schedule, Application.cpp:189-192, leaves the survivors addressing each
// surviving shard with ~76 % at G = 8, past the static 49 %). The block holds the mean + 8 sigma +
// 64 (at most the slots); every rank derives the same capacities from the same crash set, and an
// overflow fails loudly (GM_ERR_XCHG).
static size_t xcap(const gm_ctx *c, size_t rows, int q) {
  const PState &p = c->p;
  if (p.xcap_frac > 0.f) return std::min(rows, (size_t)std::ceil((double)rows * p.xcap_frac));
  const double pq = c->ph.xq[q];
  const double m = (double)rows * pq + 8.0 * std::sqrt((double)rows * pq * (1.0 - pq)) + 64.0;
  return std::min(rows, (size_t)std::ceil(m));
}
struct XChunk {  // the block layout of chunk ch (rows of shard g in chunk ch: [nloc_g ch / K, nloc_g (ch+1) / K))
  std::vector<size_t> sc, sd, rc, rd;  // send / receive record counts (block capacities) and row offsets per shard
  size_t rbase = 0, rrows = 0;         // this chunk's first received row, rows received
};
static XChunk xchunk(const gm_ctx *c, int ch) {
  const PState &p = c->p;
  const int G = p.G, K = p.nchunk;
  auto nloc_of = [&](int g) { return (int64_t)p.n * (g + 1) / G - (int64_t)p.n * g / G; };
  auto rows = [&](int g, int cc) { return (size_t)(nloc_of(g) * (cc + 1) / K - nloc_of(g) * cc / K); };
  XChunk x;
  x.sc.assign(G, 0); x.sd.assign(G, 0); x.rc.assign(G, 0); x.rd.assign(G, 0);
  for (int cc = 0; cc < ch; cc++)
    for (int g = 0; g < G; g++)
      if (g != p.rank) x.rbase += xcap(c, rows(g, cc), p.rank);
  const size_t r0 = (size_t)((int64_t)p.nloc * ch / K);
  size_t off = x.rbase;
  for (int q = 0; q < G; q++) {
    if (q == p.rank) continue;
    x.sc[q] = xcap(c, rows(p.rank, ch), q);
    x.sd[q] = (size_t)q * p.nloc + r0;  // the packed block (q, r0) of pk_hdr / pk_list
    x.rc[q] = xcap(c, rows(q, ch), p.rank);
    x.rd[q] = off;
    off += x.rc[q];
  }
  x.rrows = off - x.rbase;
  return x;
}

// the address probabilities per shard from the crash set (every rank holds the whole set), and the
// outgoing block capacities per (chunk, peer) on the device (gm_p_pack reads them)
int gmh::partial_caps(gm_ctx *c) {
  const PState &p = c->p;
  const int G = p.G;
  std::vector<int64_t> live(G, 0);
  int64_t tot = 0;
  for (int g = 0; g < G; g++) {
    const int a = (int)((int64_t)p.n * g / G), b = (int)((int64_t)p.n * (g + 1) / G);
    for (int i = a; i < b; i++) live[g] += c->failed_h[i] ? 0 : 1;
    tot += live[g];
  }
  uint64_t h = 0x9E3779B97F4A7C15ull;  // the crash set every rank must hold (the capacities follow from it)
  for (int i = 0; i < p.n; i++)
    if (c->failed_h[i]) h = (h ^ (uint64_t)(uint32_t)i) * 0x100000001B3ull + 0x632BE59BD9B4E019ull;
  c->ph.crash_hash = h;
  c->ph.crash_check = true;
  c->ph.xq.assign(G, 0.0);
  for (int g = 0; g < G; g++) {
    const double fs = (double)((int64_t)p.n * (g + 1) / G - (int64_t)p.n * g / G) / p.n;
    const double fl = tot > 0 ? (double)live[g] / tot : 0.0;
    c->ph.xq[g] = 1.0 - std::pow(1.0 - std::max(fs, fl), (double)GM_FANOUT);
  }
  std::vector<int32_t> cap((size_t)p.nchunk * G, 0);
  for (int ch = 0; ch < p.nchunk; ch++) {
    const XChunk x = xchunk(c, ch);
    for (int q = 0; q < G; q++) cap[(size_t)ch * G + q] = (int32_t)x.sc[q];
  }
  HIPCHECK(ctx_memcpy(c, p.pk_cap, cap.data(), sizeof(int32_t) * cap.size(), hipMemcpyHostToDevice));
  return GM_OK;
}

// The block capacities (send counts of a rank, receive counts of its peers) derive from the crash
// set each rank was given (gm_set_failed): a rank holding another set would size its ncclAllToAllv
// differently and hang or corrupt it. After each change the group agrees on the set's hash -- an RCCL
// rank by one MAX-allreduce of (h, ~h), a loopback group on the host -- and any disagreement latches
// GM_ESTATE on every member.
// A loaded view state (gm_load_views_commit) rides along: its commit changes the crash set's hash
// check too, and the "exchange pending" flag of every member must agree -- the replayed exchange of
// tick t - 1 is a collective like any other. RCCL ranks carry the flag as words 2, 3 of the all-reduce.
static int px_agree(gm_ctx **g, int G, hipStream_t st) {
  bool same = true;
  if (G == 1) {
    gm_ctx *c = g[0];
    if (!c->ph.crash_dev) {
      HIPCHECK(hipMalloc(&c->ph.crash_dev, 4 * sizeof(uint64_t)));
      c->allocs.push_back(c->ph.crash_dev);
    }
    const uint64_t pend = c->vl.xpending ? 1 : 0;
    uint64_t hv[4] = {c->ph.crash_hash, ~c->ph.crash_hash, pend, ~pend}, mx[4] = {0, 0, 0, 0};
    HIPCHECK(hipMemcpyAsync(c->ph.crash_dev, hv, sizeof hv, hipMemcpyHostToDevice, st));
    NCCLCHECK(ncclAllReduce(c->ph.crash_dev, c->ph.crash_dev, 4, ncclUint64, ncclMax, c->comm, st));
    HIPCHECK(hipMemcpyAsync(mx, c->ph.crash_dev, sizeof mx, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
    same = mx[0] == hv[0] && mx[1] == hv[1] && mx[2] == hv[2] && mx[3] == hv[3];
  }
  for (int i = 1; i < G; i++)
    same &= g[i]->ph.crash_hash == g[0]->ph.crash_hash && g[i]->vl.xpending == g[0]->vl.xpending;
  for (int i = 0; i < G && !same; i++) g[i]->latched = GM_ESTATE;
  return same ? GM_OK : GM_ESTATE;
}

// The exchange of chunk ch on the comm stream: every member packs, then each member receives its
// blocks -- two ncclAllToAllv for an RCCL rank, device copies from its peers' packed blocks in a
// loopback group (same layout; both sides must have sized the block alike) -- and unpacks them.
// t: the tick whose sends travel -- the group's current tick, or the tick before it when a loaded
// state's exchange is replayed.
static int px_exchange(gm_ctx **g, int G, int ch, hipStream_t cs, int t) {
  const int V = g[0]->p.V;
  for (int i = 0; i < G; i++) {
    const PState &p = g[i]->p;
    if (ch == 0) HIPCHECK(hipMemsetAsync(p.pk_cnt, 0, sizeof(int32_t) * p.nchunk * p.G, cs));
    HIPCHECK(gm_launch_partial_pack(p, t, ch, cs));
  }
  for (int i = 0; i < G; i++) {
    gm_ctx *c = g[i];
    const PState &p = c->p;
    const XChunk x = xchunk(c, ch);
    if (x.rbase + x.rrows > (size_t)(p.n - p.nloc)) return GM_ESTATE;
    if (G == 1) {
      const int W = p.G;
      std::vector<size_t> hs(W), hsd(W), hr(W), hrd(W), ls(W), lsd(W), lr(W), lrd(W);
      for (int q = 0; q < W; q++) {
        hs[q] = x.sc[q] * 8;
        hsd[q] = x.sd[q] * 8;
        hr[q] = x.rc[q] * 8;
        hrd[q] = x.rd[q] * 8;
        ls[q] = x.sc[q] * V;
        lsd[q] = x.sd[q] * V;
        lr[q] = x.rc[q] * V;
        lrd[q] = x.rd[q] * V;
      }
      NCCLCHECK(ncclAllToAllv(p.pk_hdr, hs.data(), hsd.data(), p.recv_hdr, hr.data(), hrd.data(), ncclInt32, c->comm, cs));
      NCCLCHECK(ncclAllToAllv(p.pk_list, ls.data(), lsd.data(), p.recv_list[t & 1], lr.data(), lrd.data(), ncclUint32,
                              c->comm, cs));
    }
    for (int j = 0; j < G; j++) {
      if (j == i || !x.rc[j]) continue;
      const XChunk xj = xchunk(g[j], ch);
      const PState &pj = g[j]->p;
      if (xj.sc[i] != x.rc[j]) return GM_ESTATE;
      HIPCHECK(hipMemcpyAsync(p.recv_hdr + x.rd[j] * 8, pj.pk_hdr + xj.sd[i] * 8, sizeof(int32_t) * 8 * x.rc[j],
                              hipMemcpyDeviceToDevice, cs));
      HIPCHECK(hipMemcpyAsync(p.recv_list[t & 1] + x.rd[j] * V, pj.pk_list + xj.sd[i] * V, sizeof(uint32_t) * V * x.rc[j],
                              hipMemcpyDeviceToDevice, cs));
    }
    HIPCHECK(gm_launch_partial_unpack(p, t, (int)x.rbase, (int)x.rrows, cs));
    c->ph.recv_last = (int64_t)(x.rbase + x.rrows);  // the last chunk's: every list received this tick
  }
  return GM_OK;
}

// One PARTIAL tick of a group: an unsharded context, one RCCL row shard, or the G row shards of a
// loopback cluster. A loopback group runs shard after shard on its first member's streams: the sum
// of the shards' own costs (8 concurrent stream pairs on one device starve each other's small
// worklist kernels; on a node every shard has its GPU to itself). Timing events are the first
// member's (they bracket the whole group's kernels).
int gmh::tick_partial(gm_ctx **g, int G) {
  gm_ctx *L = g[0];
  if (L->t > GM_T_LIMIT) return GM_ERANGE;
  if (G == 1 && L->ph.sharded && !L->comm) return GM_EUNSUPPORTED;  // row shards need gm_comm_init (or gm_partial_loopback_tick)
  hipStream_t st = L->stream;
  const int t = L->t, par = t & 1, K = L->p.nchunk;
  auto mt = [&](gm_ctx *c, int q) { return c->ph.mtraw + (size_t)q * c->p.nloc * 16; };
  hipEvent_t k0 = nullptr, k1 = nullptr;
  if (L->timing) TRY(timing_slot(L, &k0, &k1, st));
  // S2 outputs of this tick: prefetched on the side stream while the last tick ran
  // (they depend only on (seed, t, id)), else computed here
  for (int i = 0; i < G; i++) {
    gm_ctx *c = g[i];
    c->p.drop_pct = drop_tick(c, t) ? c->cfg.drop_pct : -1;  // read by this tick's node kernels only
    if (c->ph.mt_next == t) {
      HIPCHECK(hipStreamWaitEvent(st, L->ph.mtev[par], 0));
      HIPCHECK(gm_launch_partial_reset(c->p, st));
    } else {
      HIPCHECK(gm_launch_partial_mtgen(c->p, t, mt(c, par), st, true));
    }
  }
  if (k0) HIPCHECK(hipEventRecord(k0, st));
  if (!L->ph.sharded) {
    HIPCHECK(gm_launch_partial_chunk(L->p, t, mt(L, par), 0, st));
    TRY(view_detect_tick(L, t, st));  // while recording: the tick's final views and records, reduced
    TRY(digest_tick(L, t, st));       // while recording: the state the tick leaves, digested
    if (k1) HIPCHECK(hipEventRecord(k1, st));
  } else {
    bool check = false;
    for (int i = 0; i < G; i++) {
      check |= g[i]->ph.crash_check;
      g[i]->ph.crash_check = false;
    }
    bool pend = false;
    for (int i = 0; i < G; i++) pend |= g[i]->vl.xpending;
    if (check || pend) TRY(px_agree(g, G, st));  // (a commit always asks for the check: partial_caps)
    if (pend) {
      // a loaded state: the received lists and the remote half of the inboxes of tick t are what
      // tick t - 1's exchange delivered. Replay it from what the commit wrote -- targets,
      // rowstat[.][3], lists[(t - 1) & 1] -- for all K chunks on the comm stream, before this tick's work
      HIPCHECK(hipEventRecord(L->xch.done, st));
      HIPCHECK(hipStreamWaitEvent(L->xch.stream, L->xch.done, 0));
      for (int q = 0; q < K; q++) TRY(px_exchange(g, G, q, L->xch.stream, t - 1));
      HIPCHECK(hipEventRecord(L->xch.done, L->xch.stream));
      HIPCHECK(hipStreamWaitEvent(st, L->xch.done, 0));
      for (int i = 0; i < G; i++) g[i]->vl.xpending = false;
    }
    // chunk pipeline: every chunk's node ticks queue on the compute stream; the exchange of
    // chunk q runs on the comm stream once q's kernels are done, while q+1.. still compute
    for (int q = 0; q < K; q++) {
      for (int i = 0; i < G; i++) HIPCHECK(gm_launch_partial_chunk(g[i]->p, t, mt(g[i], par), q, st));
      HIPCHECK(hipEventRecord(L->xch.chunk_ev[q], st));
    }
    // while recording: every member's reducer behind the last chunk's node kernels, on the compute
    // stream beside the exchange (which only reads what the reducer reads)
    for (int i = 0; i < G; i++) TRY(view_detect_tick(g[i], t, st));
    for (int i = 0; i < G; i++) TRY(digest_tick(g[i], t, st));  // reads what the node kernels left, as the reducer
    if (k1) HIPCHECK(hipEventRecord(k1, st));
    for (int q = 0; q < K; q++) {
      HIPCHECK(hipStreamWaitEvent(L->xch.stream, L->xch.chunk_ev[q], 0));
      TRY(px_exchange(g, G, q, L->xch.stream, t));
    }
    HIPCHECK(hipEventRecord(L->xch.done, L->xch.stream));
    HIPCHECK(hipStreamWaitEvent(st, L->xch.done, 0));  // the next tick reads the unpacked inboxes
  }
  // prefetch tick t+1's S2 outputs into the other parity buffer, last read by tick t-1
  HIPCHECK(hipEventRecord(L->ph.tickev[par], st));
  HIPCHECK(hipStreamWaitEvent(L->ph.side, L->ph.tickev[par ^ 1], 0));
  for (int i = 0; i < G; i++) {
    HIPCHECK(gm_launch_partial_mtgen(g[i]->p, t + 1, mt(g[i], par ^ 1), L->ph.side, false));
    g[i]->ph.mt_next = t + 1;
  }
  HIPCHECK(hipEventRecord(L->ph.mtev[par ^ 1], L->ph.side));
  if (L->timing) {
    HIPCHECK(hipEventRecord(L->e1, st));
    L->timed_ticks++;
  }
  return GM_OK;
}

// One PARTIAL tick of the G row-shard contexts of one cluster living on one device (tests,
// scripts/partial_shard_profile.py): the tick gm_tick runs per rank (tick_partial), the exchange by
// device copies instead of RCCL. A device error of the tick (an overflowing block: GM_ERANGE) is
// returned by this call.
extern "C" int gm_partial_loopback_tick(gm_ctx **ctxs, int32_t G) {
  if (!ctxs || G < 2) return GM_EINVAL;
  for (int g = 0; g < G; g++) {
    gm_ctx *c = ctxs[g];
    if (!c || c->cfg.mode != GM_MODE_PARTIAL || c->p.G != G || c->p.rank != g || c->t != ctxs[0]->t ||
        c->n != ctxs[0]->n || c->p.V != ctxs[0]->p.V || c->p.nchunk != ctxs[0]->p.nchunk)
      return GM_EINVAL;
    if (c->latched != GM_OK) return c->latched;
    if (c->vl.loading) return GM_ESTATE;  // between gm_load_views_begin and gm_load_views_commit
  }
  for (int g = 0; g < G; g++) TRY(before_tick_events(ctxs[g]));
  for (int g = 0; g < G; g++) HIPCHECK(hipStreamSynchronize(ctxs[g]->stream));  // the tick runs on the first member's streams
  const int rc = tick_partial(ctxs, G);
  HIPCHECK(hipStreamSynchronize(ctxs[0]->stream));
  HIPCHECK(hipStreamSynchronize(ctxs[0]->ph.side));  // the prefetch writes every member's S2 buffer
  TRY(rc);
  for (int g = 0; g < G; g++) {
    TRY(check_err(ctxs[g]));
    advance(ctxs[g]);
  }
  return GM_OK;
}

extern "C" int gm_shard_exchange_bytes(gm_ctx *c, int64_t *bytes) {
  if (!c || !bytes) return GM_EINVAL;
  *bytes = 0;
  if (c->cfg.mode == GM_MODE_PARTIAL)  // record slots received in the last tick: 32 B header + the V-entry list
    *bytes = c->ph.recv_last * (int64_t)(32 + 4 * c->p.V);
  return GM_OK;
}
