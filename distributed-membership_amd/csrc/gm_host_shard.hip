// gm_host_shard.hip -- SCALED column shards: attaching RCCL, the phase API, the sharded tick and its
// draw rounds, and the loopback groups.
//
// A tick of a column shard: merge/sweep own columns, all-gather per-row counts,
// then rounds of {draw, MAX-allreduce of resolved draws, accept} until every row
// has its targets. Collectives are RCCL on the context stream (gm_comm_init),
// or in-process between contexts of one device (gm_shard_loopback, tests).
#include <utility>

#include "gm_host.h"

using namespace gmh;

extern "C" int gm_comm_unique_id(uint8_t *out128) {
  if (!out128) return GM_EINVAL;
  ncclUniqueId id;
  NCCLCHECK(ncclGetUniqueId(&id));
  memcpy(out128, &id, sizeof id);
  return GM_OK;
}

extern "C" int gm_comm_init(gm_ctx *c, const uint8_t *id128, int32_t nranks, int32_t rank) {
  if (!c || !id128) return GM_EINVAL;
  if (c->cfg.mode == GM_MODE_SCALED ? (c->s.shard_count != nranks || c->s.shard_rank != rank)
      : c->cfg.mode == GM_MODE_PARTIAL ? (c->p.G != nranks || c->p.rank != rank) : true)
    return GM_EINVAL;
  if (c->comm) return GM_OK;
  ncclUniqueId id;
  memcpy(&id, id128, sizeof id);
  HIPCHECK(hipSetDevice(c->cfg.device));
  NCCLCHECK(ncclCommInitRank(&c->comm, nranks, id, rank));
  // Every rank must run the same cluster: the collectives' sizes follow from n, the band width
  // (column shards) and the chunk count (row shards, GM_CHUNKS), and the replayed draws from the
  // seeds. One all-gather of a config signature; a rank that disagrees fails here (GM_EINVAL)
  // instead of hanging or corrupting an all-to-allv later.
  const gm_config &g = c->cfg;
  const int64_t sig[GM_SIG_WORDS] = {g.mode, g.n, c->s.band, c->p.V, c->p.nchunk, (int64_t)g.rd_seed, g.drop_pct,
                                     g.drop_from, g.drop_to, (int64_t)g.drop_seed, g.init_mode, g.init_t0,
                                     (int64_t)g.init_seed, (int64_t)g.view_seed, c->ph.sharded, GM_ABI_VERSION,
                                     (int64_t)(c->p.xcap_frac * 1e6f)};
  int64_t *dsig = nullptr;
  HIPCHECK(hipMalloc(&dsig, sizeof(int64_t) * GM_SIG_WORDS * (nranks + 1)));
  std::vector<int64_t> all((size_t)GM_SIG_WORDS * nranks);
  int rc = GM_OK;
  if (hipMemcpyAsync(dsig, sig, sizeof sig, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
      ncclAllGather(dsig, dsig + GM_SIG_WORDS, GM_SIG_WORDS, ncclInt64, c->comm, c->stream) != ncclSuccess ||
      hipMemcpyAsync(all.data(), dsig + GM_SIG_WORDS, sizeof(int64_t) * all.size(), hipMemcpyDeviceToHost,
                     c->stream) != hipSuccess ||
      hipStreamSynchronize(c->stream) != hipSuccess) {
    snprintf(g_errbuf, sizeof g_errbuf, "gm_comm_init: config all-gather failed");
    rc = GM_ECOMM;
  }
  (void)hipFree(dsig);
  for (int r = 0; rc == GM_OK && r < nranks; r++)
    for (int k = 0; k < GM_SIG_WORDS; k++)
      if (all[(size_t)r * GM_SIG_WORDS + k] != sig[k]) {
        snprintf(g_errbuf, sizeof g_errbuf, "gm_comm_init: rank %d disagrees on config word %d (%lld vs %lld)", r,
                 k, (long long)all[(size_t)r * GM_SIG_WORDS + k], (long long)sig[k]);
        rc = GM_EINVAL;
        break;
      }
  if (rc != GM_OK) {
    (void)ncclCommDestroy(c->comm);
    c->comm = nullptr;
  }
  return rc;
}

extern "C" int gm_comm_info(gm_ctx *c, int32_t info[4]) {
  if (!c || !info) return GM_EINVAL;
  if (!c->comm) {
    info[0] = 0, info[1] = -1, info[2] = -1, info[3] = c->cfg.device;
    return GM_OK;
  }
  int cnt = 0, rk = 0, dev = 0;
  NCCLCHECK(ncclCommCount(c->comm, &cnt));
  NCCLCHECK(ncclCommUserRank(c->comm, &rk));
  NCCLCHECK(ncclCommCuDevice(c->comm, &dev));
  info[0] = cnt, info[1] = rk, info[2] = dev, info[3] = c->cfg.device;
  return GM_OK;
}

extern "C" int gm_shard_layout(gm_ctx *c, int32_t *c0, int32_t *w) {
  if (c && c0 && w && c->cfg.mode == GM_MODE_PARTIAL) {  // row shard: nodes [n0, n0 + nloc)
    *c0 = c->p.n0;
    *w = c->p.nloc;
    return GM_OK;
  }
  if (!c || !c0 || !w || c->cfg.mode != GM_MODE_SCALED) return GM_EINVAL;
  *c0 = c->s.c0;
  *w = c->s.w;
  return GM_OK;
}

static int shard_ready(gm_ctx *c) {
  if (!c || c->cfg.mode != GM_MODE_SCALED || !c->s.sharded) return GM_EINVAL;
  if (c->latched != GM_OK) return c->latched;
  if (c->ld.loading) return GM_ESTATE;  // between gm_load_begin and gm_load_commit
  if (c->t > GM_T_LIMIT) return GM_ERANGE;
  return GM_OK;
}

// the unchunked merge of one shard: its band kernels over every row, its row totals
static int shard_merge(gm_ctx *c, hipStream_t st) {
  TRY(ramp_starters(c, st));
  const bool drop = drop_tick(c, c->t);
  HIPCHECK(hipMemsetAsync(c->s.xcnt, 0, xcnt_bytes(c->s), st));
  hipEvent_t k0 = nullptr, k1 = nullptr;
  if (c->timing) TRY(timing_slot(c, &k0, &k1, st));
  HIPCHECK(gm_launch_tick(c->s, c->t, drop ? c->cfg.drop_pct : -1, st, k0, k1, false));
  TRY(detect_tick(c, c->t, st));
  HIPCHECK(gm_launch_xrows(c->s, 0, c->n, st));  // this shard's row totals for the all-gather
  // msgcount: this shard's fresh counts (its columns), SUM-allreduced before the draws
  if (mc_on(c, c->t)) HIPCHECK(gm_launch_msgcount(c->s, c->t, drop, 0, st));
  return GM_OK;
}

extern "C" int gm_shard_merge(gm_ctx *c) {
  TRY(shard_ready(c));
  TRY(before_tick_events(c));
  return shard_merge(c, c->stream);
}

extern "C" int gm_shard_draw(gm_ctx *c, int32_t round, int32_t D) {
  TRY(shard_ready(c));
  // round 0 covers the precomputed S2 outputs [0, 16), round q >= 1 outputs [16 + 64(q-1), 16 + 64q)
  if (round < 0 || D != (round == 0 ? GM_D_FIRST : GM_D_MORE)) return GM_EINVAL;
  HIPCHECK(gm_launch_draw(c->s, c->t, round, D, 0, c->stream));
  return GM_OK;
}

extern "C" int gm_shard_accept(gm_ctx *c, int32_t D, int32_t *npending) {
  TRY(shard_ready(c));
  if (D <= 0 || D > c->dmax || !npending) return GM_EINVAL;
  HIPCHECK(hipMemsetAsync(c->s.npending, 0, sizeof(int32_t), c->stream));
  HIPCHECK(gm_launch_accept(c->s, c->t, D, 0, 0, c->stream));
  HIPCHECK(hipMemcpyAsync(npending, c->s.npending, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHECK(hipStreamSynchronize(c->stream));
  return GM_OK;
}

// The last device work of a shard's tick c->t; time does not advance here (gm_tick, the loopback
// driver and gm_shard_end_tick do that).
static int shard_finish(gm_ctx *c, hipStream_t st) {
  // msgcount: sent / received once the targets are final (after draw_settle when bounded
  // rounds left rows to the host-driven loop)
  if (!c->draw_check && mc_on(c, c->t)) HIPCHECK(gm_launch_msgcount(c->s, c->t, drop_tick(c, c->t), 1, st));
  if (c->timing) {  // band-kernel events are in the timing ring (no host wait here)
    HIPCHECK(hipEventRecord(c->e1, st));
    c->timed_ticks++;
  }
  return GM_OK;
}

extern "C" int gm_shard_end_tick(gm_ctx *c) {
  TRY(shard_ready(c));
  TRY(shard_finish(c, c->stream));
  advance(c);
  return GM_OK;
}

__global__ void gm_max_into(int32_t *dst, const int32_t *src, size_t n) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    dst[i] = max(dst[i], src[i]);
}
__global__ void gm_add_into(uint32_t *dst, const uint32_t *src, size_t n) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    dst[i] += src[i];
}
__global__ void gm_xc_mirror(int32_t *chunk, int rank, int G, size_t words) {  // stub all-gather
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < words; i += (size_t)gridDim.x * blockDim.x) {
    const int32_t v = chunk[(size_t)rank * words + i];
    for (int g = 0; g < G; g++)
      if (g != rank) chunk[(size_t)g * words + i] = v;
  }
}

// The column shards' group collectives, enqueued on st. A group of one is a rank of an RCCL
// communicator (in-place collectives) or the stub (no peers: the all-gather mirrors its slot, the
// reductions are the identity); a group of G > 1 is a whole loopback cluster on one device: device
// copies, and reductions into member 0 copied back to the others.
//
// all-gather of every shard's per-row (present, numfailed) for exchange chunk ch
static int grp_allgather(gm_ctx **g, int G, int ch, hipStream_t st) {
  const SState &s = g[0]->s;
  const size_t r0 = (size_t)ch << s.xlog;
  if (G > 1) {
    const size_t bytes = sizeof(int32_t) * 2 * xchunk_rows(s, ch);
    for (int dst = 0; dst < G; dst++)
      for (int src = 0; src < G; src++)
        if (src != dst) {
          const size_t o = S_XC(s, src, r0);
          HIPCHECK(hipMemcpyAsync(g[dst]->s.xcnt + o, g[src]->s.xcnt + o, bytes, hipMemcpyDeviceToDevice, st));
        }
  } else if (s.stub) {  // one kernel mirrors the chunk's slot into every peer slot (the all-gather's local cost)
    hipLaunchKernelGGL(gm_xc_mirror, dim3(256), dim3(256), 0, st, s.xcnt + S_XC(s, 0, r0), s.shard_rank,
                       s.shard_count, (size_t)2 << s.xlog);
    HIPCHECK(hipGetLastError());
  } else {  // chunk-major: the chunk's slots are contiguous, rank q's at q << xlog rows -- in place
    NCCLCHECK(ncclAllGather(s.xcnt + S_XC(s, s.shard_rank, r0), s.xcnt + S_XC(s, 0, r0), (size_t)2 << s.xlog, ncclInt32,
                            g[0]->comm, st));
  }
  return GM_OK;
}

// MAX-reduce of the resolved draws: cnt words at off of status (l = 0) or of statusl[l]
static int grp_max(gm_ctx **g, int G, int l, size_t off, size_t cnt, hipStream_t st) {
  auto buf = [&](int i) { return (l ? g[i]->s.statusl[l] : g[i]->s.status) + off; };
  if (G == 1) {
    if (!g[0]->s.stub) NCCLCHECK(ncclAllReduce(buf(0), buf(0), cnt, ncclInt32, ncclMax, g[0]->comm, st));
    return GM_OK;
  }
  for (int i = 1; i < G && cnt; i++) hipLaunchKernelGGL(gm_max_into, dim3(256), dim3(256), 0, st, buf(0), buf(i), cnt);
  for (int i = 1; i < G && cnt; i++)
    HIPCHECK(hipMemcpyAsync(buf(i), buf(0), sizeof(int32_t) * cnt, hipMemcpyDeviceToDevice, st));
  HIPCHECK(hipGetLastError());
  return GM_OK;
}

// msgcount: SUM-reduce of tick t's whole-row fresh counts (and of the kept entries on a loss tick)
static int grp_mc_sum(gm_ctx **g, int G, int t, hipStream_t st) {
  const size_t n = (size_t)g[0]->n;
  for (int k = 0; k < (drop_tick(g[0], t) ? 2 : 1); k++) {
    auto buf = [&](int i) { return k == 0 ? g[i]->s.mc_fresh + (size_t)(t & 1) * n : g[i]->s.mc_rdrop; };
    if (G == 1) {
      if (!g[0]->s.stub) NCCLCHECK(ncclAllReduce(buf(0), buf(0), n, ncclUint32, ncclSum, g[0]->comm, st));
      continue;
    }
    for (int i = 1; i < G; i++) hipLaunchKernelGGL(gm_add_into, dim3(64), dim3(256), 0, st, buf(0), buf(i), n);
    for (int i = 1; i < G; i++) HIPCHECK(hipMemcpyAsync(buf(i), buf(0), sizeof(uint32_t) * n, hipMemcpyDeviceToDevice, st));
  }
  HIPCHECK(hipGetLastError());
  return GM_OK;
}

// a loopback cluster: every shard of one SCALED cluster, in rank order, each ready to tick
static int shard_group_ready(gm_ctx **ctxs, int G) {
  if (!ctxs || G < 2) return GM_EINVAL;
  for (int g = 0; g < G; g++) {
    TRY(shard_ready(ctxs[g]));
    const SState &sg = ctxs[g]->s;
    if (sg.shard_count != G || sg.shard_rank != g || ctxs[g]->n != ctxs[0]->n || sg.xlog != ctxs[0]->s.xlog) return GM_EINVAL;
  }
  return GM_OK;
}

// The phase API's collectives between the G shard contexts of one device (the Python
// membership.sharded.loopback_tick drives the phases): what = 0 all-gathers xcnt, what = 1
// MAX-allreduces status[0, n*D), what = 2 SUM-allreduces the msgcount counts of this tick.
extern "C" int gm_shard_loopback(gm_ctx **ctxs, int32_t G, int32_t what, int32_t D) {
  TRY(shard_group_ready(ctxs, G));
  for (int g = 0; g < G; g++) HIPCHECK(hipStreamSynchronize(ctxs[g]->stream));
  hipStream_t st = ctxs[0]->stream;
  if (what == 0) {
    for (int ch = 0; ch < ctxs[0]->s.xk; ch++) TRY(grp_allgather(ctxs, G, ch, st));
  } else if (what == 2) {
    if (!mc_on(ctxs[0], ctxs[0]->t)) return GM_ESTATE;
    TRY(grp_mc_sum(ctxs, G, ctxs[0]->t, st));
  } else {
    if (D <= 0 || D > ctxs[0]->dmax) return GM_EINVAL;
    TRY(grp_max(ctxs, G, 0, 0, (size_t)ctxs[0]->n * D, st));
  }
  HIPCHECK(hipStreamSynchronize(st));
  return GM_OK;
}

// Host-collective hook: the phase exchange buffers of ONE shard context as plain host arrays, so
// that any host-side collective (gloo across processes: membership.sharded.host_tick) can stand
// in for RCCL / gm_shard_loopback. Layouts (n = cluster size, G = shard count):
//   what 0  export: this rank's per-row (present, numfailed) int32[n][2]; import: all G slots
//           int32[G][n][2] (the all-gather's result)
//   what 1  export / import: the resolved draws int32[n][D]; import the MAX over the ranks
//   what 2  (msgcount recording) export / import: uint32[n] fresh counts, plus uint32[n] kept
//           entries on keyed-loss ticks; import the SUM over the ranks
static int shard_buf(gm_ctx *c, int what, int D, std::vector<std::pair<void *, size_t>> &parts, bool import) {
  const size_t n = (size_t)c->n;
  SState &s = c->s;
  parts.clear();
  if (what == 0) {  // host layout [n][2] (export) / [G][n][2] (import); device chunk-major (S_XC)
    for (int g = import ? 0 : s.shard_rank; g < (import ? s.shard_count : s.shard_rank + 1); g++)
      for (int ch = 0; ch < s.xk; ch++)
        parts.push_back({s.xcnt + S_XC(s, g, (size_t)ch << s.xlog), sizeof(int32_t) * 2 * xchunk_rows(s, ch)});
    (void)n;
  } else if (what == 1) {
    if (D <= 0 || D > c->dmax) return GM_EINVAL;
    parts.push_back({s.status, sizeof(int32_t) * n * D});
  } else if (what == 2) {
    if (!mc_on(c, c->t)) return GM_ESTATE;
    parts.push_back({s.mc_fresh + (size_t)(c->t & 1) * n, sizeof(uint32_t) * n});
    if (drop_tick(c, c->t)) parts.push_back({s.mc_rdrop, sizeof(uint32_t) * n});
  } else {
    return GM_EINVAL;
  }
  return GM_OK;
}

extern "C" int gm_shard_export(gm_ctx *c, int32_t what, int32_t D, void *out, size_t cap, size_t *bytes) {
  if (!c || !bytes) return GM_EINVAL;
  TRY(shard_ready(c));
  std::vector<std::pair<void *, size_t>> parts;
  TRY(shard_buf(c, what, D, parts, false));
  size_t tot = 0;
  for (auto &p : parts) tot += p.second;
  *bytes = tot;
  if (!out) return GM_OK;
  if (cap < tot) return GM_ERANGE;
  HIPCHECK(hipStreamSynchronize(c->stream));
  size_t off = 0;
  for (auto &p : parts) {
    HIPCHECK(ctx_memcpy(c, (uint8_t *)out + off, p.first, p.second, hipMemcpyDeviceToHost));
    off += p.second;
  }
  return GM_OK;
}

extern "C" int gm_shard_import(gm_ctx *c, int32_t what, int32_t D, const void *in, size_t bytes) {
  if (!c || !in) return GM_EINVAL;
  TRY(shard_ready(c));
  std::vector<std::pair<void *, size_t>> parts;
  TRY(shard_buf(c, what, D, parts, true));
  size_t tot = 0;
  for (auto &p : parts) tot += p.second;
  if (bytes != tot) return GM_EINVAL;
  HIPCHECK(hipStreamSynchronize(c->stream));
  size_t off = 0;
  for (auto &p : parts) {
    HIPCHECK(ctx_memcpy(c, p.first, (const uint8_t *)in + off, p.second, hipMemcpyHostToDevice));
    off += p.second;
  }
  return GM_OK;
}

// Diagnostics: one column shard alone on a device (no RCCL, no peers): the all-gather of
// per-row counts mirrors this shard's counts into every peer slot and the draw kernel
// resolves draws landing in peer columns as fresh column ix (SState.stub) -- a symmetric
// stand-in with the real kernels at the true shard shape (scripts/shard_profile.py --sb).
extern "C" int gm_shard_stub(gm_ctx *c, int32_t on) {
  if (!c || c->cfg.mode != GM_MODE_SCALED || !c->s.sharded) return GM_EINVAL;
  c->s.stub = on ? 1 : 0;
  return GM_OK;
}

// Bounded rounds 1 and 2 of tick t over the rows round 0 left pending: their sorted list (identical on
// every rank) takes the next 64 S2 outputs, then up to 256 rows the next 256; a row still short sets
// GM_ERR_DRAWS. Rows the rounds could not take are counted in npending (draw_settle finishes them with
// host-driven rounds).
static int run_bounded(gm_ctx **g, int G, int t) {
  hipStream_t st = g[0]->stream;
  for (int l = 1; l <= 2; l++) {
    const int D = l == 1 ? GM_D_MORE : GM_D_LAST;
    for (int i = 0; i < G; i++) {
      HIPCHECK(gm_launch_plist_sort(g[i]->s, l, st));
      HIPCHECK(gm_launch_draw(g[i]->s, t, l, D, l, st));
    }
    TRY(grp_max(g, G, l, 0, (size_t)g[0]->s.plist_cap[l] * D, st));
    for (int i = 0; i < G; i++) HIPCHECK(gm_launch_accept(g[i]->s, t, D, l, l == 1 ? 2 : -1, st));
  }
  for (int i = 0; i < G && getenv("GM_DEBUG_ROUNDS"); i++) {  // diagnostics: rows left after round 0, error flags
    const SState &s = g[i]->s;
    uint32_t pc1 = 0, pc2 = 0, e = 0;
    HIPCHECK(hipMemcpyAsync(&pc1, s.plist_cnt[1], sizeof pc1, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipMemcpyAsync(&pc2, s.plist_cnt[2], sizeof pc2, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipMemcpyAsync(&e, s.err, sizeof e, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
    fprintf(stderr, "[gm] t=%d rows pending after round 0: %u (cap %d), after round 1: %u (cap %d), err 0x%x\n", t,
            pc1, s.plist_cap[1], pc2, s.plist_cap[2], e);
  }
  return GM_OK;
}

// The end of a sharded tick's device work: the counts of rows still drawing go to the host without
// a wait (draw_settle reads them before anything uses the tick). deferred (the pipelined tick):
// bounded rounds 1, 2 have not run; draw_settle runs them only when round 0 left rows pending -- in
// the steady state it leaves none, so a tick pays neither their six launches nor their two
// MAX-allreduces. Every rank takes the same decision (the acceptance is identical on all ranks), so
// the ranks' RCCL calls stay in step.
// ds: the stream whose work decides the counts (the pipelined tick's comm stream: the copy follows
// its last acceptance directly instead of behind a cross-stream join)
static int end_draws(gm_ctx **g, int G, bool deferred, hipStream_t ds) {
  if (!deferred) TRY(run_bounded(g, G, g[0]->t));
  for (int i = 0; i < G; i++)
    HIPCHECK(hipMemcpyAsync(g[i]->draw_left_h, g[i]->s.npending, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, ds));
  HIPCHECK(hipEventRecord(g[0]->draw_ev, ds));
  for (int i = 0; i < G; i++) {
    g[i]->draw_rounds = deferred;
    g[i]->draw_check = true;  // before shard_finish: the msgcount phase waits for draw_settle
    TRY(shard_finish(g[i], g[0]->stream));
  }
  return GM_OK;
}

// Every member counts the same pending rows (each replays every row's draws and accepts the same
// MAX-reduced statuses): anything else is a bug caught here
static int pending_agree(gm_ctx **g, int G) {
  for (int i = 1; i < G; i++)
    for (int k = 0; k < 2; k++)
      if (g[i]->draw_left_h[k] != g[0]->draw_left_h[k]) {
        snprintf(g_errbuf, sizeof g_errbuf, "pipelined loopback tick: shards disagree on pending rows (%d vs %d)",
                 g[i]->draw_left_h[k], g[0]->draw_left_h[k]);
        return GM_ESTATE;
      }
  return GM_OK;
}
// the rows still drawing after the rounds enqueued so far, read back with a wait
static int read_pending(gm_ctx **g, int G, int32_t *pend) {
  for (int i = 0; i < G; i++)
    HIPCHECK(hipMemcpyAsync(g[i]->draw_left_h, g[i]->s.npending, sizeof(int32_t), hipMemcpyDeviceToHost, g[0]->stream));
  HIPCHECK(hipStreamSynchronize(g[0]->stream));
  *pend = g[0]->draw_left_h[0];
  return pending_agree(g, G);
}

// One host-driven round of tick t: every row still drawing takes D more S2 outputs (round >= 1: each
// row from its own next round, gm_s_draw reads it from pending[r]); *pend: the rows left after it
static int draw_round(gm_ctx **g, int G, int t, int round, int D, int32_t *pend) {
  hipStream_t st = g[0]->stream;
  for (int i = 0; i < G; i++) HIPCHECK(gm_launch_draw(g[i]->s, t, round, D, 0, st));
  TRY(grp_max(g, G, 0, 0, (size_t)g[0]->n * D, st));
  for (int i = 0; i < G; i++) {
    HIPCHECK(hipMemsetAsync(g[i]->s.npending, 0, sizeof(int32_t), st));
    HIPCHECK(gm_launch_accept(g[i]->s, t, D, 0, 0, st));
  }
  return read_pending(g, G, pend);
}

static int draws_exhausted(gm_ctx **g, int G) {  // a row that never finds its targets: same guard as gm_s_pick
  const uint32_t e = GM_ERR_DRAWS;
  for (int i = 0; i < G; i++) {
    HIPCHECK(hipMemcpyAsync(g[i]->s.err, &e, sizeof e, hipMemcpyHostToDevice, g[0]->stream));
    g[i]->latched = GM_ERANGE;
  }
  HIPCHECK(hipStreamSynchronize(g[0]->stream));
  return GM_ERANGE;
}

// The column-shard tick, pipelined over the exchange's row chunks (north_star: the exchange
// overlapped with the local merge on a second stream). The compute stream runs the band kernels
// chunk after chunk; as soon as chunk ch's are done (event), the comm stream all-gathers the
// chunk's per-row counts, draws round 0 of its rows (every rank replays every row's first 16 S2
// outputs and resolves the draws landing in its columns), MAX-allreduces their statuses and runs
// the acceptance -- while the band kernels of chunks ch+1.. still run. A row's draws need only
// its own post-sweep row (in chunk ch) and the other ranks' counts of that row; the acceptance
// appends to the inboxes of tick t+1 (the other parity), which no band kernel of tick t reads.
// The bounded rounds 1, 2 are left to draw_settle. Ticks that record msgcount (their
// fresh-count all-reduce precedes every draw), the join ramp and the host-driven draw loop (mass
// failure, heavy loss) take the same steps unchunked.
// A loopback group shares its first member's stream pair: G concurrent pairs on one device starve
// each other's small kernels (on a node every shard has its GPU to itself).
int gmh::tick_sharded(gm_ctx **g, int G) {
  gm_ctx *L = g[0];
  if (G == 1 && !L->comm && !L->s.stub) return GM_EUNSUPPORTED;  // multi-GPU ticks need gm_comm_init (or a loopback)
  const SState &s0 = L->s;  // the chunking is the same on every member
  const size_t n = (size_t)L->n;
  const int t = L->t;
  hipStream_t st = L->stream, cs = L->xch.stream;
  // mass failure or heavy loss leaves many entries stale, so rows need many draws: the
  // host-driven unbounded loop below (also GM_SHARD_SYNC=1)
  const bool sync = L->shard_sync == 1 || (L->shard_sync < 0 && (L->cfg.drop_pct >= 30 || 10 * L->nfailed > (int64_t)n));
  const bool pipe = !sync && !mc_on(L, t) && !s0.ramp && !(getenv("GM_SHARD_PIPE") && !atoi(getenv("GM_SHARD_PIPE")));
  if (pipe) {
    // no fills: gm_s_xrows writes this rank's xcnt slots whole (no join ramp here) and gm_s_mtgen
    // zeroes the draw rounds' counters
    for (int i = 0; i < G; i++) HIPCHECK(gm_launch_tick_prologue(g[i]->s, t, st, true));
    hipEvent_t k0 = nullptr, k1 = nullptr;  // the first member's: they bracket the group's band kernels
    if (L->timing) TRY(timing_slot(L, &k0, &k1, st));
    if (k0) HIPCHECK(hipEventRecord(k0, st));
    for (int ch = 0; ch < s0.xk; ch++) {
      const int r0 = ch << s0.xlog, r1 = r0 + xchunk_rows(s0, ch);
      for (int i = 0; i < G; i++) {
        const SState &s = g[i]->s;
        HIPCHECK(gm_launch_band_rows(s, t, drop_tick(g[i], t) ? g[i]->cfg.drop_pct : -1, r0, r1, st));
        const int zr = g[i]->diag_zero_row;
        if (zr >= r0 && zr < r1)
          for (int b = 0; b < s.nb; b++) HIPCHECK(hipMemsetAsync(s.table + ((size_t)b * n + zr) * s.band, 0, s.band, st));
      }
      HIPCHECK(hipEventRecord(L->xch.chunk_ev[ch], st));
    }
    if (k1) HIPCHECK(hipEventRecord(k1, st));
    for (int i = 0; i < G; i++) TRY(detect_tick(g[i], t, st));  // on the compute stream, beside the comm stream's draws
    for (int ch = 0; ch < s0.xk; ch++) {
      const int r0 = ch << s0.xlog, r1 = r0 + xchunk_rows(s0, ch);
      HIPCHECK(hipStreamWaitEvent(cs, L->xch.chunk_ev[ch], 0));
      for (int i = 0; i < G; i++) HIPCHECK(gm_launch_xrows(g[i]->s, r0, r1, cs));
      TRY(grp_allgather(g, G, ch, cs));
      for (int i = 0; i < G; i++) HIPCHECK(gm_launch_draw(g[i]->s, t, 0, GM_D_FIRST, 0, cs, r0, r1));
      TRY(grp_max(g, G, 0, (size_t)r0 * GM_D_FIRST, (size_t)(r1 - r0) * GM_D_FIRST, cs));
      for (int i = 0; i < G; i++) HIPCHECK(gm_launch_accept(g[i]->s, t, GM_D_FIRST, 0, 1, cs, r0, r1));
    }
    HIPCHECK(hipEventRecord(L->xch.done, cs));
    HIPCHECK(hipStreamWaitEvent(st, L->xch.done, 0));
    return end_draws(g, G, true, cs);
  }
  for (int i = 0; i < G; i++) TRY(shard_merge(g[i], st));
  for (int ch = 0; ch < s0.xk; ch++) TRY(grp_allgather(g, G, ch, st));
  if (mc_on(L, t)) TRY(grp_mc_sum(g, G, t, st));
  if (!sync) {
    // bounded rounds, stream-ordered (no host round trip): round 0 = every row's first 16
    // S2 outputs; rows left pending go to a list (sorted: identical on every rank) that
    // round 1 serves with the next 64; a row still short after that sets GM_ERR_DRAWS
    for (int i = 0; i < G; i++) {
      const SState &s = g[i]->s;
      for (int l = 1; l <= 2; l++) HIPCHECK(hipMemsetAsync(s.plist_cnt[l], 0, sizeof(uint32_t), st));
      HIPCHECK(hipMemsetAsync(s.npending, 0, sizeof(int32_t), st));
      HIPCHECK(gm_launch_draw(s, t, 0, GM_D_FIRST, 0, st));
    }
    TRY(grp_max(g, G, 0, 0, n * GM_D_FIRST, st));
    for (int i = 0; i < G; i++) HIPCHECK(gm_launch_accept(g[i]->s, t, GM_D_FIRST, 0, 1, st));
    return end_draws(g, G, false, st);
  }
  int32_t pend = 0;
  for (int round = 0;; round++) {
    TRY(draw_round(g, G, t, round, round ? GM_D_MORE : GM_D_FIRST, &pend));
    if (getenv("GM_DEBUG_ROUNDS")) fprintf(stderr, "[gm] t=%d round %d: %d rows still drawing\n", t, round, pend);
    if (pend == 0) break;
    if (round >= GM_MAX_ROUNDS) return draws_exhausted(g, G);
  }
  for (int i = 0; i < G; i++) TRY(shard_finish(g[i], st));
  return GM_OK;
}

// The rows the last sharded tick's bounded rounds left (a full pending list, or still short of
// targets after 336 S2 outputs): host-driven rounds, each row continuing from its own next round,
// until every row has its targets -- tick t = c->t - 1 completes before anything reads it or the
// next tick starts.
int gmh::draw_settle(gm_ctx **g, int G) {
  gm_ctx *L = g[0];
  if (!L->draw_check) return L->latched;
  const bool deferred = L->draw_rounds;
  for (int i = 0; i < G; i++) g[i]->draw_check = g[i]->draw_rounds = false;
  // the next tick's launches wait on these two counts: spin on the event rather than block (the
  // wait costs 2-18 us of GPU idle per pipelined tick, profiles/r06/stub_tail/). No work of the
  // next tick is enqueued before it: its S2 precompute zeroes the counts the copy reads
  hipError_t q;
  while ((q = hipEventQuery(L->draw_ev)) == hipErrorNotReady) {
  }
  HIPCHECK(q);
  TRY(pending_agree(g, G));
  int32_t pend = L->draw_left_h[0];
  const int t = L->t - 1;
  if (deferred && L->draw_left_h[1] > 0) {  // the pipelined tick's bounded rounds, only if round 0 left rows pending
    TRY(run_bounded(g, G, t));
    TRY(read_pending(g, G, &pend));
  }
  for (int round = 0; pend > 0; round++) {
    if (getenv("GM_DEBUG_ROUNDS")) fprintf(stderr, "[gm] t=%d settle round %d: %d rows still drawing\n", t, round, pend);
    if (round >= GM_MAX_ROUNDS) return draws_exhausted(g, G);
    TRY(draw_round(g, G, t, 1, GM_D_MORE, &pend));
  }
  for (int i = 0; i < G; i++)
    if (mc_on(g[i], t)) HIPCHECK(gm_launch_msgcount(g[i]->s, t, drop_tick(g[i], t), 1, L->stream));
  return L->latched;
}

// One column-shard tick of the G shard contexts of one cluster living on one device (tests,
// scripts/sb_loopback_profile.py): the tick gm_tick runs per rank (tick_sharded, draw_settle),
// with the group's collectives done by device copies and reduce kernels instead of RCCL. The
// join ramp and msgcount recording are not driven here (GM_EINVAL).
extern "C" int gm_shard_loopback_tick(gm_ctx **ctxs, int32_t G) {
  TRY(shard_group_ready(ctxs, G));
  for (int g = 0; g < G; g++)
    if (ctxs[g]->t != ctxs[0]->t || ctxs[g]->s.ramp || mc_on(ctxs[g], ctxs[g]->t)) return GM_EINVAL;
  TRY(draw_settle(ctxs, G));
  for (int g = 0; g < G; g++) {
    TRY(before_tick_events(ctxs[g]));
    HIPCHECK(hipStreamSynchronize(ctxs[g]->stream));  // the tick runs on the first member's streams
  }
  int rc = tick_sharded(ctxs, G);
  for (int g = 0; g < G && rc == GM_OK; g++) advance(ctxs[g]);
  // settled here, not lazily as gm_tick does: a later call on one member alone (gm_sync, gm_read_*,
  // gm_drain_events) could not reduce across its peers
  if (rc == GM_OK) rc = draw_settle(ctxs, G);
  HIPCHECK(hipStreamSynchronize(ctxs[0]->xch.stream));
  HIPCHECK(hipStreamSynchronize(ctxs[0]->stream));
  return rc;
}
