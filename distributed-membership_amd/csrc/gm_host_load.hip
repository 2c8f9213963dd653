// gm_host_load.hip -- SCALED state loading, the inverse of the read-backs (gm_host_read.hip):
// gm_load_begin / gm_load_rows / gm_load_commit (gm_load.hip has the kernels and what they check).
#include "gm_host.h"

using namespace gmh;

#define GM_LOAD_STAGE_BYTES (256ull << 20)  // staged (hb, ts) of one encode launch; + 44 B per node: < 512 MiB
#define GM_LOAD_REJECTED(call) call ": state rejected (check flags 0x%x)"

static void load_free(gm_ctx *c) {
  if (c->ld.blob) (void)hipFree(c->ld.blob);
  c->ld.blob = nullptr;
  c->ld.hb = c->ld.ts = c->ld.base = c->ld.own = c->ld.nodes = nullptr;
  c->ld.status = nullptr;
  c->ld.cap = 0;
  std::vector<uint8_t>().swap(c->ld.seen);
}

void gmh::load_destroy(gm_ctx *c) {
  load_free(c);
  for (hipEvent_t e : c->ld.ev)
    if (e) (void)hipEventDestroy(e);
}

// the status word of the load kernels enqueued so far (fmt: GM_LOAD_REJECTED of the call); a failure
// voids the load (gm_load_begin starts over)
static int load_status(gm_ctx *c, const char *fmt) {
  uint32_t st = 0;
  const int rc = kernel_status(c, c->ld.status, GM_ERANGE, fmt, &st);
  if (!st) return rc;
  HIPCHECK(ctx_memset(c, c->ld.status, 0, sizeof st));
  c->ld.voided = true;
  return (st & GM_LD_EINVAL) ? GM_EINVAL : rc;
}

extern "C" int gm_load_begin(gm_ctx *c, int32_t t) {
  if (!c) return GM_EINVAL;
  if (c->cfg.mode != GM_MODE_SCALED || c->s.ramp || c->s.mc_sent) return GM_EUNSUPPORTED;
  if (t < 1 || t > GM_T_LIMIT) return GM_EINVAL;
  if (c->latched != GM_OK) return c->latched;
  SState &s = c->s;
  if (!c->ld.loading) {  // settle the run so far; its device error, if any, is the caller's to see
    TRY(settled_read(c));
  } else {
    HIPCHECK(hipStreamSynchronize(c->stream));
    HIPCHECK(ctx_memset(c, s.err, 0, sizeof(uint32_t)));  // a voided load's pool overflow
  }
  const size_t n = (size_t)c->n, w = (size_t)s.w;
  size_t cap = std::min<size_t>(n, std::max<size_t>(1, GM_LOAD_STAGE_BYTES / (2 * sizeof(int32_t) * w)));
  if (getenv("GM_LOAD_STAGE_ROWS"))  // diagnostics (tests): smaller encode launches
    cap = std::max<size_t>(1, std::min<size_t>(cap, (size_t)atol(getenv("GM_LOAD_STAGE_ROWS"))));
  if (!c->ld.blob || (size_t)c->ld.cap != cap) {
    load_free(c);
    // int32 words: hb, ts [cap][w]; base [cap]; own [n][2]; heartbeat, failed, counts [n], targets [n][5]; status
    const size_t words = 2 * cap * w + cap + 2 * n + (3 + GM_FANOUT) * n + 4;
    if (hipMalloc(&c->ld.blob, words * sizeof(int32_t)) != hipSuccess) {
      c->ld.blob = nullptr;
      snprintf(g_errbuf, sizeof g_errbuf, "hipMalloc(%zu) failed (load staging)", words * sizeof(int32_t));
      return GM_ENOMEM;
    }
    c->ld.bytes = words * sizeof(int32_t);
    c->ld.cap = (int)cap;
    c->ld.hb = (int32_t *)c->ld.blob;
    c->ld.ts = c->ld.hb + cap * w;
    c->ld.base = c->ld.ts + cap * w;
    c->ld.own = c->ld.base + cap;
    c->ld.nodes = c->ld.own + 2 * n;
    c->ld.status = (uint32_t *)(c->ld.nodes + (3 + GM_FANOUT) * n);
  }
  HIPCHECK(ctx_memset(c, c->ld.status, 0, sizeof(uint32_t)));
  HIPCHECK(ctx_memset(c, c->ld.own, 0xFF, sizeof(int32_t) * 2 * n));
  // the escape lists and payload slots of parity (t - 1) & 1 are allocated by the encode; the other
  // parity's counters are the next tick's, zeroed "a tick ahead" (band_reset_pools)
  HIPCHECK(ctx_memset(c, s.tesc_cnt, 0, 2 * (size_t)s.esc_stripes * sizeof(unsigned long long)));
  HIPCHECK(ctx_memset(c, s.pesc_cnt, 0, 2 * (size_t)s.esc_stripes * sizeof(unsigned long long)));
  if (s.fb_cnt) HIPCHECK(ctx_memset(c, s.fb_cnt, 0, 2 * sizeof(uint32_t)));
  c->ld.loading = true;
  c->ld.voided = false;
  c->ld.t = t;
  c->ld.seen.assign(n, 0);
  c->ld.rows = 0;
  c->ld.ms[0] = c->ld.ms[1] = 0;
  return GM_OK;
}

extern "C" int gm_load_rows(gm_ctx *c, int32_t r0, int32_t count, const int32_t *hb, const int32_t *ts) {
  if (!c || r0 < 0 || count < 0 || r0 + (int64_t)count > c->n || (count > 0 && (!hb || !ts))) return GM_EINVAL;
  if (!c->ld.loading || c->ld.voided) return GM_ESTATE;
  for (int i = 0; i < count; i++)
    if (c->ld.seen[r0 + i]) return GM_ESTATE;  // each row exactly once
  const SState &s = c->s;
  const size_t w = (size_t)s.w;
  if (c->timing)
    for (hipEvent_t &e : c->ld.ev)
      if (!e) HIPCHECK(hipEventCreate(&e));
  for (int off = 0; off < count; off += c->ld.cap) {
    const int m = std::min(c->ld.cap, count - off), rb = r0 + off;
    HIPCHECK(ctx_memcpy(c, c->ld.hb, hb + (size_t)off * w, sizeof(int32_t) * m * w, hipMemcpyHostToDevice));
    HIPCHECK(ctx_memcpy(c, c->ld.ts, ts + (size_t)off * w, sizeof(int32_t) * m * w, hipMemcpyHostToDevice));
    if (c->timing) HIPCHECK(hipEventRecord(c->ld.ev[0], c->stream));
    HIPCHECK(gm_launch_load_check(s, c->ld.t, rb, m, c->ld.hb, c->ld.ts, c->ld.base, c->ld.own, c->ld.status, c->stream));
    if (c->timing) HIPCHECK(hipEventRecord(c->ld.ev[1], c->stream));
    TRY(load_status(c, GM_LOAD_REJECTED("gm_load_rows")));  // nothing of the block is written before its checks pass
    if (c->timing) {  // (load_status waited for the stream)
      float a = 0;
      HIPCHECK(hipEventElapsedTime(&a, c->ld.ev[0], c->ld.ev[1]));
      c->ld.ms[0] += a;
      HIPCHECK(hipEventRecord(c->ld.ev[0], c->stream));
    }
    HIPCHECK(gm_launch_load_encode(s, c->ld.t, rb, m, c->ld.hb, c->ld.ts, c->ld.base, c->stream));
    if (c->timing) {
      float b = 0;
      HIPCHECK(hipEventRecord(c->ld.ev[2], c->stream));
      HIPCHECK(hipStreamSynchronize(c->stream));
      HIPCHECK(hipEventElapsedTime(&b, c->ld.ev[0], c->ld.ev[2]));
      c->ld.ms[1] += b;
    }
    for (int i = 0; i < m; i++) c->ld.seen[rb + i] = 1;
    c->ld.rows += m;
  }
  return GM_OK;
}

extern "C" int gm_load_commit(gm_ctx *c, const int32_t *heartbeat, const int32_t *failed, const int32_t *targets,
                              const int32_t *counts) {
  if (!c || !heartbeat || !failed || !targets || !counts) return GM_EINVAL;
  if (!c->ld.loading || c->ld.voided || c->ld.rows != c->n) return GM_ESTATE;  // rows missing
  SState &s = c->s;
  const size_t n = (size_t)c->n;
  const int t = c->ld.t;
  int32_t *d_hb = c->ld.nodes, *d_f = d_hb + n, *d_cnt = d_f + n, *d_tg = d_cnt + n;
  HIPCHECK(ctx_memcpy(c, d_hb, heartbeat, sizeof(int32_t) * n, hipMemcpyHostToDevice));
  HIPCHECK(ctx_memcpy(c, d_f, failed, sizeof(int32_t) * n, hipMemcpyHostToDevice));
  HIPCHECK(ctx_memcpy(c, d_cnt, counts, sizeof(int32_t) * n, hipMemcpyHostToDevice));
  HIPCHECK(ctx_memcpy(c, d_tg, targets, sizeof(int32_t) * n * GM_FANOUT, hipMemcpyHostToDevice));
  uint32_t e = 0;  // the encode's own flag: an escape pool too small for this state
  const int rc = kernel_status(c, s.err, GM_ERANGE, "gm_load_commit: the state overflows the escape pools (flags 0x%x)", &e);
  if (e) {
    HIPCHECK(ctx_memset(c, s.err, 0, sizeof e));
    c->ld.voided = true;
  }
  TRY(rc);
  HIPCHECK(gm_launch_load_nodes(s, t, d_hb, d_f, d_tg, d_cnt, c->ld.own, c->ld.status, 0, c->stream));
  TRY(load_status(c, GM_LOAD_REJECTED("gm_load_commit")));
  for (int p = 0; p < 2; p++) HIPCHECK(ctx_memset(c, s.inbox_cnt[p], 0, sizeof(int32_t) * n));
  HIPCHECK(gm_launch_load_nodes(s, t, d_hb, d_f, d_tg, d_cnt, c->ld.own, c->ld.status, 1, c->stream));
  HIPCHECK(gm_launch_load_inbox(s, t, c->ld.status, c->stream));
  TRY(load_status(c, GM_LOAD_REJECTED("gm_load_commit")));  // an inbox past its capacity: GM_ERANGE
  // as a tick would have left it: no records of a last tick (the totals and the recorder carry on)
  HIPCHECK(ctx_memset(c, s.ev_spill_cnt, 0, (1 + S_EV_STRIPES) * sizeof(uint32_t)));
  c->pending.clear();
  c->undrained = false;
  c->nfailed = 0;
  for (size_t i = 0; i < n; i++) {
    // a node that was crashed before the load and still is keeps the tick it failed at (gm_detect's
    // fail_tick); one the load crashes counts as failed at the end of tick t - 1
    if (!failed[i]) c->fail_t[i] = 0x7FFFFFFF;
    else if (!c->failed_h[i]) c->fail_t[i] = t - 1;
    c->failed_h[i] = failed[i];
    c->nfailed += failed[i] != 0;
  }
  c->t = t;
  c->ld.loading = false;
  load_free(c);
  return GM_OK;
}

extern "C" int gm_load_stats(gm_ctx *c, double stats[4]) {
  if (!c || !stats) return GM_EINVAL;
  if (c->cfg.mode != GM_MODE_SCALED) return GM_EUNSUPPORTED;
  stats[0] = (double)c->ld.rows;
  stats[1] = (double)c->ld.bytes;
  stats[2] = c->ld.ms[0];
  stats[3] = c->ld.ms[1];
  return GM_OK;
}

// ------------------------------------------------------------------ PARTIAL: loading a view state
// gm_load_views_begin / gm_load_views / gm_load_views_commit (gm_load_views.hip has the kernels and
// what they check). A row shard's received lists and the remote half of its inboxes are not loaded:
// the commit marks the context "exchange pending" and the next tick replays the exchange of tick
// t - 1 from what the commit wrote (tick_partial).
#define GM_VLOAD_STAGE_BYTES (256ull << 20)  // the whole staging block: staged views, bitmap, status
#define GM_VLOAD_NODE_WORDS (3 + GM_FANOUT)  // staged int32 words per node of the commit
#define GM_VLOAD_REJECTED(call)                                                                                      \
  call ": state rejected (check flags 0x%x: 1 id, 2 order, 4 gap, 8 even hb, 10 hb ahead, 20 age, 40 own entry, " \
       "80 heartbeat, 100 failed, 200 count, 400 target, 800 crashed sender, 1000 node missing, 10000 inbox)"

static void vload_free(gm_ctx *c) {
  if (c->vl.blob) (void)hipFree(c->vl.blob);
  c->vl.blob = nullptr;
  c->vl.rows = nullptr;
  c->vl.given = c->vl.status = nullptr;
  c->vl.cap = c->vl.ncap = 0;
  std::vector<uint8_t>().swap(c->vl.seen);
}

void gmh::vload_destroy(gm_ctx *c) {
  vload_free(c);
  for (hipEvent_t e : c->vl.ev)
    if (e) (void)hipEventDestroy(e);
}

// the status word of the view-load kernels enqueued so far; a failure voids the load
static int vload_status(gm_ctx *c, const char *fmt) {
  uint32_t st = 0;
  const int rc = kernel_status(c, c->vl.status, GM_ERANGE, fmt, &st);
  if (!st) return rc;
  HIPCHECK(ctx_memset(c, c->vl.status, 0, sizeof st));
  c->vl.voided = true;
  return (st & GM_PL_EINVAL_MASK) ? GM_EINVAL : rc;
}

extern "C" int gm_load_views_begin(gm_ctx *c, int32_t t) {
  if (!c) return GM_EINVAL;
  if (c->cfg.mode != GM_MODE_PARTIAL || c->p.mc_sent) return GM_EUNSUPPORTED;
  if (t < 5 + 1 || t > GM_T_LIMIT / 2 + 1) return GM_EINVAL;  // t0 + 1 for a t0 create_partial accepts
  if (c->latched != GM_OK) return c->latched;
  PState &p = c->p;
  // settle the run so far on both streams (and a row shard's exchange); its device error, if any, is
  // the caller's to see. A voided load left nothing in flight but its own kernels
  HIPCHECK(hipStreamSynchronize(c->stream));
  HIPCHECK(hipStreamSynchronize(c->ph.side));
  if (c->xch.stream) HIPCHECK(hipStreamSynchronize(c->xch.stream));
  if (!c->vl.loading) TRY(check_err(c));
  c->pending.clear();  // undrained events of the run so far are discarded
  c->undrained = false;
  const size_t nl = (size_t)p.nloc, row_bytes = sizeof(uint64_t) * (size_t)p.V;
  const size_t gwords = (nl + 31) / 32, tail = sizeof(uint32_t) * (gwords + 4);
  size_t cap = std::min<size_t>(nl, std::max<size_t>(1, (GM_VLOAD_STAGE_BYTES - tail) / row_bytes));
  if (getenv("GM_LOAD_STAGE_ROWS"))  // diagnostics (tests): smaller blocks
    cap = std::max<size_t>(1, std::min<size_t>(cap, (size_t)atol(getenv("GM_LOAD_STAGE_ROWS"))));
  if (!c->vl.blob || (size_t)c->vl.cap != cap) {
    vload_free(c);
    const size_t stage = std::max<size_t>(cap * row_bytes, sizeof(int32_t) * GM_VLOAD_NODE_WORDS);
    if (hipMalloc(&c->vl.blob, stage + tail) != hipSuccess) {
      c->vl.blob = nullptr;
      snprintf(g_errbuf, sizeof g_errbuf, "hipMalloc(%zu) failed (view load staging)", stage + tail);
      return GM_ENOMEM;
    }
    c->vl.bytes = stage + tail;
    c->vl.cap = (int)cap;
    c->vl.ncap = (int)std::min<size_t>(nl, stage / (sizeof(int32_t) * GM_VLOAD_NODE_WORDS));
    c->vl.rows = (uint64_t *)c->vl.blob;
    c->vl.given = (uint32_t *)((uint8_t *)c->vl.blob + stage);
    c->vl.status = c->vl.given + gwords;
  }
  HIPCHECK(ctx_memset(c, c->vl.given, 0, tail));  // the bitmap and the status word
  c->vl.loading = true;
  c->vl.voided = false;
  c->vl.xpending = false;
  c->vl.t = t;
  c->vl.seen.assign(nl, 0);
  c->vl.nrows = 0;
  c->vl.ms[0] = c->vl.ms[1] = 0;
  return GM_OK;
}

extern "C" int gm_load_views(gm_ctx *c, int32_t r0, int32_t count, const uint64_t *views) {
  if (!c) return GM_EINVAL;
  if (c->cfg.mode != GM_MODE_PARTIAL) return GM_EUNSUPPORTED;
  const PState &p = c->p;
  if (count < 0 || r0 < p.n0 || r0 + (int64_t)count > (int64_t)p.n0 + p.nloc || (count > 0 && !views)) return GM_EINVAL;
  if (!c->vl.loading || c->vl.voided) return GM_ESTATE;
  const int l0 = r0 - p.n0;
  for (int i = 0; i < count; i++)
    if (c->vl.seen[l0 + i]) return GM_ESTATE;  // each node exactly once
  if (c->timing)
    for (hipEvent_t &e : c->vl.ev)
      if (!e) HIPCHECK(hipEventCreate(&e));
  for (int off = 0; off < count; off += c->vl.cap) {
    const int m = std::min(c->vl.cap, count - off), lb = l0 + off;
    HIPCHECK(ctx_memcpy(c, c->vl.rows, views + (size_t)off * p.V, sizeof(uint64_t) * m * p.V, hipMemcpyHostToDevice));
    if (c->timing) HIPCHECK(hipEventRecord(c->vl.ev[0], c->stream));
    HIPCHECK(gm_launch_view_load_check(p, c->vl.t, m, c->vl.rows, c->vl.status, c->stream));
    if (c->timing) HIPCHECK(hipEventRecord(c->vl.ev[1], c->stream));
    TRY(vload_status(c, GM_VLOAD_REJECTED("gm_load_views")));  // nothing of the block is written before its checks pass
    if (c->timing) {  // (vload_status waited for the stream)
      float a = 0;
      HIPCHECK(hipEventElapsedTime(&a, c->vl.ev[0], c->vl.ev[1]));
      c->vl.ms[0] += a;
      HIPCHECK(hipEventRecord(c->vl.ev[0], c->stream));
    }
    HIPCHECK(gm_launch_view_load_store(p, c->vl.t, lb, m, c->vl.rows, c->vl.given, c->stream));
    if (c->timing) {
      float b = 0;
      HIPCHECK(hipEventRecord(c->vl.ev[2], c->stream));
      HIPCHECK(hipStreamSynchronize(c->stream));
      HIPCHECK(hipEventElapsedTime(&b, c->vl.ev[0], c->vl.ev[2]));
      c->vl.ms[1] += b;
    }
    for (int i = 0; i < m; i++) c->vl.seen[lb + i] = 1;
    c->vl.nrows += m;
  }
  return GM_OK;
}

// one pass of gm_pl_nodes over this context's nodes, staged ncap nodes at a time through the block
// (the copies wait for the stream, so a launch is done with the staged arrays before the next copy)
static int vload_nodes_pass(gm_ctx *c, const int32_t *heartbeat, const int32_t *failed_own, const int32_t *targets,
                            const int32_t *counts, int write) {
  const PState &p = c->p;
  for (int off = 0; off < p.nloc; off += c->vl.ncap) {
    const int m = std::min(c->vl.ncap, p.nloc - off);
    int32_t *d_hb = (int32_t *)c->vl.rows, *d_f = d_hb + m, *d_cnt = d_f + m, *d_tg = d_cnt + m;
    HIPCHECK(ctx_memcpy(c, d_hb, heartbeat + off, sizeof(int32_t) * m, hipMemcpyHostToDevice));
    HIPCHECK(ctx_memcpy(c, d_f, failed_own + off, sizeof(int32_t) * m, hipMemcpyHostToDevice));
    HIPCHECK(ctx_memcpy(c, d_cnt, counts + off, sizeof(int32_t) * m, hipMemcpyHostToDevice));
    HIPCHECK(ctx_memcpy(c, d_tg, targets + (size_t)off * GM_FANOUT, sizeof(int32_t) * m * GM_FANOUT, hipMemcpyHostToDevice));
    HIPCHECK(gm_launch_view_load_nodes(p, c->vl.t, off, m, d_hb, d_f, d_cnt, d_tg, c->vl.given, c->vl.status, write,
                                       c->stream));
  }
  return GM_OK;
}

extern "C" int gm_load_views_commit(gm_ctx *c, const int32_t *heartbeat, const int32_t *failed, const int32_t *targets,
                                    const int32_t *counts) {
  if (!c || !heartbeat || !failed || !targets || !counts) return GM_EINVAL;
  if (c->cfg.mode != GM_MODE_PARTIAL) return GM_EUNSUPPORTED;
  if (!c->vl.loading || c->vl.voided || c->vl.nrows != c->p.nloc) return GM_ESTATE;  // nodes missing
  PState &p = c->p;
  const size_t n = (size_t)c->n;
  const int t = c->vl.t;
  for (size_t i = 0; i < n; i++)  // the other shards' flags never reach the device: checked here
    if (failed[i] != 0 && failed[i] != 1) {
      c->vl.voided = true;
      snprintf(g_errbuf, sizeof g_errbuf, GM_VLOAD_REJECTED("gm_load_views_commit"), GM_PL_EFAILED);
      return GM_EINVAL;
    }
  TRY(vload_nodes_pass(c, heartbeat, failed + p.n0, targets, counts, 0));
  TRY(vload_status(c, GM_VLOAD_REJECTED("gm_load_views_commit")));
  TRY(vload_nodes_pass(c, heartbeat, failed + p.n0, targets, counts, 1));
  HIPCHECK(gm_launch_view_load_inbox(p, t, c->vl.status, c->stream));
  TRY(vload_status(c, GM_VLOAD_REJECTED("gm_load_views_commit")));  // an inbox past its capacity: GM_ERANGE
  // as tick t - 1 would have left it: the error flag clear, no records, no prefetched S2 outputs
  HIPCHECK(ctx_memset(c, p.err, 0, sizeof(uint32_t)));
  c->pending.clear();
  c->undrained = false;
  c->ph.mt_next = -1;
  c->nfailed = 0;
  for (size_t i = 0; i < n; i++) {
    if (!failed[i]) c->fail_t[i] = 0x7FFFFFFF;
    else if (!c->failed_h[i]) c->fail_t[i] = t - 1;
    c->failed_h[i] = failed[i];
    c->nfailed += failed[i] != 0;
  }
  c->vc.nfailed = -1;  // the census rebuilds its crash bitmap: a load may clear flags as well as set them
  if (c->ph.sharded) {
    // stamps of an earlier run in the packed blocks must not pass for records of the replayed tick
    HIPCHECK(ctx_memset(c, p.pk_hdr, 0xFF, sizeof(int32_t) * (size_t)p.G * p.nloc * 8));
    HIPCHECK(hipStreamSynchronize(c->stream));
    TRY(partial_caps(c));  // the block capacities and the crash hash follow the loaded flags
  }
  c->t = t;
  c->vl.loading = false;
  c->vl.xpending = c->ph.sharded;
  vload_free(c);
  return GM_OK;
}

extern "C" int gm_load_views_stats(gm_ctx *c, double stats[4]) {
  if (!c || !stats) return GM_EINVAL;
  if (c->cfg.mode != GM_MODE_PARTIAL) return GM_EUNSUPPORTED;
  stats[0] = (double)c->vl.nrows;
  stats[1] = (double)c->vl.bytes;
  stats[2] = c->vl.ms[0];
  stats[3] = c->vl.ms[1];
  return GM_OK;
}
