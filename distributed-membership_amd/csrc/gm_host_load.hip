// gm_host_load.hip -- loading a state, the inverse of the read-backs (gm_host_read.hip). SCALED:
// gm_load_begin / gm_load_rows / gm_load_commit (kernels and what they check: gm_load.hip); PARTIAL:
// gm_load_views_begin / gm_load_views / gm_load_views_commit (gm_load_views.hip). Both are a gm_load_stage
// (gm_host.h) driven by the same functions: load_begin, load_blocks, load_status, load_flags, load_end.
#include "gm_host.h"

using namespace gmh;

#define GM_LOAD_REJECTED(call) call ": state rejected (check flags 0x%x)"
#define GM_VLOAD_REJECTED(call)                                                                                      \
  call ": state rejected (check flags 0x%x: 1 id, 2 order, 4 gap, 8 even hb, 10 hb ahead, 20 age, 40 own entry, " \
       "80 heartbeat, 100 failed, 200 count, 400 target, 800 crashed sender, 1000 node missing, 10000 inbox)"

// a begin's last step: nothing given yet, the times of an earlier load forgotten
static void load_begin(gm_load_stage &ld, int t, size_t rows) {
  ld.loading = true;
  ld.voided = false;
  ld.t = t;
  ld.seen.assign(rows, 0);
  ld.rows = 0;
  ld.ms[0] = ld.ms[1] = 0;
}

// the status word of the load's kernels enqueued so far (waits for the stream; fmt: the call's
// GM_*_REJECTED). A failure voids the load (only the begin starts over): GM_EINVAL for the flags in
// `einval`, GM_ERANGE for the others
static int load_status(gm_ctx *c, gm_load_stage &ld, uint32_t einval, const char *fmt) {
  uint32_t st = 0;
  const int rc = kernel_status(c, ld.status, GM_ERANGE, fmt, &st);
  if (!st) return rc;
  HIPCHECK(ctx_memset(c, ld.status, 0, sizeof st));
  ld.voided = true;
  return (st & einval) ? GM_EINVAL : rc;
}

// Rows [r0, r0 + count) of this context (each exactly once) through the block, cap rows at a time:
// copy_in(off, m) stages rows off.. of the caller's arrays, check(rb, m) launches the checks of rows
// rb.. and store(rb, m) writes them into the state. Nothing of a block is written before its checks
// pass. gm_set_timing on: ms[0] is the check kernel alone, ms[1] the store kernel alone.
template <class CopyIn, class Check, class Store>
static int load_blocks(gm_ctx *c, gm_load_stage &ld, int r0, int count, uint32_t einval, const char *rejected,
                       CopyIn copy_in, Check check, Store store) {
  if (!ld.loading || ld.voided) return GM_ESTATE;
  for (int i = 0; i < count; i++)
    if (ld.seen[r0 + i]) return GM_ESTATE;
  for (int off = 0; off < count; off += ld.cap) {
    const int m = std::min(ld.cap, count - off), rb = r0 + off;
    TRY(copy_in(off, m));
    TRY(stage_mark(c, ld, 0));
    HIPCHECK(check(rb, m));
    TRY(stage_mark(c, ld, 1));
    TRY(load_status(c, ld, einval, rejected));
    TRY(stage_span(c, ld, 0, 0, 1));
    TRY(stage_mark(c, ld, 0));
    HIPCHECK(store(rb, m));
    TRY(stage_mark(c, ld, 2));
    TRY(stage_span(c, ld, 1, 0, 2));
    for (int i = 0; i < m; i++) ld.seen[rb + i] = 1;
    ld.rows += m;
  }
  return GM_OK;
}

// A commit's host side, once its kernels have passed: as tick t - 1 would have left it, no records of a
// last tick (the totals and the recorder carry on), and the crash flags of the loaded state. A node that
// was crashed before the load and still is keeps the tick it failed at (gm_detect's fail_tick); one the
// load crashes counts as failed at the end of tick t - 1
static void load_flags(gm_ctx *c, const int32_t *failed, int t) {
  c->pending.clear();
  c->undrained = false;
  c->nfailed = 0;
  for (size_t i = 0; i < (size_t)c->n; i++) {
    if (!failed[i]) c->fail_t[i] = 0x7FFFFFFF;
    else if (!c->failed_h[i]) c->fail_t[i] = t - 1;
    c->failed_h[i] = failed[i];
    c->nfailed += failed[i] != 0;
  }
}

static void load_end(gm_ctx *c, gm_load_stage &ld) {
  c->t = ld.t;
  ld.loading = false;
  stage_free(ld);
  std::vector<uint8_t>().swap(ld.seen);
}

// ------------------------------------------------------------------ SCALED
// The block, in int32 words: the staged hb, ts [cap][w] of one encode launch (256 MiB at most; with the
// 44 B per node that follow, < 512 MiB); their base ticks [cap]; every row's own entry as staged, own
// [n][2]; the commit's node arrays heartbeat, failed, counts [n], targets [n][5]; the status word.
struct LoadPlanes {
  int32_t *hb, *ts, *base, *own;
};

static LoadPlanes load_planes(const gm_ctx *c) {  // (no block: cap is 0, all null)
  const size_t cw = (size_t)c->ld.cap * c->s.w;
  int32_t *hb = (int32_t *)c->ld.blob, *base = hb + 2 * cw;
  return {hb, hb + cw, base, base + c->ld.cap};
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
  const size_t cap = stage_cap(GM_STAGE_BYTES, 2 * sizeof(int32_t) * w, n, "GM_LOAD_STAGE_ROWS");
  const size_t words = 2 * cap * w + cap + 2 * n + (3 + GM_FANOUT) * n;
  TRY(stage_alloc(c->ld, (int)cap, sizeof(int32_t) * (words + 4), sizeof(int32_t) * words, "load staging"));
  HIPCHECK(ctx_memset(c, c->ld.status, 0, sizeof(uint32_t)));
  HIPCHECK(ctx_memset(c, load_planes(c).own, 0xFF, sizeof(int32_t) * 2 * n));
  // the escape lists and payload slots of parity (t - 1) & 1 are allocated by the encode; the other
  // parity's counters are the next tick's, zeroed "a tick ahead" (band_reset_pools)
  HIPCHECK(ctx_memset(c, s.tesc_cnt, 0, 2 * (size_t)s.esc_stripes * sizeof(unsigned long long)));
  HIPCHECK(ctx_memset(c, s.pesc_cnt, 0, 2 * (size_t)s.esc_stripes * sizeof(unsigned long long)));
  if (s.fb_cnt) HIPCHECK(ctx_memset(c, s.fb_cnt, 0, 2 * sizeof(uint32_t)));
  load_begin(c->ld, t, n);
  return GM_OK;
}

extern "C" int gm_load_rows(gm_ctx *c, int32_t r0, int32_t count, const int32_t *hb, const int32_t *ts) {
  if (!c || r0 < 0 || count < 0 || r0 + (int64_t)count > c->n || (count > 0 && (!hb || !ts))) return GM_EINVAL;
  const SState &s = c->s;
  const size_t w = (size_t)s.w;
  const int t = c->ld.t;
  const LoadPlanes d = load_planes(c);
  return load_blocks(
      c, c->ld, r0, count, GM_LD_EINVAL, GM_LOAD_REJECTED("gm_load_rows"),
      [&](int off, int m) -> int {
        HIPCHECK(ctx_memcpy(c, d.hb, hb + (size_t)off * w, sizeof(int32_t) * m * w, hipMemcpyHostToDevice));
        HIPCHECK(ctx_memcpy(c, d.ts, ts + (size_t)off * w, sizeof(int32_t) * m * w, hipMemcpyHostToDevice));
        return GM_OK;
      },
      [&](int rb, int m) { return gm_launch_load_check(s, t, rb, m, d.hb, d.ts, d.base, d.own, c->ld.status, c->stream); },
      [&](int rb, int m) { return gm_launch_load_encode(s, t, rb, m, d.hb, d.ts, d.base, c->stream); });
}

extern "C" int gm_load_commit(gm_ctx *c, const int32_t *heartbeat, const int32_t *failed, const int32_t *targets,
                              const int32_t *counts) {
  if (!c || !heartbeat || !failed || !targets || !counts) return GM_EINVAL;
  if (!c->ld.loading || c->ld.voided || c->ld.rows != c->n) return GM_ESTATE;  // rows missing
  SState &s = c->s;
  const size_t n = (size_t)c->n;
  const int t = c->ld.t;
  int32_t *own = load_planes(c).own, *d_hb = own + 2 * n, *d_f = d_hb + n, *d_cnt = d_f + n, *d_tg = d_cnt + n;
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
  HIPCHECK(gm_launch_load_nodes(s, t, d_hb, d_f, d_tg, d_cnt, own, c->ld.status, 0, c->stream));
  TRY(load_status(c, c->ld, GM_LD_EINVAL, GM_LOAD_REJECTED("gm_load_commit")));
  for (int p = 0; p < 2; p++) HIPCHECK(ctx_memset(c, s.inbox_cnt[p], 0, sizeof(int32_t) * n));
  HIPCHECK(gm_launch_load_nodes(s, t, d_hb, d_f, d_tg, d_cnt, own, c->ld.status, 1, c->stream));
  HIPCHECK(gm_launch_load_inbox(s, t, c->ld.status, c->stream));
  TRY(load_status(c, c->ld, GM_LD_EINVAL, GM_LOAD_REJECTED("gm_load_commit")));  // an inbox past its capacity: GM_ERANGE
  HIPCHECK(ctx_memset(c, s.ev_spill_cnt, 0, (1 + S_EV_STRIPES) * sizeof(uint32_t)));
  load_flags(c, failed, t);
  load_end(c, c->ld);
  return GM_OK;
}

extern "C" int gm_load_stats(gm_ctx *c, double stats[4]) {
  return stage_stats(c, GM_MODE_SCALED, c ? &c->ld : nullptr, stats);
}

// ------------------------------------------------------------------ PARTIAL
// A row shard's received lists and the remote half of its inboxes are not loaded: the commit marks the
// context "exchange pending" and the next tick replays the exchange of tick t - 1 from what the commit
// wrote (tick_partial).
// The block (256 MiB at most): the staged views [cap][V] of one launch -- the commit stages the node
// arrays through the same rows, ncap nodes at a time --, the "given" bitmap of this context's nodes, the
// status word.
#define GM_VLOAD_NODE_WORDS (3 + GM_FANOUT)  // staged int32 words per node of the commit

static size_t vload_tail(const PState &p) { return sizeof(uint32_t) * (((size_t)p.nloc + 31) / 32 + 4); }
static uint32_t *vload_given(const gm_ctx *c) { return c->vl.status - ((size_t)c->p.nloc + 31) / 32; }

extern "C" int gm_load_views_begin(gm_ctx *c, int32_t t) {
  if (!c) return GM_EINVAL;
  if (c->cfg.mode != GM_MODE_PARTIAL || c->p.mc_sent || c->vdet.tmax) return GM_EUNSUPPORTED;
  if (t < 5 + 1 || t > GM_T_LIMIT / 2 + 1) return GM_EINVAL;  // t0 + 1 for a t0 create_partial accepts
  if (c->latched != GM_OK) return c->latched;
  const PState &p = c->p;
  // settle the run so far on both streams (and a row shard's exchange); its device error, if any, is
  // the caller's to see. A voided load left nothing in flight but its own kernels
  HIPCHECK(hipStreamSynchronize(c->stream));
  HIPCHECK(hipStreamSynchronize(c->ph.side));
  if (c->xch.stream) HIPCHECK(hipStreamSynchronize(c->xch.stream));
  if (!c->vl.loading) TRY(check_err(c));
  c->pending.clear();  // undrained events of the run so far are discarded
  c->undrained = false;
  const size_t nl = (size_t)p.nloc, row_bytes = sizeof(uint64_t) * (size_t)p.V, tail = vload_tail(p);
  const size_t cap = stage_cap(GM_STAGE_BYTES - tail, row_bytes, nl, "GM_LOAD_STAGE_ROWS");
  const size_t stage = std::max<size_t>(cap * row_bytes, sizeof(int32_t) * GM_VLOAD_NODE_WORDS);
  TRY(stage_alloc(c->vl, (int)cap, stage + tail, stage + tail - 4 * sizeof(uint32_t), "view load staging"));
  HIPCHECK(ctx_memset(c, vload_given(c), 0, tail));  // the bitmap and the status word
  c->vl.xpending = false;
  load_begin(c->vl, t, nl);
  return GM_OK;
}

extern "C" int gm_load_views(gm_ctx *c, int32_t r0, int32_t count, const uint64_t *views) {
  if (!c) return GM_EINVAL;
  if (c->cfg.mode != GM_MODE_PARTIAL) return GM_EUNSUPPORTED;
  const PState &p = c->p;
  if (count < 0 || r0 < p.n0 || r0 + (int64_t)count > (int64_t)p.n0 + p.nloc || (count > 0 && !views)) return GM_EINVAL;
  const int t = c->vl.t;
  uint64_t *rows = (uint64_t *)c->vl.blob;
  return load_blocks(
      c, c->vl, r0 - p.n0, count, GM_PL_EINVAL_MASK, GM_VLOAD_REJECTED("gm_load_views"),
      [&](int off, int m) -> int {
        HIPCHECK(ctx_memcpy(c, rows, views + (size_t)off * p.V, sizeof(uint64_t) * m * p.V, hipMemcpyHostToDevice));
        return GM_OK;
      },
      [&](int, int m) { return gm_launch_view_load_check(p, t, m, rows, c->vl.status, c->stream); },
      [&](int lb, int m) { return gm_launch_view_load_store(p, t, lb, m, rows, vload_given(c), c->stream); });
}

// one pass of gm_pl_nodes over this context's nodes, staged ncap nodes at a time through the block
// (the copies wait for the stream, so a launch is done with the staged arrays before the next copy)
static int vload_nodes_pass(gm_ctx *c, const int32_t *heartbeat, const int32_t *failed_own, const int32_t *targets,
                            const int32_t *counts, int write) {
  const PState &p = c->p;
  uint32_t *given = vload_given(c);
  const size_t stage = (uint8_t *)given - (uint8_t *)c->vl.blob;
  const int ncap = (int)std::min<size_t>((size_t)p.nloc, stage / (sizeof(int32_t) * GM_VLOAD_NODE_WORDS));
  for (int off = 0; off < p.nloc; off += ncap) {
    const int m = std::min(ncap, p.nloc - off);
    int32_t *d_hb = (int32_t *)c->vl.blob, *d_f = d_hb + m, *d_cnt = d_f + m, *d_tg = d_cnt + m;
    HIPCHECK(ctx_memcpy(c, d_hb, heartbeat + off, sizeof(int32_t) * m, hipMemcpyHostToDevice));
    HIPCHECK(ctx_memcpy(c, d_f, failed_own + off, sizeof(int32_t) * m, hipMemcpyHostToDevice));
    HIPCHECK(ctx_memcpy(c, d_cnt, counts + off, sizeof(int32_t) * m, hipMemcpyHostToDevice));
    HIPCHECK(ctx_memcpy(c, d_tg, targets + (size_t)off * GM_FANOUT, sizeof(int32_t) * m * GM_FANOUT, hipMemcpyHostToDevice));
    HIPCHECK(gm_launch_view_load_nodes(p, c->vl.t, off, m, d_hb, d_f, d_cnt, d_tg, given, c->vl.status, write, c->stream));
  }
  return GM_OK;
}

extern "C" int gm_load_views_commit(gm_ctx *c, const int32_t *heartbeat, const int32_t *failed, const int32_t *targets,
                                    const int32_t *counts) {
  if (!c || !heartbeat || !failed || !targets || !counts) return GM_EINVAL;
  if (c->cfg.mode != GM_MODE_PARTIAL) return GM_EUNSUPPORTED;
  if (!c->vl.loading || c->vl.voided || c->vl.rows != c->p.nloc) return GM_ESTATE;  // nodes missing
  PState &p = c->p;
  const int t = c->vl.t;
  for (size_t i = 0; i < (size_t)c->n; i++)  // the other shards' flags never reach the device: checked here
    if (failed[i] != 0 && failed[i] != 1) {
      c->vl.voided = true;
      snprintf(g_errbuf, sizeof g_errbuf, GM_VLOAD_REJECTED("gm_load_views_commit"), GM_PL_EFAILED);
      return GM_EINVAL;
    }
  TRY(vload_nodes_pass(c, heartbeat, failed + p.n0, targets, counts, 0));
  TRY(load_status(c, c->vl, GM_PL_EINVAL_MASK, GM_VLOAD_REJECTED("gm_load_views_commit")));
  TRY(vload_nodes_pass(c, heartbeat, failed + p.n0, targets, counts, 1));
  HIPCHECK(gm_launch_view_load_inbox(p, t, c->vl.status, c->stream));
  TRY(load_status(c, c->vl, GM_PL_EINVAL_MASK, GM_VLOAD_REJECTED("gm_load_views_commit")));  // an inbox past its capacity: GM_ERANGE
  HIPCHECK(ctx_memset(c, p.err, 0, sizeof(uint32_t)));  // the error flag clear, no prefetched S2 outputs
  c->ph.mt_next = -1;
  load_flags(c, failed, t);
  c->vc.nfailed = -1;  // the census rebuilds its crash bitmap: a load may clear flags as well as set them
  if (c->ph.sharded) {
    // stamps of an earlier run in the packed blocks must not pass for records of the replayed tick
    HIPCHECK(ctx_memset(c, p.pk_hdr, 0xFF, sizeof(int32_t) * (size_t)p.G * p.nloc * 8));
    HIPCHECK(hipStreamSynchronize(c->stream));
    TRY(partial_caps(c));  // the block capacities and the crash hash follow the loaded flags
  }
  c->vl.xpending = c->ph.sharded;
  load_end(c, c->vl);
  return GM_OK;
}

extern "C" int gm_load_views_stats(gm_ctx *c, double stats[4]) {
  return stage_stats(c, GM_MODE_PARTIAL, c ? &c->vl : nullptr, stats);
}
