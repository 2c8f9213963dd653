// gm_host_events.hip -- what a tick leaves for the caller: the event records drained into reference
// log order, the detection recorder and the msgcount history.
#include "gm_host.h"

using namespace gmh;

// The S_BC words of the last tick in (row, band) order (the device keeps [band][row] records).
static int read_bcnt(gm_ctx *c, std::vector<uint32_t> &bc) {
  const SState &s = c->s;
  const size_t n = (size_t)c->n, nrb = n * s.nb;
  std::vector<uint4> rec(nrb);
  HIPCHECK(hipMemcpyAsync(rec.data(), s.brec, sizeof(uint4) * nrb, hipMemcpyDeviceToHost, c->stream));
  HIPCHECK(hipStreamSynchronize(c->stream));
  bc.resize(nrb);
  for (size_t b = 0; b < (size_t)s.nb; b++)
    for (size_t r = 0; r < n; r++) bc[r * s.nb + b] = rec[b * n + r].z;
  return GM_OK;
}

// Host-side staging bound: records kept for gm_drain_events (a caller that never drains gets
// GM_ERANGE instead of unbounded host memory)
#define GM_PENDING_CAP (1ull << 27)

// SCALED: the last tick's join + remove records (the band kernel's striped partial sums) and
// how many of them spilled to the ring
static int tick_event_total(gm_ctx *c, uint64_t *total, uint32_t *spilled) {
  std::vector<uint32_t> cnt(1 + S_EV_STRIPES);
  HIPCHECK(hipMemcpyAsync(cnt.data(), c->s.ev_spill_cnt, sizeof(uint32_t) * cnt.size(), hipMemcpyDeviceToHost, c->stream));
  HIPCHECK(hipStreamSynchronize(c->stream));
  *spilled = cnt[0];
  *total = 0;
  for (int k = 1; k <= S_EV_STRIPES; k++) *total += cnt[k];
  return GM_OK;
}

static int drain_scaled(gm_ctx *c, std::vector<gm_event> &out) {
  const SState &s = c->s;
  const size_t nrb = (size_t)c->n * s.nb;
  std::vector<uint32_t> bc;
  uint64_t total = 0;
  uint32_t nsp = 0;
  TRY(tick_event_total(c, &total, &nsp));
  if (total == 0) return GM_OK;  // the common tick: nothing to stage, one 1 KB copy
  if (out.size() + total > GM_PENDING_CAP) return GM_ERANGE;
  TRY(read_bcnt(c, bc));
  const int t = c->t - 1;
  auto push = [&](int r, uint32_t rec) {
    out.push_back(gm_event{t, r, (int)(rec >> 30) == (int)S_EV_ADD ? GM_EV_JOINED : GM_EV_REMOVED,
                           (int32_t)(rec & 0x3FFFFFFFu)});
  };
  bool any = false;
  for (uint32_t v : bc) any |= S_BC_NEV(v) != 0;
  if (any) {
    std::vector<uint32_t> ev(nrb * s.evs);
    HIPCHECK(ctx_memcpy(c, ev.data(), s.ev_band, sizeof(uint32_t) * ev.size(), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < nrb; i++) {
      const int k = std::min<int>((int)S_BC_NEV(bc[i]), s.evs);
      for (int q = 0; q < k; q++) push((int)(i / s.nb), ev[i * s.evs + q]);
    }
  }
  nsp = std::min(nsp, s.ev_spill_cap);
  if (nsp) {
    std::vector<uint64_t> sp(nsp);
    HIPCHECK(ctx_memcpy(c, sp.data(), s.ev_spill, sizeof(uint64_t) * nsp, hipMemcpyDeviceToHost));
    for (uint64_t v : sp) push((int)(v >> 32), (uint32_t)v);
  }
  return GM_OK;
}

static void sort_canonical(std::vector<gm_event>::iterator b, std::vector<gm_event>::iterator e) {
  // canonical order of the build-defined modes: loggers descending; joins ascending id, then removals descending id
  std::sort(b, e, [](const gm_event &a, const gm_event &b) {
    if (a.logger != b.logger) return a.logger > b.logger;
    if (a.kind != b.kind) return a.kind < b.kind;
    return a.kind == GM_EV_JOINED ? a.subject < b.subject : a.subject > b.subject;
  });
}

static int drain_partial(gm_ctx *c, std::vector<gm_event> &out) {
  const PState &p = c->p;
  std::vector<int32_t> cnt(p.nloc);
  HIPCHECK(hipMemcpyAsync(cnt.data(), p.ev_cnt, sizeof(int32_t) * p.nloc, hipMemcpyDeviceToHost, c->stream));
  HIPCHECK(hipStreamSynchronize(c->stream));
  size_t tot = 0;
  for (int32_t v : cnt) tot += (size_t)(v & 0xFFFF) + (size_t)(v >> 16);
  if (!tot) return GM_OK;
  // joins: the set bits of each node's join mask over its final list of the tick (lists of parity t & 1,
  // intact until tick t + 2); removals: the records at the back of the node's event row
  const size_t row = 2 * (size_t)p.V;
  const int t = c->t - 1;
  std::vector<uint32_t> jm(p.nloc);
  HIPCHECK(ctx_memcpy(c, jm.data(), p.ev_jm, sizeof(uint32_t) * jm.size(), hipMemcpyDeviceToHost));
  // only the rows that hold events are copied: runs of such rows as async copies on the context
  // stream, one wait at the end -- not the whole list / event buffers (~4.3 GB of lists
  // per S-C context for a tick with any join). Gaps up to `gap` rows are bridged, so there are at
  // most ~4096 copies however the rows are spread.
  const int gap = std::max(64, p.nloc / 4096);
  auto copy_rows = [&](void *dst, const void *src, size_t rowb, int sel) -> hipError_t {
    int r = 0;
    while (r < p.nloc) {
      auto has = [&](int q) { return sel == 0 ? (cnt[q] & 0xFFFF) != 0 : (cnt[q] >> 16) != 0; };
      while (r < p.nloc && !has(r)) r++;
      if (r >= p.nloc) break;
      int e = r + 1, last = r;
      while (e < p.nloc && e - last <= gap) {
        if (has(e)) last = e;
        e++;
      }
      const hipError_t err = hipMemcpyAsync((uint8_t *)dst + (size_t)r * rowb, (const uint8_t *)src + (size_t)r * rowb,
                                            (size_t)(last + 1 - r) * rowb, hipMemcpyDeviceToHost, c->stream);
      if (err != hipSuccess) return err;
      r = last + 1;
    }
    return hipSuccess;
  };
  bool any_join = false, any_rem = false;
  for (int32_t v : cnt) {
    any_join |= (v & 0xFFFF) != 0;
    any_rem |= (v >> 16) != 0;
  }
  std::vector<uint64_t> lst;
  if (any_join) {
    lst.resize((size_t)p.nloc * p.V);
    HIPCHECK(copy_rows(lst.data(), p.lists + (size_t)(t & 1) * p.rows * p.V, sizeof(uint64_t) * p.V, 0));
  }
  std::vector<uint32_t> ev;
  if (any_rem) {
    ev.resize((size_t)p.nloc * row);
    HIPCHECK(copy_rows(ev.data(), p.ev, sizeof(uint32_t) * row, 1));
  }
  HIPCHECK(hipStreamSynchronize(c->stream));
  out.reserve(out.size() + tot);
  for (int r = 0; r < p.nloc; r++) {
    const int nj = cnt[r] & 0xFFFF, nr = cnt[r] >> 16;
    if (__builtin_popcount(jm[r]) != nj) return GM_ESTATE;
    for (uint32_t b = jm[r]; b; b &= b - 1)
      out.push_back(gm_event{t, p.n0 + r, GM_EV_JOINED, (int32_t)(lst[(size_t)r * p.V + __builtin_ctz(b)] >> 32)});
    for (int q = 0; q < nr; q++)
      out.push_back(gm_event{t, p.n0 + r, GM_EV_REMOVED, (int32_t)(ev[(size_t)r * row + row - 1 - q] & 0x3FFFFFFFu)});
  }
  return GM_OK;
}

// SCALED / PARTIAL: move the last tick's device records (one tick's worth is kept on the
// device, overwritten by the next tick) to the host list, in canonical order.
static int stage_events(gm_ctx *c) {
  TRY(f_settle(c));
  if (!c->undrained) return GM_OK;
  c->undrained = false;
  const size_t first = c->pending.size();
  if (c->cfg.mode == GM_MODE_SCALED) TRY(drain_scaled(c, c->pending));
  else if (c->cfg.mode == GM_MODE_PARTIAL) TRY(drain_partial(c, c->pending));
  sort_canonical(c->pending.begin() + first, c->pending.end());
  return GM_OK;
}

// Before a tick overwrites the device records: stage them (keep_events) or drop them.
int gmh::before_tick_events(gm_ctx *c) {
  if (c->cfg.mode == GM_MODE_FAITHFUL) return GM_OK;
  if (c->keep_events) return stage_events(c);
  c->undrained = false;
  return GM_OK;
}

extern "C" int gm_keep_events(gm_ctx *c, int32_t on) {
  if (!c) return GM_EINVAL;
  c->keep_events = on != 0;
  return GM_OK;
}

extern "C" int gm_drain_events(gm_ctx *c, gm_event *out, size_t cap, size_t *n) {
  if (!c || !n) return GM_EINVAL;
  TRY(stage_events(c));
  *n = c->pending.size();
  if (c->pending.size() > cap) return GM_ERANGE;
  if (!c->pending.empty()) memcpy(out, c->pending.data(), sizeof(gm_event) * c->pending.size());
  c->pending.clear();
  return GM_OK;
}

extern "C" int gm_event_counts(gm_ctx *c, uint64_t counts[6]) {
  if (!c || !counts) return GM_EINVAL;
  TRY(f_settle(c));
  for (int k = 0; k < 6; k++) counts[k] = 0;
  if (c->cfg.mode == GM_MODE_SCALED) {
    uint32_t nsp = 0;
    TRY(tick_event_total(c, &counts[0], &nsp));  // join+remove records of the last tick (per-kind split needs a drain)
  } else if (c->cfg.mode == GM_MODE_PARTIAL) {
    std::vector<int32_t> cnt(c->p.nloc);
    HIPCHECK(hipMemcpyAsync(cnt.data(), c->p.ev_cnt, sizeof(int32_t) * c->p.nloc, hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(hipStreamSynchronize(c->stream));
    for (int32_t v : cnt) {
      counts[GM_EV_JOINED] += (uint64_t)(v & 0xFFFF);
      counts[GM_EV_REMOVED] += (uint64_t)(v >> 16);
    }
    counts[0] = counts[GM_EV_JOINED] + counts[GM_EV_REMOVED];
  } else {
    for (const gm_event &e : c->pending) counts[e.kind]++;
  }
  return GM_OK;
}

extern "C" int gm_event_totals(gm_ctx *c, uint64_t totals[6]) {
  if (!c || !totals) return GM_EINVAL;
  TRY(f_settle(c));
  for (int k = 0; k < 6; k++) totals[k] = c->ev_tot[k];
  if (c->cfg.mode == GM_MODE_PARTIAL) return GM_EUNSUPPORTED;
  if (c->cfg.mode == GM_MODE_SCALED) {
    std::vector<uint64_t> cum((size_t)c->n * c->s.nb);
    HIPCHECK(hipMemcpyAsync(cum.data(), c->s.evcum, sizeof(uint64_t) * cum.size(), hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(hipStreamSynchronize(c->stream));
    uint64_t j = 0, r = 0;
    for (uint64_t v : cum) {
      j += (uint32_t)v;
      r += v >> 32;
    }
    totals[GM_EV_JOINED] = j;
    totals[GM_EV_REMOVED] = r;
  }
  totals[0] = 0;
  for (int k = 1; k < 6; k++) totals[0] += totals[k];
  return GM_OK;
}

// FAITHFUL / SCALED: detection records and timeline from the next tick on, for ticks < tmax
extern "C" int gm_detect_record(gm_ctx *c, int32_t tmax) {
  if (!c || tmax <= 0 || tmax > GM_T_LIMIT + 1) return GM_EINVAL;
  if (c->cfg.mode == GM_MODE_PARTIAL) return GM_EUNSUPPORTED;
  if (c->det.tmax) return GM_ESTATE;
  TRY(f_settle(c));  // FAITHFUL: the ticks enqueued so far are collected unrecorded
  const size_t rows = c->cfg.mode == GM_MODE_SCALED ? (size_t)c->s.w : (size_t)c->n;
  std::vector<gm_detect_rec> init(rows, gm_detect_rec{-1, -1, -1, 0u, 0u, 0u, 0ull});
  if (c->cfg.mode == GM_MODE_SCALED) {
    TRY(dalloc(c, &c->det.rec, rows));
    TRY(dalloc(c, &c->det.tl, 3 * (size_t)tmax));
    HIPCHECK(ctx_memset(c, c->det.tl, 0, sizeof(uint64_t) * 3 * (size_t)tmax));
    HIPCHECK(ctx_memcpy(c, c->det.rec, init.data(), sizeof(gm_detect_rec) * rows, hipMemcpyHostToDevice));
  } else {
    c->det.rec_h.swap(init);
    c->det.tl_h.assign(3 * (size_t)tmax, 0);
  }
  c->det.tmax = tmax;
  return GM_OK;
}

extern "C" int gm_detect(gm_ctx *c, gm_detect_rec *out) {
  if (!c || !out) return GM_EINVAL;
  if (!c->det.tmax) return GM_ESTATE;
  TRY(f_settle(c));
  size_t rows = (size_t)c->n, c0 = 0;
  if (c->cfg.mode == GM_MODE_SCALED) {
    rows = (size_t)c->s.w;
    c0 = (size_t)c->s.c0;
    HIPCHECK(ctx_memcpy(c, out, c->det.rec, sizeof(gm_detect_rec) * rows, hipMemcpyDeviceToHost));
  } else {
    memcpy(out, c->det.rec_h.data(), sizeof(gm_detect_rec) * rows);
  }
  for (size_t i = 0; i < rows; i++) out[i].fail_tick = c->failed_h[c0 + i] ? c->fail_t[c0 + i] : -1;
  return GM_OK;
}

extern "C" int gm_detect_timeline(gm_ctx *c, int32_t t, uint64_t *out) {
  if (!c || !out) return GM_EINVAL;
  if (!c->det.tmax) return GM_ESTATE;
  if (t <= 0 || t > c->det.tmax) return GM_EINVAL;
  TRY(f_settle(c));
  if (c->cfg.mode == GM_MODE_SCALED)
    HIPCHECK(ctx_memcpy(c, out, c->det.tl, sizeof(uint64_t) * 3 * (size_t)t, hipMemcpyDeviceToHost));
  else
    memcpy(out, c->det.tl_h.data(), sizeof(uint64_t) * 3 * (size_t)t);
  return GM_OK;
}

// SCALED / PARTIAL: per-tick, per-node entry counts from the next tick on, for ticks < tmax
// (FAITHFUL always counts, as EmulNet does)
extern "C" int gm_msgcount_record(gm_ctx *c, int32_t tmax) {
  if (!c || tmax <= 0 || tmax > GM_T_LIMIT + 1) return GM_EINVAL;
  if (c->cfg.mode == GM_MODE_FAITHFUL) return GM_OK;
  if (c->ticks_done) return GM_ESTATE;  // the received counts need the senders' counts of the tick before
  if (c->cfg.mode == GM_MODE_SCALED ? c->s.mc_sent != nullptr : c->p.mc_sent != nullptr) return GM_ESTATE;
  const size_t rows = c->cfg.mode == GM_MODE_SCALED ? (size_t)c->n : (size_t)c->p.nloc;
  uint32_t *ms = nullptr, *mr = nullptr;
  TRY(dalloc(c, &ms, (size_t)tmax * rows));
  TRY(dalloc(c, &mr, (size_t)tmax * rows));
  HIPCHECK(hipMemsetAsync(ms, 0, sizeof(uint32_t) * tmax * rows, c->stream));
  HIPCHECK(hipMemsetAsync(mr, 0, sizeof(uint32_t) * tmax * rows, c->stream));
  if (c->cfg.mode == GM_MODE_SCALED) {
    TRY(dalloc(c, &c->s.mc_fresh, 2 * rows));
    TRY(dalloc(c, &c->s.mc_rdrop, rows));
    HIPCHECK(hipMemsetAsync(c->s.mc_fresh, 0, sizeof(uint32_t) * 2 * rows, c->stream));
    HIPCHECK(hipMemsetAsync(c->s.mc_rdrop, 0, sizeof(uint32_t) * rows, c->stream));
    c->s.mc_sent = ms;
    c->s.mc_recv = mr;
    c->s.mc_tmax = tmax;
  } else {
    c->p.mc_sent = ms;
    c->p.mc_recv = mr;
    c->p.mc_tmax = tmax;
  }
  return GM_OK;
}

extern "C" int gm_msgcount(gm_ctx *c, int32_t t, int32_t *sent, int32_t *recv) {
  if (!c || !sent || !recv || t < 0) return GM_EINVAL;
  TRY(f_settle(c));  // a column shard's last tick may still owe its host-driven draw rounds
  if (c->cfg.mode != GM_MODE_FAITHFUL) {  // [nodes][t] of this context's nodes, from the recorded history
    const bool sc = c->cfg.mode == GM_MODE_SCALED;
    const uint32_t *ms = sc ? c->s.mc_sent : c->p.mc_sent, *mr = sc ? c->s.mc_recv : c->p.mc_recv;
    const int tmax = sc ? c->s.mc_tmax : c->p.mc_tmax;
    if (!ms) return GM_ESTATE;  // gm_msgcount_record was not called
    if (t > tmax) return GM_EINVAL;
    const size_t rows = sc ? (size_t)c->n : (size_t)c->p.nloc;
    HIPCHECK(hipStreamSynchronize(c->stream));
    std::vector<uint32_t> hs((size_t)t * rows), hr(hs.size());
    if (t > 0) {
      HIPCHECK(ctx_memcpy(c, hs.data(), ms, sizeof(uint32_t) * hs.size(), hipMemcpyDeviceToHost));
      HIPCHECK(ctx_memcpy(c, hr.data(), mr, sizeof(uint32_t) * hr.size(), hipMemcpyDeviceToHost));
    }
    for (size_t i = 0; i < rows; i++)
      for (int j = 0; j < t; j++) {
        sent[i * t + j] = (int32_t)hs[(size_t)j * rows + i];
        recv[i * t + j] = (int32_t)hr[(size_t)j * rows + i];
      }
    return GM_OK;
  }
  if (t > c->f.tmax) return GM_EINVAL;
  TRY(f_settle(c));
  HIPCHECK(hipStreamSynchronize(c->stream));
  std::vector<int32_t> hs((size_t)(c->n + 1) * c->f.tmax), hr(hs.size());
  HIPCHECK(ctx_memcpy(c, hs.data(), c->f.sent, sizeof(int32_t) * hs.size(), hipMemcpyDeviceToHost));
  HIPCHECK(ctx_memcpy(c, hr.data(), c->f.recv, sizeof(int32_t) * hr.size(), hipMemcpyDeviceToHost));
  for (int i = 0; i < c->n; i++)
    for (int j = 0; j < t; j++) {
      sent[(size_t)i * t + j] = hs[(size_t)(i + 1) * c->f.tmax + j];
      recv[(size_t)i * t + j] = hr[(size_t)(i + 1) * c->f.tmax + j];
    }
  return GM_OK;
}
