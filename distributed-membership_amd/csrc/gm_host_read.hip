// gm_host_read.hip -- read-backs of the state as of the last tick: rows and tables decoded on the host
// or on the device, views, node flags, targets, the rendered dump, and the two censuses.
#include <string>

#include "gm_host.h"

using namespace gmh;

// The escape list of band b of one row -> values by column of the row (esc_row). piece: the row's B
// stored cells of the band; word: the list's record word; extent: the words of its stripe's pool
// region the caller can reach. The cells' escape bytes must number what the word counts and the
// list's pool part must lie within the extent; only then does fetch(k, in, &inl, &pool) name the k
// entries (the inline slot's first `in`, the pool's rest), each of which must sit on an escape byte.
// GM_ESTATE otherwise.
template <class Fetch>
static int place_esc_list(const SState &s, int b, const uint8_t *piece, uint32_t word, size_t extent, uint16_t *esc_row,
                          Fetch fetch) {
  size_t k = 0;
  for (int j = 0; j < s.band; j++) k += s_is_esc(piece[j]);
  if (!k) return GM_OK;
  const size_t in = std::min<size_t>(k, S_ESC_IN);
  if (S_EW_TOT(word) != k || S_EW_OFF(word) + (k - in) > extent) return GM_ESTATE;
  const uint32_t *inl = nullptr, *pool = nullptr;
  TRY(fetch(k, in, &inl, &pool));
  for (size_t i = 0; i < k; i++) {
    const uint32_t e = i < S_ESC_IN ? inl[i] : pool[i - S_ESC_IN];
    const uint32_t col = e & 0xFFFFu;
    if (col >= (uint32_t)s.band || !s_is_esc(piece[col])) return GM_ESTATE;
    esc_row[(size_t)b * s.band + col] = (uint16_t)(e >> 16);
  }
  return GM_OK;
}

// One row of stored bytes (column order) -> absolute (hb, ts), -1 = absent; escaped cells take
// their value from `esc` (per column, from the row's escape entries). Cells are relative to the
// row's last written tick wt.
static void decode_scaled_row(const gm_ctx *c, const uint8_t *row, const uint16_t *esc, int wt,
                              std::vector<int32_t> &hb, std::vector<int32_t> &ts) {
  const SState &s = c->s;
  hb.resize(s.w);
  ts.resize(s.w);
  for (int j = 0; j < s.w; j++) {
    const uint32_t e = s_is_esc(row[j]) ? (uint32_t)esc[j] : s_widen(row[j]);
    hb[j] = e == 0 ? -1 : 2 * wt - 255 + (int32_t)S_H(e) - s_hbase(s.ramp, s.c0 + j);
    ts[j] = e == 0 ? -1 : wt - (int32_t)S_AGE(e);
  }
}

// Row r of this context's table as absolute (hb, ts) per column, -1 = absent.
static int read_table_row(gm_ctx *c, int r, std::vector<int32_t> &hb, std::vector<int32_t> &ts, int &w) {
  if (c->cfg.mode == GM_MODE_FAITHFUL) {
    TRY(f_settle(c));
    w = c->n;
    std::vector<uint32_t> row(w);
    HIPCHECK(ctx_memcpy(c, row.data(), c->f.table + (size_t)r * c->f.np, sizeof(uint32_t) * w, hipMemcpyDeviceToHost));
    hb.resize(w);
    ts.resize(w);
    for (int j = 0; j < w; j++) {
      hb[j] = row[j] == GM_ABSENT ? -1 : (int32_t)(row[j] & 0xFFFF);
      ts[j] = row[j] == GM_ABSENT ? -1 : (int32_t)(row[j] >> 16);
    }
    return GM_OK;
  }
  if (c->cfg.mode == GM_MODE_PARTIAL) {  // the node's V-entry list as of the last tick
    const PState &p = c->p;
    if (r < p.n0 || r >= p.n0 + p.nloc) return GM_EINVAL;  // another row shard's node
    std::vector<uint64_t> lst(p.V);
    HIPCHECK(ctx_memcpy(c, lst.data(), p.lists + ((size_t)((c->t - 1) & 1) * p.rows + (r - p.n0)) * p.V,
                       sizeof(uint64_t) * p.V, hipMemcpyDeviceToHost));
    w = c->n;
    hb.assign(w, -1);
    ts.assign(w, -1);
    for (uint64_t e : lst) {
      if (!e) continue;
      const int id = (int)(e >> 32), h = (int)(uint32_t)e;
      if (id < 1 || id > c->n) return GM_ESTATE;
      hb[id - 1] = h;
      ts[id - 1] = (h + 1) / 2;
    }
    return GM_OK;
  }
  const SState &s = c->s;  // band-tiled: one B-cell piece of the row per band slab
  w = s.w;  // this context's columns
  std::vector<uint8_t> row(s.wp);
  std::vector<uint32_t> eb(s.nb);
  int32_t wt = 0;
  const size_t piece = s.band;  // bytes of one (band, row) piece of the stored cells
  HIPCHECK(ctx_memcpy2d(c, row.data(), piece, s.table + (size_t)r * s.band, piece * s.n, piece, s.nb,
                        hipMemcpyDeviceToHost));
  HIPCHECK(ctx_memcpy2d(c, eb.data(), sizeof(uint32_t), (const uint8_t *)(s.brec + r) + 12, sizeof(uint4) * s.n,
                        sizeof(uint32_t), s.nb, hipMemcpyDeviceToHost));
  HIPCHECK(ctx_memcpy(c, &wt, s.wtick + r, sizeof wt, hipMemcpyDeviceToHost));
  std::vector<uint16_t> esc(s.wp);  // escaped cells by column (the entries of the row's band lists)
  const int par = (c->t - 1) & 1;
  std::vector<uint32_t> ent;
  for (int b = 0; b < s.nb; b++) {
    // only this list's entries are fetched, once its record word has passed the checks
    auto fetch = [&](size_t k, size_t in, const uint32_t **inl, const uint32_t **pool) -> int {
      ent.resize(k);
      HIPCHECK(ctx_memcpy(c, ent.data(), s.tesc_in[par] + ((size_t)b * s.n + r) * S_ESC_IN, sizeof(uint32_t) * in,
                         hipMemcpyDeviceToHost));
      const size_t stripe = ((size_t)b * s.n + r) & (size_t)(s.esc_stripes - 1);
      if (k > in)
        HIPCHECK(ctx_memcpy(c, ent.data() + in, s.tesc[par] + stripe * s.tesc_region + S_EW_OFF(eb[b]),
                           sizeof(uint32_t) * (k - in), hipMemcpyDeviceToHost));
      *inl = ent.data();
      *pool = ent.data() + S_ESC_IN;
      return GM_OK;
    };
    TRY(place_esc_list(s, b, row.data() + (size_t)b * s.band, eb[b], s.tesc_region, esc.data(), fetch));
  }
  decode_scaled_row(c, row.data(), esc.data(), wt, hb, ts);
  return GM_OK;
}

extern "C" int gm_read_row(gm_ctx *c, int32_t r, int32_t c0, int32_t len, int32_t *hb, int32_t *ts) {
  if (!c || !hb || !ts || r < 0 || r >= c->n || c0 < 0 || len < 0) return GM_EINVAL;
  TRY(f_settle(c));
  HIPCHECK(hipStreamSynchronize(c->stream));
  std::vector<int32_t> rh, rt;
  int w;
  TRY(read_table_row(c, r, rh, rt, w));
  if (c0 + len > w) return GM_EINVAL;
  for (int j = 0; j < len; j++) {
    hb[j] = rh[c0 + j];
    ts[j] = rt[c0 + j];
  }
  return GM_OK;
}

// SCALED bulk readback: one copy of the table, the records, the row ticks and the last
// tick's escape entries (inline + each stripe's used pool part), decoded row by row.
struct ScaledSnapshot {
  std::vector<uint8_t> tab, row;
  std::vector<uint4> rec;
  std::vector<std::vector<uint32_t>> pool;  // per stripe: its used part of the region
  std::vector<uint32_t> inl;
  std::vector<uint16_t> esc;
  std::vector<int32_t> wts;
  int load(gm_ctx *c) {
    const SState &s = c->s;
    tab.resize((size_t)s.n * s.wp);
    rec.resize((size_t)s.n * s.nb);
    wts.resize(s.n);
    std::vector<unsigned long long> cnt(s.esc_stripes);
    HIPCHECK(ctx_memcpy(c, tab.data(), s.table, tab.size(), hipMemcpyDeviceToHost));
    HIPCHECK(ctx_memcpy(c, rec.data(), s.brec, sizeof(uint4) * rec.size(), hipMemcpyDeviceToHost));
    HIPCHECK(ctx_memcpy(c, wts.data(), s.wtick, sizeof(int32_t) * s.n, hipMemcpyDeviceToHost));
    const int par = (c->t - 1) & 1;
    HIPCHECK(ctx_memcpy(c, cnt.data(), s.tesc_cnt + (size_t)par * s.esc_stripes, sizeof(unsigned long long) * cnt.size(),
                       hipMemcpyDeviceToHost));
    inl.resize((size_t)s.n * s.nb * S_ESC_IN);
    HIPCHECK(ctx_memcpy(c, inl.data(), s.tesc_in[par], sizeof(uint32_t) * inl.size(), hipMemcpyDeviceToHost));
    pool.assign(s.esc_stripes, {});
    for (int k = 0; k < s.esc_stripes; k++) {
      const size_t used = std::min<unsigned long long>(cnt[k], s.tesc_region);
      pool[k].resize(used);
      if (used)
        HIPCHECK(ctx_memcpy(c, pool[k].data(), s.tesc[par] + (size_t)k * s.tesc_region, sizeof(uint32_t) * used,
                           hipMemcpyDeviceToHost));
    }
    row.resize(s.wp);
    esc.resize(s.wp);
    return GM_OK;
  }
  int decode(const gm_ctx *c, int i, std::vector<int32_t> &rh, std::vector<int32_t> &rt) {
    const SState &s = c->s;
    for (int b = 0; b < s.nb; b++) {
      const uint8_t *pc = tab.data() + ((size_t)b * s.n + i) * s.band;
      memcpy(row.data() + (size_t)b * s.band, pc, s.band);
      const uint32_t w = rec[(size_t)b * s.n + i].w;
      const std::vector<uint32_t> &reg = pool[((size_t)b * s.n + i) & (size_t)(s.esc_stripes - 1)];
      auto fetch = [&](size_t k, size_t in, const uint32_t **li, const uint32_t **lp) -> int {
        *li = inl.data() + ((size_t)b * s.n + i) * S_ESC_IN;
        *lp = reg.data() + (k > in ? S_EW_OFF(w) : 0);
        return GM_OK;
      };
      TRY(place_esc_list(s, b, pc, w, reg.size(), esc.data(), fetch));
    }
    decode_scaled_row(c, row.data(), esc.data(), wts[i], rh, rt);
    return GM_OK;
  }
};

extern "C" int gm_read_table(gm_ctx *c, int32_t r0, int32_t count, int32_t *hb, int32_t *ts) {
  if (!c || r0 < 0 || count < 0 || r0 + (int64_t)count > c->n || (count > 0 && (!hb || !ts))) return GM_EINVAL;
  TRY(f_settle(c));
  HIPCHECK(hipStreamSynchronize(c->stream));
  std::vector<int32_t> rh, rt;
  ScaledSnapshot snap;
  if (c->cfg.mode == GM_MODE_SCALED) TRY(snap.load(c));
  for (int i = 0; i < count; i++) {
    int w;
    if (c->cfg.mode == GM_MODE_SCALED) {
      TRY(snap.decode(c, r0 + i, rh, rt));
      w = c->s.w;
    } else {
      TRY(read_table_row(c, r0 + i, rh, rt, w));
    }
    memcpy(hb + (size_t)i * w, rh.data(), sizeof(int32_t) * w);
    memcpy(ts + (size_t)i * w, rt.data(), sizeof(int32_t) * w);
  }
  return GM_OK;
}

// ------------------------------------------------------------------ SCALED rows decoded on the device
// gm_read_rows (gm_read.hip has the kernel and what it checks): what gm_read_table returns, at a cost
// that follows count, not n. A read-back: it settles the enqueued ticks, reports their device error,
// and writes nothing but its own staging block.
extern "C" int gm_read_rows(gm_ctx *c, int32_t r0, int32_t count, int32_t *hb, int32_t *ts) {
  if (!c) return GM_EINVAL;
  if (c->cfg.mode != GM_MODE_SCALED) return GM_EUNSUPPORTED;
  if (r0 < 0 || count < 0 || r0 + (int64_t)count > c->n || (count > 0 && (!hb || !ts))) return GM_EINVAL;
  TRY(settled_read(c));
  if (count == 0) return GM_OK;
  const SState &s = c->s;
  const size_t w = (size_t)s.w, row_bytes = 2 * sizeof(int32_t) * w;
  gm_stage &rd = c->rd;  // allocated by the first call and reused, in `allocs`: the planes hb, ts [cap][w]
  if (!rd.blob) {        // of one decode launch (bytes: theirs), then the status word
    uint8_t *blob = nullptr;
    const int cap = stage_cap(GM_STAGE_BYTES, row_bytes, (size_t)c->n, "GM_READ_STAGE_ROWS");
    TRY(dalloc(c, &blob, cap * row_bytes + 16));
    rd.blob = blob;
    rd.cap = cap;
    rd.bytes = cap * row_bytes;
    rd.status = (uint32_t *)(blob + rd.bytes);
  }
  int32_t *stage = (int32_t *)rd.blob;
  HIPCHECK(ctx_memset(c, rd.status, 0, sizeof(uint32_t)));
  const int par = (c->t - 1) & 1;
  for (int off = 0; off < count; off += rd.cap) {  // gm_set_timing on: ms[0] the decode kernel, ms[1] the copies
    const int m = std::min(rd.cap, count - off);
    TRY(stage_mark(c, rd, 0));
    HIPCHECK(gm_launch_read_decode(s, par, r0 + off, m, stage, rd.status, c->stream));
    TRY(stage_mark(c, rd, 1));
    // nothing of the block is handed out before its checks pass
    TRY(kernel_status(c, rd.status, GM_ESTATE, "gm_read_rows: the stored state is inconsistent (flags 0x%x)"));
    HIPCHECK(ctx_memcpy(c, hb + (size_t)off * w, stage, sizeof(int32_t) * m * w, hipMemcpyDeviceToHost));
    HIPCHECK(ctx_memcpy(c, ts + (size_t)off * w, stage + (size_t)m * w, sizeof(int32_t) * m * w, hipMemcpyDeviceToHost));
    TRY(stage_mark(c, rd, 2));
    TRY(stage_span(c, rd, 0, 0, 1));
    TRY(stage_span(c, rd, 1, 1, 2));
    rd.rows += m;
  }
  return GM_OK;
}

extern "C" int gm_read_rows_stats(gm_ctx *c, double stats[4]) {
  return stage_stats(c, GM_MODE_SCALED, c ? &c->rd : nullptr, stats);
}

extern "C" int gm_read_views(gm_ctx *c, int32_t r0, int32_t count, uint64_t *out) {
  if (!c || count < 0 || (count > 0 && !out)) return GM_EINVAL;
  if (c->cfg.mode != GM_MODE_PARTIAL) return GM_EUNSUPPORTED;
  const PState &p = c->p;
  if (r0 < p.n0 || r0 + (int64_t)count > (int64_t)p.n0 + p.nloc) return GM_EINVAL;  // this shard's nodes only
  HIPCHECK(hipStreamSynchronize(c->stream));
  if (count)
    HIPCHECK(ctx_memcpy(c, out, p.lists + ((size_t)((c->t - 1) & 1) * p.rows + (r0 - p.n0)) * p.V,
                       sizeof(uint64_t) * p.V * (size_t)count, hipMemcpyDeviceToHost));
  return GM_OK;
}

extern "C" int gm_read_nodes(gm_ctx *c, int32_t *st4) {
  if (!c || !st4) return GM_EINVAL;
  TRY(f_settle(c));
  HIPCHECK(hipStreamSynchronize(c->stream));
  const int n = c->cfg.mode == GM_MODE_PARTIAL ? c->p.nloc : c->n;  // a row shard reports its own nodes
  std::vector<int32_t> a(n), b(n), f(n), h(n);
  if (c->cfg.mode == GM_MODE_FAITHFUL) {
    HIPCHECK(ctx_memcpy(c, a.data(), c->f.inited, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
    HIPCHECK(ctx_memcpy(c, b.data(), c->f.ingroup, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
    HIPCHECK(ctx_memcpy(c, f.data(), c->f.failed, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
    HIPCHECK(ctx_memcpy(c, h.data(), c->f.hbctr, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
  } else {
    const bool part = c->cfg.mode == GM_MODE_PARTIAL;
    std::fill(a.begin(), a.end(), 1);
    std::fill(b.begin(), b.end(), 1);
    if (!part && c->s.ramp) {  // join ramp: started (inited) / in the group as of the last tick
      const int t = c->t - 1;
      for (int i = 0; i < n; i++) {
        a[i] = t >= s_start(i);
        // JOINREP is processed at start+2 only by a node still running then
        b[i] = i == 0 ? a[i] : s_ingroup(1, c->s.intro_until, i, t) && c->fail_t[i] >= s_start(i) + 2;
      }
    }
    HIPCHECK(ctx_memcpy(c, f.data(), part ? c->p.failed : c->s.failed, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
    HIPCHECK(ctx_memcpy(c, h.data(), part ? c->p.hbctr : c->s.hbctr, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
  }
  for (int i = 0; i < n; i++) {
    st4[4 * i] = a[i];
    st4[4 * i + 1] = b[i];
    st4[4 * i + 2] = f[i];
    st4[4 * i + 3] = h[i];
  }
  return GM_OK;
}

// One line of the dump: "t node inited ingroup failed heartbeat count", then the count entries " id:hb:ts"
struct DumpEntry {
  int id, hb, ts;
};

static void dump_line(std::string &out, int t, int node, const int32_t *st4, const std::vector<DumpEntry> &ent) {
  char tmp[96];
  snprintf(tmp, sizeof tmp, "%d %d %d %d %d %d %d", t, node, st4[0], st4[1], st4[2], st4[3], (int)ent.size());
  out += tmp;
  for (const DumpEntry &e : ent) {
    snprintf(tmp, sizeof tmp, " %d:%d:%d", e.id, e.hb, e.ts);
    out += tmp;
  }
  out += "\n";
}

extern "C" int gm_dump_tables(gm_ctx *c, char *buf, size_t cap, size_t *len) {
  if (!c || !len) return GM_EINVAL;
  std::vector<int32_t> st(4 * (size_t)c->n);
  TRY(gm_read_nodes(c, st.data()));
  std::string out;
  std::vector<DumpEntry> ent;
  const int t = c->t - 1;
  if (c->cfg.mode == GM_MODE_PARTIAL) {  // the V-entry lists (id order) of the last tick, one copy
    const PState &p = c->p;          // a row shard renders its own nodes (global indices)
    std::vector<uint64_t> all((size_t)p.nloc * p.V);
    HIPCHECK(ctx_memcpy(c, all.data(), p.lists + (size_t)(t & 1) * p.rows * p.V, sizeof(uint64_t) * all.size(),
                       hipMemcpyDeviceToHost));
    for (int i = 0; i < p.nloc; i++) {
      ent.clear();
      for (int j = 0; j < p.V; j++) {
        const uint64_t e = all[(size_t)i * p.V + j];
        const int h = (int)(uint32_t)e;
        if (e) ent.push_back({(int)(e >> 32), h, (h + 1) / 2});
      }
      dump_line(out, t, p.n0 + i, &st[4 * (size_t)i], ent);
    }
  } else {
    const bool scaled = c->cfg.mode == GM_MODE_SCALED;
    const int c0 = scaled ? c->s.c0 : 0;
    std::vector<int32_t> rh, rt;
    ScaledSnapshot snap;
    if (scaled) TRY(snap.load(c));
    for (int i = 0; i < c->n; i++) {
      int w = c->s.w;
      if (scaled) TRY(snap.decode(c, i, rh, rt));
      else TRY(read_table_row(c, i, rh, rt, w));
      ent.clear();
      for (int j = 0; j < w; j++)
        if (rh[j] >= 0) ent.push_back({c0 + j + 1, rh[j], rt[j]});
      dump_line(out, t, i, &st[4 * (size_t)i], ent);
    }
  }
  *len = out.size();
  if (!buf || cap < out.size()) return GM_ERANGE;
  memcpy(buf, out.data(), out.size());
  return GM_OK;
}

extern "C" int gm_read_targets(gm_ctx *c, int32_t *targets, int32_t *counts) {
  if (!c || !targets || !counts) return GM_EINVAL;
  const bool part = c->cfg.mode == GM_MODE_PARTIAL;
  if (part) {  // this context's own nodes: [nloc][5] global indices, counts [nloc]
    if (c->xch.stream) HIPCHECK(hipStreamSynchronize(c->xch.stream));
    HIPCHECK(hipStreamSynchronize(c->stream));
  } else if (c->cfg.mode == GM_MODE_SCALED) {
    TRY(draw_settle(&c, 1));
  } else {
    return GM_EUNSUPPORTED;
  }
  const size_t rows = part ? (size_t)c->p.nloc : (size_t)c->n;
  std::vector<int32_t> st(rows * 4);
  HIPCHECK(ctx_memcpy(c, targets, part ? c->p.targets : c->s.targets, sizeof(int32_t) * rows * GM_FANOUT, hipMemcpyDeviceToHost));
  HIPCHECK(ctx_memcpy(c, st.data(), part ? c->p.rowstat : c->s.rowstat, sizeof(int32_t) * rows * 4, hipMemcpyDeviceToHost));
  for (size_t r = 0; r < rows; r++) {
    counts[r] = st[r * 4 + 3];
    for (int q = counts[r]; q < GM_FANOUT; q++) targets[r * GM_FANOUT + q] = 0;
  }
  return check_err(c);
}

// SCALED: the census of the state as of the last tick (gm_census.hip). A read-back: it settles the
// enqueued ticks, reports their device error, and writes nothing but its own scratch.
extern "C" int gm_census(gm_ctx *c, gm_census_rec *out, uint64_t *hist) {
  if (!c || (!out && !hist)) return GM_EINVAL;
  if (c->cfg.mode != GM_MODE_SCALED) return GM_EUNSUPPORTED;
  TRY(settled_read(c));
  const SState &s = c->s;
  const size_t rec_bytes = sizeof(gm_census_rec) * (size_t)s.w;
  const size_t hist_bytes = sizeof(uint64_t) * 2 * GM_CENSUS_LAGS * GM_CENSUS_AGES;
  if (!c->cen.blob) TRY(dalloc(c, &c->cen.blob, rec_bytes + hist_bytes + sizeof(uint64_t)));
  gm_census_rec *d_rec = (gm_census_rec *)c->cen.blob;
  uint64_t *d_hist = (uint64_t *)(c->cen.blob + rec_bytes);
  uint32_t *d_status = (uint32_t *)(c->cen.blob + rec_bytes + hist_bytes);
  HIPCHECK(ctx_memset(c, c->cen.blob, 0, rec_bytes + hist_bytes + sizeof(uint64_t)));
  HIPCHECK(gm_launch_census(s, d_rec, d_hist, d_status, c->t - 1, c->stream));
  TRY(kernel_status(c, d_status, GM_ESTATE, "gm_census: the stored state is inconsistent (flags 0x%x)"));
  if (out) HIPCHECK(ctx_memcpy(c, out, d_rec, rec_bytes, hipMemcpyDeviceToHost));
  if (hist) HIPCHECK(ctx_memcpy(c, hist, d_hist, hist_bytes, hipMemcpyDeviceToHost));
  return GM_OK;
}

// PARTIAL: the view census of the state as of the last tick (gm_view_census.hip). A read-back: it
// waits for the enqueued ticks, reports their device error, and writes nothing but its own scratch.
extern "C" int gm_view_census(gm_ctx *c, gm_view_rec *out, uint64_t *hist, uint64_t *sizes) {
  if (!c || (!out && !hist && !sizes)) return GM_EINVAL;
  if (c->cfg.mode != GM_MODE_PARTIAL) return GM_EUNSUPPORTED;
  if (c->latched != GM_OK) return c->latched;
  if (c->xch.stream) HIPCHECK(hipStreamSynchronize(c->xch.stream));  // a row shard's exchange and unpacks
  TRY(check_err(c));  // waits for the stream
  const PState &p = c->p;
  const size_t n = (size_t)p.n;
  const size_t acc_bytes = 16 * n, hist_bytes = sizeof(uint64_t) * 2 * GM_VIEW_AGES;
  const size_t sizes_bytes = sizeof(uint64_t) * GM_VIEW_SIZES, cls_words = (n + 31) / 32;
  const size_t zero_bytes = acc_bytes + hist_bytes + sizes_bytes + sizeof(uint64_t);  // all but the bitmap
  if (!c->vc.blob) TRY(dalloc(c, &c->vc.blob, zero_bytes + sizeof(uint32_t) * cls_words));
  if (out && !c->vc.rec) TRY(dalloc(c, &c->vc.rec, n));
  uint64_t *d_hist = (uint64_t *)(c->vc.blob + acc_bytes);
  uint64_t *d_sizes = (uint64_t *)(c->vc.blob + acc_bytes + hist_bytes);
  uint32_t *d_status = (uint32_t *)(c->vc.blob + acc_bytes + hist_bytes + sizes_bytes);
  uint32_t *d_cls = (uint32_t *)(c->vc.blob + zero_bytes);
  HIPCHECK(ctx_memset(c, c->vc.blob, 0, zero_bytes));
  if (c->vc.nfailed != c->nfailed) {  // the subjects' classes: every shard is given the whole crash set.
    // PARTIAL crash flags are only ever set, so the count of set flags names the set the bitmap holds
    const std::vector<uint32_t> cls = crash_bitmap(c);
    HIPCHECK(ctx_memcpy(c, d_cls, cls.data(), sizeof(uint32_t) * cls_words, hipMemcpyHostToDevice));
    c->vc.nfailed = c->nfailed;
  }
  HIPCHECK(gm_launch_view_census(p, d_cls, c->vc.blob, out ? c->vc.rec : nullptr, d_hist, d_sizes, d_status, c->t - 1,
                                 c->stream));
  TRY(kernel_status(c, d_status, GM_ESTATE,
                    "gm_view_census: a stored view cannot be right (flags 0x%x: 1 id, 2 heartbeat, 4 age)"));
  if (out) HIPCHECK(ctx_memcpy(c, out, c->vc.rec, sizeof(gm_view_rec) * n, hipMemcpyDeviceToHost));
  if (hist) HIPCHECK(ctx_memcpy(c, hist, d_hist, hist_bytes, hipMemcpyDeviceToHost));
  if (sizes) HIPCHECK(ctx_memcpy(c, sizes, d_sizes, sizes_bytes, hipMemcpyDeviceToHost));
  return GM_OK;
}

// PARTIAL: reachability in the view graph as of the last tick (gm_view_reach.hip). A read-back with the
// census's preamble; it writes nothing but its own scratch. A context with a communicator walks with its
// peers (gm_host_view_reach.hip); what follows is the single context. One launch pair per level on the context's
// stream; the level's row of counts comes back before the next one is enqueued, and the walk stops at an
// empty level, at max_hops, or once every live source has reached every live node.
extern "C" int gm_view_reach(gm_ctx *c, const int32_t *sources, int32_t nsrc, int32_t dir, int32_t max_hops,
                             uint64_t *counts, uint64_t *seen, int64_t info[4]) {
  if (!c) return GM_EINVAL;
  if (c->cfg.mode != GM_MODE_PARTIAL) return GM_EUNSUPPORTED;
  const PState &p = c->p;
  if (c->comm) {  // an RCCL rank: the collective walk (gm_host_view_reach.hip), whatever the shard count
    TRY(view_reach_args(p.n, sources, nsrc, dir, max_hops, counts, info));
    return view_reach_group(&c, 1, sources, nsrc, dir, max_hops, counts, seen, info);
  }
  if (c->cfg.shard_count > 1 || p.nloc != p.n) return GM_EUNSUPPORTED;  // a row shard without peers to exchange with
  TRY(view_reach_args(p.n, sources, nsrc, dir, max_hops, counts, info));
  if (c->vl.loading) return GM_ESTATE;  // between gm_load_views_begin and the commit
  if (c->latched != GM_OK) return c->latched;
  if (c->xch.stream) HIPCHECK(hipStreamSynchronize(c->xch.stream));  // one rank forced into the sharded tick
  TRY(check_err(c));  // waits for the stream
  const size_t n = (size_t)p.n, words = sizeof(uint64_t) * n;
  const size_t row_bytes = sizeof(uint64_t) * GM_REACH_SOURCES, counts_bytes = row_bytes * GM_VIEW_HOPS;
  const size_t src_off = 3 * words + counts_bytes, status_off = src_off + sizeof(int32_t) * GM_REACH_SOURCES;
  if (!c->vr.blob) TRY(dalloc(c, &c->vr.blob, status_off + sizeof(uint64_t)));
  uint64_t *d_seen = (uint64_t *)c->vr.blob, *d_front = d_seen + n, *d_next = d_front + n, *d_counts = d_next + n;
  int32_t *d_src = (int32_t *)(c->vr.blob + src_off);
  uint32_t *d_status = (uint32_t *)(c->vr.blob + status_off);
  HIPCHECK(ctx_memset(c, c->vr.blob, 0, status_off + sizeof(uint64_t)));
  HIPCHECK(ctx_memcpy(c, d_src, sources, sizeof(int32_t) * nsrc, hipMemcpyHostToDevice));
  HIPCHECK(gm_launch_view_reach_seed(p, d_src, nsrc, d_seen, d_front, d_counts, c->stream));
  std::vector<uint64_t> cnt((size_t)GM_VIEW_HOPS * GM_REACH_SOURCES, 0);
  HIPCHECK(ctx_memcpy(c, cnt.data(), d_counts, row_bytes, hipMemcpyDeviceToHost));
  // the device's crash flags are failed_h's (gm_set_failed, the load's commit), so nfailed counts them
  const uint64_t live = (uint64_t)(p.n - c->nfailed);
  uint64_t full = 0, reached[GM_REACH_SOURCES];
  int64_t live_sources = 0;
  for (int k = 0; k < GM_REACH_SOURCES; k++) {
    reached[k] = cnt[k];
    if (cnt[k]) full |= 1ull << k;
    live_sources += cnt[k] != 0;
  }
  for (int h = 1; h < max_hops && full; h++) {
    bool all = true;  // every live source has reached every live node: the next level is empty
    for (int k = 0; k < nsrc; k++) all = all && (!((full >> k) & 1) || reached[k] == live);
    if (all) break;
    HIPCHECK(gm_launch_view_reach_hop(p, c->t - 1, dir, h, nsrc, full, d_seen, d_front, d_next, d_counts, d_status,
                                      c->stream));
    uint64_t *row = cnt.data() + (size_t)h * GM_REACH_SOURCES;
    HIPCHECK(ctx_memcpy(c, row, d_counts + (size_t)h * GM_REACH_SOURCES, row_bytes, hipMemcpyDeviceToHost));
    bool any = false;
    for (int k = 0; k < GM_REACH_SOURCES; k++) {
      reached[k] += row[k];
      any = any || row[k];
    }
    if (!any) break;
  }
  // nothing is handed out before the walk's checks pass
  TRY(kernel_status(c, d_status, GM_ESTATE, "gm_view_reach: a stored view names an id outside [1, n] (flags 0x%x)"));
  int hops = 0;
  for (int h = 0; h < max_hops; h++)
    for (int k = 0; k < GM_REACH_SOURCES; k++)
      if (cnt[(size_t)h * GM_REACH_SOURCES + k]) hops = h;
  bool last = false;
  for (int k = 0; k < GM_REACH_SOURCES; k++) last = last || cnt[(size_t)(max_hops - 1) * GM_REACH_SOURCES + k];
  if (seen) HIPCHECK(ctx_memcpy(c, seen, d_seen, words, hipMemcpyDeviceToHost));
  if (counts) memcpy(counts, cnt.data(), counts_bytes);
  if (info) {
    info[0] = (int64_t)live;
    info[1] = hops;
    info[2] = last ? 1 : 0;
    info[3] = live_sources;
  }
  return GM_OK;
}
