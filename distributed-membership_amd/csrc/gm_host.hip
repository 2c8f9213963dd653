// gm_host.hip -- libgm: the C ABI of include/gm_abi.h on top of the HIP kernels.
//
// The host side owns the per-context device state, launches one tick per gm_tick on the context
// stream, and turns device event records into reference log order. gm_host.h maps the units; this
// one creates and destroys a context, dispatches the tick by mode, latches device errors and holds
// the small calls that belong to no mode.
#include <chrono>
#include <utility>

#include "gm_host.h"

using namespace gmh;

thread_local char gmh::g_errbuf[256];

extern "C" const char *gm_strerror(int code) {
  switch (code) {
    case GM_OK: return "ok";
    case GM_EINVAL: return "invalid argument";
    case GM_ENOMEM: return g_errbuf[0] ? g_errbuf : "out of memory";
    case GM_EDEVICE: return g_errbuf[0] ? g_errbuf : "HIP runtime error";
    case GM_ERANGE: return "bounded resource overflowed";
    case GM_ESTATE: return "protocol invariant violated";
    case GM_EUNSUPPORTED: return "unsupported configuration";
    case GM_ECOMM: return g_errbuf[0] ? g_errbuf : "collective failure";
    default: return "unknown error";
  }
}

// Params::setparams (Params.cpp:19-40): same fscanf key sequence
extern "C" int gm_parse_conf(const char *path, gm_config *cfg) {
  if (!path || !cfg) return GM_EINVAL;
  FILE *fp = fopen(path, "r");
  if (!fp) return GM_EINVAL;
  int n = 0, single = 0, drop = 0;
  double prob = 0;
  if (fscanf(fp, "MAX_NNB: %d", &n) != 1) n = 0;
  if (fscanf(fp, "\nSINGLE_FAILURE: %d", &single) != 1) single = 0;
  if (fscanf(fp, "\nDROP_MSG: %d", &drop) != 1) drop = 0;
  if (fscanf(fp, "\nMSG_DROP_PROB: %lf", &prob) != 1) prob = 0;
  fclose(fp);
  cfg->n = n;
  cfg->single_failure = single;
  cfg->drop_msg = drop;
  cfg->drop_prob = prob;
  return n > 0 ? GM_OK : GM_EINVAL;
}

// diagnostics (GM_CREATE_TIMING): where context creation time goes
static std::chrono::steady_clock::time_point g_ctime;
void gmh::lap(const char *what) {
  if (!getenv("GM_CREATE_TIMING")) return;
  const auto t1 = std::chrono::steady_clock::now();
  fprintf(stderr, "[gm] create: %-24s %7.2f ms\n", what, std::chrono::duration<double, std::milli>(t1 - g_ctime).count());
  g_ctime = t1;
}

extern "C" int gm_create(const gm_config *cfg, gm_ctx **out) {
  if (!cfg || !out) return GM_EINVAL;
  *out = nullptr;
  if (cfg->abi_version != GM_ABI_VERSION) return GM_EINVAL;
  if (cfg->n <= 0 || (cfg->mode != GM_MODE_FAITHFUL && cfg->mode != GM_MODE_SCALED && cfg->mode != GM_MODE_PARTIAL))
    return GM_EINVAL;
  g_errbuf[0] = 0;
  gm_ctx *c = new gm_ctx();
  c->cfg = *cfg;
  c->n = cfg->n;
  c->failed_h.assign(cfg->n, 0);
  c->fail_t.assign(cfg->n, 0x7FFFFFFF);
  int rc = GM_OK;
  g_ctime = std::chrono::steady_clock::now();
  if (hipSetDevice(cfg->device) != hipSuccess) rc = GM_EDEVICE;
  lap("hipSetDevice");
  if (rc == GM_OK && hipFree(nullptr) != hipSuccess) rc = GM_EDEVICE;  // runtime + device init
  lap("runtime init");
  if (rc != GM_OK || hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreate(&c->e0) != hipSuccess || hipEventCreate(&c->e1) != hipSuccess ||
      hipEventCreate(&c->k0) != hipSuccess || hipEventCreate(&c->k1) != hipSuccess) {
    snprintf(g_errbuf, sizeof g_errbuf, "HIP device %d unavailable", cfg->device);
    rc = GM_EDEVICE;
  }
  lap("stream + events");
  if (rc == GM_OK)
    rc = cfg->mode == GM_MODE_FAITHFUL ? create_faithful(c) : cfg->mode == GM_MODE_SCALED ? create_scaled(c)
                                                                                        : create_partial(c);
  lap("mode state");
  if (rc != GM_OK) {
    gm_destroy(c);
    return rc;
  }
  *out = c;
  return GM_OK;
}

// inbox slots per receiver: the compiled capacity; GM_INBOX_CAP (diagnostics, tests) lowers it
// to show that an overflow fails loudly (GM_ERR_INBOX -> GM_ERANGE), never silently
int gmh::inbox_cap(int cap) {
  const char *e = getenv("GM_INBOX_CAP");
  return e ? std::max(1, std::min(cap, atoi(e))) : cap;
}

// the exchange stream and events of a sharded context (column or row shards), one event per chunk
int gmh::exchange_create(gm_ctx *c, int chunks) {
  HIPCHECK(hipStreamCreateWithFlags(&c->xch.stream, hipStreamNonBlocking));
  c->xch.chunk_ev.assign(chunks, nullptr);
  for (hipEvent_t &e : c->xch.chunk_ev) HIPCHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  HIPCHECK(hipEventCreateWithFlags(&c->xch.done, hipEventDisableTiming));
  return GM_OK;
}

// Streams are synchronised before anything is freed; the communicator goes before the buffers; every
// feature and mode then frees what it created outside `allocs`.
extern "C" int gm_destroy(gm_ctx *c) {
  if (!c) return GM_EINVAL;
  if (c->batch) return GM_ESTATE;  // gm_batch_destroy first: the batch's slots point into this context
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->ph.side) (void)hipStreamSynchronize(c->ph.side);  // the S2 prefetch of tick t+1 may still be writing
  if (c->xch.stream) (void)hipStreamSynchronize(c->xch.stream);
  if (c->comm) (void)ncclCommDestroy(c->comm);
  for (void *p : c->allocs) (void)hipFree(p);
  stage_destroy(c->ld, true);
  stage_destroy(c->vl, true);
  stage_destroy(c->rd, false);  // its block was in `allocs`
  destroy_scaled(c);
  destroy_faithful(c);
  for (hipEvent_t e : {c->e0, c->e1, c->k0, c->k1})
    if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : c->tev) (void)hipEventDestroy(e);
  for (hipEvent_t e : c->xch.chunk_ev) (void)hipEventDestroy(e);
  if (c->xch.done) (void)hipEventDestroy(c->xch.done);
  if (c->xch.stream) (void)hipStreamDestroy(c->xch.stream);
  destroy_partial(c);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
  return GM_OK;
}

// A device error word -> the latched code and gm_strerror's detail
void gmh::latch_device_error(gm_ctx *c, uint32_t flags) {
  if (!flags) return;
  snprintf(g_errbuf, sizeof g_errbuf, "device error flags 0x%x", flags);
  c->latched = (flags & (GM_ERR_SELF | GM_ERR_BUFFER)) ? GM_ESTATE : GM_ERANGE;
}

int gmh::check_err(gm_ctx *c) {
  uint32_t *errp = c->cfg.mode == GM_MODE_FAITHFUL ? c->f.err : c->cfg.mode == GM_MODE_SCALED ? c->s.err : c->p.err;
  uint32_t e = 0;
  HIPCHECK(hipMemcpyAsync(&e, errp, sizeof e, hipMemcpyDeviceToHost, c->stream));
  HIPCHECK(hipStreamSynchronize(c->stream));
  latch_device_error(c, e);
  return c->latched;
}

// The preamble of a SCALED read-back (gm_census, gm_read_rows, gm_load_begin): not during a load, not
// after a latched error; it settles the enqueued ticks and reports their device error (waits for the stream)
int gmh::settled_read(gm_ctx *c) {
  if (c->ld.loading) return GM_ESTATE;  // between gm_load_begin and gm_load_commit
  if (c->latched != GM_OK) return c->latched;
  TRY(draw_settle(&c, 1));
  return check_err(c);
}

// The status word of a feature's kernels (waits for the stream): non-zero -> `code`, with fmt (one %x:
// the flags) as gm_strerror's detail
int gmh::kernel_status(gm_ctx *c, const uint32_t *d_status, int code, const char *fmt, uint32_t *flags) {
  uint32_t st = 0;
  HIPCHECK(ctx_memcpy(c, &st, d_status, sizeof st, hipMemcpyDeviceToHost));
  if (flags) *flags = st;
  if (!st) return GM_OK;
  snprintf(g_errbuf, sizeof g_errbuf, fmt, st);
  return code;
}

// Everything that reads the state (records, tables, counters, the S1 stream) or starts the
// next tick first completes the enqueued ticks: FAITHFUL collects its mailboxes; a column
// shard finishes the draws its bounded rounds left (rare).
int gmh::f_settle(gm_ctx *c) {
  return c->cfg.mode == GM_MODE_FAITHFUL ? f_collect(c) : c->cfg.mode == GM_MODE_SCALED ? draw_settle(&c, 1) : GM_OK;
}

// Tick-kernel timing: a ring of GM_TEV_RING event pairs on the tick's stream; a slot
// is folded into kernel_ms_sum when it is reused (its tick finished long before).
int gmh::timing_slot(gm_ctx *c, hipEvent_t *k0, hipEvent_t *k1, hipStream_t st) {
  if (c->timed_ticks == 0) HIPCHECK(hipEventRecord(c->e0, st));
  while (c->tev.size() < 2 * (size_t)GM_TEV_RING) {
    hipEvent_t e;
    HIPCHECK(hipEventCreate(&e));
    c->tev.push_back(e);
  }
  const int slot = c->ktimed % GM_TEV_RING;
  if (c->ktimed >= GM_TEV_RING) {
    float x = 0;
    HIPCHECK(hipEventSynchronize(c->tev[2 * slot + 1]));
    HIPCHECK(hipEventElapsedTime(&x, c->tev[2 * slot], c->tev[2 * slot + 1]));
    c->kernel_ms_sum += x;
  }
  *k0 = c->tev[2 * slot];
  *k1 = c->tev[2 * slot + 1];
  c->ktimed++;
  return GM_OK;
}

void gmh::advance(gm_ctx *c) {  // a tick was enqueued: globaltime moves on
  c->t++;
  c->ticks_done++;
  c->undrained = c->cfg.mode != GM_MODE_FAITHFUL;
}

extern "C" int gm_tick(gm_ctx *c) {
  if (!c) return GM_EINVAL;
  if (c->latched != GM_OK) return c->latched;
  if (c->ld.loading || c->vl.loading) return GM_ESTATE;  // between gm_load_begin / gm_load_views_begin and the commit
  if (c->cfg.mode == GM_MODE_SCALED) TRY(draw_settle(&c, 1));
  TRY(before_tick_events(c));
  int rc = c->cfg.mode == GM_MODE_FAITHFUL ? tick_faithful(c) : c->cfg.mode == GM_MODE_SCALED ? tick_scaled(c)
                                                                                             : tick_partial(&c, 1);
  if (rc == GM_OK) advance(c);
  return rc;
}

extern "C" int gm_sync(gm_ctx *c) {
  if (!c) return GM_EINVAL;
  TRY(f_settle(c));  // a sharded tick's remaining draw rounds
  HIPCHECK(hipStreamSynchronize(c->stream));
  return check_err(c);
}

extern "C" int gm_time(gm_ctx *c, int32_t *t) {
  if (!c || !t) return GM_EINVAL;
  *t = c->t;
  return GM_OK;
}

extern "C" int gm_rand(gm_ctx *c, int32_t *out) {
  if (!c || !out) return GM_EINVAL;
  if (c->cfg.mode != GM_MODE_FAITHFUL) return GM_EUNSUPPORTED;
  TRY(f_settle(c));
  int32_t st[33];
  HIPCHECK(hipMemcpyAsync(st, c->f.s1, sizeof st, hipMemcpyDeviceToHost, c->stream));
  HIPCHECK(hipStreamSynchronize(c->stream));
  int f = st[31], r = st[32];
  uint32_t v = (uint32_t)st[f] + (uint32_t)st[r];
  st[f] = (int32_t)v;
  st[31] = (f + 1) % 31;
  st[32] = (r + 1) % 31;
  HIPCHECK(ctx_memcpy(c, c->f.s1, st, sizeof st, hipMemcpyHostToDevice));
  *out = (int32_t)(v >> 1);
  return GM_OK;
}

extern "C" int gm_set_failed(gm_ctx *c, const int32_t *idx, int32_t n) {
  if (!c || n < 0 || (n > 0 && !idx)) return GM_EINVAL;
  for (int k = 0; k < n; k++)  // validate everything before any state changes
    if (idx[k] < 0 || idx[k] >= c->n) return GM_EINVAL;
  if (c->ld.loading || c->vl.loading) return GM_ESTATE;  // the commit sets the crash flags
  TRY(f_settle(c));
  for (int k = 0; k < n; k++) {
    c->nfailed += c->failed_h[idx[k]] == 0;
    if (!c->failed_h[idx[k]]) c->fail_t[idx[k]] = c->t - 1;
    c->failed_h[idx[k]] = 1;
    // join ramp: the introducer's last tick bounds who gets a JOINREP
    if (idx[k] == 0 && c->cfg.mode == GM_MODE_SCALED && c->s.ramp) c->s.intro_until = std::min(c->s.intro_until, c->t - 1);
  }
  int32_t *dst = c->cfg.mode == GM_MODE_FAITHFUL ? c->f.failed : c->cfg.mode == GM_MODE_SCALED ? c->s.failed : c->p.failed;
  const bool part = c->cfg.mode == GM_MODE_PARTIAL;  // a row shard holds its own nodes' flags only
  HIPCHECK(hipStreamSynchronize(c->stream));
  HIPCHECK(ctx_memcpy(c, dst, c->failed_h.data() + (part ? c->p.n0 : 0), sizeof(int32_t) * (part ? c->p.nloc : c->n),
                     hipMemcpyHostToDevice));
  if (part && c->ph.sharded) TRY(partial_caps(c));  // the exchange blocks follow the live nodes per shard
  if (part) TRY(view_detect_flags(c));  // while recording: the crash bitmap the next tick's reducer reads
  TRY(digest_flags(c));  // join ramp, once a digest was taken: the crashed nodes' last ticks on the device
  return GM_OK;
}

extern "C" int gm_set_dropmsg(gm_ctx *c, int32_t on) {
  if (!c) return GM_EINVAL;
  c->dropmsg = on ? 1 : 0;
  return GM_OK;
}

extern "C" int gm_tick_stats(gm_ctx *c, int64_t stats[4]) {
  if (!c || !stats) return GM_EINVAL;
  if (c->cfg.mode == GM_MODE_FAITHFUL) return GM_EUNSUPPORTED;
  const bool part = c->cfg.mode == GM_MODE_PARTIAL;
  const int rows = part ? c->p.nloc : c->n, r0 = part ? c->p.n0 : 0;  // a row shard reports its own nodes
  std::vector<int32_t> rs((size_t)rows * 4);
  uint32_t e = 0;
  HIPCHECK(hipMemcpyAsync(rs.data(), part ? c->p.rowstat : c->s.rowstat, sizeof(int32_t) * rs.size(),
                          hipMemcpyDeviceToHost, c->stream));
  HIPCHECK(hipMemcpyAsync(&e, part ? c->p.err : c->s.err, sizeof e, hipMemcpyDeviceToHost, c->stream));
  HIPCHECK(hipStreamSynchronize(c->stream));
  int64_t m = 0, live = 0, mx = 0;
  for (int r = 0; r < rows; r++) {
    m += rs[4 * r];
    mx = std::max<int64_t>(mx, rs[4 * r]);
    live += c->failed_h[r0 + r] ? 0 : 1;
  }
  stats[0] = m;
  stats[1] = live;
  stats[2] = mx;
  stats[3] = e;
  return GM_OK;
}

extern "C" int gm_pool_info(gm_ctx *c, int64_t info[4]) {
  if (!c || !info) return GM_EINVAL;
  if (c->cfg.mode != GM_MODE_SCALED) return GM_EUNSUPPORTED;
  info[0] = c->s.esc_dense;
  info[1] = (int64_t)c->s.tesc_cap;
  info[2] = (int64_t)c->s.pesc_cap;
  info[3] = (int64_t)c->s.ev_spill_cap;
  return GM_OK;
}

extern "C" int gm_set_timing(gm_ctx *c, int32_t on) {
  if (!c) return GM_EINVAL;
  c->timing = on != 0;
  c->timed_ticks = 0;  // (re)opens the timing window at the next tick
  c->ktimed = 0;
  c->kernel_ms_sum = 0;
  return GM_OK;
}

extern "C" int gm_last_kernel_ms(gm_ctx *c, float *ms) {
  if (!c || !ms) return GM_EINVAL;
  *ms = 0.f;
  if (!c->timing || c->cfg.mode == GM_MODE_FAITHFUL || c->timed_ticks == 0) return GM_OK;
  HIPCHECK(hipEventSynchronize(c->e1));
  double sum = c->kernel_ms_sum;  // folded ring slots + the pairs still in the ring
  for (int k = std::max(0, c->ktimed - GM_TEV_RING); k < c->ktimed; k++) {
    const int slot = k % GM_TEV_RING;
    float x = 0;
    HIPCHECK(hipEventElapsedTime(&x, c->tev[2 * slot], c->tev[2 * slot + 1]));
    sum += x;
  }
  *ms = c->ktimed ? (float)(sum / c->ktimed) : 0.f;
  return GM_OK;
}

static uint64_t mix64h(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
  return z ^ (z >> 31);
}

extern "C" int gm_crash_set(int32_t n, int32_t count, uint64_t seed, int32_t *out) {
  if (n <= 0 || count < 0 || count > n || (count && !out)) return GM_EINVAL;
  std::vector<std::pair<uint64_t, int32_t>> k(n);
  for (int i = 0; i < n; i++) k[i] = {mix64h(seed + 0x9E3779B97F4A7C15ULL * (uint64_t)(i + 1)), i};
  std::partial_sort(k.begin(), k.begin() + count, k.end());
  for (int i = 0; i < count; i++) out[i] = k[i].second;
  std::sort(out, out + count);
  return GM_OK;
}
