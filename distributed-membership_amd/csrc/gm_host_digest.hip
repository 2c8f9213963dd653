// gm_host_digest.hip -- state digests (gm_digest.hip): gm_digest, a read-back of the state as of the
// last tick, and the recorder (gm_digest_record, gm_digest_trace), which enqueues the same kernels
// behind each recorded tick and keeps only the two sums per tick on the device.
#include "gm_digest.h"
#include "gm_host.h"

using namespace gmh;

static size_t dg_count(const gm_ctx *c) { return c->cfg.mode == GM_MODE_PARTIAL ? (size_t)c->p.nloc : (size_t)c->n; }
static uint64_t *dg_rows(const gm_ctx *c) { return (uint64_t *)c->dg.blob; }
static uint64_t *dg_nodes(const gm_ctx *c) { return dg_rows(c) + dg_count(c); }
static uint64_t *dg_sums(const gm_ctx *c) { return dg_nodes(c) + dg_count(c); }
static uint32_t *dg_status(const gm_ctx *c) { return (uint32_t *)(dg_sums(c) + 2); }

// Join ramp: the device copy of fail_t, which gm_read_nodes' inGroup rule reads for crashed nodes.
// Called when the scratch is allocated and by gm_set_failed, after the context's stream was waited for.
int gmh::digest_flags(gm_ctx *c) {
  if (!c->dg.fail_t) return GM_OK;
  HIPCHECK(ctx_memcpy(c, c->dg.fail_t, c->fail_t.data(), sizeof(int32_t) * (size_t)c->n, hipMemcpyHostToDevice));
  return GM_OK;
}

// the scratch block: rows, nodes, sums[2], the status word
static int dg_alloc(gm_ctx *c) {
  if (c->dg.blob) return GM_OK;
  uint8_t *blob = nullptr;
  TRY(dalloc(c, &blob, sizeof(uint64_t) * (2 * dg_count(c) + 2) + sizeof(uint64_t)));
  if (c->cfg.mode == GM_MODE_SCALED && c->s.ramp) TRY(dalloc(c, &c->dg.fail_t, (size_t)c->n));
  c->dg.blob = blob;
  return digest_flags(c);
}

// The digest of the state as of tick T, enqueued on st: the word arrays of the scratch, then their
// fold into sums[2] (anywhere on the device); the kernels OR what they find wrong into *status.
static int dg_enqueue(gm_ctx *c, int T, uint64_t *sums, uint32_t *status, hipStream_t st) {
  const size_t count = dg_count(c);
  int r0 = 0;
  if (c->cfg.mode == GM_MODE_SCALED) {
    HIPCHECK(hipMemsetAsync(dg_rows(c), 0, sizeof(uint64_t) * count, st));  // the passes add into it
    HIPCHECK(gm_launch_digest_table(c->s, T, dg_rows(c), status, st));
    HIPCHECK(gm_launch_digest_nodes(c->s, T, c->dg.fail_t, dg_nodes(c), st));
  } else {
    HIPCHECK(gm_launch_digest_views(c->p, T, dg_rows(c), dg_nodes(c), status, st));
    r0 = c->p.n0;
  }
  HIPCHECK(hipMemsetAsync(sums, 0, 2 * sizeof(uint64_t), st));
  HIPCHECK(gm_launch_digest_fold(dg_rows(c), dg_nodes(c), (int)count, r0, sums, st));
  return GM_OK;
}

static const char *const DG_WHAT =
    "the stored state is inconsistent (flags 0x%x: 1 escape lists against cells, 2 a view entry's id)";

extern "C" int gm_digest(gm_ctx *c, uint64_t sums[2], uint64_t *rows, uint64_t *nodes) {
  if (!c || (!sums && !rows && !nodes)) return GM_EINVAL;
  if (c->cfg.mode == GM_MODE_FAITHFUL) return GM_EUNSUPPORTED;
  if (c->ld.loading || c->vl.loading) return GM_ESTATE;  // between a load's begin and its commit
  if (c->cfg.mode == GM_MODE_SCALED) {
    TRY(settled_read(c));
  } else {
    if (c->latched != GM_OK) return c->latched;
    if (c->xch.stream) HIPCHECK(hipStreamSynchronize(c->xch.stream));  // a row shard's exchange and unpacks
    TRY(check_err(c));  // waits for the stream
  }
  TRY(dg_alloc(c));
  HIPCHECK(ctx_memset(c, dg_status(c), 0, sizeof(uint32_t)));
  TRY(dg_enqueue(c, c->t - 1, dg_sums(c), dg_status(c), c->stream));
  // nothing is handed out before the checks pass
  TRY(kernel_status(c, dg_status(c), GM_ESTATE, DG_WHAT));
  const size_t bytes = sizeof(uint64_t) * dg_count(c);
  if (sums) HIPCHECK(ctx_memcpy(c, sums, dg_sums(c), 2 * sizeof(uint64_t), hipMemcpyDeviceToHost));
  if (rows) HIPCHECK(ctx_memcpy(c, rows, dg_rows(c), bytes, hipMemcpyDeviceToHost));
  if (nodes) HIPCHECK(ctx_memcpy(c, nodes, dg_nodes(c), bytes, hipMemcpyDeviceToHost));
  return GM_OK;
}

extern "C" int gm_digest_record(gm_ctx *c, int32_t tmax) {
  if (!c || tmax <= 0 || tmax > GM_T_LIMIT + 1) return GM_EINVAL;
  if (c->cfg.mode == GM_MODE_FAITHFUL) return GM_EUNSUPPORTED;
  // column shards settle their targets in deferred draw rounds, after the point a stream-ordered reducer could run
  if (c->cfg.mode == GM_MODE_SCALED && c->s.sharded) return GM_EUNSUPPORTED;
  if (c->dg.tmax) return GM_ESTATE;
  if (c->ld.loading || c->vl.loading) return GM_ESTATE;
  TRY(dg_alloc(c));
  gm_digest_state &d = c->dg;
  if (!d.trace) TRY(dalloc(c, &d.trace, 2 * (size_t)tmax));
  if (!d.status) TRY(dalloc(c, &d.status, 1));
  HIPCHECK(ctx_memset(c, d.trace, 0, sizeof(uint64_t) * 2 * (size_t)tmax));
  HIPCHECK(ctx_memset(c, d.status, 0, sizeof(uint32_t)));
  HIPCHECK(hipStreamSynchronize(c->stream));  // a row-shard group ticks on its first member's stream
  d.tmax = tmax;
  return GM_OK;
}

// Tick t of context c, enqueued on st behind the tick's last kernel: its digest into row t, while recording
int gmh::digest_tick(gm_ctx *c, int t, hipStream_t st) {
  if (t >= c->dg.tmax) return GM_OK;  // off (tmax 0) or past the recorded window
  return dg_enqueue(c, t, c->dg.trace + 2 * (size_t)t, c->dg.status, st);
}

extern "C" int gm_digest_trace(gm_ctx *c, int32_t t, uint64_t *out) {
  if (!c || !out) return GM_EINVAL;
  if (!c->dg.tmax) return GM_ESTATE;
  if (t <= 0 || t > c->dg.tmax) return GM_EINVAL;
  if (c->xch.stream) HIPCHECK(hipStreamSynchronize(c->xch.stream));
  TRY(kernel_status(c, c->dg.status, GM_ESTATE, DG_WHAT));
  HIPCHECK(ctx_memcpy(c, out, c->dg.trace, sizeof(uint64_t) * 2 * (size_t)t, hipMemcpyDeviceToHost));
  return GM_OK;
}
