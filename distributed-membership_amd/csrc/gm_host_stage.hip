// gm_host_stage.hip -- the staged block (gm_stage, gm_host.h) of gm_read_rows, gm_load_* and
// gm_load_views_*: rows per launch, the block itself, the timed spans and the stats.
#include "gm_host.h"

using namespace gmh;

// rows per launch: what `budget` bytes hold at row_bytes each, at most `rows` and at least one; the
// environment variable `env` (diagnostics, tests) asks for smaller launches
int gmh::stage_cap(size_t budget, size_t row_bytes, size_t rows, const char *env) {
  size_t cap = std::min(rows, std::max<size_t>(1, budget / row_bytes));
  if (getenv(env)) cap = std::max<size_t>(1, std::min<size_t>(cap, (size_t)atol(getenv(env))));
  return (int)cap;
}

// a load's block of `bytes` for launches of cap rows, the status word at status_off; one of the same
// cap is kept (a context's cap determines its size)
int gmh::stage_alloc(gm_stage &st, int cap, size_t bytes, size_t status_off, const char *what) {
  if (st.blob && st.cap == cap) return GM_OK;
  stage_free(st);
  if (hipMalloc(&st.blob, bytes) != hipSuccess) {
    st.blob = nullptr;
    snprintf(g_errbuf, sizeof g_errbuf, "hipMalloc(%zu) failed (%s)", bytes, what);
    return GM_ENOMEM;
  }
  st.bytes = bytes;
  st.cap = cap;
  st.status = (uint32_t *)((uint8_t *)st.blob + status_off);
  return GM_OK;
}

void gmh::stage_free(gm_stage &st) {
  if (st.blob) (void)hipFree(st.blob);
  st.blob = nullptr;
  st.status = nullptr;
  st.cap = 0;
}

void gmh::stage_destroy(gm_stage &st, bool owned) {  // owned: the block is not in `allocs`
  if (owned) stage_free(st);
  for (hipEvent_t e : st.ev)
    if (e) (void)hipEventDestroy(e);
}

// The timed spans of a staged call. With gm_set_timing off both return at once: no event call, no wait.
// stage_mark records event k on the stream (created on first use); stage_span waits for event `to` and
// adds the time since event `from` to ms[slot].
int gmh::stage_mark(gm_ctx *c, gm_stage &st, int k) {
  if (!c->timing) return GM_OK;
  if (!st.ev[k]) HIPCHECK(hipEventCreate(&st.ev[k]));
  HIPCHECK(hipEventRecord(st.ev[k], c->stream));
  return GM_OK;
}

int gmh::stage_span(gm_ctx *c, gm_stage &st, int slot, int from, int to) {
  if (!c->timing) return GM_OK;
  float ms = 0;
  HIPCHECK(hipEventSynchronize(st.ev[to]));
  HIPCHECK(hipEventElapsedTime(&ms, st.ev[from], st.ev[to]));
  st.ms[slot] += ms;
  return GM_OK;
}

// what gm_load_stats, gm_load_views_stats and gm_read_rows_stats return for a context of `mode`
int gmh::stage_stats(const gm_ctx *c, int mode, const gm_stage *st, double stats[4]) {
  if (!c || !stats) return GM_EINVAL;
  if (c->cfg.mode != mode) return GM_EUNSUPPORTED;
  stats[0] = (double)st->rows;
  stats[1] = (double)st->bytes;
  stats[2] = st->ms[0];
  stats[3] = st->ms[1];
  return GM_OK;
}
