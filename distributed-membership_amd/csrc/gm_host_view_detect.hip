// gm_host_view_detect.hip -- PARTIAL detection recorder (gm_view_detect_record, gm_view_detect,
// gm_view_detect_timeline): the state behind gm_view_detect.hip's reducer. Everything lives on the
// device from the record call on (freed with the context's allocations by gm_destroy); a tick only
// enqueues the reducer, and only while its t is below tmax.
#include "gm_host.h"

using namespace gmh;

// The crash bitmap of the whole cluster from failed_h, for the ticks from now on. Called when
// recording starts and by gm_set_failed while recording, after the context's stream was waited for:
// the reducer of the last tick has read the bitmap that tick saw.
int gmh::view_detect_flags(gm_ctx *c) {
  if (!c->vdet.tmax) return GM_OK;
  const std::vector<uint32_t> cls = crash_bitmap(c);
  HIPCHECK(ctx_memcpy(c, c->vdet.cls, cls.data(), sizeof(uint32_t) * cls.size(), hipMemcpyHostToDevice));
  return GM_OK;
}

// Tick t of context c, enqueued on st after the tick's node kernels: the reducer, while recording
int gmh::view_detect_tick(gm_ctx *c, int t, hipStream_t st) {
  if (t >= c->vdet.tmax) return GM_OK;  // off (tmax 0) or past the recorded window
  HIPCHECK(gm_launch_view_detect(c->p, c->vdet.cls, c->vdet.rec, c->vdet.tl + (size_t)GM_VIEW_DETECT_COLS * t,
                                 c->vdet.status, t, st));
  return GM_OK;
}

extern "C" int gm_view_detect_record(gm_ctx *c, int32_t tmax) {
  if (!c || tmax <= 0 || tmax > GM_T_LIMIT + 1) return GM_EINVAL;
  if (c->cfg.mode != GM_MODE_PARTIAL) return GM_EUNSUPPORTED;
  if (c->vdet.tmax) return GM_ESTATE;
  if (c->vl.loading) return GM_ESTATE;  // the commit sets the crash flags
  gm_view_detect_state &d = c->vdet;
  const size_t n = (size_t)c->n, tl_words = (size_t)GM_VIEW_DETECT_COLS * (size_t)tmax;
  TRY(dalloc(c, &d.rec, n));
  TRY(dalloc(c, &d.tl, tl_words));
  TRY(dalloc(c, &d.cls, (n + 31) / 32));
  TRY(dalloc(c, &d.status, 1));
  gm_view_detect_rec none{};
  none.fail_tick = none.first_removed = none.last_removed = none.last_held = -1;
  std::vector<gm_view_detect_rec> init(n, none);
  HIPCHECK(ctx_memset(c, d.tl, 0, sizeof(uint64_t) * tl_words));
  HIPCHECK(ctx_memset(c, d.status, 0, sizeof(uint32_t)));
  HIPCHECK(ctx_memcpy(c, d.rec, init.data(), sizeof(gm_view_detect_rec) * n, hipMemcpyHostToDevice));
  d.tmax = tmax;
  return view_detect_flags(c);
}

// what a read of the recorder starts with: the reducers enqueued so far are done and met nothing wrong
static int view_detect_settled(gm_ctx *c) {
  if (!c->vdet.tmax) return GM_ESTATE;
  return kernel_status(c, c->vdet.status, GM_ESTATE,
                       "gm_view_detect: a recorded tick left a view or a removal record that cannot be right "
                       "(flags 0x%x: 1 entry id, 2 removal record, 4 record count)");
}

extern "C" int gm_view_detect(gm_ctx *c, gm_view_detect_rec *out) {
  if (!c || !out) return GM_EINVAL;
  TRY(view_detect_settled(c));
  const size_t n = (size_t)c->n;
  HIPCHECK(ctx_memcpy(c, out, c->vdet.rec, sizeof(gm_view_detect_rec) * n, hipMemcpyDeviceToHost));
  for (size_t i = 0; i < n; i++) out[i].fail_tick = c->failed_h[i] ? c->fail_t[i] : -1;
  return GM_OK;
}

extern "C" int gm_view_detect_timeline(gm_ctx *c, int32_t t, uint64_t *out) {
  if (!c || !out) return GM_EINVAL;
  if (!c->vdet.tmax) return GM_ESTATE;
  if (t <= 0 || t > c->vdet.tmax) return GM_EINVAL;
  TRY(view_detect_settled(c));
  HIPCHECK(ctx_memcpy(c, out, c->vdet.tl, sizeof(uint64_t) * GM_VIEW_DETECT_COLS * (size_t)t, hipMemcpyDeviceToHost));
  return GM_OK;
}
