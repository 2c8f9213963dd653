// gm_host_batch.hip -- FAITHFUL: R independent clusters ticked together. A batch tick is the seven
// launches of tick_faithful with the member as the grid's y dimension (gm_fb_*, gm_faithful.hip);
// everything else a member does stays the per-context call it was. The members share the batch's
// stream from gm_batch_create to gm_batch_destroy, which orders their calls and the batch ticks
// without an event or a wait per member.
#include "gm_host.h"

using namespace gmh;

static void batch_free(gm_batch *b) {
  for (int r = 0; r < GM_BATCH_RING; r++) {
    if (b->ring_ev[r]) (void)hipEventDestroy(b->ring_ev[r]);
    if (b->ring[r]) (void)hipHostFree(b->ring[r]);
  }
  if (b->slots) (void)hipFree(b->slots);
  if (b->stream) (void)hipStreamDestroy(b->stream);
  delete b;
}

extern "C" int gm_batch_create(gm_ctx **ctxs, int32_t R, gm_batch **out) {
  if (!ctxs || !out || R < 1 || R > 65535) return GM_EINVAL;  // R is the grid's y dimension
  *out = nullptr;
  for (int i = 0; i < R; i++)
    if (!ctxs[i]) return GM_EINVAL;
  for (int i = 0; i < R; i++)
    if (ctxs[i]->cfg.mode != GM_MODE_FAITHFUL) return GM_EUNSUPPORTED;
  std::vector<gm_ctx *> sorted(ctxs, ctxs + R);
  std::sort(sorted.begin(), sorted.end());
  if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) return GM_EINVAL;  // the same context twice
  for (int i = 0; i < R; i++)
    if (ctxs[i]->batch) return GM_ESTATE;
  for (int i = 0; i < R; i++)
    if (ctxs[i]->cfg.device != ctxs[0]->cfg.device) return GM_EINVAL;
  g_errbuf[0] = 0;
  gm_batch *b = new gm_batch();
  const size_t bytes = sizeof(FBSlot) * (size_t)R;
  bool ok = hipSetDevice(ctxs[0]->cfg.device) == hipSuccess &&
            hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking) == hipSuccess &&
            hipMalloc((void **)&b->slots, bytes) == hipSuccess;
  for (int r = 0; ok && r < GM_BATCH_RING; r++)
    ok = hipHostMalloc((void **)&b->ring[r], bytes, hipHostMallocDefault) == hipSuccess &&
         hipEventCreateWithFlags(&b->ring_ev[r], hipEventDisableTiming) == hipSuccess;
  ok = ok && hipFuncSetAttribute((const void *)gm_fb_recv, hipFuncAttributeMaxDynamicSharedMemorySize, F_RECV_LDS) ==
                 hipSuccess;
  // what a member enqueued on its own stream is done before the batch's stream takes over
  for (int i = 0; ok && i < R; i++) ok = hipStreamSynchronize(ctxs[i]->stream) == hipSuccess;
  if (!ok) {
    snprintf(g_errbuf, sizeof g_errbuf, "gm_batch_create: HIP resources for %d members unavailable", R);
    batch_free(b);
    return GM_EDEVICE;
  }
  b->m.assign(ctxs, ctxs + R);
  b->own.resize(R);
  b->cur.resize(R);
  b->step = -1;
  for (int i = 0; i < R; i++) {
    gm_ctx *c = ctxs[i];
    b->own[i] = c->stream;
    c->stream = b->stream;
    c->batch = b;
    b->gx_node = std::max(b->gx_node, c->n);
    b->gx_s1 = std::max(b->gx_s1, f_s1expand_blocks(c->f));
    b->gx_emit = std::max(b->gx_emit, f_sendemit_blocks(c->f));
    b->smem = std::max(b->smem, c->fh.smem);
  }
  *out = b;
  return GM_OK;
}

// Every member's slot from its context, as the tick about to be launched starts (f_tick_begin has
// swapped c->f's buffers already: the slot gets the order before that), through the next pinned buffer
// of the ring; a buffer is reused once the copy out of it is done.
static int upload_slots(gm_batch *b) {
  const int R = (int)b->m.size();
  for (int i = 0; i < R; i++) {
    const gm_ctx *c = b->m[i];
    FBSlot &s = b->cur[i];
    s.f = c->f;
    std::swap(s.f.buf, s.f.buf2);
    std::swap(s.f.bkey, s.f.bkey2);
    s.f.drop_pct_now = c->dropmsg ? (int)(c->cfg.drop_prob * 100) : -1;
    s.t = c->t;
    s.pad = 0;
  }
  const int r = b->uploads % GM_BATCH_RING;
  if (b->uploads >= GM_BATCH_RING) HIPCHECK(hipEventSynchronize(b->ring_ev[r]));
  memcpy(b->ring[r], b->cur.data(), sizeof(FBSlot) * (size_t)R);
  HIPCHECK(hipMemcpyAsync(b->slots, b->ring[r], sizeof(FBSlot) * (size_t)R, hipMemcpyHostToDevice, b->stream));
  HIPCHECK(hipEventRecord(b->ring_ev[r], b->stream));
  b->uploads++;
  b->step = 0;
  return GM_OK;
}

extern "C" int gm_batch_tick(gm_batch *b) {
  if (!b) return GM_EINVAL;
  const int R = (int)b->m.size();
  // all or nothing: every member is checked, and the due mailboxes collected, before any member changes
  for (gm_ctx *c : b->m)
    if (c->latched != GM_OK) return c->latched;
  b->due.clear();
  for (int i = 0; i < R; i++) {
    bool collect = false;
    TRY(f_tick_check(b->m[i], &collect));
    if (collect) b->due.push_back(i);
  }
  if (!b->due.empty()) {  // every due member's mailbox copy, one wait, then the records
    bool enq = false;
    for (int i : b->due) TRY(f_collect_enqueue(b->m[i], &enq));
    HIPCHECK(hipStreamSynchronize(b->stream));
    int failed = GM_OK;  // a runtime error of a collection that latched nothing
    for (int i : b->due)
      if (b->m[i]->fh.inflight) {
        const int rc = f_collect_parse(b->m[i]);
        if (failed == GM_OK) failed = rc;
      }
    for (gm_ctx *c : b->m)
      if (c->latched != GM_OK) return c->latched;
    if (failed != GM_OK) return failed;
  }
  // the members' host parts; a slot still holds its member if the member moved by batch ticks alone
  bool same = b->step >= 0;
  const bool odd = b->step & 1;
  for (int i = 0; i < R; i++) {
    gm_ctx *c = b->m[i];
    const FBSlot &s = b->cur[i];
    const FState st = f_tick_begin(c);
    same = same && c->t == s.t + b->step && st.drop_pct_now == s.f.drop_pct_now &&
           st.buf == (odd ? s.f.buf2 : s.f.buf) && st.bkey == (odd ? s.f.bkey2 : s.f.bkey);
  }
  if (!same) TRY(upload_slots(b));
  const FBSlot *sl = b->slots;
  const int step = b->step;
  hipLaunchKernelGGL(gm_fb_recv, dim3(1, R), dim3(1024), F_RECV_LDS, b->stream, sl, step);
  hipLaunchKernelGGL(gm_fb_recvout, dim3(64, R), dim3(256), 0, b->stream, sl, step);
  hipLaunchKernelGGL(gm_fb_node, dim3(b->gx_node, R), dim3(256), b->smem, b->stream, sl, step);
  hipLaunchKernelGGL(gm_fb_sendprep, dim3(1, R), dim3(64), 0, b->stream, sl, step);
  hipLaunchKernelGGL(gm_fb_s1expand, dim3(b->gx_s1, R), dim3(256), 0, b->stream, sl, step);
  hipLaunchKernelGGL(gm_fb_sendscan, dim3(1, R), dim3(1024), 0, b->stream, sl, step);
  hipLaunchKernelGGL(gm_fb_sendemit, dim3(b->gx_emit, R), dim3(256), 0, b->stream, sl, step);
  HIPCHECK(hipGetLastError());
  b->step++;
  for (gm_ctx *c : b->m) advance(c);
  return GM_OK;
}

extern "C" int gm_batch_destroy(gm_batch *b) {
  if (!b) return GM_EINVAL;
  (void)hipStreamSynchronize(b->stream);  // the members' enqueued ticks and copies end on the batch's stream
  for (size_t i = 0; i < b->m.size(); i++) {
    b->m[i]->stream = b->own[i];
    b->m[i]->batch = nullptr;
  }
  batch_free(b);
  return GM_OK;
}
