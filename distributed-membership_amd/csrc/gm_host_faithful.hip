// gm_host_faithful.hip -- FAITHFUL host side: the state of gm_faithful.hip's kernels, the tick that
// enqueues them, and the mailbox that brings a tick's log records back in the reference's order.
#include "gm_host.h"

using namespace gmh;

// glibc srandom_r (TYPE_3) seeding of the S1 stream; the draws themselves are
// stepped on the device (gm_f_send) and by gm_rand.
static void s1_seed(uint32_t seed, int32_t st[33]) {
  if (seed == 0) seed = 1;
  int32_t word = (int32_t)seed;
  st[0] = word;
  for (int i = 1; i < 31; i++) {
    long hi = word / 127773, lo = word % 127773;
    word = (int32_t)(16807 * lo - 2836 * hi);
    if (word < 0) word += 2147483647;
    st[i] = word;
  }
  int f = 3, r = 0;
  for (int k = 0; k < 310; k++) {
    st[f] = (int32_t)((uint32_t)st[f] + (uint32_t)st[r]);
    f = (f + 1) % 31;
    r = (r + 1) % 31;
  }
  st[31] = f;
  st[32] = r;
}

// P_q = R^(q+1), q = 0..63, rows padded to 32 words: R is one 31-draw round of the S1
// register in fptr-rotated order, x[j] += x[(j + 28) % 31] for j ascending (gm_f_s1expand)
static std::vector<uint32_t> s1_round_powers() {
  // column i of P_q = the round applied q+1 times to basis vector e_i (31 adds per round)
  std::vector<uint32_t> P((size_t)64 * 31 * 32, 0u);
  for (int i = 0; i < 31; i++) {
    uint32_t x[31] = {0};
    x[i] = 1;
    for (int q = 0; q < 64; q++) {
      for (int j = 0; j < 31; j++) x[j] += x[(j + 28) % 31];
      for (int k = 0; k < 31; k++) P[((size_t)q * 31 + k) * 32 + i] = x[k];
    }
  }
  return P;
}

int gmh::create_faithful(gm_ctx *c) {
  const int n = c->n;
  if (n > F_MAX_NODES) return GM_EUNSUPPORTED;  // EmulNet.cpp:108 assert(src <= MAX_NODES)
  FState &f = c->f;
  f.n = n;
  f.np = (n + 63) / 64 * 64;
  f.tmax = F_MAX_TIME;
  f.gstride = n + GM_FANOUT;
  f.draw_cap = 5 * n * n + 2 * n + 1024;
  f.rd_seed = c->cfg.rd_seed;
  f.ev_cap = std::max(1 << 18, 4 * n * n + 64 * n);
  TRY(dalloc(c, &f.table, (size_t)n * f.np));
  TRY(dalloc(c, &f.start, n));
  TRY(dalloc(c, &f.failed, n));
  TRY(dalloc(c, &f.inited, n));
  TRY(dalloc(c, &f.ingroup, n));
  TRY(dalloc(c, &f.hbctr, n));
  TRY(dalloc(c, &f.started_now, n));
  TRY(dalloc(c, &f.buf, F_ENBUFFSIZE));
  TRY(dalloc(c, &f.bufsize, 1));
  TRY(dalloc(c, &f.holepos, 2 * F_ENBUFFSIZE));
  TRY(dalloc(c, &f.buf2, F_ENBUFFSIZE));
  TRY(dalloc(c, &f.bkey, F_ENBUFFSIZE));
  TRY(dalloc(c, &f.bkey2, F_ENBUFFSIZE));
  TRY(dalloc(c, &f.sidx, F_ENBUFFSIZE));
  TRY(dalloc(c, &f.rmeta, 2));
  TRY(dalloc(c, &f.q, F_ENBUFFSIZE));
  TRY(dalloc(c, &f.q_off, n));
  TRY(dalloc(c, &f.q_cnt, n));
  TRY(dalloc(c, &f.scount, n));
  TRY(dalloc(c, &f.jcnt, n));
  TRY(dalloc(c, &f.gcnt, n));
  TRY(dalloc(c, &f.fcnt, n));
  TRY(dalloc(c, &f.jrq, (size_t)n * n));
  TRY(dalloc(c, &f.gossip, (size_t)n * f.gstride));
  TRY(dalloc(c, &f.fcols, (size_t)n * n));
  TRY(dalloc(c, &f.s1, 33));
  TRY(dalloc(c, &f.draws, f.draw_cap));
  TRY(dalloc(c, &f.sbase, n));
  TRY(dalloc(c, &f.smeta, 3));
  TRY(dalloc(c, &f.spre, (size_t)f.draw_cap + 1));
  TRY(dalloc(c, &f.qidx, F_ENBUFFSIZE));
  TRY(dalloc(c, &f.s1mat, (size_t)64 * 31 * 32));
  TRY(dalloc(c, &f.s1vb, (size_t)(f.draw_cap / 1984 + 2) * 32));
  TRY(dalloc(c, &f.sent, (size_t)(n + 1) * f.tmax));  // rows 1..n: sent_msgs[id][time]
  TRY(dalloc(c, &f.recv, (size_t)(n + 1) * f.tmax));
  // one block = the tick's mailbox: event count, error flags, then the events, so that one
  // small copy per tick brings back all three (GM_F_MAILBOX events; more: a second copy)
  uint8_t *mb = nullptr;
  TRY(dalloc(c, &mb, 16 + sizeof(FEvent) * (size_t)f.ev_cap));
  f.ev_count = (unsigned long long *)mb;
  f.err = (uint32_t *)(mb + 8);
  f.ev = (FEvent *)(mb + 16);
  lap("faithful allocations");
  if (hipHostMalloc(&c->fh.mail, 16 + sizeof(FEvent) * GM_F_MAILBOX, hipHostMallocDefault) != hipSuccess) return GM_ENOMEM;
  lap("pinned mailbox");
  HIPCHECK(ctx_memset(c, f.table, 0xFF, sizeof(uint32_t) * (size_t)n * f.np));
  std::vector<int32_t> start(n);
  for (int i = 0; i < n; i++) start[i] = (int)(0.25 * i);  // (int)(STEP_RATE*i), Application.cpp:143
  HIPCHECK(ctx_memcpy(c, f.start, start.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice));
  for (int32_t *p : {f.failed, f.inited, f.ingroup, f.hbctr, f.started_now, f.q_off, f.q_cnt,
                     f.scount, f.jcnt, f.gcnt, f.fcnt})
    HIPCHECK(ctx_memset(c, p, 0, sizeof(int32_t) * (size_t)n));
  HIPCHECK(ctx_memset(c, f.sent, 0, sizeof(int32_t) * (size_t)(n + 1) * f.tmax));
  HIPCHECK(ctx_memset(c, f.recv, 0, sizeof(int32_t) * (size_t)(n + 1) * f.tmax));
  HIPCHECK(ctx_memset(c, f.bufsize, 0, sizeof(int32_t)));
  HIPCHECK(ctx_memset(c, f.ev_count, 0, sizeof(unsigned long long)));
  HIPCHECK(ctx_memset(c, f.err, 0, sizeof(uint32_t)));
  int32_t st[33];
  s1_seed(c->cfg.time_seed, st);  // srand(time(NULL)) at Application.cpp:50 and :96
  HIPCHECK(ctx_memcpy(c, f.s1, st, sizeof st, hipMemcpyHostToDevice));
  lap("faithful memsets");
  const std::vector<uint32_t> pm = s1_round_powers();
  HIPCHECK(ctx_memcpy(c, f.s1mat, pm.data(), sizeof(uint32_t) * pm.size(), hipMemcpyHostToDevice));
  lap("S1 powers");
  HIPCHECK(hipFuncSetAttribute((const void *)gm_f_recv, hipFuncAttributeMaxDynamicSharedMemorySize, F_RECV_LDS));
  lap("kernel attributes");
  const int nw = f.np / 64;
  c->fh.smem = (size_t)f.np * 8 + (size_t)nw * 8 * 3 + (size_t)nw * 4 + 624 * 4 + 48 * 4;
  return GM_OK;
}

void gmh::destroy_faithful(gm_ctx *c) {
  if (c->fh.mail) (void)hipHostFree(c->fh.mail);
}

static bool ev_order(const FEvent &a, const FEvent &b) {
  if (a.t != b.t) return a.t < b.t;
  if (a.logger != b.logger) return a.logger > b.logger;  // node phase: i descending
  return a.seq < b.seq;
}

// Records of a FAITHFUL tick can be at most n * (2n + 4): per node n joins, n removals and
// the start / join / time-mark lines.
static int64_t f_tick_event_bound(const gm_ctx *c) { return (int64_t)c->n * (2 * c->n + 4); }

// FAITHFUL detection recorder: N <= 1000, so the records are aggregated here on the host, where
// the tick's log lines are gathered. failed_h is the flag every collected tick ran with:
// gm_set_failed and nodeStart's reset (tick_faithful) collect the enqueued ticks before they change it.
static void detect_host(gm_ctx *c, int t, int kind, int subject) {
  if (t >= c->det.tmax || subject < 1 || subject > c->n) return;  // det.tmax 0: off
  gm_detect_rec &d = c->det.rec_h[subject - 1];
  uint64_t *row = c->det.tl_h.data() + 3 * (size_t)t;
  if (kind == GM_EV_JOINED) {
    d.joins++;
    row[0]++;
  } else if (kind == GM_EV_REMOVED) {
    const bool live = !c->failed_h[subject - 1];
    if (d.removals++ == 0) d.first_removed = t;
    d.last_removed = t;
    d.removed_tick_sum += (uint64_t)t;
    d.false_removals += live;
    row[1]++;
    row[2] += live;
  }
}

// Collect the mailbox of every tick enqueued since the last collection, in two halves so that a
// batch collects several members with one wait between them. f_collect_enqueue: one copy of the
// count, the error flags and the first GM_F_MAILBOX records on the context's stream (false:
// nothing enqueued since the last collection). After the stream was waited for, f_collect_parse
// stages the records to `pending` in the reference's order (more than GM_F_MAILBOX: a second copy)
// and resets the count in stream order.
int gmh::f_collect_enqueue(gm_ctx *c, bool *enqueued) {
  *enqueued = c->fh.inflight != 0;
  if (!*enqueued) return GM_OK;
  HIPCHECK(hipMemcpyAsync(c->fh.mail, c->f.ev_count, 16 + sizeof(FEvent) * GM_F_MAILBOX, hipMemcpyDeviceToHost,
                          c->stream));
  return GM_OK;
}

int gmh::f_collect_parse(gm_ctx *c) {
  c->fh.inflight = 0;
  const unsigned long long nev = *(const unsigned long long *)c->fh.mail;
  const uint32_t e = *(const uint32_t *)((const uint8_t *)c->fh.mail + 8);
  HIPCHECK(hipMemsetAsync(c->f.ev_count, 0, sizeof(unsigned long long), c->stream));
  if (nev > (unsigned long long)c->f.ev_cap) {
    c->latched = GM_ERANGE;
    return c->latched;
  }
  if (nev) {
    std::vector<FEvent> ev(nev);
    memcpy(ev.data(), (const uint8_t *)c->fh.mail + 16, sizeof(FEvent) * std::min<size_t>(nev, GM_F_MAILBOX));
    if (nev > GM_F_MAILBOX) {
      HIPCHECK(ctx_memcpy(c, ev.data() + GM_F_MAILBOX, c->f.ev + GM_F_MAILBOX, sizeof(FEvent) * (nev - GM_F_MAILBOX),
                         hipMemcpyDeviceToHost));
    }
    std::sort(ev.begin(), ev.end(), ev_order);
    for (const FEvent &e : ev) {
      c->pending.push_back(gm_event{e.t, e.logger, e.kind, e.subject});
      if (e.kind > 0 && e.kind < 6) c->ev_tot[e.kind]++;
      detect_host(c, e.t, e.kind, e.subject);
    }
  }
  latch_device_error(c, e);
  return c->latched;
}

int gmh::f_collect(gm_ctx *c) {
  bool enq = false;
  TRY(f_collect_enqueue(c, &enq));
  if (!enq) return c->latched;
  HIPCHECK(hipStreamSynchronize(c->stream));
  return f_collect_parse(c);
}

// The host part of one member's FAITHFUL tick, shared by gm_tick and gm_batch_tick, in two steps so
// that a batch can check every member before it changes any. f_tick_check: the time limit, and
// whether the mailbox must be collected before this tick is enqueued -- the record buffer could
// fill, or nodeStart resets a crash flag the recorder still reads.
int gmh::f_tick_check(const gm_ctx *c, bool *collect) {
  if (c->t >= F_MAX_TIME) return GM_ERANGE;  // EmulNet.cpp:109 assert(time < MAX_TIME)
  *collect = (c->fh.inflight + 1) * f_tick_event_bound(c) > c->f.ev_cap;
  if (c->det.tmax && c->nfailed)  // the recorder reads failed_h as the enqueued ticks saw it
    for (int i = 0; i < c->n; i++) *collect |= (int)(0.25 * i) == c->t && c->failed_h[i];
  return GM_OK;
}

// f_tick_begin (after the collection, if one was due): nodeStart of this tick's starters resets
// bFailed on the device (MP1Node.cpp:108-116), mirrored here; the tick is counted as enqueued.
// Returns the state the tick's kernels get up to gm_f_recvout, drop_pct_now filled in; the rest get
// it with buf / buf2 and bkey / bkey2 swapped (gm_f_recvout compacts the survivors into buf2),
// which is what c->f holds afterwards.
FState gmh::f_tick_begin(gm_ctx *c) {
  if (c->nfailed)
    for (int i = 0; i < c->n; i++)
      if ((int)(0.25 * i) == c->t && c->failed_h[i]) {
        c->failed_h[i] = 0;
        c->fail_t[i] = 0x7FFFFFFF;
        c->nfailed--;
      }
  FState st = c->f;
  st.drop_pct_now = c->dropmsg ? (int)(c->cfg.drop_prob * 100) : -1;  // EmulNet.cpp:92
  std::swap(c->f.buf, c->f.buf2);
  std::swap(c->f.bkey, c->f.bkey2);
  c->fh.inflight++;
  return st;
}

// FAITHFUL ticks are enqueued without a host wait: the records stay on the device until a
// call needs them (f_settle) or the next tick could overflow the record buffer.
int gmh::tick_faithful(gm_ctx *c) {
  bool collect = false;
  TRY(f_tick_check(c, &collect));
  if (collect) TRY(f_collect(c));
  FState st = f_tick_begin(c);
  hipLaunchKernelGGL(gm_f_recv, dim3(1), dim3(1024), F_RECV_LDS, c->stream, st, c->t);
  hipLaunchKernelGGL(gm_f_recvout, dim3(64), dim3(256), 0, c->stream, st, c->t);
  std::swap(st.buf, st.buf2);
  std::swap(st.bkey, st.bkey2);
  hipLaunchKernelGGL(gm_f_node, dim3(c->n), dim3(256), c->fh.smem, c->stream, st, c->t);
  hipLaunchKernelGGL(gm_f_sendprep, dim3(1), dim3(64), 0, c->stream, st);
  hipLaunchKernelGGL(gm_f_s1expand, dim3(f_s1expand_blocks(st)), dim3(256), 0, c->stream, st);
  hipLaunchKernelGGL(gm_f_sendscan, dim3(1), dim3(1024), 0, c->stream, st, c->t);
  hipLaunchKernelGGL(gm_f_sendemit, dim3(f_sendemit_blocks(st)), dim3(256), 0, c->stream, st);
  HIPCHECK(hipGetLastError());
  return c->latched;
}
