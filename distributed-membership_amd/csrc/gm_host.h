// gm_host.h -- internal to libgm's host units (gm_host*.hip): the context, the error plumbing and the
// functions that cross units. Nothing here is exported: the library's C symbols are include/gm_abi.h's.
//
//   gm_host.hip           create / destroy, gm_tick and the small calls, timing ring, error latching
//   gm_host_faithful.hip  FAITHFUL: state, tick, mailbox collection
//   gm_host_batch.hip     FAITHFUL: R contexts ticked together (gm_batch_*)
//   gm_host_scaled.hip    SCALED: state, the single-context tick
//   gm_host_shard.hip     SCALED column shards: RCCL attach, phase API, the sharded tick, loopback
//   gm_host_partial.hip   PARTIAL: state, tick, the row shards' exchange
//   gm_host_events.hip    event drains, detection recorder, msgcount
//   gm_host_view_detect.hip  PARTIAL detection recorder (gm_view_detect_*)
//   gm_host_read.hip      read-backs: rows, tables, views, nodes, targets, the censuses, view reachability
//   gm_host_view_reach.hip   view reachability across row shards: the group walk, gm_view_reach_loopback
//   gm_host_digest.hip    state digests: gm_digest, the per-tick recorder (gm_digest_record / _trace)
//   gm_host_stage.hip     the staged block of gm_read_rows and the loads: size, timing, stats
//   gm_host_load.hip      gm_load_*, gm_load_views_*: one block loop, one commit tail
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gm_abi.h"
#include "gm_device.h"
#include "gm_faithful.h"
#include "gm_partial.h"
#include "gm_scaled.h"

#define GM_T_LIMIT 32766  // packed 16-bit hb/ts stay exact: hb <= 2t+1 < 0xFFFF
#define GM_F_MAILBOX 4096  // FAITHFUL events copied back with the count and error flags
#define GM_D_FIRST S_MT_RAW  // S2 outputs per row in the first round (steady state needs ~5-6)
#define GM_D_MORE GM_D_MORE_ROUND  // S2 outputs per row in later rounds (transients with many stale entries)
#define GM_MAX_ROUNDS 4096    // draw rounds per sharded tick (16 + 64 * 4096 S2 outputs per row)
#define GM_D_LAST GM_D_LAST_ROUND  // bounded rounds: S2 outputs of round 2 (outputs [80, 336))
#define GM_SIG_WORDS 17      // gm_comm_init: config words every rank must agree on
#define GM_TEV_RING 64       // tick-kernel timing: event pairs in the ring (timing_slot)

// detection recorder (gm_detect_record; tmax 0 = off): per-subject records and the per-tick
// timeline [tmax][3]. SCALED keeps them on the device (gm_s_detect adds each tick's records),
// FAITHFUL on the host (f_collect)
struct gm_detect_state {
  int tmax = 0;
  gm_detect_rec *rec = nullptr;      // device [s.w]
  uint64_t *tl = nullptr;            // device [tmax][3]
  std::vector<gm_detect_rec> rec_h;  // FAITHFUL [n]
  std::vector<uint64_t> tl_h;        // FAITHFUL [tmax][3]
};

// SCALED census (gm_census): device scratch, allocated by the first call -- the records [s.w], the
// histogram, the kernels' status word
struct gm_census_scratch {
  uint8_t *blob = nullptr;
};

// PARTIAL view census (gm_view_census): device scratch, allocated on first use. blob: the per-subject
// accumulators [n] (16 bytes each), the two histograms, the kernels' status word and the crash bitmap of the
// cluster, rebuilt from failed_h when the crash set has changed; rec: the records [n], once a call asks for them
struct gm_view_census_scratch {
  uint8_t *blob = nullptr;
  gm_view_rec *rec = nullptr;
  int64_t nfailed = -1;              // gm_ctx.nfailed when the bitmap was last built (-1: never)
};

// PARTIAL view-graph reachability (gm_view_reach): device scratch, one block allocated on first use. blob: the
// per-node words seen, front, next [n] (8 bytes each), the counts [GM_VIEW_HOPS][GM_REACH_SOURCES], the
// sources [GM_REACH_SOURCES] and the kernels' status word
struct gm_view_reach_scratch {
  uint8_t *blob = nullptr;
};

// The walk across row shards (gm_view_reach with a communicator, gm_view_reach_loopback): a member's device
// scratch, one block allocated by the first sharded walk (gm_host_view_reach.hip carves it): the slices seen,
// front and next [nloc], the cluster-wide words wide [n], the receive area, the counts, the status word and
// the sources. agree: the device words of an RCCL rank's agreement before the first level
struct gm_view_reach_shard_scratch {
  uint8_t *blob = nullptr;
  uint64_t *agree = nullptr;
};

// PARTIAL detection recorder (gm_view_detect_record; tmax 0 = off), all on the device and allocated
// when recording starts: gm_p_view_detect adds each recorded tick's views and records
struct gm_view_detect_state {
  int tmax = 0;
  gm_view_detect_rec *rec = nullptr;  // [n]: this context's observers over all subjects of the cluster
  uint64_t *tl = nullptr;             // [tmax][GM_VIEW_DETECT_COLS]
  uint32_t *cls = nullptr;            // the crash bitmap of the cluster as the next tick will see it (bit id - 1)
  uint32_t *status = nullptr;         // the reducer's status word (GM_VD_E*)
};

// State digests (gm_digest, gm_digest_record): device scratch, allocated by the first call of either.
// blob: the word arrays rows, nodes [n] (PARTIAL: [nloc]), the two sums, the status word of gm_digest.
// The recorder (tmax 0 = off) keeps the trace and a status word of its own, and uses the word arrays as
// each recorded tick's scratch (stream-ordered with gm_digest's use of them).
struct gm_digest_state {
  uint8_t *blob = nullptr;
  int32_t *fail_t = nullptr;         // join ramp: device copy of gm_ctx.fail_t (gm_read_nodes' inGroup rule)
  int tmax = 0;
  uint64_t *trace = nullptr;         // [tmax][2]
  uint32_t *status = nullptr;        // the recorded ticks' status word
};

#define GM_STAGE_BYTES (256ull << 20)  // what a staged call's rows of one launch may take on the device

// What every staged call keeps (gm_read_rows, gm_load_*, gm_load_views_*): rows cross between the host
// and the state through one device block, cap rows per launch, each launch checked by the call's kernels
// through the status word at the block's end. The planes in front of it are the call's own, carved out
// where they are used (gm_host_load.hip, gm_host_read.hip). gm_host_stage.hip has the helpers.
struct gm_stage {
  void *blob = nullptr;              // the device block
  size_t bytes = 0;                  // its size as the stats report it (gm_read_rows: of the planes alone)
  int cap = 0;                       // rows per launch
  uint32_t *status = nullptr;        // the status word of the call's kernels (in the block)
  int64_t rows = 0;                  // rows done: since the begin (loads), since gm_create (gm_read_rows)
  double ms[2] = {0, 0};             // gm_set_timing on: ms in the call's two timed spans (stage_span)
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
};

// A state load, begin .. rows .. commit: c->ld (SCALED, gm_load_*), c->vl (PARTIAL, gm_load_views_*).
// The block is allocated by the begin and freed by the commit.
struct gm_load_stage : gm_stage {
  bool loading = false;              // between the begin and a successful commit
  bool voided = false;               // a load call failed: only the begin starts over
  bool xpending = false;             // PARTIAL row shards: committed, the exchange of tick t - 1 is replayed by the next tick
  int t = 0;                         // the begin's t
  std::vector<uint8_t> seen;         // this context's rows given so far
};

// FAITHFUL, host side of FState
struct gm_faithful_host {
  size_t smem = 0;                   // gm_f_node's dynamic LDS
  void *mail = nullptr;              // pinned host copy of the FAITHFUL tick mailbox
  int inflight = 0;                  // FAITHFUL ticks enqueued since the last mailbox collection
};

// PARTIAL, host side of PState
struct gm_partial_host {
  uint32_t *mtraw = nullptr;         // [2][nloc][16] S2 outputs by tick parity
  hipStream_t side = nullptr;        // S2 outputs of tick t+1, computed while tick t runs
  hipEvent_t tickev[2] = {nullptr, nullptr};  // by parity: the tick that read that S2 buffer is done
  hipEvent_t mtev[2] = {nullptr, nullptr};    // by parity: the prefetched S2 outputs are written
  int mt_next = -1;                  // the tick whose S2 outputs were prefetched
  int64_t recv_last = 0;             // lists received from other row shards in the last tick
  bool sharded = false;              // row-shard exchange each tick (G > 1, or one rank forced by GM_FORCE_SHARD=1)
  std::vector<double> xq;            // per row shard q: probability that a sender addresses q (xcap)
  uint64_t crash_hash = 0;           // hash of the whole crash set the block capacities were derived from
  bool crash_check = false;          // agree it across the ranks at the next RCCL tick
  uint64_t *crash_dev = nullptr;     // [4] device words of that check (the hash, the "exchange pending" flag)
};

// The chunk-pipelined exchange of a sharded tick, SCALED column shards and PARTIAL row shards alike:
// the exchange of chunk q runs on its own stream once q's kernels are done, while q+1.. still compute
struct gm_shard_exchange {
  hipStream_t stream = nullptr;      // RCCL exchange stream (overlaps the next chunk's kernels)
  std::vector<hipEvent_t> chunk_ev;  // per chunk: its kernels are done (compute stream)
  hipEvent_t done = nullptr;         // the tick's exchange and what follows it are done (exchange stream)
};

// R FAITHFUL contexts of one device ticked together (gm_batch_*, gm_host_batch.hip). While a context
// is a member its `stream` is the batch's, so every call on a member and every batch tick are
// ordered by construction. The device slots hold every member's FState as of the last upload;
// the kernels derive time and buffer order from the batch ticks since (FBSlot, gm_faithful.h), so
// a slot is uploaded again only when its member changed other than by the batch's own tick.
#define GM_BATCH_RING 4
struct gm_batch {
  std::vector<gm_ctx *> m;           // the members
  std::vector<hipStream_t> own;      // their own streams, given back by gm_batch_destroy
  hipStream_t stream = nullptr;
  FBSlot *slots = nullptr;           // device [R]
  std::vector<FBSlot> cur;           // what the device slots hold
  int step = 0;                      // batch ticks since the slots were uploaded (-1: never uploaded)
  FBSlot *ring[GM_BATCH_RING] = {nullptr, nullptr, nullptr, nullptr};  // pinned [R] each: the uploads' sources
  hipEvent_t ring_ev[GM_BATCH_RING] = {nullptr, nullptr, nullptr, nullptr};  // the upload from that buffer is done
  int uploads = 0;
  int gx_node = 0, gx_s1 = 0, gx_emit = 0;  // grid x of the kernels that size it from n: the largest member's
  size_t smem = 0;                   // gm_fb_node's dynamic LDS: the largest member's
  std::vector<int> due;              // scratch: members whose mailbox this tick collects
};

struct gm_ctx {
  gm_config cfg;
  hipStream_t stream = nullptr;
  gm_batch *batch = nullptr;         // FAITHFUL: the batch this context belongs to (stream is then the batch's)
  int dmax = 0;                      // status exchange depth (sharded)
  ncclComm_t comm = nullptr;         // RCCL communicator across column shards
  hipEvent_t k0 = nullptr, k1 = nullptr;  // per-tick band-kernel events (sharded)
  std::vector<hipEvent_t> tev;            // per-tick band-kernel event pairs (single context)
  double kernel_ms_sum = 0;
  int shard_sync = -1;               // sharded tick draw rounds: 1 host-driven unbounded loop, 0 bounded
  int diag_zero_row = -1;            // diagnostics (GM_DIAG_ZERO_ROW, tests): the pipelined column-shard tick
                                     //   clears this row's cells after its band kernels, so its records'
                                     //   counts disagree with the cells and a draw finds no holder
                                     // stream-ordered, -1 auto (env GM_SHARD_SYNC)
  int64_t nfailed = 0;               // nodes with failed_h set (gm_set_failed; nodeStart clears it)
  // sharded bounded draw rounds: rows they could not finish (npending) copied back without a
  // wait; the next call that needs the tick finishes them with host-driven rounds (draw_settle)
  int32_t *draw_left_h = nullptr;    // pinned [2]: rows left to the host-driven rounds, rows pending after round 0
  bool draw_rounds = false;          // the pipelined tick deferred bounded rounds 1, 2 to draw_settle
  hipEvent_t draw_ev = nullptr;
  bool draw_check = false;
  int t = 0;
  int n = 0;
  int dropmsg = 0;
  int latched = GM_OK;
  bool timing = false;
  int64_t ticks_done = 0;  // gm_tick calls that enqueued a tick
  int timed_ticks = 0;  // ticks in the current timing window
  int ktimed = 0;       // band-kernel event pairs recorded in the window (ring slots in use: min(ktimed, GM_TEV_RING))
  hipEvent_t e0 = nullptr, e1 = nullptr;
  // events: the device keeps one tick's records; with keep_events (default) a tick's records
  // are staged to `pending` before the next tick overwrites them (gm_keep_events)
  bool keep_events = true;
  bool undrained = false;      // the device holds the last tick's records, not yet staged
  uint64_t ev_tot[6] = {0, 0, 0, 0, 0, 0};  // FAITHFUL: cumulative records per kind
  std::vector<gm_event> pending;
  std::vector<void *> allocs;
  std::vector<int32_t> failed_h;
  std::vector<int32_t> fail_t;  // last tick a failed node ran (join ramp: its inGroup is frozen there)
  gm_detect_state det;
  FState f{};  // FAITHFUL
  gm_faithful_host fh;
  SState s{};  // SCALED
  gm_census_scratch cen;
  gm_load_stage ld;
  gm_stage rd;
  PState p{};  // PARTIAL
  gm_partial_host ph;
  gm_view_census_scratch vc;
  gm_view_reach_scratch vr;
  gm_view_reach_shard_scratch vrs;
  gm_view_detect_state vdet;
  gm_load_stage vl;
  gm_shard_exchange xch;  // SCALED column shards, PARTIAL row shards
  gm_digest_state dg;     // SCALED, PARTIAL
};

namespace gmh {
extern thread_local char g_errbuf[256];  // gm_strerror's detail (gm_host.hip)
}

#define HIPCHECK(x)                                                                   \
  do {                                                                                \
    hipError_t e_ = (x);                                                              \
    if (e_ != hipSuccess) {                                                           \
      snprintf(gmh::g_errbuf, sizeof gmh::g_errbuf, "%s:%d %s", __FILE__, __LINE__, hipGetErrorString(e_)); \
      return GM_EDEVICE;                                                              \
    }                                                                                 \
  } while (0)
#define NCCLCHECK(x)                                                                 \
  do {                                                                               \
    ncclResult_t r_ = (x);                                                           \
    if (r_ != ncclSuccess) {                                                         \
      snprintf(gmh::g_errbuf, sizeof gmh::g_errbuf, "%s:%d RCCL %s", __FILE__, __LINE__, ncclGetErrorString(r_)); \
      return GM_ECOMM;                                                               \
    }                                                                                \
  } while (0)
#define TRY(x)              \
  do {                      \
    int r_ = (x);           \
    if (r_ != GM_OK) return r_; \
  } while (0)

// Every copy and fill of a context goes through its own stream. That stream is non-blocking, so the
// legacy null stream that hipMemcpy / hipMemset use neither waits for its kernels nor is waited for by
// them: a fill at creation could still be running when the init kernel writes (seen as an own entry
// missing from an S-C view after a 8.6 GB fill of the lists), and a host-to-device copy may return
// before its DMA lands. Fills are enqueued in order; copies wait for the stream (the host buffers are
// the caller's).
static inline hipError_t ctx_memset(gm_ctx *c, void *p, int v, size_t n) { return hipMemsetAsync(p, v, n, c->stream); }
static inline hipError_t ctx_memcpy(gm_ctx *c, void *d, const void *src, size_t n, hipMemcpyKind k) {
  const hipError_t e = hipMemcpyAsync(d, src, n, k, c->stream);
  return e == hipSuccess ? hipStreamSynchronize(c->stream) : e;
}
static inline hipError_t ctx_memcpy2d(gm_ctx *c, void *d, size_t dpitch, const void *src, size_t spitch, size_t width,
                                      size_t height, hipMemcpyKind k) {
  const hipError_t e = hipMemcpy2DAsync(d, dpitch, src, spitch, width, height, k, c->stream);
  return e == hipSuccess ? hipStreamSynchronize(c->stream) : e;
}

// PARTIAL: the crash set of the whole cluster as one bit per node (bit i of word i / 32: node i, id i + 1),
// what the view census and the detection recorder test a subject against
static inline std::vector<uint32_t> crash_bitmap(const gm_ctx *c) {
  std::vector<uint32_t> cls(((size_t)c->n + 31) / 32, 0u);
  if (c->nfailed)
    for (size_t i = 0; i < (size_t)c->n; i++)
      if (c->failed_h[i]) cls[i >> 5] |= 1u << (i & 31);
  return cls;
}

template <class T>
static int dalloc(gm_ctx *c, T **p, size_t count) {
  void *q = nullptr;
  size_t bytes = sizeof(T) * (count ? count : 1);
  if (hipMalloc(&q, bytes) != hipSuccess) {
    snprintf(gmh::g_errbuf, sizeof gmh::g_errbuf, "hipMalloc(%zu) failed", bytes);
    return GM_ENOMEM;
  }
  c->allocs.push_back(q);
  *p = (T *)q;
  return GM_OK;
}

// What one host unit defines and another calls.
namespace gmh {

// gm_host.hip
void lap(const char *what);  // diagnostics (GM_CREATE_TIMING): where context creation time goes
int inbox_cap(int cap);
int exchange_create(gm_ctx *c, int chunks);
void latch_device_error(gm_ctx *c, uint32_t flags);
int check_err(gm_ctx *c);
int f_settle(gm_ctx *c);
int settled_read(gm_ctx *c);
int kernel_status(gm_ctx *c, const uint32_t *d_status, int code, const char *fmt, uint32_t *flags = nullptr);
int timing_slot(gm_ctx *c, hipEvent_t *k0, hipEvent_t *k1, hipStream_t st);
void advance(gm_ctx *c);

static inline bool drop_tick(const gm_ctx *c, int t) {  // keyed loss applies to the lists sent at t - 1
  return c->cfg.drop_pct > 0 && t - 1 >= c->cfg.drop_from && t - 1 < c->cfg.drop_to;
}
static inline bool mc_on(const gm_ctx *c, int t) { return c->s.mc_sent && t < c->s.mc_tmax; }

// the chunk-major exchange buffer of a column shard (SState.xcnt, S_XC)
static inline size_t xcnt_bytes(const SState &s) {
  return sizeof(int32_t) * 2 * (size_t)s.xk * s.shard_count * ((size_t)1 << s.xlog);
}
static inline int xchunk_rows(const SState &s, int ch) {  // real rows of exchange chunk ch
  return (int)std::min<int64_t>((int64_t)1 << s.xlog, (int64_t)s.n - ((int64_t)ch << s.xlog));
}

// gm_host_faithful.hip
int create_faithful(gm_ctx *c);
void destroy_faithful(gm_ctx *c);
int f_collect(gm_ctx *c);
int f_collect_enqueue(gm_ctx *c, bool *enqueued);
int f_collect_parse(gm_ctx *c);
int f_tick_check(const gm_ctx *c, bool *collect);
FState f_tick_begin(gm_ctx *c);
int tick_faithful(gm_ctx *c);
// grid x of the two FAITHFUL kernels sized from the draw capacity (grid-stride: any size computes the same)
static inline int f_s1expand_blocks(const FState &f) { return std::min(1024, (f.draw_cap / 31 + 1 + 7) / 8); }
static inline int f_sendemit_blocks(const FState &f) { return std::min(1024, (f.draw_cap + 255) / 256); }

// gm_host_scaled.hip
int create_scaled(gm_ctx *c);
void destroy_scaled(gm_ctx *c);
int tick_scaled(gm_ctx *c);
int ramp_starters(gm_ctx *c, hipStream_t st);
int detect_tick(gm_ctx *c, int t, hipStream_t st);

// A sharded tick is written once, over a GROUP of local ranks (gm_ctx **g, count G): gm_tick passes
// {c} (its peers are RCCL ranks, or none under gm_shard_stub), the loopback entry points the G
// contexts of one cluster living on one device. A tick is a sequence of steps "every member
// enqueues this launch" separated by group collectives (grp_*, px_*), the only code that differs by
// group kind. Streams and events are the first member's; buffers and host bookkeeping each member's.
// gm_host_shard.hip
int tick_sharded(gm_ctx **g, int G);
int draw_settle(gm_ctx **g, int G);

// gm_host_partial.hip
int create_partial(gm_ctx *c);
void destroy_partial(gm_ctx *c);
int tick_partial(gm_ctx **g, int G);
int partial_caps(gm_ctx *c);

// gm_host_events.hip
int before_tick_events(gm_ctx *c);

// gm_host_view_detect.hip
int view_detect_flags(gm_ctx *c);
int view_detect_tick(gm_ctx *c, int t, hipStream_t st);

// gm_host_view_reach.hip
int view_reach_args(int n, const int32_t *sources, int nsrc, int dir, int max_hops, const uint64_t *counts,
                    const int64_t *info);
int view_reach_group(gm_ctx **g, int G, const int32_t *sources, int nsrc, int dir, int max_hops, uint64_t *counts,
                     uint64_t *seen, int64_t info[4]);

// gm_host_digest.hip
int digest_flags(gm_ctx *c);
int digest_tick(gm_ctx *c, int t, hipStream_t st);

// gm_host_stage.hip
int stage_cap(size_t budget, size_t row_bytes, size_t rows, const char *env);
int stage_alloc(gm_stage &st, int cap, size_t bytes, size_t status_off, const char *what);
void stage_free(gm_stage &st);
void stage_destroy(gm_stage &st, bool owned);
int stage_mark(gm_ctx *c, gm_stage &st, int k);
int stage_span(gm_ctx *c, gm_stage &st, int slot, int from, int to);
int stage_stats(const gm_ctx *c, int mode, const gm_stage *st, double stats[4]);

}  // namespace gmh
