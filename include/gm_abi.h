/* gm_abi.h -- C ABI of the MI355X-native gossip-membership simulator (libgm.so).
 *
 * The drop-in boundary. The reference's own plugin seam is the
 * Application <-> MP1Node <-> EmulNet API: the driver calls, per node and per
 * globaltime tick, MP1Node::recvLoop (-> EmulNet::ENrecv) and MP1Node::nodeStart /
 * nodeLoop (-> checkMessages, nodeLoopOps, sendMemberList -> EmulNet::ENsend),
 * then Application::fail pokes Member::bFailed / Params::dropmsg and draws from
 * rand(). Here the whole per-tick body of Application::mp1Run for ALL nodes is
 * one call, gm_tick(); fault injection keeps its host-side driver (gm_rand,
 * gm_set_failed, gm_set_dropmsg); dbg.log / msgcount.log content comes back as
 * plain records. Plain C types only; no HIP or torch types cross the boundary.
 *
 * Reference interface each entry point replaces (file:line in the reference):
 *   gm_create       Application::Application + EmulNet::EmulNet + ENinit + new MP1Node
 *                   (Application.cpp:47-70, EmulNet.cpp:12-27,72-77, MP1Node.cpp:25-34),
 *                   Params::setparams values in gm_config (Params.cpp:19-40)
 *   gm_tick         Application::mp1Run (Application.cpp:121-164): recvLoop/ENrecv for
 *                   i ascending, then nodeStart/nodeLoop (checkMessages, updatelistCallBack,
 *                   joinreqCallBack, nodeLoopOps, sendMemberList, ENsend) for i descending
 *                   (MP1Node.cpp:47-54,73-163,182-495; EmulNet.cpp:87-177)
 *   gm_rand         rand() in Application::fail (Application.cpp:182,189) -- the SAME S1
 *                   stream ENsend draws from (EmulNet.cpp:90)
 *   gm_set_failed   mp1[i]->getMemberNode()->bFailed = true (Application.cpp:186,194)
 *   gm_set_dropmsg  par->dropmsg = 0/1 (Application.cpp:178,199)
 *   gm_drain_events Log::LOG / logNodeAdd / logNodeRemove call sites inside the tick
 *                   (Log.cpp:44-131; MP1Node.cpp:135,153,295,437; Application.cpp:158)
 *   gm_detect       Log::logNodeAdd / logNodeRemove (Log.cpp:116-131) as the grader reads their
 *                   lines: who was removed, by how many observers, when, and who by mistake
 *   gm_msgcount     EmulNet::sent_msgs / recv_msgs as dumped by ENcleanup (EmulNet.cpp:184-220)
 *   gm_dump_tables  Member::memberList of every node (Member.h:89-122), for parity tests
 *   gm_digest, gm_digest_record, gm_digest_trace
 *                   Member::memberList of every node (Member.h:89-122) with Member's flags and
 *                   heartbeat and the gossipnodes of nodeLoopOps (MP1Node.cpp:449-489): the content
 *                   gm_dump_tables renders, hashed where it lives
 *   gm_destroy      Application::~Application / ENcleanup storage release
 *   gm_batch_tick   R independent Application processes, each at its own globaltime, advanced by
 *                   one mp1Run each (the grader's three testcases, a seed ensemble)
 *
 * Conventions: every function returns GM_OK (0) or a negative GM_E* code and never
 * throws; the context owns all device memory; output buffers are caller-owned;
 * one host thread per context. (a batch and its members: one thread for all of them). gm_tick enqueues the tick on the context's HIP
 * stream and returns (a tick is a BSP round: sends of tick t are consumed in
 * tick t+1); every read-back function and gm_sync wait for enqueued ticks.
 */
#ifndef GM_ABI_H
#define GM_ABI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GM_ABI_VERSION 2

enum gm_status {
  GM_OK = 0,
  GM_EINVAL = -1,     /* bad argument / config */
  GM_ENOMEM = -2,     /* device or host allocation failed */
  GM_EDEVICE = -3,    /* HIP runtime error */
  GM_ERANGE = -4,     /* a bounded resource overflowed (inbox, event ring, draw table) */
  GM_ESTATE = -5,     /* protocol invariant the fast path relies on was violated */
  GM_EUNSUPPORTED = -6,
  GM_ECOMM = -7       /* collective (RCCL) failure */
};

enum gm_mode {
  GM_MODE_FAITHFUL = 0, /* the reference: EmulNet cap 30000, per-entry messages, S1 drops */
  GM_MODE_SCALED = 1,   /* build-defined large-N regime: converged start, keyed drops */
  GM_MODE_PARTIAL = 2   /* build-defined V-entry membership views (scenario S-C; oracle/ref_cpu.c PARTIAL) */
};

enum gm_event_kind {
  GM_EV_JOINED = 1,        /* "Node a.b.c.d:p joined at time t"   (Log.cpp:116-120) */
  GM_EV_REMOVED = 2,       /* "Node a.b.c.d:p removed at time t"  (Log.cpp:127-131) */
  GM_EV_START_GROUP = 3,   /* "Starting up group..."              (MP1Node.cpp:135) */
  GM_EV_TRY_JOIN = 4,      /* "Trying to join..."                 (MP1Node.cpp:152-153) */
  GM_EV_TIME_MARK = 5      /* "@@time=t"                          (Application.cpp:156-160) */
};

typedef struct gm_config {
  int32_t abi_version;     /* = GM_ABI_VERSION */
  int32_t mode;            /* enum gm_mode */
  int32_t n;               /* EN_GPSZ (= MAX_NNB) */
  int32_t single_failure;  /* SINGLE_FAILURE (host-side fail() uses it; kept for completeness) */
  int32_t drop_msg;        /* DROP_MSG */
  double drop_prob;        /* MSG_DROP_PROB (FAITHFUL: drop iff rand()%100 < (int)(p*100)) */
  uint32_t time_seed;      /* S1: srand(TIME_SEED) */
  uint64_t rd_seed;        /* S2: per-(tick, id) mt19937 seed contract */
  /* SCALED only */
  int32_t drop_pct;        /* per-entry drop percentage */
  int32_t drop_from;       /* drops apply to sends at ticks in [drop_from, drop_to) */
  int32_t drop_to;
  uint64_t drop_seed;
  /* placement */
  int32_t device;          /* HIP device ordinal */
  int32_t shard_rank;      /* shard of this context: SCALED column shard / PARTIAL row shard; 0 */
  int32_t shard_count;     /* number of shards (GPUs); 1 */
  /* SCALED initial state: 0 = cold converged start (every cell {hb 0, ts 0},
   * first tick 1); 1 = warm converged start at t0: own entry {2*t0-1, t0},
   * others {2*(t0-1-a)-1, t0-a} with a = splitmix64(init_seed, r, c) % 4,
   * heartbeat counters 2*t0, first tick t0+1 (no mass-staleness transient);
   * 2 = join ramp (one context, no drops): node i starts at tick (int)(0.25*i)
   * (Application.cpp:130), JOINREQ -> introducer -> JOINREP + newNodes-first gossip
   * (MP1Node.cpp:126-163,226-251) over the unbounded network; state as of tick 0
   * (the introducer's own entry), first tick 1 */
  int32_t init_mode;
  int32_t init_t0;
  uint64_t init_seed;
  int32_t band;            /* SCALED columns per band of the tick kernel (64/128/256/512/1024; 0 = auto:
                              1024, the band fast path, whenever the row width allows it) */
  int32_t view;            /* PARTIAL view capacity V (2..32; 0 = 32) */
  uint64_t view_seed;      /* PARTIAL initial views and eviction tie-break */
  int32_t device_share;    /* SCALED: contexts of this cluster that share this context's device and
                              split its free HBM for the escape pools / event ring (0 = shard_count:
                              every shard on one device, as the loopback tests run them; 1 = a device
                              of its own, one RCCL rank per GPU) */
  int32_t reserved;
} gm_config;

/* one log record; gm_drain_events returns them already in reference log order (Log.cpp lines of a
 * tick: loggers descending, joins in dequeue / ascending id order, removals descending id) */
typedef struct gm_event {
  int32_t t;
  int32_t logger;          /* node index (id = logger + 1) whose LOG call it is */
  int32_t kind;            /* enum gm_event_kind */
  int32_t subject;         /* node id joined/removed; 0 otherwise */
} gm_event;

typedef struct gm_ctx gm_ctx;

/* Params::setparams equivalent: parse a reference testcase .conf
 * ("MAX_NNB: %d\nSINGLE_FAILURE: %d\nDROP_MSG: %d\nMSG_DROP_PROB: %lf"). */
int gm_parse_conf(const char *path, gm_config *cfg);

int gm_create(const gm_config *cfg, gm_ctx **out);
int gm_destroy(gm_ctx *ctx);

/* Enqueue one Application::mp1Run tick at the context's current globaltime,
 * then advance globaltime. Returns a latched device error from an earlier tick.
 * FAITHFUL ticks do not wait on the host either: their records and error flags
 * are collected by the next call that reads state (gm_drain_events, gm_sync,
 * gm_rand, gm_set_failed, gm_msgcount, gm_read_*, gm_event_*), or by gm_tick
 * itself once the device record buffer could fill; an error raised by tick t is
 * reported by that call. */
int gm_tick(gm_ctx *ctx);
int gm_sync(gm_ctx *ctx);
int gm_time(gm_ctx *ctx, int32_t *t);

/* Application::fail hooks (called between ticks, host order preserved) */
int gm_rand(gm_ctx *ctx, int32_t *out);
/* gm_set_failed: sharded contexts (column or row shards of one cluster) must all be given the
 * SAME crash set, as every rank of the reference run sees one Application::fail. Row shards derive
 * their exchange block sizes from it; they all-reduce a hash of the set at the next tick and return
 * GM_ESTATE when a rank disagrees. */
int gm_set_failed(gm_ctx *ctx, const int32_t *idx, int32_t n);
int gm_set_dropmsg(gm_ctx *ctx, int32_t on);

/* Drain every event produced since the last drain, in reference log order
 * (ticks ascending; node phase i descending; per node: start line or joins in
 * dequeue order, then removals by descending id, then @@time). If cap is too
 * small, *n receives the number pending and GM_ERANGE is returned (nothing drained).
 * SCALED / PARTIAL keep one tick's records on the device; with event keeping on
 * (the default) gm_tick first stages the previous tick's undrained records to host
 * memory (a readback per tick), so nothing is lost between drains. */
int gm_drain_events(gm_ctx *ctx, gm_event *out, size_t cap, size_t *n);
/* on = 1 (default): keep every tick's records until drained. on = 0 (benchmarks):
 * a tick overwrites the previous tick's undrained records (no per-tick readback);
 * gm_drain_events then returns the last tick's records only.
 * Limits: with on = 1 the host stages at most 2^27 records between drains (GM_ERANGE
 * beyond: a TREMOVE tick of S-B's 1 % crash removes ~687 M entries, of S-A's ~22 M);
 * clusters that large run with on = 0 and read the device totals (gm_event_totals) or the
 * per-subject detection records (gm_detect_record). The
 * device keeps E = band/32 records per (row, band) plus a spill ring sized from free HBM
 * (>= 2^24 records; GM_ERR_EVENTS -> GM_ERANGE past it). */
int gm_keep_events(gm_ctx *ctx, int32_t on);
/* counts[0] = records produced in the last tick (SCALED / PARTIAL telemetry; PARTIAL
 * also splits them per kind in counts[kind]; FAITHFUL: records pending per kind) */
int gm_event_counts(gm_ctx *ctx, uint64_t counts[6]);
/* totals[k] = records of kind k produced since gm_create, totals[0] = their sum,
 * independent of draining (FAITHFUL, SCALED; SCALED counts on the device, per (row,
 * band) cell). PARTIAL: GM_EUNSUPPORTED (views churn ~V joins per node and tick). */
int gm_event_totals(gm_ctx *ctx, uint64_t totals[6]);

/* sent/recv message counts per node id 1..n for ticks [0, t): out arrays [n][t].
 * FAITHFUL: EmulNet's sent_msgs / recv_msgs (EmulNet.cpp:111,172), always recorded.
 * SCALED / PARTIAL: the same per-entry-message counts in the list-gossip regime, recorded
 * once gm_msgcount_record was called (GM_ESTATE otherwise): sent = entries a node put on
 * the wire (its fresh entries x its targets, before loss: the loss is decided in flight),
 * recv = entries of the lists delivered to it that survived the loss (PARTIAL: of every
 * delivered list; all are merged). Gossip LIST entries only (the ramp's JOINREQ / JOINREP are not counted).
 * A PARTIAL row shard reports its own nodes ([nloc][t]). */
int gm_msgcount(gm_ctx *ctx, int32_t t, int32_t *sent, int32_t *recv);
/* SCALED / PARTIAL: start recording the per-node counts of gm_msgcount for ticks < tmax
 * (device history of 8 * tmax bytes per node). Only before the first tick (GM_ESTATE
 * after); FAITHFUL: no-op. SCALED column shards count their own columns' fresh entries and
 * SUM-allreduce them (N x 4 B per tick, only while recording), so every rank returns the
 * whole cluster's counts, equal to the single-context ones. */
int gm_msgcount_record(gm_ctx *ctx, int32_t tmax);

/* ---- failure-detection statistics (FAITHFUL, SCALED). The reference's grader reads completeness
 * and accuracy out of dbg.log's "joined" / "removed" lines (Log::logNodeAdd / logNodeRemove,
 * Log.cpp:116-131, called from MP1Node.cpp:295,437). The recorder keeps what the grader derives
 * from them, per subject node and per tick, without draining: SCALED reduces each tick's records
 * on the device before the next tick overwrites them (independent of gm_keep_events), FAITHFUL
 * aggregates where it collects its records. */
typedef struct gm_detect_rec {      /* 32 bytes, one per subject node */
  int32_t  fail_tick;        /* the tick after which gm_set_failed marked the node; -1 = never failed */
  int32_t  first_removed;    /* tick of the first REMOVED record naming this subject; -1 = none */
  int32_t  last_removed;     /* tick of the last one; -1 = none */
  uint32_t removals;         /* REMOVED records naming this subject */
  uint32_t false_removals;   /* those logged in a tick during which the subject's bFailed was 0 */
  uint32_t joins;            /* JOINED records naming this subject */
  uint64_t removed_tick_sum; /* sum of the ticks of its removals
                                (mean latency = sum / removals - fail_tick) */
} gm_detect_rec;
/* Start recording from the next tick, for ticks < tmax (0 < tmax <= 32767, else GM_EINVAL); a tick
 * >= tmax is not recorded at all. May be called between any two ticks; a second call returns
 * GM_ESTATE. PARTIAL: GM_EUNSUPPORTED (views churn ~V joins per node and tick, and a removal there
 * is an eviction; gm_view_detect_record is that mode's recorder). While recording is off no kernel is
 * added to a tick. */
int gm_detect_record(gm_ctx *ctx, int32_t tmax);
/* One record per subject this context owns: out[n], or out[w] for a SCALED column shard over the
 * columns [c0, c0 + w) of gm_shard_layout. GM_ESTATE before gm_detect_record. */
int gm_detect(gm_ctx *ctx, gm_detect_rec *out);
/* out[t][3] = joins, removals, false removals recorded in tick i, for i < t <= tmax (ticks before
 * recording began: 0). A column shard reports its own columns. */
int gm_detect_timeline(gm_ctx *ctx, int32_t t, uint64_t *out);

/* Dense readback of observer row r: hb/ts per subject column (absent -> -1),
 * columns [c0, c0+len) of this context's shard (c0 relative to the shard start). */
int gm_read_row(gm_ctx *ctx, int32_t r, int32_t c0, int32_t len, int32_t *hb, int32_t *ts);
/* Dense readback of observer rows [r0, r0+count): hb/ts [count][w] over this context's
 * w columns (absent -> -1); one bulk copy of the table, for parity tests at larger N. SCALED: the
 * whole stored state is copied and decoded on the host whatever count is -- at large N read through
 * gm_read_rows, which returns the same arrays decoded on the device. */
int gm_read_table(gm_ctx *ctx, int32_t r0, int32_t count, int32_t *hb, int32_t *ts);
/* SCALED: rows [r0, r0 + count) as gm_read_table returns them -- hb / ts [count][w] over this
 * context's w columns, -1 = absent -- decoded on the device; only the rows asked for are copied.
 * The rows are decoded in blocks of max(1, 256 MiB / (8 w)) rows through one device staging buffer
 * (<= 256 MiB), allocated by the first call, reused, and freed by gm_destroy. Column shards (their own
 * w columns), join-ramp contexts and contexts recording msgcount or detection are supported. The call
 * is a read-back: it settles pending draw rounds, waits for the enqueued ticks, reports a latched
 * device error and changes nothing a later tick or read observes. GM_EINVAL: r0 < 0, count < 0,
 * r0 + count > n, a NULL array with count > 0 (count == 0 is GM_OK). FAITHFUL / PARTIAL:
 * GM_EUNSUPPORTED; between gm_load_begin and gm_load_commit: GM_ESTATE; a stored state whose escape
 * lists disagree with its cells: GM_ESTATE. */
int gm_read_rows(gm_ctx *ctx, int32_t r0, int32_t count, int32_t *hb, int32_t *ts);
/* stats = {rows decoded since gm_create, bytes of the staging buffer, and while gm_set_timing is on
 * the milliseconds spent in the decode kernel and in the device-to-host copies} */
int gm_read_rows_stats(gm_ctx *ctx, double stats[4]);
/* PARTIAL: the raw V-entry views (id << 32 | hb, 0 = empty, ascending id) of nodes
 * [r0, r0 + count) as of the last tick, [count][V]; a row shard reads its own nodes. */
int gm_read_views(gm_ctx *ctx, int32_t r0, int32_t count, uint64_t *out);
/* node state: inited, inGroup, bFailed, heartbeat counter (4 int32 per node) */
int gm_read_nodes(gm_ctx *ctx, int32_t *state4);
/* SCALED: the gossip targets every node drew in the last tick (the gossipnodes of nodeLoopOps,
 * MP1Node.cpp:449-489, as node indices; [n][5], unused slots 0) and their counts [n] -- with the
 * tables and node state, the whole state between two ticks.
 * PARTIAL: the same for this context's own nodes, [nloc][5] global node indices and counts [nloc]
 * (a row shard reads its own nodes, as gm_read_views does). A crashed node reports the targets of its
 * last tick until the next tick freezes it, count 0 from then on. */
int gm_read_targets(gm_ctx *ctx, int32_t *targets, int32_t *counts);
/* ---- SCALED: load a cluster state into a context, the inverse of gm_read_table / gm_read_nodes /
 * gm_read_targets (the oracle's oc_load_scaled, oracle/ref_cpu.c). The state between two ticks is
 * layout-independent, so a state read from a context of any band width, from column shards, or from
 * the oracle loads into any other. Contexts created with init_mode 0 or 1 only: FAITHFUL, PARTIAL,
 * join-ramp contexts and contexts recording msgcount return GM_EUNSUPPORTED. A column shard loads its
 * own columns [c0, c0 + w) and the same node arrays as every other shard.
 *
 * gm_load_begin settles the run so far, allocates a device staging buffer (<= 512 MiB whatever n is;
 * the commit frees it) and puts the context into the loading state: until gm_load_commit succeeds,
 * gm_tick, the shard phase calls and gm_set_failed return GM_ESTATE and the read-back functions are
 * undefined. t >= 1 is the next tick to run.
 * gm_load_rows gives rows [r0, r0 + count): hb / ts [count][w] over this context's w columns, -1 =
 * absent -- exactly what gm_read_table(r0, count) returns. Blocks in any order, each row exactly once
 * (a repeat, or a commit with rows missing: GM_ESTATE). The block is staged and encoded on the device.
 * gm_load_commit gives the heartbeat counters, crash flags (0 / 1), last tick's gossip targets [n][5]
 * and their counts [n] (0..5), builds the inboxes of tick t from them and sets the time to t. The
 * context is then as tick t - 1 would have left it: no pending events (gm_drain_events returns none,
 * gm_event_counts 0), the error flag clear. gm_event_totals and a detection recorder carry on.
 *
 * Everything is checked on the device before it is written. GM_EINVAL: ts > t - 1; one of hb / ts
 * negative and the other not; a heartbeat ahead of its row's tick; counts outside 0..5; a target
 * outside [0, n); failed not 0 / 1; a live row whose own entry is not {heartbeat - 1, t - 1} (the
 * self bump of tick t - 1; the cold start's {0, 0} with heartbeat 0 at t = 1 is the one exception);
 * a crashed row with targets that did not run tick t - 1. GM_ERANGE: an entry whose heartbeat lag or
 * age does not fit the cell (relative to t - 1, or for a crashed row to its newest ts); more lists
 * for one receiver than its inbox holds; a state that overflows the escape pools. After a failed
 * call the context stays in the loading state; gm_load_begin starts over. */
int gm_load_begin(gm_ctx *ctx, int32_t t);
int gm_load_rows(gm_ctx *ctx, int32_t r0, int32_t count, const int32_t *hb, const int32_t *ts);
int gm_load_commit(gm_ctx *ctx, const int32_t *heartbeat, const int32_t *failed, const int32_t *targets,
                   const int32_t *counts);
/* stats = {rows encoded since the last gm_load_begin, bytes of its staging buffer, and, while
 * gm_set_timing is on (HIP events around each launch, one wait per block), the milliseconds spent in
 * the check kernel and in the encode kernel} */
int gm_load_stats(gm_ctx *ctx, double stats[4]);

/* ---- PARTIAL: load a view state into a context, the inverse of gm_read_views / gm_read_nodes /
 * gm_read_targets. The state between two ticks -- every node's final view of tick t - 1, the heartbeat
 * counters, the crash flags, the targets drawn in t - 1 -- does not depend on the layout: a state read
 * from one context loads into G row shards (each its own nodes) and the other way round. FAITHFUL /
 * SCALED contexts and contexts recording msgcount or gm_view_detect_record (their history for ticks < t
 * would be missing) return GM_EUNSUPPORTED.
 *
 * gm_load_views_begin settles the run so far on both streams, discards undrained events, allocates one
 * device staging buffer of at most 256 MiB (max(1, 256 MiB / 8V) views per block; GM_LOAD_STAGE_ROWS
 * lowers that for tests; the commit frees it) and puts the context into the loading state: until
 * gm_load_views_commit succeeds, gm_tick, gm_partial_loopback_tick and gm_set_failed return GM_ESTATE
 * and the read-back functions are undefined. t is the next tick to run; it must be a tick a created
 * context could be at (init_t0 + 1 for an init_t0 gm_create accepts: 6 <= t <= 16384), else GM_EINVAL.
 * gm_load_views gives the views of nodes [r0, r0 + count), global indices inside this context's
 * [n0, n0 + nloc): [count][V], exactly what gm_read_views(r0, count) returns. Blocks in any order,
 * each node exactly once (a repeat, or a commit with nodes missing: GM_ESTATE).
 * gm_load_views_commit gives the heartbeat counters [nloc], the crash flags of the WHOLE cluster [n]
 * (every row shard the same array, as with gm_set_failed), the targets [nloc][5] and counts [nloc] of
 * this context's nodes as gm_read_targets returns them, builds the inboxes of tick t and sets the time
 * to t. The context is then as tick t - 1 would have left it: no pending events, the error flag clear,
 * the exchange block capacities and the crash-set hash following the loaded flags. A row shard's
 * received lists are not part of the state: its next tick first replays the exchange of tick t - 1
 * (every member of the group -- all RCCL ranks, all G loopback contexts -- must have committed a load;
 * a group where only some have latches GM_ESTATE on all of them).
 *
 * Everything is checked on the device before anything of the block or the commit is written.
 * GM_EINVAL for a view: an id outside [1, n]; ids not strictly ascending; a non-empty slot after an
 * empty one; an even heartbeat; a heartbeat above 2(t - 1) - 1; and, found at the commit, where the
 * flags are known, an entry of a live node's view aged GM_VIEW_AGES or more (what gm_view_census would
 * reject). GM_EINVAL at the commit: a node whose own entry is missing or not {heartbeat - 1}; a live
 * node whose heartbeat is not 2(t - 1); a crashed node whose heartbeat is odd or above 2(t - 1);
 * failed not 0 / 1; counts outside 0..5; a target outside [0, n), equal to the node itself, named
 * twice, or not an entry of the node's own view; a crashed node with targets that did not run tick
 * t - 1. GM_ERANGE: more lists for one receiver than its inbox holds (for lists sent by other row
 * shards, and for a packed exchange block past its capacity, at the tick that replays the exchange).
 * After a failed call the context stays in the loading state; gm_load_views_begin starts over. */
int gm_load_views_begin(gm_ctx *ctx, int32_t t);
int gm_load_views(gm_ctx *ctx, int32_t r0, int32_t count, const uint64_t *views);
int gm_load_views_commit(gm_ctx *ctx, const int32_t *heartbeat, const int32_t *failed, const int32_t *targets,
                         const int32_t *counts);
/* stats = {views stored since the last gm_load_views_begin, bytes of its staging buffer, and, while
 * gm_set_timing is on, the milliseconds spent in the check kernel and in the store kernel} */
int gm_load_views_stats(gm_ctx *ctx, double stats[4]);

/* ---- SCALED: the membership census, reduced on the device (the table is not copied to the host). */
#define GM_CENSUS_LAGS 64
#define GM_CENSUS_AGES 32
typedef struct gm_census_rec {   /* 40 bytes, one per subject column of this context */
  int32_t  hb_min, hb_max;       /* over the entries counted in holders; -1 = none */
  int32_t  ts_min, ts_max;       /* -1 = none */
  uint32_t holders;              /* live observers (failed == 0) whose table holds the subject */
  uint32_t stale;                /* of those, entries with T - ts >= TFAIL (what numfailed counts) */
  uint64_t hb_sum, ts_sum;       /* sums over the holders' entries */
} gm_census_rec;
/* SCALED. The state as of the last tick run, T = gm_time - 1 (after create or gm_load_commit: as
 * created / loaded). out[w] over this context's columns [c0, c0 + w) (gm_shard_layout);
 * hist[2][GM_CENSUS_LAGS][GM_CENSUS_AGES]: cells of live observers by (subject's failed flag,
 * lag = (2T - hb) >> 1 clipped to GM_CENSUS_LAGS - 1, age = T - ts). Either pointer may be NULL, not both.
 * (hb, ts) of a cell are what gm_read_table returns for it; rows with failed != 0 (frozen tables)
 * contribute nothing, a live observer's own entry counts. A column shard reports its own columns; the
 * shards' histograms add up to the cluster's. Join-ramp contexts are supported. The call is a
 * read-back: it waits for the enqueued ticks, reports a latched device error and changes nothing a
 * later tick or read observes. FAITHFUL / PARTIAL: GM_EUNSUPPORTED; while loading: GM_ESTATE; a
 * stored state whose escape lists disagree with its cells: GM_ESTATE. */
int gm_census(gm_ctx *ctx, gm_census_rec *out, uint64_t *hist);

/* ---- PARTIAL: the view census, reduced on the device (the views are not copied to the host). */
#define GM_VIEW_AGES  32
#define GM_VIEW_SIZES 33          /* view sizes 0..32 (P_VMAX) */
typedef struct gm_view_rec {      /* 24 bytes, one per subject node of the CLUSTER (index = id - 1) */
  int32_t  hb_min, hb_max;        /* over the entries counted in holders; -1 = none */
  uint32_t holders;               /* live observers (failed == 0) whose view holds the subject;
                                     a live node's own entry counts */
  uint32_t stale;                 /* of those, entries with T - (hb+1)/2 >= TFAIL */
  uint64_t hb_sum;
} gm_view_rec;
/* PARTIAL. The state as of the last tick run, T = gm_time - 1 (after create: as created, T = init_t0).
 * The views are exactly what gm_read_views returns; a view whose observer has failed != 0 is frozen
 * and contributes nothing to any output. out[n] over all subjects of the cluster;
 * hist[2][GM_VIEW_AGES]: entries of live observers by (subject's crash flag as given to
 * gm_set_failed, age = T - (hb + 1) / 2 -- the timestamp is derived from the heartbeat, so age and
 * heartbeat lag are one number); sizes[GM_VIEW_SIZES]: live observers by the entries their view holds.
 * Any of the three pointers may be NULL, not all. A row shard reduces its own nodes' views over all n
 * subjects: the shards' holders / stale / hb_sum / hist / sizes add up to the cluster's, hb_min /
 * hb_max combine by min / max over the shards that hold the subject (membership.merge_view_shards).
 * The call is a read-back: it waits for the enqueued ticks (both streams of a row shard), reports a
 * latched device error and changes nothing a later tick or read observes; its device scratch is
 * allocated by the first call and freed by gm_destroy. FAITHFUL / SCALED: GM_EUNSUPPORTED. A stored
 * entry that cannot be right -- an id outside [1, n], an even heartbeat, a heartbeat above 2T - 1, an
 * age >= GM_VIEW_AGES (the sweep removes at age 20) -- : GM_ESTATE, no output written. */
int gm_view_census(gm_ctx *ctx, gm_view_rec *out, uint64_t *hist, uint64_t *sizes);

/* ---- PARTIAL: reachability in the view graph, walked on the device (the views are not copied to the
 * host). A partial-view protocol is correct only while its overlay stays connected; the census shows
 * degrees, this shows paths. The definition is normative.
 *
 * The view graph G_T is taken at the last tick run, T = gm_time - 1 (after create or a view load: as
 * created / loaded). Vertices: the nodes whose crash flag is 0, as gm_read_nodes reports it (the flags
 * gm_view_census uses for observers). Edges: i -> j iff i and j are both vertices, i != j, and the
 * stored view of i (what gm_read_views returns) holds an entry with id j + 1. An entry naming a crashed
 * node, or the node itself, is not an edge; a crashed node's frozen view contributes nothing. Gossip
 * travels along edges: a node sends its list to targets drawn from its own view.
 *
 * Up to GM_REACH_SOURCES sources s_0 .. s_{nsrc-1} are walked independently (bit k of a 64-bit word per
 * node belongs to source k):
 *   GM_REACH_OUT  d_k(x) = length of the shortest path s_k -> x ("who can hear from s_k")
 *   GM_REACH_IN   d_k(x) = length of the shortest path x -> s_k ("whose gossip can reach s_k")
 * counts[GM_VIEW_HOPS][GM_REACH_SOURCES]: counts[h][k] = vertices x with d_k(x) == h, for h < max_hops;
 * counts[0][k] is 1 for a live source and 0 for a crashed one, whose whole column is 0; rows >= max_hops
 * and columns >= nsrc are 0. seen[n] (may be NULL): bit k of seen[x] is set iff d_k(x) < max_hops;
 * crashed nodes are 0. info = {live vertices, hops = the largest h with a non-zero row of counts,
 * stopped = 1 iff row max_hops - 1 is non-zero (the walk ended because of max_hops; 0: a level came up
 * empty first), live sources}. counts and info may not both be NULL. 1 <= max_hops <= GM_VIEW_HOPS;
 * max_hops = 1 returns the sources only, so calls with max_hops = 1, 2, 3, .. yield per-node distances
 * from seen. The same node may be named twice; its bits then behave identically.
 *
 * GM_EINVAL: nsrc outside 1..GM_REACH_SOURCES, a source outside [0, n), dir not 0 / 1, max_hops out of
 * range, sources NULL, counts and info both NULL. FAITHFUL / SCALED: GM_EUNSUPPORTED. Between
 * gm_load_views_begin and the commit: GM_ESTATE. A stored entry the walk meets whose id is outside
 * [1, n]: GM_ESTATE, nothing written to the caller's arrays. The call is a read-back: it reports a
 * latched device error, waits for the enqueued ticks, and writes nothing a tick or another read
 * observes. One launch pair per hop on the context's stream; the host reads the hop's row of counts
 * (512 bytes) to decide whether to go on. Its device scratch is one block, allocated by the first call
 * and freed by gm_destroy: the per-node words seen, front and next (3 x 8 n bytes) plus the counts
 * (32 KiB), the sources and a status word.
 *
 * Row shards. The definition does not change: G_T, counts and info are the whole cluster's, whichever
 * member reports them, and a sharded walk returns exactly what the single-context walk returns on the
 * joined state. Sources are global node indices and may lie on any shard. The members exchange the
 * frontier once per level: GM_REACH_IN gathers every member's last level into every member (8 bytes per
 * node of the other shards received per member and level); GM_REACH_OUT proposes into a cluster-wide
 * array and sends each member its slice of every other member's (the same size); each level's row of
 * counts is summed over the group, and every decision to walk another level is taken from summed rows
 * only. A member's device scratch is one block, allocated by its first sharded walk and freed by
 * gm_destroy: seen and two more word arrays over its own nodes, one over the cluster's n nodes, a
 * receive area of one slice of its own size per other member, the counts, the sources, a status word.
 * The walk reads the views of tick T, the crash flags and nothing of the tick's exchange: it runs on a
 * group whose exchange is still pending after a view load, and leaves it pending.
 *
 *   gm_view_reach on a context with a communicator (gm_comm_init) is a collective: every rank calls it
 *   with the same arguments. counts and info are the cluster's on every rank; seen has the rank's own
 *   nloc words (gm_shard_layout). A context of shard_count 1 with a communicator takes this path too,
 *   with the single-context results. Before the first level the ranks agree, by one MAX all-reduce of
 *   (h, ~h), on a hash of the sources, nsrc, dir, max_hops, the tick and the crash set; the result of
 *   each rank's own checks (a latched error, a load in progress) rides along. A disagreement, or a
 *   failed check on another rank: GM_ESTATE on every rank (the failing rank returns its own code).
 *   The argument errors above return GM_EINVAL before any collective. After the last level the status
 *   words are combined, so a bad entry met by one rank is GM_ESTATE on all. A row shard WITHOUT a
 *   communicator: GM_EUNSUPPORTED (it has nobody to exchange with).
 *
 *   gm_view_reach_loopback walks the G row-shard contexts of one cluster living on one device, device
 *   copies standing in for the collectives: the counterpart of gm_partial_loopback_tick, with its group
 *   checks (G >= 2, PARTIAL members, ranks 0 .. G - 1 in order, equal t, n, V and chunk count:
 *   GM_EINVAL otherwise). seen[n] is the whole cluster's, the shards' parts in node order. The argument
 *   errors of gm_view_reach: GM_EINVAL. A latched error of a member is returned; a member between
 *   gm_load_views_begin and its commit, or members holding different crash sets: GM_ESTATE. Nothing is
 *   written to the caller's arrays on any failure. The members' streams are waited for and the walk
 *   runs on the first member's stream, shard after shard. */
#define GM_VIEW_HOPS 64
#define GM_REACH_SOURCES 64
#define GM_REACH_OUT 0
#define GM_REACH_IN 1
int gm_view_reach(gm_ctx *ctx, const int32_t *sources, int32_t nsrc, int32_t dir, int32_t max_hops,
                  uint64_t *counts, uint64_t *seen, int64_t info[4]);
int gm_view_reach_loopback(gm_ctx **ctxs, int32_t G, const int32_t *sources, int32_t nsrc, int32_t dir,
                           int32_t max_hops, uint64_t *counts, uint64_t *seen, int64_t info[4]);

/* ---- PARTIAL: how crashed nodes fade from the views, recorded on the device. gm_detect_record stays
 * unsupported in this mode: a full view evicts a crashed node's stale entry in favour of fresher ones
 * long before TREMOVE, so REMOVED records are nearly absent and JOINED records are churn. What a
 * partial-view run is asked instead -- for how long does some live node still hold a dead node's
 * entry, how many observer-ticks of stale belief is that, does the entry still spread, how often does a
 * starved view remove a live node -- is reduced each recorded tick from what the tick leaves on the
 * device: its final views, the join masks over them and the removal records. The recorder holds only
 * that: an eviction writes no record and shows as `held` fading, not as a removal.
 *
 * Tick t is the tick that ran (the t of its gm_event records). "Crashed in tick t" and "live observer
 * in tick t" follow the crash flags as tick t saw them: the gm_set_failed calls made before it ran. */
typedef struct gm_view_detect_rec {  /* 48 bytes, one per subject node of the WHOLE cluster (index = id - 1) */
  int32_t  fail_tick;        /* as gm_detect_rec: last tick the node ran before gm_set_failed; -1 = never failed */
  int32_t  first_removed;    /* tick of the first REMOVED record naming it; -1 = none */
  int32_t  last_removed;     /* tick of the last one; -1 = none */
  uint32_t removals;         /* REMOVED records naming it (TREMOVE removals; evictions are not records) */
  uint32_t false_removals;   /* those logged in a tick during which the subject was not crashed */
  int32_t  last_held;        /* last recorded tick at whose end a live observer's view held it while it
                                was crashed; -1 = none. Extinction tick = last_held + 1. */
  uint32_t late_joins;       /* JOINED records naming it, logged by live observers while it was crashed */
  uint32_t reserved;         /* 0 */
  uint64_t removed_tick_sum; /* as gm_detect_rec */
  uint64_t held_sum;         /* sum over recorded ticks in which it was crashed of the live observers
                                holding it at the end of the tick: observer-ticks of stale belief */
} gm_view_detect_rec;
#define GM_VIEW_DETECT_COLS 5  /* timeline columns: joins, removals, false_removals, held, late_joins */
/* PARTIAL; FAITHFUL / SCALED: GM_EUNSUPPORTED. Start recording from the next tick, for ticks < tmax
 * (0 < tmax <= 32767, else GM_EINVAL); a tick >= tmax is not recorded at all. May be called between any
 * two ticks, also after gm_load_views_commit (fail_tick then follows the load's rule); a second call
 * returns GM_ESTATE. Device memory: 48 n + 40 tmax + n / 8 bytes. While recording, one reducer kernel
 * follows the tick's node kernels (inside the span gm_last_kernel_ms reports), gm_set_failed also
 * refreshes the recorder's crash bitmap, and gm_load_views_begin returns GM_EUNSUPPORTED (the history
 * for ticks before the load would be missing). While recording is off, no kernel, allocation or copy is
 * added to a tick. Recording does not depend on gm_keep_events and does not disturb gm_drain_events:
 * it only reads what a drain would read. */
int gm_view_detect_record(gm_ctx *ctx, int32_t tmax);
/* out[n], one record per subject of the cluster. A row shard reduces its own observers' views and
 * event rows over all n subjects and returns that part; fail_tick is filled on every shard from the
 * common crash set. The parts combine on the host (membership.merge_view_detect_shards): counts and
 * sums add, first_removed is the minimum over the parts that have one, last_removed and last_held the
 * maximum. GM_ESTATE before gm_view_detect_record, and when a recorded tick met a view entry or a
 * removal record that cannot be right (an id outside [1, n], a record count past the event row). */
int gm_view_detect(gm_ctx *ctx, gm_view_detect_rec *out);
/* out[t][GM_VIEW_DETECT_COLS], row i for tick i < t <= tmax (t <= 0 or t > tmax: GM_EINVAL): joins =
 * all JOINED records of the tick; removals = all REMOVED records; false_removals = those whose subject
 * was not crashed in the tick; held = entries naming a subject crashed in the tick, in the tick's final
 * views of the observers live in it; late_joins = the JOINED records among those held entries. A tick
 * before recording began is all zero. A row shard reports its own observers' rows; the shards'
 * timelines add up. GM_ESTATE as gm_view_detect. */
int gm_view_detect_timeline(gm_ctx *ctx, int32_t t, uint64_t *out);

/* ---- SCALED / PARTIAL: layout-independent digests of the state between two ticks, computed on the
 * device (the tables and views are not copied to the host). The definition is normative; all
 * arithmetic is mod 2^64, mix is splitmix64's finalizer (gm_mix64, csrc/gm_device.h):
 *
 *   GM_DIGEST_VERSION 1
 *   KCOL  = 0x6D656D6265727368   KNODE = 0x6E6F646573746174   KROW = 0x726F77666F6C6421
 *
 *   kcol(c)         = mix(KCOL ^ c)                        c = global subject index (id - 1)
 *   cell(c, hb, ts) = mix(kcol(c) ^ ((uint64)hb << 32 | (uint32)ts))
 *   rows[r]         = sum of cell(c, hb, ts) over the PRESENT entries (hb >= 0) of observer r among this
 *                     context's columns
 *                     -- (hb, ts) exactly what gm_read_table / gm_read_rows return
 *                     -- PARTIAL: the entries of the view gm_read_views returns, c = id - 1, ts = (hb + 1) / 2
 *   knode(r)        = mix(KNODE ^ r)                       r = global node index
 *   nodes[r]        = mix(knode(r) ^ ((uint64)heartbeat << 8 | count << 3 | failed << 2 | inGroup << 1 | inited))
 *                     + sum over q < count of mix(mix(knode(r) + q + 1) ^ (uint64)target_q)
 *                     -- the four words of gm_read_nodes, and counts / targets (draw order) of gm_read_targets
 *                     -- slots >= count are not read: the device array holds anything there
 *   fold(r, x)      = mix(mix(KROW ^ r) ^ x)
 *   sums[0] = sum over r of fold(r, rows[r])   sums[1] = sum over r of fold(r, nodes[r])   over this context's nodes
 *
 * An absent entry adds nothing; a present {0, 0} (cold start) adds mix(kcol(c)), so it differs from an
 * absent one. Rows of crashed observers (frozen tables, based at the tick they last ran) are part of the
 * state and are digested -- here the digest differs from the censuses. The definition does not depend on
 * the band width, on the fast or the general path, on column or row sharding, or on whether the state was
 * ticked, loaded or produced by the oracle (membership.digest restates it in NumPy).
 * SCALED column shard: rows[r] covers its own columns [c0, c0 + w); nodes[r] is the node word for
 * c0 <= r < c0 + w and 0 elsewhere (a shard's heartbeat counter is current only for the nodes whose
 * column it holds). The shards' rows and nodes therefore ADD UP element-wise to the single context's
 * arrays; a shard's own sums are of its partial words and only comparable between equal layouts: the
 * cluster's sums come from folding the added arrays (membership.digest.merge_columns).
 * PARTIAL row shard: arrays of its own nloc nodes, with global r: the arrays concatenate and the
 * shards' sums add up to the cluster's (membership.digest.merge_rows). */
#define GM_DIGEST_VERSION 1
/* SCALED / PARTIAL; FAITHFUL: GM_EUNSUPPORTED. The state as of the last tick run (after create or a
 * load commit: as created / loaded). sums[2], rows and nodes [n] (PARTIAL: [nloc]); any of the three
 * pointers may be NULL, not all (GM_EINVAL). Column shards, row shards, join-ramp contexts and contexts
 * recording msgcount or detection are supported. The call is a read-back: it settles pending draw
 * rounds, waits for the enqueued ticks (both streams of a row shard), reports a latched device error and
 * writes nothing a tick or another read observes; its device scratch (one block: the two word arrays,
 * the sums, the status word) is allocated by the first call and freed by gm_destroy. Between
 * gm_load_begin / gm_load_views_begin and the commit: GM_ESTATE. A stored state whose escape lists
 * disagree with its cells (a piece's escape bytes against its list's count, the pool extent against the
 * stripe's region, every entry a column < band that holds an escape byte), or a view entry with an id
 * outside [1, n]: GM_ESTATE, nothing written to the caller's arrays. */
int gm_digest(gm_ctx *ctx, uint64_t sums[2], uint64_t *rows, uint64_t *nodes);
/* Start recording from the next tick, for ticks < tmax (0 < tmax <= 32767, else GM_EINVAL; a second
 * call: GM_ESTATE): after each such tick t the digest kernels run on the stream that ran the tick,
 * behind its last kernel (inside the span gm_last_kernel_ms reports), and write sums into row t of a
 * device array [tmax][2] -- no host wait, no copy. Row t holds what gm_digest would return if called
 * right after that gm_tick, before any gm_set_failed that follows it. FAITHFUL: GM_EUNSUPPORTED. SCALED
 * column shards: GM_EUNSUPPORTED (their targets are settled by deferred draw rounds, after the point
 * where a stream-ordered reducer could run; gm_digest on demand serves them). PARTIAL row shards record
 * their own nodes; the shards' traces add up. While recording is off a tick gains no kernel, no
 * allocation and no copy. Recording does not depend on gm_keep_events; loads are allowed while
 * recording (a tick that did not run leaves its row 0). */
int gm_digest_record(gm_ctx *ctx, int32_t tmax);
/* out[t][2] = sums recorded after tick i, for i < t <= tmax (t <= 0 or t > tmax: GM_EINVAL). A tick
 * before recording began, or one that never ran, is {0, 0}. GM_ESTATE before gm_digest_record, and when
 * a recorded tick raised the status word (an inconsistent stored state, as gm_digest). */
int gm_digest_trace(gm_ctx *ctx, int32_t t, uint64_t *out);

/* Render the membership lists of every node in the parity dump format
 * ("t i inited inGroup bFailed heartbeat n id:hb:ts ...\n" per node). */
int gm_dump_tables(gm_ctx *ctx, char *buf, size_t cap, size_t *len);

/* SCALED telemetry of the last tick: [0]=delivered gossip lists M, [1]=live nodes,
 * [2]=max inbox depth, [3]=error flags */
int gm_tick_stats(gm_ctx *ctx, int64_t stats[4]);
/* SCALED escape storage as sized at create: info = {1 if the pools are dense-equivalent (no run can
 * overflow them) else 0, table escape-pool entries, payload escape-pool 16-byte slots, event spill
 * ring records}; GM_EUNSUPPORTED for the other modes */
int gm_pool_info(gm_ctx *ctx, int64_t info[4]);
/* Mean per-tick duration (ms) of the tick kernel over the timing window, measured
 * with HIP events recorded on the context stream before the window's first
 * kernel and after its last. gm_set_timing(ctx, 1) opens a new window at the
 * next tick; 0 when nothing was timed. */
int gm_set_timing(gm_ctx *ctx, int32_t on);
int gm_last_kernel_ms(gm_ctx *ctx, float *ms);

/* ---- FAITHFUL batches: R contexts of one device ticked together. The seam is R independent
 * Application processes (Application.cpp:27-202 run R times: the grader's three testcases, the seed
 * pairs of an ensemble): the members share nothing and may differ in n, seeds, conf values, dropmsg
 * state, crash sets, globaltime and whether they record detection. A batch tick is the same seven
 * launches as gm_tick's with the member as a second grid dimension, so R clusters cost about the
 * launch latency of one.
 * gm_batch_create: waits once for what each member has enqueued; from then until gm_batch_destroy the
 * members run on the batch's stream, so every call on a member (gm_tick, gm_rand, gm_set_failed,
 * gm_set_dropmsg, gm_drain_events, gm_msgcount, gm_dump_tables, gm_read_*, gm_detect*, gm_event_*,
 * gm_sync, gm_time) keeps its meaning and is ordered with the batch ticks; a gm_tick of one member
 * between two batch ticks leaves that member one tick further than the others. One host thread drives
 * a batch and its members. GM_EINVAL: ctxs or out NULL, R < 1 or R > 65535, a NULL member, the same
 * context twice, members on different devices; GM_EUNSUPPORTED: a member is not FAITHFUL; GM_ESTATE: a
 * member already belongs to a batch. gm_destroy of a member returns GM_ESTATE and destroys nothing.
 * gm_batch_tick: one gm_tick of every member -- the same tables, records, counters and S1 stream bit
 * for bit -- enqueued without a host wait. All or nothing: it first checks every member and collects
 * the mailboxes that are due (a member's record buffer could fill, or the detection recorder needs
 * the enqueued ticks before a crash flag is reset), all of them with one host wait; then either every
 * member's tick is enqueued and every globaltime advances, or nothing is and none does. Returns the
 * lowest-index member's latched error if a member has one, GM_ERANGE if a member is at MAX_TIME
 * (EmulNet.h:11). gm_set_timing / gm_last_kernel_ms of a member are not fed by batch ticks.
 * gm_batch_destroy: waits for the batch's stream and gives the members their own streams back; they
 * live on. */
typedef struct gm_batch gm_batch;
int gm_batch_create(gm_ctx **ctxs, int32_t R, gm_batch **out);
int gm_batch_tick(gm_batch *b);
int gm_batch_destroy(gm_batch *b);

/* ---- SCALED column sharding (multi-GPU). A context with shard_count = G > 1
 * owns subject columns [c0, c0 + w) of every observer row (one context per GPU).
 * Once RCCL is attached (gm_comm_init, same unique id on every rank), gm_tick
 * runs the sharded tick: merge/sweep own columns -> ncclAllGather of per-row
 * (present, numfailed) -> rounds of {draw + resolve own-column draws ->
 * ncclAllReduce(MAX) of resolved draws -> acceptance} until every row has its
 * gossip targets (stream-ordered bounded rounds; rows they cannot take finish in host-driven
 * rounds before the tick is read or the next one starts). No gossip payload crosses GPUs. The phase functions expose
 * the same steps for G contexts on one device (gm_shard_loopback: the tick's own collectives
 * over a group of G contexts). */
int gm_comm_unique_id(uint8_t *out128);   /* ncclGetUniqueId, on one rank */
/* ncclCommInitRank, then an all-gather of the config words every rank must share (mode, n,
 * band, view, GM_CHUNKS, seeds, drop schedule, init state): GM_EINVAL if any rank differs.
 * The seam it replaces: every MP1Node shares one Params / EmulNet (Application.cpp:47-66). */
int gm_comm_init(gm_ctx *ctx, const uint8_t *id128, int32_t nranks, int32_t rank);
/* info = {ranks in the RCCL communicator (0 before gm_comm_init), this rank in it (-1),
 * the device RCCL bound (-1), the context's HIP device} */
int gm_comm_info(gm_ctx *ctx, int32_t info[4]);
int gm_shard_layout(gm_ctx *ctx, int32_t *c0, int32_t *w);
int gm_shard_merge(gm_ctx *ctx);
int gm_shard_draw(gm_ctx *ctx, int32_t round, int32_t D);
int gm_shard_accept(gm_ctx *ctx, int32_t D, int32_t *npending);
int gm_shard_end_tick(gm_ctx *ctx);
/* what = 0: all-gather the per-row counts; what = 1: MAX-allreduce the first n*D draws;
 * what = 2 (msgcount recording, after what = 0): SUM-allreduce this tick's fresh counts */
int gm_shard_loopback(gm_ctx **ctxs, int32_t G, int32_t what, int32_t D);
/* One whole tick of the G column-shard contexts of one cluster on one device: the sharded tick
 * gm_tick runs per rank (the same host code over the group of G contexts, on the first context's
 * streams), its collectives done by device copies and reduce kernels instead of RCCL. It takes
 * gm_tick's decisions: pipelined over the exchange row chunks with the bounded rounds 1, 2 run only
 * when round 0 left rows pending, or the host-driven draw loop under mass failure / heavy loss
 * (GM_SHARD_SYNC). The tick is complete when the call returns: rows the bounded rounds cannot take
 * finish in host-driven rounds here (gm_tick leaves them to the next call on the context), and
 * shards that count different pending rows return GM_ESTATE. Not for the join ramp or msgcount
 * recording (GM_EINVAL; use the phase API). */
int gm_shard_loopback_tick(gm_ctx **ctxs, int32_t G);
/* Host-collective hook: the exchange buffers of ONE column-shard context as host arrays, so a
 * host-side collective (e.g. gloo between processes) can stand in for RCCL or gm_shard_loopback
 * between the phase calls. what = 0: export this rank's per-row counts int32[n][2], import all
 * G slots int32[G][n][2]; what = 1: export / import the draws int32[n][D] (import their MAX over
 * the ranks); what = 2 (msgcount recording): uint32[n] fresh counts (+ uint32[n] kept entries on
 * keyed-loss ticks), import their SUM. gm_shard_export with out = NULL returns the size in *bytes;
 * gm_shard_import requires exactly that many bytes. (The seam they replace is EmulNet's shared
 * in-process buffer, EmulNet.cpp:87-177, which the reference's single process never had to cross.) */
int gm_shard_export(gm_ctx *ctx, int32_t what, int32_t D, void *out, size_t cap, size_t *bytes);
int gm_shard_import(gm_ctx *ctx, int32_t what, int32_t D, const void *in, size_t bytes);
/* Diagnostics: tick ONE column shard alone on a device (no RCCL): peers' per-row counts
 * mirror this shard's and draws landing in peer columns resolve to fresh column ix --
 * the real kernels at the true shard shape, for measurement only (not a simulation). */
int gm_shard_stub(gm_ctx *ctx, int32_t on);

/* ---- PARTIAL row sharding (scenario S-C multi-GPU). A PARTIAL context with
 * shard_count = G > 1 owns nodes [n*g/G, n*(g+1)/G) (gm_shard_layout returns the
 * range; gm_read_nodes / gm_dump_tables / gm_drain_events / gm_tick_stats report
 * its own nodes, with global indices). With RCCL attached (gm_comm_init) gm_tick
 * runs the local kernels in row chunks and, per chunk on a second stream, two
 * ncclAllToAllv of fixed-size blocks (record headers stamped with the tick; the lists'
 * fresh entries, 4 bytes each, read in place by the next tick) -- sizes come from the
 * shard layout, so no host round trip -- then appends the received records to their
 * targets' inboxes. After every change of the crash set the ranks agree on its hash (the block
 * sizes follow from it); a rank holding another set latches GM_ESTATE. gm_partial_loopback_tick runs
 * the same tick (the same host code) over the G contexts of one cluster on one device, the block
 * exchange by device copies and the agreement on the host, where it latches GM_ESTATE on all G; a
 * device error of the tick (an overflowing block: GM_ERANGE) is returned by the call. */
int gm_partial_loopback_tick(gm_ctx **ctxs, int32_t G);
/* bytes this shard received from the other shards in the last tick's exchange (whole blocks) */
int gm_shard_exchange_bytes(gm_ctx *ctx, int64_t *bytes);

/* Crash set of the SCALED fault schedule: `count` node indices, ascending,
 * chosen by a splitmix64-keyed permutation of [0, n) (host fault injection). */
int gm_crash_set(int32_t n, int32_t count, uint64_t seed, int32_t *out);

const char *gm_strerror(int code);

#ifdef __cplusplus
}
#endif
#endif /* GM_ABI_H */
