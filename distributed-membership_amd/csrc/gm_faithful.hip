// gm_faithful.hip -- FAITHFUL-mode tick kernels (the reference's own regime:
// N <= 1000, EmulNet buffer cap 30000, per-entry messages, glibc-rand drops).
//
// One Application::mp1Run tick (Application.cpp:121-164) = three launches:
//   gm_f_recv   recv phase: EmulNet::ENrecv for receivers ascending
//               (EmulNet.cpp:144-177). One workgroup walks the receivers in
//               order; for each it matches the buffer in parallel, emits the
//               matches in descending buffer index (the order the reference's
//               backward scan dequeues them) and applies the swap-with-last
//               compaction in closed form: the i-th hole from the top is
//               filled from position B-i, following the chain through holes
//               that were themselves refilled earlier in the scan.
//   gm_f_node   node phase: nodeStart / nodeLoop for every node in parallel
//               (one workgroup per node; MP1Node.cpp:73-163,182-495). The
//               queue merge is commutative on the table (max heartbeat); the
//               order-dependent parts -- joined-event order and newNodes
//               order -- come from first-occurrence positions in the queue.
//               Sweep, self bump (incl. the updateMyPos `&&` quirk) and the
//               mt19937 + Lemire gossip-target draw run per node.
//   gm_f_send   EmulNet::ENsend for every send of the tick (EmulNet.cpp:87-118):
//               sends are ordered node-descending (the node-phase order), each
//               consumes the next glibc rand() draw of the S1 stream; the
//               30000 cap is a prefix count over the not-drop-drawn sends.
#include <type_traits>
#include "gm_device.h"
#include "gm_abi.h"
#include "gm_faithful.h"

#define F_RECV_THREADS 1024
#define F_NODE_THREADS 256
#define F_SEND_THREADS 1024

__device__ __forceinline__ uint32_t f_strkey(int32_t id) {
  // strcmp over the 6 address bytes {id LE, port 0} compares up to the first
  // NUL byte (EmulNet.cpp:154): keep the bytes before the first zero byte.
  uint32_t u = (uint32_t)id, key = 0;
  for (int b = 0; b < 4; b++) {
    uint32_t byte = (u >> (8 * b)) & 0xFFu;
    if (byte == 0) break;
    key |= byte << (8 * b);
  }
  return key;
}

// ---------------------------------------------------------------- recv phase
// gm_f_recv (one workgroup) walks the receivers ascending on an LDS image of the buffer:
// one u32 per buffered message, its destination key << 16 | its index in the tick-start
// buffer (F_ENBUFFSIZE < 2^16; the key -- the strcmp prefix of the destination address,
// EmulNet.cpp:154 -- of ids 1..n is <= n; it is kept beside the buffer in bkey), message
// counts per (key, segment of `seg` slots, seg sized from n so the table stays ~24 KB),
// the receivers' active flags and two k-entry scratch arrays. Per receiver with k messages:
//   ranks  a DPP scan over the key's segment counts gives every segment's first rank;
//   scan   waves take the segments holding a match (and those of the vacated tail
//          [B-k, B)) round-robin; a match stores its position at hit[rank], every tail
//          slot gets its hole rank (1-based descending, 0 = no match);
//   fill   one thread per rank: queue slot k-1-rank (descending buffer index = the
//          reference's dequeue order) gets the message's tick-start index, and a match
//          below B-k is overwritten in closed form: the hole of descending rank i
//          receives what sits at B-i when it is processed, i.e. follow the chain
//          through earlier tail holes to an original element;
// with one LDS-only barrier after each. gm_f_recvout (many workgroups) then materialises
// the queues and compacts the survivors into the other buffer. Ranks over the LDS room
// use the same code on global scratch with full barriers.
#define F_EL_SLOTS ((F_ENBUFFSIZE + 255) / 256 * 256)  // el[] incl. the b128 overread pad
#define F_CW_BYTES 24576                               // count table budget
static_assert(4 * F_EL_SLOTS + F_CW_BYTES + 4 * (F_MAX_NODES + 1) + F_MAX_NODES + 4 * 1024 <= F_RECV_LDS,
              "gm_f_recv LDS budget");

__device__ __forceinline__ void lds_barrier() {
  // every wave's LDS traffic done, then the barrier; global stores stay in flight
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// Every kernel of the tick exists twice over ONE body (gm_faithful_tick.h, included as text): gm_f_*
// runs it for the cluster given as kernel arguments (gm_tick), gm_fb_* for the member blockIdx.y of a
// batch (gm_batch_tick), whose state and tick it loads from the batch's slots first.
//
// A batched workgroup's member: slot blockIdx.y as uploaded, `step` batch ticks later. The index is
// the same for the whole workgroup, so the slot comes in by scalar loads. Every tick swaps buf / buf2
// and bkey / bkey2 (gm_f_recvout compacts the survivors into the other buffer): the kernels up to
// gm_fb_recvout see the order the tick starts with (post 0), the ones after it the swapped one (post 1).
__device__ __forceinline__ FState fb_member(const FBSlot *__restrict__ slots, int step, int post, int *t) {
  const FBSlot *m = slots + blockIdx.y;
  FState s = m->f;
  *t = m->t + step;
  if ((step + post) & 1) {
    FMsg *b = s.buf;
    s.buf = s.buf2;
    s.buf2 = b;
    uint16_t *k = s.bkey;
    s.bkey = s.bkey2;
    s.bkey2 = k;
  }
  return s;
}

__global__ __launch_bounds__(F_RECV_THREADS) void gm_f_recv(FState s, int t) {
#define F_BODY_RECV
#include "gm_faithful_tick.h"
}
__global__ __launch_bounds__(F_RECV_THREADS) void gm_fb_recv(const FBSlot *slots, int step) {
  int t;
  FState s = fb_member(slots, step, 0, &t);
#define F_BODY_RECV
#include "gm_faithful_tick.h"
}

// queues and survivors (grid-stride over both), recv_msgs counters
__global__ __launch_bounds__(256) void gm_f_recvout(FState s, int t) {
#define F_BODY_RECVOUT
#include "gm_faithful_tick.h"
}
__global__ __launch_bounds__(256) void gm_fb_recvout(const FBSlot *slots, int step) {
  int t;
  FState s = fb_member(slots, step, 0, &t);
#define F_BODY_RECVOUT
#include "gm_faithful_tick.h"
}

// ---------------------------------------------------------------- node phase
__device__ void f_emit(FState &s, int t, int i, int seq, int kind, int subject) {
  unsigned long long slot = atomicAdd(s.ev_count, 1ull);
  if (slot < (unsigned long long)s.ev_cap) {
    FEvent e;
    e.t = t;
    e.logger = i;
    e.kind = kind;
    e.subject = subject;
    e.seq = seq;
    s.ev[slot] = e;
  } else {
    atomicOr(s.err, GM_ERR_EVENTS);
  }
}

__global__ __launch_bounds__(F_NODE_THREADS) void gm_f_node(FState s, int t) {
#define F_BODY_NODE
#include "gm_faithful_tick.h"
}
__global__ __launch_bounds__(F_NODE_THREADS) void gm_fb_node(const FBSlot *slots, int step) {
  int t;
  FState s = fb_member(slots, step, 1, &t);
  if ((int)blockIdx.x >= s.n) return;  // the grid is the largest member's
#define F_BODY_NODE
#include "gm_faithful_tick.h"
}

// ---------------------------------------------------------------- send phase
// S1: one glibc rand() draw per ENsend, in send order (EmulNet.cpp:90). glibc TYPE_3 keeps
// rptr 3 words behind fptr (mod 31), both advancing by one per draw. With the ring rotated
// so that x[j] is the word fptr reaches at step j of a 31-step round, step j is
// x[j] += x[(j + 28) % 31] and its draw is x[j] >> 1: a round maps the register vector v
// linearly (mod 2^32) to v' = R v and its 31 draws are v' >> 1. So round m's draws are
// (R^(m+1) v0) >> 1, computed in parallel from precomputed powers: the prep kernel steps
// block states v_(64b) = (R^64)^b v0 serially (one 31x31 product per 1984 draws) and the
// expansion evaluates round 64b + q as R^(q+1) v_(64b), one output word per lane.

// node-phase order is i descending: exclusive scan of scount over i = n-1..0; S1 block states
__global__ __launch_bounds__(64) void gm_f_sendprep(FState s) {
#define F_BODY_SENDPREP
#include "gm_faithful_tick.h"
}
__global__ __launch_bounds__(64) void gm_fb_sendprep(const FBSlot *slots, int step) {
  int t;
  FState s = fb_member(slots, step, 1, &t);
  (void)t;
#define F_BODY_SENDPREP
#include "gm_faithful_tick.h"
}

// the tick's S draws: round m (lanes 0..30 of a half-wave) = P_(m mod 64) v_(64 (m / 64));
// the rounds holding the last draw write the register back (words j < S mod 31 from round
// S/31, the rest from round S/31 - 1; none change when S < 31 for j >= S)
__global__ __launch_bounds__(256) void gm_f_s1expand(FState s) {
#define F_BODY_S1EXPAND
#include "gm_faithful_tick.h"
}
__global__ __launch_bounds__(256) void gm_fb_s1expand(const FBSlot *slots, int step) {
  int t;
  FState s = fb_member(slots, step, 1, &t);
  (void)t;
#define F_BODY_S1EXPAND
#include "gm_faithful_tick.h"
}

// ENsend's drop draw and the 30000 cap (EmulNet.cpp:90-99): exclusive prefix count of the
// not-drop-drawn sends in send order (pre[o]); a send is buffered at B0 + pre[o] iff kept
// and pre[o] < room. One workgroup; thread t scans a contiguous run of ordinals.
__global__ __launch_bounds__(F_SEND_THREADS) void gm_f_sendscan(FState s, int t) {
#define F_BODY_SENDSCAN
#include "gm_faithful_tick.h"
}
__global__ __launch_bounds__(F_SEND_THREADS) void gm_fb_sendscan(const FBSlot *slots, int step) {
  int t;
  FState s = fb_member(slots, step, 1, &t);
#define F_BODY_SENDSCAN
#include "gm_faithful_tick.h"
}

// materialise every buffered send (grid-stride over ordinals)
__global__ __launch_bounds__(256) void gm_f_sendemit(FState s) {
#define F_BODY_SENDEMIT
#include "gm_faithful_tick.h"
}
__global__ __launch_bounds__(256) void gm_fb_sendemit(const FBSlot *slots, int step) {
  int t;
  FState s = fb_member(slots, step, 1, &t);
  (void)t;
#define F_BODY_SENDEMIT
#include "gm_faithful_tick.h"
}
