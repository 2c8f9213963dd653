// gm_load_views.hip -- PARTIAL: load a view state into a context (gm_load_views_begin / gm_load_views /
// gm_load_views_commit, the inverse of gm_read_views / gm_read_nodes / gm_read_targets).
//
// The PARTIAL state between two ticks is what the tick kernels of tick t read of tick t - 1: every
// node's final list (lists[(t - 1) & 1], id << 32 | hb, id-sorted, 0 = empty), the heartbeat counters,
// the crash flags and the gossip targets drawn in t - 1. The inboxes of tick t follow from the
// targets; a row shard's received lists follow from its peers' lists and targets (the replayed
// exchange of tick t - 1, gm_host_partial.hip). So a load is a check-and-store pass:
//
//   gm_pl_check  half-wave per staged node (V <= 32 lanes, one 8-byte entry per lane, two nodes per
//                wave: a row is one coalesced run). Per lane: the id in [1, n], the heartbeat odd and
//                at most 2(t - 1) - 1. The strict id order by a shuffle from the lane below; "no entry
//                after an empty slot" by a ballot of the occupied lanes (it must be a run of low bits).
//                A violation ORs its code into the status word; nothing else is written.
//   gm_pl_store  (after the host read a clean status) the staged rows into lists[(t - 1) & 1], the
//                view size into rowstat[.][1], the node's bit into the "given" bitmap.
//   gm_pl_nodes  half-wave per node over the STORED list, check (write = 0) then write (write = 1):
//                crash flag 0 / 1, count 0..5; the node's own entry present as {heartbeat - 1} (a
//                ballot of id == self && hb == heartbeat - 1); a live node's heartbeat 2(t - 1) and no
//                entry of its view aged GM_VIEW_AGES or more (liveness is known at the commit only, so
//                this view check is made here); a crashed node's heartbeat even and at most 2(t - 1),
//                and targets only if it ran tick t - 1; every target in [0, n), not the node itself,
//                named once, and an entry of the node's view (one ballot per target). The write pass
//                stores hbctr, failed, targets and rowstat's count word, clears the node's event words
//                and rowstat[.][0, 2] and both parities' inbox counters.
//   gm_pl_inbox  thread per node: each LOCAL target's inbox of parity t & 1 gets the node's row by one
//                returning atomic (p_node's send round, p_send: row[1 + slot] = li); a receiver past kcap is
//                GM_PL_EINBOX. Targets owned by another row shard are left to the exchange.
#include <hip/hip_runtime.h>

#include "gm_abi.h"
#include "gm_device.h"
#include "gm_partial.h"

static_assert(P_VMAX == 32, "a view is one half-wave");

__device__ __forceinline__ uint32_t pl_half(uint64_t bal, int sub) { return (uint32_t)(bal >> (32 * sub)); }

// staged rows [0, cnt) = local rows [r0, r0 + cnt); stage [cnt][V]
__global__ __launch_bounds__(256) void gm_pl_check(PState s, int t, int cnt, const uint64_t *__restrict__ stage,
                                                   uint32_t *status) {
  const int lane = threadIdx.x & 63, sub = lane >> 5, e = lane & 31;
  const int64_t node = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 2 + sub;
  const bool on = node < cnt && e < s.V;
  const uint64_t x = on ? stage[node * s.V + e] : 0ull;
  const uint32_t id = (uint32_t)(x >> 32), hb = (uint32_t)x;
  const uint32_t below = (uint32_t)__shfl_up((int)id, 1, 32);  // lane e - 1 of this half-wave
  const uint32_t held = pl_half(__ballot(x != 0), sub);
  uint32_t bad = 0;
  if (x != 0) {
    if (id < 1u || id > (uint32_t)s.n) bad |= GM_PL_EID;
    if (e > 0 && below >= id) bad |= GM_PL_EORDER;
    if (!(hb & 1u)) bad |= GM_PL_EHBPAR;
    if (hb > (uint32_t)(2 * t - 3)) bad |= GM_PL_EHBTOP;
  }
  if (e == 0 && (held & (held + 1u))) bad |= GM_PL_EGAP;  // occupied lanes must be a run from lane 0
  if (bad) atomicOr(status, bad);
}

__global__ __launch_bounds__(256) void gm_pl_store(PState s, int t, int r0, int cnt, const uint64_t *__restrict__ stage,
                                                   uint32_t *given) {
  const int lane = threadIdx.x & 63, sub = lane >> 5, e = lane & 31;
  const int64_t node = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 2 + sub;
  const bool on = node < cnt && e < s.V;
  const uint64_t x = on ? stage[node * s.V + e] : 0ull;
  const uint32_t held = pl_half(__ballot(x != 0), sub);
  if (!on) return;
  const size_t li = (size_t)r0 + (size_t)node;
  s.lists[((size_t)((t - 1) & 1) * s.rows + li) * s.V + e] = x;
  if (e == 0) {
    s.rowstat[li * 4 + 1] = __builtin_popcount(held);
    atomicOr(given + (li >> 5), 1u << (li & 31));
  }
}

// nodes [r0, r0 + cnt) of this context (local rows); heartbeat / failed / counts [cnt], targets [cnt][5]
__global__ __launch_bounds__(256) void gm_pl_nodes(PState s, int t, int r0, int cnt, const int32_t *__restrict__ heartbeat,
                                                   const int32_t *__restrict__ failed, const int32_t *__restrict__ counts,
                                                   const int32_t *__restrict__ targets, const uint32_t *__restrict__ given,
                                                   uint32_t *status, int write) {
  const int lane = threadIdx.x & 63, sub = lane >> 5, e = lane & 31;
  const int64_t node = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 2 + sub;
  const bool on = node < cnt;
  const size_t li = (size_t)r0 + (size_t)(on ? node : 0);
  const int i = s.n0 + (int)li;  // global node index
  const int f = on ? failed[node] : 0, k = on ? counts[node] : 0, hbc = on ? heartbeat[node] : 0;
  const int top = 2 * (t - 1);
  const bool ran = hbc == top;   // the node ran tick t - 1
  if (write) {
    if (!on) return;
    if (e < GM_FANOUT) s.targets[li * GM_FANOUT + e] = e < k ? targets[node * GM_FANOUT + e] : 0;
    if (e == 0) {
      s.hbctr[li] = hbc;
      s.failed[li] = f;
      s.rowstat[li * 4] = 0;
      if (f && !ran) s.rowstat[li * 4 + 1] = 0;  // frozen by an earlier tick (p_frozen)
      s.rowstat[li * 4 + 2] = 0;
      s.rowstat[li * 4 + 3] = k;
      s.ev_cnt[li] = 0;
      s.ev_jm[li] = 0;
      s.inbox[0][li * P_KMAX] = 0;
      s.inbox[1][li * P_KMAX] = 0;
    }
    return;
  }
  const uint64_t x = on && e < s.V ? s.lists[((size_t)((t - 1) & 1) * s.rows + li) * s.V + e] : 0ull;
  const uint32_t id = (uint32_t)(x >> 32), hb = (uint32_t)x;
  uint32_t bad = 0;
  const uint32_t self = pl_half(__ballot(x != 0 && id == (uint32_t)(i + 1) && hb == (uint32_t)(hbc - 1)), sub);
  const int kk = min(max(k, 0), GM_FANOUT);
  int tg[GM_FANOUT];
#pragma unroll
  for (int q = 0; q < GM_FANOUT; q++) {
    tg[q] = on && q < kk ? targets[node * GM_FANOUT + q] : -1;
    // the ballot is taken by the whole wave, whatever this half-wave's count
    const uint32_t inview = pl_half(__ballot(x != 0 && tg[q] >= 0 && id == (uint32_t)tg[q] + 1u), sub);
    if (q < kk) {
      if (tg[q] < 0 || tg[q] >= s.n || tg[q] == i || !inview) bad |= GM_PL_ETARGET;
#pragma unroll
      for (int j = 0; j < q; j++)
        if (tg[j] == tg[q]) bad |= GM_PL_ETARGET;
    }
  }
  if (on) {
    if (!((given[li >> 5] >> (li & 31)) & 1u)) bad |= GM_PL_EMISSING;
    if (f != 0 && f != 1) bad |= GM_PL_EFAILED;
    if (k < 0 || k > GM_FANOUT) bad |= GM_PL_ECOUNT;
    if (!self) bad |= GM_PL_ESELF;
    if (f == 0) {
      if (!ran) bad |= GM_PL_EHEARTBEAT;
      // age (t - 1) - (hb + 1) / 2 >= GM_VIEW_AGES: what gm_view_census rejects in a live observer's view
      if (x != 0 && (t - 1) - (int)((hb + 1u) >> 1) >= GM_VIEW_AGES) bad |= GM_PL_EAGE;
    } else {
      if ((hbc & 1) || hbc > top || hbc < 2) bad |= GM_PL_EHEARTBEAT;
      if (k > 0 && !ran) bad |= GM_PL_ECRASHED;  // a node that did not run tick t - 1 sent nothing
    }
  } else {
    bad = 0;
  }
  if (bad) atomicOr(status, bad);
}

// the sends of tick t - 1 to this context's own nodes, delivered at tick t
__global__ __launch_bounds__(256) void gm_pl_inbox(PState s, int t, uint32_t *status) {
  const int li = blockIdx.x * blockDim.x + threadIdx.x;
  if (li >= s.nloc) return;
  const int par = t & 1;
  const int k = min(s.rowstat[(size_t)li * 4 + 3], GM_FANOUT);
  for (int q = 0; q < k; q++) {
    const int d = s.targets[(size_t)li * GM_FANOUT + q] - s.n0;
    if (d < 0 || d >= s.nloc) continue;  // another row shard's node: the exchange delivers it
    int32_t *row = s.inbox[par] + (size_t)d * P_KMAX;
    const int slot = atomicAdd(row, 1);
    if (slot < s.kcap) row[1 + slot] = li;
    else atomicOr(status, GM_PL_EINBOX);
  }
}

// ------------------------------------------------------------ launch wrappers
hipError_t gm_launch_view_load_check(const PState &s, int t, int cnt, const uint64_t *stage, uint32_t *status,
                                     hipStream_t st) {
  if (cnt > 0) hipLaunchKernelGGL(gm_pl_check, dim3((cnt + 7) / 8), dim3(256), 0, st, s, t, cnt, stage, status);
  return hipGetLastError();
}

hipError_t gm_launch_view_load_store(const PState &s, int t, int r0, int cnt, const uint64_t *stage, uint32_t *given,
                                     hipStream_t st) {
  if (cnt > 0) hipLaunchKernelGGL(gm_pl_store, dim3((cnt + 7) / 8), dim3(256), 0, st, s, t, r0, cnt, stage, given);
  return hipGetLastError();
}

hipError_t gm_launch_view_load_nodes(const PState &s, int t, int r0, int cnt, const int32_t *heartbeat,
                                     const int32_t *failed, const int32_t *counts, const int32_t *targets,
                                     const uint32_t *given, uint32_t *status, int write, hipStream_t st) {
  if (cnt > 0)
    hipLaunchKernelGGL(gm_pl_nodes, dim3((cnt + 7) / 8), dim3(256), 0, st, s, t, r0, cnt, heartbeat, failed, counts,
                       targets, given, status, write);
  return hipGetLastError();
}

hipError_t gm_launch_view_load_inbox(const PState &s, int t, uint32_t *status, hipStream_t st) {
  hipLaunchKernelGGL(gm_pl_inbox, dim3((s.nloc + 255) / 256), dim3(256), 0, st, s, t, status);
  return hipGetLastError();
}
