// gm_view_reach_shard.hip -- PARTIAL view-graph reachability across row shards: the kernels of a walk
// whose nodes are spread over the members of a group (gm_host_view_reach.hip runs the levels and the
// exchange between them). gm_view_reach.hip has the single-context walk and the definition of the
// word arrays; what differs here is where a word lives.
//
// A member owns the nodes [n0, n0 + nloc): its views, their crash flags, and the slices seen, front and
// next [nloc] of the walk, indexed by local node. Words of other members' nodes pass through one
// cluster-wide array, wide [n], indexed by global node:
//
//   GM_REACH_IN   wide is the whole cluster's front: before the pass the members' front slices are
//                 gathered into every member's wide. gm_vrs_gather is gm_vr_gather over the member's own
//                 views -- V lanes per view, 64 / V views per wave step, frozen and saturated observers
//                 skipped before their entries load -- gathering wide[id - 1] and storing next[local].
//   GM_REACH_OUT  wide is the whole cluster's next: gm_vrs_scatter is gm_vr_scatter over the member's own
//                 views, proposing with one no-return 64-bit atomicOr per entry into wide[id - 1]. The
//                 `& ~seen` filter applies where the subject is the member's own node; a proposal to
//                 another member's node goes unfiltered (its seen word is not here) and is masked by that
//                 member's commit. After the pass slice q of every member's wide travels to member q.
//   gm_vrs_commit one thread per own node: the proposals -- next[local] (IN), or the own slice of wide
//                 OR-ed with the slices received from the other members (OUT) -- minus seen, 0 for a
//                 crashed node; seen |= new, front = new, the own proposal word cleared. Per-source
//                 counts as gm_vr_commit: one ballot per source bit, LDS, one atomic per block and source.
//   gm_vrs_seed   one lane per source: the owner of a live source sets its bit and counts[0][k] = 1.
//
// Every entry is checked against [1, n] before it indexes anything (GM_VRS_EID); such an entry is no edge.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "gm_abi.h"
#include "gm_device.h"
#include "gm_partial.h"

#define GM_VRS_UNROLL 4     // wave steps in flight
#define GM_VRS_WAVES 8192   // waves of a view pass at scale (256 CUs x 8 workgroups x 4 waves)

static_assert(GM_REACH_SOURCES == 64, "one bit of a 64-bit word per source, one lane of a wave per source");

typedef unsigned long long vrs_u64;

// src: global node indices. failed, seen, front: the member's slices.
__global__ __launch_bounds__(64) void gm_vrs_seed(const int32_t *__restrict__ src, const int32_t *__restrict__ failed,
                                                  vrs_u64 *seen, vrs_u64 *front, vrs_u64 *counts, int n0, int nloc,
                                                  int nsrc) {
  const int k = threadIdx.x;
  if (k >= nsrc) return;
  const int64_t s = (int64_t)src[k] - n0;
  if (s < 0 || s >= nloc || failed[s] != 0) return;  // another member's node, or a crashed source
  atomicOr(seen + s, 1ull << k);                     // a node may be named twice
  atomicOr(front + s, 1ull << k);
  counts[k] = 1;
}

// lists: the member's views of parity T & 1, [nloc][V]. wide: the cluster's front [n]. full: the bits of
// the live sources. spw: steps per wave, a multiple of GM_VRS_UNROLL.
__global__ __launch_bounds__(256) void gm_vrs_gather(const uint64_t *__restrict__ lists,
                                                     const int32_t *__restrict__ failed,
                                                     const vrs_u64 *__restrict__ seen,
                                                     const vrs_u64 *__restrict__ wide, vrs_u64 *next,
                                                     uint32_t *status, vrs_u64 full, int n, int nloc, int V,
                                                     int spw) {
  const int lane = threadIdx.x & 63;
  const int vpw = 64 / V;  // views per wave step
  const int sub = lane / V, e = lane - sub * V;
  const bool on = sub < vpw;  // V not a divisor of 64: the last lanes idle
  const int64_t s0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * spw;
  bool bad = false;
  for (int k = 0; k < spw; k += GM_VRS_UNROLL) {
    uint64_t x[GM_VRS_UNROLL];
    vrs_u64 have[GM_VRS_UNROLL], g[GM_VRS_UNROLL];
    bool want[GM_VRS_UNROLL];
#pragma unroll
    for (int u = 0; u < GM_VRS_UNROLL; u++) {  // frozen and saturated views are skipped before their entries are loaded
      const int64_t view = (s0 + k + u) * vpw + sub;
      want[u] = on && view < nloc && failed[view] == 0;
      have[u] = want[u] ? seen[view] : full;
      want[u] = want[u] && (have[u] & full) != full;
      x[u] = want[u] ? __builtin_nontemporal_load(lists + view * V + e) : 0ull;
    }
#pragma unroll
    for (int u = 0; u < GM_VRS_UNROLL; u++) {
      g[u] = 0;
      if (!x[u]) continue;
      const uint32_t id = (uint32_t)(x[u] >> 32);
      if (id < 1u || id > (uint32_t)n) bad = true;  // nothing of such an entry is used as an index
      else g[u] = wide[id - 1u];
    }
#pragma unroll
    for (int u = 0; u < GM_VRS_UNROLL; u++) {
      const int64_t view = (s0 + k + u) * vpw + sub;
      vrs_u64 v = g[u];
      // the view's lanes e .. V - 1 OR-ed into lane e: a shuffle tree that stops at the view's end
      for (int d = 1; d < V; d <<= 1) {
        const vrs_u64 o = (vrs_u64)__shfl_down((long long)v, d, 64);
        if (e + d < V) v |= o;
      }
      v &= ~have[u];
      if (want[u] && e == 0 && v) next[view] = v;
    }
  }
  if (bad) atomicOr(status, GM_VRS_EID);
}

// wide: the cluster's next [n], zero before the pass. seen, front: the member's slices.
__global__ __launch_bounds__(256) void gm_vrs_scatter(const uint64_t *__restrict__ lists,
                                                      const vrs_u64 *__restrict__ seen,
                                                      const vrs_u64 *__restrict__ front, vrs_u64 *wide,
                                                      uint32_t *status, int n, int n0, int nloc, int V, int spw) {
  const int lane = threadIdx.x & 63;
  const int vpw = 64 / V;
  const int sub = lane / V, e = lane - sub * V;
  const bool on = sub < vpw;
  const int64_t s0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * spw;
  bool bad = false;
  for (int k = 0; k < spw; k += GM_VRS_UNROLL) {
    uint64_t x[GM_VRS_UNROLL];
    vrs_u64 f[GM_VRS_UNROLL], sj[GM_VRS_UNROLL];
#pragma unroll
    for (int u = 0; u < GM_VRS_UNROLL; u++) {  // only the last level's nodes load their view
      const int64_t view = (s0 + k + u) * vpw + sub;
      f[u] = on && view < nloc ? front[view] : 0ull;
      x[u] = f[u] ? __builtin_nontemporal_load(lists + view * V + e) : 0ull;
    }
#pragma unroll
    for (int u = 0; u < GM_VRS_UNROLL; u++) {
      sj[u] = ~0ull;
      if (!x[u]) continue;
      const uint32_t id = (uint32_t)(x[u] >> 32);
      if (id < 1u || id > (uint32_t)n) {
        bad = true;
      } else {
        const int64_t j = (int64_t)id - 1 - n0;  // an own subject is filtered here, another member's by its commit
        sj[u] = j >= 0 && j < nloc ? seen[j] : 0ull;
      }
    }
#pragma unroll
    for (int u = 0; u < GM_VRS_UNROLL; u++) {
      const vrs_u64 add = f[u] & ~sj[u];  // the node's own entry adds nothing: front is part of seen
      if (add) atomicOr(wide + ((uint32_t)(x[u] >> 32) - 1u), add);
    }
  }
  if (bad) atomicOr(status, GM_VRS_EID);
}

// prop: the member's own proposal words [nloc] (IN: next; OUT: its slice of wide). recv: nrecv slices
// [nloc] received from the other members (OUT), OR-ed in. row: counts[h], GM_REACH_SOURCES words.
__global__ __launch_bounds__(256) void gm_vrs_commit(const int32_t *__restrict__ failed, vrs_u64 *seen, vrs_u64 *front,
                                                     vrs_u64 *prop, const vrs_u64 *__restrict__ recv, int nrecv,
                                                     vrs_u64 *row, int nloc, int nsrc) {
  __shared__ uint32_t cnt[GM_REACH_SOURCES];
  const int tid = threadIdx.x, lane = tid & 63;
  if (tid < GM_REACH_SOURCES) cnt[tid] = 0;
  __syncthreads();
  const int x = blockIdx.x * 256 + tid;
  vrs_u64 nw = 0;
  if (x < nloc) {
    const vrs_u64 own = prop[x], fr = front[x];
    vrs_u64 nx = own;
    for (int q = 0; q < nrecv; q++) nx |= recv[(size_t)q * nloc + x];
    if (own) prop[x] = 0;
    if (nx && failed[x] == 0) {
      const vrs_u64 sn = seen[x];
      nw = nx & ~sn;
      if (nw) seen[x] = sn | nw;
    }
    if (fr != nw) front[x] = nw;
  }
  if (__builtin_amdgcn_ballot_w64(nw != 0)) {  // whole wave
    uint32_t mine = 0;
    for (int k = 0; k < nsrc; k++) {
      const uint32_t c = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64((nw >> k) & 1ull));
      if (lane == k) mine = c;
    }
    if (mine) atomicAdd(&cnt[lane], mine);
  }
  __syncthreads();
  if (tid < GM_REACH_SOURCES && cnt[tid]) atomicAdd(row + tid, (vrs_u64)cnt[tid]);
}

// steps per wave so that about GM_VRS_WAVES waves cover the views, a multiple of GM_VRS_UNROLL
static int vrs_spw(int64_t steps) {
  const int64_t spw = (steps + GM_VRS_WAVES - 1) / GM_VRS_WAVES;
  return (int)std::max<int64_t>(GM_VRS_UNROLL, (spw + GM_VRS_UNROLL - 1) / GM_VRS_UNROLL * GM_VRS_UNROLL);
}

static bool vrs_member_ok(const PState &s) {
  return s.V >= 2 && s.V <= P_VMAX && s.nloc >= 1 && s.n0 >= 0 && (int64_t)s.n0 + s.nloc <= s.n &&
         s.rows >= s.nloc;
}

// seen, front [s.nloc] and counts [GM_VIEW_HOPS][GM_REACH_SOURCES] zeroed on st before; src [nsrc] global
// node indices in [0, s.n)
hipError_t gm_launch_view_reach_shard_seed(const PState &s, const int32_t *src, int nsrc, uint64_t *seen,
                                           uint64_t *front, uint64_t *counts, hipStream_t st) {
  if (!vrs_member_ok(s) || nsrc < 1 || nsrc > GM_REACH_SOURCES) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gm_vrs_seed, dim3(1), dim3(64), 0, st, src, s.failed, (vrs_u64 *)seen, (vrs_u64 *)front,
                     (vrs_u64 *)counts, s.n0, s.nloc, nsrc);
  return hipGetLastError();
}

// The view pass of level h over the member's own views. IN: wide [s.n] holds the cluster's front, the
// pass writes next [s.nloc]. OUT: wide is zero, the pass proposes into it.
hipError_t gm_launch_view_reach_shard_pass(const PState &s, int T, int dir, uint64_t full, const uint64_t *seen,
                                           const uint64_t *front, uint64_t *next, uint64_t *wide, uint32_t *status,
                                           hipStream_t st) {
  if (!vrs_member_ok(s)) return hipErrorInvalidValue;
  const int vpw = 64 / s.V;
  const int64_t steps = ((int64_t)s.nloc + vpw - 1) / vpw;
  const int spw = vrs_spw(steps);
  const int64_t waves = (steps + spw - 1) / spw;
  const uint64_t *lists = s.lists + (size_t)(T & 1) * s.rows * s.V;
  const dim3 grid((unsigned)((waves + 3) / 4));
  if (dir == GM_REACH_IN)
    hipLaunchKernelGGL(gm_vrs_gather, grid, dim3(256), 0, st, lists, s.failed, (const vrs_u64 *)seen,
                       (const vrs_u64 *)wide, (vrs_u64 *)next, status, (vrs_u64)full, s.n, s.nloc, s.V, spw);
  else
    hipLaunchKernelGGL(gm_vrs_scatter, grid, dim3(256), 0, st, lists, (const vrs_u64 *)seen, (const vrs_u64 *)front,
                       (vrs_u64 *)wide, status, s.n, s.n0, s.nloc, s.V, spw);
  return hipGetLastError();
}

// The commit of level h (1 <= h < GM_VIEW_HOPS): prop [s.nloc] and the nrecv received slices, see
// gm_vrs_commit; the level's counts are added to counts[h].
hipError_t gm_launch_view_reach_shard_commit(const PState &s, int h, int nsrc, uint64_t *seen, uint64_t *front,
                                             uint64_t *prop, const uint64_t *recv, int nrecv, uint64_t *counts,
                                             hipStream_t st) {
  if (!vrs_member_ok(s) || h < 1 || h >= GM_VIEW_HOPS || nrecv < 0 || (nrecv > 0 && !recv))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(gm_vrs_commit, dim3((s.nloc + 255) / 256), dim3(256), 0, st, s.failed, (vrs_u64 *)seen,
                     (vrs_u64 *)front, (vrs_u64 *)prop, (const vrs_u64 *)recv, nrecv,
                     (vrs_u64 *)counts + (size_t)h * GM_REACH_SOURCES, s.nloc, nsrc);
  return hipGetLastError();
}
