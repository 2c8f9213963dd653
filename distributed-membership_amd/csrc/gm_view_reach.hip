// gm_view_reach.hip -- PARTIAL view-graph reachability (gm_view_reach): who hears from a node, and whom it hears.
//
// The view graph G_T of include/gm_abi.h: the live nodes, and an edge i -> j where the stored view of
// i names j. Up to 64 sources are walked at once, breadth first, one bit of a 64-bit word per source
// and node. The walk keeps three word arrays on the device -- seen (every level so far), front (the
// last level), next (what a hop proposes) -- and one row of per-source counts per level. A hop is two
// launches on the context's stream, ordered by the kernel boundary; the host reads the hop's row of
// counts and stops at an empty level (gm_host_read.hip gm_view_reach). Nothing a tick reads is
// written: the kernels' only outputs are this scratch.
//
//   gm_vr_seed     one lane per source: a live source gets its bit in seen and front, counts[0][k] = 1
//   gm_vr_gather   GM_REACH_IN, d(x) = the path x -> s: a node joins a source's level when its own view
//                  names a node of the last one. gm_vc_reduce's lane mapping: V lanes per view, 64 / V
//                  views per wave step, GM_VR_UNROLL steps in flight. The observer's crash flag and its
//                  seen word are read first: a frozen view, and one whose observer already holds every
//                  live source's bit, is not loaded, so the traffic shrinks as the walk saturates. A
//                  lane loads its entry, checks the id and gathers the 8-byte front word of its subject
//                  (a crashed subject never carries a bit: no crash lookup of subjects). The view's
//                  lanes are OR-ed by a shuffle tree that stops at the view's end, and one lane stores
//                  next[o]. No atomics.
//   gm_vr_scatter  GM_REACH_OUT, d(x) = the path s -> x: a node of the last level proposes its bits to
//                  every node its view names. Only observers with a non-zero front word load their view;
//                  a lane gathers seen[j] of its subject and issues one no-return 64-bit atomicOr on
//                  next[j] where the subject lacks a bit. Crashed subjects are not looked up here: the
//                  commit drops what was proposed to them, so they never enter seen or front.
//   gm_vr_commit   one thread per node: new = next & ~seen (0 for a crashed node), seen |= new, front =
//                  new, next = 0. The level's per-source counts are bit-sliced: per wave one ballot per
//                  source bit, skipped when the wave has no new bit, added up per block in LDS, then one
//                  64-bit atomic add per block and source with a non-zero count into counts[h].
//
// Every entry is checked before it indexes anything (GM_VR_EID); such an entry is no edge.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "gm_abi.h"
#include "gm_device.h"
#include "gm_partial.h"

#define GM_VR_UNROLL 4     // wave steps in flight
#define GM_VR_WAVES 8192   // waves of a view pass at scale (256 CUs x 8 workgroups x 4 waves)
#define GM_VR_EID 1u       // status word: an entry's id is outside [1, n]

static_assert(GM_REACH_SOURCES == 64, "one bit of a 64-bit word per source, one lane of a wave per source");

typedef unsigned long long vr_u64;

__global__ __launch_bounds__(64) void gm_vr_seed(const int32_t *__restrict__ src, const int32_t *__restrict__ failed,
                                                 vr_u64 *seen, vr_u64 *front, vr_u64 *counts, int n, int nsrc) {
  const int k = threadIdx.x;
  if (k >= nsrc) return;
  const int s = src[k];
  if (s < 0 || s >= n || failed[s] != 0) return;  // the host has checked the range
  atomicOr(seen + s, 1ull << k);                  // a node may be named twice
  atomicOr(front + s, 1ull << k);
  counts[k] = 1;
}

// lists: the views of parity T & 1, [n][V]. full: the bits of the live sources. spw: steps per wave, a
// multiple of GM_VR_UNROLL.
__global__ __launch_bounds__(256) void gm_vr_gather(const uint64_t *__restrict__ lists,
                                                    const int32_t *__restrict__ failed,
                                                    const vr_u64 *__restrict__ seen,
                                                    const vr_u64 *__restrict__ front, vr_u64 *next,
                                                    uint32_t *status, vr_u64 full, int n, int V, int spw) {
  const int lane = threadIdx.x & 63;
  const int vpw = 64 / V;  // views per wave step
  const int sub = lane / V, e = lane - sub * V;
  const bool on = sub < vpw;  // V not a divisor of 64: the last lanes idle
  const int64_t s0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * spw;
  bool bad = false;
  for (int k = 0; k < spw; k += GM_VR_UNROLL) {
    uint64_t x[GM_VR_UNROLL];
    vr_u64 have[GM_VR_UNROLL], g[GM_VR_UNROLL];
    bool want[GM_VR_UNROLL];
#pragma unroll
    for (int u = 0; u < GM_VR_UNROLL; u++) {  // frozen and saturated views are skipped before their entries are loaded
      const int64_t view = (s0 + k + u) * vpw + sub;
      want[u] = on && view < n && failed[view] == 0;
      have[u] = want[u] ? seen[view] : full;
      want[u] = want[u] && (have[u] & full) != full;
      x[u] = want[u] ? __builtin_nontemporal_load(lists + view * V + e) : 0ull;
    }
#pragma unroll
    for (int u = 0; u < GM_VR_UNROLL; u++) {
      g[u] = 0;
      if (!x[u]) continue;
      const uint32_t id = (uint32_t)(x[u] >> 32);
      if (id < 1u || id > (uint32_t)n) bad = true;  // nothing of such an entry is used as an index
      else g[u] = front[id - 1u];
    }
#pragma unroll
    for (int u = 0; u < GM_VR_UNROLL; u++) {
      const int64_t view = (s0 + k + u) * vpw + sub;
      vr_u64 v = g[u];
      // the view's lanes e .. V - 1 OR-ed into lane e: a shuffle tree that stops at the view's end
      for (int d = 1; d < V; d <<= 1) {
        const vr_u64 o = (vr_u64)__shfl_down((long long)v, d, 64);
        if (e + d < V) v |= o;
      }
      v &= ~have[u];
      if (want[u] && e == 0 && v) next[view] = v;
    }
  }
  if (bad) atomicOr(status, GM_VR_EID);
}

__global__ __launch_bounds__(256) void gm_vr_scatter(const uint64_t *__restrict__ lists,
                                                     const vr_u64 *__restrict__ seen,
                                                     const vr_u64 *__restrict__ front, vr_u64 *next,
                                                     uint32_t *status, int n, int V, int spw) {
  const int lane = threadIdx.x & 63;
  const int vpw = 64 / V;
  const int sub = lane / V, e = lane - sub * V;
  const bool on = sub < vpw;
  const int64_t s0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * spw;
  bool bad = false;
  for (int k = 0; k < spw; k += GM_VR_UNROLL) {
    uint64_t x[GM_VR_UNROLL];
    vr_u64 f[GM_VR_UNROLL], sj[GM_VR_UNROLL];
#pragma unroll
    for (int u = 0; u < GM_VR_UNROLL; u++) {  // only the last level's nodes load their view
      const int64_t view = (s0 + k + u) * vpw + sub;
      f[u] = on && view < n ? front[view] : 0ull;
      x[u] = f[u] ? __builtin_nontemporal_load(lists + view * V + e) : 0ull;
    }
#pragma unroll
    for (int u = 0; u < GM_VR_UNROLL; u++) {
      sj[u] = ~0ull;
      if (!x[u]) continue;
      const uint32_t id = (uint32_t)(x[u] >> 32);
      if (id < 1u || id > (uint32_t)n) bad = true;
      else sj[u] = seen[id - 1u];
    }
#pragma unroll
    for (int u = 0; u < GM_VR_UNROLL; u++) {
      const vr_u64 add = f[u] & ~sj[u];  // the node's own entry adds nothing: front is part of seen
      if (add) atomicOr(next + ((uint32_t)(x[u] >> 32) - 1u), add);
    }
  }
  if (bad) atomicOr(status, GM_VR_EID);
}

// row: counts[h], GM_REACH_SOURCES words
__global__ __launch_bounds__(256) void gm_vr_commit(const int32_t *__restrict__ failed, vr_u64 *seen, vr_u64 *front,
                                                    vr_u64 *next, vr_u64 *row, int n, int nsrc) {
  __shared__ uint32_t cnt[GM_REACH_SOURCES];
  const int tid = threadIdx.x, lane = tid & 63;
  if (tid < GM_REACH_SOURCES) cnt[tid] = 0;
  __syncthreads();
  const int x = blockIdx.x * 256 + tid;
  vr_u64 nw = 0;
  if (x < n) {
    const vr_u64 nx = next[x], fr = front[x];
    if (nx) {
      next[x] = 0;
      if (failed[x] == 0) {
        const vr_u64 sn = seen[x];
        nw = nx & ~sn;
        if (nw) seen[x] = sn | nw;
      }
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
  if (tid < GM_REACH_SOURCES && cnt[tid]) atomicAdd(row + tid, (vr_u64)cnt[tid]);
}

// steps per wave so that about GM_VR_WAVES waves cover the views, a multiple of GM_VR_UNROLL
static int vr_spw(int64_t steps) {
  const int64_t spw = (steps + GM_VR_WAVES - 1) / GM_VR_WAVES;
  return (int)std::max<int64_t>(GM_VR_UNROLL, (spw + GM_VR_UNROLL - 1) / GM_VR_UNROLL * GM_VR_UNROLL);
}

// seen, front, next [s.n], counts [GM_VIEW_HOPS][GM_REACH_SOURCES] and status zeroed on st before; src
// [nsrc] node indices in [0, s.n). One context holding the whole cluster (s.nloc == s.n).
hipError_t gm_launch_view_reach_seed(const PState &s, const int32_t *src, int nsrc, uint64_t *seen, uint64_t *front,
                                     uint64_t *counts, hipStream_t st) {
  if (s.nloc != s.n || nsrc < 1 || nsrc > GM_REACH_SOURCES) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gm_vr_seed, dim3(1), dim3(64), 0, st, src, s.failed, (vr_u64 *)seen, (vr_u64 *)front,
                     (vr_u64 *)counts, s.n, nsrc);
  return hipGetLastError();
}

// Level h (1 <= h < GM_VIEW_HOPS) of the walk from level h - 1: the view pass of the direction, then the
// commit, which adds the level's counts to counts[h]. full: the bits of the live sources.
hipError_t gm_launch_view_reach_hop(const PState &s, int T, int dir, int h, int nsrc, uint64_t full, uint64_t *seen,
                                    uint64_t *front, uint64_t *next, uint64_t *counts, uint32_t *status,
                                    hipStream_t st) {
  if (s.V < 2 || s.V > P_VMAX || s.nloc != s.n || h < 1 || h >= GM_VIEW_HOPS) return hipErrorInvalidValue;
  const int vpw = 64 / s.V;
  const int64_t steps = ((int64_t)s.n + vpw - 1) / vpw;
  const int spw = vr_spw(steps);
  const int64_t waves = (steps + spw - 1) / spw;
  const uint64_t *lists = s.lists + (size_t)(T & 1) * s.rows * s.V;
  const dim3 grid((unsigned)((waves + 3) / 4));
  if (dir == GM_REACH_IN)
    hipLaunchKernelGGL(gm_vr_gather, grid, dim3(256), 0, st, lists, s.failed, (const vr_u64 *)seen,
                       (const vr_u64 *)front, (vr_u64 *)next, status, (vr_u64)full, s.n, s.V, spw);
  else
    hipLaunchKernelGGL(gm_vr_scatter, grid, dim3(256), 0, st, lists, (const vr_u64 *)seen, (const vr_u64 *)front,
                       (vr_u64 *)next, status, s.n, s.V, spw);
  hipLaunchKernelGGL(gm_vr_commit, dim3((s.n + 255) / 256), dim3(256), 0, st, s.failed, (vr_u64 *)seen,
                     (vr_u64 *)front, (vr_u64 *)next, (vr_u64 *)counts + (size_t)h * GM_REACH_SOURCES, s.n, nsrc);
  return hipGetLastError();
}
