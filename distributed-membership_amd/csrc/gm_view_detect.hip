// gm_view_detect.hip -- PARTIAL detection recorder (gm_view_detect_record): the per-tick reducer.
//
// A tick leaves on the device its final views (lists of parity t & 1, id-sorted), the join masks over
// them (ev_jm) and the TREMOVE removal records at the back of each event row (counts in ev_cnt); the
// next tick overwrites the masks and the records. While recording is on, gm_p_view_detect runs once
// per tick after the node kernels and folds them into one gm_view_detect_rec per subject of the
// cluster and one timeline row per tick. The tick kernels are not touched: the reducer reads what
// gm_drain_events would copy to the host, plus failed[] as the tick saw it and the recorder's own
// crash bitmap of the whole cluster (one bit per node, bit id - 1: n / 8 bytes, L2-resident).
//
//   lane mapping   as gm_vc_reduce (gm_view_census.hip): V lanes per view, 64 / V views per wave step,
//                  one 8-byte entry per lane loaded nontemporally, a batch of GM_VD_UNROLL steps in
//                  flight. The observers' crash flags, ev_cnt and ev_jm of a batch are one coalesced
//                  load each, issued a batch ahead and handed to the steps by shuffle; a frozen view
//                  is not loaded.
//   per entry      the subject's bit of the crash bitmap. Only a hit touches the records:
//                  atomicMax(last_held, t), one add to held_sum, one to late_joins when the entry's
//                  ev_jm bit is set -- all without a return value. The census' scatter over every
//                  entry shrinks to the entries naming a crashed subject (~1 % at S-C, fading to none;
//                  ~V holders per subject, so no address is hot at scale; many observers on one
//                  subject at small n are still exact: they are atomics).
//   per observer   ev_cnt >> 16 is rarely non-zero; its lanes then read the removal records from the
//                  back of the event row and update the subject's record as det_add (gm_detect.hip).
//   timeline       held and late joins by wave ballot and popcount, joins and removals per lane; one
//                  shuffle reduction per wave at the end, the waves' sums in LDS, one global add per
//                  workgroup and non-zero counter. No atomic per entry.
// Every id is range-checked before it indexes anything (GM_VD_E*); the host turns a status bit into
// GM_ESTATE.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "gm_abi.h"
#include "gm_device.h"
#include "gm_partial.h"

#define GM_VD_UNROLL 8     // wave steps in flight (fewer where 64 / V views per step make 8 steps exceed 64 views)
#define GM_VD_WAVES 32768  // waves of the launch at scale: several rounds of the resident ones (256 CUs x 24), 64 KB of lists each at S-C
#define GM_VD_EID 1u       // status word: a view entry's id is outside [1, n]
#define GM_VD_EREC 2u      //   a removal record is not a REMOVE of an id in [1, n]
#define GM_VD_ECNT 4u      //   more removal records than an event row holds

static_assert(sizeof(gm_view_detect_rec) == 48, "gm_view_detect_rec layout");
static_assert(GM_VIEW_DETECT_COLS == 5, "timeline columns: joins, removals, false removals, held, late joins");

__device__ __forceinline__ bool vd_crashed(const uint32_t *__restrict__ cls, uint32_t j) {
  return (cls[j >> 5] >> (j & 31u)) & 1u;
}

// lists: the views of parity t & 1, [nloc][V]; failed [nloc]: the observers' crash flags as tick t saw
// them; cls: one bit per subject of the cluster as tick t saw it; rec [n]; tl: the timeline row of
// tick t. spw: steps per wave, a multiple of the steps per batch.
__global__ __launch_bounds__(256) void gm_p_view_detect(const uint64_t *__restrict__ lists,
                                                        const int32_t *__restrict__ failed,
                                                        const uint32_t *__restrict__ ev,
                                                        const int32_t *__restrict__ ev_cnt,
                                                        const uint32_t *__restrict__ ev_jm,
                                                        const uint32_t *__restrict__ cls, gm_view_detect_rec *rec,
                                                        unsigned long long *tl, uint32_t *status, int n, int nloc,
                                                        int V, int t, int spw) {
  __shared__ uint32_t wsum[4][GM_VIEW_DETECT_COLS];
  const int tid = threadIdx.x, lane = tid & 63;
  const int vpw = 64 / V;                // views per wave step
  const int sub = lane / V, e = lane - sub * V;
  const bool on = sub < vpw;             // V not a divisor of 64: the last lanes idle
  const int64_t s0 = ((int64_t)blockIdx.x * 4 + (tid >> 6)) * spw;
  uint32_t tj = 0, tr = 0, tf = 0;       // this lane's share of joins, removals, false removals
  uint32_t th = 0, tlj = 0;              // the wave's held entries and late joins (uniform)
  uint32_t bad = 0;
  // what a batch of U steps needs per view -- crash flag, ev_cnt, ev_jm -- is one coalesced load each:
  // lane l takes view l of the batch (U * vpw <= 64), the steps fetch theirs by shuffle. The next
  // batch's are loaded while this one's entries are in flight, so a batch costs one round trip.
  const int U = min(GM_VD_UNROLL, 64 / vpw), bviews = U * vpw;
  int32_t ncnt = -1;    // the next batch: ev_cnt of view `lane`, -1 = no such view or a frozen one
  uint32_t njm = 0;
  auto fetch = [&](int64_t step) {  // three independent loads: none waits for the flag
    const int64_t v = step * vpw + lane;
    const bool in = lane < bviews && v < nloc;
    const int32_t f = in ? failed[v] : 1, c = in ? ev_cnt[v] : 0;
    njm = in ? ev_jm[v] : 0u;
    ncnt = f ? -1 : c;
  };
  fetch(s0);
  for (int k = 0; k < spw; k += U) {
    const int32_t ccnt = ncnt;
    const uint32_t cjm = njm;
    uint64_t x[GM_VD_UNROLL];
    int32_t cnt[GM_VD_UNROLL];
    uint32_t jm[GM_VD_UNROLL];
    const int64_t view0 = (s0 + k) * vpw + sub;  // this lane's view of step 0 of the batch, + vpw per step
#pragma unroll
    for (int u = 0; u < GM_VD_UNROLL; u++) {  // frozen views are skipped before their entries are loaded
      const int src = u * vpw + sub;            // (lanes past the last view read some other lane: not `on`)
      cnt[u] = __shfl(ccnt, src, 64);
      jm[u] = __shfl(cjm, src, 64);
      const bool live = u < U && on && cnt[u] >= 0;
      cnt[u] = live ? cnt[u] : 0;
      x[u] = live ? __builtin_nontemporal_load(lists + (view0 + u * vpw) * V + e) : 0ull;
    }
    if (k + U < spw) fetch(s0 + k + U);
#pragma unroll
    for (int u = 0; u < GM_VD_UNROLL; u++) {
      bool hit = false, late = false;
      if (x[u]) {
        const uint32_t id = (uint32_t)(x[u] >> 32);
        if (id < 1u || id > (uint32_t)n) {  // nothing of such an entry is used as an index
          bad |= GM_VD_EID;
        } else if (vd_crashed(cls, id - 1u)) {
          gm_view_detect_rec *d = rec + (id - 1u);
          hit = true;
          late = (jm[u] >> e) & 1u;
          atomicMax(&d->last_held, t);
          atomicAdd((unsigned long long *)&d->held_sum, 1ull);
          if (late) atomicAdd(&d->late_joins, 1u);
        }
      }
      th += (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(hit));
      tlj += (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(late));
      if (e == 0) tj += (uint32_t)cnt[u] & 0xFFFFu;
      const uint32_t nr = (uint32_t)cnt[u] >> 16;
      if (!nr) continue;
      if (nr > 2u * (uint32_t)V) {
        bad |= GM_VD_ECNT;
        continue;
      }
      const uint32_t *evr = ev + (size_t)(view0 + u * vpw) * 2 * V;
      for (uint32_t q = (uint32_t)e; q < nr; q += (uint32_t)V) {  // the removals, from the back of the row
        const uint32_t r = evr[2 * V - 1 - q], id = r & 0x3FFFFFFFu;
        if ((r >> 30) != P_EV_REMOVE || id < 1u || id > (uint32_t)n) {
          bad |= GM_VD_EREC;
          continue;
        }
        gm_view_detect_rec *d = rec + (id - 1u);
        const bool live_subject = !vd_crashed(cls, id - 1u);
        atomicAdd(&d->removals, 1u);
        if (live_subject) atomicAdd(&d->false_removals, 1u);
        atomicAdd((unsigned long long *)&d->removed_tick_sum, (unsigned long long)t);
        atomicMin((unsigned int *)&d->first_removed, (unsigned int)t);  // -1 (none yet) is the largest unsigned
        atomicMax(&d->last_removed, t);
        tr++;
        tf += live_subject ? 1u : 0u;
      }
    }
  }
  if (bad) atomicOr(status, bad);
  // the timeline row: per wave, per workgroup, then one add per counter
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    tj += __shfl_xor(tj, o, 64);
    tr += __shfl_xor(tr, o, 64);
    tf += __shfl_xor(tf, o, 64);
  }
  if (lane == 0) {
    uint32_t *w = wsum[tid >> 6];
    w[0] = tj;
    w[1] = tr;
    w[2] = tf;
    w[3] = th;
    w[4] = tlj;
  }
  __syncthreads();
  if (tid < GM_VIEW_DETECT_COLS) {
    const uint32_t v = wsum[0][tid] + wsum[1][tid] + wsum[2][tid] + wsum[3][tid];
    if (v) atomicAdd(tl + tid, (unsigned long long)v);
  }
}

// One recorded tick t of this context's observers: rec [s.n] and the timeline row tl_row
// [GM_VIEW_DETECT_COLS] are added to; cls is the crash bitmap of the whole cluster as tick t saw it.
hipError_t gm_launch_view_detect(const PState &s, const uint32_t *cls, gm_view_detect_rec *rec, uint64_t *tl_row,
                                 uint32_t *status, int t, hipStream_t st) {
  if (s.V < 2 || s.V > P_VMAX) return hipErrorInvalidValue;
  const int vpw = 64 / s.V;
  const int64_t steps = ((int64_t)s.nloc + vpw - 1) / vpw;
  int64_t spw = (steps + GM_VD_WAVES - 1) / GM_VD_WAVES;
  const int U = std::min(GM_VD_UNROLL, 64 / vpw);  // steps per batch, as the kernel derives it
  spw = std::max<int64_t>(U, (spw + U - 1) / U * U);
  const int64_t waves = (steps + spw - 1) / spw;
  const uint64_t *lists = s.lists + (size_t)(t & 1) * s.rows * s.V;
  hipLaunchKernelGGL(gm_p_view_detect, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, st, lists, s.failed, s.ev,
                     s.ev_cnt, s.ev_jm, cls, rec, (unsigned long long *)tl_row, status, s.n, s.nloc, s.V, t, (int)spw);
  return hipGetLastError();
}
