// gm_view_census.hip -- PARTIAL view census (gm_view_census): what the views hold at tick T.
//
// One pass over the stored views of this context's live observers: per subject node of the cluster
// one gm_view_rec (holders, stale entries, heartbeat range and sum), the histogram of the entries
// by (subject's crash flag, age) and the histogram of the view sizes. The views stay on the device;
// 24 n bytes plus the two histograms go back (gm_host_read.hip gm_view_census). Nothing the tick kernels
// read is written: the reducer's only outputs are its own scratch.
//
// An entry's timestamp is derived from its heartbeat (ts = (hb + 1) / 2, gm_partial_node.h), so its age
// and its heartbeat lag are one number: lag = (2T - 1 - hb) / 2. Everything is accumulated in lag
// units and converted once per subject at the flush.
//
//   gm_vc_reduce  lane mapping as in the tick: V lanes per view, 64 / V views per wave step, one
//                 8-byte entry per lane (V = 32: a view is one coalesced 256-byte load), GM_VC_UNROLL
//                 steps in flight per wave. The observer's crash flag is read first; a frozen view is
//                 not loaded. The two histograms are counted in LDS (the age bins in GM_VC_COPIES
//                 copies: a warm cluster puts almost every entry into four or five bins; a lane adds
//                 to copy lane % copies, adjacent words, distinct banks) and flushed with one global
//                 add per non-zero counter. The per-subject part is a scatter to ids spread uniformly
//                 over all n, so it goes straight to a 16-byte device accumulator per subject with
//                 no-return atomics: one 64-bit add of 1 | lag << 32 (holders and the lag sum; both
//                 fit 32 bits: n < 2^25, lag < 32), one 32-bit OR of 1 << lag (the lags present: the
//                 minimum and the maximum), and one 32-bit add to the stale count where lag >= TFAIL.
//                 Every entry is checked before it indexes anything (GM_VC_E*).
//   gm_vc_flush   one thread per subject: the accumulator -> gm_view_rec.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "gm_abi.h"
#include "gm_device.h"
#include "gm_partial.h"

#define GM_VC_UNROLL 4     // wave steps in flight
#define GM_VC_COPIES 32    // LDS copies of an age bin
#define GM_VC_SCOPIES 8    // LDS copies of a view-size bin
#define GM_VC_WAVES 8192   // waves of the launch at scale (256 CUs x 8 workgroups x 4 waves)
#define GM_VC_EID 1u       // status word: an entry's id is outside [1, n]
#define GM_VC_EHB 2u       //   its heartbeat is even or above 2T - 1
#define GM_VC_EAGE 4u      //   its age is GM_VIEW_AGES or more

static_assert(GM_VIEW_AGES == 32, "the lags present are one 32-bit mask");
static_assert(GM_VIEW_SIZES == P_VMAX + 1, "view sizes 0..P_VMAX");
static_assert(sizeof(gm_view_rec) == 24, "gm_view_rec layout");

struct VcAcc {               // per subject, zeroed by a fill
  unsigned long long a;      // holders | lag sum << 32
  uint32_t stale;
  uint32_t lagmask;          // bit l: some holder's entry lags l ticks
};
static_assert(sizeof(VcAcc) == 16, "VcAcc layout");

// lists: the views of parity T & 1, [nloc][V]; failed [nloc]: the observers' crash flags; cls: one
// bit per subject of the cluster (bit id - 1 set: crashed). spw: steps per wave, a multiple of
// GM_VC_UNROLL.
__global__ __launch_bounds__(256) void gm_vc_reduce(const uint64_t *__restrict__ lists,
                                                    const int32_t *__restrict__ failed,
                                                    const uint32_t *__restrict__ cls, VcAcc *acc,
                                                    unsigned long long *hist, unsigned long long *sizes,
                                                    uint32_t *status, int n, int nloc, int V, int T, int spw) {
  __shared__ uint32_t lh[2 * GM_VIEW_AGES * GM_VC_COPIES];  // [class][lag][copy]
  __shared__ uint32_t ls[GM_VIEW_SIZES * GM_VC_SCOPIES];    // [size][copy]
  const int tid = threadIdx.x, lane = tid & 63;
  for (int i = tid; i < 2 * GM_VIEW_AGES * GM_VC_COPIES; i += 256) lh[i] = 0;
  for (int i = tid; i < GM_VIEW_SIZES * GM_VC_SCOPIES; i += 256) ls[i] = 0;
  __syncthreads();
  const int vpw = 64 / V;                // views per wave step
  const int sub = lane / V, e = lane - sub * V;
  const bool on = sub < vpw;             // V not a divisor of 64: the last lanes idle
  const uint64_t vmask = ((1ull << V) - 1) << (sub * V);  // the lanes of this lane's view (sub * V <= lane)
  const int64_t s0 = ((int64_t)blockIdx.x * 4 + (tid >> 6)) * spw;
  const int two_t1 = 2 * T - 1;
  uint32_t bad = 0;
  for (int k = 0; k < spw; k += GM_VC_UNROLL) {
    uint64_t x[GM_VC_UNROLL];
    bool live[GM_VC_UNROLL];
#pragma unroll
    for (int u = 0; u < GM_VC_UNROLL; u++) {  // frozen views are skipped before their entries are loaded
      const int64_t view = (s0 + k + u) * vpw + sub;
      live[u] = on && view < nloc && failed[view] == 0;
      x[u] = live[u] ? __builtin_nontemporal_load(lists + view * V + e) : 0ull;
    }
#pragma unroll
    for (int u = 0; u < GM_VC_UNROLL; u++) {
      const uint64_t held = __builtin_amdgcn_ballot_w64(x[u] != 0) & vmask;
      if (live[u] && e == 0) atomicAdd(&ls[__builtin_popcountll(held) * GM_VC_SCOPIES + (sub & (GM_VC_SCOPIES - 1))], 1u);
      if (!x[u]) continue;
      const uint32_t id = (uint32_t)(x[u] >> 32);
      const int64_t d = (int64_t)two_t1 - (int64_t)(int32_t)(uint32_t)x[u];  // 2 lag: even and >= 0 for an odd hb <= 2T - 1
      const uint32_t why = (id < 1u || id > (uint32_t)n) ? GM_VC_EID
                           : (d < 0 || (d & 1))          ? GM_VC_EHB
                           : d >= 2 * GM_VIEW_AGES       ? GM_VC_EAGE
                                                         : 0u;
      if (why) {  // nothing of such an entry is used as an index
        bad |= why;
        continue;
      }
      const uint32_t lag = (uint32_t)d >> 1, j = id - 1u;
      const uint32_t c = (cls[j >> 5] >> (j & 31u)) & 1u;
      atomicAdd(&lh[(c * GM_VIEW_AGES + lag) * GM_VC_COPIES + (lane & (GM_VC_COPIES - 1))], 1u);
      VcAcc *a = acc + j;
      atomicAdd(&a->a, 1ull | ((unsigned long long)lag << 32));
      atomicOr(&a->lagmask, 1u << lag);
      if (lag >= GM_TFAIL) atomicAdd(&a->stale, 1u);
    }
  }
  if (bad) atomicOr(status, bad);
  __syncthreads();
  for (int i = tid; i < 2 * GM_VIEW_AGES; i += 256) {
    uint32_t v = 0;
    for (int q = 0; q < GM_VC_COPIES; q++) v += lh[i * GM_VC_COPIES + q];
    if (v) atomicAdd(hist + i, (unsigned long long)v);
  }
  for (int i = tid; i < GM_VIEW_SIZES; i += 256) {
    uint32_t v = 0;
    for (int q = 0; q < GM_VC_SCOPIES; q++) v += ls[i * GM_VC_SCOPIES + q];
    if (v) atomicAdd(sizes + i, (unsigned long long)v);
  }
}

__global__ __launch_bounds__(256) void gm_vc_flush(const VcAcc *__restrict__ acc, gm_view_rec *rec, int n, int T) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const VcAcc v = acc[j];
  const uint32_t holders = (uint32_t)v.a;
  const int two_t1 = 2 * T - 1;
  gm_view_rec d;
  d.hb_min = d.hb_max = -1;
  if (v.lagmask) {
    d.hb_max = two_t1 - 2 * __builtin_ctz(v.lagmask);
    d.hb_min = two_t1 - 2 * (31 - __builtin_clz(v.lagmask));
  }
  d.holders = holders;
  d.stale = v.stale;
  d.hb_sum = (uint64_t)((long long)holders * two_t1 - 2ll * (long long)(v.a >> 32));
  rec[j] = d;
}

// acc [s.n], hist [2][GM_VIEW_AGES], sizes [GM_VIEW_SIZES] and status zeroed on st before; cls the
// crash bitmap of the whole cluster; rec [s.n] or nullptr (no flush)
hipError_t gm_launch_view_census(const PState &s, const uint32_t *cls, void *acc, gm_view_rec *rec, uint64_t *hist,
                                 uint64_t *sizes, uint32_t *status, int T, hipStream_t st) {
  if (s.V < 2 || s.V > P_VMAX) return hipErrorInvalidValue;
  const int vpw = 64 / s.V;
  const int64_t steps = ((int64_t)s.nloc + vpw - 1) / vpw;
  int64_t spw = (steps + GM_VC_WAVES - 1) / GM_VC_WAVES;
  spw = std::max<int64_t>(GM_VC_UNROLL, (spw + GM_VC_UNROLL - 1) / GM_VC_UNROLL * GM_VC_UNROLL);
  const int64_t waves = (steps + spw - 1) / spw;
  const uint64_t *lists = s.lists + (size_t)(T & 1) * s.rows * s.V;
  hipLaunchKernelGGL(gm_vc_reduce, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, st, lists, s.failed, cls,
                     (VcAcc *)acc, (unsigned long long *)hist, (unsigned long long *)sizes, status, s.n, s.nloc, s.V, T,
                     (int)spw);
  if (rec) hipLaunchKernelGGL(gm_vc_flush, dim3((s.n + 255) / 256), dim3(256), 0, st, (const VcAcc *)acc, rec, s.n, T);
  return hipGetLastError();
}
