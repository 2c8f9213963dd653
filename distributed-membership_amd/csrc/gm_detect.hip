// gm_detect.hip -- SCALED detection recorder (gm_detect_record): the per-tick reducer.
//
// The band kernels leave one tick's join / removal records on the device -- per (row, band) the
// first `evs` in ev_band, the rest in the spill ring -- and the next tick overwrites them. While
// recording is on, gm_s_detect runs once per tick after the band kernels and folds the records
// into one gm_detect_rec per subject column and one timeline row per tick. The band kernels are
// not touched: the reducer reads what gm_drain_events would copy to the host (brec's S_BC_NEV,
// ev_band, ev_spill), plus failed[] as the tick saw it.
//
// Tiling: a workgroup takes one band and GM_DET_ROWS rows. A removal sweep names the same few
// subjects in every row (S-A's TREMOVE peak: 655 subjects x ~65 k loggers in two ticks), so a
// global atomic per record would serialise on a few hundred addresses (the escape pool's single
// counter cost 25 ms that way, gm_scaled.h). The workgroup counts into an LDS histogram over the
// band's columns instead and flushes each non-zero column with one add per field. The tick is the
// same for the whole launch, so first / last / tick sum follow from the count.
//
// Quiet ticks: the band kernel keeps the tick's record total in S_EV_STRIPES partial sums indexed
// (band * n + row) & (S_EV_STRIPES - 1). A workgroup whose rows' stripes are all zero holds no
// record and leaves before it reads brec (64 MB at S-A); a stripe shared with other rows can only
// keep a workgroup in, never let it skip records.
#include <hip/hip_runtime.h>

#include "gm_abi.h"
#include "gm_scaled.h"

#define GM_DET_ROWS 1024  // rows of one band per workgroup
#define GM_DET_BMAX 1024  // widest band

// joins / removals of one subject in tick t -> its record; live: failed[subject] was 0 in that tick
__device__ __forceinline__ void det_add(gm_detect_rec *d, uint32_t joins, uint32_t rem, bool live, int t) {
  if (joins) atomicAdd(&d->joins, joins);
  if (!rem) return;
  atomicAdd(&d->removals, rem);
  if (live) atomicAdd(&d->false_removals, rem);
  atomicAdd((unsigned long long *)&d->removed_tick_sum, (unsigned long long)rem * (unsigned long long)t);
  atomicMin((unsigned int *)&d->first_removed, (unsigned int)t);  // -1 (none yet) is the largest unsigned
  atomicMax(&d->last_removed, t);
}

// Grid (ceil(n / GM_DET_ROWS), nb + 1): y < nb the (row run, band) tiles, y = nb the spill ring.
// rec: [w] records of this shard's columns; tl: the timeline row of tick t (joins, removals, false).
__global__ __launch_bounds__(256) void gm_s_detect(SState s, gm_detect_rec *rec, unsigned long long *tl, int t) {
  __shared__ uint32_t hist[2 * GM_DET_BMAX];  // [kind - 1][column of the band]
  __shared__ uint16_t nevs[GM_DET_ROWS];      // records of each row held in its ev_band slots
  __shared__ uint32_t wsum[4][3];
  const int tid = threadIdx.x;
  uint32_t tj = 0, tr = 0, tf = 0;  // this thread's share of the timeline row
  if ((int)blockIdx.y < s.nb) {
    const int b = blockIdx.y, r0 = blockIdx.x * GM_DET_ROWS, rows = min(GM_DET_ROWS, s.n - r0);
    const size_t slab = (size_t)b * s.n;
    uint32_t any = 0;
    for (int i = tid; i < rows; i += 256) any |= s.ev_spill_cnt[1 + ((slab + r0 + i) & (S_EV_STRIPES - 1))];
    if (!__syncthreads_or(any != 0)) return;  // no record in these rows this tick
    for (int i = tid; i < s.band; i += 256) hist[i] = hist[GM_DET_BMAX + i] = 0;
    any = 0;
    for (int i = tid; i < rows; i += 256) {
      const uint32_t k = min(S_BC_NEV(s.brec[slab + r0 + i].z), (uint32_t)s.evs);
      nevs[i] = (uint16_t)k;
      any |= k;
    }
    if (!__syncthreads_or(any != 0)) return;  // the stripes were other rows'
    // (row, slot) flat over the run: a row's slots on adjacent lanes (evs = band / 32 is a power of two)
    const int lg = __ffs(s.evs) - 1, total = rows << lg;
    for (int j = tid; j < total; j += 256) {
      const int i = j >> lg, q = j & (s.evs - 1);
      if (q >= nevs[i]) continue;
      const uint32_t e = s.ev_band[((size_t)(r0 + i) * s.nb + b) * s.evs + q];
      const uint32_t kind = e >> 30;
      const int col = (int)(e & 0x3FFFFFFFu) - 1 - s.c0 - b * s.band;
      if ((kind == S_EV_ADD || kind == S_EV_REMOVE) && (unsigned)col < (unsigned)s.band)
        atomicAdd(&hist[(kind - 1) * GM_DET_BMAX + col], 1u);
    }
    __syncthreads();
    for (int col = tid; col < s.band; col += 256) {
      const uint32_t joins = hist[col], rem = hist[GM_DET_BMAX + col];
      const int lc = b * s.band + col;  // shard-local column
      if (!(joins | rem) || lc >= s.w) continue;
      const bool live = s.failed[s.c0 + lc] == 0;
      det_add(rec + lc, joins, rem, live, t);
      tj += joins;
      tr += rem;
      tf += live ? rem : 0u;
    }
  } else {
    // spilled records carry logger and subject and are few: global atomics directly
    const uint32_t ns = min(s.ev_spill_cnt[0], s.ev_spill_cap);
    for (uint32_t q = blockIdx.x * 256u + tid; q < ns; q += gridDim.x * 256u) {
      const uint32_t e = (uint32_t)s.ev_spill[q];
      const uint32_t kind = e >> 30;
      const int lc = (int)(e & 0x3FFFFFFFu) - 1 - s.c0;
      if ((kind != S_EV_ADD && kind != S_EV_REMOVE) || (unsigned)lc >= (unsigned)s.w) continue;
      const bool live = s.failed[s.c0 + lc] == 0;
      const uint32_t joins = kind == S_EV_ADD, rem = kind == S_EV_REMOVE;
      det_add(rec + lc, joins, rem, live, t);
      tj += joins;
      tr += rem;
      tf += live ? rem : 0u;
    }
  }
  // the timeline row: per wave, per workgroup, then one add per counter
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    tj += __shfl_xor(tj, o, 64);
    tr += __shfl_xor(tr, o, 64);
    tf += __shfl_xor(tf, o, 64);
  }
  if ((tid & 63) == 0) {
    wsum[tid >> 6][0] = tj;
    wsum[tid >> 6][1] = tr;
    wsum[tid >> 6][2] = tf;
  }
  __syncthreads();
  if (tid < 3) {
    const uint32_t v = wsum[0][tid] + wsum[1][tid] + wsum[2][tid] + wsum[3][tid];
    if (v) atomicAdd(tl + tid, (unsigned long long)v);
  }
}

hipError_t gm_launch_detect(const SState &s, gm_detect_rec *rec, uint64_t *timeline, int t, hipStream_t st) {
  const dim3 grid((s.n + GM_DET_ROWS - 1) / GM_DET_ROWS, s.nb + 1);
  hipLaunchKernelGGL(gm_s_detect, grid, dim3(256), 0, st, s, rec, (unsigned long long *)timeline + 3 * (size_t)t, t);
  return hipGetLastError();
}
