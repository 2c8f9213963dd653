// gm_band.hip -- the band sweep's general path: gm_s_band (every band width, keyed loss, the join
// ramp), gm_s_band_listed (the units gm_s_band_fast handed back), the join ramp's gm_s_selfcheck, and
// the band launcher, which picks between them and the fast path (gm_band_fast.hip).
#include "gm_band.h"

// One unit of the general path (every band width, keyed loss, the join ramp, and the units the
// fast path hands back).
// UNI: the grid's own unit (its row metadata in scalar registers); the listed pass loads its units'
// rows through vector registers.
template <int B, bool DROP, bool UNI>
__device__ __forceinline__ void band_unit(const SState &s, int t, int drop_pct, int band, int ub, uint32_t *lds) {
  UnitIn<B> in;
  unit_load<B, UNI>(s, t, band, ub, in);
  u32x2 m[S_SB];
  uint32_t ent;
  unit_gather<B, DROP>(s, t, in, m, ent);
  unit_finish<B, DROP>(s, t, drop_pct, in, m, ent, lds);
}

#ifndef GM_DROP_MINW
#define GM_DROP_MINW 8  // the keyed-loss instantiation at 8 waves per SIMD (64 VGPRs + 20 B of spills: 7.39 ms vs 7.63 at its own 79 VGPRs)
#endif
#ifndef GM_BAND_MINW
#define GM_BAND_MINW 1
#endif
// grid (units of a band / 4, bands): blockIdx.y is the band, so workgroups still dispatch
// band-major, and the wave-uniform unit index needs no division
// units [u0, u1) of every band: a row chunk of the column-sharded pipeline, or all of them
template <int B, bool DROP>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(DROP ? GM_DROP_MINW : GM_BAND_MINW, 8))) void gm_s_band(SState s, int t, int drop_pct, int u0, int u1) {
  constexpr int RPW = 64 / (B / S_COLS_PER_LANE);
  const int ub = __builtin_amdgcn_readfirstlane(u0 + (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6));
  if (ub >= u1) return;  // whole wave
  UnitIn<B> in;
  unit_load<B, RPW == 1>(s, t, (int)blockIdx.y, ub, in);
  u32x2 m[S_SB];
  uint32_t ent;
  unit_gather<B, DROP>(s, t, in, m, ent);
  __shared__ uint32_t lds_all[4 * S_LDS_WAVE_WORDS];  // escaped rows only (esc_apply / esc_emit)
  unit_finish<B, DROP>(s, t, drop_pct, in, m, ent, lds_all + (threadIdx.x >> 6) * S_LDS_WAVE_WORDS);
  if (ub == 0 && blockIdx.y == 0) band_reset_pools(s, t);
}

// The general path over the units gm_s_band_fast handed back this tick (s.fb_list): a fixed grid of
// waves striding over the list (rows through vector registers: the units come from memory).
// Only the units of rows [u0, u1) (one row per unit at B = 1024): the pipelined sharded tick runs it
// after each row chunk's fast pass, over the list so far.
template <int B>
__global__ __launch_bounds__(256) void gm_s_band_listed(SState s, int t, int u0, int u1) {
  __shared__ uint32_t lds_all[4 * S_LDS_WAVE_WORDS];
  uint32_t *lds = lds_all + (threadIdx.x >> 6) * S_LDS_WAVE_WORDS;
  const uint32_t cnt = s.fb_cnt[t & 1];
  const uint32_t nw = gridDim.x * 4;
  for (uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6); i < cnt; i += nw) {
    const int2 u = s.fb_list[i];
    const int ub = __builtin_amdgcn_readfirstlane(u.y);
    if (ub < u0 || ub >= u1) continue;
    band_unit<B, false, false>(s, t, -1, __builtin_amdgcn_readfirstlane(u.x), ub, lds);
  }
}

// the fast path and its kernel: one compile unit with the kernels above (see the file's header)
#include "gm_band_fast.hip"

// --------------------------------------------------------------- gm_s_selfcheck
// Join ramp: rows that appended their own entry this tick (updateMyPos found no self and no
// larger id of its start group). The reference appends only if NO larger id is present
// after the merge (lower_bound == end); a larger id of a later group would have taken the
// quirk path with a heartbeat the narrow cell cannot hold. Verify, one wave per row: no
// cell above the group is present after the sweep, none was removed by it (events).
__global__ __launch_bounds__(256) void gm_s_selfcheck(SState s) {
  const int lane = threadIdx.x & 63;
  const int nw = gridDim.x * 4;
  const uint32_t cnt = min(*s.selfadd_cnt, (uint32_t)S_SELFADD_CAP);
  for (uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6); i < cnt; i += nw) {
    const int r = s.selfadd[i];
    const int gend = (r | 3) - s.c0;  // last shard column of the row's start group
    const int b0 = (gend + 1) / s.band;
    bool bad = false;
    for (int b = b0 + 1 + lane; b < s.nb; b += 64) {  // whole bands above: nothing present, no events
      const uint32_t v = s.brec[(size_t)b * s.n + r].z;
      bad |= S_BC_PRES(v) != 0 || S_BC_NEV(v) != 0;
    }
    if (b0 < s.nb) {
      const uint8_t *cells = s.table + ((size_t)b0 * s.n + r) * s.band;
      for (int j = lane; j < s.band; j += 64)
        bad |= b0 * s.band + j > gend && cells[j] != 0;
      const uint32_t v = s.brec[(size_t)b0 * s.n + r].z;
      const int ne = min((int)S_BC_NEV(v), s.evs);
      const uint32_t *ev = s.ev_band + ((size_t)r * s.nb + b0) * s.evs;
      for (int q = lane; q < ne; q += 64) bad |= (int)(ev[q] & 0x3FFFFFFFu) - 1 - s.c0 > gend;
      if ((int)S_BC_NEV(v) > s.evs) {  // spilled records of this (row, band)
        const uint32_t ns = min(*s.ev_spill_cnt, s.ev_spill_cap);
        for (uint32_t q = lane; q < ns; q += 64) {
          const uint64_t e = s.ev_spill[q];
          bad |= (int)(e >> 32) == r && (int)((uint32_t)e & 0x3FFFFFFFu) - 1 - s.c0 > gend;
        }
      }
    }
    if (__ballot(bad) && lane == 0) atomicOr(s.err, GM_ERR_SELF);
  }
}

// ------------------------------------------------------------ launch wrappers
// the band kernels of rows [r0, r1) (r0, r1 multiples of the rows per unit, or r1 = n)
template <int B>
static void launch_band_b(const SState &s, int t, int drop_pct, int r0, int r1, hipStream_t st) {
  constexpr int RPW = 64 / (B / S_COLS_PER_LANE);
  const int u0 = r0 / RPW, u1 = (r1 + RPW - 1) / RPW;
  if (u1 <= u0) return;
  const dim3 nblk((u1 - u0 + 3) / 4, s.nb);  // (units of the chunk in a band / 4, bands)
  if (drop_pct >= 0) {
    hipLaunchKernelGGL((gm_s_band<B, true>), dim3(nblk), dim3(256), 0, st, s, t, drop_pct, u0, u1);
  } else if (B == 1024 && !s.ramp && s.fb_list) {  // the fast path, then the units it handed back
    // GM_FAST_XS stripes of q rows each (the kernel's row order); waves past u1 exit
    const int q = (u1 - u0 + GM_FAST_XS - 1) / GM_FAST_XS;
    const dim3 nblk2((GM_FAST_XS * q + GM_FAST_WG - 1) / GM_FAST_WG, (s.nb + GM_FAST_BPW - 1) / GM_FAST_BPW);
    if (u0 == 0 && r1 == s.n)
      hipLaunchKernelGGL((gm_s_band_fast<B == 1024 ? B : 1024, false, GM_FAST_BPW>), nblk2, dim3(64 * GM_FAST_WG), 0,
                         st, s, t, u0, u1);
    else
      hipLaunchKernelGGL((gm_s_band_fast<B == 1024 ? B : 1024, true, GM_FAST_BPW>), nblk2, dim3(64 * GM_FAST_WG), 0,
                         st, s, t, u0, u1);
    hipLaunchKernelGGL((gm_s_band_listed<B == 1024 ? B : 1024>), dim3(S_FB_BLOCKS), dim3(256), 0, st, s, t, u0, u1);
  } else {
    hipLaunchKernelGGL((gm_s_band<B, false>), dim3(nblk), dim3(256), 0, st, s, t, drop_pct, u0, u1);
  }
}

hipError_t gm_launch_band_rows(const SState &s, int t, int drop_pct, int r0, int r1, hipStream_t st) {
  return gm_band_dispatch(s.band, [&](auto b) {
    launch_band_b<decltype(b)::value>(s, t, drop_pct, r0, r1, st);
    return hipGetLastError();
  });
}

void gm_launch_selfcheck(const SState &s, hipStream_t st) {
  hipLaunchKernelGGL(gm_s_selfcheck, dim3(16), dim3(256), 0, st, s);
  (void)hipMemsetAsync(s.selfadd_cnt, 0, sizeof(uint32_t), st);
}
