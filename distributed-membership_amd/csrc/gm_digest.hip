// gm_digest.hip -- layout-independent digests of the state between two ticks (gm_digest, the recorder).
//
// The definition is include/gm_abi.h's (GM_DIGEST_VERSION 1): one 64-bit word per observer row, a sum
// over the row's present entries of cell(c, hb, ts) = mix(mix(KCOL ^ c) ^ (hb << 32 | ts)); one word per
// node over its flags, heartbeat counter and last targets; two sums of fold(r, word) for the context.
// Everything is a sum mod 2^64, so bands, lists, column shards and row shards combine by addition and the
// stored form (band width, bytes against escape entries, fast or general path) drops out. Nothing a
// tick reads is written: the outputs are the caller's word arrays, sums and status word.
//
//   gm_dg_bytes   SCALED, the stored bytes: gm_r_decode's work split. One wave stays in one band and
//                 walks a run of rows; a lane owns 16 columns of the band (four dwords of a row's piece,
//                 each load contiguous over the row's LPR = B / 16 lanes), so the 16 column keys
//                 mix(KCOL ^ c) are paid once per wave and stay in registers. Per row the base tick is
//                 wtick[r] (a crashed row carries the tick it last ran: its frozen table is state);
//                 per cell hb = 2 wt - 255 + h - s_hbase(c), ts = wt - age, one mix. The row's lanes
//                 are summed on DPP (quad_perm, row_half_mirror, row_mirror; two swizzles above 16
//                 lanes) and one lane adds the piece's sum to rows[r] with a no-return 64-bit atomic.
//                 Escape bytes hold no value: they are counted per piece and compared with the
//                 piece's list word (S_EW_TOT), as gm_c_bytes does. Padding columns add nothing.
//   gm_dg_esc     SCALED, the escape lists of parity T & 1, shaped as gm_c_esc: 16 lanes per (band, row)
//                 list, the inline slot then the pool, a tile without any list returns at once. An
//                 entry's key depends on its column, so it pays two mixes. The list's lanes are one
//                 DPP row; one atomic add per list. The list's extent and every entry are checked
//                 before they are used (the checks of gm_c_esc).
//   gm_dg_nodes   SCALED, one thread per node: the four words of gm_read_nodes, rowstat[.][3] and the
//                 targets below that count. A column shard writes 0 outside its own columns.
//   gm_dg_views   PARTIAL: gm_vc_reduce's lane mapping, V lanes per view, 64 / V views per wave step,
//                 GM_DG_UNROLL steps in flight. A frozen (crashed) observer's view is digested. Two
//                 mixes per entry, a segmented shuffle tree over the view's lanes (V need not be a
//                 power of two), one plain store per view. The view's first lane also writes the
//                 node word.
//   gm_dg_fold    fold(r, .) over both arrays: a block reduction, one 64-bit atomic per block and sum.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "gm_abi.h"
#include "gm_device.h"
#include "gm_digest.h"

#define GM_DG_KCOL 0x6D656D6265727368ull
#define GM_DG_KNODE 0x6E6F646573746174ull
#define GM_DG_KROW 0x726F77666F6C6421ull
#define GM_DG_UNROLL 2       // rows (SCALED) / view steps (PARTIAL) a lane has in flight
#define GM_DG_WAVES 8192     // waves of a streaming launch at scale (256 CUs x 8 workgroups x 4 waves)
#define GM_DG_RUN_MAX 4096   // gm_dg_esc: rows of one band per workgroup, at most
#define GM_DG_RUN_MIN 256

static_assert(GM_DIGEST_VERSION == 1, "the kernels implement version 1 of the definition");

typedef unsigned long long dg_u64;

__device__ __forceinline__ uint64_t dg_cell(uint64_t kcol, int hb, int ts) {
  return gm_mix64(kcol ^ (((uint64_t)(uint32_t)hb << 32) | (uint32_t)ts));
}

// a DPP move of a 64-bit value (both halves, the same control); every source lane is active
template <int CTRL>
__device__ __forceinline__ uint64_t dg_dpp(uint64_t v) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)v, CTRL, 0xF, 0xF, false);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(v >> 32), CTRL, 0xF, 0xF, false);
  return ((uint64_t)hi << 32) | lo;
}
// the sum over each aligned group of W lanes, in every lane of the group (W a power of two <= 64)
template <int W>
__device__ __forceinline__ uint64_t dg_group_sum(uint64_t v) {
  if (W >= 2) v += dg_dpp<0xB1>(v);   // quad_perm [1, 0, 3, 2]
  if (W >= 4) v += dg_dpp<0x4E>(v);   // quad_perm [2, 3, 0, 1]
  if (W >= 8) v += dg_dpp<0x141>(v);  // row_half_mirror
  if (W >= 16) v += dg_dpp<0x140>(v); // row_mirror
  if (W >= 32) v += (uint64_t)__shfl_xor((long long)v, 16, 64);
  if (W >= 64) v += (uint64_t)__shfl_xor((long long)v, 32, 64);
  return v;
}

// ------------------------------------------------------------------ SCALED: the stored bytes
// Grid (workgroups of 4 waves, nb). spw: steps (of RPW rows) per wave, a multiple of GM_DG_UNROLL.
template <int B>
__global__ __launch_bounds__(256) void gm_dg_bytes(SState s, dg_u64 *rows, uint32_t *status, int spw) {
  constexpr int LPR = B / S_COLS_PER_LANE, RPW = 64 / LPR, Q = S_COLS_PER_LANE;
  const int lane = threadIdx.x & 63, sub = lane / LPR, li = lane % LPR;
  const int band = blockIdx.y;
  const size_t slab = (size_t)band * s.n;
  const int64_t step0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * spw;
  if (step0 * RPW >= s.n) return;  // whole wave
  // cell q = 4 k + j of the lane is column 4 (k LPR + li) + j of the band (gm_r_decode's mapping)
  uint64_t kc[Q];
  int hoff[Q];
  uint32_t real = 0;
#pragma unroll
  for (int q = 0; q < Q; q++) {
    const int lc = band * B + 4 * ((q >> 2) * LPR + li) + (q & 3);
    kc[q] = gm_mix64(GM_DG_KCOL ^ (uint64_t)(s.c0 + lc));
    hoff[q] = -255 - s_hbase(s.ramp, s.c0 + lc);
    real |= (lc < s.w ? 1u : 0u) << q;
  }
  bool bad = false;
  for (int k = 0; k < spw; k += GM_DG_UNROLL) {
    uint32_t tw[GM_DG_UNROLL][4], ew[GM_DG_UNROLL];
    int wt[GM_DG_UNROLL];
#pragma unroll
    for (int u = 0; u < GM_DG_UNROLL; u++) {  // rows past the end stay in the wave: no cells, no escapes
      const int64_t i = (step0 + k + u) * RPW + sub;
      const bool valid = i < s.n;
      const uint32_t *piece = (const uint32_t *)(s.table + (slab + (size_t)i) * B);
#pragma unroll
      for (int d = 0; d < 4; d++) tw[u][d] = valid ? __builtin_nontemporal_load(piece + d * LPR + li) : 0u;
      wt[u] = valid ? s.wtick[i] : 0;
      ew[u] = valid && li == 0 ? s.brec[slab + (size_t)i].w : 0u;
    }
#pragma unroll
    for (int u = 0; u < GM_DG_UNROLL; u++) {
      const int64_t i = (step0 + k + u) * RPW + sub;
      uint64_t acc = 0;
      uint32_t nesc = 0;
#pragma unroll
      for (int q = 0; q < Q; q++) {
        const uint32_t x = (tw[u][q >> 2] >> (8 * (q & 3))) & 0xFFu;
        if (x >= 16) {  // h = 224 + 2 h4, age a (s_widen)
          if ((real >> q) & 1u) acc += dg_cell(kc[q], 2 * wt[u] + hoff[q] + 224 + 2 * (int)(x >> 4), wt[u] - (int)(x & 15u));
        } else if (x) {
          nesc++;
        }
      }
      acc = dg_group_sum<LPR>(acc);
      // the piece's escape bytes against its list word, as the host decoder checks them
      const uint32_t tot = (uint32_t)dg_group_sum<LPR>((uint64_t)nesc);
      if (li == 0 && i < s.n) {
        if (acc) atomicAdd(rows + i, (dg_u64)acc);
        if (S_EW_TOT(ew[u]) != tot) bad = true;
      }
    }
  }
  if (bad) atomicOr(status, GM_DG_ESTATE);
}

// ------------------------------------------------------------------ SCALED: the escape lists
// Grid (ceil(n / rrun), nb): the lists of the tile's rows, crashed rows included.
__global__ __launch_bounds__(256) void gm_dg_esc(SState s, dg_u64 *rows, uint32_t *status, int T, int rrun) {
  const int tid = threadIdx.x;
  const int b = blockIdx.y, r0 = blockIdx.x * rrun, nrows = min(rrun, s.n - r0);
  const int B = s.band, par = T & 1;
  const size_t slab = (size_t)b * s.n;
  uint32_t any = 0;
  for (int i = tid; i < nrows; i += 256) any |= S_EW_TOT(s.brec[slab + r0 + i].w);
  if (!__syncthreads_or(any != 0)) return;  // the steady tick: no list in these rows
  bool bad = false;
  const int li = tid & 15;
  // every 16-lane group runs the same number of rounds, so the DPP row of a list is always whole
  for (int i0 = 0; i0 < nrows; i0 += 16) {
    const int i = i0 + (tid >> 4);
    uint64_t acc = 0;
    if (i < nrows) {
      const int r = r0 + i;
      const uint32_t w = s.brec[slab + r].w;
      const int tot = (int)S_EW_TOT(w);
      // the list's extent before anything of it is read (gm_dg_bytes compares tot with the piece's bytes)
      if (tot > B || (tot > S_ESC_IN && S_EW_OFF(w) + (uint32_t)(tot - S_ESC_IN) > s.tesc_region)) {
        bad = true;
      } else if (tot) {
        const int wt = s.wtick[r];
        const EscList l = esc_list(s, par, slab, r, w);
        const uint8_t *cells = s.table + (slab + r) * B;
        for (int j = li; j < tot; j += 16) {
          const uint32_t e = *l.at(j);
          const uint32_t col = e & 0xFFFFu, cell = e >> 16;
          if (col >= (uint32_t)B || !s_is_esc(cells[col])) {  // an entry for a cell that is no escape
            bad = true;
            continue;
          }
          const int lc = b * B + (int)col;
          if (!cell || lc >= s.w) continue;  // absent
          const int c = s.c0 + lc;
          acc += dg_cell(gm_mix64(GM_DG_KCOL ^ (uint64_t)c), 2 * wt - 255 + (int)S_H(cell) - s_hbase(s.ramp, c),
                         wt - (int)S_AGE(cell));
        }
      }
    }
    acc = dg_group_sum<16>(acc);
    if (li == 0 && acc) atomicAdd(rows + r0 + i, (dg_u64)acc);
  }
  if (bad) atomicOr(status, GM_DG_ESTATE);
}

// ------------------------------------------------------------------ node words
// the word of node r: st = the flags and the heartbeat counter as gm_read_nodes returns them, the
// first `count` targets in draw order (slots from count on are not read)
__device__ __forceinline__ uint64_t dg_node_word(int r, int inited, int ingroup, int failed, int heartbeat, int count,
                                                 const int32_t *targets) {
  const uint64_t kn = gm_mix64(GM_DG_KNODE ^ (uint64_t)r);
  uint64_t v = gm_mix64(kn ^ (((uint64_t)(int64_t)heartbeat << 8) | ((uint64_t)(int64_t)count << 3) |
                              ((uint64_t)(int64_t)failed << 2) | ((uint64_t)ingroup << 1) | (uint64_t)inited));
  for (int q = 0; q < count && q < GM_FANOUT; q++)
    v += gm_mix64(gm_mix64(kn + (uint64_t)q + 1) ^ (uint64_t)(int64_t)targets[q]);
  return v;
}

__global__ __launch_bounds__(256) void gm_dg_nodes(SState s, int T, const int32_t *fail_t, dg_u64 *nodes) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= s.n) return;
  if (r < s.c0 || r >= s.c0 + s.w) {  // a column shard's heartbeat counter is current for its own columns only
    nodes[r] = 0;
    return;
  }
  const int failed = s.failed[r];
  int inited = 1, ingroup = 1;
  if (s.ramp) {  // started / in the group as of tick T (gm_read_nodes)
    // the copy of fail_t is refreshed when a node is marked; a mark cleared since (nodeStart of a node
    // crashed before it started) leaves the host's entry at "never", as a clear flag says here
    const int last = failed ? fail_t[r] : 0x7FFFFFFF;
    inited = T >= s_start(r);
    ingroup = r == 0 ? inited : (s_ingroup(1, s.intro_until, r, T) && last >= s_start(r) + 2);
  }
  nodes[r] = dg_node_word(r, inited, ingroup, failed, s.hbctr[r], s.rowstat[4 * (size_t)r + 3],
                          s.targets + (size_t)r * GM_FANOUT);
}

// ------------------------------------------------------------------ PARTIAL: views and node words
// lists: the views of parity T & 1, [nloc][V]. spw: steps per wave, a multiple of GM_DG_UNROLL.
__global__ __launch_bounds__(256) void gm_dg_views(const uint64_t *__restrict__ lists, const int32_t *__restrict__ failed,
                                                   const int32_t *__restrict__ hbctr,
                                                   const int32_t *__restrict__ rowstat,
                                                   const int32_t *__restrict__ targets, dg_u64 *rows, dg_u64 *nodes,
                                                   uint32_t *status, int n, int n0, int nloc, int V, int spw) {
  const int lane = threadIdx.x & 63;
  const int vpw = 64 / V;  // views per wave step
  const int sub = lane / V, e = lane - sub * V;
  const bool on = sub < vpw;  // V not a divisor of 64: the last lanes idle
  const int64_t s0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * spw;
  bool bad = false;
  for (int k = 0; k < spw; k += GM_DG_UNROLL) {
    uint64_t x[GM_DG_UNROLL];
#pragma unroll
    for (int u = 0; u < GM_DG_UNROLL; u++) {
      const int64_t view = (s0 + k + u) * vpw + sub;
      x[u] = on && view < nloc && rows ? __builtin_nontemporal_load(lists + view * V + e) : 0ull;
    }
#pragma unroll
    for (int u = 0; u < GM_DG_UNROLL; u++) {
      const int64_t view = (s0 + k + u) * vpw + sub;
      uint64_t v = 0;
      if (x[u]) {
        const uint32_t id = (uint32_t)(x[u] >> 32), hb = (uint32_t)x[u];
        if (id < 1u || id > (uint32_t)n) bad = true;
        else v = dg_cell(gm_mix64(GM_DG_KCOL ^ (uint64_t)(id - 1u)), (int)hb, (int)((hb + 1u) >> 1));
      }
      // the view's lanes e .. V - 1 summed into lane e: a shuffle tree that stops at the view's end
      for (int d = 1; d < V; d <<= 1) {
        const uint64_t o = (uint64_t)__shfl_down((long long)v, d, 64);
        if (e + d < V) v += o;
      }
      if (on && e == 0 && view < nloc) {
        if (rows) rows[view] = v;
        if (nodes)
          nodes[view] = dg_node_word(n0 + (int)view, 1, 1, failed[view], hbctr[view], rowstat[4 * view + 3],
                                     targets + view * GM_FANOUT);
      }
    }
  }
  if (bad) atomicOr(status, GM_DG_EID);
}

// ------------------------------------------------------------------ fold
__device__ __forceinline__ uint64_t dg_fold(uint64_t r, uint64_t x) { return gm_mix64(gm_mix64(GM_DG_KROW ^ r) ^ x); }

__global__ __launch_bounds__(256) void gm_dg_fold(const dg_u64 *__restrict__ rows, const dg_u64 *__restrict__ nodes,
                                                  int count, int r0, dg_u64 *sums) {
  __shared__ uint64_t part[2][4];
  uint64_t a = 0, b = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (int64_t)gridDim.x * 256) {
    a += dg_fold((uint64_t)(r0 + i), rows[i]);
    b += dg_fold((uint64_t)(r0 + i), nodes[i]);
  }
  a = dg_group_sum<64>(a);
  b = dg_group_sum<64>(b);
  if ((threadIdx.x & 63) == 0) {
    part[0][threadIdx.x >> 6] = a;
    part[1][threadIdx.x >> 6] = b;
  }
  __syncthreads();
  if (threadIdx.x < 2)
    atomicAdd(sums + threadIdx.x, (dg_u64)(part[threadIdx.x][0] + part[threadIdx.x][1] + part[threadIdx.x][2] +
                                           part[threadIdx.x][3]));
}

// ------------------------------------------------------------------ launch wrappers
// steps per wave so that about GM_DG_WAVES waves cover `steps`, a multiple of GM_DG_UNROLL
static int dg_spw(int64_t steps, int64_t waves) {
  const int64_t spw = (steps + waves - 1) / waves;
  return (int)std::max<int64_t>(GM_DG_UNROLL, (spw + GM_DG_UNROLL - 1) / GM_DG_UNROLL * GM_DG_UNROLL);
}

template <int B>
static void launch_bytes_b(const SState &s, uint64_t *rows, uint32_t *status, hipStream_t st) {
  constexpr int RPW = 64 / (B / S_COLS_PER_LANE);
  const int64_t steps = ((int64_t)s.n + RPW - 1) / RPW;
  const int spw = dg_spw(steps, std::max<int64_t>(1, GM_DG_WAVES / s.nb));
  const int64_t waves = (steps + spw - 1) / spw;
  hipLaunchKernelGGL(gm_dg_bytes<B>, dim3((unsigned)((waves + 3) / 4), s.nb), dim3(256), 0, st, s, (dg_u64 *)rows, status,
                     spw);
}

hipError_t gm_launch_digest_table(const SState &s, int T, uint64_t *rows, uint32_t *status, hipStream_t st) {
  const hipError_t e = gm_band_dispatch(s.band, [&](auto b) {
    launch_bytes_b<decltype(b)::value>(s, rows, status, st);
    return hipGetLastError();
  });
  if (e != hipSuccess) return e;
  const int64_t want = ((int64_t)s.n * s.nb + 1023) / 1024;
  const int rrun = (int)std::min<int64_t>(GM_DG_RUN_MAX, std::max<int64_t>(GM_DG_RUN_MIN, want));
  hipLaunchKernelGGL(gm_dg_esc, dim3((s.n + rrun - 1) / rrun, s.nb), dim3(256), 0, st, s, (dg_u64 *)rows, status, T, rrun);
  return hipGetLastError();
}

hipError_t gm_launch_digest_nodes(const SState &s, int T, const int32_t *fail_t, uint64_t *nodes, hipStream_t st) {
  if (s.ramp && !fail_t) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gm_dg_nodes, dim3((s.n + 255) / 256), dim3(256), 0, st, s, T, fail_t, (dg_u64 *)nodes);
  return hipGetLastError();
}

hipError_t gm_launch_digest_views(const PState &p, int T, uint64_t *rows, uint64_t *nodes, uint32_t *status,
                                  hipStream_t st) {
  if (p.V < 2 || p.V > P_VMAX) return hipErrorInvalidValue;
  const int vpw = 64 / p.V;
  const int64_t steps = ((int64_t)p.nloc + vpw - 1) / vpw;
  const int spw = dg_spw(steps, GM_DG_WAVES);
  const int64_t waves = (steps + spw - 1) / spw;
  const uint64_t *lists = p.lists + (size_t)(T & 1) * p.rows * p.V;
  hipLaunchKernelGGL(gm_dg_views, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, st, lists, p.failed, p.hbctr, p.rowstat,
                     p.targets, (dg_u64 *)rows, (dg_u64 *)nodes, status, p.n, p.n0, p.nloc, p.V, spw);
  return hipGetLastError();
}

hipError_t gm_launch_digest_fold(const uint64_t *rows, const uint64_t *nodes, int count, int r0, uint64_t *sums,
                                 hipStream_t st) {
  const int blocks = std::max(1, std::min(1024, (count + 255) / 256));
  hipLaunchKernelGGL(gm_dg_fold, dim3(blocks), dim3(256), 0, st, (const dg_u64 *)rows, (const dg_u64 *)nodes, count, r0,
                     (dg_u64 *)sums);
  return hipGetLastError();
}
