// gm_partial.hip -- PARTIAL-view tick (scenario S-C: V-entry membership views).
//
// The reference is full-membership only; GM_MODE_PARTIAL caps every membership
// list at V entries with the semantics restated (and specified) by the oracle,
// oracle/ref_cpu.c "PARTIAL": entries carry their heartbeat's production tick
// (ts = (hb+1)/2), merge keeps the largest hb per id (updatelistCallBack,
// MP1Node.cpp:259-301), self bump, TFAIL/TREMOVE sweep (MP1Node.cpp:404-447),
// eviction to the V freshest (keyed tie-break), then the reference gossip draw
// over the final list (MP1Node.cpp:449-489) and sendMemberList of its fresh
// entries (MP1Node.cpp:360-395).
//
// One wave per node, everything in a ~4.8 KB LDS slice so 8 waves share a SIMD
// (the per-node work is short dependent-load chains + LDS atomics: latency is
// hidden by occupancy, and the instruction count per node is what bounds the
// kernel once it is):
//   1. loads issue together: the node's own list (one 8-byte entry per lane),
//      its inbox (sender indices), its 16 precomputed S2 outputs, then every
//      delivered list (V lanes per list, several lists per wave step);
//   2. merge into an open-addressing LDS table keyed by id (32-bit CAS claim +
//      ds_max of the heartbeat word), own entries first so they carry the
//      "own" bit, delivered entries filtered to fresh + not dropped;
//   3. self bump, then one sweep compacts the table in place into a dense
//      array (TREMOVE removals counted and logged on the way);
//   4. eviction to V only when the union exceeds V: ballots over the classes of
//      heartbeat distance from the top find the cut heartbeat; inside the cut
//      bucket a 6-bit radix histogram of the eviction keys and (rarely) an
//      exact min-selection pick the smallest keys -- no full sort;
//   5. the <= V kept entries are ranked by id (broadcast LDS compare) = the
//      id-sorted list, stored as one coalesced row; joins as a bit mask over it;
//   6. the gossip draw: the 16 precomputed S2 outputs resolved in parallel across
//      the wave (duplicates by shuffle-compares), the rare rest on scalars.
// Nodes with more than P_KSMALL delivered lists (Poisson tail, ~0.2 % at 12) do not fit
// the small table: the small kernel defers them to a worklist that the big
// kernel (1024-slot table) drains, and those with more than P_KP lists (~2e-5) to the
// huge kernel's (4096 slots): every delivered list is merged, as EmulNet delivers them all.
// Lists are double-buffered by tick parity: a receiver reads its senders' lists
// of tick t-1 directly, so no separate payload copy is written.
//
// The files of the PARTIAL kernel group (gm_partial.h: PState, the table sizes, the launch wrappers):
//   gm_partial_node.h    the node tick p_node, a function per stage above where that costs neither
//                        registers nor time (profiles/partial_split/), and what it stands on:
//                        the P_* table constants, PLds, the wave helpers, p_insert, p_owner,
//                        PPre / p_preload, p_frozen (header)
//   gm_partial.hip       this file: the LDS-DMA prefetch (p_prefetch / p_unpack_next), p_small_node,
//                        the three tick kernels, gm_p_mtgen, gm_p_init, their launchers
//   gm_partial_xchg.hip  the row-shard exchange: gm_p_unpack, gm_p_pack, their launchers (a unit of
//                        its own: all 17 kernels compile to the same assembly as in one unit)
#include <algorithm>

#include "gm_partial_node.h"

// The small kernel's next node, prefetched while the wave works on the current one: ONE
// packed word per lane -- inbox ids on lanes 0..15, S2 outputs on 16..31, crash flag / inbox
// count / heartbeat counter on lanes 32 / 33 / 34 -- by an LDS-DMA load (global_load_lds:
// no VGPR holds it across the node, and no register copy at the loop edge waits for it) into
// the wave's P_PF_BYTES area. The compiler does not see this load (inline asm): every node
// starts with vmcnt(0), which retires the DMA its predecessor issued.
#define P_PF_LANES 40
#define P_PF_BYTES (P_PF_LANES * 4)
__device__ __forceinline__ void p_prefetch(const PState &s, int t, const uint32_t *mtraw, int li, int lane,
                                           uint32_t lds) {
  const int par = t & 1;
  const uint32_t *a = lane < 16   ? (const uint32_t *)s.inbox[par] + (size_t)li * P_KMAX + 1 + lane
                      : lane < 32 ? mtraw + (size_t)li * 16 + (lane - 16)
                      : lane == 32 ? (const uint32_t *)s.failed + li
                      : lane == 33 ? (const uint32_t *)s.inbox[par] + (size_t)li * P_KMAX
                                   : (const uint32_t *)s.hbctr + li;
  if (lane < P_PF_LANES) {
    uint32_t keep;  // m0 = the LDS destination (lane l writes dword l); the reads of the area
                    // by the node before are waited for first
    asm volatile(
        "s_waitcnt lgkmcnt(0)\n\ts_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\t"
        "global_load_lds_dword %1, off\n\ts_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(a), "s"(lds)
        : "memory");
  }
}
template <int VF>
__device__ __forceinline__ PPre p_unpack_next(const PState &s, int t, int li, uint32_t pv, int lane) {
  const int V = VF ? VF : s.V;
  PPre p;
  p.failed = (int)__builtin_amdgcn_readlane(pv, 32);
  p.k = (int)__builtin_amdgcn_readlane(pv, 33);
  p.hbctr = (int)__builtin_amdgcn_readlane(pv, 34);
  p.own = lane < V ? s.lists[((size_t)((t & 1) ^ 1) * s.rows + li) * V + lane] : 0ull;
  p.sv = lane < 16 ? (int)pv : 0;
  p.raw0 = pv;
  p.roff = 16;
  return p;
}

// rows [r0, r1) = chunk `chunk` of this shard's nodes
template <bool MC, bool RM, int VF>
__device__ __forceinline__ void p_small_node(const PState &s, int t, const PPre &pre, int li, int lane,
                                             unsigned char *base, int chunk, int r0) {
  if (pre.failed) {
    p_frozen(s, t, li, lane);
    return;
  }
  if (pre.k > P_KSMALL) {  // deferred to gm_p_tick_big (<= P_KP lists) or gm_p_tick_huge
    if (lane == 0) {
      if (pre.k <= P_KP) s.big[r0 + atomicAdd(&s.big_cnt[chunk], 1)] = li;
      else s.huge[r0 + atomicAdd(&s.huge_cnt[chunk], 1)] = li;
    }
    return;
  }
  p_node<P_HS, false, MC, RM, VF>(s, t, pre, li, lane, base);
}

// P_NPW consecutive nodes per wave: each node's loads are prefetched during the node before it
// (p_prefetch), so a node starts with one global round trip (its delivered lists) instead of two.
// Held to 8 waves per SIMD (64 VGPRs; the loop keeps more live otherwise, and some SGPRs spill to
// VGPR lanes: ~40 more VALU per node, still faster than one node per wave: 26.1 vs 27.5 ms).
// P_SWG = 1 wave per workgroup: a finished wave releases its LDS slice at once (with 4 waves per
// workgroup the slice waited for the workgroup's last wave: 23.5 -> 22.8 ms)
template <bool MC, bool RM, int VF>
__global__ __launch_bounds__(64 * P_SWG) __attribute__((amdgpu_waves_per_eu(8, 8))) void gm_p_tick_small_pf(
    PState s, int t, const uint32_t *mtraw, int chunk, int r0, int r1, int npw) {
  // static LDS: its addresses are compile-time constants (offsets fold into the LDS instructions)
  __shared__ __align__(16) unsigned char p_smem[P_SWG * (PLds<P_HS>::bytes + P_PF_BYTES)];
  const int wave = P_SWG == 1 ? 0 : __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int l0 = r0 + (blockIdx.x * P_SWG + wave) * npw;
  if (l0 >= r1) return;  // whole wave; no workgroup barrier in this kernel
  unsigned char *base = p_smem + (size_t)wave * PLds<P_HS>::bytes;
  const int l1 = min(r1, l0 + npw);
  uint32_t *pf = (uint32_t *)(p_smem + P_SWG * (size_t)PLds<P_HS>::bytes + (size_t)wave * P_PF_BYTES);
  const uint32_t pfa =
      __builtin_amdgcn_readfirstlane((uint32_t)(size_t)(__attribute__((address_space(3))) uint32_t *)pf);
  p_prefetch(s, t, mtraw, l0, lane, pfa);
  for (int li = l0; li < l1; li++) {
    // the kernel arguments and the lane index pass through empty asm each node, so the
    // compiler re-derives what it needs per node instead of hoisting every address and
    // lane-dependent value out of the loop (that held 120 VGPRs live: occupancy 4).
    // (s is the first kernel argument: it sits at offset 0 of the kernarg segment)
    const __attribute__((address_space(4))) PState *ka =
        (const __attribute__((address_space(4))) PState *)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(ka));
    const PState &ss = *(const PState *)ka;
    int ln = lane;
    asm volatile("" : "+v"(ln));
    const int tt = t, cc = chunk, rr = r0;
    const uint32_t *mt = mtraw;
    // the node before is done except for its stores: retire them (and, for the compiler's
    // bookkeeping, every load it issued), so no stale pending load makes it wait on the DMA
    // issued next
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
    asm volatile("" ::: "memory");       // the prefetch area is read only after the wait
    const uint32_t pv = ln < P_PF_LANES ? pf[ln] : 0u;
    if (li + 1 < l1) p_prefetch(ss, tt, mt, li + 1, ln, pfa);
    const PPre pre = p_unpack_next<VF>(ss, tt, li, pv, ln);
    p_small_node<MC, RM, VF>(ss, tt, pre, li, ln, base, cc, rr);
  }
}

// drains the worklist gm_p_tick_small_pf filled (a fixed grid; every wave exits when the list is done),
// P_BWG waves per workgroup
#define P_BWG 4
template <bool MC>
__global__ __launch_bounds__(64 * P_BWG, 3) void gm_p_tick_big(PState s, int t, const uint32_t *mtraw, int chunk, int r0) {
  extern __shared__ __align__(16) unsigned char p_smem[];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int nbig = s.big_cnt[chunk];
  for (int w = blockIdx.x * P_BWG + wave; w < nbig; w += gridDim.x * P_BWG) {
    const int li = s.big[r0 + w];
    const PPre pre = p_preload(s, t, mtraw, li, lane, P_KMAX - 1);
    p_node<P_HB, true, MC>(s, t, pre, li, lane, p_smem + (size_t)wave * PLds<P_HB>::bytes);
  }
}

// drains the nodes with more than P_KP lists (Poisson tail: ~2e-5 of the nodes at S-C), one wave per
// workgroup for the 33 KB table
template <bool MC>
__global__ __launch_bounds__(64) void gm_p_tick_huge(PState s, int t, const uint32_t *mtraw, int chunk, int r0) {
  extern __shared__ __align__(16) unsigned char p_smem[];
  const int lane = threadIdx.x & 63;
  const int nh = s.huge_cnt[chunk];
  for (int w = blockIdx.x; w < nh; w += gridDim.x) {
    const int li = s.huge[r0 + w];
    const PPre pre = p_preload(s, t, mtraw, li, lane, P_KMAX - 1);
    p_node<P_HH, true, MC>(s, t, pre, li, lane, p_smem);
  }
}

// first 16 S2 outputs of every node for tick t (see gm_mt_first16); resets the chunks' big and
// huge worklists (the outgoing record counts pk_cnt are cleared by the host, gm_host_partial.hip)
__global__ __launch_bounds__(256) void gm_p_mtgen(PState s, int t, uint32_t *mtraw, int reset) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (reset && r < s.nchunk) s.big_cnt[r] = s.huge_cnt[r] = 0;
  if (r >= s.nloc) return;
  uint32_t out[16];
  gm_mt_first16(gm_rd_seed(s.rd_seed, t, s.n0 + r + 1), out);
  uint4 *dst = (uint4 *)(mtraw + (size_t)r * 16);
#pragma unroll
  for (int q = 0; q < 4; q++) dst[q] = make_uint4(out[4 * q], out[4 * q + 1], out[4 * q + 2], out[4 * q + 3]);
}

// warm start at t0 (oracle op_create): self {2t0-1}, V-1 distinct peers chosen by
// mix64(view_seed ^ i<<32 ^ j) % n with hb 2(t0-1-a)-1, sorted by id; written to the
// parity of tick t0.
__global__ __launch_bounds__(64) void gm_p_init(PState s, int t0, uint64_t init_seed) {
  const int li = blockIdx.x * blockDim.x + threadIdx.x;
  if (li >= s.nloc) return;
  const int i = s.n0 + li;
  const int V = s.V;
  uint64_t ent[P_VMAX];
  int cnt = 1;
  ent[0] = ((uint64_t)(uint32_t)(i + 1) << 32) | (uint32_t)(2 * t0 - 1);
  for (uint64_t j = 0; cnt < V; j++) {
    const int q = (int)(gm_mix64(s.view_seed ^ ((uint64_t)(uint32_t)i << 32) ^ j) % (uint64_t)s.n);
    bool dup = q == i;
    for (int a = 1; a < cnt && !dup; a++) dup = (int)(ent[a] >> 32) == q + 1;
    if (dup) continue;
    const int a = (int)((gm_mix64(init_seed ^ ((uint64_t)(uint32_t)i << 32) ^ (uint64_t)(uint32_t)q) >> 40) % 4);
    ent[cnt++] = ((uint64_t)(uint32_t)(q + 1) << 32) | (uint32_t)(2 * (t0 - 1 - a) - 1);
  }
  for (int a = 1; a < cnt; a++)
    for (int b = a; b > 0 && ent[b - 1] > ent[b]; b--) {
      const uint64_t x = ent[b];
      ent[b] = ent[b - 1];
      ent[b - 1] = x;
    }
  uint64_t *dst = s.lists + ((size_t)(t0 & 1) * s.rows + li) * V;
  for (int a = 0; a < V; a++) dst[a] = a < cnt ? ent[a] : 0ull;
  s.hbctr[li] = 2 * t0;
}

#define P_BIG_GRID 1024
#define P_HUGE_GRID 256

// S2 precompute for every row + reset of the per-chunk worklists
hipError_t gm_launch_partial_mtgen(const PState &s, int t, uint32_t *mtraw, hipStream_t st, bool reset) {
  hipLaunchKernelGGL(gm_p_mtgen, dim3((std::max(s.nloc, s.nchunk) + 255) / 256), dim3(256), 0, st, s, t, mtraw,
                     reset ? 1 : 0);
  return hipGetLastError();
}

// the per-tick resets gm_p_mtgen does when the S2 outputs were prefetched without them
hipError_t gm_launch_partial_reset(const PState &s, hipStream_t st) {
  hipError_t e = hipMemsetAsync(s.big_cnt, 0, sizeof(int32_t) * s.nchunk, st);
  if (e == hipSuccess) e = hipMemsetAsync(s.huge_cnt, 0, sizeof(int32_t) * s.nchunk, st);
  return e;
}

// The small kernel's instantiation as compile-time constants: calls f(mc, rm, vf) with
// std::integral_constant arguments for (msgcount recording, received lists possible, the view width
// folded in: P_VMAX at S-C -- shifts, not multiplies -- else 0 = run time) and returns its hipError_t
template <typename F>
inline hipError_t p_small_dispatch(bool mc, bool rm, int V, F &&f) {
  using T = std::true_type;
  using N = std::false_type;
  using V32 = std::integral_constant<int, P_VMAX>;
  using V0 = std::integral_constant<int, 0>;
  switch ((mc ? 4 : 0) | (rm ? 2 : 0) | (V == P_VMAX ? 1 : 0)) {
    case 0: return f(N{}, N{}, V0{});
    case 1: return f(N{}, N{}, V32{});
    case 2: return f(N{}, T{}, V0{});
    case 3: return f(N{}, T{}, V32{});
    case 4: return f(T{}, N{}, V0{});
    case 5: return f(T{}, N{}, V32{});
    case 6: return f(T{}, T{}, V0{});
    default: return f(T{}, T{}, V32{});
  }
}

// the node ticks of chunk c (rows [nloc*c/K, nloc*(c+1)/K))
hipError_t gm_launch_partial_chunk(const PState &s, int t, const uint32_t *mtraw, int c, hipStream_t st) {
  const int r0 = (int)((int64_t)s.nloc * c / s.nchunk), r1 = (int)((int64_t)s.nloc * (c + 1) / s.nchunk);
  const bool mc = s.mc_sent != nullptr && t < s.mc_tmax;
  if (r1 > r0) {
    const bool rm = s.rows != s.n || s.G > 1 || s.nloc != s.n;  // received lists possible
    // nodes per wave: P_NPW; a row shard's chunk (a few hundred thousand nodes per launch) takes
    // P_NPW_CHUNK, so the launch's last round of waves is a smaller share of it
    const int npw = s.nchunk > 1 ? P_NPW_CHUNK : P_NPW;
    const dim3 grid((r1 - r0 + P_SWG * npw - 1) / (P_SWG * npw));
    (void)p_small_dispatch(mc, rm, s.V, [&](auto m, auto r, auto v) {  // (a launch error shows at the end)
      hipLaunchKernelGGL((gm_p_tick_small_pf<decltype(m)::value, decltype(r)::value, decltype(v)::value>), grid,
                         dim3(64 * P_SWG), 0, st, s, t, mtraw, c, r0, r1, npw);
      return hipSuccess;
    });
  }
  hipLaunchKernelGGL(mc ? gm_p_tick_big<true> : gm_p_tick_big<false>, dim3(P_BIG_GRID), dim3(64 * P_BWG),
                     gm_partial_lds_bytes(), st, s, t, mtraw, c, r0);
  hipLaunchKernelGGL(mc ? gm_p_tick_huge<true> : gm_p_tick_huge<false>, dim3(P_HUGE_GRID), dim3(64),
                     PLds<P_HH>::bytes, st, s, t, mtraw, c, r0);
  return hipGetLastError();
}

hipError_t gm_launch_partial_init(const PState &s, int t0, uint64_t init_seed, hipStream_t st) {
  hipLaunchKernelGGL(gm_p_init, dim3((s.nloc + 63) / 64), dim3(64), 0, st, s, t0, init_seed);
  return hipGetLastError();
}

size_t gm_partial_lds_bytes() { return P_BWG * (size_t)PLds<P_HB>::bytes; }  // gm_p_tick_big's dynamic LDS
