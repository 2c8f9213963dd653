// gm_scaled.h -- device state of the SCALED tick, the cell encoding, the store side of the band
// sweep and the host launch wrappers. The kernels are in units by concern: gm_scaled.hip (overview;
// gm_s_mtgen, init, msgcount, gm_launch_tick), gm_band.hip / gm_band_fast.hip (the band sweep),
// gm_pick.hip (the single-context draw), gm_draw.hip (the column-shard draw protocol).
#pragma once
#include <stdint.h>

#include <type_traits>

#include "gm_abi.h"
#include "gm_device.h"

#define S_KMAX 64                // inbox capacity (gossip lists per receiver per tick)
#define S_COLS_PER_LANE 16       // 32 B of table + 16 B per sender payload per lane and row
#define S_ROW_ALIGN 512          // padded row width granule (a multiple of every band width up to 512)
#define S_CHUNK(B) ((B) >= 1024 ? 128 : 64)  // columns per rank-select chunk (<= 8 chunks per band)
#define S_SB 8                   // sender ids prefetched per row; payload loads in flight per lane
#define S_MT_RAW 16              // mt19937 outputs precomputed per row and tick (gm_s_mtgen)
#define S_SELFADD_CAP 65536      // join ramp: self appends verified per tick (gm_s_selfcheck)
#define S_PLIST_CAP 4096         // sharded tick: rows a second (bounded) draw round takes
#define S_FB_BLOCKS 2048         // workgroups (4 waves) of gm_s_band's pass over the fast path's handed-back units
#define GM_D_MORE_ROUND 64       // S2 outputs of bounded round 1 (= one host-driven round)
#define GM_D_LAST_ROUND 256      // S2 outputs of bounded round 2 (= host-driven rounds 2..5)

// SCALED cell (16 bits), relative to the tick w the row was last written at:
//   h = 255 - (2w - hb) (8 bits, the heartbeat; larger = newer), age = w - ts (5 bits);
//   cell = h << 5 | age, 0 = absent. Every tick rewrites every live cell, re-basing it
// to the new tick (h -= 2, age += 1: cell - 63). Ordering cells by value orders them
// by heartbeat first and, for equal heartbeats, keeps the older timestamp -- so the
// merge of updatelistCallBack is a max. In the SCALED regime a live node's heartbeat
// at tick t is 2t-1 (h = 254); h falls by 2 per tick of heartbeat lag, and a present
// entry lagging more than ~126 ticks sets GM_ERR_LAG instead of wrapping.
#define S_CELL(h, age) (((h) << 5) | (age))
// Stored table cell: ONE BYTE per (observer, subject). The 16-bit cell above is the
// working format in registers; in HBM a cell is
//   0             absent
//   h4 << 4 | a   h = 224 + 2 h4 (h4 in [3, 15]: even h in [230, 254], heartbeat lag <= 12
//                 ticks), age a <= 14 -- every live entry of a warm, steady cluster. The range
//                 is one short of the byte's at both ends, so that a stored byte re-based by one
//                 tick (h4 - 1, a + 1) is again a byte: gm_s_band's fast path merges and sweeps
//                 the stored bytes themselves and tests only its outputs
//   1 (S_B_ESC)   escaped: the exact 16-bit cell is an entry of the (band, row)'s escape list
//                 (codes 2..15, h4 = 0, are unused)
// Cells outside the byte's range (odd h of cold-start / JOINREQ entries, lag > 12 or age > 14,
// e.g. a crashed node's entries in the ticks before TREMOVE) escape. The pool is COMPACT: per
// (band, row) the escaped cells of the row's band slice (lane by lane; entries carry their columns,
// so the order is not significant), as consecutive u32
// ENTRIES of the tick that wrote them (tick parity: written at t, read at t+1), one u32 per
// escaped cell: its column in the band (low 16 bits) | its 16-bit cell << 16. The first S_ESC_IN
// entries sit in the list's fixed inline slot (no allocation: a crash window escapes ~1 % of a
// row's cells, ~10 per 1024-column band), the rest in the pool region of the list's stripe.
// The (band, row) record's .w is the list's word: entry count | offset in the stripe's region
// << 11 (0: no escapes), so a reader knows the list's extent with the row's metadata and
// prefetches the inline entries with the payload gathers; it scatters the entries into its
// row's cells through LDS (entries carry their columns: no per-cell search). Capacity is
// bounded (gm_host_scaled.hip: dense-equivalent for small clusters, a fraction of the cells beyond);
// an overflow sets GM_ERR_ESC (-> GM_ERANGE) -- never a silent divergence.
#define S_B_ESC 1u
#define S_H4_MIN_H 230u  // smallest h a stored byte holds (h4 = 3)
#define S_AGE_MAX_B 14u  // largest age a stored byte holds
#define S_ESC_IN 16                 // entries of a (band, row) list held inline (64 B per list)
#define S_EW_TOT(w) ((w) & 0x7FFu)  // escape-list word: entry count (<= band width)
#define S_EW_OFF(w) ((w) >> 11)     // offset of entries S_ESC_IN.. in the stripe's pool region
#define S_EW_REGION_MAX (1u << 21)  // pool entries per stripe the word can address
__host__ __device__ inline bool s_is_esc(uint32_t b) { return b != 0 && b < 16; }
__host__ __device__ inline uint32_t s_widen(uint32_t b) {  // byte -> 16-bit cell (escape codes: look in the pool)
  return b == 0 ? 0u : (7168u + ((b & 0xF0u) << 2) + (b & 0x0Fu));
}
__host__ __device__ inline uint32_t s_narrow(uint32_t c) {  // 16-bit cell -> byte (an escape code if not representable)
  if (c == 0) return 0u;
  const uint32_t h = c >> 5, a = c & 31u;
  if (h >= S_H4_MIN_H && !(h & 1) && a <= S_AGE_MAX_B) return (((h - 224) >> 1) << 4) | a;
  return S_B_ESC;
}
__host__ __device__ inline int s_start(int j) { return j >> 2; }  // (int)(0.25 * j) for j >= 0
__host__ __device__ inline int s_hbase(int ramp, int j) { return (ramp && j > 0) ? 2 * (s_start(j) + 1) : 0; }
__host__ __device__ inline bool s_ingroup(int ramp, int intro_until, int r, int t) {
  return !ramp || r == 0 || (t >= s_start(r) + 2 && s_start(r) + 1 <= intro_until);
}
// column shards: xcnt's per-(rank, row) present word carries a flag for a self append
#define S_XC_SELFAPP 0x40000000
// int32 index of (rank g, row r)'s present word in the chunk-major xcnt (numfailed follows it)
#define S_XC(s, g, r) \
  ((((((size_t)(r) >> (s).xlog) * (size_t)(s).shard_count + (size_t)(g)) << (s).xlog) + ((size_t)(r) & ((1u << (s).xlog) - 1))) * 2)
#define S_XC_COUNT 0x3FFFFFFF
#define S_H(c) ((c) >> 5)
#define S_AGE(c) ((c) & 31u)
// payload (sendMemberList's fresh entries, re-based to the receiving tick: h' = h - 2):
// one NIBBLE per cell, 0 = not sent, n in [1, 14] = h' = 224 + 2n (the even values
// [226, 252]: heartbeat lag <= 13 ticks -- every value of a warm, steady cluster), 15 =
// escape: the byte h' is in the wide plane (odd h' of cold-start / JOINREQ entries, or a
// larger lag). Larger nibble = larger h' = newer, so the merge maxes nibbles directly.
#define S_NIB_BASE 224u
#define S_NIB_ESC 15u
#define S_NIB_H(n) (S_NIB_BASE + 2u * (n))

// keyed loss threshold (gm_device.h gm_drop_thresh; gm_band.h s_keep)
__host__ __device__ inline uint32_t s_drop_thresh(int pct) { return gm_drop_thresh(pct); }

// status word of a state-loading call's device checks (gm_load.hip)
#define GM_LD_EINVAL 1u  // the state is malformed (-> GM_EINVAL)
#define GM_LD_ERANGE 2u  // an entry or an inbox beyond what the stored form holds (-> GM_ERANGE)

#define S_EV_STRIPES 16384  // the tick's event total in partial sums (a TREMOVE tick adds ~4 M of them)
#define S_EV_ADD 1u
#define S_EV_REMOVE 2u

// bcnt word of one (row, band): present | numfailed << 11 | events << 22 (saturating)
#include <hip/hip_runtime.h>
#define S_BC_PRES(v) ((v) & 0x7FFu)
#define S_BC_FAIL(v) (((v) >> 11) & 0x7FFu)
#define S_BC_NEV(v) ((v) >> 22)

struct SState {
  int n;                   // observers (rows) = N
  int wp;                  // padded shard width (columns per row, multiple of S_ROW_ALIGN)
  int w;                   // real shard width
  int c0;                  // first global subject column of this shard
  int band;                // columns per band (64..512, divides wp)
  int nb;                  // bands per row = wp / band
  int evs;                 // event slots per (row, band) = band / 32; more spill to the ring
  uint32_t ev_spill_cap;
  uint64_t rd_seed, drop_seed;
  // Band-tiled layout: cell (r, c) of band b = c / band lives at ((b * n + r) * band + c % band),
  // so one band of all rows is one contiguous slab (the unit gm_s_band sweeps).
  uint8_t *table;          // [nb][n][band] stored cell bytes (s_narrow of S_CELL)
  uint32_t *tesc_in[2];    // [nb * n][S_ESC_IN] by tick parity: the first entries of each (band, row) list
  uint32_t *tesc[2];       // escape pools by tick parity: a list's entries beyond S_ESC_IN, from brec.w
  // Allocation is STRIPED: (band, row) list u allocates in stripe (band * n + row) & (stripes - 1),
  // a region of `region` entries with its own counter -- one global counter would serialise
  // every (band, row) of a crash-window tick on one address (4 M atomics at S-A: 25 ms)
  int esc_stripes;         // power of two
  unsigned long long *tesc_cnt;  // [2][esc_stripes] cells allocated per stripe this tick (zeroed a tick ahead)
  uint32_t tesc_region;    // entries per stripe
  size_t tesc_cap;         // entries per pool = esc_stripes * tesc_region
  uint8_t *msg;            // [nb][n][2][band/2] gossip payload nibbles, both tick parities of a (band, row) adjacent
  // escaped payload bytes (nibble 15): per (band, sender) of tick parity p the lanes holding escapes
  // write their 16 payload bytes h' into consecutive 16-byte slots of pesc[p] from the record's base,
  // in lane order (pesc_rec[p][band * n + sender] = {base, lane mask lo, lane mask hi, 0}, written
  // only by senders with escapes and read only where a receiver meets nibble 15)
  uint8_t *pesc[2];
  uint4 *pesc_rec[2];
  unsigned long long *pesc_cnt;  // [2][esc_stripes] slots allocated per stripe this tick
  uint32_t pesc_region;    // 16-byte slots per stripe
  uint32_t pesc_cap;       // 16-byte slots per pool
  int32_t *wtick;          // [n] tick each row's cells are relative to (last written)
  int32_t *inbox_cnt[2];   // [n] lists queued for each receiver, by delivery-tick parity
  int32_t *inbox[2];       // [n][S_KMAX] sender rows
  int32_t *hbctr;          // [n] MP1Node heartbeat counter (Member::heartbeat)
  int32_t *failed;         // [n] Member::bFailed
  uint4 *brec;             // [nb][n] per-(band, row) record after the sweep: .x/.y = present cells per 64-column
                           // chunk (band/64 bytes, rank-select), .z = bcnt word (S_BC_*), .w = the slice's escape-list
                           // word (S_EW_*, 0: none); rows adjacent = whole-line writes
  uint32_t *ev_band;       // [n][nb][evs] kind<<30 | subject id
  uint64_t *ev_spill;      // overflow: (logger<<32) | kind<<30 | subject id
  uint32_t *ev_spill_cnt;  // [1 + S_EV_STRIPES]: spill records, then the tick's total records in
                           // S_EV_STRIPES striped partial sums (one hot address would serialise)
  uint64_t *evcum;         // [n][nb] cumulative events since create: joins | removals << 32 (single writer per cell)
  uint32_t *mtraw;        // [n][S_MT_RAW] first mt19937 outputs of each row's S2 stream this tick
  int32_t *rowstat;        // [n][4]: lists delivered, present, numfailed, targets chosen
  int32_t *targets;        // [n][GM_FANOUT]
  uint32_t *err;
  // ---- column-sharded mode (shard_count > 1, or one shard forced by GM_FORCE_SHARD=1 to
  // rehearse the sharded protocol + RCCL on one GPU; see gm_s_draw / gm_s_accept)
  int shard_rank, shard_count;
  int sharded;
  int stub;                // diagnostics (gm_shard_stub): one shard alone on a device; draws landing in
                           // other shards' columns resolve to fresh column ix (a symmetric stand-in)
  // ---- join ramp (gm_config.init_mode 2, single context): node j starts at tick j/4
  // (Application.cpp:130, STEP_RATE 0.25) and is in the group from tick j/4 + 2 if the
  // introducer (node 0) answered its JOINREQ at j/4 + 1 (ran that tick: <= intro_until).
  // A column's heartbeats are stored offset by s_hbase(j) = 2(j/4 + 1) (0 for j = 0), so
  // every live node's own heartbeat still reads 2t-1 and the narrow cell applies.
  int ramp;
  int intro_until;
  int32_t *mecol;            // [n] ramp: myPos's column this tick (self, or the updateMyPos quirk's target)
  int32_t *selfadd;          // [S_SELFADD_CAP] ramp: rows that appended their own entry this tick
  uint32_t *selfadd_cnt;
  int32_t *xcnt;             // bound exchange buffer, chunk-major: [chunk][shard_count][2^xlog][2] (present,
                             //   numfailed) per shard and row (s_xc): a row chunk's slots of every rank are
                             //   contiguous, so each chunk's all-gather is one in-place ncclAllGather
  int32_t *status;           // bound exchange buffer [n][D]: resolved draws, MAX-allreduced
  int32_t *acc;              // [n][8]: targets so far, g[5], numpot, size
  int32_t *pending;          // [n] rows still drawing
  int32_t *npending;         // rows still drawing after the last accept round
  // bounded rounds (gm_host_shard.hip tick_sharded): pending list l = 1, 2 holds the rows left after round l-1
  // (ascending after gm_s_plist_sort: the same order on every rank); statusl[l] = the bound
  // exchange buffer [plist_cap[l]][D_l] of round l's draws, by list position. Index 0 unused.
  int plist_cap[3];
  int32_t *plist[3];
  uint32_t *plist_cnt[3];
  int32_t *statusl[3];
  // ---- msgcount analogue (gm_msgcount_record, single context; nullptr = off): per tick and
  // row, gossip entries sent (fresh entries x targets, before loss) and received (after loss),
  // EmulNet's sent_msgs / recv_msgs per entry message (EmulNet.cpp:111,172)
  uint32_t *mc_sent, *mc_recv;  // [mc_tmax][n]
  uint32_t *mc_fresh;           // [2][n] fresh entries of each row's payload, by tick parity
  uint32_t *mc_rdrop;           // [n] entries a row received after keyed loss (DROP band kernel)
  int mc_tmax;
  int kcap;                     // inbox slots used (S_KMAX; lowered only by the diagnostics env GM_INBOX_CAP)
  // fast path (B = 1024, gm_s_band_fast): the units it hands back to the general path this tick,
  // by tick parity (the count of tick t+1 is zeroed during tick t); nullptr: fast path off
  uint32_t *fb_cnt;             // [2]
  int2 *fb_list;                // [nb * n]: (band, row)
  int lag_hmin;                 // a present cell with h < lag_hmin sets GM_ERR_LAG: 3 (lag > 125 ticks, the
                                // encoding's limit); the diagnostics env GM_LAG_CAP=L (L >= 15) lowers it to lag > L
  // ---- round-5 fields, kept at the end: the band kernels are short-lived waves whose first scalar
  // loads come from this struct in the kernel arguments, and fields inserted above shifted their
  // offsets and the compiler's load grouping (S-A band kernels +7 %, profiles/r05/sa_regression/)
  int esc_dense;                // the pools are dense-equivalent (no run can overflow them); gm_pool_info
  int xlog;                     // column shards: log2 of the rows per exchange chunk (rows [c << xlog, (c + 1) << xlog))
  int xk;                       // exchange chunks = ceil(n / 2^xlog)
  // gm_s_pick0 (single context, B = 1024): rows whose first 16 S2 outputs do not finish their draw go
  // to this list, which gm_s_pick then takes from output 0 (nullptr: gm_s_pick takes every row)
  int32_t *pk_list;             // [n]
  uint32_t *pk_cnt;
};

// ------------------------------------------------------------------ device helpers
// The store side of the band sweep (narrowing, escape lists, payload nibbles and escape slots),
// shared by the band kernels (gm_band.h) and the state loader's encode kernel (gm_load.hip):
// one encoder of the stored form.
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef int32_t i32x4 __attribute__((ext_vector_type(4)));
typedef uint8_t u8x16 __attribute__((ext_vector_type(16)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

// Buffer resource over [p, p + bytes) built from wave-uniform values (SGPRs): loads
// beyond `bytes` return 0 without touching memory, stores beyond it are dropped.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t gm_rsrc(const void *p, uint32_t bytes) {
  const uint64_t a = (uint64_t)p;
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)a);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(a >> 32));
  return __builtin_amdgcn_make_buffer_rsrc((void *)(((uint64_t)hi << 32) | lo), (short)0,
                                           (int)__builtin_amdgcn_readfirstlane(bytes), 0x00020000);
}
#define GM_AUX_NT 2  // non-temporal (streamed once)
#define GM_OOB 0x80000000u

// Packed 16-bit lanes of a 32-bit register: two cells per VGPR, v_pk_* arithmetic.
typedef uint16_t u16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ u16x2 pk(uint32_t v) { return __builtin_bit_cast(u16x2, v); }
__device__ __forceinline__ uint32_t unpk(u16x2 v) { return __builtin_bit_cast(uint32_t, v); }
// payload bytes 0,1 / 2,3 of a dword, zero-extended into the two halves
// a += b per u16 half, opaque to the compiler: plain vector adds of the sweep's
// per-pair counts get re-associated into a tree that keeps every pair's term live
// (9 VGPR spills at occupancy 8); an in-order chain consumes each term at once
__device__ __forceinline__ u16x2 padd(u16x2 a, u16x2 b) {
  uint32_t r;
  asm("v_pk_add_u16 %0, %1, %2" : "=v"(r) : "v"(unpk(a)), "v"(unpk(b)));
  return pk(r);
}
// min(x, 1) per u16 half as ONE v_pk_min_u16: written as plain vector min the compiler
// lowers it to a compare + select per half (5 instructions instead of 1)
__device__ __forceinline__ u16x2 pmin1(u16x2 a) {
  uint32_t r;
  asm("v_pk_min_u16 %0, %1, 1 op_sel_hi:[1,0]" : "=v"(r) : "v"(unpk(a)));
  return pk(r);
}

// stored cell bytes 0,1 (hi = 0) or 2,3 (hi = 1) of a dword, zero-extended into the two u16 halves
__device__ __forceinline__ uint32_t byte_pair(uint32_t w, int hi) {
  return __builtin_amdgcn_perm(0u, w, hi ? 0x0c030c02u : 0x0c010c00u);
}
// s_widen of two stored bytes (nz = min(x, 1)); an escape byte gives garbage, replaced by its wide cell
// (h4 << 4 | a -> 7168 + (h4 << 6) + a = x + 3 (x & 0xF0) + 7168: two multiply-adds)
__device__ __forceinline__ u16x2 widen2(u16x2 x, u16x2 nz) {
  return nz * (u16x2)(7168) + ((x & (u16x2)(0xF0)) * (u16x2)(3) + x);
}

// (row16_scan and dpp_scan, the DPP scans of a 16-lane row and of the wave, are gm_device.h's)

// Stored bytes of two swept cells (pres = min(v2, 1)): tt = v2 - (S_CELL(230, 0) - 1) (wraps below
// h = 230) = (h - 230) << 5 | (age + 1); representable iff nothing above the h field (h <= 254, no
// wrap), h even (bit 5) and age <= 14 (bit 4 of age + 1) -> h4 << 4 | age (h4 = (h - 224) / 2 =
// the tt field + 3), else S_B_ESC (bad = 1); absent 0. gm_scaled.h: a stored byte is always one
// re-base away from another byte, which the fast path of gm_s_band relies on.
__device__ __forceinline__ u16x2 narrow2(u16x2 v2, u16x2 pres, u16x2 &bad) {
  const u16x2 tt = v2 - (u16x2)(S_CELL(S_H4_MIN_H, 0) - 1);
  bad = pmin1(tt & (u16x2)(0xFC30)) & pres;
  const uint32_t tu = unpk(tt);
  const u16x2 enc = pk((tu & 0x000F000Fu) | ((tu >> 2) & 0x00F000F0u)) + (u16x2)(0x2F);
  return enc * (pres - bad) + bad;
}

// The lane's escaped cells as a mask: bit 8j + i set where byte j of stored dword i (cell 4i + j)
// is the escape code S_B_ESC (the narrowing writes no other code below 16). x = w ^ 0x01010101 has
// a zero byte exactly there (carry-free SWAR zero-byte test); the four dwords' byte flags are
// merged by shifts alone (no quarter-rate 32-bit multiply to gather them). esc_cell maps a bit
// back to its cell; the list's entries carry their columns, so their order is not significant.
__device__ __forceinline__ uint32_t esc_mask16(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3) {
  static_assert(S_B_ESC == 1u, "esc_mask16 tests for the byte 0x01");
  const uint32_t w[4] = {w0, w1, w2, w3};
  uint32_t m = 0;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const uint32_t x = w[i] ^ 0x01010101u;
    const uint32_t e = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u;  // bit 7 of each zero byte
    m |= e >> (7 - i);
  }
  return m;
}
__device__ __forceinline__ int esc_cell(int p) { return ((p & 7) << 2) | (p >> 3); }

// exclusive prefix of v over the LPR aligned lanes of this lane's row, and the row total;
// every lane of the row is active (the callers branch on row-uniform conditions only)
template <int LPR>
__device__ __forceinline__ int row_scan(int v, int li, int lane, int &total) {
  int x = v;
  if (LPR == 64) {
    x = dpp_scan(v);
    total = __builtin_amdgcn_readlane(x, 63);
  } else {
#pragma unroll
    for (int o = 1; o < LPR; o <<= 1) {
      const int y = __shfl_up(x, o, 64);
      if (li >= o) x += y;
    }
    total = __shfl(x, lane - li + LPR - 1, 64);
  }
  return x - v;
}

// any lane of this lane's row
template <int LPR>
__device__ __forceinline__ bool row_any(bool p, int sub) {
  const uint64_t b = __builtin_amdgcn_ballot_w64(p);
  return LPR == 64 ? b != 0 : ((b >> (sub * LPR)) & ((1ull << LPR) - 1)) != 0;
}

// stripe of the (band, row) list at slab + r (gm_scaled.h: striped pool allocation)
__device__ __forceinline__ int esc_stripe(const SState &s, size_t slab, int r) {
  return (int)((slab + (size_t)r) & (size_t)(s.esc_stripes - 1));
}
// The escape-list word of a (band, row) list of `total` escaped cells written at tick parity
// par: up to S_ESC_IN entries need no allocation; beyond, one reservation (the row's first lane)
// in its stripe's pool region, broadcast to the row -- 0 with GM_ERR_ESC if the region overflowed
// (the run is void). total is row-uniform.
template <int LPR>
__device__ __forceinline__ uint32_t row_alloc(const SState &s, int par, size_t slab, int r, int total, int li,
                                              int lane) {
  if (total <= S_ESC_IN) return (uint32_t)total;
  uint32_t w = 0;
  if (li == 0) {
    const int stripe = esc_stripe(s, slab, r);
    const unsigned long long need = (unsigned long long)(total - S_ESC_IN);
    const unsigned long long b = atomicAdd(s.tesc_cnt + par * s.esc_stripes + stripe, need);
    if (b + need <= (unsigned long long)s.tesc_region) w = (uint32_t)total | ((uint32_t)b << 11);
    else atomicOr(s.err, GM_ERR_ESC);
  }
  return LPR == 64 ? __builtin_amdgcn_readfirstlane(w) : (uint32_t)__shfl((int)w, lane - li, 64);
}
// a list's storage: entry i < S_ESC_IN in the inline slot, the rest in its stripe's pool region
struct EscList {
  uint32_t *inl, *pool;
  __device__ __forceinline__ uint32_t *at(int i) const { return i < S_ESC_IN ? inl + i : pool + (i - S_ESC_IN); }
};
__device__ __forceinline__ EscList esc_list(const SState &s, int par, size_t slab, int r, uint32_t word) {
  EscList l;
  l.inl = s.tesc_in[par] + (slab + (size_t)r) * S_ESC_IN;
  l.pool = s.tesc[par] + (size_t)esc_stripe(s, slab, r) * s.tesc_region + S_EW_OFF(word);
  return l;
}

// LDS of the band kernel: 32 B per lane (its 16 working cells), i.e. one wave's rows' cells in
// column order -- the meeting point of escape entries and the lanes holding their columns
#define S_LDS_WAVE_WORDS (64 * 8)
__device__ __forceinline__ void lds_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Reader: the row's list (tot entries, row-uniform) into the lanes' cells: every lane of the
// row parks its 16 cells in LDS, the row's lanes scatter the entries by column (lane li < 16
// has entry li prefetched in `ent`; entries beyond S_ESC_IN load here), then every lane takes
// its cells back. lds = this wave's area.
template <int LPR>
__device__ __forceinline__ void esc_apply(uint32_t *lds, int lane, int li, const EscList &l, int tot, uint32_t ent,
                                          u16x2 tw[8]) {
  u32x4 *mine = (u32x4 *)(lds + lane * 8);
  mine[0] = (u32x4){unpk(tw[0]), unpk(tw[1]), unpk(tw[2]), unpk(tw[3])};
  mine[1] = (u32x4){unpk(tw[4]), unpk(tw[5]), unpk(tw[6]), unpk(tw[7])};
  lds_wave_sync();
  uint16_t *row = (uint16_t *)(lds + (lane - li) * 8);  // the row's B cells in column order
  constexpr int P = LPR < S_ESC_IN ? LPR : S_ESC_IN;  // entries prefetched (one per lane)
  if (li < min(tot, P)) row[ent & 0xFFFFu] = (uint16_t)(ent >> 16);
  for (int i = P + li; i < tot; i += LPR) {  // rare: lists longer than the prefetch
    const uint32_t e = *l.at(i);
    row[e & 0xFFFFu] = (uint16_t)(e >> 16);
  }
  lds_wave_sync();
  const u32x4 a = mine[0], b = mine[1];
  tw[0] = pk(a.x); tw[1] = pk(a.y); tw[2] = pk(a.z); tw[3] = pk(a.w);
  tw[4] = pk(b.x); tw[5] = pk(b.y); tw[6] = pk(b.z); tw[7] = pk(b.w);
}

// Writer: the lane's 16 swept cells wait in its LDS slot (esc_park, right after the sweep, so
// they need no registers through the stores); its escaped cells (mask em, esc_mask16's bit order)
// become entries eoff, eoff + 1, ... of the list, a set bit's cell one dynamic LDS read (no
// register indexing).
// colb = the lane's first column in the band.
__device__ __forceinline__ void esc_park(uint32_t *lds, int lane, const uint32_t cw[8]) {
  u32x4 *mine = (u32x4 *)(lds + lane * 8);
  mine[0] = (u32x4){cw[0], cw[1], cw[2], cw[3]};
  mine[1] = (u32x4){cw[4], cw[5], cw[6], cw[7]};
}
// inl_only (row-uniform): the list fits its inline slot, so no entry needs the pool address.
// An escaped cell that is present with h < hmin (3: h <= 2, its next re-base would wrap) sets
// GM_ERR_LAG; only escaped cells can be that low (a stored byte holds h >= 226)
__device__ __forceinline__ void esc_emit(uint32_t *lds, int lane, const EscList &l, int eoff, uint32_t em, int colb,
                                         bool inl_only, uint32_t *err, int hmin) {
  if (!em) return;
  const uint16_t *cells = (const uint16_t *)(lds + lane * 8);
  int j = eoff;
  bool low = false;
  for (uint32_t m = em; m; m &= m - 1) {
    const int q = esc_cell(__builtin_ctz(m));
    const uint32_t c = cells[q];
    low |= c < (uint32_t)S_CELL(hmin, 0);
    *(inl_only ? l.inl + j : l.at(j)) = (uint32_t)(colb + q) | (c << 16);
    j++;
  }
  if (low) atomicOr(err, GM_ERR_LAG);
}
#define S_PESC_NONE 0xFFFFFFFFu  // payload escape record: no slots (overflow)

// One work unit of the band sweep: unit u = (band u / U, rows [(u % U) * RPW, +RPW)).
// unit_load issues the row metadata and the table slice; unit_gather the payload slices
// (needs the sender ids); unit_finish merges, sweeps, stores and records the counts.
template <int B>
struct UnitIn {
  int band, r, k;  // k: lists delivered to this lane's row, -1 = not merged (crashed / absent / not in the group)
  int snd[S_SB];
  u32x4 ta;        // the row's 16 cell bytes of this lane (as loaded)
  uint32_t ebase;  // the row slice's escape list in the pool of tick t-1 (S_PESC_NONE: none)
  uint32_t bz;     // the (band, row) record's count word of tick t-1 (S_BC_PRES: present cells as loaded)
  uint64_t evc;    // evcum of the (row, band) as of tick t-1 (uni: read by unit_load)
  bool uni;        // the fast path's unit: its evcum cell is written back plainly, not by an atomic
  const uint8_t *msg;     // s.msg and the inline escape entries of tick t-1, read with the row's
  const uint32_t *tesc;   // kernel-argument words (unit_load)
};

// The sweep's packed pass over the lane's 16 cells mm (16-bit cells relative to the tick being
// written, MP1Node.cpp:426-444): age >= TFAIL counts toward numfailed; fresh entries (age < TFAIL)
// form the payload sent at that tick. The swept cell is narrowed to its stored byte (S_B_ESC where
// the byte cannot hold it). A fresh stored byte h4 << 4 | a sends h' = h - 2, i.e. the nibble
// h4 - 1 (>= 2: h4 >= 3); escaped cells send the escape nibble 15 (their byte h' goes to the
// payload's wide plane). Out: cw the cells, bw their stored bytes, nwv the payload nibbles (nib_max's
// word order), the present / stale counts, badv != 0: a cell escaped, nmx the largest nibble, amax the
// largest age (TREMOVE removals are the caller's).
__device__ __forceinline__ void sweep_cells(const u16x2 mm[8], u16x2 &np2, u16x2 &nf2, u16x2 &badv, u16x2 &nmx,
                                            u16x2 &amax, u16x2 nwv[2], uint32_t cw[8], uint32_t bw[4]) {
  uint32_t bprev = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const u16x2 v = mm[i];
    const u16x2 a = v & (u16x2)(31);
    const u16x2 stale = (a + (u16x2)(32 - GM_TFAIL)) >> (u16x2)(5);  // age >= TFAIL
    amax = __builtin_elementwise_max(amax, a);  // TREMOVE removals (rare) are applied below
    const u16x2 pres = pmin1(v);
    nf2 = padd(nf2, stale);
    np2 = padd(np2, pres);
    u16x2 bad;
    const u16x2 b = narrow2(v, pres, bad);
    // payload nibble of the fresh present cells: h4 - 1, or 15 where that is 0 (h4 <= 1)
    const u16x2 p = __builtin_elementwise_sub_sat(pres, stale);
    const u16x2 qn = __builtin_elementwise_sub_sat(b >> (u16x2)(4), (u16x2)(1));
    const u16x2 nib = p * (__builtin_elementwise_sub_sat((u16x2)(1), qn) * (u16x2)(S_NIB_ESC) + qn);
    nwv[i >> 2] = nwv[i >> 2] + nib * (u16x2)(1u << (4 * (3 - (i & 3))));
    badv |= bad;
    nmx = __builtin_elementwise_max(nmx, nib);
    cw[i] = unpk(v);
    if (i & 1) bw[i >> 1] = __builtin_amdgcn_perm(unpk(b), bprev, 0x06040200u);
    else bprev = unpk(b);
  }
}

// Rare: the escaping lanes' 16 payload bytes h' (from the swept cells cw) into consecutive slots of
// this parity's payload pool (read where a receiver meets nibble 15), one reservation per row. pesc:
// this lane's nibbles hold an escape; called where some lane of the row does (row-uniform).
template <int LPR>
__device__ __forceinline__ void payload_escapes(const SState &s, int par, size_t slab, int r, int li, int lane,
                                                int sub, bool pesc, const uint32_t cw[8]) {
  const uint64_t bal = __builtin_amdgcn_ballot_w64(pesc);
  const uint64_t rm = LPR == 64 ? bal : (bal >> (sub * LPR)) & ((1ull << LPR) - 1);
  uint32_t pbase = S_PESC_NONE;
  if (li == 0) {
    const int ps = esc_stripe(s, slab, r);
    const unsigned long long b = atomicAdd(s.pesc_cnt + par * s.esc_stripes + ps, (unsigned long long)__builtin_popcountll(rm));
    if (b + (unsigned long long)__builtin_popcountll(rm) <= (unsigned long long)s.pesc_region)
      pbase = (uint32_t)ps * s.pesc_region + (uint32_t)b;
    else atomicOr(s.err, GM_ERR_ESC);
    s.pesc_rec[par][slab + r] = make_uint4(pbase, (uint32_t)rm, (uint32_t)(rm >> 32), 0u);
  }
  pbase = LPR == 64 ? __builtin_amdgcn_readfirstlane(pbase) : (uint32_t)__shfl((int)pbase, lane - li, 64);
  uint32_t pw[8];
#pragma unroll
  for (int i = 0; i < 8; i++) {  // removed cells send nothing: the swept cells suffice
    const u16x2 v = pk(cw[i]);
    const u16x2 stale = ((v & (u16x2)(31)) + (u16x2)(32 - GM_TFAIL)) >> (u16x2)(5);
    pw[i] = unpk(__builtin_elementwise_sub_sat(v >> (u16x2)(5), stale * (u16x2)(255) + (u16x2)(2)));
  }
  const u32x4 wv = {__builtin_amdgcn_perm(pw[1], pw[0], 0x06040200u), __builtin_amdgcn_perm(pw[3], pw[2], 0x06040200u),
                    __builtin_amdgcn_perm(pw[5], pw[4], 0x06040200u), __builtin_amdgcn_perm(pw[7], pw[6], 0x06040200u)};
  if (pesc && pbase != S_PESC_NONE)
    *(u32x4 *)(s.pesc[par] + ((size_t)pbase + __builtin_popcountll(rm & ((1ull << li) - 1))) * 16) = wv;
}

// The unit's commit, shared by both paths of unit_finish. unit_stores (a merged row's lanes): the
// swept slice's table bytes and payload nibbles, and its escape list; returns the list's word.
template <int B>
__device__ __forceinline__ uint32_t unit_stores(const SState &s, int t, const UnitIn<B> &in, const uint32_t bw[4],
                                                uint32_t ov0, uint32_t ov1, bool esc_row, uint32_t em, uint32_t *lds) {
  constexpr int LPR = B / S_COLS_PER_LANE;  // lanes per row
  constexpr int Q = S_COLS_PER_LANE;        // cells per lane
  const int lane = threadIdx.x & 63;
  const int par = t & 1;
  const int li = lane % LPR;
  const int band = in.band, r = in.r;
  const size_t slab = (size_t)band * s.n;
  const __amdgpu_buffer_rsrc_t trs = gm_rsrc(s.table + slab * B, (uint32_t)(s.n * B));
  const __amdgpu_buffer_rsrc_t prs = gm_rsrc(s.msg + slab * B, (uint32_t)(s.n * B));
  const uint32_t toff = (uint32_t)(r * B + li * Q);  // bytes
  uint32_t eb_out = 0;
  const u32x4 nb4 = {bw[0], bw[1], bw[2], bw[3]};
  __builtin_amdgcn_raw_buffer_store_b128(nb4, trs, toff, 0, GM_AUX_NT);
  const u32x2 ov = {ov0, ov1};
  __builtin_amdgcn_raw_buffer_store_b64(ov, prs, (uint32_t)(r * B + par * (B / 2) + li * 8), 0, GM_AUX_NT);
  if (band == 0 && li == 0) s.wtick[r] = t;
  if (esc_row) {  // the escaped cells as entries of this tick's list (the record's .w)
    int etot;
    const int eoff = row_scan<LPR>(__builtin_popcount(em), li, lane, etot);
    eb_out = row_alloc<LPR>(s, par, slab, r, etot, li, lane);
    if (eb_out != 0) esc_emit(lds, lane, esc_list(s, par, slab, r, eb_out), eoff, em, li * Q, etot <= S_ESC_IN, s.err, s.lag_hmin);
  }
  return eb_out;
}

// The band width as a compile-time constant: calls f(std::integral_constant<int, B>{}) for band = B
// and returns its hipError_t; hipErrorInvalidValue for a width no kernel is instantiated at.
template <typename F>
inline hipError_t gm_band_dispatch(int band, F &&f) {
  switch (band) {
    case 64: return f(std::integral_constant<int, 64>{});
    case 128: return f(std::integral_constant<int, 128>{});
    case 256: return f(std::integral_constant<int, 256>{});
    case 512: return f(std::integral_constant<int, 512>{});
    case 1024: return f(std::integral_constant<int, 1024>{});
    default: return hipErrorInvalidValue;
  }
}

// host launch wrappers, for the gm_host*.hip units (gm_scaled.hip, gm_band.hip, gm_draw.hip; gm_detect.hip,
// gm_load.hip, gm_census.hip, gm_read.hip). Launchers only another SCALED kernel unit calls are
// declared in gm_band.h / gm_select.h.
hipError_t gm_launch_tick(const SState &s, int t, int drop_pct, hipStream_t st, hipEvent_t k0, hipEvent_t k1,
                          bool pick);
hipError_t gm_launch_tick_prologue(const SState &s, int t, hipStream_t st, bool zero_draw = false);
hipError_t gm_launch_band_rows(const SState &s, int t, int drop_pct, int r0, int r1, hipStream_t st);
hipError_t gm_launch_xrows(const SState &s, int r0, int r1, hipStream_t st);
hipError_t gm_launch_draw0(const SState &s, int t, int r0, int r1, hipStream_t st);
hipError_t gm_launch_draw(const SState &s, int t, int round, int D, int listed, hipStream_t st, int r0 = 0, int r1 = -1);
hipError_t gm_launch_accept(const SState &s, int t, int D, int in_list, int out, hipStream_t st, int r0 = 0,
                            int r1 = -1);
hipError_t gm_launch_plist_sort(const SState &s, int l, hipStream_t st);
hipError_t gm_launch_init(const SState &s, int warm, int t0, uint64_t seed, hipStream_t st);
hipError_t gm_launch_msgcount(const SState &s, int t, bool dropped, int phase, hipStream_t st);
hipError_t gm_launch_detect(const SState &s, gm_detect_rec *rec, uint64_t *timeline, int t, hipStream_t st);
hipError_t gm_launch_census(const SState &s, gm_census_rec *rec, uint64_t *hist, uint32_t *status, int T,
                            hipStream_t st);
hipError_t gm_launch_load_check(const SState &s, int t, int r0, int cnt, const int32_t *hb, const int32_t *ts,
                                int32_t *base, int32_t *own, uint32_t *status, hipStream_t st);
hipError_t gm_launch_load_encode(const SState &s, int t, int r0, int cnt, const int32_t *hb, const int32_t *ts,
                                 const int32_t *base, hipStream_t st);
hipError_t gm_launch_load_nodes(const SState &s, int t, const int32_t *heartbeat, const int32_t *failed,
                                const int32_t *targets, const int32_t *counts, const int32_t *own, uint32_t *status,
                                int write, hipStream_t st);
hipError_t gm_launch_load_inbox(const SState &s, int t, uint32_t *status, hipStream_t st);
hipError_t gm_launch_read_decode(const SState &s, int par, int r0, int rows, int32_t *stage, uint32_t *status,
                                 hipStream_t st);
