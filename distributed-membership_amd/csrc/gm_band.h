// gm_band.h -- device side shared by the band sweep's two units (internal to the SCALED kernels):
// gm_band.hip (the general path: every band width, keyed loss, the join ramp, the listed pass) and
// gm_band_fast.hip (gm_s_band_fast, B = 1024). The row metadata and table / payload loads, the
// nibble and keyed-loss helpers, the general path's merge and sweep (unit_finish) and the unit's
// records. The store side below them is in gm_scaled.h (shared with gm_load.hip / gm_read.hip).
#pragma once
#include "gm_device.h"
#include "gm_scaled.h"

// ------------------------------------------------------------------- gm_s_band
// One wave per work unit: unit u is (band u / U, rows [(u % U) * RPW, +RPW)),
// U = ceil(n / RPW) units per band, LPR = B/8 lanes per row, 8 columns per lane.
// Units are numbered band-major, so the waves in flight cover a few consecutive
// thousand rows of one band: the band's payload slab (n * B * 2 B per parity) is
// read ~5 times per sender slice while it sits in the Infinity Cache, and HBM sees
// each payload byte about once. Each wave issues its row's metadata (crash flag,
// inbox count, first S_SB sender ids) together with its table slice, then the
// payload slices, merges, sweeps, stores and exits (short-lived waves keep more
// bytes in flight than a persistent loop; measured with scripts/ubench).
template <int B>
struct RowMeta {
  int k;           // lists delivered to the row (-1: no such row, or a crashed node)
  int snd[S_SB];   // first S_SB senders
  uint32_t ebase;  // the (band, row) record's escape-list word of the last tick (S_EW_*, 0: no escaped cells)
  uint32_t bz;     // the record's count word of the last tick (S_BC_*: the slice's present cells as stored)
  uint64_t evc;    // EVC: the (row, band)'s cumulative events (evcum), read with the metadata
  uint32_t ebase2, bz2;  // band2 >= 0: the same words of the (band2, row) record
  uint64_t evc2;         // and its evcum cell (EVC)
};

// Every load of the row's metadata issues at once, none behind a branch on another (one
// memory round trip before the payload gathers can issue, not a chain of three).
// a load through a pointer known to be global memory (a pointer out of an asm statement is no
// longer known to be one, and a generic pointer's loads are never scalar)
template <typename T>
__device__ __forceinline__ T gld(const T *p) {
#if __HIP_DEVICE_COMPILE__
  return *(const __attribute__((address_space(1))) T *)p;
#else
  return *p;  // (host pass: never executed)
#endif
}
// band2 >= 0 (one row per wave): also the record and evcum cell of the row in band2 -- loaded here,
// before the empty asm statements below, which the compiler takes for memory writes (a load after
// them is not known unclobbered and becomes a vector load)
template <int B, bool UNI, bool EVC = false>
__device__ __forceinline__ RowMeta<B> row_meta(const SState &s, int r, int par, int t, size_t slab, int band,
                                               int band2 = -1) {
  RowMeta<B> m;
  const int rc = min(r, s.n - 1);  // r >= n (a partial unit): loads stay in bounds, k = -1
  const int32_t *ibase = par ? s.inbox[1] : s.inbox[0], *cbase = par ? s.inbox_cnt[1] : s.inbox_cnt[0];
  const int32_t *fbase = s.failed;
  const uint4 *rbase = s.brec;
  const uint64_t *ecbase = s.evcum;
  int ramp = s.ramp;
  // every kernel-argument word the row's loads need, in one batch: without this the compiler
  // interleaves these (scalar-cache) loads with the row's memory loads, and a wait for one of them
  // waits for all -- the evcum cell then issued only after the inbox had arrived (a second round trip
  // before the gathers). A plain asm statement (not volatile: no memory effect assumed).
  if (UNI) asm("" : "+s"(ibase), "+s"(cbase), "+s"(fbase), "+s"(rbase), "+s"(ecbase), "+s"(ramp));
  const int32_t *ib = ibase + (size_t)rc * S_KMAX;
  const i32x4 av = gld((const i32x4 *)ib), bv = gld((const i32x4 *)(ib + 4));
  int4 a = make_int4(av.x, av.y, av.z, av.w);
  int4 b = make_int4(bv.x, bv.y, bv.z, bv.w);
  int k = gld(cbase + rc);
  int failed = gld(fbase + rc);
  const u32x4 rv = gld((const u32x4 *)(rbase + slab + rc));
  const uint4 rec = make_uint4(rv.x, rv.y, rv.z, rv.w);
  m.ebase = rec.w;
  m.bz = rec.z;
  // the fast path (one row per wave): the unit is the only writer of its evcum cell this tick, so it is read
  // here (in flight with the rest) and written back plainly -- no device-scope atomic per unit with
  // events (at the TREMOVE peak ~4 M of them held the fast path's waves: +2 ms per tick)
  m.evc = EVC ? gld(ecbase + (size_t)rc * s.nb + band) : 0ull;
  if (band2 >= 0) {
    const u32x4 rec2 = gld((const u32x4 *)(rbase + (size_t)band2 * s.n + rc));
    m.ebase2 = rec2.w;
    m.bz2 = rec2.z;
    m.evc2 = EVC ? gld(ecbase + (size_t)rc * s.nb + band2) : 0ull;
  }
  // empty asm statements that read the values here: without them the compiler sinks the
  // inbox-count load into a branch on `failed` and the sender ids behind that, two more
  // round trips before the gathers (one row per wave: scalar registers)
  if (UNI) {
    asm volatile("" : "+s"(k), "+s"(failed), "+s"(a.x), "+s"(a.y), "+s"(a.z), "+s"(a.w));
    asm volatile("" : "+s"(b.x), "+s"(b.y), "+s"(b.z), "+s"(b.w));
  } else {
    asm volatile("" : "+v"(k), "+v"(failed));
  }
  m.snd[0] = a.x; m.snd[1] = a.y; m.snd[2] = a.z; m.snd[3] = a.w;
  m.snd[4] = b.x; m.snd[5] = b.y; m.snd[6] = b.z; m.snd[7] = b.w;
  // not in the group (join ramp) or crashed: untouched
  m.k = (r >= s.n || failed || !s_ingroup(ramp, s.intro_until, r, t)) ? -1 : k;
  if (r >= s.n) m.ebase = m.ebase2 = 0;
  return m;
}

// Payload nibbles (gm_scaled.h S_NIB_*): dword w of a lane's 8-byte slice holds cells
// 8w..8w+7; cell 8w+2k sits in nibble 3-k of the low u16, cell 8w+2k+1 in nibble 3-k
// of the high u16. So v_pk_max_u16 of the dword shifted left by 4k leaves, in the top
// nibble of each u16, the max over lists of cells (8w+2k, 8w+2k+1) -- the table word
// 4w+k: max() of u16 lanes is decided by the top nibble whatever the bits below it.
__device__ __forceinline__ void nib_max(u16x2 acc[8], uint32_t x0, uint32_t x1) {
  const u16x2 a = pk(x0), b = pk(x1);
  acc[0] = __builtin_elementwise_max(acc[0], a);
  acc[1] = __builtin_elementwise_max(acc[1], a << (u16x2)(4));
  acc[2] = __builtin_elementwise_max(acc[2], a << (u16x2)(8));
  acc[3] = __builtin_elementwise_max(acc[3], a << (u16x2)(12));
  acc[4] = __builtin_elementwise_max(acc[4], b);
  acc[5] = __builtin_elementwise_max(acc[5], b << (u16x2)(4));
  acc[6] = __builtin_elementwise_max(acc[6], b << (u16x2)(8));
  acc[7] = __builtin_elementwise_max(acc[7], b << (u16x2)(12));
}
// nibble of lane cell q (0..15) in a lane slice (x0, x1)
__device__ __forceinline__ uint32_t nib_of(uint32_t x0, uint32_t x1, int q) {
  const uint32_t x = q < 8 ? x0 : x1;
  const int c = q & 7;
  return (x >> (16 * (c & 1) + 4 * (3 - (c >> 1)))) & 15u;
}
// escaped payload byte h' of lane li's cell q in sender sn's slice of tick parity pp: the
// sender's escaping lanes hold consecutive 16-byte slots from its record's base, in lane order
__device__ __forceinline__ uint32_t pesc_value(const SState &s, int pp, int band, int sn, int li, int q) {
  const uint4 rc = s.pesc_rec[pp][(size_t)band * s.n + sn];
  const uint64_t m = (uint64_t)rc.y | ((uint64_t)rc.z << 32);
  const uint32_t slot = rc.x + (uint32_t)__builtin_popcountll(m & ((1ull << li) - 1));
  return rc.x == S_PESC_NONE || slot >= s.pesc_cap ? 0u : (uint32_t)s.pesc[pp][(size_t)slot * 16 + q];
}
// payload value of a delivered cell: h' from its nibble, or from the sender's escape slots
__device__ __forceinline__ uint32_t nib_value(uint32_t nb, const SState &s, int pp, int band, int sn, int li, int q) {
  return nb == S_NIB_ESC ? pesc_value(s, pp, band, sn, li, q) : nb ? S_NIB_H(nb) : 0u;
}

// Keyed loss of the SCALED regime (build-defined; the reference drops whole messages with
// rand() % 100 < MSG_DROP_PROB * 100, EmulNet.cpp:90-94): the entry of global column c in the list
// src sent to dst at tick t_send is lost iff 16-bit half (c & 1) of fmix32(pair ^ (c >> 1) * phi) is
// below T = ceil(pct * 65536 / 100) (s_drop_thresh), pair = low word of mix64(seed ^ t_send << 48 ^
// src << 24 ^ dst): one 32-bit hash per column pair, whose halves are exactly the two u16 halves
// of the packed nibble layout (oracle/ref_cpu.c scaled_recv states the same function)
#define S_PHI 0x9E3779B9u
__device__ __forceinline__ uint32_t s_drop_pair(const SState &s, int t, int sn, int r) {
  return (uint32_t)gm_mix64(s.drop_seed ^ ((uint64_t)(uint32_t)(t - 1) << 48) ^ ((uint64_t)(uint32_t)sn << 24) ^
                            (uint64_t)(uint32_t)r);
}
__device__ __forceinline__ bool s_keep(const SState &s, int t, int sn, int r, int c, uint32_t T) {
  const uint32_t h = gm_fmix32(s_drop_pair(s, t, sn, r) ^ ((uint32_t)(c >> 1) * S_PHI));
  return ((h >> (16 * (c & 1))) & 0xFFFFu) >= T;
}
// payload nibble position of lane cell q (0..15) in its 8-byte slice (nib_max's order)
__device__ __forceinline__ constexpr int nib_pos(int q) { return 32 * (q >> 3) + 16 * (q & 1) + 4 * (3 - ((q & 7) >> 1)); }
// 0xF at the nibbles of the lane's kept cells in list sn -> row r (64 bits = the slice). Even c0:
// cells (2i, 2i+1) are a hash pair whose halves sit at the same nibble of the two u16 halves of
// dword i / 4 -- one fmix32 and four packed ops per pair; else one hash per cell (odd offsets)
__device__ __forceinline__ uint64_t s_keep_nibbles(const SState &s, int t, int sn, int r, int colb, uint32_t T,
                                                   bool agrp) {
  const uint32_t pair = s_drop_pair(s, t, sn, r);
  const int c = s.c0 + colb;
  if (T > 65535u) return 0;  // every entry lost
  if (agrp) {
    const u16x2 t2 = (u16x2)((uint16_t)T);
    uint32_t kw[2] = {0u, 0u};
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const uint32_t h = gm_fmix32(pair ^ ((uint32_t)((c >> 1) + i) * S_PHI));
      const u16x2 drop = pmin1(__builtin_elementwise_sub_sat(t2, pk(h)));  // 1 where the half is < T
      kw[i >> 2] |= unpk(((u16x2)(1) - drop) * (u16x2)(0xFu << (4 * (3 - (i & 3)))));
    }
    return (uint64_t)kw[0] | ((uint64_t)kw[1] << 32);
  }
  uint64_t km = 0;
  for (int q = 0; q < 16; q++) {
    const uint32_t h = gm_fmix32(pair ^ ((uint32_t)((c + q) >> 1) * S_PHI));
    if (((h >> (16 * ((c + q) & 1))) & 0xFFFFu) >= T) km |= 0xFull << nib_pos(q);
  }
  return km;
}
// bit 4i set where nibble i of x is non-zero
__device__ __forceinline__ uint32_t nz_nibble_bits(uint32_t x) { return (x | (x >> 1) | (x >> 2) | (x >> 3)) & 0x11111111u; }

// the unit's table slice (this lane's 16 cell bytes); r >= n: out of range -> zeros
template <int B>
__device__ __forceinline__ void unit_table(const SState &s, UnitIn<B> &in) {
  constexpr int LPR = B / S_COLS_PER_LANE, Q = S_COLS_PER_LANE;
  const int li = (threadIdx.x & 63) % LPR;
  const __amdgpu_buffer_rsrc_t trs = gm_rsrc(s.table + (size_t)in.band * s.n * B, (uint32_t)(s.n * B));
  in.ta = __builtin_amdgcn_raw_buffer_load_b128(trs, (uint32_t)(in.r * B + li * Q), 0, GM_AUX_NT);
}

// UNI: the row is wave-uniform and known to be (one row per wave, a grid-derived unit)
// in2 (one row per wave): the same row's unit in band2 -- the row's inbox, count and state are shared,
// its record words and evcum cell load with this unit's; its table slice issues later (unit_table)
template <int B, bool UNI = false, bool EVC = false, bool TWO = false>
__device__ __forceinline__ void unit_load(const SState &s, int t, int band, int ub, UnitIn<B> &in,
                                          UnitIn<B> &in2, int band2) {
  constexpr int LPR = B / S_COLS_PER_LANE, RPW = 64 / LPR;
  const int sub = (threadIdx.x & 63) / LPR;
  in.band = band;
  in.r = ub * RPW + sub;
  in.msg = s.msg;
  in.tesc = (t & 1) ? s.tesc_in[0] : s.tesc_in[1];
  if (UNI) asm("" : "+s"(in.msg), "+s"(in.tesc));
  const size_t slab = (size_t)in.band * s.n;
  // the table slice first: it is independent of the metadata, both in flight together
  unit_table<B>(s, in);
  const RowMeta<B> meta = row_meta<B, UNI, EVC>(s, in.r, t & 1, t, slab, band, TWO ? band2 : -1);
#pragma unroll
  for (int j = 0; j < S_SB; j++) in.snd[j] = meta.snd[j];
  in.k = meta.k;
  in.ebase = meta.ebase;
  in.bz = meta.bz;
  in.evc = meta.evc;
  in.uni = EVC;
  if (TWO) {
    in2.band = band2;
    in2.r = in.r;
#pragma unroll
    for (int j = 0; j < S_SB; j++) in2.snd[j] = meta.snd[j];
    in2.k = meta.k;
    in2.ebase = meta.ebase2;
    in2.bz = meta.bz2;
    in2.evc = meta.evc2;
    in2.uni = EVC;
    in2.msg = in.msg;
    in2.tesc = in.tesc;
  }
}
template <int B, bool UNI = false, bool EVC = false>
__device__ __forceinline__ void unit_load(const SState &s, int t, int band, int ub, UnitIn<B> &in) {
  unit_load<B, UNI, EVC, false>(s, t, band, ub, in, in, -1);
}

// every payload slice at once; slots j >= k read out of range (zeros = "not sent"); with them,
// lane li < 16 of a row whose slice held escaped cells fetches entry li of its list (ent)
template <int B, bool DROP>
__device__ __forceinline__ void unit_gather(const SState &s, int t, const UnitIn<B> &in, u32x2 m[S_SB], uint32_t &ent) {
  constexpr int LPR = B / S_COLS_PER_LANE;
  const int li = (threadIdx.x & 63) % LPR;
  ent = 0;
  if (li < (int)min(S_EW_TOT(in.ebase), (uint32_t)S_ESC_IN))
    ent = gld(in.tesc + ((size_t)in.band * s.n + in.r) * S_ESC_IN + li);
  const __amdgpu_buffer_rsrc_t prs = gm_rsrc(in.msg + (size_t)in.band * s.n * B, (uint32_t)(s.n * B));
  const uint32_t poff = (uint32_t)(((t & 1) ^ 1) * (B / 2) + li * 8);  // + sender * B
  const int k = min(in.k, S_KMAX);
#pragma unroll
  for (int j = 0; j < S_SB; j++)
    m[j] = __builtin_amdgcn_raw_buffer_load_b64(prs, j < k ? poff + (uint32_t)in.snd[j] * B : GM_OOB, 0, 0);
}

// unit_records (every lane): the (band, row) record (rank-select chunk counts, the row's present /
// numfailed / event counts, the escape-list word eb_out), the events, a column shard's exchange
// slot. live: the row was merged and swept (else only its record is written).
// pre (one row per wave, the fast path): the chunk counts and row totals were reduced by the caller
// (row_counts), which needed the totals first -- piece_in / pf_in, not reduced again here
struct RowCounts {
  uint64_t piece;  // present cells per 128-column chunk, one byte each
  int pf;          // the row slice's present | numfailed << 16
};
// one row per wave: the present | numfailed counts per 8-lane chunk on DPP (xor 1, xor 2 by quad_perm,
// then + the mirrored lane of the other quad), the 8 chunk words by readlane on the scalar side
__device__ __forceinline__ RowCounts row_counts(int npres, int nfail) {
  int pf = npres | (nfail << 16);
  pf += __builtin_amdgcn_update_dpp(0, pf, 0xB1, 0xF, 0xF, false);   // quad_perm [1,0,3,2]
  pf += __builtin_amdgcn_update_dpp(0, pf, 0x4E, 0xF, 0xF, false);   // quad_perm [2,3,0,1]
  pf += __builtin_amdgcn_update_dpp(0, pf, 0x141, 0xF, 0xF, false);  // row_half_mirror
  RowCounts rc;
  rc.piece = 0;
  rc.pf = 0;
#pragma unroll
  for (int c = 0; c < 8; c++) {
    const int v = __builtin_amdgcn_readlane(pf, 8 * c);
    rc.piece |= (uint64_t)(v & 0xFF) << (8 * c);
    rc.pf += v;
  }
  return rc;
}
template <int B, bool DROP>
__device__ __forceinline__ void unit_records(const SState &s, int t, const UnitIn<B> &in, bool live, uint32_t eb_out,
                                             int npres, int nfail, int nev, uint32_t evk, int nkept,
                                             const RowCounts *pre = nullptr) {
  constexpr int LPR = B / S_COLS_PER_LANE;  // lanes per row
  constexpr int Q = S_COLS_PER_LANE;        // cells per lane
  const int lane = threadIdx.x & 63;
  const int sub = lane / LPR, li = lane % LPR;
  const int band = in.band, r = in.r;
  const int colb = band * B + li * Q;  // shard-local column of this lane's first cell
  const size_t slab = (size_t)band * s.n;
  if (DROP && s.mc_rdrop) {  // msgcount: the row's kept entries (wave-uniform test)
    int v = nkept;
#pragma unroll
    for (int o = 1; o < LPR; o <<= 1) v += __shfl_xor(v, o, 64);
    if (live && li == 0 && v) atomicAdd(&s.mc_rdrop[r], (uint32_t)v);
  }
  // present cells per 64-column chunk (4 lanes) for the draw's rank-select, gathered
  // into the row's first lane: bytes 0..B/64-1 of the (band, row) record
  constexpr int CH = S_CHUNK(B), LPC = CH / Q;  // columns / lanes per rank-select chunk
  // per-row reductions over the row's LPR lanes (aligned lane segments): counts packed
  // as present | numfailed << 16 (each <= B)
  int pf = npres | (nfail << 16);
  uint64_t piece = 0;
  if (LPR == 64 && LPC == 8 && pre) {
    piece = pre->piece;
    pf = pre->pf;
  } else if (LPR == 64 && LPC == 8) {
    const RowCounts rc = row_counts(npres, nfail);
    piece = rc.piece;
    pf = rc.pf;
  } else {
    int cc = npres;
#pragma unroll
    for (int o = 1; o < LPC; o <<= 1) cc += __shfl_xor(cc, o, 64);
#pragma unroll
    for (int c = 0; c < B / CH; c++) piece |= (uint64_t)(__shfl(cc, sub * LPR + LPC * c, 64) & 0xFF) << (8 * c);
#pragma unroll
    for (int o = LPR / 2; o >= 1; o >>= 1) pf += __shfl_xor(pf, o, 64);
  }
  int x = 0, tot = 0;
  if (__builtin_amdgcn_ballot_w64(nev != 0)) {  // wave-uniform: events anywhere in this wave
    // cumulative (joins, removals) of this (row, band): ADD kinds are 01, REMOVE kinds 10
    int jr = __builtin_popcount(evk & 0x55555555u) | (__builtin_popcount(evk & 0xAAAAAAAAu) << 16);
    x = nev;
    if (LPR == 64) {  // one row per wave: inclusive scans on DPP, totals from lane 63
      x = dpp_scan(x);
      jr = dpp_scan(jr);
      tot = __builtin_amdgcn_readlane(x, 63);
      jr = __builtin_amdgcn_readlane(jr, 63);
    } else {
#pragma unroll
      for (int o = 1; o < LPR; o <<= 1) {
        const int y = __shfl_up(x, o, 64);
        if (li >= o) x += y;
      }
      tot = __shfl(x, sub * LPR + LPR - 1, 64);
#pragma unroll
      for (int o = LPR / 2; o >= 1; o >>= 1) jr += __shfl_xor(jr, o, 64);
    }
    // single writer per (row, band): one row per wave writes back the value row_meta read; otherwise
    // a no-return atomic (no wave waits on a load)
    if (live && li == 0 && jr) {
      const unsigned long long add = (unsigned long long)(jr & 0xFFFF) | ((unsigned long long)(jr >> 16) << 32);
      if (in.uni) s.evcum[(size_t)r * s.nb + band] = in.evc + add;  // the only writer of the cell (row_meta)
      else atomicAdd((unsigned long long *)&s.evcum[(size_t)r * s.nb + band], add);
    }
  }
  const int E = s.evs;
  uint32_t sbase = 0;  // one spill-ring reservation per (row, band) that overflows its slots
  if (live && li == 0 && tot > E) sbase = atomicAdd(s.ev_spill_cnt, (uint32_t)(tot - E));
  if (live && li == 0 && tot)  // the tick's total (host staging), striped partial sums
    atomicAdd(s.ev_spill_cnt + 1 + ((slab + (size_t)r) & (S_EV_STRIPES - 1)), (uint32_t)tot);
  sbase = LPR == 64 ? __builtin_amdgcn_readfirstlane(sbase) : __shfl(sbase, sub * LPR, 64);
  if (live && nev) {
    int slot = x - nev;
    uint32_t *slots = s.ev_band + ((size_t)r * s.nb + band) * E;
    for (uint32_t ek = evk; ek; ek &= ek - 1) {
      const int bit = __builtin_ctz(ek);  // low bit of a set 2-bit kind field (ADD=1, REMOVE=2)
      const int q = bit >> 1;
      const uint32_t kind = (evk >> (2 * q)) & 3u;
      const uint32_t rec = (kind << 30) | (uint32_t)(s.c0 + colb + q + 1);
      if (slot < E) {
        slots[slot] = rec;
      } else {
        const uint32_t sp = sbase + (uint32_t)(slot - E);
        if (sp < s.ev_spill_cap) s.ev_spill[sp] = ((uint64_t)(uint32_t)r << 32) | rec;
        else atomicOr(s.err, GM_ERR_EVENTS);
      }
      slot++;
    }
  }
  if (li == 0 && r < s.n) {
    // one 16-byte record per (band, row), consecutive rows adjacent: whole-line writes
    const uint32_t bc = (uint32_t)(pf & 0xFFFF) | ((uint32_t)(pf >> 16) << 11) | ((uint32_t)min(tot, 1023) << 22);
    s.brec[slab + r] = live ? make_uint4((uint32_t)piece, (uint32_t)(piece >> 32), bc, eb_out)
                            : make_uint4(0u, 0u, 0u, eb_out);
    // (a column shard's row totals for the all-gather are summed from these records by gm_s_xrows)
  }
}

template <int B, bool DROP>
__device__ __forceinline__ void unit_finish(const SState &s, int t, int drop_pct, const UnitIn<B> &in,
                                            const u32x2 m[S_SB], uint32_t ent, uint32_t *lds) {
  constexpr int LPR = B / S_COLS_PER_LANE;  // lanes per row
  constexpr int RPW = 64 / LPR;             // rows per wave
  constexpr int Q = S_COLS_PER_LANE;        // cells per lane (8 packed pairs)
  const int lane = threadIdx.x & 63;
  const int par = t & 1;
  const int sub = lane / LPR, li = lane % LPR;
  const int band = in.band, r = in.r;
  const int colb = band * B + li * Q;  // shard-local column of this lane's first cell
  const size_t slab = (size_t)band * s.n;
  // this band's slabs: table [n][B] cell bytes, payload nibbles [n][2][B/2] bytes (32-bit offsets)
  const __amdgpu_buffer_rsrc_t trs = gm_rsrc(s.table + slab * B, (uint32_t)(s.n * B));
  const __amdgpu_buffer_rsrc_t prs = gm_rsrc(s.msg + slab * B, (uint32_t)(s.n * B));
  const uint32_t toff = (uint32_t)(r * B + li * Q);  // bytes
  const uint32_t poff = (uint32_t)((par ^ 1) * (B / 2) + li * 8);  // + sender * B
  int k = in.k;
  if (k > S_KMAX) {
    if (li == 0) atomicOr(s.err, GM_ERR_INBOX);
    k = S_KMAX;
  }
  const bool live = k >= 0;
  const u32x4 ta = in.ta;
  struct {
    int snd[S_SB];
  } meta;
#pragma unroll
  for (int j = 0; j < S_SB; j++) meta.snd[j] = in.snd[j];
  // lists to merge in this wave (uniform loop bound)
  int kw = 0;
  {
    const int kl = live ? k : 0;
#pragma unroll
    for (int w = 0; w < RPW; w++) kw = max(kw, __builtin_amdgcn_readlane(kl, w * LPR));
  }
  int npres = 0, nfail = 0, nev = 0;
  int nkept = 0;     // DROP: delivered entries this lane kept after the keyed loss (msgcount)
  uint32_t evk = 0;  // 2 bits per cell: event kind
  bool esc_st = false;  // this lane stored escaped cells
  uint32_t eb_out = 0;  // the row slice's escape-list word of this tick (the record's .w)
  if (!live && in.ebase != 0) {
    // a row not swept this tick (crashed, not yet in the group) keeps its cells as they are: its
    // escape list moves to this tick's storage (row-uniform branch; entries carry their columns)
    const int etot = (int)S_EW_TOT(in.ebase);
    eb_out = row_alloc<LPR>(s, par, slab, r, etot, li, lane);
    if (eb_out != 0) {
      const EscList src = esc_list(s, par ^ 1, slab, r, in.ebase), dst = esc_list(s, par, slab, r, eb_out);
      constexpr int P = LPR < S_ESC_IN ? LPR : S_ESC_IN;  // entries prefetched (one per lane)
      if (li < min(etot, P)) *dst.at(li) = ent;
      for (int i = P + li; i < etot; i += LPR) *dst.at(i) = *src.at(i);
    }
  }
  if (live) {
    // merge key per cell = the largest delivered payload h' (0 = nothing delivered), as
    // key5 = h' << 5 (the cell with age 0) in the u16 halves of each table word
    const int32_t *ib = s.inbox[par] + (size_t)r * S_KMAX;
    u16x2 key5[8];
    {
      // DROP (keyed loss on this tick's deliveries): a list's lost entries are cleared from its
      // nibbles before the max, per (list, lane) from 4 hashes of the pair key (s_keep_bits)
      const uint32_t T = DROP ? s_drop_thresh(drop_pct) : 0u;
      const bool agrp = ((s.c0 + colb) & 1) == 0;  // shard-uniform: the lane's cells are 8 whole hash pairs
      u16x2 acc[8];
#pragma unroll
      for (int i = 0; i < 8; i++) acc[i] = (u16x2)(0);
      auto merge_list = [&](int sn, uint32_t x0, uint32_t x1) {
        if (DROP) {
          if (!(x0 | x1)) return;
          const uint64_t km = s_keep_nibbles(s, t, sn, r, colb, T, agrp);
          x0 &= (uint32_t)km;
          x1 &= (uint32_t)(km >> 32);
          if (s.mc_rdrop) nkept += __builtin_popcount(nz_nibble_bits(x0)) + __builtin_popcount(nz_nibble_bits(x1));
        }
        nib_max(acc, x0, x1);
      };
#pragma unroll
      for (int j = 0; j < S_SB; j++)
        if (j < kw) merge_list(meta.snd[j], m[j].x, m[j].y);  // slots j >= k loaded zeros
      for (int j = S_SB; j < k; j++) {  // rare: more lists than prefetched ids
        const int sn = ib[j];
        const u32x2 mv = __builtin_amdgcn_raw_buffer_load_b64(prs, poff + (uint32_t)sn * B, 0, 0);
        merge_list(sn, mv.x, mv.y);
      }
      u16x2 nmax = (u16x2)(0);
#pragma unroll
      for (int i = 0; i < 8; i++) {
        const u16x2 nb = acc[i] >> (u16x2)(12);
        nmax = __builtin_elementwise_max(nmax, nb);
        // h' = 224 + 2n for n >= 1: key5 = 7168 + 64 n, 0 for n = 0
        key5[i] = pmin1(nb) * (u16x2)(S_NIB_BASE << 5) + nb * (u16x2)(64);
      }
      if (__builtin_elementwise_max(nmax.x, nmax.y) == S_NIB_ESC) {
        // rare (cold start, JOINREQ entries, lag > 13 ticks): some list escaped a cell of
        // this lane; the exact key of those cells = max over the (kept) lists' decoded values
#pragma unroll
        for (int i = 0; i < 8; i++) {
          const u16x2 nb = acc[i] >> (u16x2)(12);
#pragma unroll
          for (int h = 0; h < 2; h++) {
            if (nb[h] != S_NIB_ESC) continue;
            const int q = 2 * i + h;
            uint32_t kv = 0;
            for (int j = 0; j < k; j++) {  // reloads (no dynamic register indexing: no scratch)
              const int sn = ib[j];
              if (DROP && !s_keep(s, t, sn, r, s.c0 + colb + q, T)) continue;
              const u32x2 mm = __builtin_amdgcn_raw_buffer_load_b64(prs, poff + (uint32_t)sn * B, 0, 0);
              kv = max(kv, nib_value(nib_of(mm.x, mm.y, q), s, par ^ 1, band, sn, li, q));
            }
            key5[i][h] = (uint16_t)(kv << 5);
          }
        }
      }
    }
    if (s.ramp && r == 0) {  // the introducer takes the JOINREQs of the nodes that started at t-1:
      // entry {hb 0, ts t} = stored heartbeat 2t (offset 2(t-1+1)) = h 255 (MP1Node.cpp:226-251)
#pragma unroll
      for (int q = 0; q < Q; q++) {
        const int c = s.c0 + colb + q;  // a real column of this shard (not row padding)
        if (c >= 1 && colb + q < s.w && s_start(c) == t - 1) key5[q >> 1][q & 1] = (uint16_t)(255u << 5);
      }
    }
    // widen the stored bytes to 16-bit cells; a row slice holding escaped cells (rare: a crashed
    // node's entries before their removal, cold-start / JOINREQ entries) takes those from its
    // list in the last tick's pool. npb: cells present as loaded (join detection below).
    const uint32_t tb4[4] = {ta.x, ta.y, ta.z, ta.w};
    u16x2 tw[8], npb = (u16x2)(0);
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const u16x2 x = pk(byte_pair(tb4[i >> 1], i & 1));
      const u16x2 nz = pmin1(x);
      npb = padd(npb, nz);
      tw[i] = widen2(x, nz);
    }
    if (in.ebase != 0)  // row-uniform: the row slice held escaped cells after the last tick
      esc_apply<LPR>(lds, lane, li, esc_list(s, par ^ 1, slab, r, in.ebase), (int)S_EW_TOT(in.ebase), ent, tw);
    // merge: re-base the cell to tick t (h -= 2, age += 1; absent stays 0), then max
    // with the delivered key (insert if absent; raise hb and stamp ts = t if newer)
    u16x2 mm[8];
#pragma unroll
    for (int i = 0; i < 8; i++)
      mm[i] = __builtin_elementwise_max(__builtin_elementwise_sub_sat(tw[i], (u16x2)(63)), key5[i]);
    const int selfc = (r >= s.c0 && r < s.c0 + s.w) ? r - s.c0 - colb : -1;
    int selfapp = -1;  // lane cell of an appended self entry: no join record (push_back, not logNodeAdd)
    if (selfc >= 0 && selfc < Q) {  // updateMyPos + heartbeat++ + myPos->setheartbeat(heartbeat++)
      const int hb = s.hbctr[r] + 1;
      s.hbctr[r] = hb + 1;
      // myPos = lower_bound(self) (MP1Node.cpp:308-322): self if present; else, by the `&&` at
      // :316, the next larger id if one is present -- that entry takes the heartbeat and ts
      // (the quirk); else self is appended. Nodes of one start tick (ids 4g..4g+3) share this
      // lane, and the quirk's target is always one of them in practice (gm_s_selfcheck turns
      // any other case into GM_ERR_SELF)
      int tq = selfc;
      uint32_t selfcell = 0;
#pragma unroll
      for (int q = 0; q < Q; q++)
        if (q == selfc) selfcell = (unpk(mm[q >> 1]) >> (16 * (q & 1))) & 0xFFFFu;
      if (selfcell == 0) {
        if (!s.ramp) {
          atomicOr(s.err, GM_ERR_SELF);
        } else {
#pragma unroll
          for (int q = Q - 1; q >= 0; q--)  // smallest present id above self in the group
            if (q > selfc && q <= (selfc | 3) && ((unpk(mm[q >> 1]) >> (16 * (q & 1))) & 0xFFFFu)) tq = q;
          if (tq == selfc) {  // appended: verify afterwards that no larger id was present
            selfapp = selfc;
            const uint32_t slot = atomicAdd(s.selfadd_cnt, 1u);
            if (slot < S_SELFADD_CAP) s.selfadd[slot] = r;
            else atomicOr(s.err, GM_ERR_SELF);
            // column shards: the other ranks check their (higher) columns in gm_s_draw
            if (s.sharded) atomicOr((uint32_t *)(s.xcnt + S_XC(s, s.shard_rank, r)), S_XC_SELFAPP);
          }
        }
      }
      if (s.ramp) s.mecol[r] = s.c0 + colb + tq;
      const int h = 255 - (2 * t - (hb + s_hbase(s.ramp, s.c0 + colb + tq)));
      if (h < s.lag_hmin || h > 255) atomicOr(s.err, GM_ERR_LAG);
#pragma unroll
      for (int i = 0; i < 8; i++) {
        if ((tq >> 1) != i) continue;
        uint32_t v = unpk(mm[i]);
        const int sh = 16 * (tq & 1);
        v = (v & ~(0xFFFFu << sh)) | ((uint32_t)S_CELL(h, 0) << sh);
        mm[i] = pk(v);
      }
    }
    // sweep (MP1Node.cpp:426-444), one packed pass: age >= TFAIL counts toward numfailed,
    // age >= TREMOVE removes; fresh entries (age < TFAIL) form the payload sent at tick t.
    // The swept cell is narrowed to its stored byte (S_B_ESC where the byte cannot hold it).
    // A fresh stored byte h4 << 4 | a sends h' = h - 2, i.e. the nibble h4 - 1 (>= 2: h4 >= 3);
    // escaped cells send the escape nibble 15 (their byte h' goes to the payload's wide plane).
    u16x2 np2 = (u16x2)(0), nf2 = (u16x2)(0), badv = (u16x2)(0), nmx = (u16x2)(0), amax = (u16x2)(0);
    u16x2 nwv[2] = {(u16x2)(0), (u16x2)(0)};
    uint32_t cw[8], bw[4];
    sweep_cells(mm, np2, nf2, badv, nmx, amax, nwv, cw, bw);  // (gm_scaled.h: shared with the state loader)
    int ngone = 0;
    uint32_t gmask = 0;  // lane cells removed this tick (bit q = cell q)
    if (__builtin_elementwise_max(amax.x, amax.y) >= GM_TREMOVE) {
      // rare: age >= TREMOVE removes (MP1Node.cpp:429-444): the removed cells' stored bytes
      // become 0 (absent) and leave the present count. They sent nothing (stale: the nibbles
      // stand) and were escaped (age > 15), so the lane's escape flag is re-taken from the stored
      // bytes. cw keeps their old cells: only the escape mask's cells and fresh cells are read
      // from it afterwards
      u16x2 ng2 = (u16x2)(0);
      uint32_t gprev = 0;
#pragma unroll
      for (int i = 0; i < 8; i++) {
        const u16x2 v = pk(cw[i]);
        const u16x2 gone = ((v & (u16x2)(31)) + (u16x2)(32 - GM_TREMOVE)) >> (u16x2)(5);
        gmask |= ((unpk(gone) & 1u) | ((unpk(gone) >> 15) & 2u)) << (2 * i);
        ng2 = padd(ng2, gone);
        const uint32_t gb = unpk(gone * (u16x2)(0xFF));  // 0xFF in the low byte of a removed cell's half
        if (i & 1) bw[i >> 1] &= ~__builtin_amdgcn_perm(gb, gprev, 0x06040200u);
        else gprev = gb;
      }
      np2 = np2 - ng2;
      ngone = (int)ng2.x + (int)ng2.y;
      badv = (u16x2)(esc_mask16(bw[0], bw[1], bw[2], bw[3]) != 0 ? 1 : 0);
    }
    esc_st = unpk(badv) != 0;
    const bool esc_row = row_any<LPR>(esc_st, sub);
    uint32_t em = 0;  // the lane's escaped cells (entries of this tick's list, emitted after the stores)
    if (esc_row) {  // rare: cells the byte cannot hold; the lane's cells wait in its LDS slot
      if (esc_st) {  // (a present cell with h <= 2 escapes: esc_emit flags it)
        em = esc_mask16(bw[0], bw[1], bw[2], bw[3]);
        esc_park(lds, lane, cw);
      }
    }
    const bool pesc = __builtin_elementwise_max(nmx.x, nmx.y) == S_NIB_ESC;
    // rare: the escaping lanes' payload bytes h' go to this tick's payload pool
    if (row_any<LPR>(pesc, sub)) payload_escapes<LPR>(s, par, slab, r, li, lane, sub, pesc, cw);
    nfail = (int)nf2.x + (int)nf2.y;
    npres = (int)np2.x + (int)np2.y;
    // joins: present after the merge (npres + ngone) but not as loaded (npb) -- the merge never
    // deletes; removals: ngone. Rare: this lane's events, as 2-bit kinds per cell
    if (npres + ngone == (int)npb.x + (int)npb.y && ngone) {
      // removals only (the crash case): REMOVE kinds (10) at the removed cells
      uint32_t x = gmask;
      x = (x | (x << 8)) & 0x00FF00FFu;
      x = (x | (x << 4)) & 0x0F0F0F0Fu;
      x = (x | (x << 2)) & 0x33333333u;
      x = (x | (x << 1)) & 0x55555555u;
      evk = x << 1;
      nev = __builtin_popcount(gmask);
    } else if (npres + ngone != (int)npb.x + (int)npb.y) {
      // joins (and possibly removals): the bytes as loaded, re-read (still in memory: the
      // stores come below) rather than kept live through the sweep for this rare path
      const u32x4 ra = __builtin_amdgcn_raw_buffer_load_b128(trs, toff, 0, 0);
      const uint32_t tb0[4] = {ra.x, ra.y, ra.z, ra.w};
#pragma unroll
      for (int q = 0; q < Q; q++) {  // from the loaded and the swept cells only (the merge never deletes:
        // present before and absent after = removed; a cell inserted this tick has age 0)
        const uint32_t before = (tb0[q >> 2] >> (8 * (q & 3))) & 0xFFu;
        const uint32_t after = (bw[q >> 2] >> (8 * (q & 3))) & 0xFFu;  // stored byte: 0 = absent
        const uint32_t ev = !before ? (after && q != selfapp ? S_EV_ADD : 0u) : (!after ? S_EV_REMOVE : 0u);
        evk |= ev << (2 * q);
      }
      nev = __builtin_popcount((evk | (evk >> 1)) & 0x55555555u);
    }
    eb_out = unit_stores<B>(s, t, in, bw, unpk(nwv[0]), unpk(nwv[1]), esc_row, em, lds);
  }
  unit_records<B, DROP>(s, t, in, live, eb_out, npres, nfail, nev, evk, nkept);
}

// the pools of tick t+1 start empty (the tick t-1 lists in them are read through their bases,
// never through the counters), and so does the fast path's hand-back list of tick t+1 (whichever
// kernel ran tick t: a keyed-loss tick between two fast ticks must not leave a count behind); one
// wave of the tick's first band kernel
__device__ __forceinline__ void band_reset_pools(const SState &s, int t) {
  const int S = s.esc_stripes;
  for (int i = threadIdx.x; i < S; i += 64) {
    s.tesc_cnt[((t & 1) ^ 1) * S + i] = 0;
    s.pesc_cnt[((t & 1) ^ 1) * S + i] = 0;
  }
  if (s.fb_cnt && threadIdx.x == 0) s.fb_cnt[(t & 1) ^ 1] = 0;
}

// launcher only another SCALED unit calls (gm_launch_tick):
// the join ramp's check of the tick's self appends, and the fill of their count (gm_band.hip)
void gm_launch_selfcheck(const SState &s, hipStream_t st);
