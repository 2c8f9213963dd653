// gm_band_fast.hip -- the band sweep's fast path (B = 1024, no keyed loss, no join ramp): the merge
// and the sweep on the stored bytes themselves, one row per wave (unit_fast), and its kernel
// gm_s_band_fast. The units it hands back go to gm_s_band_listed (gm_band.hip).
// Compiled as part of gm_band.hip, which includes this file and launches the kernel (launch_band_b):
// as a unit of its own the kernel's register allocation and schedule change.
#include "gm_band.h"

// ------------------------------------------------------------ gm_s_band fast path
// Lane-mask bit p in esc_mask16's order is cell esc_cell(p); esc_bit is the inverse.
__device__ __forceinline__ int esc_bit(int q) { return ((q & 3) << 3) | (q >> 2); }
// One marked cell of the fast path, exactly (16-bit cell c: the merged byte y widened, or the escaped
// cell re-based and merged; the general path's arithmetic): its stored byte, payload nibble (high-
// nibble form), whether it is removed (TREMOVE) or needs the wide payload plane (bail), and the
// corrections of the SWAR pass's present / stale counts, which counted the byte y.
struct FastCell {
  uint32_t nbyte, nib, c;
  bool gone, bail;
  int dpres, dfail;
};
__device__ __forceinline__ FastCell fast_cell(const SState &s, int t, uint32_t y, uint32_t c, bool self, int hbself) {
  FastCell o;
  if (self) {  // heartbeat++; myPos->setheartbeat(heartbeat++) (MP1Node.cpp:412-415)
    if (c == 0) atomicOr(s.err, GM_ERR_SELF);  // converged start: the own entry is always present
    const int h = 255 - (2 * t - hbself);
    if (h < s.lag_hmin || h > 255) atomicOr(s.err, GM_ERR_LAG);
    c = (uint32_t)S_CELL(h, 0) & 0xFFFFu;
  }
  // branch-free (selects, not exec-mask branches: the scalar unit is what a divergent branch costs)
  const uint32_t age = c & 31u, h = c >> 5, hp = h - 2u;
  const bool pres = c != 0, stale = pres && age >= GM_TFAIL;
  o.gone = pres && age >= GM_TREMOVE;  // TREMOVE (MP1Node.cpp:429-444): absent; it sent nothing (stale)
  const bool keep = pres && !o.gone;
  const bool fits = h >= S_H4_MIN_H && !(h & 1u) && age <= S_AGE_MAX_B;  // s_narrow's test
  o.nbyte = keep ? (fits ? ((((h - 224u) >> 1) << 4) | age) : S_B_ESC) : 0u;
  // fresh: the nibble of h' = h - 2, or the wide plane (general path)
  const bool fresh = keep && !stale;
  const bool nibok = !(hp & 1u) && hp >= S_NIB_H(1) && hp <= S_NIB_H(14);
  o.bail = fresh && !nibok;
  o.nib = fresh && nibok ? ((hp - S_NIB_BASE) >> 1) << 4 : 0u;
  o.c = c;
  const bool fpres = y >= 16u, fstale = fpres && (y & 15u) >= GM_TFAIL;
  o.dpres = (int)(pres && !o.gone) - (int)fpres;
  o.dfail = (int)stale - (int)fstale;
  return o;
}
// gm_s_band's fast path (one row per wave; no keyed loss, no join ramp): the merge and the sweep on
// the stored bytes themselves. A stored byte x = h4 << 4 | a (h4 >= 3, a <= 14: gm_scaled.h) re-based
// by one tick is x - 15 (h4 - 1, a + 1) and a delivered nibble n is the byte n << 4 (h' = 224 + 2n,
// age 0); bytes order as their cells do, so the merge of updatelistCallBack (MP1Node.cpp:278-299) is
// max(sat(x - 15), n << 4), and the sweep's counts (MP1Node.cpp:426-444) and the payload nibbles of
// sendMemberList (MP1Node.cpp:360-395: the fresh cells' h4 - 1) come from SWAR over the packed
// result, four cells per instruction. The rare cells are marked and redone one by one with the 16-bit
// cell, as the general path computes them: escaped cells (their value is the row slice's escape
// list's), results a byte cannot hold (age 15, h4 <= 2: they escape, or are removed at TREMOVE), and
// the row's own cell (heartbeat bump). A delivered escape nibble, or a fresh cell whose payload needs
// the wide plane, sends the whole wave to the general path: the function then returns false before
// any global store. Returns true when the unit is done.
// nxt: called at most once, as soon as the payload words m are consumed (or not needed): the wave's
// next unit issues its table slice and payload gathers into m there, in flight under this unit's sweep
// (a unit handed to the general path may return before it: the caller then issues them).
template <int B, typename F>
__device__ __forceinline__ bool unit_fast(const SState &s, int t, const UnitIn<B> &in, const u32x2 m[S_SB],
                                          uint32_t ent, uint32_t *lds, uint32_t *park, F &&nxt) {
  static_assert(B / S_COLS_PER_LANE == 64, "the fast path takes one row per wave");
  constexpr int Q = S_COLS_PER_LANE;
  const int lane = threadIdx.x & 63, li = lane;
  const int par = t & 1;
  const int band = in.band, r = in.r;
  const int colb = band * B + li * Q;  // shard-local column of this lane's first cell
  const size_t slab = (size_t)band * s.n;
  const int k = in.k;  // wave-uniform
  if (k > S_KMAX || s.ramp) return false;  // inbox error / join ramp: general path (nxt: as for a bail)
  if (k < 0) {  // a row not merged this tick (crashed): its cells stay as they are, its escape list moves
    nxt();        // to this tick's storage (entries carry their columns), its record is written
    uint32_t eb_out = 0;
    if (in.ebase != 0) {
      const int etot = (int)S_EW_TOT(in.ebase);
      eb_out = row_alloc<64>(s, par, slab, r, etot, li, lane);
      if (eb_out != 0) {
        const EscList src = esc_list(s, par ^ 1, slab, r, in.ebase), dst = esc_list(s, par, slab, r, eb_out);
        if (li < min(etot, S_ESC_IN)) *dst.at(li) = ent;
        for (int i = S_ESC_IN + li; i < etot; i += 64) *dst.at(i) = *src.at(i);
      }
    }
    unit_records<B, false>(s, t, in, false, eb_out, 0, 0, 0, 0u, 0);
    return true;
  }
  // 1. the delivered lists: per cell pair the largest nibble, in the top nibble of each u16 (nib_max)
  u16x2 acc[8];
#pragma unroll
  for (int i = 0; i < 8; i++) acc[i] = (u16x2)(0);
#pragma unroll
  for (int j = 0; j < S_SB; j++)
    if (j < k) nib_max(acc, m[j].x, m[j].y);  // slots j >= k loaded zeros
  if (k > S_SB) {  // more lists than prefetched ids (a Poisson tail: ~7 % of rows at fanout 5)
    const __amdgpu_buffer_rsrc_t prs = gm_rsrc(s.msg + slab * B, (uint32_t)(s.n * B));
    const uint32_t poff = (uint32_t)((par ^ 1) * (B / 2) + li * 8);
    const int32_t *ib = s.inbox[par] + (size_t)r * S_KMAX;
    for (int j = S_SB; j < k; j++) {
      const int sn = ib[j];
      const u32x2 mv = __builtin_amdgcn_raw_buffer_load_b64(prs, poff + (uint32_t)sn * B, 0, 0);
      nib_max(acc, mv.x, mv.y);
    }
  }
  {
    u16x2 amx = acc[0];
#pragma unroll
    for (int i = 1; i < 8; i++) amx = __builtin_elementwise_max(amx, acc[i]);
    if (__builtin_amdgcn_ballot_w64(__builtin_elementwise_max(amx.x, amx.y) >= (uint16_t)(S_NIB_ESC << 12)))
      return false;  // a delivered escape nibble: its value is in the sender's wide plane
  }
  // 2. re-base and merge, two cells per u16x2, packed back to bytes
  const uint32_t tb4[4] = {in.ta.x, in.ta.y, in.ta.z, in.ta.w};
  uint32_t bw[4], yprev = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const u16x2 x = pk(byte_pair(tb4[i >> 1], i & 1));
    const u16x2 kb = (acc[i] >> (u16x2)(8)) & (u16x2)(0xF0);
    const u16x2 y = __builtin_elementwise_max(__builtin_elementwise_sub_sat(x, (u16x2)(15)), kb);
    if (i & 1) bw[i >> 1] = __builtin_amdgcn_perm(unpk(y), yprev, 0x06040200u);
    else yprev = unpk(y);
  }
  // 3. SWAR over the merged bytes: present (h4 >= 1) and stale (age >= TFAIL) counts, payload nibbles
  // (fresh present cells: h4 - 1, in the byte's high nibble), and the cells to redo
  int npres = 0, nfail = 0;
  uint32_t nb[4], spm = 0;
#pragma unroll
  for (int w = 0; w < 4; w++) {
    const uint32_t v = bw[w];
    const uint32_t lo = v & 0x0F0F0F0Fu;
    const uint32_t st = (lo + 0x01010101u * (16 - GM_TFAIL)) & 0x10101010u;  // age >= TFAIL
    const uint32_t a15 = (lo + 0x01010101u) & 0x10101010u;                   // age 15: not a byte next tick
    const uint32_t hi = v & 0xF0F0F0F0u;
    const uint32_t hs = hi >> 1;
    const uint32_t pr = (hs + 0x78787878u) & 0x80808080u;  // h4 >= 1: present
    const uint32_t g3 = (hs + 0x68686868u) & 0x80808080u;  // h4 >= 3
    nfail += __builtin_popcount(st);
    npres += __builtin_popcount(pr);
    spm |= ((pr & ~g3) | (a15 << 3)) >> (7 - w);  // esc_mask16's bit order
    uint32_t st4 = st << 4;
    asm volatile("" : "+v"(st4));  // else (st << 4) - st becomes a quarter-rate multiply by 15
    nb[w] = (hi - (pr >> 3)) & ~(st4 - st);
  }
  const int selfc = (r >= s.c0 && r < s.c0 + s.w) ? r - s.c0 - colb : -1;
  const bool selflane = selfc >= 0 && selfc < Q;
  int hbself = 0;
  if (selflane) {
    spm |= 1u << esc_bit(selfc);
    hbself = s.hbctr[r] + 1;
  }
  // 4. the marked cells, exactly (fast_cell). The lane's merged bytes and nibble bytes wait in LDS
  // (park: 32 B per lane), so that a cell is one byte read and two byte writes there, not register
  // selects. Escaped cells go entry-parallel: lane j takes entry j of the row slice's escape list (the
  // entries carry their columns) and that column's parked byte, whichever lane holds it; what the
  // holding lane needs back (that its cell was escaped, its removal bits, its count corrections) meets
  // in that lane's three words `cor` (LDS or / add). The other marked cells (age 15, h4 <= 2, the own
  // cell) are taken one by one in their own lane. An escaped cell that stays escaped is this tick's
  // list entry straight from its entry lane (sv / sent: VALU issue is what these ticks spend, and
  // the wave pays every instruction of a per-lane loop at its longest lane); past 64 entries (a cold
  // start) they go through the row's 16-bit cells like the per-lane loop's new ones.
  int ngone = 0;
  uint32_t gmask = 0, em = 0, sent = 0;
  bool sv = false, epar = true;
  const bool eslice = in.ebase != 0;  // row-uniform
  // 4a. the crash window's common case, without the park: no other cell is marked, the list fits its
  // inline slot, every escaped cell is stale and no delivered list has a fresh entry at its column
  // (its merged byte is 0). Then an escaped cell is only re-based (c - 63): it stays escaped -- its
  // entry lane writes it to this tick's list -- or reaches TREMOVE (a removal: the uniform loop over
  // the gone entries), and its holding lane restores the escape byte and counts the cell present
  // and stale, as fast_cell would (y = 0: dpres = dfail = 1; removed: dpres = 0, dfail = 1).
  bool quick = false;
  if (eslice && S_EW_TOT(in.ebase) <= S_ESC_IN && !__builtin_amdgcn_ballot_w64(spm != 0)) {
    const int etot = (int)S_EW_TOT(in.ebase);
    // 0x80 in the bytes whose stored cell is escaped (byte == S_B_ESC), exact per byte (recomputed
    // below rather than held across the ballot: registers are what sets this kernel's occupancy);
    // an escaped column is loud when its merged byte (the delivered nibble << 4) has a nonzero high
    // nibble -- the SWAR pass's present test on bw, no multiply
    auto esc_bytes = [&](int w) {
      const uint32_t z = tb4[w] ^ (0x01010101u * S_B_ESC);
      return ~(((z & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | z) & 0x80808080u;
    };
    bool loud = false;
#pragma unroll
    for (int w = 0; w < 4; w++) loud |= ((((bw[w] >> 1) & 0x78787878u) + 0x78787878u) & esc_bytes(w)) != 0u;
    const bool ent_lane = li < etot;
    const uint32_t ev = ent_lane ? ent >> 16 : 0u;
    const uint32_t c = ev ? ev - 63u : 0u;  // the re-based cell (y = 0 delivers nothing)
    const bool gone = ent_lane && (c & 31u) >= GM_TREMOVE;
    const bool fresh = ent_lane && (c & 31u) < GM_TFAIL;
    if (!__builtin_amdgcn_ballot_w64(loud || fresh)) {
      quick = true;
      int ne = 0;
#pragma unroll
      for (int w = 0; w < 4; w++) {
        const uint32_t eb = esc_bytes(w);
        static_assert(S_B_ESC == 1u, "the escape byte is restored as the detection mask's low bit");
        bw[w] |= eb >> 7;  // the escape byte S_B_ESC = 1 back (the merged byte there was 0)
        ne += __builtin_popcount(eb);
      }
      npres += ne;
      nfail += ne;
      const uint32_t col = ent & 0xFFFFu;
      if (__builtin_amdgcn_ballot_w64(gone)) {
        // TREMOVE ticks: each gone entry's lane sets, in the holding lane's LDS words, its cell's removal
        // bit and a 0xFF over its byte (one scatter for all of them -- a uniform step per gone entry
        // cost ~6 VALU each, ~5 per unit at the peak); the holding lanes read their words back. The
        // wave's LDS is free here: the quick path parks nothing, and stores no escape bytes (em = 0)
        uint32_t *gw = lds;                    // [64] removal bits per lane (cell order)
        u32x4 *gbm = (u32x4 *)(lds + 64);      // [64][4] byte masks per lane (cell 4w + b: byte b of word w)
        gw[li] = 0u;
        gbm[li] = (u32x4){0u, 0u, 0u, 0u};
        lds_wave_sync();
        if (gone) {
          const uint32_t ol = col / Q, q = col % Q;
          atomicOr(gw + ol, 1u << q);
          atomicOr(lds + 64 + 4 * ol + (q >> 2), 0xFFu << (8 * (q & 3)));
        }
        lds_wave_sync();
        gmask = gw[li];
        const u32x4 bm = gbm[li];
        lds_wave_sync();  // read back before any later use of the wave's LDS
        ngone = __builtin_popcount(gmask);
        npres -= ngone;
        bw[0] &= ~bm.x;  // the removed cells' bytes to 0 (absent)
        bw[1] &= ~bm.y;
        bw[2] &= ~bm.z;
        bw[3] &= ~bm.w;
      }
      sv = ent_lane && !gone;
      sent = col | (c << 16);
    }
  }
  const bool slow = !quick && (eslice || __builtin_amdgcn_ballot_w64(spm != 0));
  if (slow) {
    uint16_t *row16 = (uint16_t *)lds;  // the wave's LDS: a 16-bit cell per column (lane li: [16 li, +16))
    u32x4 *pk4 = (u32x4 *)(park + li * 8);
    pk4[0] = (u32x4){bw[0], bw[1], bw[2], bw[3]};
    pk4[1] = (u32x4){nb[0], nb[1], nb[2], nb[3]};
    uint8_t *pall = (uint8_t *)park;  // lane l's cell q: byte 32 l + q, its nibble byte 32 l + 16 + q
    uint8_t *pb = pall + li * 32;
    // per lane: cor[li] = its escaped cells as loaded (esc order), cor[64 + li] = removal bits (cell
    // order), cor[128 + li] = the present / stale corrections, packed as dpres + dfail << 16
    uint32_t *cor = park + S_LDS_WAVE_WORDS;
    if (eslice) cor[li] = cor[64 + li] = cor[128 + li] = 0u;
    lds_wave_sync();
    bool bail = false;
    uint32_t escm = 0;  // this lane's escaped cells (esc order): the entry lanes took them
    if (eslice) {
      const int tot = (int)S_EW_TOT(in.ebase);
      epar = tot <= 64;
      const int selfb = r - s.c0 - band * B;  // the own column in the band (row-uniform), if in [0, B)
      const int hbs = (selfb >= 0 && selfb < B) ? __builtin_amdgcn_readlane(hbself, selfb / Q) : 0;
      const EscList l = esc_list(s, par ^ 1, slab, r, in.ebase);
      for (int j0 = 0; j0 < tot; j0 += 64) {
        const int j = j0 + li;
        if (j < tot) {
          const uint32_t e = j < S_ESC_IN ? ent : *l.at(j);  // lane li < S_ESC_IN prefetched entry li
          const int col = (int)(e & 0xFFFFu), q = col % Q, ol = col / Q;
          uint8_t *cb = pall + ol * 32 + q;
          const uint32_t y = cb[0];  // the merged byte of an escaped cell: the delivered key alone
          const uint32_t ev = e >> 16;
          const FastCell o = fast_cell(s, t, y, max(ev ? ev - 63u : 0u, s_widen(y)), col == selfb, hbs);
          bail |= o.bail;
          // the holding lane's words, unconditionally (LDS ops with zero operands, no branches)
          atomicOr(cor + ol, 1u << esc_bit(q));
          atomicOr(cor + 64 + ol, o.gone ? 1u << q : 0u);
          atomicAdd(cor + 128 + ol, (uint32_t)(o.dpres + o.dfail * 65536));
          cb[0] = (uint8_t)o.nbyte;
          cb[16] = (uint8_t)o.nib;
          const bool eout = o.nbyte == S_B_ESC;  // an entry of this tick's list
          if (epar) {
            sv = eout;
            sent = (uint32_t)col | (o.c << 16);
          } else if (eout) {
            row16[col] = (uint16_t)o.c;  // esc_emit reads it here (em: the escape bytes, below)
          }
        }
      }
      lds_wave_sync();
      escm = cor[li];
    }
    for (uint32_t mm = spm & ~escm; mm; mm &= mm - 1) {
      const int p = __builtin_ctz(mm), q = esc_cell(p);
      const uint32_t y = pb[q];  // the merged byte (exact: the stored cell did not escape)
      const FastCell o = fast_cell(s, t, y, s_widen(y), q == selfc, hbself);
      bail |= o.bail;
      if (o.gone) {
        gmask |= 1u << q;
        ngone++;
      }
      if (o.nbyte == S_B_ESC) {
        em |= 1u << p;
        row16[li * Q + q] = (uint16_t)o.c;
      }
      npres += o.dpres;
      nfail += o.dfail;
      pb[q] = (uint8_t)o.nbyte;
      pb[16 + q] = (uint8_t)o.nib;
    }
    if (__builtin_amdgcn_ballot_w64(bail)) return false;  // (nxt not called: the caller issues it)
    lds_wave_sync();  // other lanes' entries wrote into this lane's park and words
    if (eslice) {
      const uint32_t ge = cor[64 + li], cd = cor[128 + li];
      gmask |= ge;
      ngone += __builtin_popcount(ge);
      const int dp = (int)(int16_t)(cd & 0xFFFFu);
      npres += dp;
      nfail += ((int)cd - dp) >> 16;
    }
    const u32x4 b0 = pk4[0], b1 = pk4[1];
    bw[0] = b0.x; bw[1] = b0.y; bw[2] = b0.z; bw[3] = b0.w;
    nb[0] = b1.x; nb[1] = b1.y; nb[2] = b1.z; nb[3] = b1.w;
    if (!epar) em = esc_mask16(bw[0], bw[1], bw[2], bw[3]);  // every escape byte: row16 holds its cell
  }
  // payload words in nib_max's order: the high nibbles of cells [4, 0, 5, 1] | those of [6, 2, 7, 3]
  // shifted down, for cells 0..7 and likewise 8..15
  const uint32_t ov0 = __builtin_amdgcn_perm(nb[1], nb[0], 0x01050004u) | (__builtin_amdgcn_perm(nb[1], nb[0], 0x03070206u) >> 4);
  const uint32_t ov1 = __builtin_amdgcn_perm(nb[3], nb[2], 0x01050004u) | (__builtin_amdgcn_perm(nb[3], nb[2], 0x03070206u) >> 4);
  // 5. events: removals = gmask; joins = cells present now but absent as loaded -- there are some iff
  // the slice's present cells before the sweep (npres + ngone over the row) differ from the count
  // the record kept of the last tick (first tick after gm_s_init: no count kept, so the cells are
  // compared; they are always compared where any differ)
  int nev = 0;
  uint32_t evk = 0;
  // (the record's chunk counts and totals, reduced once here: their present total is the sweep's, and
  // the removals are added only where there are some)
  const RowCounts rcnt = row_counts(npres, nfail);
  int tot = rcnt.pf & 0xFFFF;
  if (__builtin_amdgcn_ballot_w64(ngone != 0)) {
    int g = ngone;
    g += __builtin_amdgcn_update_dpp(0, g, 0xB1, 0xF, 0xF, false);   // quad_perm [1,0,3,2]
    g += __builtin_amdgcn_update_dpp(0, g, 0x4E, 0xF, 0xF, false);   // quad_perm [2,3,0,1]
    g += __builtin_amdgcn_update_dpp(0, g, 0x141, 0xF, 0xF, false);  // row_half_mirror
    g += __builtin_amdgcn_update_dpp(0, g, 0x140, 0xF, 0xF, false);  // row_mirror
    tot += __builtin_amdgcn_readlane(g, 0) + __builtin_amdgcn_readlane(g, 16) + __builtin_amdgcn_readlane(g, 32) +
           __builtin_amdgcn_readlane(g, 48);
  }
  if (tot != (int)S_BC_PRES(in.bz)) {
#pragma unroll
    for (int q = 0; q < Q; q++) {
      const uint32_t before = (tb4[q >> 2] >> (8 * (q & 3))) & 0xFFu;
      const uint32_t after = (bw[q >> 2] >> (8 * (q & 3))) & 0xFFu;  // 0 = absent
      const uint32_t ev = !before ? (after ? S_EV_ADD : 0u) : (!after ? S_EV_REMOVE : 0u);
      evk |= ev << (2 * q);
    }
    nev = __builtin_popcount((evk | (evk >> 1)) & 0x55555555u);
  } else if (ngone) {  // removals only (the crash case): REMOVE kinds (10) at the removed cells
    uint32_t x = gmask;
    x = (x | (x << 8)) & 0x00FF00FFu;
    x = (x | (x << 4)) & 0x0F0F0F0Fu;
    x = (x | (x << 2)) & 0x33333333u;
    x = (x | (x << 1)) & 0x55555555u;
    evk = x << 1;
    nev = ngone;
  }
  // 6. commit: the table and payload stores (the general path's), then this tick's escape list --
  // the entry lanes' survivors first (ballot rank), the lanes' escape bytes after them (esc_emit)
  nxt();  // the next unit's loads: in flight under this unit's stores
  if (selflane) s.hbctr[r] = hbself + 1;
  uint32_t eb_out = unit_stores<B>(s, t, in, bw, ov0, ov1, false, 0u, lds);
  const uint64_t svb = __builtin_amdgcn_ballot_w64(sv);
  const bool emany = __builtin_amdgcn_ballot_w64(em != 0) != 0;
  if (svb || emany) {
    const int ns = __builtin_popcountll(svb);
    int etot = ns, eoff = 0;
    if (emany) {
      eoff = row_scan<64>(__builtin_popcount(em), li, lane, etot);
      etot += ns;
    }
    eb_out = row_alloc<64>(s, par, slab, r, etot, li, lane);
    if (eb_out != 0) {
      const EscList l = esc_list(s, par, slab, r, eb_out);
      if (sv) {
        *l.at(lanes_below(svb)) = sent;
        if ((sent >> 16) < (uint32_t)S_CELL(s.lag_hmin, 0)) atomicOr(s.err, GM_ERR_LAG);
      }
      if (emany) esc_emit(lds, lane, l, ns + eoff, em, li * Q, etot <= S_ESC_IN, s.err, s.lag_hmin);
    }
  }
  unit_records<B, false>(s, t, in, true, eb_out, npres, nfail, nev, evk, 0, &rcnt);
  return true;
}

// The fast path's kernel (B = 1024, no keyed loss, no join ramp): every unit takes unit_fast; a
// unit it hands back (not merged, a delivered escape nibble, a payload for the wide plane) goes to
// s.fb_list for gm_s_band's listed pass right after, untouched. The list of tick t+1 starts empty.
// CH: a row chunk [u0, u1) of the pipelined column-shard tick; otherwise every row (no unit bounds
// among the kernel arguments: the wave's first loads issue as in round 4's codegen)
// Held to 7 waves per SIMD (72 VGPRs; the crash-window quick path alone would take 75, occupancy 6).
// BPW: bands per wave (blockIdx.y = a group of BPW bands). With 2, the wave's second unit is the same
// row in the next band: it shares the row's metadata (one round trip, not two), and its table slice
// and payload gathers issue as soon as the first unit's payload words are merged (nxt), so they are
// in flight under the first unit's sweep and stores -- one dependent round trip per unit instead of
// two (inbox, then gathers).
#ifndef GM_FAST_WG
#define GM_FAST_WG 1  // waves per workgroup of gm_s_band_fast (1: a finished wave frees its LDS slice at once;
                      // 4: 3.29 ms per S-A tick, 1: 3.22, profiles/r06/ab_fwg/)
#endif
// XS: the row interleave of the grid's x. Workgroups are dealt to the XCDs round-robin in practice (no
// promise of HIP's: only the speed rests on it), so with XS = 8 one XCD walks consecutive rows of a band
// pair: the rows' shared metadata lines (16 rows per line of the crash flag and of the inbox count, 4
// per line of records) are fetched into one L2, not eight, and the record stores fill their lines in
// one L2. 1: rows in grid order.
#ifndef GM_FAST_XS
#define GM_FAST_XS 8
#endif
#ifndef GM_FAST_MINW
#define GM_FAST_MINW 7  // gm_s_band_fast's waves per SIMD (72 VGPRs at 7)
#endif
#ifndef GM_FAST_BPW
#define GM_FAST_BPW 2  // bands per wave of gm_s_band_fast (profiles/r05/ab4, ab5: 3.38 vs 3.48 ms at one)
#endif
template <int B, bool CH, int BPW>
__global__ __launch_bounds__(64 * GM_FAST_WG) __attribute__((amdgpu_waves_per_eu(GM_FAST_MINW, 8))) void gm_s_band_fast(SState s, int t, int u0, int u1) {
  if (!CH) {
    u0 = 0;
    u1 = s.n;
  }
  const int wv = GM_FAST_WG == 1 ? 0 : (int)(threadIdx.x >> 6);
  // wave w of the grid's x takes row u0 + (w % XS) * q + w / XS: the XS stripes of q consecutive rows
  // interleave over the grid, so the workgroups XS apart walk one stripe row by row
  const uint32_t w = (uint32_t)((int)blockIdx.x * GM_FAST_WG + wv);
  const uint32_t q = (uint32_t)(u1 - u0 + GM_FAST_XS - 1) / GM_FAST_XS;
  const int ub = __builtin_amdgcn_readfirstlane(u0 + (int)((w % GM_FAST_XS) * q + w / GM_FAST_XS));
  if ((GM_FAST_WG > 1 && w / GM_FAST_XS >= q) || ub >= u1) return;  // whole wave (one row per wave)
  // per wave: escape cells by column, the park, the per-lane words of the escaped cells' outcomes
  constexpr int W = 2 * S_LDS_WAVE_WORDS + 192;
  __shared__ uint32_t lds_all[GM_FAST_WG * W];
  uint32_t *lds = lds_all + wv * W;
  const int b0 = (int)blockIdx.y * BPW;
  const bool two = BPW == 2 && b0 + 1 < s.nb;  // wave-uniform
  UnitIn<B> in, in2;
  unit_load<B, true, true, BPW == 2>(s, t, b0, ub, in, in2, two ? b0 + 1 : b0);
  u32x2 m[S_SB];
  uint32_t ent, ent2 = 0;
  unit_gather<B, false>(s, t, in, m, ent);
  bool issued = false;  // wave-uniform
  const bool ok = unit_fast<B>(s, t, in, m, ent, lds, lds + S_LDS_WAVE_WORDS, [&]() {
    if (two) {
      unit_table<B>(s, in2);
      unit_gather<B, false>(s, t, in2, m, ent2);
    }
    issued = true;
  });
  if (!ok && (threadIdx.x & 63) == 0) {
    const uint32_t slot = atomicAdd(&s.fb_cnt[t & 1], 1u);  // < the units of a tick: the list's size
    s.fb_list[slot] = make_int2(b0, ub);
  }
  if (two) {
    if (!issued) {  // the first unit went to the general path before its payload words were consumed
      unit_table<B>(s, in2);
      unit_gather<B, false>(s, t, in2, m, ent2);
    }
    lds_wave_sync();  // the first unit's LDS reads are done before the second one's writes
    if (!unit_fast<B>(s, t, in2, m, ent2, lds, lds + S_LDS_WAVE_WORDS, []() {}) && (threadIdx.x & 63) == 0) {
      const uint32_t slot = atomicAdd(&s.fb_cnt[t & 1], 1u);
      s.fb_list[slot] = make_int2(b0 + 1, ub);
    }
  }
  if (ub == 0 && blockIdx.y == 0) band_reset_pools(s, t);
}
