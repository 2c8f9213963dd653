// gm_partial_node.h -- one node's PARTIAL tick on one wave (p_node, a sequence of stages) and what it
// stands on: the table constants, the wave helpers, the LDS table insert, the row-shard owner and the
// preloaded values. Included by gm_partial.hip (the tick kernels) and gm_partial_xchg.hip (p_owner,
// p_aged). The stages are numbered as in gm_partial.hip's overview.
#pragma once
#include <type_traits>

#include "gm_device.h"
#include "gm_partial.h"

#define P_IDMASK 0x01FFFFFFu  // ids <= 2^25
#define P_OWN 0x80000000u     // table id-word flag: the id was in the node's own list
#define P_SELF 0x40000000u    // table id-word flag: the node's own entry
#define P_MISC_BYTES (64 * 4 + P_VMAX * 4 + P_VMAX * 4 + P_VMAX * 8)

// Lemire's rejection threshold 2^32 mod size for every list size 1..P_VMAX (a final list holds at
// most V <= P_VMAX entries), read by a scalar load instead of a 32-bit remainder per node
struct PThrTab {
  uint32_t v[P_VMAX + 1];
  constexpr PThrTab() : v() {
    for (uint32_t n = 1; n <= P_VMAX; n++) v[n] = (0u - n) % n;
  }
};
inline __constant__ PThrTab p_thr_tab = PThrTab();  // inline: one table, whichever units include this

template <int H>
struct PLds {
  static constexpr int bytes = H * 8 + P_MISC_BYTES;
};

// compile-time sizes of a node tick on an H-slot table (BIG: the big and huge kernels)
template <int H, bool BIG>
struct PDim {
  static constexpr int TS = H / 64;                                      // table slots per lane
  static constexpr int KK = H == P_HH ? P_KMAX : BIG ? P_KP : P_KSMALL;  // lists merged at most
  static constexpr int DS = ((1 + KK) * P_VMAX + 63) / 64;               // dense entries per lane
  static constexpr int NSTEP = (KK + 1) / 2;                             // list-load steps (>= 2 lists per step)
  using mask_t = typename std::conditional<(DS > 32), uint64_t, uint32_t>::type;  // one bit per dense slot
};

// the regions of a wave's LDS slice (PLds<H>::bytes from `base`): the table's id and heartbeat words,
// then the misc area
struct PTab {
  uint32_t *tid, *thb, *hist, *kid, *khb;
  uint64_t *fin;
};
template <int H>
__device__ __forceinline__ PTab p_tab(unsigned char *base) {
  PTab b;
  b.tid = (uint32_t *)base;
  b.thb = b.tid + H;
  b.hist = b.thb + H;
  b.kid = b.hist + 64;
  b.khb = b.kid + P_VMAX;
  b.fin = (uint64_t *)(b.khb + P_VMAX);
  return b;
}

// a node's wave-uniform values (and the lane): the tick, the global node index (ids, keys, seeds,
// targets), the local row, the view width, the tick's parity
struct PNode {
  int t, i, li, V, par, lane;
};

// LDS hand-off between the lanes of ONE wave (every LDS region here is private to its wave):
// a wave's LDS instructions execute in issue order, so wavefront scope needs no lgkmcnt wait --
// only the compiler must not move LDS accesses across it (workgroup scope waited lgkmcnt(0)
// at each of the ~16 hand-offs of a node)
__device__ __forceinline__ void p_wsync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ int p_age(int t, uint32_t hb) { return t - (int)((hb + 1u) >> 1); }
// p_age(t, hb) >= A as one compare: t - floor((hb+1)/2) >= A <=> hb < 2(t-A)+1 (heartbeats < 2^31)
__device__ __forceinline__ bool p_aged(int t, uint32_t hb, int A) { return (int)hb < 2 * (t - A) + 1; }

// eviction tie-break key (oracle op_evict_key): fmix32 of the id under a per-(tick, observer)
// seed -- a bijection, so distinct ids give distinct keys; oseed = (uint32)mix64(mix64(view_seed
// ^ t) ^ obs) is wave-uniform
__device__ __forceinline__ uint32_t p_evict_key(uint32_t oseed, uint32_t id) { return gm_fmix32(id ^ oseed); }

// exclusive wave prefix of small per-lane counts c < 2^BITS (ballot per bit + mbcnt)
template <int BITS>
__device__ __forceinline__ int p_excl(int c, int *total) {
  int pos = 0, tot = 0;
#pragma unroll
  for (int b = 0; b < BITS; b++) {
    const uint64_t bal = __ballot((c >> b) & 1);
    pos += lanes_below(bal) << b;
    tot += __builtin_popcountll(bal) << b;
  }
  *total = tot;
  return pos;
}

__device__ __forceinline__ uint64_t p_readlane64(uint64_t v, int l) {
  const uint32_t lo = __builtin_amdgcn_readlane((uint32_t)v, l);
  const uint32_t hi = __builtin_amdgcn_readlane((uint32_t)(v >> 32), l);
  return ((uint64_t)hi << 32) | lo;
}

// claim or find the slot of `id`, raise its heartbeat word. Every lane of the wave runs the probe
// loop (no divergent loop: its exec-mask bookkeeping was ~5 SALU per probe). A lane with nothing to
// insert (take false) points at its own word of the misc area (hist[lane], 2H words past tid),
// which holds P_TRASH while the lists merge: its CAS changes nothing and finds "its" id at once, and
// its max of 0 changes nothing (distinct words: no same-address serialisation). A lane that found
// its slot repeats an idempotent CAS. The merge claims bare ids (flags are ORed in after it), so one
// compare finds an id. Returns the slot (>= 2H for a lane that took nothing).
#define P_TRASH 0xFFFFFFFFu
template <int H>
__device__ __forceinline__ int p_insert(uint32_t *tid, bool take, uint32_t id, uint32_t hb, int lane) {
  // slot = low bits of id ^ id >> 9: view ids are uniform node indices, so this spreads them like a
  // multiplicative hash without its quarter-rate 32-bit multiply (the slot never shows in a result:
  // the table is compacted and ranked by id). Probing steps a byte offset: with the table at LDS
  // address 0 the slot's address is the offset
  const uint32_t idw = take ? id : P_TRASH;
  uint32_t a = take ? ((id ^ (id >> 9)) & (H - 1)) * 4 : 8 * H + 4 * lane;
  for (;;) {  // claim-or-compare in one LDS op
    const uint32_t cur = atomicCAS((uint32_t *)((unsigned char *)tid + a), 0u, idw);
    const bool more = cur != 0 && cur != idw;
    if (!__ballot(more)) break;
    if (more) a = (a + 4) & (4 * H - 1);
  }
  atomicMax((uint32_t *)((unsigned char *)tid + a + (take ? 4 * H : 0)), take ? hb : 0u);
  return (int)(a >> 2);
}

// owning row shard of node d: contiguous balanced ranges [n*g/G, n*(g+1)/G), boundaries
// in shard_n0[0..G]; a float estimate is off by at most one, two compares fix it
__device__ __forceinline__ int p_owner(const PState &s, int d) {
  int g = min(s.G - 1, max(0, (int)((float)d * (float)s.G / (float)s.n)));
  if (g + 1 < s.G && s.shard_n0[g + 1] <= d) g++;
  if (g > 0 && s.shard_n0[g] > d) g--;
  return g;
}

// A node's independent loads, issued together before any branch on them (one memory
// round trip instead of a chain): crash flag, inbox count, own list, inbox row, S2
// outputs, heartbeat counter. `nin` = inbox lanes to fetch (the kernel's list bound).
struct PPre {
  int failed, k, hbctr;
  uint64_t own;
  int sv;
  uint32_t raw0;  // S2 output d on lane roff + d
  int roff;
};
__device__ __forceinline__ PPre p_preload(const PState &s, int t, const uint32_t *mtraw, int li, int lane, int nin) {
  const int par = t & 1, V = s.V;
  PPre p;
  p.failed = s.failed[li];
  p.k = s.inbox[par][(size_t)li * P_KMAX];
  p.hbctr = s.hbctr[li];
  p.own = lane < V ? s.lists[((size_t)(par ^ 1) * s.rows + li) * V + lane] : 0ull;
  p.sv = lane < nin ? s.inbox[par][(size_t)li * P_KMAX + 1 + lane] : 0;
  p.raw0 = lane < 16 ? mtraw[(size_t)li * 16 + lane] : 0u;
  p.roff = 0;
  return p;
}

// ---- 1. the list loads (the node's independent loads arrived with `pre`)
// lists per load step (per), entry (l) and list slot (jo) of this lane; V = 32 (S-C) takes the
// shifts instead of three integer divisions. The step's per-list values come by ds_bpermute
// (the LDS port) rather than two readlanes + a select: VALU issue is what bounds this kernel
struct PStep {
  int per, l, jo;
};
__device__ __forceinline__ PStep p_step(const PNode &nd) {
  const bool v32 = nd.V == P_VMAX;
  PStep sp;
  if (v32) {
    sp.per = 2;
    sp.l = nd.lane & 31;
    sp.jo = nd.lane >> 5;
  } else {
    sp.per = 64 / nd.V;
    sp.l = nd.lane % nd.V;
    sp.jo = nd.lane / nd.V;
  }
  return sp;
}
// v of lane st * per + jo
__device__ __forceinline__ int p_step_val(const PStep &sp, int v, int st) {
  return __shfl(v, min(st * sp.per + sp.jo, 63), 64);
}

// clear the table (both word arrays are contiguous)
template <int H>
__device__ __forceinline__ void p_clear(const PTab &b, int lane) {
  uint4 *z = (uint4 *)b.tid;
#pragma unroll
  for (int q = 0; q < H / 128; q++) z[lane + 64 * q] = make_uint4(0, 0, 0, 0);
  b.tid[2 * H + lane] = P_TRASH;  // hist[lane]: the lane's trash word while the lists merge (p_insert)
}

// the kk delivered lists (sender rows sv, lane j for list j) into dv: V lanes per list, `per` lists per step
template <int H, bool BIG, bool RM>
__device__ __forceinline__ void p_load_lists(const PState &s, const PNode &nd, const PStep &sp, int sv, int kk,
                                             uint64_t (&dv)[PDim<H, BIG>::NSTEP]) {
  const int t = nd.t, V = nd.V, par = nd.par;
  const uint64_t *prev = s.lists + (size_t)(par ^ 1) * s.rows * V;
#pragma unroll
  for (int st = 0; st < PDim<H, BIG>::NSTEP; st++) {
    dv[st] = 0;
    if (st * sp.per >= kk) continue;  // wave-uniform: no list in this step (k ~ 5 of up to 12 at S-C; -1.1 %,
                                      // profiles/r05/ab7/)
    const int j = st * sp.per + sp.jo;
    const bool ok = sp.jo < sp.per && j < kk;
    const int sn = p_step_val(sp, sv, st);
    uint64_t e = 0;
    if (ok && (!RM || sn < s.nloc)) {
      e = prev[(size_t)sn * V + sp.l];
    } else if (RM && ok) {  // a list another shard sent at t-1: wire entry id | (2(t-1)-1 - hb) << 25
      const uint32_t w = s.recv_list[par ^ 1][(size_t)(sn - s.nloc) * V + sp.l];
      if (w) e = ((uint64_t)(w & ((1u << P_WIRE_IDBITS) - 1)) << 32) | (uint32_t)(2 * t - 3 - (int)(w >> P_WIRE_IDBITS));
    }
    dv[st] = e;
  }
}

// drop keys: one (t_send, src, dst) hash per delivered list, lane j for list j
struct PDrop {
  bool dropping;
  uint32_t pairv;  // low word of mix64(seed ^ t_send << 48 ^ src << 24 ^ dst)
  uint32_t dthr;
};
template <bool RM>
__device__ __forceinline__ PDrop p_drop_keys(const PState &s, const PNode &nd, int sv, int k) {
  const int par = nd.par;
  // global sender index of each list (the drop keys), after the list loads are in flight
  const int sg = nd.lane < k ? (!RM || sv < s.nloc ? s.n0 + sv : s.rsrc[par ^ 1][sv - s.nloc]) : 0x7FFFFFFF;
  PDrop dr;
  dr.dropping = s.drop_pct >= 0;
  dr.pairv = 0;
  if (dr.dropping)
    dr.pairv = (uint32_t)gm_mix64(s.drop_seed ^ ((uint64_t)(uint32_t)(nd.t - 1) << 48) ^ ((uint64_t)(uint32_t)sg << 24) ^
                                  (uint64_t)(uint32_t)nd.i);
  dr.dthr = gm_drop_thresh(s.drop_pct);
  return dr;
}

// ---- 2. merge: own entries first (their slots get P_OWN after the merge), then the delivered lists.
// Returns the slot of the lane's own entry; nrecv counts the delivered entries kept (msgcount)
template <int H, bool BIG>
__device__ __forceinline__ int p_merge(const PNode &nd, const PTab &b, const PStep &sp, uint64_t own, int kk,
                                       const uint64_t (&dv)[PDim<H, BIG>::NSTEP], const PDrop &dr, bool mc, int &nrecv) {
  const int t = nd.t, lane = nd.lane;
  uint32_t *tid = b.tid;
  const int hslot = p_insert<H>(tid, own != 0, (uint32_t)(own >> 32), (uint32_t)own, lane);
  p_wsync();
  {
    const uint32_t tfresh = (uint32_t)max(0, 2 * t - 11);  // hb >= 2t-11 <=> (t-1) - (hb+1)/2 < TFAIL
#pragma unroll
    for (int st = 0; st < PDim<H, BIG>::NSTEP; st++) {
      if (st * sp.per >= kk) continue;  // wave-uniform
      const uint64_t e = dv[st];
      bool take = e != 0 && (uint32_t)e >= tfresh;
      const uint32_t id = (uint32_t)(e >> 32);
      if (dr.dropping) {  // per-entry drops keyed by (t_send, src, dst, id-1): lost iff the top 16 bits of
        // fmix32(pair ^ (id-1)) are below the threshold
        const uint32_t pair = (uint32_t)p_step_val(sp, (int)dr.pairv, st);
        take = take && (gm_fmix32(pair ^ (id - 1)) >> 16) >= dr.dthr;
      }
      (void)p_insert<H>(tid, take, id, (uint32_t)e, lane);
      if (mc) nrecv += __builtin_popcountll(__ballot(take));
    }
  }
  atomicOr(&tid[hslot], own != 0 ? P_OWN : 0u);  // after the merge: its probes compare bare ids (a lane
                                                 // with no own entry ORs 0 into its trash word)
  return hslot;
}

// ---- 3. self bump (heartbeat++; myPos->setheartbeat(heartbeat++))
template <int H>
__device__ __forceinline__ void p_self_bump(const PState &s, const PNode &nd, const PTab &b, uint64_t own, int hslot,
                                            int hbnew) {
  const int lane = nd.lane;
  const uint32_t self_id = (uint32_t)(nd.i + 1);
  const uint64_t sb = __ballot(own != 0 && (uint32_t)(own >> 32) == self_id);
  int hs;
  if (sb) {
    hs = __builtin_amdgcn_readlane(hslot, __builtin_ctzll(sb));
  } else {  // cannot happen for a live node (the oracle aborts): flag, and re-insert self
    hs = 0;
    if (lane == 0) {
      atomicOr(s.err, GM_ERR_SELF);
      hs = p_insert<H>(b.tid, true, self_id, 1u, lane);  // self is in no own slot: its id is bare
    }
    hs = __builtin_amdgcn_readfirstlane(hs);
  }
  if (lane == 0) {
    b.thb[hs] = (uint32_t)hbnew;
    b.tid[hs] |= P_SELF | P_OWN;
    s.hbctr[nd.li] = hbnew + 1;
  }
}

// ---- 5. compact the kept entries (<= V), rank them by id: the id-sorted final list, stored as the
// node's row of this tick. Returns its size; x = the lane's entry of it, f = the entry's rotated id word
// (id << 2 | own << 1 | self)
template <int H, bool BIG>
__device__ __forceinline__ int p_compact_rank(const PState &s, const PNode &nd, const PTab &b, int dm,
                                              const uint32_t (&dw)[PDim<H, BIG>::DS],
                                              const uint32_t (&dh)[PDim<H, BIG>::DS],
                                              typename PDim<H, BIG>::mask_t keep, uint64_t &x, uint32_t &f) {
  const int V = nd.V, lane = nd.lane;
  uint32_t *hist = b.hist, *kid = b.kid, *khb = b.khb;
  uint64_t *fin = b.fin;
  uint64_t *cur = s.lists + (size_t)nd.par * s.rows * V;
  int cnt = 0;
  p_wsync();  // the eviction histogram is dead: it takes the stores of the entries not kept
#pragma unroll
  for (int q = 0; q < PDim<H, BIG>::DS; q++) {
    if (q >= dm) break;
    const bool kq = (keep >> q) & 1;
    const uint64_t bal = __ballot(kq);
    const int p = cnt + lanes_below(bal);
    // id word rotated left by 2: id << 2 | own << 1 | self (ids < 2^25, bits 25..29 clear),
    // so the rank below compares whole words
    *(kq ? kid + p : hist + lane) = __builtin_amdgcn_alignbit(dw[q], dw[q], 30);
    *(kq ? khb + p : hist + lane) = dh[q];
    cnt += __builtin_popcountll(bal);
  }
  if (lane >= cnt && lane < P_VMAX) kid[lane] = ~0u;  // sentinels rank after every real entry
  p_wsync();
  {
    // entry e = lane % 32 on both half-waves; each half compares it against half of the
    // kept ids (cnt <= P_VMAX = 32), the two partial ranks add across the halves
    static_assert(P_VMAX == 32, "the id rank splits a wave into two half-waves of P_VMAX lanes");
    const int e = lane & (P_VMAX - 1);
    const uint32_t mw = e < cnt ? kid[e] : 0u, mh = e < cnt ? khb[e] : 0u;
    const uint32_t myid = mw >> 2;
    int rank = 0;
    const uint4 *kv = (const uint4 *)kid + (lane >> 5) * (P_VMAX / 8);
#pragma unroll
    for (int q = 0; q < P_VMAX / 8; q++) {  // broadcast reads, 4 ids each (ids are distinct)
      const uint4 v = kv[q];
      rank += (v.x < mw) + (v.y < mw) + (v.z < mw) + (v.w < mw);
    }
    rank += __shfl_xor(rank, 32, 64);
    p_wsync();
    if (lane < cnt) {
      fin[rank] = ((uint64_t)myid << 32) | mh;
      kid[rank] = mw;
    }
  }
  p_wsync();
  x = lane < cnt ? fin[lane] : 0ull;
  f = lane < cnt ? kid[lane] : 0u;
  if (lane < V) cur[(size_t)nd.li * V + lane] = x;
  return cnt;
}

// the gossip draw's rare tail: outputs past the 16 precomputed ones, from the lazy generator in the
// (free) table region, resolved on scalars. ng of the `target` targets are chosen (gl[0..ng), ng <= 4
// here); returns the new count
__device__ __forceinline__ int p_draw_lazy(const PState &s, const PNode &nd, const PTab &b, uint64_t x, uint32_t size,
                                           uint32_t thr, int target, int ng) {
  const int t = nd.t, i = nd.i, lane = nd.lane;
  uint32_t *gl = b.hist;
  p_wsync();
  int g0 = -1, g1 = -1, g2 = -1, g3 = -1, g4 = -1;
  if (ng > 0) g0 = (int)__builtin_amdgcn_readfirstlane(gl[0]);
  if (ng > 1) g1 = (int)__builtin_amdgcn_readfirstlane(gl[1]);
  if (ng > 2) g2 = (int)__builtin_amdgcn_readfirstlane(gl[2]);
  if (ng > 3) g3 = (int)__builtin_amdgcn_readfirstlane(gl[3]);
  GmLazyMT mt;
  bool done = false;
  for (int batch = 1; !done; batch++) {
    if (batch > (1 << 16)) {
      if (lane == 0) atomicOr(s.err, GM_ERR_DRAWS);
      break;
    }
    if (lane == 0 && batch == 1) {
      mt.seed(b.tid, gm_rd_seed(s.rd_seed, t, i + 1));
      for (int q = 0; q < 16; q++) (void)mt.next();
    }
    uint32_t raw = 0;
    for (int q = 0; q < 16; q++) {
      uint32_t o = 0;
      if (lane == 0) o = mt.next();
      o = __builtin_amdgcn_readfirstlane(o);
      if (lane == q) raw = o;
    }
    const uint64_t prod = (uint64_t)raw * size;
    const int ix = (int)(prod >> 32);
    uint64_t mk = __ballot(lane < 16 && (uint32_t)prod >= thr);
    while (mk && !done) {
      const int d = __builtin_ctzll(mk);
      mk &= mk - 1;
      const int ixd = __builtin_amdgcn_readlane(ix, d);
      const uint64_t e = p_readlane64(x, ixd);
      const int c = (int)(e >> 32) - 1;
      if (c == i) continue;                                    // "me"
      if (p_aged(t, (uint32_t)e, GM_TFAIL)) continue;           // age >= TFAIL
      if ((ng > 0 && g0 == c) || (ng > 1 && g1 == c) || (ng > 2 && g2 == c) || (ng > 3 && g3 == c)) continue;
      if (ng == 0) g0 = c;
      else if (ng == 1) g1 = c;
      else if (ng == 2) g2 = c;
      else if (ng == 3) g3 = c;
      else g4 = c;
      ng++;
      if (ng >= target) done = true;
    }
  }
  p_wsync();
  if (lane < ng) gl[lane] = (uint32_t)(lane == 0 ? g0 : lane == 1 ? g1 : lane == 2 ? g2 : lane == 3 ? g3 : g4);
  return ng;
}

// ---- 6. gossip draw over the final list (MP1Node.cpp:449-489): x = the lane's entry of the cnt.
// Returns the number of targets; the targets in draw order are left in hist[0..ng) (hist is free
// after the compaction)
__device__ __forceinline__ int p_draw(const PState &s, const PNode &nd, const PTab &b, uint32_t raw0, int roff,
                                      uint64_t x, int cnt, int numfailed) {
  const int t = nd.t, i = nd.i, lane = nd.lane;
  const int numpot = cnt - 1 - numfailed;
  const int target = min(GM_FANOUT, numpot);
  int ng = 0;
  uint32_t *gl = b.hist;  // the chosen targets in draw order
  if (numpot > 0) {
    const uint32_t size = (uint32_t)cnt;
    const uint32_t thr = p_thr_tab.v[size];  // size = cnt <= V <= P_VMAX
    {  // the 16 precomputed outputs in parallel, output d on lane d: it is taken iff Lemire
       // accepts it, the drawn entry is not "me" and not aged, and no earlier such output drew
       // the same id (that one was taken, or repeated a taken one) -- the reference's loop
      // every 16-lane group g evaluates all 16 outputs (output d = lane % 16) and tests
      // d against the earlier outputs q in [4g, 4g + 4); the groups' results are OR-ed
      const int d = lane & 15, g4 = (lane >> 4) * 4;
      const uint32_t rawd = __shfl(raw0, roff + d, 64);
      const uint64_t prod = (uint64_t)rawd * size;
      const int ixv = (int)(prod >> 32);
      const uint32_t elo = __shfl((uint32_t)x, ixv, 64), ehi = __shfl((uint32_t)(x >> 32), ixv, 64);
      const int c = (int)ehi - 1;
      const bool okd = (uint32_t)prod >= thr && c != i && !p_aged(t, elo, GM_TFAIL);
      const int cv = okd ? c : -2;
      int dup = 0;
#pragma unroll
      for (int j = 0; j < 4; j++) dup |= (g4 + j < d) & (__shfl(cv, g4 + j, 64) == cv);
      uint64_t db = __ballot(dup);  // OR of the four groups' verdicts, bit d
      db |= db >> 32;
      db |= db >> 16;
      dup = (int)((uint32_t)db >> d) & 1;
      const bool ok = lane < 16 && okd;
      const bool acc = ok && !dup;
      const uint64_t ab = __ballot(acc);
      const int rk = lanes_below(ab);
      ng = min(__builtin_popcountll(ab), target);
      gl[acc && rk < target ? rk : 16 + lane] = (uint32_t)c;  // others: trash words past the targets
    }
    if (ng < target) ng = p_draw_lazy(s, nd, b, x, size, thr, target, ng);  // rare
  }
  return ng;
}

// the per-node values the tick records next to the targets (rowstat, ev_cnt, ev_jm, msgcount)
struct PStat {
  int cnt, numfailed, removed, nrem, nj, nrecv;
  uint64_t jb;
};

// One node's tick on one wave. li: the node's local row (global index n0 + li);
// pre.k: lists queued for it this tick.
// MC: the msgcount-recording instantiation (gm_msgcount_record); the others carry no trace of it
// RM: lists of other row shards may be delivered (sharded contexts); without, every sender is a
// local row and the list loads carry no branch
// VF: the view width when known at compile time (32: S-C), 0 = s.V at run time
template <int H, bool BIG, bool MC, bool RM = true, int VF = 0>
__device__ __forceinline__ void p_node(const PState &s, int t, const PPre &pre, int li, int lane, unsigned char *base) {
  using D = PDim<H, BIG>;
  using mask_t = typename D::mask_t;
  constexpr int TS = D::TS, DS = D::DS;
  const int V = VF ? VF : s.V;
  const PNode nd = {t, s.n0 + li, li, V, t & 1, lane};
  const PTab tab = p_tab<H>(base);
  int k = pre.k;
  if (lane == 0) s.inbox[nd.par][(size_t)li * P_KMAX] = 0;  // consumed; the append target of tick t+1
  const int kmax = min((int)D::KK, s.kcap);  // lists stored in the inbox row (the append counter may count more)
  if (k > kmax) {  // the huge kernel takes up to the inbox capacity; beyond it the tick is void
    if (lane == 0) atomicOr(s.err, GM_ERR_INBOX);
    k = kmax;  // never read sender slots that were not written
  }
  // ---- 1. loads
  const int sv = lane < k ? pre.sv : 0x7FFFFFFF;  // list rows
  p_clear<H>(tab, lane);
  const int kk = min(k, (int)D::KK);
  const PStep sp = p_step(nd);
  uint64_t dv[D::NSTEP];
  p_load_lists<H, BIG, RM>(s, nd, sp, sv, kk, dv);
  const PDrop dr = p_drop_keys<RM>(s, nd, sv, k);
  const bool mc = MC && t < s.mc_tmax;  // msgcount recording (wave-uniform)
  PStat st;
  st.nrecv = 0;
  p_wsync();
  // ---- 2. merge
  const int hslot = p_merge<H, BIG>(nd, tab, sp, pre.own, kk, dv, dr, mc, st.nrecv);
  p_wsync();
  // ---- 3. self bump, then sweep + compaction
  p_self_bump<H>(s, nd, tab, pre.own, hslot, pre.hbctr + 1);
  p_wsync();
  // The sweep, the dense loads and the eviction's class search stay inline: each of them as a function
  // of its own (arguments by reference, by value or as bare scalars; the class search with and without
  // the dense loads) changes gm_p_tick_big's register count (146 / 148 -> 156 / 158 VGPRs), and sweep
  // and eviction both as functions spill the small kernel (profiles/partial_split/README.md)
  uint32_t *tid = tab.tid, *thb = tab.thb;
  uint32_t *evr = s.ev + (size_t)li * 2 * V;
  int m;
  {
    uint32_t w[TS], hh[TS];
#pragma unroll
    for (int q = 0; q < TS / 4; q++) {
      const uint4 a = ((const uint4 *)tid)[lane * (TS / 4) + q];
      const uint4 b = ((const uint4 *)thb)[lane * (TS / 4) + q];
      w[4 * q] = a.x; w[4 * q + 1] = a.y; w[4 * q + 2] = a.z; w[4 * q + 3] = a.w;
      hh[4 * q] = b.x; hh[4 * q + 1] = b.y; hh[4 * q + 2] = b.z; hh[4 * q + 3] = b.w;
    }
    using tmask_t = typename std::conditional<(TS > 32), uint64_t, uint32_t>::type;  // one bit per table slot
    constexpr int CB = TS <= 8 ? 4 : TS <= 16 ? 5 : TS <= 32 ? 6 : 7;               // bits of a per-lane slot count
    // alive <=> present and not aged past TREMOVE <=> hb >= xa: every present entry has hb >= 1
    // (heartbeats start at 2t-1 >= 1; hb < 2^31) and an empty slot holds hb 0, so one compare per
    // slot gives the alive bit; removals = present - alive (rare: tested once per row)
    const uint32_t xa = (uint32_t)max(2 * (t - GM_TREMOVE) + 1, 1);
    // the alive count by compares whose results feed carry-ins (v_cmp + v_addc per slot), not by a
    // per-lane bit mask built and popcounted (~4 VALU per slot); the mask is built only in the rare
    // removal branch
    int rcount = 0, na = 0;
#pragma unroll
    for (int u = 0; u < TS; u++) {
      na += hh[u] >= xa;
      rcount += (int)min(w[u], 1u);
    }
    rcount -= na;
    st.removed = st.nrem = 0;
    if (__ballot(rcount != 0)) {  // rare: TREMOVE removals in this row
      tmask_t alive = 0, rown = 0;
#pragma unroll
      for (int u = 0; u < TS; u++) alive |= (tmask_t)(hh[u] >= xa) << u;
#pragma unroll
      for (int u = 0; u < TS; u++) rown |= (tmask_t)((w[u] >> 31) & (uint32_t)!((alive >> u) & 1)) << u;
      (void)p_excl<CB>(rcount, &st.removed);
      const int ro = __builtin_popcountll(rown);
      int rpos = p_excl<CB>(ro, &st.nrem);
      if (st.nrem) {  // REMOVE events of the node's own entries, from the back of its event row
#pragma unroll
        for (int u = 0; u < TS; u++)
          if ((rown >> u) & 1) evr[2 * V - 1 - rpos++] = (P_EV_REMOVE << 30) | (w[u] & P_IDMASK);
      }
    }
    // the alive slots' dense positions: an inclusive DPP scan of the per-lane counts (A/B on one box
    // against p_excl's ballot per count bit: -0.3 %, profiles/r04/sc_sweep/)
    const int incl = dpp_scan(na);
    m = __builtin_amdgcn_readlane(incl, 63);
    int pos = incl - na;
    // every slot is stored: dead ones to a per-lane slot of [H-64, H), past the dense
    // range (m <= (1+KK)V+1 < H-64) and free of bank conflicts
#pragma unroll
    for (int u = 0; u < TS; u++) {
      const bool a = hh[u] >= xa;
      const int at = a ? pos : H - 64 + lane;
      tid[at] = w[u];
      thb[at] = hh[u];
      pos += a;
    }
  }
  p_wsync();
  // ---- 4. dense entries e = s*64 + lane; eviction to V
  // only the first dm = ceil(m / 64) of the DS per-lane slots hold entries (m is wave-uniform):
  // every per-slot loop below skips the rest with a scalar branch
  const int dm = (m + 63) >> 6;
  uint32_t dw[DS], dh[DS];
#pragma unroll
  for (int q = 0; q < DS; q++) {  // DS*64 < H: the reads stay inside the table
    dw[q] = dh[q] = 0u;
    if (q < dm) {
      const int e = q * 64 + lane;
      const uint32_t a = tid[e], b = thb[e];
      dw[q] = e < m ? a : 0u;
      dh[q] = e < m ? b : 0u;
    }
  }
  mask_t keep = 0;
  if (m <= V) {
#pragma unroll
    for (int q = 0; q < DS; q++)
      if (q < dm && dw[q]) keep |= (mask_t)1 << q;
  } else {
    // heartbeat distance from the top (2t-1 = this tick's self heartbeat); alive entries have
    // age < TREMOVE, i.e. distance <= 40; every heartbeat is odd (2k - 1, MP1Node.cpp:412-415), so the
    // distances are even. The cut class (the smallest distance whose cumulative count of candidates
    // -- self excluded -- reaches V - 1) is found by ballots, class by class: the candidates crowd into
    // ~4 classes, so a 64-bin LDS histogram took its atomics ~58 lanes to one address at a time
    // (serialised in the LDS pipe: ~4 ms of the S-C tick, profiles/r06/sc_sections/)
    const int top = 2 * t - 1;
    const int need = V - 1;  // self is always kept
    int dd[DS];              // the slot's distance class, 64 = no candidate (empty, or self)
    bool odd = false;
#pragma unroll
    for (int q = 0; q < DS; q++) {
      dd[q] = 64;
      if (q < dm && dw[q] && !(dw[q] & P_SELF)) dd[q] = min(max(top - (int)dh[q], 0), 63);
      odd |= dd[q] & 1;
    }
    if (__ballot(odd) && lane == 0) atomicOr(s.err, GM_ERR_PARITY);  // cannot happen: heartbeats are odd
    int dcut = 62, before = 0, bsz = 0;
    for (int d = 0; d <= 62; d += 2) {  // wave-uniform; ends within the populated classes (m - 1 > need)
      int c = 0;
#pragma unroll
      for (int q = 0; q < DS; q++)
        if (q < dm) c += __builtin_popcountll(__ballot(dd[q] == d));
      if (before + c >= need) {
        dcut = d;
        bsz = c;
        break;
      }
      before += c;
    }
    const int needb = need - before;  // 1 <= needb <= bsz
    mask_t bucket = 0;
#pragma unroll
    for (int q = 0; q < DS; q++) {
      if (q >= dm) continue;
      keep |= (mask_t)(((dw[q] & P_SELF) != 0) | (dd[q] < dcut)) << q;
      bucket |= (mask_t)(dd[q] == dcut) << q;
    }
    if (needb == bsz) {
      keep |= bucket;
    } else {
      // the needb smallest eviction keys of the bucket: 6-bit radix on the top bits,
      // then exact min-selection inside the cut bin
      uint32_t *hist = tab.hist;
      const uint32_t oseed = (uint32_t)gm_mix64(gm_mix64(s.view_seed ^ (uint64_t)(uint32_t)t) ^ (uint64_t)(uint32_t)nd.i);
      uint32_t key[DS];
#pragma unroll
      for (int q = 0; q < DS; q++) {
        key[q] = ~0u;
        if (q < dm && __ballot((bucket >> q) & 1)) key[q] = ((bucket >> q) & 1) ? p_evict_key(oseed, dw[q] & P_IDMASK) : ~0u;
      }
      p_wsync();
      hist[lane] = 0;
      p_wsync();
#pragma unroll
      for (int q = 0; q < DS; q++)
        if (q < dm) atomicAdd(((bucket >> q) & 1) ? &hist[key[q] >> 26] : &tid[H - 64 + lane], 1u);
      p_wsync();
      const int c = (int)hist[lane];
      const int inc = dpp_scan(c);
      const uint64_t over2 = __ballot(inc >= needb);
      const int bcut = __builtin_ctzll(over2);
      const int before2 = __builtin_amdgcn_readlane(inc - c, bcut);
      const int bsz2 = __builtin_amdgcn_readlane(c, bcut);
      int needc = needb - before2;  // 1 <= needc <= bsz2
      mask_t cand = 0;
#pragma unroll
      for (int q = 0; q < DS; q++) {
        if (q >= dm) continue;
        const mask_t b = (bucket >> q) & 1;
        const int bin = (int)(key[q] >> 26);
        keep |= (b & (mask_t)(bin < bcut)) << q;
        cand |= (b & (mask_t)(bin == bcut)) << q;
      }
      if (needc == bsz2) {
        keep |= cand;
      } else {
        for (; needc > 0; needc--) {  // take the smallest remaining candidate key (keys are distinct)
          uint32_t mn = ~0u;
#pragma unroll
          for (int q = 0; q < DS; q++)
            if (q < dm && ((cand >> q) & 1)) mn = min(mn, key[q]);
#pragma unroll
          for (int o = 32; o >= 1; o >>= 1) mn = min(mn, (uint32_t)__shfl_xor((int)mn, o, 64));
#pragma unroll
          for (int q = 0; q < DS; q++)
            if (q < dm && ((cand >> q) & 1) && key[q] == mn) {
              keep |= (mask_t)1 << q;
              cand &= ~((mask_t)1 << q);
            }
        }
      }
    }
  }
  // ---- 5. the final list
  uint64_t x;
  uint32_t f;
  st.cnt = p_compact_rank<H, BIG>(s, nd, tab, dm, dw, dh, keep, x, f);
  // joins (ascending id): a mask over the final list (ev_jm)
  st.jb = __ballot(lane < st.cnt && !(f & 2u));  // rotated P_OWN
  st.nj = __builtin_popcountll(st.jb);
  st.numfailed = st.removed + __builtin_popcountll(__ballot(lane < st.cnt && p_aged(t, (uint32_t)x, GM_TFAIL)));
  // ---- 6. gossip draw, sends and the node's records
  const int ng = p_draw(s, nd, tab, pre.raw0, pre.roff, x, st.cnt, st.numfailed);
  p_wsync();
  // ---- sends: one parallel round of inbox appends, one lane per local target. A target owned by
  // another row shard is only recorded (targets / rowstat): gm_p_pack builds the exchange records from
  // them and this tick's list after the chunk (no record written per (sender, shard) here).
  // (inline: as a function of its own it cost 0.2 ms of the S-C tick, the eviction's rare tail 0.6 ms,
  // profiles/partial_split/README.md)
  const int par = nd.par;
  const int dst = lane < ng ? (int)tab.hist[lane] : 0;
  const int owner = (s.G > 1 && lane < ng) ? p_owner(s, dst) : s.rank;
  if (lane < ng) {
    s.targets[(size_t)li * GM_FANOUT + lane] = dst;
    if (owner == s.rank) {
      int32_t *row = s.inbox[par ^ 1] + (size_t)(dst - s.n0) * P_KMAX;  // count and slots share a line
      const int slot = atomicAdd(row, 1);
      if (slot < s.kcap) row[1 + slot] = li;
      else atomicOr(s.err, GM_ERR_INBOX);
    }
  }
  if (lane < 4) s.rowstat[(size_t)li * 4 + lane] = lane == 0 ? kk : lane == 1 ? st.cnt : lane == 2 ? st.numfailed : ng;
  if (lane == 0) s.ev_cnt[li] = st.nj | (st.nrem << 16);
  if (lane == 1) s.ev_jm[li] = (uint32_t)st.jb;  // lanes < cnt <= 32
  if (mc && lane == 0) {  // entries sent = fresh entries of the final list x targets (MP1Node.cpp:372-375)
    s.mc_sent[(size_t)t * s.nloc + li] = (uint32_t)(ng * (st.cnt - (st.numfailed - st.removed)));
    s.mc_recv[(size_t)t * s.nloc + li] = (uint32_t)st.nrecv;
  }
}

// crashed node: frozen (its list carried to this tick's buffer unchanged), inbox dropped
__device__ __forceinline__ void p_frozen(const PState &s, int t, int li, int lane) {
  const int par = t & 1, V = s.V;
  if (lane < V) s.lists[((size_t)par * s.rows + li) * V + lane] = s.lists[((size_t)(par ^ 1) * s.rows + li) * V + lane];
  if (lane < 4) s.rowstat[(size_t)li * 4 + lane] = 0;
  if (lane == 0) {
    s.inbox[par][(size_t)li * P_KMAX] = 0;
    s.ev_cnt[li] = 0;
    s.ev_jm[li] = 0;
  }
}
