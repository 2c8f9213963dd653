// gm_host_view_reach.hip -- PARTIAL view-graph reachability across row shards: the walk of a GROUP
// (gm_host.h: gm_ctx **g, count G), written once. gm_view_reach passes {c} when the context has a
// communicator (its peers are RCCL ranks), gm_view_reach_loopback the G row-shard contexts of one cluster
// living on one device. Kernels: gm_view_reach_shard.hip. The single-context walk stays in
// gm_host_read.hip.
//
// A level is "every member enqueues this launch" separated by group collectives (vrx_*), the only code
// that differs by group kind: an RCCL rank uses ncclAllToAllv / ncclAllReduce on its stream, a loopback
// group device copies on its first member's stream and sums on the host.
//
//   GM_REACH_IN   vrx_gather_front: every member's front slice into every member's wide; pass; commit
//   GM_REACH_OUT  pass (proposals into the member's wide); vrx_scatter_next: slice q of every member's
//                 wide into member q's receive area; commit (own slice | received slices); the rest of
//                 wide cleared for the next level
//   vrx_sum_row   the level's row of counts summed over the group; every decision to go on is taken from
//                 summed rows only, so all ranks leave the loop at the same level
//
// The walk reads lists[(t - 1) & 1] and the crash flags and writes its own scratch: nothing of the tick's
// exchange (inboxes, received lists, a pending replay after a view load) is touched.
#include "gm_host.h"

using namespace gmh;

namespace {

struct VrsMem {  // one member's scratch, carved out of its block
  uint64_t *seen, *front, *next, *wide, *recv, *counts, *status;
  int32_t *src;
  size_t bytes;
};

// the block: seen, front, next [nloc]; wide [n]; the receive area, W - 1 slices of nloc words (n - nloc
// when the shards are even, up to W - 1 words more when this shard is one of the larger); the counts
// [GM_VIEW_HOPS][GM_REACH_SOURCES]; the status word; the sources
VrsMem vrs_carve(const gm_ctx *c) {
  const PState &p = c->p;
  const size_t nl = (size_t)p.nloc, n = (size_t)p.n, W = (size_t)p.G;
  const size_t recv = std::max(n - nl, (W - 1) * nl);
  VrsMem m;
  uint64_t *w = (uint64_t *)c->vrs.blob;
  m.seen = w, w += nl;
  m.front = w, w += nl;
  m.next = w, w += nl;
  m.wide = w, w += n;
  m.recv = w, w += recv;
  m.counts = w, w += (size_t)GM_VIEW_HOPS * GM_REACH_SOURCES;
  m.status = w, w += 1;
  m.src = (int32_t *)w;
  m.bytes = sizeof(uint64_t) * (size_t)(w - (uint64_t *)c->vrs.blob) + sizeof(int32_t) * GM_REACH_SOURCES;
  return m;
}

int64_t shard_lo(const PState &p, int q) { return (int64_t)p.n * q / p.G; }

// the hash of the whole crash set as partial_caps keeps it for a sharded context
uint64_t crash_hash_of(const gm_ctx *c) {
  if (c->ph.sharded) return c->ph.crash_hash;
  uint64_t h = 0x9E3779B97F4A7C15ull;
  if (c->nfailed)
    for (int i = 0; i < c->p.n; i++)
      if (c->failed_h[i]) h = (h ^ (uint64_t)(uint32_t)i) * 0x100000001B3ull + 0x632BE59BD9B4E019ull;
  return h;
}

// what every rank of a collective walk must have been given: the arguments, the tick and the crash set
uint64_t walk_hash(const gm_ctx *c, const int32_t *sources, int nsrc, int dir, int max_hops) {
  uint64_t h = crash_hash_of(c);
  auto mix = [&h](uint64_t v) { h = (h ^ v) * 0x100000001B3ull + 0x632BE59BD9B4E019ull; };
  mix((uint64_t)nsrc), mix((uint64_t)dir), mix((uint64_t)max_hops), mix((uint64_t)c->t);
  for (int k = 0; k < nsrc; k++) mix((uint64_t)(uint32_t)sources[k]);
  return h;
}

// RCCL rank: the ranks agree on the walk's hash and on every rank's local checks before the first
// level, px_agree's method: one MAX all-reduce of (h, ~h), the local status riding along as word 2.
// A rank whose checks failed returns its own code, every other rank GM_ESTATE.
int vrx_agree(gm_ctx *c, uint64_t h, int local, hipStream_t st) {
  const uint64_t hv[3] = {h, ~h, (uint64_t)(-(int64_t)local)};
  uint64_t mx[3] = {0, 0, 0};
  HIPCHECK(hipMemcpyAsync(c->vrs.agree, hv, sizeof hv, hipMemcpyHostToDevice, st));
  NCCLCHECK(ncclAllReduce(c->vrs.agree, c->vrs.agree, 3, ncclUint64, ncclMax, c->comm, st));
  HIPCHECK(hipMemcpyAsync(mx, c->vrs.agree, sizeof mx, hipMemcpyDeviceToHost, st));
  HIPCHECK(hipStreamSynchronize(st));
  if (local != GM_OK) return local;
  if (mx[2]) {
    snprintf(g_errbuf, sizeof g_errbuf, "gm_view_reach: another rank failed its checks (code -%llu)",
             (unsigned long long)mx[2]);
    return GM_ESTATE;
  }
  if (mx[0] != hv[0] || mx[1] != hv[1]) {
    snprintf(g_errbuf, sizeof g_errbuf, "gm_view_reach: the ranks disagree on the sources, the arguments, the tick or the crash set");
    return GM_ESTATE;
  }
  return GM_OK;
}

// IN: the members' front slices into every member's wide
int vrx_gather_front(gm_ctx **g, int G, const std::vector<VrsMem> &m, hipStream_t st) {
  for (int i = 0; i < G; i++) {
    gm_ctx *c = g[i];
    const PState &p = c->p;
    HIPCHECK(hipMemcpyAsync(m[i].wide + p.n0, m[i].front, sizeof(uint64_t) * p.nloc, hipMemcpyDeviceToDevice, st));
    if (G == 1) {  // one gather of uneven slices: the same front slice to every peer, theirs to their places
      const int W = p.G;
      std::vector<size_t> sc(W), sd(W, 0), rc(W), rd(W);
      for (int q = 0; q < W; q++) {
        sc[q] = q == p.rank ? 0 : (size_t)p.nloc;
        rc[q] = q == p.rank ? 0 : (size_t)(shard_lo(p, q + 1) - shard_lo(p, q));
        rd[q] = (size_t)shard_lo(p, q);
      }
      NCCLCHECK(ncclAllToAllv(m[i].front, sc.data(), sd.data(), m[i].wide, rc.data(), rd.data(), ncclUint64, c->comm, st));
    }
    for (int j = 0; j < G; j++)
      if (j != i)
        HIPCHECK(hipMemcpyAsync(m[i].wide + g[j]->p.n0, m[j].front, sizeof(uint64_t) * g[j]->p.nloc,
                                hipMemcpyDeviceToDevice, st));
  }
  return GM_OK;
}

// OUT: slice q of every member's wide into member q's receive area, one slot of nloc words per peer in
// rank order (RCCL has no bitwise-OR reduction: the commit ORs the slots)
int vrx_scatter_next(gm_ctx **g, int G, const std::vector<VrsMem> &m, hipStream_t st) {
  for (int i = 0; i < G; i++) {
    gm_ctx *c = g[i];
    const PState &p = c->p;
    if (G == 1) {
      const int W = p.G;
      std::vector<size_t> sc(W), sd(W), rc(W), rd(W);
      for (int q = 0; q < W; q++) {
        sc[q] = q == p.rank ? 0 : (size_t)(shard_lo(p, q + 1) - shard_lo(p, q));
        sd[q] = (size_t)shard_lo(p, q);
        rc[q] = q == p.rank ? 0 : (size_t)p.nloc;
        rd[q] = (size_t)(q < p.rank ? q : q - 1) * p.nloc;
      }
      rd[p.rank] = 0;
      NCCLCHECK(ncclAllToAllv(m[i].wide, sc.data(), sd.data(), m[i].recv, rc.data(), rd.data(), ncclUint64, c->comm, st));
    }
    for (int j = 0; j < G; j++)
      if (j != i)
        HIPCHECK(hipMemcpyAsync(m[i].recv + (size_t)(j < i ? j : j - 1) * p.nloc, m[j].wide + p.n0,
                                sizeof(uint64_t) * p.nloc, hipMemcpyDeviceToDevice, st));
  }
  return GM_OK;
}

// counts[h] summed over the group into row (host): an RCCL rank all-reduces its device row in place
int vrx_sum_row(gm_ctx **g, int G, const std::vector<VrsMem> &m, int h, uint64_t *row, hipStream_t st) {
  const size_t off = (size_t)h * GM_REACH_SOURCES;
  std::vector<uint64_t> part((size_t)G * GM_REACH_SOURCES);
  for (int i = 0; i < G; i++) {
    if (G == 1)
      NCCLCHECK(ncclAllReduce(m[i].counts + off, m[i].counts + off, GM_REACH_SOURCES, ncclUint64, ncclSum, g[i]->comm, st));
    HIPCHECK(hipMemcpyAsync(part.data() + (size_t)i * GM_REACH_SOURCES, m[i].counts + off,
                            sizeof(uint64_t) * GM_REACH_SOURCES, hipMemcpyDeviceToHost, st));
  }
  HIPCHECK(hipStreamSynchronize(st));
  for (int k = 0; k < GM_REACH_SOURCES; k++) {
    row[k] = 0;
    for (int i = 0; i < G; i++) row[k] += part[(size_t)i * GM_REACH_SOURCES + k];
  }
  return GM_OK;
}

// the members' status words combined (one flag: MAX is OR), so every rank returns the same code
int vrx_status(gm_ctx **g, int G, const std::vector<VrsMem> &m, hipStream_t st) {
  std::vector<uint64_t> part(G, 0);
  for (int i = 0; i < G; i++) {
    if (G == 1) NCCLCHECK(ncclAllReduce(m[i].status, m[i].status, 1, ncclUint64, ncclMax, g[i]->comm, st));
    HIPCHECK(hipMemcpyAsync(&part[i], m[i].status, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  }
  HIPCHECK(hipStreamSynchronize(st));
  uint64_t all = 0;
  for (int i = 0; i < G; i++) all |= part[i];
  if (!all) return GM_OK;
  snprintf(g_errbuf, sizeof g_errbuf, "gm_view_reach: a stored view names an id outside [1, n] (flags 0x%x)", (unsigned)all);
  return GM_ESTATE;
}

}  // namespace

int gmh::view_reach_args(int n, const int32_t *sources, int nsrc, int dir, int max_hops, const uint64_t *counts,
                         const int64_t *info) {
  if (!sources || (!counts && !info) || nsrc < 1 || nsrc > GM_REACH_SOURCES || max_hops < 1 || max_hops > GM_VIEW_HOPS ||
      (dir != GM_REACH_OUT && dir != GM_REACH_IN))
    return GM_EINVAL;
  for (int k = 0; k < nsrc; k++)
    if (sources[k] < 0 || sources[k] >= n) return GM_EINVAL;
  return GM_OK;
}

// The walk of a group: one RCCL rank (G == 1, g[0]->comm) or the G members of a loopback cluster, whose
// membership the caller has checked. The arguments have passed view_reach_args. seen: the group's nodes
// in node order -- a rank's own nloc words, a loopback group's n.
int gmh::view_reach_group(gm_ctx **g, int G, const int32_t *sources, int nsrc, int dir, int max_hops, uint64_t *counts,
                          uint64_t *seen, int64_t info[4]) {
  gm_ctx *L = g[0];
  hipStream_t st = L->stream;
  const bool rank = G == 1;
  // the members' own checks: a loopback group returns the first failure, an RCCL rank carries it into
  // the agreement so that no peer waits in a collective for a rank that has left
  int local = GM_OK;
  for (int i = 0; i < G && local == GM_OK; i++) {
    gm_ctx *c = g[i];
    if (c->latched != GM_OK) local = c->latched;
    else if (c->vl.loading) local = GM_ESTATE;  // between gm_load_views_begin and the commit
  }
  for (int i = 0; i < G && local == GM_OK; i++) {
    gm_ctx *c = g[i];
    if (c->xch.stream) HIPCHECK(hipStreamSynchronize(c->xch.stream));  // a row shard's exchange and unpacks
    local = check_err(c);  // waits for the member's stream: the walk runs on the first member's
  }
  for (int i = 1; i < G && local == GM_OK; i++)
    if (crash_hash_of(g[i]) != crash_hash_of(L)) {
      snprintf(g_errbuf, sizeof g_errbuf, "gm_view_reach_loopback: member %d holds another crash set", i);
      local = GM_ESTATE;
    }
  if (!rank) TRY(local);
  if (rank && !L->vrs.agree) TRY(dalloc(L, &L->vrs.agree, 4));
  for (int i = 0; i < G && local == GM_OK; i++)
    if (!g[i]->vrs.blob) local = dalloc(g[i], &g[i]->vrs.blob, vrs_carve(g[i]).bytes);
  if (rank) TRY(vrx_agree(L, walk_hash(L, sources, nsrc, dir, max_hops), local, st));
  TRY(local);

  std::vector<VrsMem> m(G);
  const int T = L->t - 1;
  for (int i = 0; i < G; i++) {
    m[i] = vrs_carve(g[i]);
    HIPCHECK(hipMemsetAsync(g[i]->vrs.blob, 0, m[i].bytes, st));
    HIPCHECK(hipMemcpyAsync(m[i].src, sources, sizeof(int32_t) * nsrc, hipMemcpyHostToDevice, st));
    HIPCHECK(gm_launch_view_reach_shard_seed(g[i]->p, m[i].src, nsrc, m[i].seen, m[i].front, m[i].counts, st));
  }
  const size_t row_words = GM_REACH_SOURCES;
  std::vector<uint64_t> cnt((size_t)GM_VIEW_HOPS * row_words, 0);
  TRY(vrx_sum_row(g, G, m, 0, cnt.data(), st));  // waits for the stream: `sources` is the caller's
  // every member holds the whole crash set (gm_set_failed, the load's commit), so nfailed counts the cluster's
  const uint64_t live = (uint64_t)(L->p.n - L->nfailed);
  uint64_t full = 0, reached[GM_REACH_SOURCES];
  int64_t live_sources = 0;
  for (int k = 0; k < GM_REACH_SOURCES; k++) {
    reached[k] = cnt[k];
    if (cnt[k]) full |= 1ull << k;
    live_sources += cnt[k] != 0;
  }
  for (int h = 1; h < max_hops && full; h++) {
    bool all = true;  // every live source has reached every live node: the next level is empty
    for (int k = 0; k < nsrc; k++) all = all && (!((full >> k) & 1) || reached[k] == live);
    if (all) break;
    if (dir == GM_REACH_IN) {
      TRY(vrx_gather_front(g, G, m, st));
      for (int i = 0; i < G; i++)
        HIPCHECK(gm_launch_view_reach_shard_pass(g[i]->p, T, dir, full, m[i].seen, m[i].front, m[i].next, m[i].wide,
                                                 (uint32_t *)m[i].status, st));
      for (int i = 0; i < G; i++)
        HIPCHECK(gm_launch_view_reach_shard_commit(g[i]->p, h, nsrc, m[i].seen, m[i].front, m[i].next, nullptr, 0,
                                                   m[i].counts, st));
    } else {
      for (int i = 0; i < G; i++)
        HIPCHECK(gm_launch_view_reach_shard_pass(g[i]->p, T, dir, full, m[i].seen, m[i].front, m[i].next, m[i].wide,
                                                 (uint32_t *)m[i].status, st));
      TRY(vrx_scatter_next(g, G, m, st));
      for (int i = 0; i < G; i++) {
        const PState &p = g[i]->p;
        HIPCHECK(gm_launch_view_reach_shard_commit(p, h, nsrc, m[i].seen, m[i].front, m[i].wide + p.n0, m[i].recv,
                                                   p.G - 1, m[i].counts, st));
      }
      for (int i = 0; i < G; i++) {  // the commit cleared the member's own slice: the rest of wide, once every peer has read it
        const PState &p = g[i]->p;
        const size_t hi = (size_t)p.n0 + p.nloc;
        if (p.n0) HIPCHECK(hipMemsetAsync(m[i].wide, 0, sizeof(uint64_t) * p.n0, st));
        if (hi < (size_t)p.n) HIPCHECK(hipMemsetAsync(m[i].wide + hi, 0, sizeof(uint64_t) * ((size_t)p.n - hi), st));
      }
    }
    uint64_t *row = cnt.data() + (size_t)h * row_words;
    TRY(vrx_sum_row(g, G, m, h, row, st));
    bool any = false;
    for (int k = 0; k < GM_REACH_SOURCES; k++) {
      reached[k] += row[k];
      any = any || row[k];
    }
    if (!any) break;
  }
  // nothing is handed out before the walk's checks pass, on every member
  TRY(vrx_status(g, G, m, st));
  int hops = 0;
  for (int h = 0; h < max_hops; h++)
    for (int k = 0; k < GM_REACH_SOURCES; k++)
      if (cnt[(size_t)h * row_words + k]) hops = h;
  bool last = false;
  for (int k = 0; k < GM_REACH_SOURCES; k++) last = last || cnt[(size_t)(max_hops - 1) * row_words + k];
  if (seen) {
    for (int i = 0; i < G; i++)
      HIPCHECK(hipMemcpyAsync(seen + (rank ? 0 : g[i]->p.n0), m[i].seen, sizeof(uint64_t) * g[i]->p.nloc,
                              hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
  }
  if (counts) memcpy(counts, cnt.data(), sizeof(uint64_t) * cnt.size());
  if (info) {
    info[0] = (int64_t)live;
    info[1] = hops;
    info[2] = last ? 1 : 0;
    info[3] = live_sources;
  }
  return GM_OK;
}

// The walk over the G row-shard contexts of one cluster living on one device (tests,
// scripts/view_reach_shard_cost.py): the walk gm_view_reach runs per RCCL rank, the exchange by device
// copies. The group's checks are gm_partial_loopback_tick's.
extern "C" int gm_view_reach_loopback(gm_ctx **ctxs, int32_t G, const int32_t *sources, int32_t nsrc, int32_t dir,
                                      int32_t max_hops, uint64_t *counts, uint64_t *seen, int64_t info[4]) {
  if (!ctxs || G < 2) return GM_EINVAL;
  for (int g = 0; g < G; g++) {
    gm_ctx *c = ctxs[g];
    if (!c || c->cfg.mode != GM_MODE_PARTIAL || c->p.G != G || c->p.rank != g || c->t != ctxs[0]->t ||
        c->n != ctxs[0]->n || c->p.V != ctxs[0]->p.V || c->p.nchunk != ctxs[0]->p.nchunk)
      return GM_EINVAL;
  }
  TRY(view_reach_args(ctxs[0]->n, sources, nsrc, dir, max_hops, counts, info));
  return view_reach_group(ctxs, G, sources, nsrc, dir, max_hops, counts, seen, info);
}
