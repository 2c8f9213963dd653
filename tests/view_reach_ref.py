"""View-graph reachability (gm_view_reach, include/gm_abi.h) in plain NumPy: the specification the GPU
tests compare against, exactly. A helper, not a test.

Views are what Simulator.read_views() returns: uint64 [n][V], id << 32 | hb, 0 = empty; failed is
read_nodes()[:, 2]. The graph is built as an edge list exactly as the header defines it; the walks are
level-synchronous over that list."""
import numpy as np

from membership.abi import GM_REACH_SOURCES, GM_VIEW_HOPS

import view_census_ref as census_ref

KW = census_ref.KW
CRASH_CASES = [(n, v) for n, v, _ in census_ref.CRASH_CASES]   # (64, 8), (300, 16), (1000, 32)
CRASHED = {n: c for n, _, c in census_ref.CRASH_CASES}         # crashed after tick 12
CRASH_TICKS = (8, 13, 16)
SPARSE = census_ref.SPARSE
SPARSE_TICKS = (20, 40)
HALF = dict(n=1000, v=8, crash_tick=12, crash_count=500, crash_seed=42)
HALF_TICKS = (13, 20)
RAGGED = dict(n=100003, v=32, drop_pct=5, drop_from=0, drop_to=1000, drop_seed=42)  # 1000 crashed after tick 10, T = 11


def edges(views, failed):
    """(i, j) arrays of the edges i -> j: i and j live, i != j, the view of i holds id j + 1"""
    views = np.asarray(views, dtype=np.uint64)
    live = np.asarray(failed) == 0
    n = len(live)
    assert views.ndim == 2 and views.shape[0] == n
    i = np.repeat(np.arange(n, dtype=np.int64), views.shape[1])
    e = views.reshape(-1)
    ids = (e >> np.uint64(32)).astype(np.int64)
    held = e != 0
    assert ((ids[held] >= 1) & (ids[held] <= n)).all()
    j = ids - 1
    ok = held & live[i] & (j != i)
    ok[ok] &= live[j[ok]]
    return i[ok], j[ok]


def levels(views, failed, sources, direction):
    """dist int64 [nsrc][n]: the length of the shortest path source -> x ("out") / x -> source ("in"),
    -1 = none. A crashed source has no distances at all."""
    assert direction in ("out", "in")
    i, j = edges(views, failed)
    a, b = (i, j) if direction == "out" else (j, i)  # a word travels a -> b
    order = np.argsort(b, kind="stable")
    a, b = a[order], b[order]
    heads, starts = np.unique(b, return_index=True)
    n = len(failed)
    sources = np.asarray(sources, dtype=np.int64)
    assert sources.ndim == 1 and 1 <= len(sources) <= GM_REACH_SOURCES and ((sources >= 0) & (sources < n)).all()
    seen = np.zeros(n, dtype=np.uint64)
    for k, s in enumerate(sources):
        if not failed[s]:
            seen[s] |= np.uint64(1) << np.uint64(k)
    front = seen.copy()
    dist = np.full((len(sources), n), -1, dtype=np.int64)
    h = 0
    while front.any():
        for k in range(len(sources)):
            dist[k, ((front >> np.uint64(k)) & np.uint64(1)) != 0] = h
        nxt = np.zeros(n, dtype=np.uint64)
        if len(a):
            nxt[heads] = np.bitwise_or.reduceat(front[a], starts)
        front = nxt & ~seen
        seen |= front
        h += 1
    return dist


def expected(views, failed, sources, direction, max_hops):
    """(counts uint64 [GM_VIEW_HOPS][GM_REACH_SOURCES], seen uint64 [n], info [live, hops, stopped, live
    sources]) as gm_view_reach defines them"""
    assert 1 <= max_hops <= GM_VIEW_HOPS
    failed = np.asarray(failed)
    dist = levels(views, failed, sources, direction)
    counts = np.zeros((GM_VIEW_HOPS, GM_REACH_SOURCES), dtype=np.uint64)
    seen = np.zeros(len(failed), dtype=np.uint64)
    for k in range(len(dist)):
        d = dist[k]
        within = (d >= 0) & (d < max_hops)
        counts[:max_hops, k] = np.bincount(d[within], minlength=max_hops)[:max_hops]
        seen[within] |= np.uint64(1) << np.uint64(k)
    rows = np.flatnonzero(counts.any(axis=1))
    info = [int((failed == 0).sum()), int(rows[-1]) if len(rows) else 0, int(counts[max_hops - 1].any()),
            int(sum(1 for s in np.asarray(sources) if not failed[s]))]
    return counts, seen, info


def as_walk(exp, nsrc):
    """the reference's result in the shape Simulator.view_reach() returns"""
    counts, seen, info = exp
    return {"counts": counts[:, :nsrc].copy(), "live": info[0], "hops": info[1], "stopped": bool(info[2]),
            "live_sources": info[3], "seen": seen}


def assert_walk(got, exp, what):
    counts, seen, info = exp
    nsrc = got["counts"].shape[1]
    assert got["counts"].shape == (GM_VIEW_HOPS, nsrc), what
    assert not counts[:, nsrc:].any(), what
    bad = np.argwhere(got["counts"] != counts[:, :nsrc])
    assert not len(bad), (f"{what}: counts differ at {len(bad)} places, first (hop, source) {tuple(bad[0])}: "
                          f"{got['counts'][tuple(bad[0])]} != {counts[tuple(bad[0])]}")
    assert [got["live"], got["hops"], int(got["stopped"]), got["live_sources"]] == info, f"{what}: info"
    if got["seen"] is not None:
        bad = np.flatnonzero(got["seen"] != seen)
        assert not len(bad), f"{what}: seen differs for {len(bad)} nodes, first {bad[0]}: {got['seen'][bad[0]]:#x} != {seen[bad[0]]:#x}"


def sources_for(n, failed, nsrc=GM_REACH_SOURCES, seed=1):
    """nsrc sources drawn by a seeded rng; from 4 sources on they always hold node 0, node n - 1, one
    crashed node where there is one, and one node named twice"""
    rng = np.random.default_rng(seed)
    src = rng.integers(0, n, size=nsrc).astype(np.int32)
    if nsrc >= 4:
        src[0], src[1] = 0, n - 1
        crashed = np.flatnonzero(np.asarray(failed) != 0)
        if len(crashed):
            src[2] = crashed[len(crashed) // 2]
        src[-1] = src[3]
    return src


# ---- what each case must contain, asserted from the expected arrays (so the conditions can be checked
# against the oracle alone). out / inn: expected(..., "out" / "in", GM_VIEW_HOPS) of the case's sources
def reached(exp):
    return exp[0].sum(axis=0).astype(np.int64)


def proves_strongly_connected(out, inn):
    live = out[2][0]
    src = out[0][0] == 1
    return bool((src & (reached(out) == live) & (reached(inn) == live)).any())


def check_crash_case(out, inn):
    """strongly connected, and far enough to walk: at least 3 non-empty levels. The level sizes are
    not pinned."""
    assert proves_strongly_connected(out, inn)
    for exp in (out, inn):
        assert exp[2][1] >= 2 and not exp[2][2], "fewer than 3 non-empty levels, or a stopped walk"


def check_sparse_case(t, out, inn):
    live, src = out[2][0], out[0][0] == 1
    assert src.any() and src.sum() == out[2][3], "no crashed node in this case: every source is live"
    if t == 20:
        assert (reached(out)[src] < live).any(), "every source reaches every live node"
        assert len(set(reached(inn)[src].tolist())) > 1, "in-reach does not differ between the sources"
    if t == 40:  # every view holds only its own entry
        for exp in (out, inn):
            assert exp[2][1] == 0 and np.array_equal(exp[0][0] == 1, src) and not exp[0][1:].any()


def check_half_crash_case(t, out, inn):
    assert out[2][0] == 500
    assert not proves_strongly_connected(out, inn)
    if t == 13:
        for exp in (out, inn):
            assert exp[2][1] >= 7, "fewer than 8 non-empty levels"


def check_ragged_case(out, inn, failed):
    assert failed[-1] == 0 and int((np.asarray(failed) != 0).sum()) == 1000
    for exp in (out, inn):
        assert exp[1][-1] != 0, "the last node is in nobody's walk"
        assert exp[2][1] >= 3


# ---- chosen graphs for Simulator.load_views (t = 40): every entry hb = 2(t - 1) - 1, heartbeat
# 2(t - 1), all counts 0 -- the load contract holds with no inboxes
GRAPH_T = 40
GRAPH_N = 101   # no multiple of 64 / V for V = 5 (12 views per wave step) and V = 24 (2)


def graph_state(n, v, adj, crashed=(), t=GRAPH_T):
    """a view snapshot (membership.state form) whose node i holds itself and adj[i]"""
    views = np.zeros((n, v), dtype=np.uint64)
    for i in range(n):
        ids = np.array(sorted(set([i] + list(adj.get(i, ())))), dtype=np.uint64) + np.uint64(1)
        assert len(ids) <= v, f"node {i}: {len(ids)} entries in a view of {v}"
        views[i, :len(ids)] = (ids << np.uint64(32)) | np.uint64(2 * (t - 1) - 1)
    failed = np.zeros(n, dtype=np.int32)
    failed[list(crashed)] = 1
    return {"t": t, "n0": 0, "views": views, "heartbeat": np.full(n, 2 * (t - 1), dtype=np.int32), "failed": failed,
            "targets": np.zeros((n, 5), dtype=np.int32), "counts": np.zeros(n, dtype=np.int32)}


def chain_graph(length=100):
    """0 -> 1 -> ... -> length - 1"""
    return {i: [i + 1] for i in range(length - 1)}


def bridge_graph(k):
    """two cliques of k nodes, [0, k) and [k, 2k), and the one-way edge 0 -> k"""
    adj = {i: [j for j in range(k) if j != i] for i in range(k)}
    adj.update({k + i: [k + j for j in range(k) if j != i] for i in range(k)})
    adj[0] = adj[0] + [k]
    return adj


def path_graph(length=21):
    """0 <-> 1 <-> ... <-> length - 1"""
    return {i: [j for j in (i - 1, i + 1) if 0 <= j < length] for i in range(length)}
