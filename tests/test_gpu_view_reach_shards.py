"""PARTIAL: view-graph reachability across row shards (gm_view_reach_loopback, gm_view_reach on an RCCL
rank): the frontier exchanged between the members once per level.

Every comparison is exact: the walk of a group against view_reach_ref.expected() of the group's own
concatenated read_views() and the cluster's crash flags, both directions, with seen. Each case's property is
asserted from the expected arrays alone, as view_reach_ref.check_* do.

 1. crash and fade on uneven shards, beside a single context of the same configuration
 2. half of the cluster crashed, G = 8
 3. self-only views: both walks end at level 0
 4. chosen graphs loaded into G = 3 shards of n = 101, walked before any tick (the exchange still pending):
    a chain across both boundaries, two cliques around a shard of self-only views, a crashed cut vertex on
    a boundary, a whole shard crashed; per-node distances from max_hops = 1 .. 8
 5. many workgroups, a ragged tail
 6. RCCL with one rank
 7. no side effects: a walked group ticks like an unwalked twin, ticked or freshly loaded
 8. the contract
"""
import ctypes

import numpy as np
import pytest

import view_reach_ref as ref
from membership import GM_MODE_PARTIAL, GM_MODE_SCALED, GmError, Simulator, crash_set, state
from membership.abi import (GM_REACH_SOURCES, GM_VIEW_HOPS, comm_unique_id, load_library, partial_loopback_tick,
                            partial_loopback_view_reach)

pytestmark = pytest.mark.gpu

GM_EINVAL, GM_ERANGE, GM_ESTATE, GM_EUNSUPPORTED = -1, -4, -5, -6


def _sim(n, v, **kw):
    return Simulator(n, GM_MODE_PARTIAL, view=v, init_mode=1, **dict(ref.KW, **kw))


def _group(n, v, world, **kw):
    return [_sim(n, v, shard_rank=g, shard_count=world, **kw) for g in range(world)]


def _tick(sims):
    if len(sims) == 1:
        sims[0].tick()
    else:
        partial_loopback_tick(sims)


def _run_to(groups, until, crash_tick=-1, crash=()):
    """every group ticked until its last tick is `until`; the crash set falls after crash_tick"""
    while groups[0][0].time - 1 < until:
        t = groups[0][0].time
        for sims in groups:
            _tick(sims)
            if t == crash_tick:
                for s in sims:
                    s.set_failed(crash)


def _cluster(sims):
    """(views [n][V], failed [n]) of the whole cluster from the members' own read-backs"""
    views = np.concatenate([s.read_views(*s.shard_layout()) for s in sims])
    failed = np.concatenate([s.read_nodes()[:, 2] for s in sims])
    assert len(views) == len(failed) == sims[0].n
    return views, failed


def _walk(sims, src, d, max_hops=GM_VIEW_HOPS):
    return partial_loopback_view_reach(sims, src, d, max_hops=max_hops, seen=True)


def _same_walk(a, b, what):
    assert a.keys() == b.keys()
    for key in a:
        assert np.array_equal(a[key], b[key]), f"{what}: {key}"


def _check(sims, sources=None, max_hops=GM_VIEW_HOPS, counts=(64, 37, 1), one=None):
    """both directions of the group == expected(its own read-backs), with seen; sources None: the case's
    sources, one run per entry of `counts`. one: a single context of the same state, whose walks must be
    identical. Returns (out, inn, sources, failed) of the first run's expected side."""
    views, failed = _cluster(sims)
    runs = [sources] if sources is not None else [ref.sources_for(sims[0].n, failed, k) for k in counts]
    first = None
    for src in runs:
        exp = []
        for d in ("out", "in"):
            what = f"tick {sims[0].time - 1}, {d}, {len(src)} sources, max_hops {max_hops}, G = {len(sims)}"
            exp.append(ref.expected(views, failed, src, d, max_hops))
            got = _walk(sims, src, d, max_hops)
            assert got["seen"].shape == (sims[0].n,)
            ref.assert_walk(got, exp[-1], what)
            if one is not None:
                _same_walk(got, one.view_reach(src, d, max_hops=max_hops, seen=True), what + " vs one context")
        first = first or (exp[0], exp[1], src, failed)
    return first


# ---- 1. crash and fade on uneven shards
@pytest.mark.parametrize("n,v,world", [(64, 8, 2), (300, 16, 7), (1000, 32, 3)])
def test_crash_and_fade(n, v, world):
    sims, one = _group(n, v, world), [_sim(n, v)]
    assert len({s.shard_layout()[1] for s in sims}) > 1 or n % world == 0
    crash = crash_set(n, ref.CRASHED[n], 42)
    for t in ref.CRASH_TICKS:
        _run_to([sims, one], t, 12, crash)
        out, inn, src, failed = _check(sims, one=one[0])
        assert sims[0].time - 1 == t and int((failed != 0).sum()) == (len(crash) if t > 12 else 0)
        assert len(src) == 64 and (t <= 12 or failed[src[2]] != 0) and src[-1] == src[3]  # a crashed source, a node twice
        ref.check_crash_case(out, inn)
    assert all(s.tick_stats()["err"] == 0 for s in sims)


# ---- 2. half of the cluster crashed
def test_half_cluster_crash():
    c = ref.HALF
    n, v, world = c["n"], c["v"], 8
    sims = _group(n, v, world)
    assert [s.shard_layout()[1] for s in sims] == [125] * world
    crash = crash_set(n, c["crash_count"], c["crash_seed"])
    for t in ref.HALF_TICKS:
        _run_to([sims], t, c["crash_tick"], crash)
        out, inn, src, failed = _check(sims, counts=(64,))
        ref.check_half_crash_case(t, out, inn)
    assert all(s.tick_stats()["err"] == 0 for s in sims)


# ---- 3. self-only views
def test_self_only_views():
    c = dict(ref.SPARSE)
    n, v = c.pop("n"), c.pop("v")
    sims = _group(n, v, 3, **c)
    _run_to([sims], 40)
    out, inn, src, failed = _check(sims, counts=(64,))
    ref.check_sparse_case(40, out, inn)
    for d in ("out", "in"):  # every member leaves the loop at level 0: the call returns, with one row
        got = _walk(sims, src, d)
        assert got["hops"] == 0 and not got["stopped"] and not got["counts"][1:].any()
    assert all(s.tick_stats()["err"] == 0 for s in sims)


# ---- 4. chosen graphs, loaded into shards and walked before any tick
def clique_pair_graph(n, k):
    """two cliques of k nodes, [0, k) and [n - k, n), and the one-way edge 0 -> n - k"""
    adj = {i: [j for j in range(k) if j != i] for i in range(k)}
    adj.update({n - k + i: [n - k + j for j in range(k) if j != i] for i in range(k)})
    adj[0] = adj[0] + [n - k]
    return adj


def path_over(lo, hi):
    """lo <-> lo + 1 <-> ... <-> hi"""
    return {i: [j for j in (i - 1, i + 1) if lo <= j <= hi] for i in range(lo, hi + 1)}


def ring_graph(n, skip):
    """i -> i + 1 and i -> i + skip, mod n"""
    return {i: [(i + 1) % n, (i + skip) % n] for i in range(n)}


def _loaded(n, v, adj, crashed=()):
    """G = 3 shards holding the graph, the exchange of the loaded state still pending"""
    sims = _group(n, v, 3)
    assert [s.shard_layout()[0] for s in sims] == [0, 33, 67]
    snap = ref.graph_state(n, v, adj, crashed)
    for s in sims:
        state.view_restore(s, state.slice_rows(snap, *s.shard_layout()))
        assert s.time == ref.GRAPH_T
    return sims


def _distances(sims, source, direction, upto=8):
    dist = np.full(sims[0].n, -1, dtype=np.int64)
    for h in range(1, upto + 1):
        seen = _walk(sims, [source], direction, h)["seen"]
        dist[(seen != 0) & (dist < 0)] = h - 1
    return dist


def _check_distances(sims, source, direction):
    want = ref.levels(*_cluster(sims), [source], direction)[0]
    assert np.array_equal(_distances(sims, source, direction), np.where(want < 8, want, -1))
    return want


@pytest.mark.parametrize("v", [5, 24])
def test_chosen_graphs(v):
    n = ref.GRAPH_N
    # a chain 0 -> ... -> 99
    sims = _loaded(n, v, ref.chain_graph(100))
    out, inn, _, _ = _check(sims, np.array([20, 99, 0, 100, 66, 67], dtype=np.int32))
    assert out[2][2] == 1 and out[2][1] == GM_VIEW_HOPS - 1 and (out[0][:, 0] == 1).all()  # OUT from 20: stopped
    assert np.flatnonzero(out[1] & np.uint64(1)).tolist() == list(range(20, 20 + GM_VIEW_HOPS))  # across 33 and 67
    assert np.flatnonzero(inn[1] & np.uint64(2)).tolist() == list(range(99 - GM_VIEW_HOPS + 1, 100))  # IN to 99: 67 | 66
    want = _check_distances(sims, 20, "out")
    assert want[27] == 7 and want[19] == -1
    want = _check_distances(sims, 70, "in")
    assert want[63] == 7 and want[71] == -1
    # two cliques at the ends, shard 1 holds only self-only views
    k = 4 if v == 5 else 20
    sims = _loaded(n, v, clique_pair_graph(n, k))
    views, _ = _cluster(sims)
    assert ((views[33:67] != 0).sum(axis=1) == 1).all()
    out, inn, _, _ = _check(sims, np.array([1, n - 1, 0, n - k, 50], dtype=np.int32))
    assert ref.reached(out)[:5].tolist() == [2 * k, k, 2 * k, k, 1]
    assert ref.reached(inn)[:5].tolist() == [k, 2 * k, k, 2 * k, 1]
    assert out[2][1] == 3 and inn[2][1] == 3
    assert _check_distances(sims, 1, "out").max() == 3 and _check_distances(sims, n - 1, "in").max() == 3
    # a two-way path over 23 .. 43 whose node 33 -- the first node of shard 1 -- is crashed
    sims = _loaded(n, v, path_over(23, 43), crashed=[33])
    out, inn, _, failed = _check(sims, np.array([23, 33, 43, 32, 34], dtype=np.int32))
    assert failed[33] == 1 and failed.sum() == 1
    assert ref.reached(out)[:5].tolist() == [10, 0, 10, 10, 10] and ref.reached(inn)[:5].tolist() == [10, 0, 10, 10, 10]
    assert np.flatnonzero(out[1] & np.uint64(1)).tolist() == list(range(23, 33))
    assert np.flatnonzero(inn[1] & np.uint64(4)).tolist() == list(range(34, 44))
    _check_distances(sims, 23, "out")
    # every node of shard 1 crashed: i -> i + 1 stops at the shard, i -> i + 68 jumps it
    sims = _loaded(n, v, ring_graph(n, 68), crashed=range(33, 67))
    out, inn, _, failed = _check(sims, np.array([0, 40, 67, 100], dtype=np.int32))
    assert failed[33:67].all() and failed.sum() == 34 and out[2][0] == n - 34
    assert (out[1][67:] & np.uint64(1)).any() and not out[1][33:67].any() and not inn[1][33:67].any()
    assert not out[0][:, 1].any() and out[2][3] == 3
    _check_distances(sims, 0, "out")
    _check_distances(sims, 0, "in")
    # the exchange of the loaded state is still pending and still works
    partial_loopback_tick(sims)
    assert all(s.tick_stats()["err"] == 0 for s in sims)


# ---- 5. many workgroups, ragged tail
def test_many_workgroups_ragged_tail():
    c = dict(ref.RAGGED)
    n, v = c.pop("n"), c.pop("v")
    sims = _group(n, v, 3, **c)
    _run_to([sims], 11, 10, crash_set(n, 1000, 42))
    out, inn, src, failed = _check(sims, counts=(64,))
    assert sims[0].time - 1 == 11 and src[1] == n - 1
    ref.check_ragged_case(out, inn, failed)
    assert all(s.tick_stats()["err"] == 0 for s in sims)


# ---- 6. RCCL, one rank
SENTINEL = 0xA5A5A5A5A5A5A5A5


def _bufs(n):
    return (np.full((GM_VIEW_HOPS, GM_REACH_SOURCES), SENTINEL, dtype=np.uint64), np.full(n, SENTINEL, dtype=np.uint64),
            np.full(4, -7, dtype=np.int64))


def _untouched(bufs):
    return (bufs[0] == SENTINEL).all() and (bufs[1] == SENTINEL).all() and (bufs[2] == -7).all()


def _args(sources, nsrc=None, direction=0, max_hops=GM_VIEW_HOPS, counts=None, seen=None, info=None):
    src = None if sources is None else np.ascontiguousarray(sources, dtype=np.int32)
    u64 = ctypes.POINTER(ctypes.c_uint64)
    return (None if src is None else src.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
            (0 if src is None else len(src)) if nsrc is None else nsrc, direction, max_hops,
            None if counts is None else counts.ctypes.data_as(u64), None if seen is None else seen.ctypes.data_as(u64),
            None if info is None else info.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))), src


def _bad_args(n, src):
    return [dict(sources=None, nsrc=3), dict(sources=src, nsrc=0), dict(sources=src, nsrc=-1),
            dict(sources=np.zeros(65, dtype=np.int32)), dict(sources=[0, n]), dict(sources=[-1, 0]),
            dict(sources=src, direction=2), dict(sources=src, direction=-1), dict(sources=src, max_hops=0),
            dict(sources=src, max_hops=GM_VIEW_HOPS + 1)]


@pytest.mark.parametrize("forced", [False, True])
def test_rccl_single_rank(forced, monkeypatch):
    """shard_count = 1 with a communicator: gm_view_reach takes the collective path -- the agreement, the
    gather / scatter collectives, the summed rows and the combined status all run, with one rank -- and
    returns what a plain context returns. forced: the context also ticks through the row-shard exchange."""
    n, v = 300, 16
    if forced:
        monkeypatch.setenv("GM_FORCE_SHARD", "1")
    sim = _sim(n, v, shard_rank=0, shard_count=1)
    monkeypatch.delenv("GM_FORCE_SHARD", raising=False)
    sim.comm_init(comm_unique_id(), 1, 0)
    plain = _sim(n, v)
    crash = crash_set(n, ref.CRASHED[n], 42)
    for t in (8, 13, 16):
        _run_to([[sim], [plain]], t, 12, crash)
        views, failed = _cluster([sim])
        for k in (64, 5):
            src = ref.sources_for(n, failed, k)
            for d in ("out", "in"):
                what = f"tick {t}, {d}, {k} sources"
                got = sim.view_reach(src, d, seen=True)
                ref.assert_walk(got, ref.expected(views, failed, src, d, GM_VIEW_HOPS), what)
                _same_walk(got, plain.view_reach(src, d, seen=True), what + " vs a plain context")
        got = sim.view_reach(src, "out", max_hops=3, seen=True)
        ref.assert_walk(got, ref.expected(views, failed, src, "out", 3), "max_hops 3")
    src = ref.sources_for(n, failed)
    bufs = _bufs(n)
    for kw in _bad_args(n, src):
        args, keep = _args(counts=bufs[0], seen=bufs[1], info=bufs[2], **kw)
        assert sim.lib.gm_view_reach(sim.h, *args) == GM_EINVAL and _untouched(bufs), kw
    args, keep = _args(src, seen=bufs[1])
    assert sim.lib.gm_view_reach(sim.h, *args) == GM_EINVAL and _untouched(bufs)  # counts and info both NULL
    sim._call("gm_load_views_begin", sim.h, sim.time)
    args, keep = _args(src, None, 0, GM_VIEW_HOPS, *bufs)
    assert sim.lib.gm_view_reach(sim.h, *args) == GM_ESTATE and _untouched(bufs)
    for s in (sim, plain):
        s.close()


# ---- 7. no side effects
def _digest_sums(sims):
    parts = [s.digest(rows=False, nodes=False) for s in sims]
    return tuple(sum(p[key] for p in parts) % (1 << 64) for key in ("table", "nodes"))


@pytest.mark.parametrize("loaded", [False, True])
def test_no_side_effects(loaded):
    n, v, world = 300, 16, 3
    crash = crash_set(n, 6, 42)
    a, b = _group(n, v, world), _group(n, v, world)
    if loaded:  # both groups freshly loaded from one context's state: the replay of tick t - 1's exchange pending
        one = [_sim(n, v)]
        _run_to([one], 14, 12, crash)
        snap = state.view_snapshot(one[0])
        for s in a + b:
            state.view_restore(s, state.slice_rows(snap, *s.shard_layout()))
    else:
        _run_to([a, b], 14, 12, crash)
    src = ref.sources_for(n, _cluster(a)[1])
    walks = {d: _walk(a, src, d) for d in ("out", "in")}
    assert all(w["hops"] >= 2 for w in walks.values())
    assert _digest_sums(a) == _digest_sums(b)
    for k in range(3):
        _tick(a)
        _tick(b)
        assert _digest_sums(a) == _digest_sums(b), f"the walked group differs after tick {k + 1}"
        assert [s.drain_events() for s in a] == [s.drain_events() for s in b]
    if loaded:  # and the loaded groups continue like the context they were taken from
        _run_to([one], a[0].time - 1)
        assert _digest_sums(a) == _digest_sums(one)
    assert all(s.tick_stats()["err"] == 0 for s in a + b)


# ---- 8. contract
def _rc(handles, sources, nsrc=None, direction=0, max_hops=GM_VIEW_HOPS, counts=None, seen=None, info=None):
    args, keep = _args(sources, nsrc, direction, max_hops, counts, seen, info)
    arr = (ctypes.c_void_p * max(len(handles), 1))(*handles)
    return load_library().gm_view_reach_loopback(arr, len(handles), *args)


def test_contract():
    n, v, world = 300, 16, 3
    sims = _group(n, v, world)
    for _ in range(3):
        partial_loopback_tick(sims)
    h = [s.h for s in sims]
    src = ref.sources_for(n, np.zeros(n, dtype=int))
    bufs = _bufs(n)
    # the group's checks
    later = _sim(n, v, shard_rank=1, shard_count=world)  # a member at another t
    assert later.time != sims[0].time
    scaled = Simulator(256, GM_MODE_SCALED, rd_seed=7, init_mode=1, init_t0=8, init_seed=11)
    groups = {"G = 1": h[:1], "a member missing": [h[0], None, h[2]], "ranks out of order": [h[1], h[0], h[2]],
              "a shard too few": h[:2], "members at different t": [h[0], later.h, h[2]],
              "a SCALED member": [h[0], scaled.h, h[2]]}
    for what, hs in groups.items():
        assert _rc(hs, src, None, 0, GM_VIEW_HOPS, *bufs) == GM_EINVAL and _untouched(bufs), what
    assert load_library().gm_view_reach_loopback(None, world, *_args(src, None, 0, GM_VIEW_HOPS, *bufs)[0]) == GM_EINVAL
    # the argument errors of gm_view_reach
    for kw in _bad_args(n, src):
        assert _rc(h, counts=bufs[0], seen=bufs[1], info=bufs[2], **kw) == GM_EINVAL and _untouched(bufs), kw
    assert _rc(h, src, seen=bufs[1]) == GM_EINVAL and _untouched(bufs)  # counts and info both NULL
    # a good call: what was not asked for is not written
    views, failed = _cluster(sims)
    for d, name in enumerate(("out", "in")):
        want = ref.expected(views, failed, src, name, GM_VIEW_HOPS)
        full = _bufs(n)
        assert _rc(h, src, None, d, GM_VIEW_HOPS, *full) == 0
        assert np.array_equal(full[0], want[0]) and np.array_equal(full[1], want[1]) and full[2].tolist() == want[2]
        part = _bufs(n)
        assert _rc(h, src, None, d, GM_VIEW_HOPS, None, None, part[2]) == 0
        assert part[2].tolist() == want[2] and (part[0] == SENTINEL).all() and (part[1] == SENTINEL).all()
    # a row shard without a communicator has nobody to walk with
    args, keep = _args(src, None, 0, GM_VIEW_HOPS, *bufs)
    assert sims[0].lib.gm_view_reach(sims[0].h, *args) == GM_EUNSUPPORTED and _untouched(bufs)
    with pytest.raises(ValueError):
        partial_loopback_view_reach(sims, src, "sideways")
    # crash sets that differ between the members
    sims[0].set_failed(crash_set(n, 6, 42))
    sims[1].set_failed(crash_set(n, 6, 43))
    sims[2].set_failed(crash_set(n, 6, 42))
    assert _rc(h, src, None, 0, GM_VIEW_HOPS, *bufs) == GM_ESTATE and _untouched(bufs)
    with pytest.raises(GmError) as e:
        partial_loopback_view_reach(sims, src)
    assert e.value.code == GM_ESTATE
    # a member between gm_load_views_begin and its commit
    fresh = _group(n, v, world)
    fresh[2]._call("gm_load_views_begin", fresh[2].h, fresh[2].time)
    assert _rc([s.h for s in fresh], src, None, 1, GM_VIEW_HOPS, *bufs) == GM_ESTATE and _untouched(bufs)
    for s in sims + fresh + [later, scaled]:
        s.close()


def test_latched_device_error_is_returned(monkeypatch):
    """GM_INBOX_CAP lowered as in tests/test_gpu_view_reach.py: the group's first ticks overflow their inboxes;
    the walk returns the latched GM_ERANGE and writes nothing"""
    monkeypatch.setenv("GM_INBOX_CAP", "2")
    sims = [Simulator(512, GM_MODE_PARTIAL, view=32, view_seed=5, rd_seed=7, init_mode=1, init_t0=8, init_seed=11,
                      shard_rank=g, shard_count=2) for g in range(2)]
    monkeypatch.delenv("GM_INBOX_CAP")
    try:
        for _ in range(2):
            partial_loopback_tick(sims)
    except GmError as e:
        assert e.code == GM_ERANGE
    bufs = _bufs(512)
    for d in (0, 1):
        assert _rc([s.h for s in sims], [0, 511], None, d, GM_VIEW_HOPS, *bufs) == GM_ERANGE and _untouched(bufs)
    for s in sims:
        s.close()
