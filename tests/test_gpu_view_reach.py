"""PARTIAL: view-graph reachability walked on the device (gm_view_reach, Simulator.view_reach).

Every comparison is exact: the walks of a context against view_reach_ref.expected() of that context's
own read_views() + read_nodes() -- the specification, pinned on the CPU by
tests/test_view_reach_summary.py, which also runs every case's check_* condition against the oracle.

 1. crash and fade: V = 8, 16 (several views per wave step, a ragged last step), V = 32
 2. sparse views under 90 % loss: partial reach, in-reach from 1 to all; then self-only views
 3. half of the cluster crashed: an overlay that is not strongly connected, walks of 8 and more levels
 4. chosen graphs through load_views (V = 5, 24): a chain past GM_VIEW_HOPS, a one-way bridge, a crashed
    cut vertex, a crashed source; per-node distances from max_hops = 1 .. 8
 5. many workgroups, a ragged tail
 6. no side effects: a walked twin stays equal to an unwalked one
 7. the contract
"""
import ctypes

import numpy as np
import pytest

import view_reach_ref as ref
from membership import (GM_MODE_FAITHFUL, GM_MODE_PARTIAL, GM_MODE_SCALED, GmError, Simulator, crash_set, state,
                        summarize_reach)
from membership.abi import GM_REACH_SOURCES, GM_VIEW_HOPS

pytestmark = pytest.mark.gpu

GM_EINVAL, GM_ERANGE, GM_ESTATE, GM_EUNSUPPORTED = -1, -4, -5, -6


def _sim(n, v, **kw):
    return Simulator(n, GM_MODE_PARTIAL, view=v, init_mode=1, **dict(ref.KW, **kw))


def _run_to(sim, until, crash_tick=-1, crash=()):
    while sim.time - 1 < until:
        t = sim.time
        sim.tick()
        if t == crash_tick:
            sim.set_failed(crash)


def _check(sim, sources=None, max_hops=GM_VIEW_HOPS, partial_masks=True):
    """both directions of sim == expected(its own read-backs), with seen; sources None: the case's 64
    sources, and one run each with 1 and with 37 of them. Returns (out, inn, sources, failed) of the
    expected side."""
    views = sim.read_views(0, sim.n)
    failed = sim.read_nodes()[:, 2]
    runs = [sources] if sources is not None else [ref.sources_for(sim.n, failed)]
    if sources is None and partial_masks:
        runs += [ref.sources_for(sim.n, failed, 1), ref.sources_for(sim.n, failed, 37)]
    first = None
    for src in runs:
        exp = []
        for d in ("out", "in"):
            exp.append(ref.expected(views, failed, src, d, max_hops))
            got = sim.view_reach(src, d, max_hops=max_hops, seen=True)
            ref.assert_walk(got, exp[-1], f"tick {sim.time - 1}, {d}, {len(src)} sources, max_hops {max_hops}")
        first = first or (exp[0], exp[1], src, failed)
    return first


# ---- 1. crash and fade
@pytest.mark.parametrize("n,v", ref.CRASH_CASES)
def test_crash_and_fade(n, v):
    sim = _sim(n, v)
    crash = crash_set(n, ref.CRASHED[n], 42)
    for t in ref.CRASH_TICKS:
        _run_to(sim, t, 12, crash)
        out, inn, src, failed = _check(sim)
        assert sim.time - 1 == t and int((failed != 0).sum()) == (len(crash) if t > 12 else 0)
        ref.check_crash_case(out, inn)
    assert sim.tick_stats()["err"] == 0


# ---- 2. sparse views
def test_sparse_views():
    c = dict(ref.SPARSE)
    n, v = c.pop("n"), c.pop("v")
    sim = _sim(n, v, **c)
    for t in ref.SPARSE_TICKS:
        _run_to(sim, t)
        out, inn, src, failed = _check(sim)
        ref.check_sparse_case(t, out, inn)
    assert sim.view_reach(src, "in")["hops"] == 0
    assert sim.tick_stats()["err"] == 0


# ---- 3. half of the cluster crashed
def test_half_cluster_crash():
    c = ref.HALF
    n, v = c["n"], c["v"]
    sim = _sim(n, v)
    crash = crash_set(n, c["crash_count"], c["crash_seed"])
    for t in ref.HALF_TICKS:
        _run_to(sim, t, c["crash_tick"], crash)
        out, inn, src, failed = _check(sim)
        ref.check_half_crash_case(t, out, inn)
        s = summarize_reach(sim.view_reach(src, "out"), sim.view_reach(src, "in"))
        assert s["strongly_connected"] is False and s["live"] == 500
        for name, exp in (("out", out), ("in", inn)):
            want = [500 - int(r) if live else None for r, live in zip(ref.reached(exp)[:len(src)], exp[0][0] == 1)]
            assert [x["unreached"] for x in s[name]["sources"]] == want
    assert sim.tick_stats()["err"] == 0


# ---- 4. chosen graphs through load_views
def _loaded(sim, adj, crashed=()):
    state.view_restore(sim, ref.graph_state(sim.n, sim.cfg.view, adj, crashed))
    assert sim.time == ref.GRAPH_T


def _distances(sim, source, direction, upto=8):
    """per-node distances below `upto` from the seen words of walks with max_hops = 1 .. upto"""
    dist = np.full(sim.n, -1, dtype=np.int64)
    for h in range(1, upto + 1):
        seen = sim.view_reach([source], direction, max_hops=h, seen=True)["seen"]
        dist[(seen != 0) & (dist < 0)] = h - 1
    return dist


@pytest.mark.parametrize("v", [5, 24])
def test_chosen_graphs(v):
    n = ref.GRAPH_N
    assert n % (64 // v) != 0
    sim = _sim(n, v)
    # a directed chain of 100 nodes: OUT from its head is stopped at GM_VIEW_HOPS, every row 1
    _loaded(sim, ref.chain_graph(100))
    head = sim.view_reach([0], "out", seen=True)
    assert head["stopped"] and head["hops"] == GM_VIEW_HOPS - 1 and (head["counts"][:, 0] == 1).all()
    assert np.flatnonzero(head["seen"]).tolist() == list(range(GM_VIEW_HOPS))
    back = sim.view_reach([0], "in", seen=True)
    assert not back["stopped"] and back["hops"] == 0 and back["counts"][:, 0].tolist() == [1] + [0] * (GM_VIEW_HOPS - 1)
    assert np.flatnonzero(back["seen"]).tolist() == [0]
    _check(sim, np.array([0, 99, 50, 100, 36, 99], dtype=np.int32))
    _check(sim, np.array([0, 99, 50], dtype=np.int32), max_hops=7)
    want = ref.levels(sim.read_views(0, n), sim.read_nodes()[:, 2], [0], "out")[0]
    assert np.array_equal(_distances(sim, 0, "out"), np.where(want < 8, want, -1)) and want[7] == 7
    want = ref.levels(sim.read_views(0, n), sim.read_nodes()[:, 2], [20], "in")[0]
    assert np.array_equal(_distances(sim, 20, "in"), np.where(want < 8, want, -1)) and want[13] == 7
    # two cliques joined by one one-way edge: OUT from the first covers both, IN to the first only the first
    k = v - 1
    _loaded(sim, ref.bridge_graph(k))
    out, inn, _, _ = _check(sim, np.array([1, k + 1, 0, k, 2 * k], dtype=np.int32))
    assert ref.reached(out)[:5].tolist() == [2 * k, k, 2 * k, k, 1] and ref.reached(inn)[:5].tolist() == [k, 2 * k, k, 2 * k, 1]
    assert out[2][1] == 3 and inn[2][1] == 3
    for source, d in ((1, "out"), (k + 1, "in")):
        want = ref.levels(sim.read_views(0, n), sim.read_nodes()[:, 2], [source], d)[0]
        assert want.max() == 3 and np.array_equal(_distances(sim, source, d), want)
    s = summarize_reach(sim.view_reach([1, k + 1], "out"), sim.view_reach([1, k + 1], "in"))
    assert s["strongly_connected"] is False and s["live"] == n
    # a path whose middle node is crashed at the commit: the far half is unreached; a crashed source
    _loaded(sim, ref.path_graph(21), crashed=[10])
    out, inn, _, failed = _check(sim, np.array([0, 10, 20, 9], dtype=np.int32))
    assert failed[10] == 1 and failed.sum() == 1
    assert ref.reached(out)[:4].tolist() == [10, 0, 10, 10] and ref.reached(inn)[:4].tolist() == [10, 0, 10, 10]
    got = sim.view_reach([0, 10], "out", seen=True)
    assert np.flatnonzero(got["seen"]).tolist() == list(range(10)) and got["live_sources"] == 1 and got["live"] == n - 1
    assert not got["counts"][:, 1].any()
    only = sim.view_reach([10], "in", seen=True)
    assert not only["counts"].any() and not only["seen"].any() and only["hops"] == 0 and not only["stopped"]
    # the context still ticks
    sim.tick()
    assert sim.tick_stats()["err"] == 0


# ---- 5. many workgroups, ragged tail
def test_many_workgroups_ragged_tail():
    c = dict(ref.RAGGED)
    n, v = c.pop("n"), c.pop("v")
    sim = _sim(n, v, **c)
    _run_to(sim, 11, 10, crash_set(n, 1000, 42))
    out, inn, src, failed = _check(sim, partial_masks=False)
    assert sim.time - 1 == 11 and src[1] == n - 1
    ref.check_ragged_case(out, inn, failed)
    assert sim.tick_stats()["err"] == 0


# ---- 6. no side effects
def test_no_side_effects():
    n, v = 300, 16
    a, b = _sim(n, v), _sim(n, v)
    crash = crash_set(n, 6, 42)
    src = ref.sources_for(n, np.zeros(n, dtype=int))
    events = 0
    for k in range(20):
        t = a.time
        a.tick()
        b.tick()
        if t == 12:
            a.set_failed(crash)
            b.set_failed(crash)
        for d in ("out", "in"):
            first = a.view_reach(src, d, seen=k % 2 == 0)
            second = a.view_reach(src, d, seen=k % 2 == 0)
            assert first.keys() == second.keys()
            for key in first:
                assert np.array_equal(first[key], second[key]), f"two walks of one state differ at tick {t}: {key}"
            assert first["hops"] >= 2
        assert a.dump_tables() == b.dump_tables(), f"views differ at tick {t}"
        ea, eb = a.drain_events(), b.drain_events()
        assert ea == eb, f"events differ at tick {t}"
        events += len(ea)
    assert events > 0
    assert np.array_equal(a.read_nodes(), b.read_nodes())
    assert a.tick_stats() == b.tick_stats() and a.tick_stats()["err"] == 0
    for x, y in zip(a.view_census(), b.view_census()):
        assert np.array_equal(x, y)
    da, db = a.digest(), b.digest()
    assert da["table"] == db["table"] and da["nodes"] == db["nodes"]
    assert np.array_equal(da["rows"], db["rows"]) and np.array_equal(da["node_words"], db["node_words"])


# ---- 7. contract
SENTINEL = 0xA5A5A5A5A5A5A5A5


def _bufs(n):
    return (np.full((GM_VIEW_HOPS, GM_REACH_SOURCES), SENTINEL, dtype=np.uint64), np.full(n, SENTINEL, dtype=np.uint64),
            np.full(4, -7, dtype=np.int64))


def _rc(sim, sources, nsrc=None, direction=0, max_hops=GM_VIEW_HOPS, counts=None, seen=None, info=None):
    src = None if sources is None else np.ascontiguousarray(sources, dtype=np.int32)
    u64 = ctypes.POINTER(ctypes.c_uint64)
    return sim.lib.gm_view_reach(sim.h, None if src is None else src.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                 (0 if src is None else len(src)) if nsrc is None else nsrc, direction, max_hops,
                                 None if counts is None else counts.ctypes.data_as(u64),
                                 None if seen is None else seen.ctypes.data_as(u64),
                                 None if info is None else info.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)))


def _untouched(bufs):
    return (bufs[0] == SENTINEL).all() and (bufs[1] == SENTINEL).all() and (bufs[2] == -7).all()


def test_contract():
    n, v = 300, 16
    others = (Simulator(10, GM_MODE_FAITHFUL),
              Simulator(256, GM_MODE_SCALED, rd_seed=7, init_mode=1, init_t0=8, init_seed=11),
              _sim(n, v, shard_rank=0, shard_count=2))
    for other in others:
        bufs = _bufs(n)
        assert _rc(other, [0, 1], None, 0, 4, *bufs) == GM_EUNSUPPORTED and _untouched(bufs)
    sim = _sim(n, v)
    _run_to(sim, 11)
    src = ref.sources_for(n, np.zeros(n, dtype=int))
    bufs = _bufs(n)
    bad = [dict(sources=None, nsrc=3), dict(sources=src, nsrc=0), dict(sources=src, nsrc=-1),
           dict(sources=np.zeros(65, dtype=np.int32)), dict(sources=[0, n]), dict(sources=[-1, 0]),
           dict(sources=src, direction=2), dict(sources=src, direction=-1), dict(sources=src, max_hops=0),
           dict(sources=src, max_hops=GM_VIEW_HOPS + 1)]
    for kw in bad:
        assert _rc(sim, counts=bufs[0], seen=bufs[1], info=bufs[2], **kw) == GM_EINVAL, kw
        assert _untouched(bufs), kw
    assert _rc(sim, src, seen=bufs[1]) == GM_EINVAL and _untouched(bufs)  # counts and info both NULL
    assert sim.lib.gm_view_reach(None, None, 0, 0, 1, None, None, None) == GM_EINVAL
    views, failed = sim.read_views(0, n), sim.read_nodes()[:, 2]
    for d, name in enumerate(("out", "in")):
        want = ref.expected(views, failed, src, name, GM_VIEW_HOPS)
        full = _bufs(n)
        assert _rc(sim, src, None, d, GM_VIEW_HOPS, *full) == 0
        assert np.array_equal(full[0], want[0]) and np.array_equal(full[1], want[1]) and full[2].tolist() == want[2]
        part = _bufs(n)  # counts NULL with info given, and seen NULL: what was not asked for is not written
        assert _rc(sim, src, None, d, GM_VIEW_HOPS, None, None, part[2]) == 0
        assert part[2].tolist() == want[2] and (part[0] == SENTINEL).all() and (part[1] == SENTINEL).all()
        part = _bufs(n)  # the reverse
        assert _rc(sim, src, None, d, GM_VIEW_HOPS, part[0], None, None) == 0
        assert np.array_equal(part[0], want[0]) and (part[1] == SENTINEL).all() and (part[2] == -7).all()
    # between gm_load_views_begin and the commit
    sim._call("gm_load_views_begin", sim.h, 12)
    bufs = _bufs(n)
    assert _rc(sim, src, None, 0, GM_VIEW_HOPS, *bufs) == GM_ESTATE and _untouched(bufs)
    with pytest.raises(GmError) as e:
        sim.view_reach(src)
    assert e.value.code == GM_ESTATE
    with pytest.raises(ValueError):
        sim.view_reach(src, "sideways")
    with pytest.raises(GmError) as e:
        others[0].view_reach([0])
    assert e.value.code == GM_EUNSUPPORTED
    for s in others + (sim,):
        s.close()


def test_latched_device_error_is_returned(monkeypatch):
    """GM_INBOX_CAP lowered as in tests/test_gpu_view_census.py: the first tick overflows its inboxes; the
    walk is the first call to look and returns the tick's GM_ERANGE, which stays latched"""
    monkeypatch.setenv("GM_INBOX_CAP", "2")
    sim = Simulator(512, GM_MODE_PARTIAL, view=32, view_seed=5, rd_seed=7, init_mode=1, init_t0=8, init_seed=11)
    monkeypatch.delenv("GM_INBOX_CAP")
    try:
        for _ in range(2):
            sim.tick()
    except GmError as e:
        assert e.code == GM_ERANGE
    bufs = _bufs(512)
    assert _rc(sim, [0, 511], None, 0, GM_VIEW_HOPS, *bufs) == GM_ERANGE and _untouched(bufs)
    assert _rc(sim, [0, 511], None, 1, GM_VIEW_HOPS, *bufs) == GM_ERANGE and _untouched(bufs)  # latched
    sim.close()
