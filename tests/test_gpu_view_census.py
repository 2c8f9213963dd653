"""PARTIAL: the view census reduced on the device (gm_view_census, Simulator.view_census).

Every comparison is exact: the census of a context against view_census_ref.expected() of that
context's own read_views() + read_nodes() -- the specification, pinned on the CPU by
tests/test_view_census_summary.py. Each case asserts from the expected arrays that it contains what
it is there for (the check_* conditions of view_census_ref, which the CPU file runs against the
oracle).

 1. crash and fade: V = 8, 16 (several views per wave step, a last partial step; 300 and 1000 are no
    multiples of 64), V = 32; as created, one tick after the crash, and faded. N = 64 at T = 9 is the
    heavy-contention case: every atomic of the launch lands on 64 records. The oracle's views hold no
    crashed node at T = 16 for N = 64 and 300; at N = 1000 one entry is left at T = 16, so that case
    is censused at T = 17 as well (view_census_ref.FADED_AT)
 2. sparse views under 90 % loss: old entries, views of 1..3 entries, orphans, self-only views
 3. stale entries of crashed subjects
 4. row shards against their own views and, merged, against a single context
 5. many workgroups, low contention, a ragged tail
 6. no side effects: a censused twin stays equal to an uncensused one
 7. the contract
"""
import ctypes

import numpy as np
import pytest

import view_census_ref as ref
from membership import (GM_MODE_FAITHFUL, GM_MODE_PARTIAL, GM_MODE_SCALED, GmError, Simulator, crash_set,
                        merge_view_shards, summarize_views)
from membership.abi import GM_VIEW_AGES, GM_VIEW_SIZES, VIEW_DTYPE, GmViewRec, partial_loopback_tick

pytestmark = pytest.mark.gpu

GM_EINVAL, GM_ERANGE, GM_EUNSUPPORTED = -1, -4, -6


def _sim(n, v, **kw):
    return Simulator(n, GM_MODE_PARTIAL, view=v, init_mode=1, **dict(ref.KW, **kw))


def _check(sim, failed_all=None):
    """census of sim == expected(its own read-backs); failed_all: the whole cluster's crash flags (a
    row shard). Returns (census, views, failed, t) of the expected side."""
    t = sim.time - 1
    n0, nloc = sim.shard_layout()
    views = sim.read_views(n0, nloc)
    failed = sim.read_nodes()[:, 2]
    want = ref.expected(views, failed, failed if failed_all is None else failed_all, t, sim.n)
    ref.assert_census(sim.view_census(), want, f"tick {t}")
    return want, views, failed, t


def _run_to(sim, until, crash_tick=-1, crash=()):
    while sim.time - 1 < until:
        t = sim.time
        sim.tick()
        if t == crash_tick:
            sim.set_failed(crash)


# ---- 1. crash and fade
@pytest.mark.parametrize("n,v,crashed", ref.CRASH_CASES)
def test_crash_and_fade(n, v, crashed):
    sim = _sim(n, v)
    crash = crash_set(n, crashed, 42)
    for t in ref.CRASH_TICKS[n]:
        _run_to(sim, t, 12, crash)
        census, views, failed, tt = _check(sim)
        assert tt == t
        ref.check_crash_case(t, n, v, census, failed)
    assert sim.tick_stats()["err"] == 0


# ---- 2. sparse views
def test_sparse_views():
    c = dict(ref.SPARSE)
    n, v = c.pop("n"), c.pop("v")
    sim = _sim(n, v, **c)
    for t in (20, 30, 40):
        _run_to(sim, t)
        census, views, failed, tt = _check(sim)
        assert tt == t
        ref.check_sparse_case(t, census, views, failed)
        s = summarize_views(*sim.view_census(), failed, t, v)
        ids = (views >> np.uint64(32)).astype(np.int64)
        cnt = (views != 0).sum(axis=1)
        assert s["orphans"] == int((np.bincount(ids[ids > 0] - 1, minlength=n) == 1).sum())
        assert s["view_size"] == {"min": int(cnt.min()), "mean": float(cnt.mean()), "full": float((cnt == v).mean())}
    assert s["orphans"] == n and s["view_size"]["min"] == 1
    assert sim.tick_stats()["err"] == 0


# ---- 3. stale entries of crashed subjects
def test_stale_entries_of_crashed_subjects():
    c = dict(ref.STALE_CRASHED)
    n, v, crash_tick, count = c.pop("n"), c.pop("v"), c.pop("crash_tick"), c.pop("crash_count")
    sim = _sim(n, v, **c)
    _run_to(sim, 12, crash_tick, crash_set(n, count, 42))
    census, views, failed, t = _check(sim)
    assert t == 12 and int((failed != 0).sum()) == count
    ref.check_stale_crashed_case(12, census, failed)


# ---- 4. row shards
@pytest.mark.parametrize("n,v,world", [(1000, 32, 3), (300, 16, 2)])
def test_row_shards(n, v, world):
    one = _sim(n, v)
    shards = [_sim(n, v, shard_rank=g, shard_count=world) for g in range(world)]
    crash = crash_set(n, max(1, n // 50), 42)
    _run_to(one, 13, 12, crash)
    while shards[0].time - 1 < 13:
        t = shards[0].time
        partial_loopback_tick(shards)
        if t == 12:
            for s in shards:
                s.set_failed(crash)
    whole, _, failed_all, t = _check(one)
    assert t == 13 and int((failed_all != 0).sum()) == len(crash)
    assert np.array_equal(np.concatenate([s.read_nodes()[:, 2] for s in shards]), failed_all)
    parts = []
    for s in shards:
        census, views, failed, tt = _check(s, failed_all)
        assert tt == 13 and len(views) == s.shard_layout()[1] < n and len(census[0]) == n
        assert census[2].sum() == (failed == 0).sum()
        parts.append(s.view_census())
    ref.assert_census(merge_view_shards(parts), whole, "merged row shards vs the single context")
    ref.assert_census(merge_view_shards(parts), one.view_census(), "merged row shards vs the single context's census")
    assert whole[1][1].sum() > 0, "no entry of a crashed subject"


# ---- 5. many workgroups, low contention, ragged tail
def test_many_workgroups_ragged_tail():
    n, v = 100003, 32
    sim = _sim(n, v, drop_pct=5, drop_from=0, drop_to=1000, drop_seed=42)
    _run_to(sim, 11, 10, crash_set(n, 1000, 42))
    (rec, hist, sizes), views, failed, t = _check(sim)
    assert t == 11 and int((failed != 0).sum()) == 1000 and views.nbytes == n * v * 8
    assert failed[-1] == 0 and rec["holders"][-1] > 0, "the last node's view is live"
    assert hist[1].sum() > 0 and sizes.sum() == n - 1000
    assert sim.tick_stats()["err"] == 0


# ---- 6. no side effects
def test_no_side_effects():
    n, v = 300, 16
    a, b = _sim(n, v), _sim(n, v)
    crash = crash_set(n, 6, 42)
    events = 0
    for k in range(20):
        t = a.time
        a.tick()
        b.tick()
        if t == 12:
            a.set_failed(crash)
            b.set_failed(crash)
        first = a.view_census(records=k % 2 == 0)
        second = a.view_census(records=k % 2 == 0)
        for x, y in zip(first, second):
            assert (x is None and y is None) or np.array_equal(x, y), f"two censuses of one state differ at tick {t}"
        assert (first[0] is None) == (k % 2 == 1)
        assert a.dump_tables() == b.dump_tables(), f"views differ at tick {t}"
        ea, eb = a.drain_events(), b.drain_events()
        assert ea == eb, f"events differ at tick {t}"
        events += len(ea)
    assert events > 0
    assert np.array_equal(a.read_nodes(), b.read_nodes())
    assert a.tick_stats() == b.tick_stats() and a.tick_stats()["err"] == 0


# ---- 7. contract
def _rc(sim, rec=None, hist=None, sizes=None):
    u64 = ctypes.POINTER(ctypes.c_uint64)
    return sim.lib.gm_view_census(sim.h, None if rec is None else rec.ctypes.data_as(ctypes.POINTER(GmViewRec)),
                                  None if hist is None else hist.ctypes.data_as(u64),
                                  None if sizes is None else sizes.ctypes.data_as(u64))


def _bufs(n):
    return (np.zeros(n, dtype=VIEW_DTYPE), np.zeros((2, GM_VIEW_AGES), dtype=np.uint64),
            np.zeros(GM_VIEW_SIZES, dtype=np.uint64))


def test_contract():
    for other in (Simulator(10, GM_MODE_FAITHFUL),
                  Simulator(256, GM_MODE_SCALED, rd_seed=7, init_mode=1, init_t0=8, init_seed=11)):
        assert _rc(other, *_bufs(256)) == GM_EUNSUPPORTED
    n, v = 300, 16
    sim = _sim(n, v)
    _run_to(sim, 11)
    assert _rc(sim) == GM_EINVAL
    full = _bufs(n)
    assert _rc(sim, *full) == 0
    ref.assert_census(full, _check(sim)[0], "raw call")
    for skip in range(3):
        got = _bufs(n)
        args = [None if k == skip else got[k] for k in range(3)]
        assert _rc(sim, *args) == 0
        for k in range(3):
            if k == skip:
                assert not got[k].view(np.uint8).any(), "an output that was not asked for was written"
            else:
                assert np.array_equal(got[k], full[k]), f"output {k} differs with output {skip} NULL"
    rec, hist, sizes = sim.view_census(records=False)
    assert rec is None and np.array_equal(hist, full[1]) and np.array_equal(sizes, full[2])


def test_latched_device_error_is_returned(monkeypatch):
    """GM_INBOX_CAP lowered as in tests/test_gpu_limits.py: Poisson(5) inboxes overflow 2 slots on the
    first tick; the census is the first call to look and returns the tick's GM_ERANGE"""
    monkeypatch.setenv("GM_INBOX_CAP", "2")
    sim = Simulator(512, GM_MODE_PARTIAL, view=32, view_seed=5, rd_seed=7, init_mode=1, init_t0=8, init_seed=11)
    monkeypatch.delenv("GM_INBOX_CAP")
    try:
        for _ in range(2):
            sim.tick()
    except GmError as e:
        assert e.code == GM_ERANGE
    assert _rc(sim, *_bufs(512)) == GM_ERANGE
    assert _rc(sim, *_bufs(512)) == GM_ERANGE  # latched
    sim.close()
