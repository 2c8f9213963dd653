"""State digests computed on the device (gm_digest, Simulator.digest, the per-tick recorder).

Every comparison is exact. `_check` compares the digest of a context -- words and sums -- with
membership.digest (the NumPy definition) over the read-backs of the same context, and, where an oracle
runs beside it, over the oracle's state; the oracle cases are also pinned by tests/golden/digest.
The configurations are those of tests/test_gpu_census.py, whose `_check_*` conditions assert from the
expected arrays that each case holds what it is there for.

 1. crash window: stored bytes, then (tick 26) the crashed subjects' cells in escape lists; frozen rows
 2. cold start: every cell an escape entry, lists in the pool
 3. the band fast path with three bands
 4. keyed loss: old and lagging entries of live subjects
 5. a loaded state without a tick; state.verify; two band widths
 6. column shards: words add up
 7. the join ramp (and a crash on it)
 8. PARTIAL: view widths 32 / 20 / 5, frozen views, row shards, a loaded view state
 9. the recorder against digests taken on demand; no side effects
10. the contract
"""
import copy
import ctypes

import numpy as np
import pytest

import digest_cases
import oracle_py
import partial_states
import test_gpu_census as cen
from membership import GM_MODE_FAITHFUL, GM_MODE_PARTIAL, GM_MODE_SCALED, GmError, Simulator, crash_set, digest, state
from membership.abi import partial_loopback_tick
from membership.sharded import loopback_tick

pytestmark = pytest.mark.gpu

GM_EINVAL, GM_ESTATE, GM_EUNSUPPORTED = -1, -5, -6
PKW = dict(digest_cases.PKW, init_mode=1, **digest_cases.PLOSS)


def _same(got, want, what):
    for k in ("rows", "node_words"):
        bad = np.flatnonzero(got[k] != want[k])
        assert not len(bad), f"{what}: {k} differ for {len(bad)} nodes, first {bad[0]}"
    assert (got["table"], got["nodes"]) == (want["table"], want["nodes"]), f"{what}: sums differ"
    assert got["r0"] == want["r0"] and not len(digest.diff(got, want))


def _check(sim, ora=None):
    """digest of sim == the definition over its own read-backs (== over the oracle's state); returns
    (digest, hb, ts, state4) -- for a PARTIAL context (digest, views, None, state4)"""
    got = sim.digest()
    st = sim.read_nodes()
    tg, cnt = sim.read_targets()
    t = sim.time - 1
    if sim.mode == GM_MODE_PARTIAL:
        n0, nloc = sim.shard_layout()
        a, b = sim.read_views(n0, nloc), None
        want = digest.reference_views(a, st, tg, cnt, n0)
    else:
        a, b = sim.read_table()
        want = digest.reference(a, b, st, tg, cnt, sim.shard_layout()[0])
    _same(got, want, f"tick {t} vs the read-backs")
    if ora is not None:
        assert ora.time - 1 == t
        otg, ocnt = ora.targets()
        if sim.mode == GM_MODE_PARTIAL:
            owant = digest.reference_views(ora.views(), ora.nodes(), otg, ocnt)
        else:
            owant = digest.reference(*ora.table(), ora.nodes(), otg, ocnt)
        _same(got, owant, f"tick {t} vs the oracle")
    return got, a, b, st


def _golden(name, t, got):
    g = digest_cases.load()["cases"][name][str(t)]
    assert (f"{got['table']:016x}", f"{got['nodes']:016x}") == (g["table"], g["nodes"]), f"{name} tick {t}"


# ---- 1. crash window
@pytest.mark.parametrize("n,band,with_oracle", [(300, 64, True), (1100, 512, False), (1540, 1024, False)])
def test_crash_window(n, band, with_oracle):
    seen = set()
    for t, sim, ora in cen._crash_run(n, band, 45, ora=with_oracle):
        if t not in (9, 22, 26, 45):
            continue
        got, hb, ts, st = _check(sim, ora)
        failed = st[:, 2]
        if with_oracle:
            _golden("scaled_n300_crash", t, got)
        if t == 26:  # the crashed subjects' cells are in escape lists; the crashed rows are frozen at tick 10
            cen._check_escaped_crashed(hb, ts, failed, t)
            frozen = [r for r in np.flatnonzero(failed) if ts[r, r] == 10 and (hb[r] >= 0).sum() > 1]
            assert frozen and all(got["rows"][r] != 0 for r in frozen), "no crashed row based at another tick"
        seen.add(t)
    assert seen == {9, 22, 26, 45}
    assert sim.tick_stats()["err"] == 0


# ---- 2. cold start
@pytest.mark.parametrize("n,band,with_oracle", [(96, 64, True), (1100, 512, False)])
def test_cold_start(n, band, with_oracle):
    k = dict(rd_seed=7, init_mode=0)
    ora = oracle_py.Oracle(n, oracle_py.OC_SCALED, **k) if with_oracle else None
    sim = Simulator(n, GM_MODE_SCALED, band=band, **k)
    while ora is not None and ora.time < sim.time:
        ora.tick()
    shortest = []
    for ticks in (0, 1, 2):
        for _ in range(ticks):
            sim.tick()
            if ora is not None:
                ora.tick()
        got, hb, ts, st = _check(sim, ora)
        t = sim.time - 1
        shortest.append(cen._check_all_escaped(hb, ts, st[:, 2], t, band, every=t <= 1))
        if with_oracle and t >= 1:
            _golden("scaled_n96_cold", t, got)
        if t == 0:  # every cell a present {0, 0}: not the digest of an empty table
            assert (hb == 0).all() and got["rows"].all() and len(set(got["rows"].tolist())) == 1
    assert sim.time - 1 == 3
    if n >= 1100:
        assert min(shortest) > 16, "a list fits the inline slot: no pool entry was read"


# ---- 3. the fast path, three bands
def test_fast_path_three_bands():
    n = 2564  # 3072 padded columns
    sim = Simulator(n, GM_MODE_SCALED, band=1024, **dict(cen.KW, init_mode=1))
    for k in range(15):
        sim.tick()
        if k in (0, 14):
            got, hb, ts, st = _check(sim)
    assert (hb >= 0).all() and len(set(got["rows"].tolist())) == n
    assert sim.tick_stats()["err"] == 0


# ---- 4. keyed loss
def test_keyed_loss():
    n = 600
    sim = Simulator(n, GM_MODE_SCALED, **cen.KW_LOSS)
    old = lagging = 0
    while sim.time <= 45:
        t = sim.time
        sim.tick()
        if t in (25, 39, 45):
            got, hb, ts, st = _check(sim)
            a, b = cen._check_old_live(hb, ts, st[:, 2], t)
            old, lagging = old + a, lagging + b
    assert old > 0 and lagging > 0


# ---- 5. a loaded state without a tick
def test_loaded_state_without_a_tick():
    snap, row, dead, cols = cen._edited_snapshot()
    n = 96
    sims = [Simulator(n, GM_MODE_SCALED, band=band, rd_seed=7, init_mode=0) for band in (64, 512)]
    want = digest.of_snapshot(snap)
    for sim in sims:
        state.restore(sim, snap)
        got, hb, ts, st = _check(sim)
        _same(got, want, "vs the snapshot")
        assert not len(state.verify(sim, snap))
    assert len(cols) >= 10 and st[dead, 2] == 1 and snap["ts"][dead].max() < snap["t"] - 1 - 31
    assert want["rows"][dead] != 0  # the long-dead row, which only fits its own base tick, is digested
    edited = copy.deepcopy(snap)
    edited["ts"][row, cols[0]] -= 1
    for sim in sims:
        assert list(state.verify(sim, edited)) == [row]
    edited = copy.deepcopy(snap)
    edited["counts"][row] = 5 - edited["counts"][row]
    assert list(state.verify(sims[0], edited)) == [row]
    # a column cut of the snapshot against the whole context: verify slices nothing here, widths are equal
    assert not len(digest.diff(sims[0].digest(), sims[1].digest()))


# ---- 6. column shards
def test_column_shards():
    n, world = 600, 3
    k = dict(rd_seed=7, init_mode=1, init_t0=6, init_seed=5)
    ref = Simulator(n, GM_MODE_SCALED, **k)
    shards = [Simulator(n, GM_MODE_SCALED, shard_rank=g, shard_count=world, **k) for g in range(world)]
    assert shards[1].lib.gm_digest_record(shards[1].h, 30) == GM_EUNSUPPORTED
    crash = crash_set(n, 9, 42)
    checked = 0
    while ref.time <= 24:
        t = ref.time
        ref.tick()
        loopback_tick(shards)
        if t == 8:
            for s in [ref] + shards:
                s.set_failed(crash)
        if t in (7, 16, 24):
            whole, hb, ts, st = _check(ref)
            parts = []
            for s in shards:
                c0, w = s.shard_layout()
                part = _check(s)[0]
                own = np.zeros(n, dtype=bool)
                own[c0:c0 + w] = True
                assert not part["node_words"][~own].any() and part["node_words"][own].all()
                assert np.array_equal(part["rows"], digest.row_words(hb[:, c0:c0 + w], ts[:, c0:c0 + w], c0))
                parts.append(part)
            _same(digest.merge_columns(parts), whole, f"merged shards at tick {t}")
            checked += 1
            if t == 24:
                cen._check_escaped_crashed(hb, ts, st[:, 2], t)
    assert checked == 3


# ---- 7. join ramp
@pytest.mark.parametrize("crash_tick,crash_count", [(-1, 0), (5, 6)])
def test_join_ramp(crash_tick, crash_count):
    n = 64
    ora = oracle_py.Oracle(n, oracle_py.OC_SCALED, rd_seed=7, init_mode=2, crash_tick=crash_tick,
                           crash_count=crash_count, crash_seed=42)
    sim = Simulator(n, GM_MODE_SCALED, rd_seed=7, init_mode=2, band=64)
    crash = crash_set(n, crash_count, 42)
    ora.tick()  # tick 0 (the context starts as of tick 0)
    _check(sim, ora)
    for t in (6, 40):
        while sim.time - 1 < t:
            now = sim.time
            sim.tick()
            ora.tick()
            if now == crash_tick:
                sim.set_failed(crash)
        got, hb, ts, st = _check(sim, ora)
        if t == 6:  # nodes 28.. have not started: an empty table, and distinct node words
            assert not st[28:, 0].any() and not (hb[28:] >= 0).any()
            assert not got["rows"][28:].any() and got["rows"][0] != 0
            assert np.array_equal(got["rows"] != 0, (hb >= 0).any(axis=1))
            assert len(set(got["node_words"].tolist())) == n
        elif crash_count == 0:
            assert st[:, 1].all()
    assert sim.tick_stats()["err"] == 0


# ---- 8. PARTIAL
def _partial(n, v, world=1):
    return [Simulator(n, GM_MODE_PARTIAL, view=v, shard_rank=g, shard_count=world, **PKW) for g in range(world)]


@pytest.mark.parametrize("v", [32, 20, 5])
def test_partial_views(v):
    n = 300
    ora = oracle_py.PartialOracle(n, v=v, crash_tick=10, crash_count=3, crash_seed=42, **digest_cases.PKW,
                                  **digest_cases.PLOSS)
    (sim,) = _partial(n, v)
    crash = crash_set(n, 3, 42)
    frozen = {}
    _check(sim)  # as created
    while sim.time <= 30:
        t = sim.time
        sim.tick()
        ora.tick()
        if t == 10:
            sim.set_failed(crash)
        if t in (9, 12, 30):
            got, views, _, st = _check(sim, ora)
            if v in (32, 5):
                _golden(f"partial_n300_v{v}", t, got)
            if t >= 12:  # a crashed observer's frozen view is digested, and stays what it was
                assert st[crash, 2].all() and (views[crash] != 0).any(axis=1).all()
                frozen.setdefault("rows", got["rows"][crash])
                assert got["rows"][crash].all() and np.array_equal(got["rows"][crash], frozen["rows"])
    assert sim.tick_stats()["err"] == 0


def test_partial_row_shards():
    n, v, world = 300, 32, 3
    (one,) = _partial(n, v)
    shards = _partial(n, v, world)
    crash = crash_set(n, 3, 42)
    for rec in [one] + shards:
        rec.digest_record(20)
    while one.time <= 14:
        t = one.time
        one.tick()
        partial_loopback_tick(shards)
        if t == 10:
            for s in [one] + shards:
                s.set_failed(crash)
        if t in (9, 11, 14):
            whole = _check(one)[0]
            parts = [_check(s)[0] for s in shards]
            assert [p["r0"] for p in parts] == [s.shard_layout()[0] for s in shards]
            _same(digest.merge_rows(parts), whole, f"merged row shards at tick {t}")
    # the shards' traces add up to the single context's
    tr = one.digest_trace(15)
    with np.errstate(over="ignore"):
        added = np.add.reduce([s.digest_trace(15) for s in shards], dtype=np.uint64)
    assert np.array_equal(added, tr) and tr[9:].all() and not tr[:9].any()


def test_partial_loaded_view_state():
    n, v, t = 128, 32, 40
    snap = partial_states.sweep_cases(n, v, t)
    (sim,) = _partial(n, v)
    state.view_restore(sim, snap)
    got = _check(sim)[0]
    _same(got, digest.of_view_snapshot(snap), "vs the view snapshot")
    assert not len(state.view_verify(sim, snap))
    edited = copy.deepcopy(snap)
    k = int(np.flatnonzero(edited["views"][7])[-1])
    edited["views"][7, k] -= np.uint64(2)  # one heartbeat
    assert list(state.view_verify(sim, edited)) == [7]
    shards = _partial(n, v, 3)
    for s in shards:
        state.view_restore(s, state.slice_rows(snap, *s.shard_layout()))
        assert not len(state.view_verify(s, snap))  # cut to the shard's nodes
    _same(digest.merge_rows([s.digest() for s in shards]), got, "row shards of the loaded state")


# ---- 9. the recorder
def _twins(make, until, crash_tick, crash, tmax):
    """two equal contexts ticked to `until`, the first recording: yields (t, recording, twin) after every
    tick, before the crash is set"""
    a, b = make(), make()
    a.digest_record(tmax)
    while a.time <= until:
        t = a.time
        a.tick()
        b.tick()
        yield t, a, b
        if t == crash_tick:
            a.set_failed(crash)
            b.set_failed(crash)


@pytest.mark.parametrize("mode", ["scaled", "partial"])
def test_recorder(mode):
    n, tmax, until = 300, 30, 34
    if mode == "scaled":
        make = lambda: Simulator(n, GM_MODE_SCALED, band=64, **dict(cen.KW, init_mode=1))  # noqa: E731
    else:
        make = lambda: _partial(n, 32)[0]  # noqa: E731
    crash = crash_set(n, 3, 42)
    want = np.zeros((tmax, 2), dtype=np.uint64)
    events = [[], []]
    for t, a, b in _twins(make, until, 10, crash, tmax):
        d = b.digest()  # on demand, right after the tick and before the crash is set
        if t < tmax:
            want[t] = d["table"], d["nodes"]
        if t in (10, 20):  # the recording context answers on demand as well, with the same words
            _same(a.digest(), d, f"tick {t}: the recording context on demand")
        events[0] += a.drain_events()
        events[1] += b.drain_events()
    trace = a.digest_trace(tmax)
    assert np.array_equal(trace, want), f"rows {np.flatnonzero((trace != want).any(axis=1))} differ"
    assert not trace[:9].any() and trace[9:].all() and len({tuple(r) for r in trace[9:].tolist()}) == tmax - 9
    assert np.array_equal(a.digest_trace(12), want[:12])
    if mode == "scaled":
        _golden("scaled_n300_crash", 9, {"table": int(trace[9, 0]), "nodes": int(trace[9, 1])})
    # no side effects: the recording context and its twin stay equal
    assert events[0] == events[1] and events[0]
    assert a.dump_tables() == b.dump_tables()
    for x, y in zip(a.read_targets(), b.read_targets()):
        assert np.array_equal(x, y)
    assert a.tick_stats() == b.tick_stats() and a.tick_stats()["err"] == 0
    with pytest.raises(GmError) as e:
        b.digest_trace(5)
    assert e.value.code == GM_ESTATE


def test_recorder_started_late_and_past_its_window():
    n = 300
    sim = Simulator(n, GM_MODE_SCALED, band=64, **dict(cen.KW, init_mode=1))
    for _ in range(3):  # ticks 9..11 unrecorded
        sim.tick()
    sim.digest_record(14)
    seen = {}
    for _ in range(4):  # ticks 12, 13 recorded; 14, 15 past the window
        t = sim.time
        sim.tick()
        d = sim.digest()
        seen[t] = (d["table"], d["nodes"])
    trace = sim.digest_trace(14)
    assert not trace[:12].any()
    assert [tuple(int(x) for x in r) for r in trace[12:]] == [seen[12], seen[13]]


# ---- 10. the contract
def _rc(sim, sums=True, rows=False, nodes=False, count=None):
    count = sim.n if count is None else count
    arrs = [np.zeros(k, dtype=np.uint64) if on else None for on, k in ((sums, 2), (rows, count), (nodes, count))]
    rc = sim.lib.gm_digest(sim.h, *[None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
                                    for a in arrs])
    return rc, arrs


def test_contract():
    faithful = Simulator(10, GM_MODE_FAITHFUL)
    assert _rc(faithful)[0] == GM_EUNSUPPORTED
    assert faithful.lib.gm_digest_record(faithful.h, 10) == GM_EUNSUPPORTED
    n = 300
    sim = Simulator(n, GM_MODE_SCALED, band=64, **dict(cen.KW, init_mode=1))
    for _ in range(3):
        sim.tick()
    assert _rc(sim, sums=False)[0] == GM_EINVAL
    full = sim.digest()
    for sums, rows, nodes in ((True, False, False), (False, True, False), (False, False, True)):
        rc, (s, r, w) = _rc(sim, sums, rows, nodes)
        assert rc == 0
        assert s is None or (int(s[0]), int(s[1])) == (full["table"], full["nodes"])
        assert r is None or np.array_equal(r, full["rows"])
        assert w is None or np.array_equal(w, full["node_words"])
    half = sim.digest(rows=False)
    assert half["rows"] is None and np.array_equal(half["node_words"], full["node_words"])
    _same(sim.digest(), full, "a second call")
    for bad in (0, -1, 32768):
        assert sim.lib.gm_digest_record(sim.h, bad) == GM_EINVAL
    assert sim.lib.gm_digest_trace(sim.h, 5, np.zeros(10, dtype=np.uint64).ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))) == GM_ESTATE
    sim.digest_record(20)
    assert sim.lib.gm_digest_record(sim.h, 20) == GM_ESTATE
    for bad in (0, 21):
        with pytest.raises(GmError) as e:
            sim.digest_trace(bad)
        assert e.value.code == GM_EINVAL
    # inside a load: GM_ESTATE until the commit; the loaded state digests as the one it was read from
    snap = state.snapshot(sim)
    assert sim.lib.gm_load_begin(sim.h, snap["t"]) == 0
    assert _rc(sim)[0] == GM_ESTATE
    state.restore(sim, snap)
    _same(sim.digest(), full, "after the load")
    sim.tick()  # tick 12: recorded, loads are allowed while recording
    d = sim.digest()
    trace = sim.digest_trace(13)
    assert (int(trace[12, 0]), int(trace[12, 1])) == (d["table"], d["nodes"]) and not trace[:12].any()
    (part,) = _partial(64, 8)
    assert part.lib.gm_load_views_begin(part.h, part.time) == 0
    assert _rc(part, count=64)[0] == GM_ESTATE
