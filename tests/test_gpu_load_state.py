"""SCALED: a cluster state loaded into a context (gm_load_begin / gm_load_rows / gm_load_commit,
Simulator.load_state, membership.state), the inverse of read_table / read_nodes / read_targets.

Every comparison is exact, and each case asserts from its own data (the oracle's table, or the
events of the run) that it exercises what it claims; the `_check_*` functions hold those
conditions, so they can be run against the oracle alone, without a GPU.

 1. round trip: an oracle state loaded into a cold-created context reads back equal, no tick run
 2. oracle -> GPU, then 14 ticks on both sides through the TREMOVE sweep (band 64 / auto, loss 0 / 20 %)
 3. a state whose payloads need escape slots (fresh entries lagging > 13 ticks), then 8 ticks
 4. a cold-start state (every cell escaped, lists in the pool) into a warm-created context
 5. rows crashed 50 ticks ago (their entries only fit relative to their own last tick)
 6. GPU -> GPU on the band fast path, same and other band width, through the TREMOVE peak
 7. a single context's state sliced into column shards (phase loopback; pipelined loopback)
 8. the detection recorder and the event totals carry on across a load
 9. the contract: GM_EUNSUPPORTED / GM_ESTATE / GM_EINVAL / GM_ERANGE, and a clean load after a failed one
"""
import numpy as np
import pytest

import oracle_py
from golden_util import same_state
from membership import GM_EV_REMOVED, GM_MODE_FAITHFUL, GM_MODE_PARTIAL, GM_MODE_SCALED, Simulator, crash_set, state
from membership.abi import _ptr, shard_loopback_tick
from membership.sharded import loopback_tick
from test_gpu_detect import _shard_kw
from test_gpu_multiband import _compare_tick, _same_targets

pytestmark = pytest.mark.gpu

GM_EINVAL, GM_ERANGE, GM_ESTATE, GM_EUNSUPPORTED = -1, -4, -5, -6
TFAIL = 5


def _oracle_at(n, t, crash_tick=-1, crash_count=0, **kw):
    """A fresh oracle ticked until tick t runs next."""
    ora = oracle_py.Oracle(n, oracle_py.OC_SCALED, crash_tick=crash_tick, crash_count=crash_count, crash_seed=42, **kw)
    while ora.time < t:
        ora.tick()
    return ora


def _oracle_snapshot(ora):
    hb, ts = ora.table()
    st = ora.nodes()
    tg, cnt = ora.targets()
    return {"t": ora.time, "hb": hb, "ts": ts, "heartbeat": st[:, 3].copy(), "failed": st[:, 2].copy(),
            "targets": tg, "counts": cnt}


def _cell_fields(snap):
    """(present, h, age) of the 16-bit cells relative to t - 1 (gm_scaled.h)"""
    w = snap["t"] - 1
    return snap["hb"] >= 0, 255 - (2 * w - snap["hb"]), w - snap["ts"]


def _continue(sim, ora, ticks):
    events = []
    for _ in range(ticks):
        events += _compare_tick(sim, ora, sim.time)
    return events


# ---- the states, and what each must contain (CPU-checkable)
KW300 = dict(rd_seed=7, init_t0=8, init_seed=11)


def _state300(drop):
    kw = dict(KW300, init_mode=1, drop_pct=drop, drop_from=0, drop_to=1000, drop_seed=5)
    return _oracle_at(300, 25, crash_tick=10, crash_count=9, **kw), kw


def _check_state300(snap):
    pres, h, age = _cell_fields(snap)
    live = snap["failed"] == 0
    # the crashed columns' entries in live rows are stale and outside the stored byte's range, i.e. in
    # escape lists. (In this run they are 9 - 13 ticks old at the load tick and escape by their heartbeat
    # lag; they pass age 15 two ticks into the window, which _check_old_entries asserts there.)
    stale = pres & (age >= TFAIL) & live[:, None] & (snap["failed"] == 1)[None, :]
    assert stale.sum() > 0, "no stale entry in a live row at the load tick"
    assert (stale & ~((h >= 230) & (h % 2 == 0) & (age <= 14))).sum() == stale.sum(), "a stale entry fits the byte"
    assert (snap["failed"] == 1).sum() == 9


def _check_old_entries(ora):
    """from the oracle's table after a tick: entries beyond the stored byte's age range in live rows"""
    hb, ts = ora.table()
    live = ora.nodes()[:, 2] == 0
    return int(((hb >= 0) & (ora.time - 1 - ts >= 15) & live[:, None]).sum())


KW600 = dict(rd_seed=7, drop_pct=80, drop_from=6, drop_to=24, drop_seed=42, init_mode=1, init_t0=5, init_seed=43)


def _check_payload_escapes(snap):
    pres, h, age = _cell_fields(snap)
    lag = (254 - h) // 2  # ticks the entry's heartbeat is behind a live node's own (h = 254)
    sends = snap["counts"] > 0
    assert (pres & (age < TFAIL) & (lag > 13) & sends[:, None]).sum() > 0, "no fresh entry lagging more than 13 ticks"


def _check_all_escaped(snap, band):
    pres, h, age = _cell_fields(snap)
    esc = pres & ~((h >= 230) & (h % 2 == 0) & (age <= 14))
    n = esc.shape[1]
    for c in range(0, n, band):
        assert esc[:, c:c + band].sum(axis=1).min() > 16, f"a list of band {c // band} fits the inline slot"


def _check_long_dead(snap):
    dead = snap["failed"] == 1
    assert dead.sum() == 5
    newest = snap["ts"][dead].max(axis=1)
    assert (newest < snap["t"] - 1 - 31).all(), "a crashed row is not older than the 5-bit age reaches"


# ---- 1. round trip, no tick
@pytest.mark.parametrize("feed", ["whole", "blocks-reversed"])
@pytest.mark.parametrize("band", [64, 0])
def test_round_trip_without_a_tick(band, feed, monkeypatch):
    ora, kw = _state300(0)
    snap = _oracle_snapshot(ora)
    _check_state300(snap)
    if feed != "whole":
        monkeypatch.setenv("GM_LOAD_STAGE_ROWS", "7")  # blocks of 50 rows in encode launches of 7
    sim = Simulator(300, GM_MODE_SCALED, band=band, **dict(kw, init_mode=0))  # cold: nothing of it may survive
    if feed == "whole":
        state.restore(sim, snap)
    else:
        sim._call("gm_load_begin", sim.h, snap["t"])
        for r0 in reversed(range(0, 300, 50)):
            hb, ts = np.ascontiguousarray(snap["hb"][r0:r0 + 50]), np.ascontiguousarray(snap["ts"][r0:r0 + 50])
            sim._call("gm_load_rows", sim.h, r0, 50, _ptr(hb), _ptr(ts))
        sim._call("gm_load_commit", sim.h, *[_ptr(np.ascontiguousarray(snap[k])) for k in
                                             ("heartbeat", "failed", "targets", "counts")])
        assert sim.load_stats()["rows"] == 300
    assert sim.time == snap["t"]
    assert same_state(sim, ora)
    assert _same_targets(sim.read_targets(), ora.targets())
    assert sim.dump_tables() == ora.dump()
    assert sim.drain_events() == [] and sim.event_counts()[0] == 0
    assert sim.tick_stats()["err"] == 0


# ---- 2. oracle -> GPU continues
@pytest.mark.parametrize("drop", [0, 20])
@pytest.mark.parametrize("band", [64, 0])
def test_gpu_continues_from_oracle_state(band, drop):
    ora, kw = _state300(drop)
    snap = _oracle_snapshot(ora)
    _check_state300(snap)  # at band 64 the crashed columns' stale entries are in escape lists
    sim = Simulator(300, GM_MODE_SCALED, band=band, **dict(kw, init_mode=0))
    state.restore(sim, snap)
    ev, old = [], 0
    for _ in range(14):
        ev += _compare_tick(sim, ora, sim.time)
        old += _check_old_entries(ora)
    assert old > 0, "no entry of age >= 15 inside the window"
    assert sum(e[2] == GM_EV_REMOVED for e in ev) > 0, "the TREMOVE sweep is not inside the window"


# ---- 3. payload escapes on load
def test_payload_escapes_on_load():
    ora = _oracle_at(600, 24, crash_tick=9, crash_count=6, **KW600)
    snap = _oracle_snapshot(ora)
    _check_payload_escapes(snap)
    sim = Simulator(600, GM_MODE_SCALED, **KW600)
    state.restore(sim, snap)
    assert same_state(sim, ora)
    _continue(sim, ora, 8)


# ---- 4. every cell escaped, lists in the pool
def test_cold_state_into_warm_context():
    kw = dict(rd_seed=7, init_seed=11)
    ora = _oracle_at(300, 3, init_mode=0, init_t0=0, **kw)
    snap = _oracle_snapshot(ora)
    _check_all_escaped(snap, 64)
    sim = Simulator(300, GM_MODE_SCALED, band=64, init_mode=1, init_t0=8, **kw)
    state.restore(sim, snap)
    assert same_state(sim, ora)
    assert _continue(sim, ora, 3) == []


# ---- 5. a long-dead row
def test_long_dead_rows():
    kw = dict(KW300, init_mode=1)
    ora = _oracle_at(96, 60, crash_tick=10, crash_count=5, **kw)
    snap = _oracle_snapshot(ora)
    _check_long_dead(snap)
    sim = Simulator(96, GM_MODE_SCALED, **dict(kw, init_mode=0))
    state.restore(sim, snap)
    dead = snap["failed"] == 1
    hb, ts = sim.read_table()
    assert np.array_equal(hb[dead], snap["hb"][dead]) and np.array_equal(ts[dead], snap["ts"][dead])
    assert same_state(sim, ora)
    _continue(sim, ora, 6)


# ---- 6. GPU -> GPU on the fast path, no oracle
@pytest.mark.parametrize("band_b", [1024, 64])
def test_gpu_to_gpu_fast_path(band_b):
    n = 1540
    kw = dict(KW300, init_mode=1)
    a = Simulator(n, GM_MODE_SCALED, band=1024, **kw)
    crash = crash_set(n, 16, 42)
    while a.time < 29:
        t = a.time
        a.tick()
        if t == 10:
            a.set_failed(crash)
    a.drain_events()
    b = Simulator(n, GM_MODE_SCALED, band=band_b, **dict(kw, init_mode=0))
    state.restore(b, state.snapshot(a))
    removed = []
    while a.time <= 37:
        t = a.time
        a.tick()
        b.tick()
        assert a.tick_stats()["err"] == 0 and b.tick_stats()["err"] == 0, f"error flags at tick {t}"
        ev = a.drain_events()
        assert b.drain_events() == ev, f"events differ at tick {t}"
        (ha, ta), (hb, tb) = a.read_table(), b.read_table()
        assert np.array_equal(ha, hb) and np.array_equal(ta, tb), f"tables differ at tick {t}"
        assert np.array_equal(a.read_nodes(), b.read_nodes()), f"node state differs at tick {t}"
        assert _same_targets(b.read_targets(), a.read_targets()), f"gossip targets differ at tick {t}"
        removed += [e[3] for e in ev if e[2] == GM_EV_REMOVED]
    removed = np.array(removed)
    for lo in (0, 1024):  # removed subjects (ids, 1-based) in both bands of A
        assert ((removed > lo) & (removed <= lo + 1024)).sum() > 0, f"no removal in band {lo // 1024}"


# ---- 7. single context -> column shards
@pytest.mark.parametrize("n,world,how", [(600, 3, "phase"), (2048, 8, "pipelined")])
def test_single_context_into_column_shards(n, world, how, monkeypatch):
    kw = _shard_kw(0)
    ref = Simulator(n, GM_MODE_SCALED, **kw)
    crash = crash_set(n, max(2, n // 64), 42)
    while ref.time < 20:
        t = ref.time
        ref.tick()
        if t == 8:
            ref.set_failed(crash)
    ref.drain_events()
    snap = state.snapshot(ref)
    if how == "pipelined":
        monkeypatch.setenv("GM_SCHUNKS", "4")
    shards = [Simulator(n, GM_MODE_SCALED, shard_rank=g, shard_count=world, **kw) for g in range(world)]
    monkeypatch.delenv("GM_SCHUNKS", raising=False)
    for s in shards:
        state.restore(s, state.slice_columns(snap, s.shard_layout()))

    def compare(t):
        hb, ts = ref.read_table()
        got = [s.read_table() for s in shards]
        assert np.array_equal(np.concatenate([g[0] for g in got], axis=1), hb), f"hb differs at tick {t}"
        assert np.array_equal(np.concatenate([g[1] for g in got], axis=1), ts), f"ts differs at tick {t}"
        # a shard bumps the heartbeat counters of the nodes whose columns it holds: their rows, concatenated
        own = [s.read_nodes()[c0:c0 + w] for s, (c0, w) in zip(shards, (s.shard_layout() for s in shards))]
        assert np.array_equal(np.concatenate(own), ref.read_nodes()), f"node state differs at tick {t}"
        for s in shards:
            assert np.array_equal(s.read_nodes()[:, :3], ref.read_nodes()[:, :3]), f"crash flags differ at tick {t}"
            assert s.tick_stats()["err"] == 0

    compare(ref.time)
    for k in range(16):
        t = ref.time
        ref.tick()
        if how == "pipelined":
            shard_loopback_tick(shards)
        else:
            loopback_tick(shards)
        if k % 4 == 3:
            compare(t)
    assert _same_targets(shards[0].read_targets(), ref.read_targets())
    joined = state.join_columns([state.snapshot(s) for s in shards])  # and back
    full = state.snapshot(ref)
    assert joined["t"] == full["t"]
    assert all(np.array_equal(joined[k], full[k]) for k in ("hb", "ts", "heartbeat", "failed", "counts"))
    assert ref.event_totals()["removed"] > 0  # the crashed nodes' removal lies inside the run


# ---- 8. recorders across a load
def test_recorders_carry_on_across_a_load():
    n = 300
    kw = dict(KW300, init_mode=1)
    sims = [Simulator(n, GM_MODE_SCALED, **kw) for _ in range(2)]
    crash = crash_set(n, 9, 42)
    for s in sims:
        s.detect_record(60)
    while sims[0].time <= 40:
        t = sims[0].time
        for s in sims:
            s.tick()
            if t == 10:
                s.set_failed(crash)
        if t == 20:
            state.restore(sims[0], state.snapshot(sims[0]))  # mid-run, its own state
    x, twin = sims
    assert twin.event_totals()["removed"] > 0
    assert x.event_totals() == twin.event_totals()
    assert np.array_equal(x.detect(), twin.detect())
    assert np.array_equal(x.detect_timeline(41), twin.detect_timeline(41))


# ---- 9. contract
def _load_rc(sim, snap, rows=None):
    """gm_load_begin / gm_load_rows / gm_load_commit by hand; the first status that is not GM_OK."""
    n = sim.n
    rc = sim.lib.gm_load_begin(sim.h, int(snap["t"]))
    if rc:
        return rc
    for r0, m in (rows if rows is not None else [(0, n)]):
        hb, ts = np.ascontiguousarray(snap["hb"][r0:r0 + m]), np.ascontiguousarray(snap["ts"][r0:r0 + m])
        rc = sim.lib.gm_load_rows(sim.h, r0, m, _ptr(hb), _ptr(ts))
        if rc:
            return rc
    arrs = [np.ascontiguousarray(snap[k], dtype=np.int32) for k in ("heartbeat", "failed", "targets", "counts")]
    return sim.lib.gm_load_commit(sim.h, *[_ptr(a) for a in arrs])


def test_contract_unsupported_contexts():
    for sim in (Simulator(64, GM_MODE_PARTIAL, rd_seed=7, view_seed=5, init_mode=1, init_t0=8, init_seed=11),
                Simulator(10, GM_MODE_FAITHFUL),
                Simulator(64, GM_MODE_SCALED, rd_seed=7, init_mode=2)):
        assert sim.lib.gm_load_begin(sim.h, 9) == GM_EUNSUPPORTED
    sim = Simulator(64, GM_MODE_SCALED, **dict(KW300, init_mode=1))
    sim.msgcount_record(32)
    assert sim.lib.gm_load_begin(sim.h, 9) == GM_EUNSUPPORTED


def _edits(snap):
    """(name, status, edited copy) of a valid 64-node snapshot: every rejected state"""
    t = snap["t"]
    live = int(np.flatnonzero(snap["failed"] == 0)[0])
    other = (live + 1) % 64

    def ed(name, rc, fn):
        s = {k: np.array(v, copy=True) for k, v in snap.items()}
        fn(s)
        return name, rc, s

    def dead_sender(s):  # a crashed row whose last tick was 40 before t - 1, yet it has targets
        s["failed"][live] = 1
        s["ts"][live] -= 40
        s["hb"][live] -= 80
        s["counts"][live] = 2

    return [
        ed("ts > t - 1", GM_EINVAL, lambda s: s["ts"].__setitem__((live, other), t)),
        ed("hb negative, ts not", GM_EINVAL, lambda s: s["hb"].__setitem__((live, other), -1)),
        ed("ts negative, hb not", GM_EINVAL, lambda s: s["ts"].__setitem__((live, other), -1)),
        ed("counts = 6", GM_EINVAL, lambda s: s["counts"].__setitem__(live, 6)),
        ed("counts = -1", GM_EINVAL, lambda s: s["counts"].__setitem__(live, -1)),
        ed("target = n", GM_EINVAL, lambda s: (s["counts"].__setitem__(live, 1), s["targets"].__setitem__((live, 0), 64))),
        ed("target = -1", GM_EINVAL, lambda s: (s["counts"].__setitem__(live, 1), s["targets"].__setitem__((live, 0), -1))),
        ed("failed = 2", GM_EINVAL, lambda s: s["failed"].__setitem__(live, 2)),
        ed("own entry absent", GM_EINVAL,
           lambda s: (s["hb"].__setitem__((live, live), -1), s["ts"].__setitem__((live, live), -1))),
        ed("own entry not of t - 1", GM_EINVAL, lambda s: s["ts"].__setitem__((live, live), t - 2)),
        ed("own heartbeat not the bump's", GM_EINVAL, lambda s: s["heartbeat"].__setitem__(live, s["heartbeat"][live] + 2)),
        ed("a sender that did not run t - 1", GM_EINVAL, dead_sender),
    ]


def test_contract_states_and_arguments():
    n = 64
    kw = dict(KW300, init_mode=1, init_t0=100)  # t > 41: an edited row can be 40 ticks older
    src = Simulator(n, GM_MODE_SCALED, **kw)
    crash = crash_set(n, 3, 42)
    for _ in range(4):
        src.tick()
    src.set_failed(crash)
    src.tick()
    snap = state.snapshot(src)
    sim = Simulator(n, GM_MODE_SCALED, **dict(kw, init_mode=0))
    assert _load_rc(sim, snap) == 0 and sim.time == snap["t"]  # the unedited state loads
    # GM_ESTATE: no tick, crash or shard call while loading; rows missing; a row twice
    assert sim.lib.gm_load_begin(sim.h, snap["t"]) == 0
    assert sim.lib.gm_tick(sim.h) == GM_ESTATE
    assert sim.lib.gm_set_failed(sim.h, _ptr(crash), len(crash)) == GM_ESTATE
    assert _load_rc(sim, snap, rows=[(0, 32)]) == GM_ESTATE  # commit with rows [32, 64) missing
    assert _load_rc(sim, snap, rows=[(0, 40), (32, 32)]) == GM_ESTATE  # rows [32, 40) twice
    for name, want, bad in _edits(snap):
        assert _load_rc(sim, bad) == want, name
        assert sim.lib.gm_tick(sim.h) == GM_ESTATE, name  # a failed load leaves the context loading
    assert _load_rc(sim, snap) == 0
    sim.tick()
    src.tick()
    assert np.array_equal(sim.read_table()[0], src.read_table()[0]) and sim.tick_stats()["err"] == 0
    # the cold start's own entry {0, 0} at t = 1 is the one exception to the own-entry rule
    cold = Simulator(n, GM_MODE_SCALED, rd_seed=7, init_mode=0)
    csnap = state.snapshot(cold)
    assert csnap["t"] == 1 and _load_rc(sim, csnap) == 0


def test_contract_ranges():
    # a lag beyond the cell's 8-bit h field: GM_ERANGE (the GM_ERR_LAG case), not a wrapped heartbeat
    n = 96
    src = Simulator(n, GM_MODE_SCALED, rd_seed=7, init_mode=1, init_t0=200, init_seed=11)
    src.tick()
    snap = state.snapshot(src)
    sim = Simulator(n, GM_MODE_SCALED, rd_seed=7, init_mode=0)
    bad = {k: np.array(v, copy=True) for k, v in snap.items()}
    bad["hb"][3, 4] = 0  # 255 - (2 (t - 1) - 0) < 0
    assert _load_rc(sim, bad) == GM_ERANGE
    # 65 lists for node 0 overflow its inbox (S_KMAX = 64); 64 fit
    for senders, want in ((65, GM_ERANGE), (64, 0)):
        s = {k: np.array(v, copy=True) for k, v in snap.items()}
        s["counts"][:] = 0
        s["counts"][1:1 + senders] = 1
        s["targets"][1:1 + senders, 0] = 0
        assert _load_rc(sim, s) == want, senders
    assert sim.tick_stats()["lists"] == 0 and sim.time == snap["t"]
    sim.tick()
    assert sim.tick_stats()["max_inbox"] == 64 and sim.tick_stats()["err"] == 0


def test_clean_load_after_a_failed_one_continues_against_the_oracle():
    n = 64
    kw = dict(KW300, init_mode=1)
    ora = _oracle_at(n, 12, **kw)
    snap = _oracle_snapshot(ora)
    sim = Simulator(n, GM_MODE_SCALED, **dict(kw, init_mode=0))
    bad = {k: np.array(v, copy=True) for k, v in snap.items()}
    bad["ts"][5, 6] = snap["t"]
    assert _load_rc(sim, bad, rows=[(0, 32), (32, 32)]) == GM_EINVAL
    state.restore(sim, snap)
    assert same_state(sim, ora)
    _continue(sim, ora, 3)


# ---- 10. the timed branches of the block loop
def test_timed_load_equals_untimed_load(monkeypatch):
    """gm_set_timing changes what a load measures, not what it writes: the same state through launches of
    7 rows into a timed and an untimed context, then 3 ticks on both"""
    ora, kw = _state300(0)
    snap = _oracle_snapshot(ora)
    _check_state300(snap)
    monkeypatch.setenv("GM_LOAD_STAGE_ROWS", "7")
    timed, plain = (Simulator(300, GM_MODE_SCALED, band=64, **kw) for _ in range(2))
    timed.set_timing(True)
    for sim in (timed, plain):
        state.restore(sim, snap)
    st, sp = timed.load_stats(), plain.load_stats()
    assert st["rows"] == 300 and sp["rows"] == 300
    assert st["staging_bytes"] == sp["staging_bytes"]
    assert st["check_ms"] > 0 and st["encode_ms"] > 0
    assert sp["check_ms"] == 0 and sp["encode_ms"] == 0

    def same(what):
        for a, b in zip(timed.read_table(), plain.read_table()):
            assert np.array_equal(a, b), f"tables differ {what}"
        assert np.array_equal(timed.read_nodes(), plain.read_nodes()), f"node state differs {what}"
        for a, b in zip(timed.read_targets(), plain.read_targets()):
            assert np.array_equal(a, b), f"targets differ {what}"
        assert timed.dump_tables() == plain.dump_tables(), f"dumps differ {what}"

    same("after the load")
    assert plain.dump_tables() == ora.dump()
    for _ in range(3):
        timed.tick()
        plain.tick()
    assert timed.dump_tables() == plain.dump_tables(), "dumps differ after 3 ticks"
    assert timed.tick_stats()["err"] == 0 and plain.tick_stats()["err"] == 0
