"""Detection recorder (gm_detect_record / gm_detect / gm_detect_timeline): per-subject removal and
join statistics and the per-tick timeline, reduced on the device from each tick's records (SCALED,
gm_s_detect) or where the records are collected (FAITHFUL).

The expected value is always a plain NumPy aggregation of event tuples (t, logger, kind, subject),
the false-removal rule applied from the test's own set_failed calls. The tuples come from the CPU
oracle where it is quick, else from a twin context that drains every tick (drained events are
pinned to the oracle by test_gpu_scaled.py). Every comparison is exact: integer counts. Each case
asserts from its expected events that it exercises what it is there for."""
import functools

import numpy as np
import pytest

import oracle_py
from membership import (GM_EV_JOINED, GM_EV_REMOVED, GM_MODE_FAITHFUL, GM_MODE_PARTIAL, GM_MODE_SCALED, GmError,
                        Simulator, crash_set)
from membership.abi import DETECT_DTYPE
from membership.sharded import loopback_tick

pytestmark = pytest.mark.gpu

GM_EINVAL, GM_ESTATE, GM_EUNSUPPORTED = -1, -5, -6


def aggregate(events, n, fails, tmax, t_from=0, c0=0, w=None):
    """(records [w], timeline [tmax][3]) of the events with t_from <= t < tmax naming subjects
    [c0, c0 + w). fails: {node index: the tick after which set_failed named it}."""
    w = n - c0 if w is None else w
    ev = np.asarray(events, dtype=np.int64).reshape(-1, 4)
    fail_at = np.full(n, np.iinfo(np.int64).max)
    for s, ft in fails.items():
        fail_at[s] = ft
    rec = np.zeros(w, dtype=DETECT_DTYPE)
    rec["fail_tick"] = [-1 if fail_at[c0 + i] > 1 << 40 else fail_at[c0 + i] for i in range(w)]
    first = np.full(w, np.iinfo(np.int64).max)
    last = np.full(w, -1, dtype=np.int64)
    tl = np.zeros((tmax, 3), dtype=np.uint64)
    t, kind, sub = ev[:, 0], ev[:, 2], ev[:, 3] - 1
    own = (t >= t_from) & (t < tmax) & (sub >= c0) & (sub < c0 + w)
    j = own & (kind == GM_EV_JOINED)
    r = own & (kind == GM_EV_REMOVED)
    f = r & ~(fail_at[np.clip(sub, 0, n - 1)] < t)  # the subject had not been failed before tick t ran
    np.add.at(rec["joins"], sub[j] - c0, 1)
    np.add.at(rec["removals"], sub[r] - c0, 1)
    np.add.at(rec["false_removals"], sub[f] - c0, 1)
    np.add.at(rec["removed_tick_sum"], sub[r] - c0, t[r].astype(np.uint64))
    np.minimum.at(first, sub[r] - c0, t[r])
    np.maximum.at(last, sub[r] - c0, t[r])
    rec["first_removed"] = np.where(last >= 0, first, -1)
    rec["last_removed"] = last
    for k, m in enumerate((j, r, f)):
        np.add.at(tl[:, k], t[m], 1)
    return rec, tl


def assert_records(got, want, what=""):
    for name in DETECT_DTYPE.names:
        bad = np.flatnonzero(got[name] != want[name])
        assert bad.size == 0, f"{what} {name} differs at subjects {bad[:8]}: {got[name][bad[:8]]} != {want[name][bad[:8]]}"
    assert got.dtype == DETECT_DTYPE and got.shape == want.shape


def assert_timeline(got, want, what=""):
    bad = np.flatnonzero((got != want).any(axis=1))
    assert got.shape == want.shape and bad.size == 0, f"{what} timeline differs at ticks {bad[:8]}"


def max_per_cell(events, band):
    """most records of one (tick, logger, band of `band` columns); band 0: of one (tick, logger)"""
    ev = np.asarray(events, dtype=np.int64).reshape(-1, 4)
    cell = (ev[:, 3] - 1) // band if band else np.zeros(len(ev), dtype=np.int64)
    _, cnt = np.unique(np.stack([ev[:, 0], ev[:, 1], cell], axis=1), axis=0, return_counts=True)
    return int(cnt.max()) if len(cnt) else 0


def oracle_events(n, ticks, crash_tick=-1, ncrash=0, pre_tick=False, **kw):
    """every event of `ticks` oracle ticks (crash set crash_set(n, ncrash, 42) after crash_tick)"""
    ora = oracle_py.Oracle(n, oracle_py.OC_SCALED, rd_seed=7, crash_tick=crash_tick, crash_count=ncrash, crash_seed=42,
                           **kw)
    if pre_tick:
        ora.tick()  # the ramp's tick 0: the GPU context starts as of tick 0
    out = []
    for _ in range(ticks):
        ora.tick()
        out += ora.events()
    return out


def run(sim, ticks, crash_tick=-1, crash=(), twin=None, record_after=None, tmax=None):
    """tick sim (and twin); set_failed after crash_tick; start recording at once (record_after None)
    or after that tick. Returns the twin's drained events."""
    if record_after is None:
        sim.detect_record(tmax)
    out = []
    for _ in range(ticks):
        t = sim.time
        sim.tick()
        if twin is not None:
            twin.tick()
        if t == crash_tick:
            sim.set_failed(crash)
            if twin is not None:
                twin.set_failed(crash)
        if t == record_after:
            sim.detect_record(tmax)
        if twin is not None:
            out.append(twin.drain_events_np())
    return np.concatenate(out) if out else None


# ---- case 1: N = 300, the narrowest band (2 slots per (row, band)), cold start, 30 crashed after tick 8
C1 = dict(n=300, ticks=40, crash_tick=8, ncrash=30)


@functools.lru_cache(maxsize=None)
def case1_events():
    return tuple(oracle_events(C1["n"], C1["ticks"], C1["crash_tick"], C1["ncrash"]))


def case1_sim():
    return Simulator(C1["n"], GM_MODE_SCALED, rd_seed=7, band=64)


def test_spill_at_the_narrowest_band():
    n, ticks = C1["n"], C1["ticks"]
    ev = case1_events()
    assert max_per_cell(ev, 64) > 2  # records spill past the 2 slots of a (row, 64-column band)
    crash = crash_set(n, C1["ncrash"], 42)
    sim = case1_sim()
    tmax = sim.time + ticks
    run(sim, ticks, C1["crash_tick"], crash, tmax=tmax)
    want, wtl = aggregate(ev, n, {int(s): C1["crash_tick"] for s in crash}, tmax)
    got = sim.detect()
    assert_records(got, want)
    assert_timeline(sim.detect_timeline(tmax), wtl)
    assert int(got["removals"].sum()) == 8100 == 270 * 30 and not got["false_removals"].any()
    hit = got[crash]
    assert (hit["removals"] == 270).all() and hit["first_removed"].min() >= 29 and hit["last_removed"].max() <= 34
    assert sim.tick_stats()["err"] == 0


# ---- case 2: N = 1024 on the fast-path band (32 slots), no draining on the recording context
def test_spill_on_the_fast_path_band_without_draining():
    n, ticks, crash_tick = 1024, 34, 4
    crash = crash_set(n, 200, 42)
    sim = Simulator(n, GM_MODE_SCALED, rd_seed=7)
    twin = Simulator(n, GM_MODE_SCALED, rd_seed=7)
    sim.keep_events(0)
    tmax = sim.time + ticks
    ev = run(sim, ticks, crash_tick, crash, twin=twin, tmax=tmax)
    assert max_per_cell(ev, 0) > 32  # some logger's tick holds more than its 32 slots
    want, wtl = aggregate(ev, n, {int(s): crash_tick for s in crash}, tmax)
    got = sim.detect()
    assert_records(got, want)
    assert_timeline(sim.detect_timeline(tmax), wtl)
    assert int(got["removals"].sum()) == 164800 == 824 * 200
    assert sim.tick_stats()["err"] == 0


# ---- case 3: heavy keyed loss, nobody crashes: every removal is false, and the removed re-join
def test_false_removals_and_rejoins():
    n, ticks = 96, 60
    kw = dict(drop_pct=85, drop_from=2, drop_to=60, drop_seed=42)
    ev = oracle_events(n, ticks, **kw)
    kinds = np.asarray(ev)[:, 2]
    assert (kinds == GM_EV_REMOVED).any() and (kinds == GM_EV_JOINED).any()
    sim = Simulator(n, GM_MODE_SCALED, rd_seed=7, **kw)
    tmax = sim.time + ticks
    run(sim, ticks, tmax=tmax)
    want, wtl = aggregate(ev, n, {}, tmax)
    got = sim.detect()
    assert_records(got, want)
    assert_timeline(sim.detect_timeline(tmax), wtl)
    assert got["removals"].sum() > 0 and got["joins"].sum() > 0
    assert (got["false_removals"] == got["removals"]).all() and (got["fail_tick"] == -1).all()


# ---- case 4: the join ramp: joins only, more per (row, band) than its slots
@functools.lru_cache(maxsize=None)
def ramp_events():
    return tuple(oracle_events(160, 60, pre_tick=True, init_mode=2, init_t0=0, init_seed=43))


@pytest.mark.parametrize("band", [64, 0])
def test_joins_on_the_ramp(band):
    n, ticks = 160, 60
    ev = ramp_events()
    assert max_per_cell(ev, 64) > 2  # joins spill at the 64-column band
    sim = Simulator(n, GM_MODE_SCALED, rd_seed=7, init_mode=2, init_t0=0, init_seed=43, band=band)
    tmax = sim.time + ticks
    run(sim, ticks, tmax=tmax)
    want, wtl = aggregate(ev, n, {}, tmax)
    got = sim.detect()
    assert_records(got, want)
    assert_timeline(sim.detect_timeline(tmax), wtl)
    assert int(got["joins"].sum()) == 25599 and not got["removals"].any()
    assert sim.tick_stats()["err"] == 0


# ---- case 5: warm start with keyed loss at every band width (test_scaled_every_band_width_matches_oracle's run)
C5 = dict(drop_pct=15, drop_from=4, drop_to=22, drop_seed=42, init_mode=1, init_t0=7, init_seed=43)


@functools.lru_cache(maxsize=None)
def case5_events():
    return tuple(oracle_events(700, 36, 9, 9, **C5))


@pytest.mark.parametrize("band", [64, 128, 256, 512, 1024])
def test_every_band_width(band):
    n, ticks, crash_tick = 700, 36, 9
    ev = case5_events()
    crash = crash_set(n, 9, 42)
    sim = Simulator(n, GM_MODE_SCALED, rd_seed=7, band=band, **C5)
    tmax = sim.time + ticks
    run(sim, ticks, crash_tick, crash, tmax=tmax)
    want, wtl = aggregate(ev, n, {int(s): crash_tick for s in crash}, tmax)
    got = sim.detect()
    assert_records(got, want)
    assert_timeline(sim.detect_timeline(tmax), wtl)
    assert int(got["removals"].sum()) == 6219
    assert sim.tick_stats()["err"] == 0


# ---- case 6: column shards report their own columns; together they equal the single context
def _shard_kw(drop):
    return dict(rd_seed=7, drop_pct=drop, drop_from=3, drop_to=25, drop_seed=42, init_mode=1, init_t0=6, init_seed=5)


def _shards_equal_single(ref, shards, tmax):
    want = ref.detect()
    assert want["removals"].sum() > 0  # the crashed nodes were swept inside the run
    cols = [s.shard_layout() for s in shards]
    assert [c for c, _ in cols] == sorted(c for c, _ in cols) and sum(w for _, w in cols) == ref.n
    got = [s.detect() for s in shards]
    assert [len(g) for g in got] == [w for _, w in cols]
    assert_records(np.concatenate(got), want, "shards")
    tl = sum(s.detect_timeline(tmax) for s in shards)
    assert_timeline(tl, ref.detect_timeline(tmax), "shards")
    for s in shards:
        assert s.tick_stats()["err"] == 0


@pytest.mark.parametrize("n,world,drop,how", [(600, 3, 0, "phase"), (21, 3, 30, "phase"), (2048, 8, 10, "pipelined")])
def test_column_shards_match_single_context(n, world, drop, how, monkeypatch):
    from membership.abi import shard_loopback_tick
    kw = _shard_kw(drop)
    ref = Simulator(n, GM_MODE_SCALED, **kw)
    if how == "pipelined":
        monkeypatch.setenv("GM_SCHUNKS", "4")
    shards = [Simulator(n, GM_MODE_SCALED, shard_rank=g, shard_count=world, **kw) for g in range(world)]
    monkeypatch.delenv("GM_SCHUNKS", raising=False)
    crash = crash_set(n, max(2, n // 64), 42)
    ticks = 36
    tmax = ref.time + ticks
    for s in [ref] + shards:
        s.keep_events(0)
        s.detect_record(tmax)
    for _ in range(ticks):
        t = ref.time
        ref.tick()
        if how == "pipelined":
            shard_loopback_tick(shards)
        else:
            loopback_tick(shards)
        if t == 8:
            for s in [ref] + shards:
                s.set_failed(crash)
    _shards_equal_single(ref, shards, tmax)


def test_rccl_single_rank_matches_single_context(monkeypatch):
    from membership.abi import comm_unique_id
    n, ticks = 600, 32
    kw = _shard_kw(0)
    ref = Simulator(n, GM_MODE_SCALED, **kw)
    monkeypatch.setenv("GM_FORCE_SHARD", "1")
    sh = Simulator(n, GM_MODE_SCALED, shard_rank=0, shard_count=1, **kw)
    monkeypatch.delenv("GM_FORCE_SHARD")
    sh.comm_init(comm_unique_id(), 1, 0)
    crash = crash_set(n, max(2, n // 64), 42)
    tmax = ref.time + ticks
    for s in (ref, sh):
        s.keep_events(0)
        s.detect_record(tmax)
    for _ in range(ticks):
        t = ref.time
        ref.tick()
        sh.tick()
        if t == 8:
            ref.set_failed(crash)
            sh.set_failed(crash)
    _shards_equal_single(ref, [sh], tmax)
    assert sh.dump_tables() == ref.dump_tables()


# ---- case 7: FAITHFUL aggregates on the host, where it collects the tick's records
def test_faithful_matches_its_own_events():
    n = 10
    sim = Simulator(n, GM_MODE_FAITHFUL, time_seed=3, rd_seed=7)
    tmax = 160
    sim.detect_record(tmax)
    for _ in range(100):
        sim.tick()
    fail_tick = sim.time - 1
    sim.set_failed([3])
    for _ in range(60):
        sim.tick()
    ev = [e for e in sim.drain_events() if e[2] in (GM_EV_JOINED, GM_EV_REMOVED)]
    want, wtl = aggregate(ev, n, {3: fail_tick}, tmax)
    got = sim.detect()
    assert_records(got, want)
    assert_timeline(sim.detect_timeline(tmax), wtl)
    assert got["joins"].sum() > 0
    assert got[3]["removals"] == 9 and got[3]["false_removals"] == 0 and got[3]["fail_tick"] == 99


# ---- case 8: the contract
def _code(fn, *a):
    with pytest.raises(GmError) as e:
        fn(*a)
    return e.value.code


def test_contract_errors():
    sim = Simulator(64, GM_MODE_SCALED, rd_seed=7)
    assert _code(sim.detect) == GM_ESTATE  # nothing recorded yet
    assert _code(sim.detect_timeline, 4) == GM_ESTATE
    assert _code(sim.detect_record, 0) == GM_EINVAL
    assert _code(sim.detect_record, 32768) == GM_EINVAL
    sim.tick()
    sim.detect_record(20)  # between any two ticks
    assert _code(sim.detect_record, 20) == GM_ESTATE
    assert _code(sim.detect_timeline, 21) == GM_EINVAL
    assert sim.detect().shape == (64,) and sim.detect_timeline(20).shape == (20, 3)
    sim.close()
    part = Simulator(64, GM_MODE_PARTIAL, rd_seed=7, view=8, view_seed=5, init_mode=1, init_t0=8, init_seed=11)
    assert _code(part.detect_record, 20) == GM_EUNSUPPORTED
    part.close()


def test_recording_starts_mid_run_and_stops_at_tmax():
    """Case 1's run, recorded from after tick 20 and for ticks < 32: the sweep (ticks 29-34) is cut
    by tmax, the ticks before recording stay 0, and the ticks >= tmax leave everything untouched."""
    n, ticks, tmax = C1["n"], C1["ticks"], 32
    ev = case1_events()
    ts = np.asarray(ev)[:, 0]
    assert (ts < tmax).any() and (ts >= tmax).any() and ((ts >= 21) & (ts < tmax)).any()
    crash = crash_set(n, C1["ncrash"], 42)
    sim = case1_sim()
    run(sim, ticks, C1["crash_tick"], crash, record_after=20, tmax=tmax)
    want, wtl = aggregate(ev, n, {int(s): C1["crash_tick"] for s in crash}, tmax, t_from=21)
    got = sim.detect()
    assert_records(got, want)
    tl = sim.detect_timeline(tmax)
    assert_timeline(tl, wtl)
    assert not tl[:21].any() and tl[21:].any()
    assert 0 < int(got["removals"].sum()) < 8100


def test_recorder_only_observes():
    """A recording context's drained events and tables equal a non-recording twin's."""
    n, ticks = C1["n"], C1["ticks"]
    crash = crash_set(n, C1["ncrash"], 42)
    sim, twin = case1_sim(), case1_sim()
    sim.detect_record(sim.time + ticks)
    for _ in range(ticks):
        t = sim.time
        sim.tick()
        twin.tick()
        if t == C1["crash_tick"]:
            sim.set_failed(crash)
            twin.set_failed(crash)
        assert sim.drain_events() == twin.drain_events(), f"events differ at tick {t}"
    assert sim.dump_tables() == twin.dump_tables()
    assert np.array_equal(sim.read_nodes(), twin.read_nodes())
    assert sim.event_totals() == twin.event_totals() and sim.event_totals()["removed"] == 8100
    assert int(sim.detect()["removals"].sum()) == 8100
