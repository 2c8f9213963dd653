"""SCALED: the membership census reduced on the device (gm_census, Simulator.census).

Every comparison is exact: the census of a context against a plain NumPy aggregation (`expected`)
of read_table() + read_nodes() of the same context -- those two are the specification -- and, in
cases 1 and 2, against the same aggregation of the oracle's rows. Each case asserts from the
expected arrays that it contains what it is there for; the `_check_*` functions hold those
conditions, so they can be run against the oracle alone, without a GPU.

 1. crash window (bands of 512 and of 1024 with padding columns; N = 300 at band 64: four full bands, a partial one, three of padding). The crashed
    nodes' last heartbeat is 2 * 10 - 1, so their entries lag 12 ticks at tick 22 -- still stored bytes --
    and more than 14 from tick 25 on: tick 26 is the census over their escape lists
 2. cold start: every cell but the own entries escaped before a tick and after tick 1, two thirds of
    them after tick 3; lists in the pool
 3. the band fast path with three bands
 4. keyed loss: old and lagging entries of live subjects
 5. a loaded state, no tick: the clip bin, and a long-dead row that must not count
 6. column shards against the single context, merge_shards
 7. the join ramp
 8. no side effects: a censused twin stays equal to an uncensused one
 9. the contract
"""
import ctypes

import numpy as np
import pytest

import oracle_py
from membership import GM_EV_REMOVED, GM_MODE_FAITHFUL, GM_MODE_PARTIAL, GM_MODE_SCALED, Simulator, crash_set, state
from membership.abi import CENSUS_DTYPE, GM_CENSUS_AGES, GM_CENSUS_LAGS, GmCensusRec
from membership.census import merge_shards
from membership.sharded import loopback_tick

pytestmark = pytest.mark.gpu

GM_EINVAL, GM_ESTATE, GM_EUNSUPPORTED = -1, -5, -6
TFAIL = 5
KW = dict(rd_seed=7, init_t0=8, init_seed=11)
FIELDS = CENSUS_DTYPE.names


def expected(hb, ts, failed, t, c0=0):
    """The census of (hb, ts) [n][w] (-1 = absent; the columns [c0, c0 + w) of the cluster) at tick
    t, failed [n]: (rec, hist) as gm_census defines them."""
    hb, ts = np.asarray(hb, dtype=np.int64), np.asarray(ts, dtype=np.int64)
    failed = np.asarray(failed)
    w = hb.shape[1]
    pres = (hb >= 0) & (failed == 0)[:, None]
    lag, age = (2 * t - hb) >> 1, t - ts
    assert (lag[pres] >= 0).all() and (age[pres] >= 0).all() and (age[pres] < GM_CENSUS_AGES).all()
    rec = np.zeros(w, dtype=CENSUS_DTYPE)
    rec["holders"] = pres.sum(axis=0)
    rec["stale"] = (pres & (age >= TFAIL)).sum(axis=0)
    big = np.int64(1) << 40
    for name, a in (("hb", hb), ("ts", ts)):
        rec[name + "_min"] = np.where(rec["holders"] > 0, np.where(pres, a, big).min(axis=0), -1)
        rec[name + "_max"] = np.where(pres, a, -1).max(axis=0)
        rec[name + "_sum"] = np.where(pres, a, 0).sum(axis=0)
    cls = np.broadcast_to((failed[c0:c0 + w] != 0).astype(np.int64)[None, :], pres.shape)
    hist = np.zeros((2, GM_CENSUS_LAGS, GM_CENSUS_AGES), dtype=np.uint64)
    np.add.at(hist, (cls[pres], np.minimum(lag, GM_CENSUS_LAGS - 1)[pres], age[pres]), 1)
    return rec, hist


def _assert_census(got, want, what):
    (rec, hist), (erec, ehist) = got, want
    for f in FIELDS:
        bad = np.flatnonzero(rec[f] != erec[f])
        assert not len(bad), f"{what}: {f} differs in {len(bad)} columns, first {bad[0]}: {rec[f][bad[0]]} != {erec[f][bad[0]]}"
    assert np.array_equal(hist, ehist), f"{what}: histogram differs in {(hist != ehist).sum()} bins"
    assert int(rec["holders"].sum()) == int(hist.sum())


def _check(sim, ora=None):
    """census of sim == expected(its own read-backs) (== expected(the oracle's rows)); returns
    (hb, ts, failed, t, rec, hist) of the expected side"""
    t = sim.time - 1
    got = sim.census()
    hb, ts = sim.read_table()
    failed = sim.read_nodes()[:, 2]
    c0 = sim.shard_layout()[0]
    want = expected(hb, ts, failed, t, c0)
    _assert_census(got, want, f"tick {t} vs read_table")
    if ora is not None:
        assert ora.time - 1 == t
        ohb, ots = ora.table()
        _assert_census(got, expected(ohb, ots, ora.nodes()[:, 2], t), f"tick {t} vs the oracle")
    return hb, ts, failed, t, want[0], want[1]


# ---- what each case must contain, from the expected arrays
def _lag_age(hb, ts, failed, t):
    pres = (hb >= 0) & (failed == 0)[:, None]
    return pres, (2 * t - hb.astype(np.int64)) >> 1, t - ts.astype(np.int64)


def _check_escaped_crashed(hb, ts, failed, t):
    pres, lag, _ = _lag_age(hb, ts, failed, t)
    sel = pres & (failed != 0)[None, :]
    assert sel.any() and (lag[sel] > 14).any(), "no crashed subject's entry lags more than 14 ticks"


def _check_faded(failed, rec):
    assert (failed != 0).any() and not rec["holders"][failed != 0].any(), "a crashed subject still has holders"
    assert (rec["hb_min"][failed != 0] == -1).all() and (rec["ts_max"][failed != 0] == -1).all()


def _check_all_escaped(hb, ts, failed, t, band, every=True):
    """every present cell of a live row but its own entry (hb 2t - 1 once it ran a tick) is outside the
    stored byte (every = False: most are; from tick 2 on the first even heartbeats arrive); returns the
    shortest escape list of a (band, row)"""
    pres, lag, age = _lag_age(hb, ts, failed, t)
    h = 255 - (2 * t - hb.astype(np.int64))
    esc = pres & ~((h >= 230) & (h % 2 == 0) & (age <= 14))
    fits = int((pres & ~esc & ~np.eye(len(hb), dtype=bool)).sum())
    assert esc.sum() > pres.sum() // 2 and (fits == 0 or not every), "a cell fits the stored byte"
    return min(int(esc[failed == 0][:, c:c + band].sum(axis=1).min()) for c in range(0, hb.shape[1], band))


def _check_old_live(hb, ts, failed, t):
    pres, lag, age = _lag_age(hb, ts, failed, t)
    sel = pres & (failed == 0)[None, :]
    return int((sel & (age >= 15)).sum()), int((sel & (lag > 14)).sum())


# ---- 1. crash window
def _crash_run(n, band, until, ora=True, **kw):
    """ticks a warm context (and the oracle) through the crash of 1 % after tick 10; yields after every tick"""
    k = dict(KW, init_mode=1, **kw)
    ncrash = max(1, (n + 99) // 100)
    o = oracle_py.Oracle(n, oracle_py.OC_SCALED, crash_tick=10, crash_count=ncrash, crash_seed=42, **k) if ora else None
    sim = Simulator(n, GM_MODE_SCALED, band=band, **k)
    crash = crash_set(n, ncrash, 42)
    while sim.time <= until:
        t = sim.time
        sim.tick()
        if o is not None:
            o.tick()
        if t == 10:
            sim.set_failed(crash)
        yield t, sim, o


# Rows are padded to 512 columns, so N = 1100 (1536 columns) cannot have 1024-column bands: it runs at
# its widest band, 512 (nb = 3, 436 padding columns), and band 1024 with two bands at N = 1540 (508
# padding columns; no oracle beside it: its 37 ticks there take half a minute of CPU).
@pytest.mark.parametrize("n,band,with_oracle", [(1100, 512, True), (1540, 1024, False), (300, 64, True)])
def test_crash_window(n, band, with_oracle):
    seen = set()
    for t, sim, ora in _crash_run(n, band, 45, ora=with_oracle):
        removed = any(e[2] == GM_EV_REMOVED for e in sim.drain_events())
        if not (t in (9, 22, 26, 45) or (removed and "tremove" not in seen)):
            continue
        hb, ts, failed, tt, rec, hist = _check(sim, ora)
        assert tt == t
        if t == 9:
            assert not failed.any() and (rec["holders"] == n).all() and not hist[1].any()
        if t == 22:  # 12 ticks after the crash: the crashed subjects' entries lag 12, the last lag a byte holds
            assert hist[1].sum() == rec["holders"][failed != 0].sum() > 0 and hist[1, 12].sum() > 0
        if t == 26:  # a heartbeat frozen at 2 * 10 - 1 lags (2 * 26 - 19) >> 1 = 16 ticks: escaped cells
            _check_escaped_crashed(hb, ts, failed, t)
            assert hist[1, 15:].sum() > 0 and not hist[1, :15].any()
        if removed:
            seen.add("tremove")
            assert 0 < rec["holders"][failed != 0].sum() < (failed != 0).sum() * (failed == 0).sum()
        if t == 45:
            _check_faded(failed, rec)
        seen |= {t} & {9, 22, 26, 45}
    assert seen == {9, 22, 26, 45, "tremove"}
    assert sim.tick_stats()["err"] == 0


# ---- 2. cold start
@pytest.mark.parametrize("n,band", [(96, 64), (1100, 512), (1540, 1024)])
def test_cold_start(n, band):
    k = dict(rd_seed=7, init_mode=0)
    ora = oracle_py.Oracle(n, oracle_py.OC_SCALED, **k)
    sim = Simulator(n, GM_MODE_SCALED, band=band, **k)
    while ora.time < sim.time:
        ora.tick()
    shortest = []
    for ticks in (0, 1, 2):
        for _ in range(ticks):
            sim.tick()
            ora.tick()
        hb, ts, failed, t, rec, hist = _check(sim, ora)
        shortest.append(_check_all_escaped(hb, ts, failed, t, band, every=t <= 1))
        assert (rec["holders"] == n).all()
    assert sim.time - 1 == 3
    if n >= 1100:
        assert min(shortest) > 16, "a list fits the inline slot: no pool entry was read"


# ---- 3. the fast path, three bands
def test_fast_path_three_bands():
    n = 2564  # 3072 padded columns
    sim = Simulator(n, GM_MODE_SCALED, band=1024, **dict(KW, init_mode=1))
    for k in range(15):
        sim.tick()
        if k in (0, 14):
            hb, ts, failed, t, rec, hist = _check(sim)
    assert (rec["holders"] == n).all() and hist[0].sum() == n * n
    for c in (0, 1024, 2048):  # every band holds cells, and more than one lag / age
        assert rec["holders"][c:c + 1024].sum() > 0
    assert (hist[0].sum(axis=1) > 0).sum() > 2 and (hist[0].sum(axis=0) > 0).sum() > 2
    assert sim.tick_stats()["err"] == 0


# ---- 4. keyed loss
KW_LOSS = dict(rd_seed=7, init_mode=1, init_t0=8, init_seed=11, drop_pct=80, drop_from=10, drop_to=40, drop_seed=42)


def test_keyed_loss():
    n = 600
    sim = Simulator(n, GM_MODE_SCALED, **KW_LOSS)
    old = lagging = 0
    while sim.time <= 45:
        t = sim.time
        sim.tick()
        if t in (25, 39, 45):
            hb, ts, failed, tt, rec, hist = _check(sim)
            a, b = _check_old_live(hb, ts, failed, t)
            old, lagging = old + a, lagging + b
    assert old > 0, "no entry of age >= 15 of a live subject"
    assert lagging > 0, "no entry of a live subject lagging more than 14 ticks"


# ---- 5. a loaded state, no tick
def _edited_snapshot():
    """an oracle state at t = 100 (N = 96, 3 crashed after tick 92) edited: live row `row` holds 20
    entries lagging 70 ticks; live row `dead` becomes a row that crashed 40 ticks ago"""
    n = 96
    k = dict(KW, init_mode=1, init_t0=90)
    ora = oracle_py.Oracle(n, oracle_py.OC_SCALED, crash_tick=92, crash_count=3, crash_seed=42, **k)
    while ora.time < 100:
        ora.tick()
    hb, ts = ora.table()
    st = ora.nodes()
    tg, cnt = ora.targets()
    snap = {"t": ora.time, "hb": hb, "ts": ts, "heartbeat": st[:, 3].copy(), "failed": st[:, 2].copy(),
            "targets": tg, "counts": cnt}
    live = np.flatnonzero(snap["failed"] == 0)
    row, dead = int(live[0]), int(live[1])
    cols = [c for c in live[2:22] if hb[row, c] >= 0]
    snap["hb"][row, cols] = 2 * (snap["t"] - 1) - 141  # lag (2T - hb) >> 1 = 70
    snap["failed"][dead] = 1
    snap["ts"][dead] = np.where(ts[dead] >= 0, ts[dead] - 40, -1)
    snap["hb"][dead] = np.where(hb[dead] >= 0, hb[dead] - 80, -1)
    snap["counts"][dead] = 0
    return snap, row, dead, cols


def test_loaded_state_without_a_tick():
    snap, row, dead, cols = _edited_snapshot()
    n, t = 96, snap["t"] - 1
    sim = Simulator(n, GM_MODE_SCALED, band=64, rd_seed=7, init_mode=0)
    state.restore(sim, snap)
    hb, ts, failed, tt, rec, hist = _check(sim)
    assert tt == t and np.array_equal(hb, snap["hb"]) and np.array_equal(ts, snap["ts"])
    _assert_census(sim.census(), expected(snap["hb"], snap["ts"], snap["failed"], t), "vs the edited snapshot")
    assert len(cols) >= 10 and hist[:, GM_CENSUS_LAGS - 1].sum() == len(cols), "the clip bin"
    assert (snap["ts"][dead].max() < t - 31) and failed[dead] == 1  # only fits relative to its own last tick
    assert rec["holders"].max() <= (failed == 0).sum()
    assert (rec["ts_min"][rec["holders"] > 0] > snap["ts"][dead].max()).all(), "the long-dead row was counted"


# ---- 6. column shards
def test_column_shards():
    n, world = 600, 3
    k = dict(rd_seed=7, init_mode=1, init_t0=6, init_seed=5)
    ref = Simulator(n, GM_MODE_SCALED, **k)
    shards = [Simulator(n, GM_MODE_SCALED, shard_rank=g, shard_count=world, **k) for g in range(world)]
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
            hb, ts, failed, tt, rec, hist = _check(ref)
            parts = []
            for s in shards:
                c0, w = s.shard_layout()
                _check(s)
                srec, shist = s.census()
                for f in FIELDS:
                    assert np.array_equal(srec[f], rec[f][c0:c0 + w]), f"shard at {c0}: {f} differs at tick {t}"
                parts.append((c0, srec, shist))
            _assert_census(merge_shards(parts[::-1]), (rec, hist), f"merged shards at tick {t}")
            checked += 1
            if t == 24:
                _check_escaped_crashed(hb, ts, failed, t)
    assert checked == 3


# ---- 7. join ramp
def test_join_ramp():
    n = 64
    sim = Simulator(n, GM_MODE_SCALED, rd_seed=7, init_mode=2, band=64)
    for t in (6, 40):
        while sim.time - 1 < t:
            sim.tick()
        hb, ts, failed, tt, rec, hist = _check(sim)
        st = sim.read_nodes()
        assert tt == t
        if t == 6:  # nodes 28.. have not started: they hold nothing and nobody holds them
            assert not st[28:, 0].any() and not (hb[28:] >= 0).any() and not rec["holders"][28:].any()
            assert rec["holders"][0] > 1
        else:
            assert st[:, 1].all() and (rec["holders"] == n).all()
    assert sim.tick_stats()["err"] == 0


# ---- 8. no side effects
def test_no_side_effects():
    n = 300
    runs = [_crash_run(n, 64, 34, ora=False), _crash_run(n, 64, 34, ora=False)]
    events = [[], []]
    for (t, a, _), (_, b, _) in zip(*runs):
        rec, hist = a.census()
        assert int(rec["holders"].sum()) == int(hist.sum())
        events[0] += a.drain_events()
        events[1] += b.drain_events()
    assert events[0] == events[1] and any(e[2] == GM_EV_REMOVED for e in events[0])
    (ha, ta), (hb, tb) = a.read_table(), b.read_table()
    assert np.array_equal(ha, hb) and np.array_equal(ta, tb)
    assert np.array_equal(a.read_nodes(), b.read_nodes())
    (ga, ca), (gb, cb) = a.read_targets(), b.read_targets()
    assert np.array_equal(ga, gb) and np.array_equal(ca, cb)
    assert a.tick_stats() == b.tick_stats() and a.tick_stats()["err"] == 0


# ---- 9. contract
def _rc(sim, rec=None, hist=None):
    return sim.lib.gm_census(sim.h, None if rec is None else rec.ctypes.data_as(ctypes.POINTER(GmCensusRec)),
                             None if hist is None else hist.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)))


def test_contract():
    for other in (Simulator(10, GM_MODE_FAITHFUL),
                  Simulator(64, GM_MODE_PARTIAL, rd_seed=7, view_seed=5, init_mode=1, init_t0=8, init_seed=11)):
        assert _rc(other, np.zeros(64, dtype=CENSUS_DTYPE)) == GM_EUNSUPPORTED
    n = 300
    sim = Simulator(n, GM_MODE_SCALED, band=64, **dict(KW, init_mode=1))
    for _ in range(3):
        sim.tick()
    assert _rc(sim) == GM_EINVAL
    full = sim.census()
    rec_only, none = sim.census(hist=False)
    none2, hist_only = sim.census(records=False)
    assert none is None and none2 is None
    assert np.array_equal(rec_only, full[0]) and np.array_equal(hist_only, full[1])
    again = sim.census()
    assert np.array_equal(again[0], full[0]) and np.array_equal(again[1], full[1])
    _check(sim)
    # inside a load: GM_ESTATE until the commit
    snap = state.snapshot(sim)
    assert sim.lib.gm_load_begin(sim.h, snap["t"]) == 0
    assert _rc(sim, np.zeros(n, dtype=CENSUS_DTYPE)) == GM_ESTATE
    state.restore(sim, snap)
    after = sim.census()
    assert np.array_equal(after[0], full[0]) and np.array_equal(after[1], full[1])
