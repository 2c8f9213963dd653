"""SCALED: table rows decoded on the device (gm_read_rows, Simulator.read_rows, membership.state's
device route), against the specification it mirrors: gm_read_table of the same context, and the
oracle's table where the state comes from the oracle.

Every comparison is np.array_equal. Each case reads all rows at once and in pieces (the first row,
rows [7, 40), the last row, count = 0); each reused state asserts, through test_gpu_load_state.py's
`_check_*` conditions, that it exercises what it claims (they hold for these states on the oracle
alone). The shapes are the smallest at which each path of gm_r_decode can go wrong:

 1. warm N = 300, band 64 / auto, 9 crashes at tick 10: before and inside the crash window (the
    crashed columns' stale entries in escape lists), the TREMOVE ticks, after them
 2. cold start N = 300, band 64: every cell escaped, every list past its inline slot into the pool
 3. rows crashed 50 ticks ago (N = 96): they decode relative to their own wtick
 4. the payload / lag escapes of the N = 600 state under 80 % loss
 5. band 1024 with a full first and a padded last band (N = 1540, fast path on), and N = 1100, whose
    padded row (1536 columns) takes band 512: three bands, 76 real columns in the last
 6. column shards N = 600, G = 3: each shard's own columns, and their concatenation
 7. the join ramp (s_hbase != 0), N = 120
 8. the block loop: GM_READ_STAGE_ROWS = 7, the staging buffer reused by a second call
 9. a context that calls read_rows between its ticks equals one that never does
10. the contract: GM_EUNSUPPORTED / GM_EINVAL / GM_ESTATE
11. membership.state: snapshot(device=True), save_dir -> load_dir -> restore into another band width
12. widths that are no multiple of 4 (N = 301; N = 21 on three shards of 7 columns): the cell-by-cell
    stores of a row whose pieces are not 16-byte aligned
"""
import functools

import numpy as np
import pytest

import oracle_py
from membership import (GM_EV_REMOVED, GM_MODE_FAITHFUL, GM_MODE_PARTIAL, GM_MODE_SCALED, GmError, Simulator, crash_set,
                        state)
from membership.abi import _ptr
from membership.sharded import loopback_tick
from test_gpu_detect import _shard_kw
from test_gpu_load_state import (KW300, KW600, _check_all_escaped, _check_long_dead, _check_payload_escapes,
                                 _check_state300, _continue, _oracle_at, _oracle_snapshot)
from test_gpu_multiband import _same_targets

pytestmark = pytest.mark.gpu

GM_EINVAL, GM_ESTATE, GM_EUNSUPPORTED = -1, -5, -6


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def _check_reads(sim, want=None, what=""):
    """read_rows == read_table of the same context (== want, the oracle's table), whole and in pieces"""
    n = sim.n
    ref = sim.read_table()
    got = sim.read_rows()
    assert got[0].dtype == np.int32 and got[0].shape == ref[0].shape == got[1].shape
    assert _same(got, ref), f"read_rows differs from read_table {what}"
    if want is not None:
        assert _same(got, want), f"read_rows differs from the oracle's table {what}"
    for r0, cnt in ((0, 1), (7, 33), (n - 1, 1), (5, 0), (n, 0)):
        piece = sim.read_rows(r0, cnt)
        assert piece[0].shape == (cnt, ref[0].shape[1])
        assert _same(piece, (ref[0][r0:r0 + cnt], ref[1][r0:r0 + cnt])), f"rows [{r0}, {r0 + cnt}) differ {what}"
    assert sim.tick_stats()["err"] == 0
    return got


def _tick_with_crash(sims, crash, crash_tick=10):
    t = sims[0].time
    for s in sims:
        s.tick()
        if t == crash_tick:
            s.set_failed(crash)
    return t


# ---- 1. warm, the crash window, TREMOVE
TICKS300 = (9, 12, 25, 31, 32, 33, 40)


@functools.lru_cache(maxsize=None)
def _ora300():
    """the oracle's state before each tick of TICKS300 (one run, shared by the band widths)"""
    ora = oracle_py.Oracle(300, oracle_py.OC_SCALED, crash_tick=10, crash_count=9, crash_seed=42,
                           **dict(KW300, init_mode=1))
    snaps = {}
    while ora.time <= TICKS300[-1]:
        if ora.time in TICKS300:
            snaps[ora.time] = _oracle_snapshot(ora)
        ora.tick()
    return snaps


@pytest.mark.parametrize("band", [64, 0])
def test_warm_crash_window_and_tremove(band):
    snaps = _ora300()
    _check_state300(snaps[25])
    sim = Simulator(300, GM_MODE_SCALED, band=band, **dict(KW300, init_mode=1))
    crash = crash_set(300, 9, 42)
    removed = {}
    while sim.time <= TICKS300[-1]:
        if sim.time in TICKS300:
            t = sim.time
            hb, ts = _check_reads(sim, (snaps[t]["hb"], snaps[t]["ts"]), f"before tick {t}")
            removed[t] = sim.event_totals()["removed"]
            if t == 25:  # what read_rows returned holds the stale, escaped entries of the crashed columns
                _check_state300(dict(snaps[t], hb=hb, ts=ts))
        _tick_with_crash([sim], crash)
    assert removed[25] == 0 and removed[40] > removed[31] >= 0 and removed[40] > 0, "TREMOVE is not inside the run"


# ---- 2. cold start: every cell escaped, the lists in the pool
def test_cold_start_every_cell_escaped():
    kw = dict(rd_seed=7, init_seed=11, init_mode=0, init_t0=0)
    sim = Simulator(300, GM_MODE_SCALED, band=64, **kw)
    ora = oracle_py.Oracle(300, oracle_py.OC_SCALED, **kw)
    for after in (1, 3):
        while sim.time <= after:
            ora.tick()
            sim.tick()
        snap = _oracle_snapshot(ora)
        assert snap["t"] == sim.time == after + 1
        _check_all_escaped(snap, 64)
        hb, ts = _check_reads(sim, (snap["hb"], snap["ts"]), f"after tick {after}")
        _check_all_escaped(dict(snap, hb=hb, ts=ts), 64)


# ---- 3. long-dead rows
def test_long_dead_rows_decode_relative_to_their_own_tick():
    kw = dict(KW300, init_mode=1)
    snap = _oracle_snapshot(_oracle_at(96, 60, crash_tick=10, crash_count=5, **kw))
    _check_long_dead(snap)
    sim = Simulator(96, GM_MODE_SCALED, **dict(kw, init_mode=0))
    state.restore(sim, snap)
    hb, ts = _check_reads(sim, (snap["hb"], snap["ts"]), "after the load")
    dead = snap["failed"] == 1
    assert np.array_equal(hb[dead], snap["hb"][dead]) and np.array_equal(ts[dead], snap["ts"][dead])
    _check_long_dead(dict(snap, hb=hb, ts=ts))


# ---- 4. payload / lag escapes
def test_payload_and_lag_escapes():
    ora = _oracle_at(600, 24, crash_tick=9, crash_count=6, **KW600)
    snap = _oracle_snapshot(ora)
    _check_payload_escapes(snap)
    sim = Simulator(600, GM_MODE_SCALED, **KW600)
    state.restore(sim, snap)
    hb, ts = _check_reads(sim, (snap["hb"], snap["ts"]), "at the load tick")
    _check_payload_escapes(dict(snap, hb=hb, ts=ts))
    _continue(sim, ora, 4)
    _check_reads(sim, ora.table(), "4 ticks after the load")


# ---- 5. band 1024 (a padded last band, the fast path) and band 512
@pytest.mark.parametrize("n,band", [(1540, 1024), (1100, 0)])
def test_wide_bands_with_a_padded_last_band(n, band):
    # band 1024 needs a padded row (a multiple of 512 columns) of whole bands: N = 1100 pads to 1536 and is
    # refused (test_gpu_multiband.py), so the 1024 case is N = 1540 -- band 0 full, 516 real columns in
    # band 1 -- and N = 1100 runs at the band width its row takes (pick_band: 512, 76 real columns in band 2)
    if band == 0:
        with pytest.raises(GmError):
            Simulator(n, GM_MODE_SCALED, band=1024)
    kw = dict(KW300, init_mode=1)
    sim = Simulator(n, GM_MODE_SCALED, band=band, **kw)
    crash = crash_set(n, (n + 99) // 100, 42)
    checked = []
    while sim.time <= 38:
        t = sim.time
        if t in (9, 28, 30, 32, 34, 35, 38):  # before the crash, stale entries escaping, the TREMOVE ticks, after
            _check_reads(sim, what=f"before tick {t}")
            checked.append(sim.event_totals()["removed"])
        _tick_with_crash([sim], crash)
    assert checked[0] == 0 and checked[-1] > 0, "no removal inside the run"
    assert sim.read_rows_stats()["stage_rows"] == n  # one launch held every row


# ---- 6. column shards
def test_column_shards():
    n, world = 600, 3
    kw = _shard_kw(0)
    ref = Simulator(n, GM_MODE_SCALED, **kw)
    shards = [Simulator(n, GM_MODE_SCALED, shard_rank=g, shard_count=world, **kw) for g in range(world)]
    crash = crash_set(n, 9, 42)
    for k in range(30):
        t = ref.time
        ref.tick()
        loopback_tick(shards)
        if t == 8:
            for s in [ref] + shards:
                s.set_failed(crash)
        if k in (1, 12, 24, 29):
            got = [_check_reads(s, what=f"shard {g} after tick {t}") for g, s in enumerate(shards)]
            whole = _check_reads(ref, what=f"single context after tick {t}")
            assert np.array_equal(np.concatenate([g[0] for g in got], axis=1), whole[0]), f"hb differs after tick {t}"
            assert np.array_equal(np.concatenate([g[1] for g in got], axis=1), whole[1]), f"ts differs after tick {t}"
    assert [s.shard_layout() for s in shards] == [(0, 200), (200, 200), (400, 200)]


# ---- 7. join ramp
def test_join_ramp():
    n = 120
    sim = Simulator(n, GM_MODE_SCALED, rd_seed=7, init_mode=2)
    ora = oracle_py.Oracle(n, oracle_py.OC_SCALED, rd_seed=7, init_mode=2)
    ora.tick()  # tick 0: nodeStart of nodes 0-3 (the GPU context starts as of tick 0)
    for t in (5, 20, 40):
        while sim.time < t:
            ora.tick()
            sim.tick()
        assert ora.time == sim.time == t
        hb, _ = _check_reads(sim, ora.table(), f"before tick {t}")
        if t == 40:  # every node has started (the last at tick 29) and is known: s_hbase of every column was used
            assert (hb >= 0).all()


# ---- 8. the block loop
def test_block_loop_and_buffer_reuse(monkeypatch):
    monkeypatch.setenv("GM_READ_STAGE_ROWS", "7")
    sim = Simulator(300, GM_MODE_SCALED, band=64, **dict(KW300, init_mode=1))
    crash = crash_set(300, 9, 42)
    while sim.time < 27:
        _tick_with_crash([sim], crash)
    assert sim.read_rows_stats()["rows"] == 0 and sim.read_rows_stats()["staging_bytes"] == 0
    assert _same(sim.read_rows(), sim.read_table())
    st = sim.read_rows_stats()
    assert st["rows"] == 300 and st["stage_rows"] == 7 and st["staging_bytes"] == 7 * 8 * 300
    sim.tick()
    assert _same(sim.read_rows(), sim.read_table())  # 43 launches through the same 7-row buffer
    st = sim.read_rows_stats()
    assert st["rows"] == 600 and st["stage_rows"] == 7
    _check_reads(sim, what="in blocks of 7 rows")
    assert st["decode_ms"] == 0 and st["copy_ms"] == 0  # timing is off
    sim.set_timing(True)
    sim.read_rows(0, 20)
    st = sim.read_rows_stats()
    assert st["decode_ms"] > 0 and st["copy_ms"] > 0


# ---- 9. a read-back: nothing a later tick or read observes changes
def test_reading_changes_nothing():
    kw = dict(KW300, init_mode=1)
    reader, twin = [Simulator(300, GM_MODE_SCALED, band=64, **kw) for _ in range(2)]
    for s in (reader, twin):
        s.detect_record(32)
    crash = crash_set(300, 9, 42)
    while reader.time < 26:
        _tick_with_crash([reader, twin], crash)
    events = [[], []]
    for k in range(10):  # ticks 26..35: stale entries escaping, the first removals
        reader.tick()
        twin.tick()
        events[0] += reader.drain_events()
        events[1] += twin.drain_events()
        if k < 9:
            reader.read_rows()
            reader.read_rows(11, 50)
    assert events[0] == events[1], "events differ"
    assert any(e[2] == GM_EV_REMOVED for e in events[0]), "no removal inside the run"
    assert _same(reader.read_table(), twin.read_table())
    assert np.array_equal(reader.read_nodes(), twin.read_nodes())
    assert _same_targets(reader.read_targets(), twin.read_targets())
    assert reader.event_totals() == twin.event_totals() and np.array_equal(reader.detect(), twin.detect())
    assert reader.tick_stats() == twin.tick_stats() and reader.tick_stats()["err"] == 0


# ---- 10. contract
def test_contract_modes():
    hb, ts = np.zeros((4, 64), dtype=np.int32), np.zeros((4, 64), dtype=np.int32)
    for sim in (Simulator(64, GM_MODE_PARTIAL, rd_seed=7, view_seed=5, init_mode=1, init_t0=8, init_seed=11),
                Simulator(10, GM_MODE_FAITHFUL)):
        assert sim.lib.gm_read_rows(sim.h, 0, 4, _ptr(hb), _ptr(ts)) == GM_EUNSUPPORTED
        with pytest.raises(GmError):
            sim.read_rows_stats()
    # contexts recording msgcount and detection are supported
    sim = Simulator(64, GM_MODE_SCALED, **dict(KW300, init_mode=1))
    sim.msgcount_record(32)
    sim.detect_record(32)
    for _ in range(3):
        sim.tick()
    _check_reads(sim, what="while recording msgcount and detection")


def test_contract_arguments_and_loading():
    n = 64
    kw = dict(KW300, init_mode=1)
    src = Simulator(n, GM_MODE_SCALED, **kw)
    for _ in range(4):
        src.tick()
    snap = state.snapshot(src)
    sim = Simulator(n, GM_MODE_SCALED, **dict(kw, init_mode=0))
    hb, ts = np.zeros((n, n), dtype=np.int32), np.zeros((n, n), dtype=np.int32)
    rd = sim.lib.gm_read_rows
    assert rd(None, 0, 1, _ptr(hb), _ptr(ts)) == GM_EINVAL
    assert rd(sim.h, -1, 1, _ptr(hb), _ptr(ts)) == GM_EINVAL
    assert rd(sim.h, 0, -1, _ptr(hb), _ptr(ts)) == GM_EINVAL
    assert rd(sim.h, 1, n, _ptr(hb), _ptr(ts)) == GM_EINVAL
    assert rd(sim.h, n, 1, _ptr(hb), _ptr(ts)) == GM_EINVAL
    assert rd(sim.h, 0x7FFFFFFF, 0x7FFFFFFF, _ptr(hb), _ptr(ts)) == GM_EINVAL  # r0 + count does not wrap
    assert rd(sim.h, 0, 1, None, _ptr(ts)) == GM_EINVAL and rd(sim.h, 0, 1, _ptr(hb), None) == GM_EINVAL
    assert rd(sim.h, 0, 0, None, None) == 0 and rd(sim.h, n, 0, None, None) == 0
    assert sim.lib.gm_read_rows_stats(sim.h, None) == GM_EINVAL
    assert rd(sim.h, 0, n, _ptr(hb), _ptr(ts)) == 0  # the cold-created state
    assert _same((hb, ts), sim.read_table())
    # GM_ESTATE between gm_load_begin and gm_load_commit
    assert sim.lib.gm_load_begin(sim.h, snap["t"]) == 0
    assert rd(sim.h, 0, 1, _ptr(hb), _ptr(ts)) == GM_ESTATE
    assert sim.lib.gm_load_rows(sim.h, 0, n, _ptr(snap["hb"]), _ptr(snap["ts"])) == 0
    assert rd(sim.h, 0, n, _ptr(hb), _ptr(ts)) == GM_ESTATE
    arrs = [np.ascontiguousarray(snap[k], dtype=np.int32) for k in ("heartbeat", "failed", "targets", "counts")]
    assert sim.lib.gm_load_commit(sim.h, *[_ptr(a) for a in arrs]) == 0
    assert rd(sim.h, 0, n, _ptr(hb), _ptr(ts)) == 0
    assert _same((hb, ts), (snap["hb"], snap["ts"]))
    sim.tick()
    src.tick()
    assert _same(sim.read_rows(), src.read_table())
    # a caller's own buffers: one pair reused block by block
    buf = (np.empty((16, n), dtype=np.int32), np.empty((16, n), dtype=np.int32))
    want = src.read_table()
    for r0 in (0, 16, 60):
        k = min(16, n - r0)
        got = sim.read_rows(r0, k, out=buf)
        assert got[0].shape == (k, n) and np.shares_memory(got[0], buf[0])
        assert _same(got, (want[0][r0:r0 + k], want[1][r0:r0 + k]))
    with pytest.raises(ValueError):
        sim.read_rows(0, 17, out=buf)


# ---- 11. membership.state
def test_state_device_snapshot_and_directory(tmp_path):
    n = 300
    kw = dict(KW300, init_mode=1)
    src = Simulator(n, GM_MODE_SCALED, band=64, **kw)
    crash = crash_set(n, 9, 42)
    while src.time < 27:
        _tick_with_crash([src], crash)
    src.drain_events()
    host, dev = state.snapshot(src), state.snapshot(src, device=True, chunk_rows=64)
    assert set(dev) == set(host) == set(state.KEYS) and dev["t"] == host["t"]
    for k in state.KEYS[1:]:
        assert dev[k].dtype == host[k].dtype and np.array_equal(dev[k], host[k]), k
    assert all(np.array_equal(state.snapshot(src, device=True)[k], host[k]) for k in ("hb", "ts"))
    state.save_dir(src, tmp_path / "s", chunk_rows=64)
    snap = state.load_dir(tmp_path / "s")
    assert isinstance(snap["hb"], np.memmap) and snap["t"] == host["t"]
    for k in state.KEYS[1:]:
        assert np.array_equal(snap[k], host[k]), k
    dst = Simulator(n, GM_MODE_SCALED, band=256, **dict(kw, init_mode=0))  # another band width
    state.restore(dst, snap, chunk_rows=50)
    assert dst.load_stats()["rows"] == n
    for _ in range(6):  # through the first removals
        t = src.time
        src.tick()
        dst.tick()
        assert src.drain_events() == dst.drain_events(), f"events differ at tick {t}"
        assert _same(dst.read_rows(), src.read_table()), f"tables differ at tick {t}"
        assert np.array_equal(dst.read_nodes(), src.read_nodes()), f"node state differs at tick {t}"
        assert _same_targets(dst.read_targets(), src.read_targets()), f"gossip targets differ at tick {t}"
    assert dst.tick_stats()["err"] == 0 and src.event_totals()["removed"] > 0


# ---- 12. widths that are no multiple of 4
def test_widths_not_a_multiple_of_four():
    kw = dict(KW300, init_mode=1)
    sim = Simulator(301, GM_MODE_SCALED, band=64, **kw)  # 45 real columns in the last band, rows 4-byte aligned only
    crash = crash_set(301, 9, 42)
    while sim.time <= 27:
        if sim.time in (9, 27):
            _check_reads(sim, what=f"N = 301 before tick {sim.time}")
        _tick_with_crash([sim], crash)
    n, world = 21, 3
    kw = _shard_kw(0)
    ref = Simulator(n, GM_MODE_SCALED, **kw)
    shards = [Simulator(n, GM_MODE_SCALED, shard_rank=g, shard_count=world, **kw) for g in range(world)]
    assert [s.shard_layout()[1] for s in shards] == [7, 7, 7]
    for _ in range(5):
        ref.tick()
        loopback_tick(shards)
    want = ref.read_table()
    got = []
    for s in shards:
        ref_s, n_s = s.read_table(), s.n
        assert _same(s.read_rows(), ref_s)
        assert _same(s.read_rows(n_s - 1, 1), (ref_s[0][-1:], ref_s[1][-1:]))
        got.append(s.read_rows())
    assert np.array_equal(np.concatenate([g[0] for g in got], axis=1), want[0])
    assert np.array_equal(np.concatenate([g[1] for g in got], axis=1), want[1])
