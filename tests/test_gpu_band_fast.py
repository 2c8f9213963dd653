"""gm_s_band's fast path (B = 1024: merge and sweep on the stored bytes, SWAR counts, the rare
cells redone one by one; gm_band_fast.hip unit_fast) against the general path (GM_BAND_FAST=0),
tick by tick: events in order, tick statistics, membership tables, msgcount. The schedules drive
every branch of the fast path: the crash window (cells aging to 15 escape, then TREMOVE removes
them: the per-cell pass, the quick case of a slice whose escapes only age, and the removal events), cold start (every cell escaped: escape lists read
back), a loss window (DROP ticks take the general kernel; the ticks after it deliver stale and
lagging entries, so units are handed back to the general path), and column shards. At an odd and
a padded band count (nb = 3, nb = 4) a third context runs the general band and pick kernels
together (GM_BAND_FAST=0, GM_PICK0=0) and the gossip draws are compared too. The oracle parity of
both paths at one band is test_gpu_scaled.py's (bands 1024 included); at more bands it is
test_gpu_multiband.py's: oracle windows on the production path at nb = 2 and 3, and
gm_s_pick0 == gm_s_pick at nb = 17 (a two-level band search). Reference: the merge
MP1Node.cpp:278-299, the sweep MP1Node.cpp:426-444, sendMemberList MP1Node.cpp:360-395."""
import numpy as np
import pytest

from membership import GM_MODE_SCALED, Simulator, crash_set
from membership.sharded import loopback_tick

pytestmark = pytest.mark.gpu


def _pair(monkeypatch, n, **kw):
    monkeypatch.setenv("GM_BAND_FAST", "0")
    gen = Simulator(n, GM_MODE_SCALED, **kw)
    monkeypatch.setenv("GM_BAND_FAST", "1")
    fast = Simulator(n, GM_MODE_SCALED, **kw)
    monkeypatch.delenv("GM_BAND_FAST")
    return gen, fast


def _same_tables(a, b, n, t):
    ha, ta = a.read_table(0, n)
    hb, tb = b.read_table(0, n)
    assert np.array_equal(ha, hb) and np.array_equal(ta, tb), f"tables differ at tick {t}"


@pytest.mark.parametrize("init_mode,loss,ncrash", [(1, 0, 41), (1, 0, 20), (0, 0, 41), (1, 1, 41), (0, 2, 41)])
def test_fast_path_matches_general_path(monkeypatch, init_mode, loss, ncrash):
    # ncrash 20 (1 %, S-A's share): ~10 escaped cells per 1024-column slice, so most units of the
    # crash window take the fast path's quick case (inline list, stale, undelivered; removals by the
    # gone-entry loop); 41 (2 %): ~20 per slice, past the inline slot, the park path
    n = 2048
    kw = dict(rd_seed=7, init_mode=init_mode, init_t0=8 if init_mode else 0, init_seed=11, band=1024)
    if loss == 1:  # 40 % loss for ticks 12..19: stale and lagging entries afterwards
        kw.update(drop_pct=40, drop_from=12, drop_to=20, drop_seed=5)
    elif loss == 2:  # one keyed-loss tick between fast ticks of the same parity (the hand-back
        # list's count of tick 14 must not survive into tick 16), after a cold start's hand-backs
        kw.update(drop_pct=20, drop_from=15, drop_to=16, drop_seed=5)
    gen, fast = _pair(monkeypatch, n, **kw)
    for s in (gen, fast):
        s.msgcount_record(64)
    crash = crash_set(n, ncrash, 42)
    for _ in range(56):
        t = fast.time
        gen.tick()
        fast.tick()
        if t == 10:
            gen.set_failed(crash)
            fast.set_failed(crash)
        assert gen.drain_events() == fast.drain_events(), f"events differ at tick {t}"
        assert gen.tick_stats() == fast.tick_stats(), f"tick stats differ at tick {t}"
        if t % 4 == 0 or 24 <= t <= 40:
            _same_tables(gen, fast, n, t)
        (sg, rg), (sf, rf) = gen.msgcount(t), fast.msgcount(t)
        assert np.array_equal(sg, sf) and np.array_equal(rg, rf), f"msgcount differs at tick {t}"
    assert fast.tick_stats()["err"] == 0


def _same_arrays(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("init_mode,loss,crash_pct", [(1, 0, 1), (0, 2, 2)])
@pytest.mark.parametrize("n", [2564, 3586])
def test_fast_path_matches_general_kernels_odd_and_padded_bands(monkeypatch, n, init_mode, loss, crash_pct):
    # nb = 3 (N = 2564: per row one two-band wave and a single-band tail wave; 516 real columns in the
    # last band) and nb = 4 (N = 3586: 514 real columns in the last band, N % 4 = 2 -- rows pad to a
    # multiple of 512 columns, so no 1024-band region has a last band of fewer than 513). Three contexts:
    # the production path (gm_s_band_fast + gm_s_pick0), the general band kernel with gm_s_pick0, and
    # the general kernels alone (GM_BAND_FAST=0 with GM_PICK0=0: gm_s_band + gm_s_pick, which the oracle
    # pins at many bands, test_scaled_every_band_width_matches_oracle). Both are compared with the
    # production path every tick, the gossip draws included.
    kw = dict(rd_seed=7, init_mode=init_mode, init_t0=8 if init_mode else 0, init_seed=11, band=1024)
    if loss == 2:  # as above: one keyed-loss tick between fast ticks, after a cold start's hand-backs
        kw.update(drop_pct=20, drop_from=15, drop_to=16, drop_seed=5)
    gen, fast = _pair(monkeypatch, n, **kw)
    monkeypatch.setenv("GM_BAND_FAST", "0")
    monkeypatch.setenv("GM_PICK0", "0")
    plain = Simulator(n, GM_MODE_SCALED, **kw)
    monkeypatch.delenv("GM_BAND_FAST")
    monkeypatch.delenv("GM_PICK0")
    sims = {"production path": fast, "general band kernel": gen, "general band and pick kernels": plain}
    for s in sims.values():
        s.msgcount_record(64)
    crash = crash_set(n, (n * crash_pct + 99) // 100, 42)
    for _ in range(56):
        t = fast.time
        for s in sims.values():
            s.tick()
            if t == 10:
                s.set_failed(crash)
        want = None
        for name, s in sims.items():
            got = {"events": [s.drain_events_np()], "tick stats": s.tick_stats(), "targets": s.read_targets(),
                   "msgcount": s.msgcount(t)}
            if t % 4 == 0 or 24 <= t <= 40:
                got["tables"] = s.read_table(0, n)
            if want is None:
                want = got
                continue
            assert got["tick stats"] == want["tick stats"], f"tick stats differ at tick {t}: {name}"
            for k in ("events", "targets", "msgcount", "tables"):
                assert k not in want or _same_arrays(got[k], want[k]), f"{k} differ at tick {t}: {name}"
    assert fast.tick_stats()["err"] == 0


def test_fast_path_column_shards_match_general_path(monkeypatch):
    # G = 2 column shards (loopback exchange), fast path on vs off: the shards' own columns
    # (c0 offsets, the own cell in one shard only) through the same schedule
    n, G = 4096, 2
    kw = dict(rd_seed=7, init_mode=1, init_t0=8, init_seed=11, band=1024)
    sims = {}
    for fast in (0, 1):
        monkeypatch.setenv("GM_BAND_FAST", str(fast))
        sims[fast] = [Simulator(n, GM_MODE_SCALED, shard_rank=g, shard_count=G, **kw) for g in range(G)]
    monkeypatch.delenv("GM_BAND_FAST")
    crash = crash_set(n, 41, 42)
    for _ in range(44):
        t = sims[1][0].time
        for f in (0, 1):
            loopback_tick(sims[f])
            if t == 10:
                for s in sims[f]:
                    s.set_failed(crash)
        for g in range(G):
            assert sims[0][g].drain_events() == sims[1][g].drain_events(), f"events differ at tick {t}, shard {g}"
            if t % 6 == 0 or 30 <= t <= 38:
                w = sims[0][g].shard_layout()[1]
                for r in (0, 1, 2047, 2048, n - 1):
                    a = sims[0][g].read_row(r, 0, w)
                    b = sims[1][g].read_row(r, 0, w)
                    assert all(np.array_equal(x, y) for x, y in zip(a, b)), f"row {r} differs at tick {t}"
    for g in range(G):
        assert sims[1][g].tick_stats()["err"] == 0
