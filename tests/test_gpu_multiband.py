"""The single-context SCALED tick at B = 1024 and more than one band: gm_s_band_fast with two bands
per wave (the second unit's shared row metadata, its loads issued under the first unit's stores, the
recovery after a hand-back), the single-band tail wave of an odd band count, a padded last band, and
gm_s_pick0's band search (the band prefix, the per-lane band ranges, two search levels).

1. test_oracle_window*: the production path against the oracle at nb = 2 (N = 1540: 516 real columns
   in band 1; N = 1538: N % 4 = 2, an invalid-row tail in gm_s_pick0's workgroups of 16 rows) and
   nb = 3 (N = 2564: a two-band wave plus a single-band tail wave per row, 516 real columns in band 2).
   The oracle costs ~N^2 per tick, so the GPU runs alone up to a window, hands its state to the oracle
   (read_table / read_nodes / read_targets -> load_state, as test_oracle_continues_from_gpu_state) and
   every transition inside the window is compared exactly: events in order, every cell and node state,
   the gossip draws, err == 0. A hand-over trusts the state at the window's start only. Each window
   asserts from the oracle's own data that it is what it claims (a drifted schedule fails loudly):
     A  the crash window: crashed columns escaped and stale (age >= 15), nothing removed yet
     B  the TREMOVE peak: removals in every band
     C  a cold start from the first tick, every list past its 16-entry inline slot (N = 1540 only)
2. the fast path against the general path at nb = 3 and nb = 4 with a padded last band is
   test_gpu_band_fast.py's test_fast_path_matches_general_kernels_odd_and_padded_bands.
3. test_pick0_matches_pick_two_level_search: gm_s_pick0 against gm_s_pick (GM_PICK0=0) at N = 17000
   (nb = 17: perb = 2 -- lanes 0-7 of a row's 16 hold two bands, lane 8 one, lanes 9-15 none; the
   search's first level has step 2; 616 real columns in the last band; N % 16 = 8), through the crash
   window, where stale rejections make rows use up their 16 outputs and fall to the listed gm_s_pick.
   No oracle: one oracle tick takes minutes at this N.

Every Simulator here passes band=1024: a size whose padded row is no multiple of 1024 fails at create
instead of silently testing the 512 path (test_band_1024_needs_a_padded_row_of_whole_bands).

Wall time per case (MI355X host, oracle on one core), oracle ticks in brackets:
  test_oracle_window[1540-A] 1.0 s [2]   [1540-B] 0.9 s [3]   [1538-A] 0.6 s [2]   [1538-B] 0.9 s [3]
  test_oracle_window[2564-A] 1.1 s [1]   [2564-B] 2.1 s [2]   test_oracle_window_cold_start 0.4 s [3]
  test_pick0_matches_pick_two_level_search 0.1 s [0]; test_gpu_band_fast.py's new cases 1.3 s (N = 2564)
  and 2.6 - 2.9 s (N = 3586), no oracle. A slower host core triples the oracle's share (0.8 s per
  tick at N = 1540, 2.4 s at N = 2564), which is why each window is a case of its own.

Reference: the merge MP1Node.cpp:278-299, the sweep MP1Node.cpp:426-444, the draw MP1Node.cpp:449-489."""
import numpy as np
import pytest

import oracle_py
from golden_util import same_state
from membership import GM_EV_REMOVED, GM_MODE_SCALED, GmError, Simulator, crash_set

pytestmark = pytest.mark.gpu

CRASH_TICK = 10
# One oracle run per size located the windows (warm start at t0 = 8, ceil(N / 100) nodes crashed at
# tick 10; the same ticks at N = 1538, 1540 and 2564): entries of the crashed columns reach age 15
# from tick 26 on (~9 per live row and 1024-column slice at tick 30), the first removals are tick 31's,
# the peak is ticks 34-35 (N = 1540: 9080 and 11452 of the 24384 removals), the last are tick 37's.
WINDOW_TICKS = {
    ("A", 2): (29, 30),      # 5 oracle ticks per size at N ~ 1540
    ("B", 2): (33, 34, 35),
    ("A", 3): (30,),         # 3 at N = 2564
    ("B", 3): (34, 35),
}


def _same_targets(got, want):
    # targets past a row's count are unspecified (the oracle keeps older draws there)
    (tg, cg), (tw, cw) = got, want
    used = np.arange(tg.shape[1])[None, :] < cw[:, None]
    return np.array_equal(cg, cw) and np.array_equal(np.where(used, tg, 0), np.where(used, tw, 0))


def _compare_tick(sim, ora, t):
    """One tick on both sides, every output compared; returns the oracle's events."""
    assert ora.time == t == sim.time
    ora.tick()
    sim.tick()
    err = sim.tick_stats()["err"]  # first: a latched flag makes the readbacks below raise without the tick
    assert err == 0, f"error flags {err:#x} at tick {t}"
    ev = ora.events()
    assert sim.drain_events() == ev, f"events differ at tick {t}"
    assert same_state(sim, ora), f"tables or node state differ at tick {t}"
    assert _same_targets(sim.read_targets(), ora.targets()), f"gossip targets differ at tick {t}"
    return ev


def _band_slices(n):
    return [slice(c, min(c + 1024, n)) for c in range(0, n, 1024)]


@pytest.mark.parametrize("window", ["A", "B"])
@pytest.mark.parametrize("n", [1540, 1538, 2564])
def test_oracle_window(n, window):
    nb = (n + 1023) // 1024
    ticks = WINDOW_TICKS[window, nb]
    ncrash = (n + 99) // 100
    kw = dict(rd_seed=7, init_mode=1, init_t0=8, init_seed=11)
    sim = Simulator(n, GM_MODE_SCALED, band=1024, **kw)
    crash = crash_set(n, ncrash, 42)
    while sim.time < ticks[0]:  # the GPU alone up to the window
        t = sim.time
        sim.tick()
        if t == CRASH_TICK:
            sim.set_failed(crash)
    sim.drain_events()
    ora = oracle_py.Oracle(n, oracle_py.OC_SCALED, crash_tick=CRASH_TICK, crash_count=ncrash, crash_seed=42, **kw)
    hb, ts = sim.read_table()
    st = sim.read_nodes()
    tg, cnt = sim.read_targets()
    ora.load_state(sim.time, hb, ts, st[:, 3], st[:, 2], tg, cnt)
    removed = np.zeros(0, dtype=np.int64)
    for t in ticks:
        ev = _compare_tick(sim, ora, t)
        removed = np.concatenate([removed, np.array([e[3] for e in ev if e[2] == GM_EV_REMOVED], dtype=np.int64)])
        if window == "A":  # from the oracle's data: stale entries beyond the stored byte's age range in every band
            ohb, ots = ora.table()
            live = ora.nodes()[:, 2] == 0
            old = (ohb >= 0) & (t - ots >= 15) & live[:, None]
            for b, cols in enumerate(_band_slices(n)):
                assert old[:, cols].sum() > 0, f"no entry of age >= 15 in band {b} at tick {t}"
    if window == "A":
        assert len(removed) == 0, "a removal inside the crash window"
    else:  # removed subjects (ids, 1-based) in every band
        for b in range(nb):
            assert ((removed > 1024 * b) & (removed <= 1024 * (b + 1))).sum() > 0, f"no removal in band {b}"


def test_oracle_window_cold_start():
    # window C: both sides from the first tick of a cold start. Every entry's heartbeat is outside the
    # stored byte's range, so every cell is escaped, the lists run past the inline slot into the striped
    # pool, and gm_s_band_fast hands its units back to gm_s_band_listed
    n = 1540
    kw = dict(rd_seed=7, init_mode=0, init_t0=0, init_seed=11)
    sim = Simulator(n, GM_MODE_SCALED, band=1024, **kw)
    ora = oracle_py.Oracle(n, oracle_py.OC_SCALED, crash_tick=CRASH_TICK, crash_count=16, crash_seed=42, **kw)
    for _ in range(3):
        t = sim.time
        ev = _compare_tick(sim, ora, t)
        assert ev == []  # converged: no joins, no removals
        ohb, ots = ora.table()
        h = 255 - (2 * t - ohb)  # the 16-bit cell's heartbeat field and age (gm_scaled.h)
        esc = (ohb >= 0) & ~((h >= 230) & (h % 2 == 0) & (t - ots <= 14))
        for b, cols in enumerate(_band_slices(n)):
            assert esc[:, cols].sum(axis=1).min() > 16, f"a list of band {b} fits the inline slot at tick {t}"


def test_band_1024_needs_a_padded_row_of_whole_bands():
    # rows are padded to a multiple of 512 columns: N = 3074 pads to 3584 = 3.5 bands, and an explicit
    # band of 1024 is refused (the sizes of this module and of test_gpu_band_fast.py all create)
    with pytest.raises(GmError):
        Simulator(3074, GM_MODE_SCALED, band=1024)


def test_pick0_matches_pick_two_level_search(monkeypatch):
    n, ncrash = 17000, 170
    kw = dict(rd_seed=7, init_mode=1, init_t0=8, init_seed=11, band=1024)
    pick0 = Simulator(n, GM_MODE_SCALED, **kw)
    monkeypatch.setenv("GM_PICK0", "0")
    pick = Simulator(n, GM_MODE_SCALED, **kw)
    monkeypatch.delenv("GM_PICK0")
    crash = crash_set(n, ncrash, 42)
    t = -1
    while pick0.time <= 30:  # the crashed entries are stale from tick ~15 on; the first removals are tick 31's
        t = pick0.time
        for s in (pick0, pick):
            s.tick()
            if t == CRASH_TICK:
                s.set_failed(crash)
        sa, sb = pick0.tick_stats(), pick.tick_stats()
        assert sa["err"] == 0 and sb["err"] == 0, f"error flags {sa['err']:#x} / {sb['err']:#x} at tick {t}"
        assert sa == sb, f"tick stats differ at tick {t}"
        (ta, ca), (tb, cb) = pick0.read_targets(), pick.read_targets()
        assert np.array_equal(ca, cb), f"target counts differ at tick {t}"
        assert np.array_equal(ta, tb), f"targets differ at tick {t}"
        assert pick0.event_totals() == pick.event_totals(), f"event totals differ at tick {t}"
    for r in (0, 1023, 1024, 16383, 16384, n - 1):
        a, b = pick0.read_row(r), pick.read_row(r)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), f"row {r} differs at tick {t}"
    st = pick0.tick_stats()
    assert st["err"] == 0 and st["live"] == n - ncrash
    assert pick0.event_totals()["removed"] == 0  # the run stopped before TREMOVE
