"""PARTIAL: how crashed nodes fade from the views, recorded on the device (gm_view_detect_record,
gm_view_detect, gm_view_detect_timeline; Simulator.view_detect*).

Every comparison is exact. The expected records and timeline are view_detect_ref.Expected, a plain
NumPy aggregation of what the test knows by other means: its own set_failed calls, and per tick the
views (read_views) and the drained events of a TWIN context that runs the same cluster unrecorded --
its events and views are pinned to PartialOracle by tests/test_gpu_partial.py, and
tests/test_view_detect_summary.py runs the same aggregation on the oracle itself. The recorded
context runs with keep_events(0): the recorder does not depend on event keeping. Each case asserts
from the expected data that it contains what it is there for.

 1. n = 64, V = 8: eight views per wave step, many observers per crashed subject on one address
 2. n = 300, V = 16: 30 crashed before the first tick; the fade to extinction, forget latencies
 3. n = 1000, V = 32, 30 % drops: late joins, rows written by the deferred (big-table) tick kernel
 4. n = 100, V = 12: V does not divide 64
 5. n = 128, V = 4, 90 % drops, no crash: TREMOVE removals, all of them false, nothing held
 5b. the same cluster with a crash inside its TREMOVE sweep: subjects falsely removed before they
    crash and truly removed after
 6. two crash waves: the crash bitmap is uploaded again while recording
 7. recording starts late and ends at tmax
 8. row shards on the loopback tick, GM_CHUNKS 1 and 4
 9. cross-check against the view census
10. recorder transparency: a recorded and an unrecorded context stay equal
11. the contract
"""
import ctypes

import numpy as np
import pytest

import view_detect_ref as ref
from membership import (GM_MODE_FAITHFUL, GM_MODE_PARTIAL, GM_MODE_SCALED, Simulator, crash_set,
                        merge_view_detect_shards, summarize_view_detect)
from membership.abi import VIEW_DETECT_DTYPE, GmViewDetectRec, partial_loopback_tick
from view_detect_ref import FALSE_REMOVALS, HELD, JOINS, LATE_JOINS, REMOVALS, T0

pytestmark = pytest.mark.gpu

GM_EINVAL, GM_ESTATE, GM_EUNSUPPORTED = -1, -5, -6


def _sim(case, **kw):
    c = ref.CASES[case]
    return Simulator(c["n"], GM_MODE_PARTIAL, view=c["v"], init_mode=1, **dict(ref.KW, **c.get("drops", {})), **kw)


def _crashes(case):
    c = ref.CASES[case]
    return {c["crash_tick"]: crash_set(c["n"], c["crash_count"], ref.CRASH_SEED)} if c["crash_count"] else {}


def _run(case, crashes=None, record_after=T0, tmax=None, hook=None):
    """The case on a recorded context (keep_events(0)) and its draining twin. crashes: {tick: indices
    given to set_failed after that tick ran} (T0: before the first tick). Returns (sim, twin, ex)."""
    c = ref.CASES[case]
    n, last = c["n"], T0 + c["ticks"]
    crashes = _crashes(case) if crashes is None else crashes
    tmax = last + 1 if tmax is None else tmax
    sim, twin = _sim(case), _sim(case)
    sim.keep_events(0)
    ex = ref.Expected(n, tmax)

    def after(t):
        if t in crashes:
            sim.set_failed(crashes[t])
            twin.set_failed(crashes[t])
            ex.set_failed(crashes[t], t)
        if t == record_after:
            sim.view_detect_record(tmax)

    after(T0)
    while sim.time <= last:
        t = sim.time
        sim.tick()
        twin.tick()
        ex.tick(t, twin.read_views(0, n), twin.drain_events(), recorded=record_after < t < tmax)
        if hook:
            hook(t, sim, ex)
        after(t)
    assert sim.tick_stats()["err"] == 0 and np.array_equal(twin.read_nodes()[:, 2] != 0, ex.crashed)
    return sim, twin, ex


def _compare(sim, ex, what):
    ref.assert_records(sim.view_detect(), ex.rec, what)
    ref.assert_timeline(sim.view_detect_timeline(len(ex.tl)), ex.tl, what)
    assert not sim.view_detect()["reserved"].any()


# ---- 1. many observers per crashed subject on one address
def test_small_cluster_contention():
    sim, _, ex = _run("n64_v8")
    _compare(sim, ex, "n64_v8")
    ref.check_fade(ex, "n64_v8")
    crashed = ex.crashed
    assert crashed.sum() == 4 and (ex.rec["fail_tick"][crashed] == 12).all()
    assert ex.tl[13, HELD] > 4 * 4, "fewer than four observers per crashed subject in one launch"
    assert ex.tl[:13, HELD].sum() == 0 and ex.tl[:, JOINS].sum() > 0


# ---- 2. the fade to extinction
def test_fade_to_extinction():
    sim, _, ex = _run("n300_v16")
    _compare(sim, ex, "n300_v16")
    ref.check_fade(ex, "n300_v16")
    got, crashed = sim.view_detect(), ex.crashed
    assert crashed.sum() == 30 and (got["fail_tick"][crashed] == T0).all() and (got["fail_tick"][~crashed] == -1).all()
    # the forget latency of every crashed subject, from the views of the twin alone
    assert (ex.rec["last_held"][crashed] >= 0).all(), "a crashed subject nobody held"
    want = ex.rec["last_held"][crashed].astype(np.int64) + 1 - T0
    assert np.array_equal(got["last_held"][crashed].astype(np.int64) + 1 - got["fail_tick"][crashed], want)
    assert (got["last_held"][~crashed] == -1).all() and not got["held_sum"][~crashed].any()
    s = summarize_view_detect(got, crashed, sim.view_detect_timeline(len(ex.tl)))
    assert s["extinct"] == 1.0 and s["forget_latency"]["max"] == int(want.max()) and s["forget_latency"]["min"] == int(want.min())
    assert s["stale_observer_ticks"] == int(ex.tl[:, HELD].sum()) and np.array_equal(s["fade"], ex.tl[:, HELD].astype(np.int64))


# ---- 3. late joins, rows of the deferred tick kernels
def test_late_joins_under_loss():
    most = []
    sim, _, ex = _run("n1000_v32_drops", hook=lambda t, sim, ex: most.append(sim.tick_stats()["max_inbox"]))
    _compare(sim, ex, "n1000_v32_drops")
    ref.check_fade(ex, "n1000_v32_drops")
    assert ex.tl[:, LATE_JOINS].sum() > 0 and ex.rec["late_joins"][ex.crashed].sum() == ex.tl[:, LATE_JOINS].sum()
    assert (ex.tl[:, LATE_JOINS] <= ex.tl[:, HELD]).all() and not ex.rec["late_joins"][~ex.crashed].any()
    # rows of the deferred kernels: more than P_KSMALL = 12 lists (the big table) in most ticks; more than
    # P_KP = 16 (the huge one) is a 1e-5 tail of Poisson(5) and not asserted at 1000 nodes
    assert max(most) > 12, "no node took the big-table kernel"


# ---- 4. V does not divide 64
def test_view_width_not_dividing_the_wave():
    sim, _, ex = _run("n100_v12")
    _compare(sim, ex, "n100_v12")
    ref.check_fade(ex, "n100_v12")


# ---- 5. sparse views: removals, all false
def test_sparse_views_false_removals():
    sim, _, ex = _run("sparse")
    _compare(sim, ex, "sparse")
    tl = ex.tl
    assert tl[:, REMOVALS].sum() > 0 and np.array_equal(tl[:, REMOVALS], tl[:, FALSE_REMOVALS])
    assert not tl[:, HELD].any() and not tl[:, LATE_JOINS].any()
    got = sim.view_detect()
    assert np.array_equal(got["removals"], got["false_removals"]) and (got["last_held"] == -1).all()
    seen = got["removals"] > 0
    assert (got["first_removed"][seen] <= got["last_removed"][seen]).all() and (got["first_removed"][~seen] == -1).all()
    assert (got["removals"] > 1).any(), "no subject with several removals: first / last / tick sum untested"


# ---- 5b. falsely removed before the crash, truly after
def test_sparse_views_crash_inside_the_sweep():
    sim, _, ex = _run("sparse_crash")
    _compare(sim, ex, "sparse_crash")
    ref.check_fade(ex, "sparse_crash")
    r = ex.rec[ex.crashed]
    both = (r["false_removals"] > 0) & (r["removals"] > r["false_removals"])
    assert both.any(), "no subject removed falsely before its crash and truly after"
    assert (r["first_removed"][both] <= r["fail_tick"][both]).all() and (r["last_removed"][both] > r["fail_tick"][both]).all()
    s = summarize_view_detect(sim.view_detect(), ex.crashed)
    assert s["false_removals"]["crashed_later"] == int(r["false_removals"].sum()) > 0
    assert s["false_removals"]["total"] == int(ex.tl[:, FALSE_REMOVALS].sum()) and s["removals"] == int(ex.tl[:, REMOVALS].sum())


# ---- 6. two crash waves
def test_two_crash_waves():
    """Case 2's cluster loses no message, so no view starves: the CPU search over it (the oracle,
    40 ticks) found no TREMOVE removal at all, hence no subject falsely removed before it crashes;
    test_sparse_views_crash_inside_the_sweep covers that on the cluster that has them."""
    n = ref.CASES["n300_v16"]["n"]
    first, second = crash_set(n, 30, ref.CRASH_SEED), crash_set(n, 25, ref.CRASH_SEED + 1)
    new = np.setdiff1d(second, first)
    assert 0 < len(new) and len(new) <= len(second), "the second wave names nobody new"
    sim, _, ex = _run("n300_v16", crashes={T0: first, 20: second})
    _compare(sim, ex, "two waves")
    got = sim.view_detect()
    assert (got["fail_tick"][first] == T0).all() and (got["fail_tick"][new] == 20).all()
    held = ex.tl[:, HELD]
    assert held[9:13].sum() > 0 and held[17:21].sum() == 0 and held[21] > 0 and held[-1] == 0, "not two fades"
    assert (ex.rec["last_held"][new] >= 21).all() and (ex.rec["last_held"][first] < 20).all()
    assert ex.tl[21:, LATE_JOINS].sum() > 0


# ---- 7. a late start and tmax
def test_late_start_and_tmax():
    snap = {}

    def hook(t, sim, ex):
        if t == 23:
            snap["rec"], snap["tl"] = sim.view_detect(), sim.view_detect_timeline(24)

    sim, _, ex = _run("n300_v16", record_after=14, tmax=24, hook=hook)
    assert sim.time - 1 == T0 + 40
    _compare(sim, ex, "ticks 15..23 of 9..48")
    tl = sim.view_detect_timeline(24)
    assert not tl[:15].any() and (tl[15:24, JOINS] > 0).all(), "ticks up to 14 are zero, 15..23 are recorded"
    ref.assert_records(sim.view_detect(), snap["rec"], "records after ticks past tmax")
    assert np.array_equal(tl, snap["tl"]), "the timeline changed after tmax"
    assert sim.lib.gm_view_detect_timeline(sim.h, 25, tl.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))) == GM_EINVAL


# ---- 8. row shards
@pytest.mark.parametrize("chunks", [1, 4])
@pytest.mark.parametrize("case,world", [("n1000_v32_drops", 3), ("n300_v16", 2)])
def test_row_shards(case, world, chunks, monkeypatch):
    c = ref.CASES[case]
    n, last = c["n"], T0 + 12
    monkeypatch.setenv("GM_CHUNKS", str(chunks))
    shards = [_sim(case, shard_rank=g, shard_count=world) for g in range(world)]
    monkeypatch.delenv("GM_CHUNKS")
    one = _sim(case)  # recorded and drained: the single context, and the source of the expected parts
    crashes = _crashes(case)
    layout = [s.shard_layout() for s in shards]
    parts = [ref.Expected(n, last + 1, n0, nloc) for n0, nloc in layout]
    assert sum(nloc for _, nloc in layout) == n

    def after(t):
        if t in crashes:
            for s in shards + [one]:
                s.set_failed(crashes[t])
            for p in parts:
                p.set_failed(crashes[t], t)

    after(T0)
    for s in shards + [one]:
        s.view_detect_record(last + 1)
    for s in shards:
        s.keep_events(0)
    while one.time <= last:
        t = one.time
        one.tick()
        partial_loopback_tick(shards)
        views, events = one.read_views(0, n), one.drain_events()
        for p in parts:
            p.tick(t, views, events)
        after(t)
    got = [s.view_detect() for s in shards]
    tls = [s.view_detect_timeline(last + 1) for s in shards]
    for g in range(world):
        ref.assert_records(got[g], parts[g].rec, f"shard {g}")
        ref.assert_timeline(tls[g], parts[g].tl, f"shard {g}")
        assert tls[g][:, HELD].sum() > 0, f"shard {g} held no entry of a crashed subject"
    ref.assert_records(merge_view_detect_shards(got), one.view_detect(), "merged row shards vs the single context")
    ref.assert_timeline(sum(tls), one.view_detect_timeline(last + 1), "summed row shards vs the single context")
    assert all(s.tick_stats()["err"] == 0 for s in shards)


# ---- 9. against the view census
def test_against_the_view_census():
    seen = []

    def hook(t, sim, ex):
        if t not in (10, 11):
            return
        holders = sim.view_census()[0]["holders"]
        rec, tl = sim.view_detect(), sim.view_detect_timeline(t + 1)
        crashed = ex.crashed
        assert holders[crashed].sum() == tl[t, HELD]
        assert (rec["last_held"][crashed & (holders > 0)] == t).all() and (rec["last_held"][crashed & (holders == 0)] < t).all()
        seen.append(int(tl[t, HELD]))

    _run("n300_v16", hook=hook)
    assert len(seen) == 2 and seen[0] > 0, "tick 10 is not inside the fade"


# ---- 10. recorder transparency
def test_recorder_is_transparent():
    case = "n1000_v32_drops"
    c = ref.CASES[case]
    a, b = _sim(case), _sim(case)
    a.view_detect_record(T0 + 1 + c["ticks"])
    crashes, events = _crashes(case), 0
    for _ in range(c["ticks"]):
        t = a.time
        a.tick()
        b.tick()
        ea, eb = a.drain_events(), b.drain_events()
        assert ea == eb, f"events differ at tick {t}"
        assert a.dump_tables() == b.dump_tables(), f"views differ at tick {t}"
        events += len(ea)
        if t in crashes:
            a.set_failed(crashes[t])
            b.set_failed(crashes[t])
    assert events > 0 and a.view_detect_timeline(a.time)[:, JOINS].sum() > 0
    assert np.array_equal(a.read_nodes(), b.read_nodes()) and a.tick_stats() == b.tick_stats()


# ---- 11. the contract
def _rc_record(sim, tmax):
    return sim.lib.gm_view_detect_record(sim.h, tmax)


def _rc_detect(sim, n):
    out = np.zeros(n, dtype=VIEW_DETECT_DTYPE)
    return sim.lib.gm_view_detect(sim.h, out.ctypes.data_as(ctypes.POINTER(GmViewDetectRec)))


def _rc_timeline(sim, t, rows=None):
    out = np.zeros((max(rows or t, 1), 5), dtype=np.uint64)
    return sim.lib.gm_view_detect_timeline(sim.h, t, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)))


def test_contract():
    for other in (Simulator(10, GM_MODE_FAITHFUL),
                  Simulator(256, GM_MODE_SCALED, rd_seed=7, init_mode=1, init_t0=8, init_seed=11)):
        assert _rc_record(other, 100) == GM_EUNSUPPORTED
    sim = _sim("n300_v16")
    n = sim.n
    assert _rc_detect(sim, n) == GM_ESTATE and _rc_timeline(sim, 10) == GM_ESTATE
    assert _rc_record(sim, 0) == GM_EINVAL and _rc_record(sim, 32768) == GM_EINVAL and _rc_record(sim, -1) == GM_EINVAL
    assert _rc_detect(sim, n) == GM_ESTATE, "a refused record call started recording"
    assert sim.lib.gm_detect_record(sim.h, 100) == GM_EUNSUPPORTED
    sim.tick()
    assert _rc_record(sim, 32767) == 0
    assert _rc_record(sim, 100) == GM_ESTATE
    sim.tick()
    assert _rc_detect(sim, n) == 0
    assert _rc_timeline(sim, 0) == GM_EINVAL and _rc_timeline(sim, 32768, rows=1) == GM_EINVAL
    assert _rc_timeline(sim, 1) == 0 and _rc_timeline(sim, 32767) == 0
    tl = sim.view_detect_timeline(sim.time)
    assert not tl[:10].any() and tl[10, JOINS] > 0, "recording starts with the tick after the call"
    assert sim.lib.gm_load_views_begin(sim.h, sim.time) == GM_EUNSUPPORTED
    assert sim.lib.gm_detect_record(sim.h, 100) == GM_EUNSUPPORTED
    sim.tick()  # the refused load left the context running
    assert sim.view_detect_timeline(sim.time)[11, JOINS] > 0
