"""gm_s_band_fast's row order (gm_band_fast.hip: the grid's x interleaves GM_FAST_XS stripes of
consecutive rows) and its plain, single-writer evcum write against the general path
(GM_BAND_FAST=0), tick by tick, at band 1024.

Row order: N = 2564 (nb = 3: a two-band wave and a single-band tail wave per row; N is no multiple
of the interleave, so the grid's last workgroups are idle) and N = 2048, 40 ticks with a 1 % crash at
tick 10 -- through the crash window and the TREMOVE removals. Each tick: events, tick statistics,
msgcount; tables every 4th tick; event_totals (the sum of the evcum cells) at the end. The same on one
context, on G = 2 loopback column shards (the phase API: every row in one launch), and on the
pipelined tick's row chunks (gm_shard_loopback_tick, GM_SCHUNKS=3: two exchange chunks, the kernel's
chunk variant with a unit range [u0, u1), u0 > 0; it takes no msgcount recording). Two column shards
of N = 2564 cannot be created at band 1024 (a shard's 1282 columns pad to 1536, no multiple of the
band), so the odd shape of the sharded runs is N = 4092: shards of 2044 and 2048 columns (nb = 2),
N no multiple of the interleave, and a last row chunk of 2044 rows.

Inbox sizes: the fast path's payload gathers depend on the row's inbox size k. N = 2048, 24 ticks:
every k from 0 to 10 must have occurred at some row, and some row must have had k > 8 (more lists
than sender ids prefetched) -- a condition on the inputs (checked against the CPU oracle: each tick
has about 15 rows at k = 0 and about 140 at k >= 9), next to the tick-by-tick equality."""
import numpy as np
import pytest

from membership import GM_MODE_SCALED, Simulator, crash_set
from membership.abi import shard_loopback_tick
from membership.sharded import loopback_tick

pytestmark = pytest.mark.gpu

KW = dict(rd_seed=7, init_mode=1, init_t0=8, init_seed=11, band=1024)


def _contexts(monkeypatch, n, fast, shards, chunks=0):
    monkeypatch.setenv("GM_BAND_FAST", str(fast))
    if chunks:
        monkeypatch.setenv("GM_SCHUNKS", str(chunks))
    if shards == 1:
        sims = [Simulator(n, GM_MODE_SCALED, **KW)]
    else:
        sims = [Simulator(n, GM_MODE_SCALED, shard_rank=g, shard_count=shards, **KW) for g in range(shards)]
    monkeypatch.delenv("GM_BAND_FAST")
    monkeypatch.delenv("GM_SCHUNKS", raising=False)
    return sims


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("n,how", [(2564, "one context"), (2048, "one context"),
                                   (4092, "column shards"), (2048, "column shards"),
                                   (4092, "pipelined row chunks"), (2048, "pipelined row chunks")])
def test_row_order_matches_general_path(monkeypatch, n, how):
    shards = 1 if how == "one context" else 2
    pipelined = how == "pipelined row chunks"
    gen = _contexts(monkeypatch, n, 0, shards, 3 if pipelined else 0)
    fast = _contexts(monkeypatch, n, 1, shards, 3 if pipelined else 0)
    if not pipelined:
        for s in gen + fast:
            s.msgcount_record(64)
    crash = crash_set(n, (n + 99) // 100, 42)
    for _ in range(40):
        t = fast[0].time
        for sims in (gen, fast):
            if shards == 1:
                sims[0].tick()
            elif pipelined:
                shard_loopback_tick(sims)
            else:
                loopback_tick(sims)
            if t == 10:
                for s in sims:
                    s.set_failed(crash)
        for g in range(shards):
            where = f"at tick {t}, shard {g}"
            assert _same([gen[g].drain_events_np()], [fast[g].drain_events_np()]), f"events differ {where}"
            assert gen[g].tick_stats() == fast[g].tick_stats(), f"tick stats differ {where}"
            if not pipelined:
                assert _same(gen[g].msgcount(t), fast[g].msgcount(t)), f"msgcount differs {where}"
            if t % 4 == 0:
                assert _same(gen[g].read_table(0, n), fast[g].read_table(0, n)), f"tables differ {where}"
    removed = 0
    for g in range(shards):
        assert gen[g].event_totals() == fast[g].event_totals(), f"event totals differ, shard {g}"
        assert fast[g].tick_stats()["err"] == 0
        removed += fast[g].event_totals()["removed"]
    assert removed > 0, "the schedule did not reach the removals"


def test_every_inbox_size_matches_general_path(monkeypatch):
    n = 2048
    (gen,), (fast,) = _contexts(monkeypatch, n, 0, 1), _contexts(monkeypatch, n, 1, 1)
    for s in (gen, fast):
        s.msgcount_record(64)
    seen = set()
    for _ in range(24):
        t = fast.time
        gen.tick()
        fast.tick()
        tg, cnt = fast.read_targets()
        assert _same(gen.read_targets(), (tg, cnt)), f"targets differ at tick {t}"
        # the lists drawn this tick are the next tick's inboxes: k per row
        k = np.bincount(tg[np.arange(5)[None, :] < cnt[:, None]], minlength=n)
        seen |= set(np.unique(k).tolist())
        assert _same([gen.drain_events_np()], [fast.drain_events_np()]), f"events differ at tick {t}"
        assert gen.tick_stats() == fast.tick_stats(), f"tick stats differ at tick {t}"
        assert _same(gen.msgcount(t), fast.msgcount(t)), f"msgcount differs at tick {t}"
        if t % 4 == 0:
            assert _same(gen.read_table(0, n), fast.read_table(0, n)), f"tables differ at tick {t}"
    assert gen.event_totals() == fast.event_totals()
    assert fast.tick_stats()["err"] == 0
    assert set(range(11)) <= seen and max(seen) > 8, f"inbox sizes seen: {sorted(seen)}"
