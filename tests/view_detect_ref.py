"""The PARTIAL detection recorder (gm_view_detect_record, include/gm_abi.h) in plain NumPy: the
specification the GPU tests compare against, exactly. A helper, not a test.

One Expected object follows one recorded context (or one row shard of it). The test feeds it what it
knows by other means: its own set_failed calls, and per tick the views after the tick (what
Simulator.read_views() returns, or PartialOracle.dump() through view_census_ref.views_from_dump) and
the tick's (t, logger, kind, subject) event tuples (a draining twin's, or PartialOracle.events())."""
import numpy as np

from membership.abi import GM_EV_JOINED, GM_EV_REMOVED, VIEW_DETECT_DTYPE

JOINS, REMOVALS, FALSE_REMOVALS, HELD, LATE_JOINS = range(5)

# Simulator / oracle keywords of every case (tests/test_gpu_partial.py), crash seed 42
KW = dict(rd_seed=7, view_seed=5, init_t0=8, init_seed=11)
T0 = 8
CRASH_SEED = 42
# name: n, v, the crash wave (crash_count nodes after tick crash_tick; T0 = before the first tick), ticks to run, drops
CASES = {
    "n64_v8": dict(n=64, v=8, crash_tick=12, crash_count=4, ticks=36),
    "n300_v16": dict(n=300, v=16, crash_tick=8, crash_count=30, ticks=40),
    "n1000_v32_drops": dict(n=1000, v=32, crash_tick=12, crash_count=20, ticks=24,
                            drops=dict(drop_pct=30, drop_from=5, drop_to=30, drop_seed=42)),
    "n100_v12": dict(n=100, v=12, crash_tick=10, crash_count=5, ticks=24),
    "sparse": dict(n=128, v=4, crash_tick=-1, crash_count=0, ticks=60,
                   drops=dict(drop_pct=90, drop_from=2, drop_to=60, drop_seed=42)),
    # the sparse cluster with a crash inside its TREMOVE sweep, found on the oracle: crashed subjects
    # that were falsely removed at tick 24, before they crashed, and truly after
    "sparse_crash": dict(n=128, v=4, crash_tick=24, crash_count=13, ticks=45,
                         drops=dict(drop_pct=90, drop_from=2, drop_to=60, drop_seed=42)),
}


class Expected:
    def __init__(self, n, rows, r0=0, nrows=None):
        """n subjects; a timeline of `rows` ticks; the observers [r0, r0 + nrows) (default: all)"""
        self.n, self.r0, self.nrows = n, r0, n if nrows is None else nrows
        self.rec = np.zeros(n, dtype=VIEW_DETECT_DTYPE)
        for f in ("fail_tick", "first_removed", "last_removed", "last_held"):
            self.rec[f] = -1
        self.tl = np.zeros((rows, 5), dtype=np.uint64)
        self.crashed = np.zeros(n, dtype=bool)

    def set_failed(self, idx, last_tick):
        """a gm_set_failed(idx) made after tick last_tick ran"""
        idx = np.asarray(idx, dtype=np.int64)
        new = idx[~self.crashed[idx]]
        self.rec["fail_tick"][new] = last_tick
        self.crashed[new] = True

    def tick(self, t, views, events, recorded=True):
        """Tick t ran: `views` uint64 [n][V], every node's final view of it (this object looks at its
        own observers' rows), `events` the whole cluster's records of it. Not recorded: no change."""
        if not recorded:
            return
        obs = np.arange(self.r0, self.r0 + self.nrows)
        crashed = self.crashed  # as tick t saw the flags: the set_failed calls made before it ran
        ev = np.asarray(events, dtype=np.int64).reshape(-1, 4)
        assert (ev[:, 0] == t).all()
        ev = ev[(ev[:, 1] >= self.r0) & (ev[:, 1] < self.r0 + self.nrows)]
        assert not crashed[ev[:, 1]].any(), "a crashed node logged a record"
        sub = ev[:, 3] - 1
        joined, removed = ev[:, 2] == GM_EV_JOINED, ev[:, 2] == GM_EV_REMOVED
        assert (joined | removed).all()
        live = obs[~crashed[obs]]
        ent = np.asarray(views, dtype=np.uint64)[live]
        ids = (ent[ent != 0] >> np.uint64(32)).astype(np.int64) - 1
        held = ids[crashed[ids]]
        late = sub[joined & crashed[sub]]
        rem, frem = sub[removed], sub[removed & ~crashed[sub]]
        self.tl[t] = (joined.sum(), removed.sum(), len(frem), len(held), len(late))
        r = self.rec
        r["held_sum"] += np.bincount(held, minlength=self.n).astype(np.uint64)
        r["last_held"][np.unique(held)] = t
        r["late_joins"] += np.bincount(late, minlength=self.n).astype(np.uint32)
        r["removals"] += np.bincount(rem, minlength=self.n).astype(np.uint32)
        r["false_removals"] += np.bincount(frem, minlength=self.n).astype(np.uint32)
        r["removed_tick_sum"] += (np.bincount(rem, minlength=self.n) * t).astype(np.uint64)
        u = np.unique(rem)
        r["last_removed"][u] = t
        first = r["first_removed"][u]
        r["first_removed"][u] = np.where(first < 0, t, first)


def assert_records(got, want, what):
    assert got.shape == want.shape and got.dtype == VIEW_DETECT_DTYPE, what
    for f in VIEW_DETECT_DTYPE.names:
        bad = np.flatnonzero(got[f] != want[f])
        assert not len(bad), (f"{what}: {f} differs for {len(bad)} subjects, first {bad[0]}: "
                              f"{got[f][bad[0]]} != {want[f][bad[0]]}")


def assert_timeline(got, want, what):
    bad = np.flatnonzero((got != want).any(axis=1))
    assert got.shape == want.shape and not len(bad), (
        f"{what}: timeline differs in {len(bad)} ticks, first {bad[0]}: {got[bad[0]]} != {want[bad[0]]}")


def check_fade(ex, what):
    """the case shows a fade: entries of crashed subjects held in some tick, none in a later one"""
    held = ex.tl[:, HELD]
    some = np.flatnonzero(held)
    assert len(some), f"{what}: no entry of a crashed subject was ever held"
    assert (held[some[0]:] == 0).any(), f"{what}: the crashed subjects never fade from the views"


def oracle_expected(case, crash_set):
    """Expected of a whole-cluster case run on PartialOracle (one crash wave at most, which the oracle
    applies at the end of crash_tick; a crash before the first tick, crash_tick = T0, it cannot run)."""
    import oracle_py
    from view_census_ref import views_from_dump
    c = CASES[case]
    n, v = c["n"], c["v"]
    assert c["crash_tick"] != T0
    ora = oracle_py.PartialOracle(n, v=v, crash_tick=c["crash_tick"], crash_count=c["crash_count"],
                                  crash_seed=CRASH_SEED, **dict(KW, **c.get("drops", {})))
    ex = Expected(n, T0 + 1 + c["ticks"])
    for _ in range(c["ticks"]):
        t = ora.time
        ora.tick()
        views, failed, tt = views_from_dump(ora.dump(), v)
        assert tt == t
        ex.tick(t, views, ora.events())
        if t == c["crash_tick"]:
            ex.set_failed(crash_set(n, c["crash_count"], CRASH_SEED), t)
            assert np.array_equal(failed != 0, ex.crashed)
    return ex
