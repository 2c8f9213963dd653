"""The PARTIAL view census (gm_view_census, include/gm_abi.h) in plain NumPy: the specification
the GPU tests compare against, exactly. A helper, not a test.

Views are what Simulator.read_views() returns: uint64 [rows][V], id << 32 | hb, 0 = empty.
`views_from_dump` brings PartialOracle.dump() (and Simulator.dump_tables()) into that shape."""
import numpy as np

from membership.abi import GM_VIEW_AGES, GM_VIEW_SIZES, VIEW_DTYPE

TFAIL = 5


def expected(views, failed_observers, failed_all, t, n):
    """The census at tick t of `views` [rows][V], the views of the observers whose crash flags are
    failed_observers [rows] (a row shard: its own nodes), over the n subjects of the cluster with
    the crash flags failed_all [n]. Returns (rec, hist, sizes) as gm_view_census defines them."""
    views = np.asarray(views, dtype=np.uint64)
    live = np.asarray(failed_observers) == 0
    crashed = np.asarray(failed_all) != 0
    assert views.ndim == 2 and live.shape == (views.shape[0],) and crashed.shape == (n,)
    ent = views[live]
    held = ent != 0
    sizes = np.bincount(held.sum(axis=1), minlength=GM_VIEW_SIZES).astype(np.uint64)
    assert sizes.shape == (GM_VIEW_SIZES,)
    e = ent[held]
    ids = (e >> np.uint64(32)).astype(np.int64)
    hb = (e & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32).astype(np.int64)
    assert ((ids >= 1) & (ids <= n)).all() and (hb % 2 == 1).all() and (hb <= 2 * t - 1).all()
    age = t - (hb + 1) // 2
    assert (age < GM_VIEW_AGES).all()
    j = ids - 1
    rec = np.zeros(n, dtype=VIEW_DTYPE)
    rec["holders"] = np.bincount(j, minlength=n)
    rec["stale"] = np.bincount(j[age >= TFAIL], minlength=n)
    rec["hb_sum"] = np.bincount(j, weights=hb.astype(np.float64), minlength=n).astype(np.uint64)  # exact: < 2^53
    lo = np.full(n, np.iinfo(np.int64).max)
    hi = np.full(n, -1, dtype=np.int64)
    np.minimum.at(lo, j, hb)
    np.maximum.at(hi, j, hb)
    rec["hb_min"] = np.where(rec["holders"] > 0, lo, -1)
    rec["hb_max"] = hi
    hist = np.bincount(crashed[j].astype(np.int64) * GM_VIEW_AGES + age, minlength=2 * GM_VIEW_AGES)
    return rec, hist.astype(np.uint64).reshape(2, GM_VIEW_AGES), sizes


def views_from_dump(dump, v):
    """(views uint64 [n][v], failed int32 [n], t) of a PARTIAL dump: one line per node,
    "t i inited inGroup failed heartbeat count id:hb:ts ..."."""
    lines = dump.decode().splitlines()
    views = np.zeros((len(lines), v), dtype=np.uint64)
    failed = np.zeros(len(lines), dtype=np.int32)
    t = None
    for ln in lines:
        f = ln.split()
        t, i, cnt = int(f[0]), int(f[1]), int(f[6])
        failed[i] = int(f[4])
        assert len(f) == 7 + cnt and cnt <= v
        for k, ent in enumerate(f[7:]):
            node, hb, ts = (int(x) for x in ent.split(":"))
            assert ts == (hb + 1) // 2
            views[i, k] = (node << 32) | (hb & 0xFFFFFFFF)
    return views, failed, t


def assert_census(got, want, what):
    (rec, hist, sizes), (erec, ehist, esizes) = got, want
    assert rec.shape == erec.shape, what
    for f in VIEW_DTYPE.names:
        bad = np.flatnonzero(rec[f] != erec[f])
        assert not len(bad), (f"{what}: {f} differs for {len(bad)} subjects, first {bad[0]}: "
                              f"{rec[f][bad[0]]} != {erec[f][bad[0]]}")
    assert np.array_equal(hist, ehist), f"{what}: hist differs\n{hist}\n{ehist}"
    assert np.array_equal(sizes, esizes), f"{what}: sizes differ\n{sizes}\n{esizes}"


# ---- the cases of the census tests: Simulator / oracle keywords and what each case must contain,
# asserted from the expected arrays (so the conditions can be checked against the oracle alone)
KW = dict(rd_seed=7, view_seed=5, init_t0=8, init_seed=11)
CRASH_CASES = [(64, 8, 2), (300, 16, 6), (1000, 32, 20)]               # (n, v, crashed) after tick 12
# The census ticks of a crash case: as created, one tick after the crash, and T = 16, where the
# oracle's views hold no crashed node any more at N = 64 and 300. At N = 1000 one entry is left at
# T = 16 (oracle: 592, 507, 88, 1, 0 entries of crashed nodes at T = 13..17), so that case adds T = 17.
FADED_AT = {64: 16, 300: 16, 1000: 17}
CRASH_TICKS = {64: (8, 9, 13, 16), 300: (8, 13, 16), 1000: (8, 13, 16, 17)}
SPARSE = dict(n=128, v=4, drop_pct=90, drop_from=2, drop_to=60, drop_seed=42)
STALE_CRASHED = dict(n=400, v=32, crash_tick=10, crash_count=8, drop_pct=30, drop_from=5, drop_to=30, drop_seed=42)


def oracle_census(ora, v):
    """(census, views, failed, t) of a PartialOracle's state"""
    views, failed, t = views_from_dump(ora.dump(), v)
    return expected(views, failed, failed, t, ora.n), views, failed, t


def check_crash_case(t, n, v, census, failed):
    rec, hist, sizes = census
    crashed = failed != 0
    if t <= 12:
        assert not crashed.any() and not hist[1].any() and sizes.sum() == n
    if t == 9 and (n, v) == (64, 8):  # heavy contention: every atomic of the launch lands on 64 records
        assert rec["stale"].sum() > 0
    if t == 13:  # one tick after the crash: everybody the crashed nodes were held by still holds them
        assert crashed.any() and (rec["holders"][crashed] > 0).all()
        assert hist[1].sum() == rec["holders"][crashed].sum() > 0
        assert hist[1, 1:4].sum() == hist[1].sum(), "ages of the crashed class outside 1..3"
    if t == 16 and n == 1000:  # the oracle's last entry of a crashed node, of age 4; gone at T = 17
        assert rec["holders"][crashed].sum() == 1 == hist[1, 4] == hist[1].sum()
    if t == FADED_AT[n]:  # eviction keeps the largest heartbeats: the crashed nodes are gone long before TREMOVE
        assert crashed.any() and not rec["holders"][crashed].any() and not hist[1].any()
        assert (rec["hb_min"][crashed] == -1).all() and (rec["hb_max"][crashed] == -1).all()


def check_sparse_case(t, census, views, failed):
    rec, hist, sizes = census
    n = len(rec)
    assert not failed.any()
    if t == 20:
        assert _max_age(hist) == 16 and rec["stale"].sum() > 0
    if t == 30:
        assert sizes[1] > 0 and sizes[2] > 0 and sizes[3] > 0
        assert (rec["holders"] == 1).sum() > n // 2, "fewer than half of the live subjects are orphans"
    if t == 40:
        assert sizes[1] == n and (rec["holders"] == 1).all()
        assert ((views[:, 0] >> np.uint64(32)) == np.arange(1, n + 1, dtype=np.uint64)).all() and not views[:, 1:].any()


def check_stale_crashed_case(t, census, failed):
    rec, hist, sizes = census
    if t == 12:
        assert rec["stale"][failed != 0].sum() > 0 and hist[1, TFAIL:].sum() == rec["stale"][failed != 0].sum()


def _max_age(hist):
    return int(np.flatnonzero(hist.sum(axis=0))[-1])
