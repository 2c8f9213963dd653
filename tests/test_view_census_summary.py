"""membership.views (summarize_views, merge_view_shards) on censuses computed by view_census_ref
from PartialOracle runs -- no GPU. This also pins the helper the GPU tests trust
(tests/test_gpu_view_census.py): the reference census against figures taken directly from the
oracle's views, and the conditions every case of the GPU file asserts."""
import numpy as np
import pytest

import oracle_py
import view_census_ref as ref
from membership import merge_view_shards, summarize_views
from membership.abi import GM_VIEW_AGES, GM_VIEW_SIZES, VIEW_DTYPE


def _run(n, v, ticks, **kw):
    """{T: (census, views, failed, T)} of an oracle run at the ticks asked for (8 = as created)"""
    ora = oracle_py.PartialOracle(n, v=v, **dict(ref.KW, **kw))
    out = {}
    while True:
        t = ora.time - 1
        if t in ticks:
            out[t] = ref.oracle_census(ora, v)
            assert out[t][3] == t
        if t >= max(ticks):
            return out
        ora.tick()


@pytest.fixture(scope="module")
def sparse():
    c = ref.SPARSE
    return _run(c["n"], c["v"], (20, 30, 40), drop_pct=c["drop_pct"], drop_from=c["drop_from"], drop_to=c["drop_to"],
                drop_seed=c["drop_seed"])


@pytest.fixture(scope="module")
def crash1000():
    return _run(1000, 32, ref.CRASH_TICKS[1000], crash_tick=12, crash_count=20, crash_seed=42)


def test_reference_census_of_a_hand_made_state():
    """expected() against a census worked out by hand: 4 nodes, V = 3, T = 10; node 2 crashed (its
    view is frozen), node 3 is held by nobody else"""
    def ent(node, hb):
        return (node << 32) | hb
    views = np.array([[ent(1, 19), ent(2, 9), ent(4, 17)],
                      [ent(1, 1), ent(2, 3), ent(3, 5)],      # frozen: contributes nothing
                      [ent(3, 19), 0, 0],
                      [ent(1, 15), ent(2, 11), ent(4, 19)]], dtype=np.uint64)
    failed = np.array([0, 1, 0, 0])
    rec, hist, sizes = ref.expected(views, failed, failed, 10, 4)
    assert rec["holders"].tolist() == [2, 2, 1, 2] and rec["stale"].tolist() == [0, 1, 0, 0]
    assert rec["hb_min"].tolist() == [15, 9, 19, 17] and rec["hb_max"].tolist() == [19, 11, 19, 19]
    assert rec["hb_sum"].tolist() == [34, 20, 19, 36]
    assert {(k, a): int(hist[k, a]) for k, a in zip(*np.nonzero(hist))} == {(0, 0): 3, (0, 1): 1, (0, 2): 1, (1, 4): 1, (1, 5): 1}
    assert {s: int(sizes[s]) for s in np.flatnonzero(sizes)} == {1: 1, 3: 2}
    s = summarize_views(rec, hist, sizes, failed, 10, 3)
    assert s["live_observers"] == 3 and s["orphans"] == 1
    assert s["view_size"] == {"min": 1, "mean": 7 / 3, "full": 2 / 3}
    assert s["in_degree"] == {"min": 0, "mean": 2 / 3, "max": 1, "hist": [1, 2]}
    assert s["age"] == {"live": [3, 1, 1], "crashed": [0, 0, 0, 0, 1, 1]}
    assert s["stale"] == {"live": 0, "crashed": 1} and s["max_lag"] == {"live": 2, "crashed": 5}
    assert s["crashed"] == {"subjects": 1, "held": 1, "entries": 2}


def test_dump_parser_matches_the_oracle():
    ora = oracle_py.PartialOracle(64, v=8, **ref.KW)
    views, failed, t = ref.views_from_dump(ora.dump(), 8)
    assert t == 8 and views.shape == (64, 8) and not failed.any()
    ids = (views >> np.uint64(32)).astype(np.int64)
    assert (ids > 0).all(), "created views are full"
    assert (np.diff(ids, axis=1) > 0).all(), "ascending ids"
    assert ((ids == np.arange(1, 65)[:, None]).sum(axis=1) == 1).all(), "every node holds itself"


@pytest.mark.parametrize("n,v,crashed", ref.CRASH_CASES)
def test_crash_and_fade(n, v, crashed, crash1000):
    ticks = ref.CRASH_TICKS[n]
    runs = crash1000 if n == 1000 else _run(n, v, ticks, crash_tick=12, crash_count=crashed, crash_seed=42)
    for t in ticks:
        census, views, failed, _ = runs[t]
        assert int((failed != 0).sum()) == (crashed if t > 12 else 0)
        ref.check_crash_case(t, n, v, census, failed)
        s = summarize_views(*census, failed, t, v)
        assert s["live_observers"] == n - int((failed != 0).sum())
        assert s["crashed"]["held"] == (crashed if t == 13 else 1 if (n, t) == (1000, 16) else 0)
        if t == ref.FADED_AT[n]:
            assert s["max_lag"]["crashed"] is None and s["age"]["crashed"] == []
    if (n, v) == (64, 8):
        assert int(runs[9][0][0]["stale"].sum()) == 111


def test_sparse_views(sparse):
    for t in (20, 30, 40):
        census, views, failed, _ = sparse[t]
        ref.check_sparse_case(t, census, views, failed)
    census, views, failed, _ = sparse[30]
    s = summarize_views(*census, failed, 30, 4)
    assert s["orphans"] == 99 and s["live_observers"] == 128
    assert {k: int(c) for k, c in enumerate(census[2]) if c} == {1: 95, 2: 30, 3: 3}
    # the same quantities taken directly from the views
    ids = (views >> np.uint64(32)).astype(np.int64)
    others = np.bincount(ids[ids > 0] - 1, minlength=128) - 1
    assert s["orphans"] == int((others == 0).sum()) and s["in_degree"]["max"] == int(others.max())
    cnt = (views != 0).sum(axis=1)
    assert s["view_size"] == {"min": int(cnt.min()), "mean": float(cnt.mean()), "full": float((cnt == 4).mean())}
    assert summarize_views(*sparse[40][0], sparse[40][2], 40, 4)["orphans"] == 128


def test_stale_entries_of_crashed_subjects():
    c = dict(ref.STALE_CRASHED)
    n, v = c.pop("n"), c.pop("v")
    census, views, failed, t = _run(n, v, (12,), **c)[12]
    ref.check_stale_crashed_case(12, census, failed)
    s = summarize_views(*census, failed, 12, v)
    assert s["stale"]["crashed"] == 7 and s["max_lag"]["crashed"] == 5
    assert sorted(np.flatnonzero(census[1][1]).tolist()) == [2, 3, 5]
    assert s["crashed"]["subjects"] == 8


def test_sums_rule(sparse):
    (rec, hist, sizes), _, failed, _ = sparse[30]
    summarize_views(rec, hist, sizes, failed, 30, 4)
    bad = hist.copy()
    bad[0, 3] += 1
    with pytest.raises(ValueError):
        summarize_views(rec, bad, sizes, failed, 30, 4)
    bad = sizes.copy()
    bad[2], bad[1] = bad[2] - 1, bad[1] + 1
    with pytest.raises(ValueError):
        summarize_views(rec, hist, bad, failed, 30, 4)
    with pytest.raises(ValueError):
        summarize_views(rec[:-1], hist, sizes, failed, 30, 4)


def test_merge_of_row_ranges_equals_the_whole(crash1000):
    for tick in (13, 16):
        whole, views, failed, t = crash1000[tick]
        parts = [ref.expected(views[a:b], failed[a:b], failed, t, 1000) for a, b in ((0, 400), (400, 1000))]
        if tick == 16:  # a subject held in one range only (the other range's -1 must not win the minimum), and by neither
            h0, h1 = parts[0][0]["holders"], parts[1][0]["holders"]
            assert ((h0 == 0) != (h1 == 0)).any() and ((h0 == 0) & (h1 == 0)).any()
        ref.assert_census(merge_view_shards(parts), whole, "merged row ranges")
        ref.assert_census(merge_view_shards(parts[::-1]), whole, "merged row ranges, other order")
    assert merge_view_shards(parts)[0].dtype == VIEW_DTYPE
    assert merge_view_shards(parts)[1].shape == (2, GM_VIEW_AGES) and merge_view_shards(parts)[2].shape == (GM_VIEW_SIZES,)


def test_merge_rejects_parts_of_different_lengths(crash1000):
    rec, hist, sizes = crash1000[13][0]
    with pytest.raises(ValueError):
        merge_view_shards([(rec, hist, sizes), (rec[:400], hist, sizes)])
