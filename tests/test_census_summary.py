"""membership.census on hand-made census arrays (CPU): summarize_census and merge_shards."""
import numpy as np
import pytest

from membership.abi import CENSUS_DTYPE, GM_CENSUS_AGES, GM_CENSUS_LAGS
from membership.census import BYTE_LAG_MAX, ERR_LAG_MAX, merge_shards, summarize_census

T = 100


def _build(cells, failed):
    """cells: (observer, subject, lag, age) of live observers, hb = 2T - 1 - 2 lag (odd, as in a warm
    cluster), ts = T - age; failed: per node. Returns (rec, hist) as gm_census defines them."""
    rec = np.zeros(len(failed), dtype=CENSUS_DTYPE)
    for f in ("hb_min", "hb_max", "ts_min", "ts_max"):
        rec[f] = -1
    hist = np.zeros((2, GM_CENSUS_LAGS, GM_CENSUS_AGES), dtype=np.uint64)
    for _, s, lag, age in cells:
        hb, ts = 2 * T - 1 - 2 * lag, T - age
        r = rec[s]
        r["hb_min"] = hb if r["holders"] == 0 else min(r["hb_min"], hb)
        r["ts_min"] = ts if r["holders"] == 0 else min(r["ts_min"], ts)
        r["hb_max"], r["ts_max"] = max(r["hb_max"], hb), max(r["ts_max"], ts)
        r["holders"] += 1
        r["stale"] += age >= 5
        r["hb_sum"] += hb
        r["ts_sum"] += ts
        hist[int(failed[s] != 0), min(lag, GM_CENSUS_LAGS - 1), age] += 1
    return rec, hist


# 5 nodes; node 4 crashed 8 ticks ago, node 3 crashed long ago and is gone from every view
FAILED = np.array([0, 0, 0, 1, 1])
CELLS = ([(o, o, 0, 0) for o in range(3)]                      # own entries
         + [(0, 1, 2, 1), (0, 2, 3, 1), (1, 0, 2, 0), (1, 2, 9, 4), (2, 0, 4, 2)]   # (2, 1) is missing
         + [(o, 4, 8 + o, 8) for o in range(3)])                 # the crashed subject, stale everywhere


def test_summary_of_a_small_cluster():
    rec, hist = _build(CELLS, FAILED)
    s = summarize_census(rec, hist, FAILED, T)
    assert s["live_observers"] == 3 and s["t"] == T
    assert s["coverage"] == {"min": pytest.approx(2 / 3), "mean": pytest.approx(8 / 9)}
    assert s["lag"]["live"] == [3, 0, 2, 1, 1, 0, 0, 0, 0, 1] and s["lag"]["crashed"] == [0] * 8 + [1, 1, 1]
    assert s["age"]["live"] == [4, 2, 1, 0, 1] and s["age"]["crashed"] == [0] * 8 + [3]
    assert s["l0"]["live"] == {0: 3, 1: 1, 2: 3, 5: 1} and s["l0"]["crashed"] == {0: 1, 1: 1, 2: 1}
    assert s["clipped"] == {"live": 0, "crashed": 0}
    assert s["max_lag"] == {"live": 9, "crashed": 10}
    # a crashed subject is suspected by all its holders; the long-gone one has faded
    assert s["suspected_by"] == {"subjects": 2, "faded": 1, "min": 0, "mean": 1.5, "max": 3}
    assert rec["stale"][4] == rec["holders"][4] == 3
    assert s["headroom"] == {"byte_lag": BYTE_LAG_MAX - 9, "err_lag": ERR_LAG_MAX / 10}


def test_empty_subjects_report_minus_one():
    rec, hist = _build(CELLS, FAILED)
    assert rec["holders"][3] == 0
    assert (rec["hb_min"][3], rec["hb_max"][3], rec["ts_min"][3], rec["ts_max"][3]) == (-1, -1, -1, -1)
    s = summarize_census(rec, hist, FAILED, T)  # and the summary does not read their -1 as a heartbeat
    assert s["max_lag"]["crashed"] == 10


def test_clip_bin():
    cells = [c for c in CELLS if (c[0], c[1]) not in ((0, 4), (1, 1))] + [(0, 4, 70, 3), (1, 1, 90, 2)]
    rec, hist = _build(cells, FAILED)
    assert hist[0, GM_CENSUS_LAGS - 1, 2] == 1 and hist[1, GM_CENSUS_LAGS - 1, 3] == 1
    s = summarize_census(rec, hist, FAILED, T)
    assert s["clipped"] == {"live": 1, "crashed": 1}
    assert len(s["lag"]["live"]) == GM_CENSUS_LAGS and s["lag"]["live"][-1] == 1
    assert s["max_lag"] == {"live": 90, "crashed": 70}  # exact, from the records
    assert 90 - 2 not in s["l0"]["live"]  # clipped cells have no L0
    assert s["headroom"]["byte_lag"] == BYTE_LAG_MAX - 90 and s["headroom"]["err_lag"] == ERR_LAG_MAX / 90


def test_nothing_crashed_and_nobody_alive():
    failed = np.zeros(3, dtype=np.int32)
    rec, hist = _build([(o, o, 0, 0) for o in range(3)], failed)
    s = summarize_census(rec, hist, failed, T)
    assert s["suspected_by"] == {"subjects": 0, "faded": 0, "min": None, "mean": None, "max": None}
    assert s["coverage"] == {"min": pytest.approx(1 / 3), "mean": pytest.approx(1 / 3)}
    assert s["max_lag"] == {"live": 0, "crashed": None} and s["headroom"] == {"byte_lag": BYTE_LAG_MAX, "err_lag": None}
    dead = np.ones(3, dtype=np.int32)
    rec, hist = _build([], dead)
    s = summarize_census(rec, hist, dead, T)
    assert s["live_observers"] == 0 and s["coverage"] == {"min": None, "mean": None}


def test_rejects_mismatched_arrays():
    rec, hist = _build(CELLS, FAILED)
    with pytest.raises(ValueError):
        summarize_census(rec, hist, FAILED[:4], T)
    hist[0, 0, 0] += 1
    with pytest.raises(ValueError):
        summarize_census(rec, hist, FAILED, T)


def test_merge_shards():
    rec, hist = _build(CELLS, FAILED)
    parts = []
    for c0, c1 in ((0, 2), (2, 3), (3, 5)):
        h = np.zeros_like(hist)
        for _, s, lag, age in CELLS:
            if c0 <= s < c1:
                h[int(FAILED[s] != 0), lag, age] += 1
        parts.append((c0, rec[c0:c1].copy(), h))
    mrec, mhist = merge_shards([parts[2], parts[0], parts[1]])  # any order
    assert mrec.dtype == CENSUS_DTYPE and np.array_equal(mrec, rec)
    assert mhist.dtype == np.uint64 and np.array_equal(mhist, hist)
    assert summarize_census(mrec, mhist, FAILED, T) == summarize_census(rec, hist, FAILED, T)
    with pytest.raises(ValueError):
        merge_shards([parts[0], parts[2]])  # a shard is missing
