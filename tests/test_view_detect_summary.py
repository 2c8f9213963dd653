"""CPU: the host side of the PARTIAL detection recorder -- merge_view_detect_shards and
summarize_view_detect on hand-made records -- and the cases of tests/test_gpu_view_detect.py on the
oracle: view_detect_ref.Expected over PartialOracle's views and events shows the properties each GPU
case is there for (the oracle runs one crash wave at the end of a tick, so the case that crashes before
the first tick and the two-wave case are checked on the GPU alone)."""
import numpy as np
import pytest

import oracle_py
import view_detect_ref as ref
from membership import merge_view_detect_shards, summarize_view_detect
from membership.abi import GM_VIEW_DETECT_COLS, VIEW_DETECT_DTYPE
from view_detect_ref import FALSE_REMOVALS, HELD, JOINS, LATE_JOINS, REMOVALS


def _recs(n):
    r = np.zeros(n, dtype=VIEW_DETECT_DTYPE)
    for f in ("fail_tick", "first_removed", "last_removed", "last_held"):
        r[f] = -1
    return r


def test_record_layout():
    assert VIEW_DETECT_DTYPE.itemsize == 48 and GM_VIEW_DETECT_COLS == 5
    assert [VIEW_DETECT_DTYPE.fields[f][1] for f in VIEW_DETECT_DTYPE.names] == [0, 4, 8, 12, 16, 20, 24, 28, 32, 40]


def test_merge_adds_and_combines():
    a, b, c = _recs(4), _recs(4), _recs(4)
    for p in (a, b, c):
        p["fail_tick"] = [12, -1, 12, -1]
    # subject 0: removed on a and c only; subject 1: on nobody; subject 2: on all; subject 3: on b
    a["first_removed"], a["last_removed"], a["removals"] = [20, -1, 19, -1], [22, -1, 19, -1], [3, 0, 1, 0]
    b["first_removed"], b["last_removed"], b["removals"] = [-1, -1, 17, 30], [-1, -1, 25, 30], [0, 0, 4, 1]
    c["first_removed"], c["last_removed"], c["removals"] = [18, -1, 21, -1], [18, -1, 21, -1], [1, 0, 1, 0]
    b["false_removals"] = [0, 0, 0, 1]
    a["removed_tick_sum"], b["removed_tick_sum"], c["removed_tick_sum"] = [63, 0, 19, 0], [0, 0, 80, 30], [18, 0, 21, 0]
    a["last_held"], b["last_held"], c["last_held"] = [14, -1, -1, -1], [13, -1, 15, -1], [-1, -1, 13, -1]
    a["held_sum"], b["held_sum"], c["held_sum"] = [5, 0, 0, 0], [2, 0, 7, 0], [0, 0, 1, 0]
    a["late_joins"], b["late_joins"] = [1, 0, 0, 0], [1, 0, 2, 0]
    m = merge_view_detect_shards([a, b, c])
    assert m["fail_tick"].tolist() == [12, -1, 12, -1]
    assert m["first_removed"].tolist() == [18, -1, 17, 30], "the minimum over the parts that have one"
    assert m["last_removed"].tolist() == [22, -1, 25, 30]
    assert m["removals"].tolist() == [4, 0, 6, 1] and m["false_removals"].tolist() == [0, 0, 0, 1]
    assert m["removed_tick_sum"].tolist() == [81, 0, 120, 30]
    assert m["last_held"].tolist() == [14, -1, 15, -1] and m["held_sum"].tolist() == [7, 0, 8, 0]
    assert m["late_joins"].tolist() == [2, 0, 2, 0] and not m["reserved"].any()
    assert a["removals"].tolist() == [3, 0, 1, 0], "the parts are not modified"
    one = merge_view_detect_shards([b])
    assert np.array_equal(one, b) and one is not b


def test_merge_rejects_disagreeing_parts():
    a, b = _recs(3), _recs(3)
    a["fail_tick"] = [12, -1, -1]
    with pytest.raises(ValueError, match="fail_tick"):
        merge_view_detect_shards([a, b])
    with pytest.raises(ValueError):
        merge_view_detect_shards([a, _recs(4)])
    with pytest.raises(ValueError):
        merge_view_detect_shards([])


def test_summary_extinct_and_latencies():
    r = _recs(6)
    crashed = np.array([1, 1, 1, 1, 0, 0], dtype=bool)
    r["fail_tick"] = [12, 12, 20, 12, -1, -1]
    r["last_held"] = [14, 16, 29, -1, -1, -1]    # subject 3 crashed and was never held
    r["held_sum"] = [9, 20, 40, 0, 0, 0]
    r["late_joins"] = [2, 5, 0, 0, 0, 0]
    r["removals"] = [0, 1, 3, 0, 2, 0]
    r["false_removals"] = [0, 0, 2, 0, 2, 0]     # subject 2 was removed twice before it crashed
    r["last_removed"] = [-1, 18, 27, -1, 15, -1]
    tl = np.zeros((30, 5), dtype=np.uint64)
    tl[13:30, HELD] = 3
    s = summarize_view_detect(r, crashed, tl)
    assert s["extinct"] == 0.75, "last tick 29: subject 2 is still held"
    assert s["forget_latency"] == {"min": 3, "mean": (3 + 5 + 10) / 3, "max": 10}
    assert s["stale_observer_ticks"] == 69 and s["late_joins"] == 7 and s["removals"] == 6
    assert s["false_removals"] == {"total": 4, "crashed_later": 2, "never_crashed": 2}
    assert s["fade"].tolist() == [0] * 13 + [3] * 17
    longer = np.zeros((31, 5), dtype=np.uint64)
    assert summarize_view_detect(r, crashed, longer)["extinct"] == 1.0
    # without a timeline the last tick is the latest one a record names: 29
    s = summarize_view_detect(r, crashed)
    assert s["extinct"] == 0.75 and s["fade"] is None


def test_summary_without_a_crash():
    r = _recs(5)
    r["removals"], r["false_removals"] = [1, 0, 0, 2, 0], [1, 0, 0, 2, 0]
    s = summarize_view_detect(r, np.zeros(5, dtype=bool), np.zeros((12, 5), dtype=np.uint64))
    assert s["extinct"] == 1.0 and s["forget_latency"] == {"min": None, "mean": None, "max": None}
    assert s["stale_observer_ticks"] == 0 and s["late_joins"] == 0
    assert s["false_removals"] == {"total": 3, "crashed_later": 0, "never_crashed": 3}
    assert not s["fade"].any()


def test_summary_rejects_bad_shapes():
    with pytest.raises(ValueError):
        summarize_view_detect(_recs(4), np.zeros(5, dtype=bool))
    with pytest.raises(ValueError):
        summarize_view_detect(_recs(4), np.zeros(4, dtype=bool), np.zeros((10, 3), dtype=np.uint64))


# ---- the GPU cases on the oracle: each shows what it is there for
@pytest.fixture(scope="module")
def oracle_cases():
    return {name: ref.oracle_expected(name, oracle_py.crash_set)
            for name, c in ref.CASES.items() if c["crash_tick"] != ref.T0}


@pytest.mark.parametrize("case", ["n64_v8", "n1000_v32_drops", "n100_v12", "sparse_crash"])
def test_oracle_crash_cases_fade(oracle_cases, case):
    ex, c = oracle_cases[case], ref.CASES[case]
    ref.check_fade(ex, case)
    tl, crashed = ex.tl, ex.crashed
    assert crashed.sum() == c["crash_count"] and (ex.rec["fail_tick"][crashed] == c["crash_tick"]).all()
    assert not tl[:c["crash_tick"] + 1, HELD].any() and tl[c["crash_tick"] + 1, HELD] > 0
    assert tl[:, HELD].sum() == ex.rec["held_sum"].sum() and not ex.rec["held_sum"][~crashed].any()
    assert tl[:, LATE_JOINS].sum() == ex.rec["late_joins"].sum() and (tl[:, LATE_JOINS] <= tl[:, HELD]).all()
    assert tl[ref.T0 + 2, JOINS] > 0 and not tl[:ref.T0 + 1].any()
    s = summarize_view_detect(ex.rec, crashed, tl)
    assert s["extinct"] == 1.0 and s["forget_latency"]["min"] >= 1


def test_oracle_case_properties(oracle_cases):
    assert oracle_cases["n64_v8"].tl[13, HELD] > 4 * 4
    assert oracle_cases["n1000_v32_drops"].tl[:, LATE_JOINS].sum() > 0
    tl = oracle_cases["sparse"].tl
    assert tl[:, REMOVALS].sum() > 0 and np.array_equal(tl[:, REMOVALS], tl[:, FALSE_REMOVALS]) and not tl[:, HELD].any()
    assert (oracle_cases["sparse"].rec["removals"] > 1).any()
    ex = oracle_cases["sparse_crash"]
    r = ex.rec[ex.crashed]
    both = (r["false_removals"] > 0) & (r["removals"] > r["false_removals"])
    assert both.any() and (r["first_removed"][both] <= r["fail_tick"][both]).all()
    # clusters without message loss starve no view: no TREMOVE removal, so none before a crash either
    for case in ("n64_v8", "n100_v12"):
        assert not oracle_cases[case].tl[:, REMOVALS].any()
