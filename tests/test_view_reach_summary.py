"""membership.reach (summarize_reach) on walks computed by view_reach_ref -- no GPU. This also pins the
helper the GPU tests trust (tests/test_gpu_view_reach.py): the reference on hand-made graphs with known
distances, and, on PartialOracle states, the conditions every case of the GPU file asserts, so the
GPU cases are known to be non-trivial before a GPU sees them."""
import numpy as np
import pytest

import oracle_py
import view_reach_ref as ref
from membership import summarize_reach
from membership.abi import GM_REACH_SOURCES, GM_VIEW_HOPS


def _walks(views, failed, sources, max_hops=GM_VIEW_HOPS):
    return tuple(ref.expected(views, failed, sources, d, max_hops) for d in ("out", "in"))


def _graph(adj, n, v=6, crashed=()):
    s = ref.graph_state(n, v, adj, crashed)
    return s["views"], s["failed"]


def _col(exp, k):
    c = exp[0][:, k].astype(int)
    return c[:int(np.flatnonzero(c)[-1]) + 1].tolist() if c.any() else []


# ------------------------------------------------------------------ the reference on hand-made graphs
def test_chain():
    views, failed = _graph(ref.chain_graph(10), 12)  # nodes 10, 11: alone
    out, inn = _walks(views, failed, [0, 9, 4, 11])
    assert [_col(out, k) for k in range(4)] == [[1] * 10, [1], [1] * 6, [1]]
    assert [_col(inn, k) for k in range(4)] == [[1], [1] * 10, [1] * 5, [1]]
    assert out[2] == [12, 9, 0, 4] and inn[2] == [12, 9, 0, 4]
    assert out[1].tolist() == [1, 1, 1, 1, 5, 5, 5, 5, 5, 7, 0, 8]
    dist = ref.levels(views, failed, [0], "out")[0]
    assert dist.tolist() == list(range(10)) + [-1, -1]
    # max_hops cuts the walk: levels 0 .. 3, the fourth row non-empty -> stopped
    cut = ref.expected(views, failed, [0, 9], "out", 4)
    assert _col(cut, 0) == [1, 1, 1, 1] and _col(cut, 1) == [1] and cut[2] == [12, 3, 1, 2]
    assert cut[1].tolist() == [1, 1, 1, 1, 0, 0, 0, 0, 0, 2, 0, 0]
    one = ref.expected(views, failed, [0, 9], "out", 1)  # the sources only
    assert one[2] == [12, 0, 1, 2] and one[1].tolist() == [1] + [0] * 8 + [2, 0, 0]
    s = summarize_reach(ref.as_walk(out, 4), ref.as_walk(inn, 4))
    assert s["strongly_connected"] is False and s["stopped"] is False and s["live"] == 12
    assert s["out"]["sources"][0] == {"live": True, "reached": 10, "unreached": 2, "eccentricity": 9, "mean_distance": 5.0}
    assert s["in"]["sources"][0] == {"live": True, "reached": 1, "unreached": 11, "eccentricity": 0, "mean_distance": None}
    assert s["out"]["hop_histogram"] == [4, 2, 2, 2, 2, 2, 1, 1, 1, 1] and s["out"]["hops"] == 9
    assert summarize_reach(ref.as_walk(cut, 2))["stopped"] is True


def test_one_way_bridge():
    k = 4
    views, failed = _graph(ref.bridge_graph(k), 2 * k)
    out, inn = _walks(views, failed, [0, 1, k, k + 1])
    assert [_col(out, j) for j in range(4)] == [[1, 4, 3], [1, 3, 1, 3], [1, 3], [1, 3]]
    assert [_col(inn, j) for j in range(4)] == [[1, 3], [1, 3], [1, 4, 3], [1, 3, 1, 3]]
    s = summarize_reach(ref.as_walk(out, 4), ref.as_walk(inn, 4))
    assert s["strongly_connected"] is False  # node 0 reaches everybody and is reached by its own clique only
    assert [x["unreached"] for x in s["out"]["sources"]] == [0, 0, 4, 4]
    assert [x["unreached"] for x in s["in"]["sources"]] == [4, 4, 0, 0]
    assert s["out"]["sources"][1]["mean_distance"] == (3 * 1 + 1 * 2 + 3 * 3) / 7
    # with the edge back the same walks prove strong connectivity
    adj = ref.bridge_graph(k)
    adj[k + 1] = adj[k + 1] + [1]
    views, failed = _graph(adj, 2 * k)
    out, inn = _walks(views, failed, [0, 1, k, k + 1])
    assert ref.proves_strongly_connected(out, inn)
    s = summarize_reach(ref.as_walk(out, 4), ref.as_walk(inn, 4))
    assert s["strongly_connected"] is True and summarize_reach(ref.as_walk(out, 4))["strongly_connected"] is None


def test_two_islands():
    adj = {0: [1], 1: [2], 2: [0], 3: [4], 4: [3]}
    views, failed = _graph(adj, 5)
    out, inn = _walks(views, failed, [0, 3, 3])  # node 3 named twice: the two columns are equal
    assert [_col(out, j) for j in range(3)] == [[1, 1, 1], [1, 1], [1, 1]]
    assert [_col(inn, j) for j in range(3)] == [[1, 1, 1], [1, 1], [1, 1]]
    assert out[1].tolist() == [1, 1, 1, 6, 6]
    s = summarize_reach(ref.as_walk(out, 3), ref.as_walk(inn, 3))
    assert s["strongly_connected"] is False and [x["unreached"] for x in s["out"]["sources"]] == [2, 3, 3]


def test_crashed_cut_vertex_and_crashed_source():
    views, failed = _graph(ref.path_graph(7), 7, crashed=[3])
    out, inn = _walks(views, failed, [0, 3, 6])
    assert [_col(out, j) for j in range(3)] == [[1, 1, 1], [], [1, 1, 1]]
    assert [_col(inn, j) for j in range(3)] == [[1, 1, 1], [], [1, 1, 1]]
    assert out[2] == [6, 2, 0, 2] and out[1].tolist() == [1, 1, 1, 0, 4, 4, 4]
    s = summarize_reach(ref.as_walk(out, 3), ref.as_walk(inn, 3))
    assert s["live"] == 6 and s["live_sources"] == 2 and s["strongly_connected"] is False
    assert s["out"]["sources"][1] == {"live": False, "reached": 0, "unreached": None, "eccentricity": None,
                                      "mean_distance": None}
    assert s["out"]["sources"][0]["unreached"] == 3
    # the same path with nobody crashed is strongly connected; a crashed node's frozen view is no edge
    views, failed = _graph(ref.path_graph(7), 7)
    out, inn = _walks(views, failed, [0, 3, 6])
    assert summarize_reach(ref.as_walk(out, 3), ref.as_walk(inn, 3))["strongly_connected"] is True
    only = ref.expected(views, np.array([1, 1, 1, 1, 1, 1, 0]), [6, 0], "out", GM_VIEW_HOPS)
    assert _col(only, 0) == [1] and _col(only, 1) == [] and only[2] == [1, 0, 0, 1]
    none = summarize_reach(ref.as_walk(ref.expected(views, np.ones(7, dtype=int), [2], "out", 5), 1))
    assert none["live_sources"] == 0 and none["strongly_connected"] is None and none["out"]["hop_histogram"] == []


def test_summary_rejects_walks_that_do_not_belong_together():
    views, failed = _graph(ref.path_graph(7), 7)
    out, inn = _walks(views, failed, [0, 3])
    other = ref.expected(views, failed, [0, 3, 5], "in", GM_VIEW_HOPS)
    with pytest.raises(ValueError):
        summarize_reach(ref.as_walk(out, 2), ref.as_walk(other, 3))
    bad = ref.as_walk(out, 2)
    bad["counts"][1, 0] += 7
    with pytest.raises(ValueError):
        summarize_reach(bad)


def test_sources_for():
    failed = np.zeros(300, dtype=int)
    failed[[7, 100, 250]] = 1
    src = ref.sources_for(300, failed)
    assert len(src) == GM_REACH_SOURCES and src[0] == 0 and src[1] == 299 and failed[src[2]] and src[-1] == src[3]
    assert np.array_equal(src, ref.sources_for(300, failed)) and len(ref.sources_for(300, failed, 1)) == 1
    assert np.array_equal(ref.sources_for(300, failed, 37)[:3], src[:3])


# ------------------------------------------------------------------ the GPU cases on the oracle's states
def _oracle_states(n, v, ticks, **kw):
    """{T: (views, failed)} of an oracle run at the ticks asked for (8 = as created)"""
    ora = oracle_py.PartialOracle(n, v=v, **dict(ref.KW, **kw))
    out = {}
    while True:
        t = ora.time - 1
        if t in ticks:
            out[t] = (ora.views(), ora.nodes()[:, 2].copy())
        if t >= max(ticks):
            return out
        ora.tick()


def _case(views, failed):
    src = ref.sources_for(len(failed), failed)
    return _walks(views, failed, src) + (src,)


@pytest.mark.parametrize("n,v", ref.CRASH_CASES)
def test_crash_cases_are_strongly_connected_and_deep(n, v):
    states = _oracle_states(n, v, ref.CRASH_TICKS, crash_tick=12, crash_count=ref.CRASHED[n], crash_seed=42)
    for t in ref.CRASH_TICKS:
        views, failed = states[t]
        assert int((failed != 0).sum()) == (ref.CRASHED[n] if t > 12 else 0)
        out, inn, src = _case(views, failed)
        ref.check_crash_case(out, inn)
        s = summarize_reach(ref.as_walk(out, len(src)), ref.as_walk(inn, len(src)))
        assert s["strongly_connected"] is True and s["live_sources"] == int((failed[src] == 0).sum())
        assert (s["live_sources"] < 64) == (t > 12), "a crashed source exactly where the case has a crashed node"
        assert all(x["unreached"] == 0 for x in s["out"]["sources"] if x["live"])
        assert 2 <= s["out"]["hops"] <= 5 and 2 <= s["in"]["hops"] <= 5


def test_sparse_case():
    c = dict(ref.SPARSE)
    n, v = c.pop("n"), c.pop("v")
    states = _oracle_states(n, v, ref.SPARSE_TICKS, **c)
    for t in ref.SPARSE_TICKS:
        out, inn, src = _case(*states[t])
        ref.check_sparse_case(t, out, inn)
    out, inn, src = _case(*states[20])
    s = summarize_reach(ref.as_walk(out, len(src)), ref.as_walk(inn, len(src)))
    assert s["strongly_connected"] is False
    assert {x["reached"] for x in s["out"]["sources"]} == {112, 113, 114, 115}  # of 128: nobody reaches everybody
    got = [x["reached"] for x in s["in"]["sources"]]
    assert min(got) == 1 and max(got) == 128


def test_half_cluster_crash_case():
    c = dict(ref.HALF)
    n, v = c.pop("n"), c.pop("v")
    states = _oracle_states(n, v, ref.HALF_TICKS, **c)
    for t in ref.HALF_TICKS:
        views, failed = states[t]
        out, inn, src = _case(views, failed)
        ref.check_half_crash_case(t, out, inn)
        s = summarize_reach(ref.as_walk(out, len(src)), ref.as_walk(inn, len(src)))
        assert s["strongly_connected"] is False and s["live"] == 500
        for name, exp in (("out", out), ("in", inn)):
            want = [500 - int(r) if live else None for r, live in zip(ref.reached(exp)[:len(src)], exp[0][0] == 1)]
            assert [x["unreached"] for x in s[name]["sources"]] == want
        if t == 20:
            assert {x["unreached"] for x in s["out"]["sources"] if x["live"]} == {1}
