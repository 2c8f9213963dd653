"""The PARTIAL oracle's state load (op_load_state) and telemetry (op_last_profile), on the CPU alone.

1. Round trip: a state read from a running oracle and loaded into a fresh one continues identically.
2. Rejections: every malformed state of test_gpu_load_views.py's contract section (the same mutators, run
   on an oracle-made base state) is refused, and nothing is loaded.
3. Coverage conditions: what tests/partial_states.py builds really sits on the edges the GPU tests
   (test_gpu_partial_edges.py) count on. These are conditions on the inputs, checked by the reference
   alone, so a builder that drifts cannot silently hollow those tests out."""
import copy

import numpy as np
import pytest

import oracle_py
import partial_states as ps
import test_gpu_load_views as lv  # its contract section: the mutators and chosen_state (plain NumPy)

KW = dict(rd_seed=7, view_seed=5, init_t0=8, init_seed=11)
T0 = 8
CRASH_TICK, NCRASH = T0 + 3, 3
T = 40  # the tick the built states run: ages up to GM_VIEW_AGES need t > 33
TFAIL, TREMOVE = ps.TFAIL, ps.TREMOVE


def oracle(n, v, drop=5):
    return oracle_py.PartialOracle(n, v=v, crash_tick=CRASH_TICK, crash_count=NCRASH, crash_seed=42, drop_pct=drop,
                                   drop_from=0, drop_to=1000, drop_seed=42, **KW)


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------ 1. round trip
@pytest.mark.parametrize("v", [16, 32])
@pytest.mark.parametrize("later", [0, 8])
def test_round_trip(v, later):
    """later = 0: right after the crash tick, when the crashed nodes still have targets whose lists must
    be delivered; later = 8: frozen views, no targets"""
    n = 300
    a = oracle(n, v)
    while a.time < CRASH_TICK + 1 + later:
        a.tick()
    snap = a.snapshot()
    crash = np.flatnonzero(snap["failed"])
    assert len(crash) == NCRASH and snap["t"] == CRASH_TICK + 1 + later
    assert np.all(snap["counts"][crash] > 0) if later == 0 else np.all(snap["counts"][crash] == 0)
    b = oracle(n, v)
    b.load_snapshot(snap)
    assert b.time == a.time and b.dump() == a.dump() and b.events() == []
    assert same(b.targets(), a.targets()) and np.array_equal(b.nodes(), a.nodes())
    for _ in range(25):
        a.tick()
        b.tick()
        assert b.dump() == a.dump() and b.events() == a.events(), f"tick {a.time - 1}"
        assert same(b.targets(), a.targets()) and same(b.last_msgcount(), a.last_msgcount()), f"tick {a.time - 1}"
        assert same(b.profile().values(), a.profile().values())
    assert np.array_equal(b.nodes(), a.nodes())


def test_load_applies_the_crash_tick_afterwards():
    """a state from before the crash tick: the loaded oracle's own config crashes the set on time"""
    n, v = 300, 16
    a, b = oracle(n, v), oracle(n, v)
    while a.time < CRASH_TICK - 1:
        a.tick()
    b.load_snapshot(a.snapshot())
    for _ in range(4):
        a.tick()
        b.tick()
    assert b.nodes()[:, 2].sum() == NCRASH and b.dump() == a.dump()


# ------------------------------------------------------------------ 2. rejections
@pytest.fixture(scope="module")
def base():
    """as test_gpu_load_views.base: the state right after the crash set fell, from the oracle"""
    a = oracle(300, 32)
    while a.time < CRASH_TICK + 1:
        a.tick()
    snap = a.snapshot()
    return snap, np.flatnonzero(snap["failed"])


EXPECT = {"m_id_zero": "EID", "m_id_past_n": "EID", "m_order": "EORDER", "m_repeat": "EORDER", "m_gap": "EGAP",
          "m_even_hb": "EHBPAR", "m_hb_ahead": "EHBTOP", "m_age": "EAGE", "m_self_stale": "ESELF",
          "m_self_missing": "ESELF", "m_live_heartbeat": "EHEARTBEAT", "m_crashed_odd": "EHEARTBEAT",
          "m_crashed_ahead": "EHEARTBEAT", "m_failed": "EFAILED", "m_count_high": "ECOUNT",
          "m_count_negative": "ECOUNT", "m_crashed_sender": "ECRASHED"}


@pytest.mark.parametrize("case", lv.VIEW_CASES + lv.COMMIT_CASES, ids=lambda c: getattr(c, "__name__", "m_target"))
def test_rejected_states(base, case):
    good, crash = base
    snap = lv.shifted(good, 40) if case is lv.m_age else copy.deepcopy(good)
    clean = copy.deepcopy(snap)
    case(snap, crash)
    ora, twin = oracle(300, 32), oracle(300, 32)
    before = ora.dump()
    with pytest.raises(oracle_py.OracleLoadError) as e:
        ora.load_snapshot(snap)
    want = EXPECT.get(case.__name__, "ETARGET")  # with_target's closures are all named m
    assert e.value.bits & oracle_py.OP_LD[want], (case.__name__, str(e.value))
    assert ora.dump() == before and ora.time == twin.time  # nothing was loaded
    ora.tick()
    twin.tick()
    assert ora.dump() == twin.dump()
    ora.load_snapshot(clean)  # and the clean state still loads
    assert ora.time == clean["t"] and np.array_equal(ora.views(), clean["views"])


def test_rejected_inbox_overflow_and_arguments():
    n, v, t = 300, 32, 15
    ora = oracle(n, v, drop=0)
    with pytest.raises(oracle_py.OracleLoadError) as e:
        ora.load_snapshot(lv.chosen_state(n, v, t, {7: 64}))  # 64 senders, 63 inbox slots
    assert e.value.bits == oracle_py.OP_LD["EINBOX"]
    ok = lv.chosen_state(n, v, t, {7: 63})
    ora.load_snapshot(ok)
    ora.tick()
    assert ora.profile()["lists"][7] == 63
    for bad_t in (5, 16385, -1):  # the ticks gm_load_views_begin refuses
        with pytest.raises(oracle_py.OracleLoadError) as e:
            ora.load_state(bad_t, ok["views"], ok["heartbeat"], ok["failed"], ok["targets"], ok["counts"])
        assert e.value.bits == oracle_py.OP_LD["EARG"]
    with pytest.raises(ValueError):
        ora.load_state(t, ok["views"][:, :16], ok["heartbeat"], ok["failed"], ok["targets"], ok["counts"])


# ------------------------------------------------------------------ 3. coverage conditions
def edge_tick(snap, v):
    """load, run the edge tick, return (profile, oracle). The ticks that follow it in the GPU tests stay
    within the HIP path's inbox capacity of 63 lists per receiver, which the oracle does not model."""
    n = len(snap["failed"])
    ora, on = (oracle_py.PartialOracle(n, v=v, **KW) for _ in range(2))
    on.load_snapshot(snap)
    for _ in range(4):
        on.tick()
        assert on.profile()["lists"].max() <= 63
    ora.load_snapshot(snap)
    ora.tick()
    return ora.profile(), ora


def role(snap, name):
    (r,) = snap["roles"][name]
    return r


@pytest.mark.parametrize("n,v", [(2100, 32), (300, 12), (300, 5)])
def test_coverage_deep_inbox(n, v):
    snap = ps.deep_inbox(n, v, T)
    p, _ = edge_tick(snap, v)
    for d in ps.DEPTHS:
        r = role(snap, f"depth{d}")
        assert p["lists"][r] == d and snap["counts"][snap["roles"][f"depth{d}:senders"]].tolist() == [1] * d
        assert p["union"][r] == min(n, v + (v - 1) * d) or n < v + (v - 1) * 63, (d, p["union"][r])
    assert set(ps.DEPTHS) <= set(p["lists"].tolist())
    if (n, v) == (2100, 32):  # the three tables at their design limits
        for d, size in ((12, 404), (16, 528), (63, 1985)):
            assert p["union"][role(snap, f"depth{d}")] >= size
    else:  # a small cluster: the lists overlap, the union is what the cluster holds
        assert p["union"][role(snap, "depth63")] >= min(n - 50, 250)
    assert p["stale"].max() > 0  # carried entries of age TFAIL arrive stale


@pytest.mark.parametrize("n,v", [(4096, 32), (512, 24)])
def test_coverage_eviction(n, v):
    snap = ps.eviction_cases(n, v, T)
    p, _ = edge_tick(snap, v)
    row = lambda name: {k: int(p[k][role(snap, name)]) for k in p}  # noqa: E731
    fit, over1 = row("fit"), row("over1")
    assert fit["swept"] == v and not fit["evicted"] and fit["lists"] == 1
    assert over1["swept"] == v + 1 and over1["evicted"]
    whole = row("class_whole")
    assert whole["evicted"] and whole["class_taken"] == whole["class_size"] > 1 and whole["swept"] > v + 1
    gw = row("group_whole")
    assert gw["class_taken"] < gw["class_size"] and gw["group_taken"] == gw["group_size"] > 1
    assert gw["class_taken"] > gw["group_taken"]  # groups below the cut group were taken too
    gp = row("group_part")
    assert gp["group_taken"] < gp["group_size"] and gp["class_taken"] < gp["class_size"]
    if (n, v) == (4096, 32):
        assert gp["group_taken"] >= 16 and gp["group_size"] >= 32
        for name, lists in (("big_part", 14), ("huge_part", 20)):  # the same in the big and the huge table
            x = row(name)
            assert x["lists"] == lists and 8 <= x["group_taken"] < x["group_size"] >= 32
    else:
        assert gp["group_taken"] >= 4 and gp["group_size"] >= 8
    first, firstw = row("first_part"), row("first_whole")
    assert first["class_ordinal"] == 0 and first["lists"] == v + 8 == first["class_size"] > first["class_taken"] == v - 1
    assert firstw["class_ordinal"] == 0 and firstw["class_size"] == firstw["class_taken"] == v - 1
    late, stale = row("late"), row("stale")
    assert late["class_ordinal"] >= 3 and stale["class_ordinal"] >= 3
    assert late["stale"] > 0 and late["class_taken"] < late["class_size"]  # the cut class is age TFAIL
    ages = ps.snapshot_ages(snap)
    assert (ages[role(snap, "stale")] == TREMOVE - 1).sum() == stale["class_size"] > stale["class_taken"] > 0


@pytest.mark.parametrize("v", [4, 31, 32])
def test_coverage_sweep(v):
    n = 128
    snap = ps.sweep_cases(n, v, T)
    p, ora = edge_tick(snap, v)
    row = lambda name: {k: int(p[k][role(snap, name)]) for k in p}  # noqa: E731
    ages = ps.snapshot_ages(snap)
    for a in (TFAIL - 1, TFAIL, TREMOVE - 1, TREMOVE):  # an entry at each of the four age boundaries
        r = role(snap, f"age{a}")
        assert (ages[r] == a).sum() == 1 and ages[r].max() == a
        x = row(f"age{a}")
        assert x["removed"] == x["remove_events"] == (a >= TREMOVE) and x["stale"] == (TFAIL <= a < TREMOVE)
        assert x["size"] == v - (a >= TREMOVE)
    assert 1 in p["removed"] and v - 1 in p["removed"]  # removals in one row: 1 and V - 1
    gone, fit = row("all_gone"), row("all_gone_fit")
    assert gone["removed"] == gone["remove_events"] == v - 1 and gone["swept"] == v + 1 and gone["evicted"]
    assert fit["removed"] == v - 1 and fit["swept"] == v and not fit["evicted"]
    ev = ora.events()
    for name, r in (("all_gone", role(snap, "all_gone")), ("all_gone_fit", role(snap, "all_gone_fit"))):
        kinds = [e[2] for e in ev if e[1] == r]
        assert kinds.count(1) == v - 1 and kinds.count(2) == v - 1, name  # 2V - 2 of the row's 2V event slots
    starved = row("starved")
    assert starved["removed"] > 0 and starved["numpot"] <= 0 and starved["targets"] == 0
    assert starved["size"] - 1 - starved["stale"] >= 1  # fresh peers remain
    if v >= 4:
        ref = row("refresh")
        r = role(snap, "refresh")
        assert {TREMOVE - 1, TREMOVE} <= set(ages[r].tolist()) and ref["removed"] == 0 and ref["lists"] == 1
        assert not [e for e in ev if e[1] == r and e[2] == 2]


@pytest.mark.parametrize("v", [32, 31, 3, 2])
def test_coverage_draw(v):
    n = 128
    snap = ps.draw_cases(n, v, T)
    p, _ = edge_tick(snap, v)
    for f in (0, 1, 2, 3, 4, 5, 8):
        if f"fresh{f}" not in snap["roles"]:
            assert f >= v - 1 and f > 0
            continue
        for r in snap["roles"][f"fresh{f}"]:
            assert p["numpot"][r] == f and p["targets"][r] == min(f, 5) and p["size"][r] == v
            assert p["stale"][r] == v - 1 - f
    assert set(p["targets"].tolist()) >= set(range(min(v - 1, 5) + 1))
    for size in (2, 3):
        if size <= v:
            for r in snap["roles"][f"size{size}"]:
                assert p["size"][r] == size and p["targets"][r] == size - 1
    if v >= 31:  # S2 outputs consumed: within the 16 precomputed ones, the lazy generator's first batch, later ones
        d = p["draws"]
        assert ((d > 0) & (d <= 16)).any() and ((d > 16) & (d <= 32)).any() and (d > 32).any()
        assert set(p["targets"].tolist()) == {0, 1, 2, 3, 4, 5}
        assert set(p["numpot"][p["stale"] > v // 2].tolist()) >= {0, 1, 2, 3, 4, 5, 8}
