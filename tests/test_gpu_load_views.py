"""PARTIAL: a view state loaded into a context (gm_load_views_begin / gm_load_views / gm_load_views_commit,
membership.state.view_snapshot / view_restore) continues exactly as the run it was taken from.

A continued run is compared with the oracle's own uninterrupted run, and layouts (one context, G loopback
row shards, one forced RCCL rank) with each other; the chosen state of section 5 is loaded into the oracle
as well (PartialOracle.load_snapshot). States built on the node tick's edges: test_gpu_partial_edges.py."""
import copy
import ctypes

import numpy as np
import pytest

import oracle_py
from membership import GM_EV_JOINED, GM_MODE_FAITHFUL, GM_MODE_PARTIAL, GM_MODE_SCALED, GmError, Simulator, crash_set, state
from membership.abi import partial_loopback_tick

pytestmark = pytest.mark.gpu

EINVAL, ERANGE, ESTATE, EUNSUPPORTED = -1, -4, -5, -6
KW = dict(rd_seed=7, view_seed=5, init_t0=8, init_seed=11)
T0 = 8
CRASH_TICK, NCRASH = T0 + 3, 3


def make(n, v, world=1, drop=5):
    """one context, or the `world` row shards of one cluster"""
    return [Simulator(n, GM_MODE_PARTIAL, view=v, init_mode=1, drop_pct=drop, drop_from=0, drop_to=1000, drop_seed=42,
                      shard_rank=g, shard_count=world, **KW) for g in range(world)]


def oracle(n, v, drop=5):
    return oracle_py.PartialOracle(n, v=v, crash_tick=CRASH_TICK, crash_count=NCRASH, crash_seed=42, drop_pct=drop,
                                   drop_from=0, drop_to=1000, drop_seed=42, **KW)


def tick(sims):
    if len(sims) == 1:
        sims[0].tick()
    else:
        partial_loopback_tick(sims)


def events(sims):
    return sorted((e[0], e[1], 1 if e[2] == GM_EV_JOINED else 2, e[3]) for s in sims for e in s.drain_events())


def dump(sims):
    return b"".join(s.dump_tables() for s in sims)


def snapshot(sims):
    return state.join_rows([state.view_snapshot(s) for s in sims])


def restore(sims, snap, chunk_rows=None):
    for s in sims:
        state.view_restore(s, state.slice_rows(snap, *s.shard_layout()), chunk_rows=chunk_rows)


def run_to(sims, ora, until, n):
    """tick the group (and the oracle) until their time is `until`; the crash set falls after CRASH_TICK"""
    crash = crash_set(n, NCRASH, 42)
    while sims[0].time < until:
        t = sims[0].time
        if ora is not None:
            ora.tick()
        tick(sims)
        if t == CRASH_TICK:
            for s in sims:
                s.set_failed(crash)
        for s in sims:
            s.drain_events()
    return crash


def follow(groups, ora, ticks, n, what=""):
    """every group and the oracle tick together: dumps and drained events equal every tick"""
    crash = crash_set(n, NCRASH, 42)
    for _ in range(ticks):
        t = groups[0][0].time
        ora.tick()
        want_ev, want = sorted(ora.events()), ora.dump()
        for k, sims in enumerate(groups):
            assert sims[0].time == t
            tick(sims)
            if t == CRASH_TICK:
                for s in sims:
                    s.set_failed(crash)
            assert events(sims) == want_ev, f"{what}: events of group {k} differ at tick {t}"
            assert dump(sims) == want, f"{what}: views of group {k} differ at tick {t}"
    for sims in groups:
        for s in sims:
            assert s.tick_stats()["err"] == 0


# ------------------------------------------------------------------ 1. round trip against the oracle
@pytest.mark.parametrize("v", [32, 16])
def test_round_trip_continues_like_the_oracle(v):
    n = 300
    ora, a = oracle(n, v), make(n, v)
    run_to(a, ora, T0 + 7, n)  # after tick t0 + 6
    assert dump(a) == ora.dump()
    snap = state.view_snapshot(a[0])
    assert snap["t"] == T0 + 7 and snap["views"].shape == (n, v) and snap["failed"].sum() == NCRASH
    b = make(n, v)
    state.view_restore(b[0], snap)
    assert b[0].time == a[0].time
    assert b[0].dump_tables() == a[0].dump_tables()
    for x, y in zip(b[0].read_targets(), a[0].read_targets()):
        assert np.array_equal(x, y)
    assert np.array_equal(b[0].read_nodes(), a[0].read_nodes())
    assert b[0].drain_events() == [] and b[0].event_total() == 0
    for x, y in zip(b[0].view_census(), a[0].view_census()):
        assert np.array_equal(x, y)
    st = b[0].load_views_stats()
    assert st["rows"] == n and 0 < st["staging_bytes"] <= 256 << 20
    follow([a, b], ora, 25, n, "round trip")  # through the crashed nodes' TREMOVE removals


# ------------------------------------------------------------------ 2. between layouts
def load_descending(sim, snap, block):
    """the low-level calls, blocks of `block` nodes given in descending order"""
    n0, nloc = sim.shard_layout()
    u64 = ctypes.c_uint64
    sim._call("gm_load_views_begin", sim.h, snap["t"])
    for r0 in reversed(range(0, nloc, block)):
        blk = np.ascontiguousarray(snap["views"][r0:r0 + block])
        sim._call("gm_load_views", sim.h, n0 + r0, len(blk), blk.ctypes.data_as(ctypes.POINTER(u64)))
    i32p = ctypes.POINTER(ctypes.c_int32)
    arrs = [np.ascontiguousarray(snap[k], dtype=np.int32) for k in ("heartbeat", "failed", "targets", "counts")]
    sim._call("gm_load_views_commit", sim.h, *[a.ctypes.data_as(i32p) for a in arrs])


@pytest.mark.parametrize("world,chunks,stage", [(2, 1, 0), (3, 4, 0), (3, 4, 7)])
def test_between_layouts(world, chunks, stage, monkeypatch):
    """one context -> G loopback row shards (uneven sizes) and back; stage = 7: GM_LOAD_STAGE_ROWS, so a
    block of 40 nodes takes six launches with a short last one, the commit's node arrays 56 at a time,
    and the blocks come in descending order"""
    n, v = 301, 32
    ora, one = oracle(n, v), make(n, v)
    run_to(one, ora, T0 + 7, n)
    snap = state.view_snapshot(one[0])
    monkeypatch.setenv("GM_CHUNKS", str(chunks))
    shards = make(n, v, world)
    monkeypatch.delenv("GM_CHUNKS")
    if stage:
        monkeypatch.setenv("GM_LOAD_STAGE_ROWS", str(stage))
        for s in shards:
            load_descending(s, state.slice_rows(snap, *s.shard_layout()), 40)
            assert s.load_views_stats()["staging_bytes"] < 7 * 8 * v + 64
        monkeypatch.delenv("GM_LOAD_STAGE_ROWS")
    else:
        restore(shards, snap)
    assert dump(shards) == one[0].dump_tables() and events(shards) == []
    follow([shards], ora, 25, n, f"G = {world}")
    # the way back: the shards' snapshots joined, into a fresh single context
    back = snapshot(shards)
    assert back["n0"] == 0 and back["views"].shape == (n, v) and back["t"] == T0 + 7 + 25
    single = make(n, v)
    restore(single, back)
    assert single[0].dump_tables() == ora.dump()
    follow([single, shards], ora, 4, n, "back in one context")


# ------------------------------------------------------------------ 3. one-rank RCCL row shard
def test_rccl_single_rank_row_shard(monkeypatch):
    from membership.abi import comm_unique_id
    n, v = 300, 32
    ora, one = oracle(n, v), make(n, v)
    run_to(one, ora, T0 + 7, n)
    monkeypatch.setenv("GM_FORCE_SHARD", "1")
    sh = make(n, v)
    monkeypatch.delenv("GM_FORCE_SHARD")
    sh[0].comm_init(comm_unique_id(), 1, 0)
    state.view_restore(sh[0], state.view_snapshot(one[0]))
    follow([sh], ora, 12, n, "RCCL rank")


# ------------------------------------------------------------------ 4. crash timing
@pytest.mark.parametrize("later", [0, 8])
@pytest.mark.parametrize("world", [1, 3])
def test_crash_timing(later, world):
    """later = 0: the snapshot right after set_failed -- the crashed nodes ran tick t - 1, their targets
    stand and their last lists must still be delivered; later = 8: frozen views, counts 0"""
    n, v = 300, 32
    ora, one = oracle(n, v), make(n, v)
    crash = run_to(one, ora, CRASH_TICK + 1 + later, n)
    snap = state.view_snapshot(one[0])
    assert np.array_equal(np.flatnonzero(snap["failed"]), np.sort(crash))
    assert np.all(snap["heartbeat"][crash] == 2 * CRASH_TICK)
    if later:
        assert np.all(snap["counts"][crash] == 0)
    else:
        assert np.all(snap["counts"][crash] > 0)
    grp = make(n, v, world)
    restore(grp, snap)
    assert dump(grp) == ora.dump()
    follow([grp], ora, 12, n, f"crash + {later}")


# ------------------------------------------------------------------ 5. a chosen state
def chosen_state(n, v, t, depth):
    """A state built by hand: receiver r gets depth[r] lists at tick t. Every node is live with heartbeat
    2(t - 1), holds itself, its targets and filler peers (heartbeats one tick old), ids ascending."""
    rng = np.random.default_rng(5)
    tg = [[] for _ in range(n)]
    s = 3
    for r, d in depth.items():
        for _ in range(d):
            while s % n == r or r in tg[s % n] or len(tg[s % n]) >= 5:
                s += 7
            tg[s % n].append(r)
            s += 7
    views = np.zeros((n, v), dtype=np.uint64)
    targets = np.zeros((n, 5), dtype=np.int32)
    counts = np.zeros(n, dtype=np.int32)
    for i in range(n):
        rest = [j for j in rng.permutation(n) if j != i and j not in tg[i]][:v - 1 - len(tg[i])]
        ids = np.sort(np.array([i] + tg[i] + rest)) + 1
        hb = np.where(ids == i + 1, 2 * (t - 1) - 1, 2 * (t - 2) - 1)
        views[i] = (ids.astype(np.uint64) << np.uint64(32)) | hb.astype(np.uint64)
        counts[i] = len(tg[i])
        targets[i, :counts[i]] = tg[i]
    return {"t": t, "n0": 0, "views": views, "heartbeat": np.full(n, 2 * (t - 1), dtype=np.int32),
            "failed": np.zeros(n, dtype=np.int32), "targets": targets, "counts": counts}


def test_chosen_state_reaches_all_three_node_kernels():
    """Inbox depths 0..20 on 21 receivers spread over the shards: past P_KSMALL = 12 (gm_p_tick_big) and
    P_KP = 16 (gm_p_tick_huge). tick_stats exposes the first tick's "lists merged" as their sum and
    their maximum, not per node: 210 lists in all, 20 at most, on one context and summed over G = 3.
    The oracle takes the same state: both layouts equal it, not only each other."""
    n, v, t = 300, 32, 15
    snap = chosen_state(n, v, t, {14 * d: d for d in range(21)})
    assert snap["counts"].sum() == 210
    one, three = make(n, v, drop=0), make(n, v, 3, drop=0)
    ora = oracle_py.PartialOracle(n, v=v, **KW)
    ora.load_snapshot(snap)
    restore(one, snap)
    restore(three, snap)
    assert dump(three) == dump(one) == ora.dump()
    for k in range(5):
        tick(one)
        tick(three)
        ora.tick()
        if k == 0:
            st = [s.tick_stats() for s in one + three]
            assert st[0]["lists"] == 210 and st[0]["max_inbox"] == 20
            assert sum(x["lists"] for x in st[1:]) == 210 and max(x["max_inbox"] for x in st[1:]) == 20
            sizes = one[0].view_census(records=False)[2]
            assert sizes.sum() == n and sizes[v] == n  # every view was full and stays full
        ev = events(one)
        assert events(three) == ev, f"events differ at tick {t + k}"
        assert dump(three) == dump(one), f"views differ at tick {t + k}"
        assert ev == sorted(ora.events()), f"events differ from the oracle's at tick {t + k}"
        assert dump(one) == ora.dump(), f"views differ from the oracle's at tick {t + k}"
        if k == 0:
            assert ora.profile()["lists"][[14 * d for d in range(21)]].tolist() == list(range(21))
    assert all(s.tick_stats()["err"] == 0 for s in one + three)


# ------------------------------------------------------------------ 6. the contract
@pytest.fixture(scope="module")
def base():
    """the state right after set_failed: live nodes and three crashed ones that ran tick t - 1"""
    n, v = 300, 32
    one = make(n, v)
    crash = run_to(one, None, CRASH_TICK + 1, n)
    return state.view_snapshot(one[0]), crash


def shifted(snap, dt):
    """the same state dt ticks later (heartbeats are relative to the tick)"""
    out = copy.deepcopy(snap)
    out["t"] += dt
    out["views"] = np.where(out["views"] != 0, out["views"] + np.uint64(2 * dt), out["views"])
    out["heartbeat"] = out["heartbeat"] + 2 * dt
    return out


def entry(i, hb):
    return (np.uint64(i) << np.uint64(32)) | np.uint64(hb)


def self_slot(snap, i):
    return int(np.flatnonzero((snap["views"][i] >> np.uint64(32)) == i + 1)[0])


def set_self_hb(snap, i, hb):
    snap["views"][i, self_slot(snap, i)] = entry(i + 1, hb)


def live_node(snap, k=0):
    return int(np.flatnonzero(snap["failed"] == 0)[10 + k])


def other_slot(snap, i):
    """a slot of node i's view that is neither its own entry nor the first or last one"""
    s = self_slot(snap, i)
    return 5 if s != 5 else 6


def m_id_zero(s, c):
    i = live_node(s)
    s["views"][i, 0] = np.uint64(2 * (s["t"] - 2) - 1)  # id 0 with a heartbeat


def m_id_past_n(s, c):
    i = live_node(s, 1 if self_slot(s, live_node(s)) == 31 else 0)
    s["views"][i, 31] = entry(301, 2 * (s["t"] - 2) - 1)


def m_order(s, c):
    i = live_node(s)
    a = other_slot(s, i)
    b = a + 1 if self_slot(s, i) != a + 1 else a + 2
    s["views"][i, [a, b]] = s["views"][i, [b, a]]


def m_repeat(s, c):
    i = live_node(s)
    a = other_slot(s, i)
    s["views"][i, a] = s["views"][i, a - 1] if self_slot(s, i) != a - 1 else s["views"][i, a + 1]


def m_gap(s, c):
    i = live_node(s)
    s["views"][i, other_slot(s, i)] = 0


def m_even_hb(s, c):
    i = live_node(s)
    s["views"][i, other_slot(s, i)] -= np.uint64(1)


def m_hb_ahead(s, c):
    i = live_node(s)
    a = other_slot(s, i)
    s["views"][i, a] = entry(int(s["views"][i, a] >> np.uint64(32)), 2 * (s["t"] - 1) + 1)


def m_age(s, c):  # on a state shifted by 40 ticks: age (t - 1) - 1 >= GM_VIEW_AGES
    i = live_node(s)
    a = other_slot(s, i)
    s["views"][i, a] = entry(int(s["views"][i, a] >> np.uint64(32)), 1)


def m_self_stale(s, c):
    i = live_node(s)
    set_self_hb(s, i, 2 * (s["t"] - 1) - 3)


def m_self_missing(s, c):
    i = live_node(s)
    a = self_slot(s, i)
    s["views"][i, a:-1] = s["views"][i, a + 1:]
    s["views"][i, -1] = 0


def m_live_heartbeat(s, c):
    i = live_node(s)
    s["heartbeat"][i] -= 2
    set_self_hb(s, i, int(s["heartbeat"][i]) - 1)


def m_crashed_odd(s, c):
    s["heartbeat"][c[0]] -= 1


def m_crashed_ahead(s, c):
    s["heartbeat"][c[0]] += 2


def m_failed(s, c):
    s["failed"][live_node(s)] = 2


def m_count_high(s, c):
    s["counts"][live_node(s)] = 6


def m_count_negative(s, c):
    s["counts"][live_node(s)] = -1


def with_target(fn):
    def m(s, c):
        i = next(j for j in range(50, 300) if s["failed"][j] == 0 and s["counts"][j] >= 2)
        s["targets"][i, 1] = fn(s, i)
    return m


m_target_n = with_target(lambda s, i: 300)
m_target_negative = with_target(lambda s, i: -1)
m_target_self = with_target(lambda s, i: i)
m_target_twice = with_target(lambda s, i: s["targets"][i, 0])
m_target_not_in_view = with_target(
    lambda s, i: next(j for j in range(300) if j + 1 not in set((s["views"][i] >> np.uint64(32)).tolist())))


def m_crashed_sender(s, c):  # a crashed node that did not run tick t - 1 but names targets
    s["heartbeat"][c[0]] -= 2
    set_self_hb(s, c[0], int(s["heartbeat"][c[0]]) - 1)


VIEW_CASES = [m_id_zero, m_id_past_n, m_order, m_repeat, m_gap, m_even_hb, m_hb_ahead]
COMMIT_CASES = [m_age, m_self_stale, m_self_missing, m_live_heartbeat, m_crashed_odd, m_crashed_ahead, m_failed,
                m_count_high, m_count_negative, m_target_n, m_target_negative, m_target_self, m_target_twice,
                m_target_not_in_view, m_crashed_sender]


def test_contract_rejected_states(base):
    """one bad field at a time: the code, the call that reports it, nothing written by a failed block,
    and a clean load after each failed one"""
    good, crash = base
    n, v = 300, 32
    ctx = make(n, v)[0]
    ref = make(n, v)[0]
    untouched = ctx.read_views(0, n)
    first = True
    for case in VIEW_CASES + COMMIT_CASES:
        snap = shifted(good, 40) if case is m_age else copy.deepcopy(good)
        clean = copy.deepcopy(snap)
        case(snap, crash)
        with pytest.raises(GmError) as e:
            state.view_restore(ctx, snap)
        call = "gm_load_views:" if case in VIEW_CASES else "gm_load_views_commit:"
        assert e.value.code == EINVAL and str(e.value).startswith(call), (case.__name__, str(e.value))
        if first:  # a failed block wrote nothing: the time and the views are the created context's
            assert np.array_equal(ctx.read_views(0, n), untouched)
            first = False
        for call_again in (ctx.tick, lambda: ctx.set_failed([1])):  # still loading
            with pytest.raises(GmError) as e:
                call_again()
            assert e.value.code == ESTATE, case.__name__
        with pytest.raises(GmError) as e:  # the voided load takes nothing more: begin starts over
            ctx._call("gm_load_views", ctx.h, 0, 1, snap["views"].ctypes.data_as(
                ctypes.POINTER(ctypes.c_uint64)))
        assert e.value.code == ESTATE
        state.view_restore(ctx, clean)
        assert ctx.time == clean["t"] and np.array_equal(ctx.read_views(0, n), clean["views"]), case.__name__
    # the last clean load is the base state: it ticks like a context restored once
    state.view_restore(ctx, good)
    state.view_restore(ref, good)
    for _ in range(3):
        ctx.tick()
        ref.tick()
        assert ctx.dump_tables() == ref.dump_tables() and ctx.drain_events() == ref.drain_events()
    assert ctx.tick_stats()["err"] == 0


def test_contract_inbox_overflow_is_erange():
    n, v, t = 300, 32, 15
    ctx = make(n, v, drop=0)[0]
    with pytest.raises(GmError) as e:
        state.view_restore(ctx, chosen_state(n, v, t, {7: 64}))  # 64 senders, 63 inbox slots
    assert e.value.code == ERANGE and str(e.value).startswith("gm_load_views_commit:")
    state.view_restore(ctx, chosen_state(n, v, t, {7: 63}))
    ctx.tick()
    st = ctx.tick_stats()
    assert st["err"] == 0 and st["max_inbox"] == 63 and st["lists"] == 63


def test_contract_protocol_and_modes(base):
    good, _ = base
    n, v = 300, 32
    u64p = ctypes.POINTER(ctypes.c_uint64)
    i32p = ctypes.POINTER(ctypes.c_int32)
    views = good["views"]
    arrs = [np.ascontiguousarray(good[k], dtype=np.int32) for k in ("heartbeat", "failed", "targets", "counts")]

    def code(sim, name, *args):
        with pytest.raises(GmError) as e:
            sim._call(name, sim.h, *args)
        return e.value.code

    ctx = make(n, v)[0]
    assert code(ctx, "gm_load_views", 0, 1, views.ctypes.data_as(u64p)) == ESTATE  # no begin
    assert code(ctx, "gm_load_views_commit", *[a.ctypes.data_as(i32p) for a in arrs]) == ESTATE
    for t in (5, 16385, -1):  # outside t0 + 1 for the t0 a context can be created with
        assert code(ctx, "gm_load_views_begin", t) == EINVAL
    ctx._call("gm_load_views_begin", ctx.h, good["t"])
    assert code(ctx, "gm_load_views", -1, 2, views.ctypes.data_as(u64p)) == EINVAL
    assert code(ctx, "gm_load_views", 299, 2, views.ctypes.data_as(u64p)) == EINVAL
    ctx._call("gm_load_views", ctx.h, 0, 200, views.ctypes.data_as(u64p))
    assert code(ctx, "gm_load_views_commit", *[a.ctypes.data_as(i32p) for a in arrs]) == ESTATE  # nodes missing
    assert code(ctx, "gm_load_views", 199, 2, views[199:].ctypes.data_as(u64p)) == ESTATE  # node 199 twice
    ctx._call("gm_load_views", ctx.h, 200, 100, views[200:].ctypes.data_as(u64p))
    ctx._call("gm_load_views_commit", ctx.h, *[a.ctypes.data_as(i32p) for a in arrs])
    assert ctx.time == good["t"] and ctx.load_views_stats()["rows"] == n
    ctx.tick()
    # a row shard takes its own nodes only
    sh = make(n, v, 2)
    sh[1]._call("gm_load_views_begin", sh[1].h, good["t"])
    assert code(sh[1], "gm_load_views", 149, 2, views[149:].ctypes.data_as(u64p)) == EINVAL
    with pytest.raises(GmError) as e:  # a member between begin and commit
        partial_loopback_tick(sh)
    assert e.value.code == ESTATE
    # other modes, and a context recording msgcount
    assert code(Simulator(64, GM_MODE_SCALED, rd_seed=7), "gm_load_views_begin", 9) == EUNSUPPORTED
    assert code(Simulator(10, GM_MODE_FAITHFUL), "gm_load_views_begin", 9) == EUNSUPPORTED
    rec = make(n, v)[0]
    rec.msgcount_record(40)
    assert code(rec, "gm_load_views_begin", good["t"]) == EUNSUPPORTED
    # read_targets of a SCALED context still spans the cluster
    tg, cnt = Simulator(64, GM_MODE_SCALED, rd_seed=7).read_targets()
    assert tg.shape == (64, 5) and cnt.shape == (64,)


def test_contract_group_with_one_member_not_loaded(base, monkeypatch):
    """the replayed exchange is a collective: two of three loopback shards loaded -> GM_ESTATE on all"""
    n, v = 300, 32
    monkeypatch.setenv("GM_CHUNKS", "1")
    sh = make(n, v, 3)
    monkeypatch.delenv("GM_CHUNKS")
    good, crash = base
    while sh[0].time < good["t"]:
        partial_loopback_tick(sh)
    for s in sh:  # every member holds the crash set of the state: only the pending exchange differs
        s.set_failed(crash)
    for s in sh[:2]:
        state.view_restore(s, state.slice_rows(good, *s.shard_layout()))
    with pytest.raises(GmError) as e:
        partial_loopback_tick(sh)
    assert e.value.code == ESTATE
    for s in sh:
        with pytest.raises(GmError) as e:
            s.tick()
        assert e.value.code == ESTATE


# ------------------------------------------------------------------ 7. the timed branches of the block loop
def test_timed_load_equals_untimed_load(base, monkeypatch):
    """gm_set_timing changes what a load measures, not what it writes: the same state through launches of
    7 nodes into a timed and an untimed context, and into a third, timed one whose first load a bad block
    voided: the begin of its clean load resets the times. Then 3 ticks on all three."""
    good, _ = base
    n, v = 300, 32
    monkeypatch.setenv("GM_LOAD_STAGE_ROWS", "7")
    timed, plain, again = (make(n, v)[0] for _ in range(3))
    timed.set_timing(True)
    again.set_timing(True)
    for sim in (timed, plain):
        state.view_restore(sim, good)
    # a gap in the view of a node 22 launches into the one block: the launches before it pass and are timed
    bad = copy.deepcopy(good)
    i = live_node(bad, 150)
    bad["views"][i, other_slot(bad, i)] = 0
    with pytest.raises(GmError) as e:
        state.view_restore(again, bad)
    assert e.value.code == EINVAL and str(e.value).startswith("gm_load_views:")
    sv = again.load_views_stats()
    assert i >= 7 and sv["rows"] == i // 7 * 7 and sv["check_ms"] > 0 and sv["store_ms"] > 0
    again._call("gm_load_views_begin", again.h, good["t"])
    s0 = again.load_views_stats()
    assert s0["rows"] == 0 and s0["check_ms"] == 0 and s0["store_ms"] == 0  # only the clean load counts
    assert s0["staging_bytes"] == sv["staging_bytes"]
    again._call("gm_load_views", again.h, 0, n, good["views"].ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)))
    arrs = [np.ascontiguousarray(good[k], dtype=np.int32) for k in ("heartbeat", "failed", "targets", "counts")]
    again._call("gm_load_views_commit", again.h, *[a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)) for a in arrs])
    st, sp, sa = timed.load_views_stats(), plain.load_views_stats(), again.load_views_stats()
    assert st["rows"] == n and sp["rows"] == n and sa["rows"] == n
    assert st["staging_bytes"] == sp["staging_bytes"] == sa["staging_bytes"]
    assert st["check_ms"] > 0 and st["store_ms"] > 0 and sa["check_ms"] > 0 and sa["store_ms"] > 0
    assert sp["check_ms"] == 0 and sp["store_ms"] == 0
    for sim in (timed, again):
        assert sim.time == plain.time == good["t"]
        assert np.array_equal(sim.read_views(0, n), plain.read_views(0, n))
        assert np.array_equal(sim.read_nodes(), plain.read_nodes())
        for a, b in zip(sim.read_targets(), plain.read_targets()):
            assert np.array_equal(a, b)
        assert sim.dump_tables() == plain.dump_tables()
    assert np.array_equal(plain.read_views(0, n), good["views"])
    for _ in range(3):
        for sim in (timed, plain, again):
            sim.tick()
    assert timed.dump_tables() == plain.dump_tables() == again.dump_tables(), "dumps differ after 3 ticks"
    assert all(s.tick_stats()["err"] == 0 for s in (timed, plain, again))
