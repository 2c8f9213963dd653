"""PARTIAL: the node tick (gm_partial_node.h p_node, all three tables) against the oracle on states built to
sit on its edges (tests/partial_states.py), loaded into both sides: the oracle by op_load_state, the
contexts by gm_load_views. What each builder reaches is asserted on the CPU, by the oracle's telemetry
alone (test_oracle_partial_load.py, the coverage conditions):

  deep_inbox      0 / 1 / 12 / 13 / 16 / 17 / 62 / 63 lists per receiver around P_KSMALL, P_KP and the inbox
                  capacity; at V = 32 the small, big and huge tables at their design loads (404 / 528 / 1985
                  ids); on row shards the lists arrive in wire format (the RM instantiations)
  eviction_cases  size V and V + 1; the cut class whole (needb == bsz), its cut key group whole
                  (needc == bsz2), a group of 40 taken in part (20 rounds of the exact min-selection; in the
                  big and huge tables too); the cut in the first class and after four or five classes
  sweep_cases     the ages TFAIL - 1 / TFAIL / TREMOVE - 1 / TREMOVE that p_aged folds into one compare;
                  V - 1 REMOVE and V - 1 JOINED events in one 2V-slot event row; entries a list refreshes;
                  numpot <= 0 through `removed` although fresh peers remain
  draw_cases      numpot 0..5 and 8 with mostly stale views: the draw runs through the 16 precomputed S2
                  outputs into the lazy generator's first and later batches; views of 2 and 3 entries

Every case runs the edge tick and three more that consume its targets, with 5 % keyed drops on the sends
from the edge tick on. After every tick the dumps (full bytes), the drained events, the targets in draw
order and the node arrays equal the oracle's; single contexts record msgcount, which pins the MC
instantiations of the three kernels against op_last_msgcount. The run-time-V path is covered at V = 31,
24, 12, 5, 4, 3, 2 (lanes with jo >= per, lane % V, lane / V).

Not covered, and not coverable: Lemire's rejection in the draw (`low < thr`) has probability about
size / 2^32 <= 2^-27 per draw; no state reaches it on purpose. The inbox-overflow flag GM_ERR_INBOX belongs
to test_gpu_load_views.py's contract tests."""
import functools

import numpy as np
import pytest

import oracle_py
import partial_states as ps
from membership import GM_EV_JOINED, GM_MODE_PARTIAL, Simulator, state
from membership.abi import partial_loopback_tick

pytestmark = pytest.mark.gpu

KW = dict(rd_seed=7, view_seed=5, init_t0=8, init_seed=11)
T = 40      # the edge tick (ages up to GM_VIEW_AGES = 32 need t > 33)
TICKS = 4   # the edge tick, then the ticks that consume its targets
DROP = dict(drop_pct=5, drop_from=T, drop_to=1000, drop_seed=42)  # the edge tick's own deliveries are whole
BUILDERS = {"deep_inbox": ps.deep_inbox, "eviction_cases": ps.eviction_cases, "sweep_cases": ps.sweep_cases,
            "draw_cases": ps.draw_cases}


@functools.lru_cache(maxsize=None)
def reference(builder, n, v):
    """(snapshot, the oracle's dump before the first tick, per tick: dump, sorted events, targets, counts,
    nodes, msgcount sent / received): computed once per state, shared by its layouts, never changed"""
    snap = BUILDERS[builder](n, v, T)
    ora = oracle_py.PartialOracle(n, v=v, **DROP, **KW)
    ora.load_snapshot(snap)
    start, ticks = ora.dump(), []
    for _ in range(TICKS):
        ora.tick()
        tg, cnt = ora.targets()
        sent, recv = ora.last_msgcount()
        ticks.append(dict(dump=ora.dump(), events=sorted(ora.events()), targets=tg, counts=cnt, nodes=ora.nodes(),
                          sent=sent, recv=recv))
    return snap, start, ticks


def make(n, v, world=1):
    return [Simulator(n, GM_MODE_PARTIAL, view=v, init_mode=1, shard_rank=g, shard_count=world, **DROP, **KW)
            for g in range(world)]


def first_difference(got, want):
    """the first differing dump line of each side, for the message"""
    for a, b in zip(got.splitlines(), want.splitlines()):
        if a != b:
            return f"\n got  {a[:400]!r}\n want {b[:400]!r}"
    return " (lengths differ)"


def check(builder, n, v, world=1, msgcount=False):
    snap, start, ticks = reference(builder, n, v)
    sims = make(n, v, world)
    for s in sims:
        state.view_restore(s, state.slice_rows(snap, *s.shard_layout()))
    if msgcount:
        sims[0].msgcount_record(T + TICKS)
    dump = lambda: b"".join(s.dump_tables() for s in sims)  # noqa: E731
    assert dump() == start, "the loaded views differ"
    for k, want in enumerate(ticks):
        t = T + k
        assert sims[0].time == t
        if world == 1:
            sims[0].tick()
        else:
            partial_loopback_tick(sims)
        ev = sorted((e[0], e[1], 1 if e[2] == GM_EV_JOINED else 2, e[3]) for s in sims for e in s.drain_events())
        got = dump()
        assert got == want["dump"], f"views differ at tick {t}:" + first_difference(got, want["dump"])
        assert ev == want["events"], f"events differ at tick {t}"
        tgs = [s.read_targets() for s in sims]
        tg, cnt = np.concatenate([x[0] for x in tgs]), np.concatenate([x[1] for x in tgs])
        bad = np.flatnonzero((cnt != want["counts"]) | (tg != want["targets"]).any(axis=1))
        assert bad.size == 0, f"targets differ at tick {t}: node {bad[0]}: {tg[bad[0]]} want {want['targets'][bad[0]]}"
        assert np.array_equal(np.concatenate([s.read_nodes() for s in sims]), want["nodes"]), f"nodes differ at tick {t}"
        if msgcount:
            sent, recv = sims[0].msgcount(t + 1)
            assert np.array_equal(sent[:, t], want["sent"]), f"msgcount sent differs at tick {t}"
            assert np.array_equal(recv[:, t], want["recv"]), f"msgcount received differs at tick {t}"
        if k == 0 and world == 1:  # the edge tick delivered what the state queued
            st = sims[0].tick_stats()
            assert st["lists"] == snap["counts"].sum()
            assert st["max_inbox"] == np.bincount(snap["targets"][snap["counts"] > 0, 0], minlength=1).max()
    for s in sims:
        assert s.tick_stats()["err"] == 0


# ------------------------------------------------------------------ inbox depth and table load
@pytest.mark.parametrize("msgcount", [False, True])
def test_deep_inbox_single_context(msgcount):
    check("deep_inbox", 2100, 32, msgcount=msgcount)


@pytest.mark.parametrize("chunks", [1, 4])
def test_deep_inbox_row_shards(chunks, monkeypatch):
    """G = 2 loopback row shards: receivers and senders are spread over both, so wire-format lists reach the
    big and the huge table (the RM path)"""
    monkeypatch.setenv("GM_CHUNKS", str(chunks))
    check("deep_inbox", 2100, 32, world=2)


@pytest.mark.parametrize("n,v", [(300, 12), (300, 5)])
def test_deep_inbox_run_time_width(n, v):
    """V = 12: per = 5 lists per load step, lanes 60..63 idle; V = 5: per = 12, 63 overlapping lists of 5"""
    check("deep_inbox", n, v, msgcount=True)


# ------------------------------------------------------------------ eviction, sweep, draw
@pytest.mark.parametrize("n,v", [(4096, 32), (512, 24)])
def test_eviction_cases(n, v):
    check("eviction_cases", n, v, msgcount=True)


@pytest.mark.parametrize("v", [4, 31, 32])
def test_sweep_cases(v):
    check("sweep_cases", 128, v, msgcount=True)


@pytest.mark.parametrize("v", [32, 31, 3, 2])
def test_draw_cases(v):
    check("draw_cases", 128, v, msgcount=True)
