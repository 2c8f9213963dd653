"""FAITHFUL batches (gm_batch_*, membership.Batch / BatchApplication): R independent clusters ticked in one
launch set compute, member by member, exactly what R solo runs compute -- against the seeded
reference's goldens, the CPU oracle and solo contexts (the path the goldens pin). Every comparison is
exact equality."""
import ctypes

import numpy as np
import pytest

import oracle_py
from golden_util import load_case, load_index, tick_digests_from_dump
from membership import (GM_MODE_FAITHFUL, GM_MODE_SCALED, Batch, BatchApplication, GmError, Params, Simulator, abi)
from membership.app import Log, fail_step, log_events, new_cluster

pytestmark = pytest.mark.gpu
CONFS = ("singlefailure", "multifailure", "msgdropsinglefailure")
ALL = load_index()


def first_diff(a, b):
    la, lb = a.split(b"\n"), b.split(b"\n")
    for k, (x, y) in enumerate(zip(la, lb)):
        if x != y:
            return f"line {k}: got {x!r} expected {y!r}"
    return f"length: got {len(la)} lines expected {len(lb)}"


def run_goldens(names, dumped):
    """the named goldens as ONE BatchApplication; members in `dumped` also check every tick's tables"""
    cases = [load_case(n) for n in names]
    app = BatchApplication([(Params.from_conf_text(m["conf"]), m["time_seed"], m["rd_seed"]) for m in cases],
                           ticks=700, dump_tables=[k for k, n in enumerate(names) if n in dumped])
    try:
        res = app.run()
        for n, m, r in zip(names, cases, res):
            assert r.dbg == m["dbg"], f"{n}: dbg.log differs: " + first_diff(r.dbg, m["dbg"])
            assert r.msgcount == m["msgcount"], f"{n}: msgcount.log differs: " + first_diff(r.msgcount, m["msgcount"])
            assert r.out == m["stdout"], f"{n}: stdout differs"
            assert (r.dumps is not None) == (n in dumped)
            if r.dumps is not None:
                d = tick_digests_from_dump(b"".join(r.dumps))
                assert d.shape == m["tick_digests"].shape
                bad = np.nonzero(d != m["tick_digests"])[0]
                assert bad.size == 0, f"{n}: membership tables differ first at tick {bad[:1]}"
    finally:
        app.close()


def test_goldens_as_one_batch():
    """all 75 N = 10 goldens (3 confs x 25 seed pairs), 700 ticks, one batch"""
    names = [n for n in ALL if n.split("_")[0] in CONFS]
    assert len(names) == 75
    dumped = {n for n in names if n.endswith("_T1_R1") or n.endswith("_T42_R7")}
    assert len(dumped) == 6
    run_goldens(names, dumped)


def test_mixed_sizes_in_one_batch():
    """surplus workgroups of the smaller members, the largest member's LDS, collections due at different
    ticks (n70 every ~26 ticks, n100 every ~12) in one call"""
    names = ["n20_single", "n20_multi_drop", "n50_multi_drop", "n70_single", "n100_single", "singlefailure_T42_R7",
             "msgdropsinglefailure_T42_R7"]
    run_goldens(names, {"singlefailure_T42_R7", "msgdropsinglefailure_T42_R7"})


def _final(sim):
    sent, recv = sim.msgcount(130)
    return sent.tobytes(), recv.tobytes(), sim.dump_tables(), sim.rand()


def test_interleaving_solo_calls_with_batch_ticks():
    seeds = {"A": (1001, 2002), "B": (77003, 91004)}  # outside the goldens' seed pairs

    def make(k):
        return Simulator(10, GM_MODE_FAITHFUL, 1, 0, 0.1, seeds[k][0], seeds[k][1])

    # batched: A is 5 ticks ahead, takes 3 solo ticks in the middle; B gets a crash in the middle
    a, b = make("A"), make("B")
    ev = {"A": [], "B": []}
    for _ in range(5):
        a.tick()
    batch = Batch([a, b])
    for _ in range(40):
        batch.tick()
        ev["A"] += a.drain_events()  # A drained every tick, B never
    for _ in range(3):
        a.tick()
    b.set_failed([3])
    while a.time < 130:
        batch.tick()
    assert (a.time, b.time) == (130, 122)
    ev["A"] += a.drain_events()
    ev["B"] += b.drain_events()
    got = {"A": _final(a), "B": _final(b)}
    batch.close()
    a.close()
    b.close()
    # the same per-member schedules on two solo contexts
    sa, sb = make("A"), make("B")
    want_ev = {"A": [], "B": []}
    for _ in range(130):
        sa.tick()
        want_ev["A"] += sa.drain_events()
    for _ in range(40):
        sb.tick()
    sb.set_failed([3])
    for _ in range(82):
        sb.tick()
    want_ev["B"] += sb.drain_events()
    want = {"A": _final(sa), "B": _final(sb)}
    for k in "AB":
        assert ev[k] == want_ev[k], f"{k}: records differ"
        for what, x, y in zip(("sent", "recv", "tables", "rand"), got[k], want[k]):
            assert x == y, f"{k}: {what} differs"
    assert len(ev["A"]) > 90 and len(ev["B"]) > 90  # the joins happened


def test_more_members_than_cus():
    """R = 260 members of N = 10 (gm_fb_recv takes a whole CU each: members past the CU count queue),
    30 batch ticks, against the CPU oracle: tables after the last tick, and the records as the log lines
    the oracle writes for them (its FAITHFUL record of events is its dbg.log)"""
    R, n, ticks = 260, 10, 30
    par = Params(n, 1, 0, 0.1)
    made = [new_cluster(par, s, s, 0) for s in range(1, R + 1)]
    batch = Batch([sim for _, sim in made])
    try:
        for _ in range(ticks):
            batch.tick()
        for s, (log, sim) in zip(range(1, R + 1), made):
            ora = oracle_py.Oracle(n, oracle_py.OC_FAITHFUL, 1, 0, 0.1, time_seed=s, rd_seed=s)
            for _ in range(ticks):
                ora.tick()
            assert sim.time == ora.time == ticks
            assert sim.dump_tables() == ora.dump(), f"seed {s}: tables"
            log_events(log, sim.drain_events())
            assert log.data() == ora.dbg(), f"seed {s}: records: " + first_diff(log.data(), ora.dbg())
            ora.close()
    finally:
        batch.close()
        for _, sim in made:
            sim.close()


def test_detection_recorder_in_a_batch():
    seeds = [(1, 1), (42, 7), (5, 9), (311, 12)]
    par = Params(10, 1, 0, 0.1)

    def solo(ts, rs):
        sim = Simulator(10, GM_MODE_FAITHFUL, 1, 0, 0.1, ts, rs)
        sim.detect_record(200)
        log = Log()
        for t in range(150):
            sim.tick()
            if t == 100:
                fail_step(par, sim, log, t)
        out = sim.detect(), sim.detect_timeline(200)
        sim.close()
        return out

    sims = [Simulator(10, GM_MODE_FAITHFUL, 1, 0, 0.1, ts, rs) for ts, rs in seeds]
    for s in sims:
        s.detect_record(200)
    batch = Batch(sims)
    logs = [Log() for _ in sims]
    for t in range(150):
        batch.tick()
        if t == 100:
            for s, log in zip(sims, logs):
                fail_step(par, s, log, t)
    for s, (ts, rs) in zip(sims, seeds):
        assert s.time == 150
        rec, tl = s.detect(), s.detect_timeline(200)
        wrec, wtl = solo(ts, rs)
        assert rec.tobytes() == wrec.tobytes(), f"seeds {ts, rs}: gm_detect"
        assert np.array_equal(tl, wtl), f"seeds {ts, rs}: gm_detect_timeline"
        assert (rec["fail_tick"] >= 0).sum() == 1 and rec["removals"].sum() == 9  # one crash, seen by the nine others
    batch.close()
    for s in sims:
        s.close()


def _create(lib, sims):
    arr = (ctypes.c_void_p * len(sims))(*[s.h for s in sims])
    h = ctypes.c_void_p()
    return lib.gm_batch_create(arr, len(sims), ctypes.byref(h)), h


def test_errors_and_all_or_nothing():
    lib = abi.load_library()
    f1 = Simulator(10, GM_MODE_FAITHFUL, 1, 0, 0.1, 9, 9)
    f2 = Simulator(10, GM_MODE_FAITHFUL, 1, 0, 0.1, 8, 8)
    sc = Simulator(256, GM_MODE_SCALED, rd_seed=7)
    rc, h = _create(lib, [f1, sc])
    assert rc == abi.GM_EUNSUPPORTED and not h.value
    rc, h = _create(lib, [f1, f2, f1])
    assert rc == abi.GM_EINVAL and not h.value
    sc.close()
    rc, h = _create(lib, [f1, f2])
    assert rc == abi.GM_OK and h.value
    rc2, h2 = _create(lib, [f2])
    assert rc2 == abi.GM_ESTATE and not h2.value
    assert lib.gm_destroy(f1.h) == abi.GM_ESTATE  # destroys nothing: the member goes on
    assert lib.gm_batch_tick(h) == abi.GM_OK
    f1.tick()
    f1.sync()
    assert (f1.time, f2.time) == (2, 1)
    assert lib.gm_batch_destroy(h) == abi.GM_OK
    f2.close()
    # a member at MAX_TIME: the batch tick refuses, and no member moves
    old = f1
    while old.time < 3600:
        old.tick()
    old.drain_events()
    with pytest.raises(GmError) as e:
        old.tick()
    assert e.value.code == abi.GM_ERANGE
    fresh = Simulator(10, GM_MODE_FAITHFUL, 1, 0, 0.1, 21, 22)
    for order in ([fresh, old], [old, fresh]):
        rc, h = _create(lib, order)
        assert rc == abi.GM_OK
        assert lib.gm_batch_tick(h) == abi.GM_ERANGE
        assert (old.time, fresh.time) == (3600, 0)
        assert lib.gm_batch_destroy(h) == abi.GM_OK
    # given back by gm_batch_destroy, the fresh member is a solo context like any other
    want = Simulator(10, GM_MODE_FAITHFUL, 1, 0, 0.1, 21, 22)
    for s in (fresh, want):
        for _ in range(30):
            s.tick()
    assert fresh.drain_events() == want.drain_events()
    assert fresh.dump_tables() == want.dump_tables()
    assert fresh.rand() == want.rand()
    for s in (old, fresh, want):
        s.close()
