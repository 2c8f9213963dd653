#!/usr/bin/env python3
"""Cost of the state digest (gm_digest, the per-tick recorder) at full size, and the full-size checks
no test can afford.

S-A as bench.py runs it: N = 65,536, warm start at t0 = 8, 1 % (crash_set(N, 655, 42)) crashed after
tick 10, RD_SEED 7, event keeping off, ticked to 48. Three such runs, one after the other, each with
digest_record(64): the default layout (band 1024, the fast path), GM_BAND_FAST=0 (band 1024, the general
path) and band 512. Their traces must be equal row by row; the first differing tick is reported.

Host wall-clock around synced calls (gm_sync, then the call), --reps calls each: gm_digest and, beside
it on the same tick of the same context, gm_census (the parent's kernels: the yardstick), at a steady
tick (9), a crash-window tick (26), the TREMOVE tick with the most removals (found in run 1, measured
in run 2) and tick 2 of a cold start. Reported: the times, their ratio and the stored table's bytes per
second of digest.

The recorded tick against the unrecorded one: in one context, a window of --steady ticks past the
recorder's tmax (nothing recorded) and a window inside it, each tick followed by gm_sync and timed on its
own; a second context takes the windows in the other order.

S-C (--sc-n nodes, V = 32, 5 % loss, 1 % crashed after tick 14): gm_digest beside gm_view_census on a steady
tick, and the trace of one context over 12 ticks against the added traces of G = 8 loopback row shards.

  python scripts/digest_cost.py [--out profiles/digest/cost.json]
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "distributed-membership_amd"))

import numpy as np  # noqa: E402

from membership import GM_MODE_PARTIAL, GM_MODE_SCALED, Simulator, crash_set  # noqa: E402
from membership.abi import partial_loopback_tick  # noqa: E402


def timed(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return r, [round(x, 4) for x in out]


def beside(sim, what, reps, state_bytes, yardstick, name):
    """gm_digest and the census of the same tick of the same context"""
    sim.sync()
    d, dms = timed(sim.digest, reps)
    _, sms = timed(lambda: sim.digest(rows=False, nodes=False), reps)  # the sums alone: no N x 16 B copy
    _, cms = timed(yardstick, reps)
    return d, {"what": what, "tick": sim.time - 1, "digest_ms": dms, "digest_sums_only_ms": sms, name + "_ms": cms,
               "digest_over_" + name: round(min(sms) / min(cms), 3),
               "state_GBps": round(state_bytes / (min(sms) * 1e-3) / 1e9, 1),
               "table": f"{d['table']:016x}", "nodes": f"{d['nodes']:016x}"}


def window(sim, ticks):
    tot = 0.0
    for _ in range(ticks):
        t0 = time.perf_counter()
        sim.tick()
        sim.sync()
        tot += time.perf_counter() - t0
    return round(tot * 1e3 / ticks, 4)


def sa_run(a, label, band, env, measure_at, until=48):
    """one S-A run with the recorder on; returns (trace [until + 1][2], rows measured, removals per tick, sim)"""
    for k, v in env.items():
        os.environ[k] = v
    n, ncrash = a.n, int(round(a.n * 0.01))
    table_bytes = n * ((n + 511) // 512 * 512)
    sim = Simulator(n, GM_MODE_SCALED, rd_seed=7, init_mode=1, init_t0=8, init_seed=11, band=band)
    for k in env:
        del os.environ[k]
    sim.keep_events(0)
    sim.digest_record(64)
    crash = crash_set(n, ncrash, 42)
    rows, removed_at, last = [], {}, 0
    while sim.time <= until:
        t = sim.time
        sim.tick()
        tot = sim.event_totals()["removed"]
        if tot != last:
            removed_at[t] = tot - last
            last = tot
        if t in measure_at:
            d, row = beside(sim, f"{label}: {measure_at[t]}", a.reps, table_bytes, lambda: sim.census(records=False), "census")
            tr = sim.digest_trace(t + 1)[t]
            assert (int(tr[0]), int(tr[1])) == (d["table"], d["nodes"]), "the recorded row is not the digest on demand"
            rows.append(row)
        if t == 10:
            sim.set_failed(crash)
    assert sim.tick_stats()["err"] == 0
    return sim.digest_trace(until + 1), rows, removed_at, sim


def recorded_pairs(a, sim, first_recorded):
    """two windows of a.steady ticks in one steady context, one recorded and one not"""
    out = {}
    t = sim.time
    if first_recorded:
        sim.digest_record(t + a.steady)
        out["recorded_ms"], out["plain_ms"] = window(sim, a.steady), window(sim, a.steady)
    else:
        out["plain_ms"] = window(sim, a.steady)
        sim.digest_record(sim.time + a.steady)
        out["recorded_ms"] = window(sim, a.steady)
    out["order"] = "recorded, plain" if first_recorded else "plain, recorded"
    out["diff_ms"] = round(out["recorded_ms"] - out["plain_ms"], 4)
    return out


def steady_context(n):
    sim = Simulator(n, GM_MODE_SCALED, rd_seed=7, init_mode=1, init_t0=8, init_seed=11)
    sim.keep_events(0)
    for _ in range(12):
        sim.tick()
    sim.sync()
    return sim


def sc_part(a):
    n, v, world, ticks = a.sc_n, 32, 8, 12
    kw = dict(rd_seed=7, view=v, view_seed=5, init_mode=1, init_t0=8, init_seed=11, drop_pct=5, drop_from=0,
              drop_to=1 << 20, drop_seed=42)
    crash = crash_set(n, int(round(n * 0.01)), 42)
    one = Simulator(n, GM_MODE_PARTIAL, **kw)
    one.keep_events(0)
    plain = window(one, 3)  # ticks 9..11 unrecorded
    one.digest_record(64)
    first = one.time
    rec_ms = []
    measured = None
    for _ in range(ticks):
        t = one.time
        rec_ms.append(window(one, 1))
        if t == first + 2:
            one.set_failed(crash)
        if t == first + 8:
            _, measured = beside(one, "S-C steady", a.reps, 8 * n * v, lambda: one.view_census(records=False), "view_census")
    last = one.time
    want = one.digest_trace(last)
    one.close()
    shards = [Simulator(n, GM_MODE_PARTIAL, shard_rank=g, shard_count=world, **kw) for g in range(world)]
    for s in shards:
        s.keep_events(0)
    while shards[0].time < first:
        partial_loopback_tick(shards)
    for s in shards:
        s.digest_record(64)
    while shards[0].time < last:
        t = shards[0].time
        partial_loopback_tick(shards)
        if t == first + 2:
            for s in shards:
                s.set_failed(crash)
    with np.errstate(over="ignore"):
        got = np.add.reduce([s.digest_trace(last) for s in shards], dtype=np.uint64)
    differ = [int(t) for t in np.flatnonzero((got != want).any(axis=1))]
    return {"n": n, "view": v, "measured": measured, "plain_tick_ms": plain, "recorded_tick_ms": rec_ms,
            "row_shards": world, "ticks_compared": [first, last - 1], "traces_equal": not differ,
            "first_differing_tick": differ[0] if differ else None,
            "trace_last_row": [f"{int(x):016x}" for x in want[last - 1]]}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n", type=int, default=65536)
    p.add_argument("--sc-n", type=int, default=1 << 24)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--steady", type=int, default=20, help="ticks per window of the recorded / plain pairs")
    p.add_argument("--no-cold", action="store_true")
    p.add_argument("--no-sc", action="store_true")
    p.add_argument("--out", default=None)
    a = p.parse_args()
    n = a.n
    table_bytes = n * ((n + 511) // 512 * 512)
    res = {"n": n, "table_bytes": table_bytes, "reps": a.reps, "measured": [], "runs": []}

    def flush():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(json.dumps(res, indent=1) + "\n")

    tr1, rows, removed_at, sim = sa_run(a, "band 1024 fast path", 0, {}, {9: "steady", 26: "crash window"})
    sim.close()
    res["measured"] += rows
    res["removals_per_tick"] = removed_at
    peak = max(removed_at, key=removed_at.get)
    flush()
    tr2, rows, _, sim = sa_run(a, "band 1024 general path", 0, {"GM_BAND_FAST": "0"}, {peak: "TREMOVE peak"})
    sim.close()
    res["measured"] += rows
    tr3, rows, _, sim = sa_run(a, "band 512", 512, {}, {9: "steady"})
    sim.close()
    res["measured"] += rows
    names = ["band 1024 fast path", "band 1024 general path (GM_BAND_FAST=0)", "band 512"]
    for name, tr in zip(names, (tr1, tr2, tr3)):
        differ = [int(t) for t in np.flatnonzero((tr != tr1).any(axis=1))]
        res["runs"].append({"layout": name, "ticks": [9, 48], "rows_recorded": int(tr.any(axis=1).sum()),
                            "equal_to_first": not differ, "first_differing_tick": differ[0] if differ else None,
                            "row_48": [f"{int(x):016x}" for x in tr[48]]})
    res["traces_equal"] = all(r["equal_to_first"] for r in res["runs"])
    flush()
    res["recorded_pairs"] = []
    for first_recorded in (True, False):
        sim = steady_context(n)
        res["recorded_pairs"].append(recorded_pairs(a, sim, first_recorded))
        sim.close()
    flush()
    if not a.no_cold:
        cold = Simulator(n, GM_MODE_SCALED, rd_seed=7, init_mode=0)
        cold.keep_events(0)
        cold.tick()
        cold.tick()
        _, row = beside(cold, "cold start", a.reps, table_bytes, lambda: cold.census(records=False), "census")
        res["measured"].append(row)
        cold.close()
        flush()
    if not a.no_sc:
        res["sc"] = sc_part(a)
        flush()
    print(json.dumps(res))
    if not res["traces_equal"] or (not a.no_sc and not res["sc"]["traces_equal"]):
        sys.exit(3)


if __name__ == "__main__":
    main()
