#!/usr/bin/env python3
"""Cost of the membership census (gm_census) at S-A size, and its full-size self-check.

S-A as bench.py runs it: N = 65,536, warm start at t0 = 8, 655 nodes (crash_set(N, 655, 42)) crashed
after tick 10, RD_SEED 7, event keeping off. Host wall-clock around synced calls (gm_sync, then the
call; gm_census returns after its own copies), --reps calls each, at
  * a steady tick (9, before the crash),
  * a crash-window tick (26: the crashed nodes' entries are in escape lists),
  * the TREMOVE tick with the most removals (from the event totals), and a steady tick after the sweep,
  * tick 2 of a cold start in a second context (every cell but the own entries escaped).
Beside each time: the stored table's bytes (N x padded row) divided by it -- the floor is one pass
over the table -- and the time of the route the census replaces, read_table of 256 rows (which
copies the whole table to the host for any row count).

Unperturbed run: in one context, windows of --steady ticks, each tick followed by gm_sync and timed on
its own, alternately with nothing and with an (untimed) census between the ticks.

Self-check at every measured tick: holders.sum() == hist.sum(), and the totals a warm S-A run must
show exactly -- before the crash every node holds every node; in the crash window every live node
still holds everyone, the crashed subjects' entries all stale; after the sweep the crashed subjects
have no holder and no record of them is left.

  python scripts/census_cost.py [--out profiles/census/sa_cost.json]
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "distributed-membership_amd"))

import numpy as np  # noqa: E402

from membership import GM_MODE_SCALED, Simulator, crash_set, summarize_census  # noqa: E402


def timed(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return r, out


def measure(sim, a, what, table_bytes, host_route=True):
    sim.sync()
    (rec, hist), ms = timed(sim.census, a.reps)
    assert int(rec["holders"].sum()) == int(hist.sum()), "holders and histogram cells differ"
    row = {"what": what, "tick": sim.time - 1, "census_ms": [round(x, 4) for x in ms],
           "table_GBps": round(table_bytes / (min(ms) * 1e-3) / 1e9, 1), "cells": int(hist.sum())}
    if host_route:
        _, hms = timed(lambda: sim.read_table(sim.n // 3, 256), 1)
        row["read_table_256_rows_ms"] = round(hms[0], 1)
    return rec, hist, row


def window(sim, ticks, census):
    tot = 0.0
    for _ in range(ticks):
        t0 = time.perf_counter()
        sim.tick()
        sim.sync()
        tot += time.perf_counter() - t0
        if census:
            sim.census()
    return tot * 1e3 / ticks


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n", type=int, default=65536)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--steady", type=int, default=20, help="ticks per window of the unperturbed-run pairs")
    p.add_argument("--no-cold", action="store_true")
    p.add_argument("--out", default=None)
    a = p.parse_args()
    n, ncrash = a.n, int(round(a.n * 0.01))
    live = n - ncrash
    table_bytes = n * ((n + 511) // 512 * 512)
    sim = Simulator(n, GM_MODE_SCALED, rd_seed=7, init_mode=1, init_t0=8, init_seed=11)
    sim.keep_events(0)
    crash = crash_set(n, ncrash, 42)
    crashed = np.zeros(n, dtype=bool)
    crashed[crash] = True
    rows, summaries, removed_at = [], {}, {}
    last_removed = 0
    while sim.time <= 45:
        t = sim.time
        sim.tick()
        if t == 10:
            sim.set_failed(crash)
        tot = sim.event_totals()["removed"]
        if tot != last_removed:
            removed_at[t] = tot - last_removed
            last_removed = tot
        if t in (9, 26, 45):
            what = {9: "steady", 26: "crash window", 45: "steady after the sweep"}[t]
            rec, hist, row = measure(sim, a, what, table_bytes)
            failed = crashed if t > 10 else np.zeros(n, dtype=bool)
            if t == 9:
                assert (rec["holders"] == n).all() and not hist[1].any()
            if t == 26:
                assert (rec["holders"] == live).all() and (rec["stale"][crashed] == live).all()
                assert int(hist[1].sum()) == live * ncrash and not hist[1, :15].any()
            if t == 45:
                assert (rec["holders"][~crashed] == live).all() and not rec["holders"][crashed].any()
                assert (rec["hb_min"][crashed] == -1).all() and not hist[1].any()
            rows.append(row)
            summaries[what] = summarize_census(rec, hist, failed, t)
    assert last_removed == live * ncrash, "the sweep is not over at tick 45"
    peak = max(removed_at, key=removed_at.get)
    # the TREMOVE peak again, in the same context: a census of tick `peak` needs a second pass through
    # the schedule, so it is taken in a fresh context below; here: the unperturbed-run pairs
    pairs = []
    for _ in range(3):
        off = window(sim, a.steady, False)
        on = window(sim, a.steady, True)
        pairs.append({"plain_ms": round(off, 4), "with_census_ms": round(on, 4), "diff_ms": round(on - off, 4)})
    assert sim.tick_stats()["err"] == 0
    sim.close()
    sim = Simulator(n, GM_MODE_SCALED, rd_seed=7, init_mode=1, init_t0=8, init_seed=11)
    sim.keep_events(0)
    while sim.time <= peak:
        t = sim.time
        sim.tick()
        if t == 10:
            sim.set_failed(crash)
    rec, hist, row = measure(sim, a, "TREMOVE peak", table_bytes)
    assert 0 < int(rec["holders"][crashed].sum()) < live * ncrash and (rec["holders"][~crashed] == live).all()
    row["removals_this_tick"] = removed_at[peak]
    rows.append(row)
    summaries["TREMOVE peak"] = summarize_census(rec, hist, crashed, peak)
    sim.close()
    if not a.no_cold:
        cold = Simulator(n, GM_MODE_SCALED, rd_seed=7, init_mode=0)
        cold.keep_events(0)
        cold.tick()
        cold.tick()
        rec, hist, row = measure(cold, a, "cold start", table_bytes, host_route=False)
        assert (rec["holders"] == n).all()
        rows.append(row)
        summaries["cold start"] = summarize_census(rec, hist, np.zeros(n, dtype=bool), 2)
        cold.close()
    res = {"n": n, "crashed": ncrash, "table_bytes": table_bytes, "reps": a.reps, "measured": rows,
           "removals_per_tick": removed_at, "unperturbed_pairs": pairs, "summaries": summaries}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps({k: v for k, v in res.items() if k != "summaries"}))


if __name__ == "__main__":
    main()
