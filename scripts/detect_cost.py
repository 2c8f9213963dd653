#!/usr/bin/env python3
"""Cost of the detection recorder (gm_detect_record) at S-A size, and its large-N check.

S-A as bench.py runs it: N = 65,536, warm start at t0 = 8, 655 nodes (crash_set(N, 655, 42))
crashed after tick 10, RD_SEED 7, event keeping off. Runs (one context each) with recording off
(the path without the reducer kernel) and on from the start are interleaved: off, on, off, on, off.

Timing is host wall-clock around synced work, because gm_last_kernel_ms brackets only the band
kernels and would hide the reducer:
  * ticks up to --until (default 42: the crash window and the TREMOVE sweep) one by one, each
    followed by gm_sync: the crash-window ticks (after the crash, before the first removal) and
    the two ticks with the most removals (the TREMOVE peak), per run;
  * then three windows of --steady ticks (default 20) enqueued back to back and synced once: the
    mean steady tick. A run that began with recording off then switches it ON in the same context
    and times three more windows.
The steady tick differs between otherwise equal contexts of one process by more than the reducer
costs (~0.07 ms, recording or not; within a context the windows repeat to ~0.001 ms), so the
steady cost is the same-context pair; the per-tick figures of different contexts carry that spread.

The runs that record from the start also assert what the single removal total of bench.py cannot
show: each of the 655 crashed nodes was removed exactly N - 655 = 64,881 times, and nobody else
was removed or joined.

  python scripts/detect_cost.py [--out profiles/detect/sa_cost.json]
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "distributed-membership_amd"))

import numpy as np  # noqa: E402

from membership import GM_MODE_SCALED, Simulator, crash_set, summarize  # noqa: E402

WINDOWS = 3


def steady_windows(sim, ticks):
    out = []
    for _ in range(WINDOWS):
        t0 = time.perf_counter()
        for _ in range(ticks):
            sim.tick()
        sim.sync()
        out.append((time.perf_counter() - t0) * 1e3 / ticks)
    return out


def one_run(a, record):
    n, ncrash = a.n, int(round(a.n * 0.01))
    sim = Simulator(n, GM_MODE_SCALED, rd_seed=7, init_mode=1, init_t0=8, init_seed=11)
    sim.keep_events(0)
    crash = crash_set(n, ncrash, 42)
    tmax = a.until + 2 * WINDOWS * a.steady + 1
    if record:
        sim.detect_record(tmax)
    sim.sync()
    per_tick = {}
    while sim.time <= a.until:
        t = sim.time
        t0 = time.perf_counter()
        sim.tick()
        sim.sync()
        per_tick[t] = (time.perf_counter() - t0) * 1e3
        if t == a.crash_tick:
            sim.set_failed(crash)
    out = {"record": record, "per_tick_ms": per_tick, "steady_ms": steady_windows(sim, a.steady)}
    if not record:  # the same context, the reducer switched on between two ticks
        sim.detect_record(tmax)
        out["steady_ms_switched_on"] = steady_windows(sim, a.steady)
        assert not sim.detect()["removals"].any() and not sim.detect_timeline(tmax).any()  # the sweep is over
    assert sim.tick_stats()["err"] == 0
    tot = sim.event_totals()
    assert tot["removed"] == (n - ncrash) * ncrash and tot["joined"] == 0, tot
    if record:
        rec = sim.detect()
        tl = sim.detect_timeline(tmax)
        crashed = np.zeros(n, dtype=bool)
        crashed[crash] = True
        # the large-N check: every crashed node removed by every live observer exactly once, nothing else
        assert (rec["removals"][crashed] == n - ncrash).all(), "a crashed node was not removed by every live observer"
        assert not rec["removals"][~crashed].any() and not rec["false_removals"].any() and not rec["joins"].any()
        assert (rec["fail_tick"][crashed] == a.crash_tick).all() and (rec["fail_tick"][~crashed] == -1).all()
        assert int(tl[:, 1].sum()) == (n - ncrash) * ncrash and not tl[:, 0].any() and not tl[:, 2].any()
        out["removals_per_tick"] = {int(t): int(tl[t, 1]) for t in np.flatnonzero(tl[:, 1])}
        out["summary"] = summarize(rec, crashed)
    sim.close()
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n", type=int, default=65536)
    p.add_argument("--crash-tick", type=int, default=10)
    p.add_argument("--until", type=int, default=42, help="last tick timed on its own (past the removal sweep)")
    p.add_argument("--steady", type=int, default=20, help="ticks per steady window")
    p.add_argument("--pattern", default="0,1,0,1,0",
                   help="the runs in order, 1 = recording from the start (at least one of each)")
    p.add_argument("--out", default=None)
    a = p.parse_args()
    runs = [one_run(a, record == "1") for record in a.pattern.split(",")]
    rem = next(r for r in runs if r["record"])["removals_per_tick"]
    assert max(rem) <= a.until, "the removal sweep runs past --until"
    peaks = sorted(sorted(rem, key=rem.get, reverse=True)[:2])
    window = list(range(a.crash_tick + 1, min(rem)))
    rnd = lambda xs: [round(x, 4) for x in xs]  # noqa: E731
    rows = []
    for r in runs:
        pt = r["per_tick_ms"]
        row = {"record": r["record"], "steady_ms": rnd(r["steady_ms"]),
               "crash_window_ms": round(float(np.mean([pt[t] for t in window])), 4),
               "peak_ms": {t: round(pt[t], 4) for t in peaks}}
        if "steady_ms_switched_on" in r:
            row["steady_ms_switched_on"] = rnd(r["steady_ms_switched_on"])
            row["switched_on_minus_off_ms"] = round(float(np.mean(r["steady_ms_switched_on"]) - np.mean(r["steady_ms"])), 4)
        rows.append(row)
    off = [np.mean(r["steady_ms"]) for r in rows if not r["record"]]
    res = {"n": a.n, "crashed": int(round(a.n * 0.01)), "crash_tick": a.crash_tick, "steady_ticks": a.steady,
           "crash_window_ticks": [window[0], window[-1]], "peak_ticks": peaks, "removals_per_tick": rem,
           "runs": rows,
           "steady_off_between_contexts_ms": rnd([min(off), max(off)]),
           "steady_same_context_on_minus_off_ms": [r["switched_on_minus_off_ms"] for r in rows if not r["record"]],
           "summary": next(r for r in runs if r["record"])["summary"],
           "per_tick_ms": [{"record": r["record"], "ms": {t: round(v, 4) for t, v in r["per_tick_ms"].items()}}
                           for r in runs]}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps({k: v for k, v in res.items() if k != "per_tick_ms"}))


if __name__ == "__main__":
    main()
