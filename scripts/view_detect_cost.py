#!/usr/bin/env python3
"""Cost of the PARTIAL detection recorder (gm_view_detect_record) at S-C size, and its full-size
self-check.

S-C as bench.py runs it: N = 16,777,216, V = 32, warm start at t0 = 8, 5 % per-entry loss on every
tick, RD_SEED 7, event keeping off; 1 % of the nodes (crash_set(N, N / 100, 42)) crash after tick
--crash-tick, so the timed window of --ticks ticks that follows covers the fade. The same seeded
window runs in a fresh context per leg:

  off      recorder off
  on       recorder on from the window's first tick (one reducer launch per tick)
  census   recorder off, one gm_view_census with records after every tick: the way to a fade curve
           without the recorder
  off2     recorder off again: the run-to-run spread of `off`

Per leg: host wall-clock ms per tick (gm_tick + gm_sync; the census leg's figure includes its census)
and the tick-kernel ms of gm_set_timing (gm_last_kernel_ms: the span from the node kernels' start to
their end, which holds the reducer while recording). The reducer's own time is the difference of
that span between `on` and `off`. It is reported as a multiple of the floor -- one streaming pass over
the N x V x 8 bytes of lists at 6.0 TB/s, the rate an in-order sweep of HBM reaches on this part --
and as a share of the recorder-off tick.

Self-checks at full size: the recorder's `held` of every window tick equals the census leg's holders
summed over the crashed subjects at that tick; per crashed subject, a holder at the last tick means
last_held is that tick; held_sum adds up to the held column.

--legs off runs on a library without the recorder too (the parent commit's, through GM_LIBRARY and
GM_AB_BUILD=1): the no-regression leg.

  python scripts/view_detect_cost.py [--out profiles/view_detect/sc_cost.json]
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "distributed-membership_amd"))

import numpy as np  # noqa: E402

from membership import GM_MODE_PARTIAL, Simulator, crash_set  # noqa: E402

HBM_SWEEP_BPS = 6.0e12  # achieved by an in-order sweep of a table far larger than the caches


def leg(a, what, crash):
    n, v = a.n, a.view
    sim = Simulator(n, GM_MODE_PARTIAL, rd_seed=7, view=v, view_seed=5, init_mode=1, init_t0=8, init_seed=11,
                    drop_pct=5, drop_from=0, drop_to=1 << 20, drop_seed=42)
    sim.keep_events(0)
    while sim.time <= a.crash_tick:
        sim.tick()
    sim.set_failed(crash)
    first, last = sim.time, sim.time + a.ticks - 1
    if what == "on":
        sim.view_detect_record(last + 1)
    sim.sync()
    sim.set_timing(True)
    ms, held = [], []
    while sim.time <= last:
        t0 = time.perf_counter()
        sim.tick()
        sim.sync()
        if what == "census":
            holders = sim.view_census()[0]["holders"]
            held.append(int(holders[crash].sum()))
        ms.append((time.perf_counter() - t0) * 1e3)
    row = {"leg": what, "first_tick": first, "last_tick": last, "tick_ms": [round(x, 3) for x in ms],
           "tick_ms_mean": round(float(np.mean(ms)), 4), "tick_ms_median": round(float(np.median(ms)), 4),
           "kernel_ms": round(sim.last_kernel_ms(), 4)}
    sim.set_timing(False)
    if what == "census":
        row["held"] = held
    if what == "on":
        tl = sim.view_detect_timeline(last + 1)
        rec = sim.view_detect()
        holders = sim.view_census()[0]["holders"]
        row["held"] = [int(x) for x in tl[first:, 3]]
        row["late_joins"] = [int(x) for x in tl[first:, 4]]
        row["removals"] = int(tl[:, 1].sum())
        assert int(holders[crash].sum()) == row["held"][-1], "the last tick's held is not the census' holders"
        assert (rec["last_held"][crash][holders[crash] > 0] == last).all(), "a held subject whose last_held is older"
        assert int(rec["held_sum"].sum()) == int(tl[:, 3].sum()) and not tl[:first].any()
        assert (rec["fail_tick"][crash] == a.crash_tick).all()
    assert sim.tick_stats()["err"] == 0
    sim.close()
    print(json.dumps(row), flush=True)
    return row


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n", type=int, default=1 << 24)
    p.add_argument("--view", type=int, default=32)
    p.add_argument("--crash-tick", type=int, default=10)
    p.add_argument("--ticks", type=int, default=12)
    p.add_argument("--legs", default="off,on,census,off2")
    p.add_argument("--out", default=None)
    a = p.parse_args()
    crash = crash_set(a.n, int(round(a.n * 0.01)), 42)
    rows = {}
    for what in a.legs.split(","):
        rows[what] = leg(a, "off" if what == "off2" else what, crash)
        rows[what]["leg"] = what
    res = {"n": a.n, "view": a.view, "crashed": len(crash), "list_bytes": a.n * a.view * 8, "legs": rows}
    floor_ms = res["list_bytes"] / HBM_SWEEP_BPS * 1e3
    res["floor_ms"] = round(floor_ms, 4)
    if "on" in rows and "off" in rows:
        off_k = [rows[k]["kernel_ms"] for k in ("off", "off2") if k in rows]
        red = rows["on"]["kernel_ms"] - float(np.mean(off_k))
        res["reducer_kernel_ms"] = round(red, 4)
        res["reducer_over_floor"] = round(red / floor_ms, 2)
        res["reducer_share_of_off_tick"] = round(red / float(np.mean([rows[k]["tick_ms_mean"] for k in ("off", "off2") if k in rows])), 4)
        res["off_kernel_ms_spread"] = round(max(off_k) - min(off_k), 4)
    if "on" in rows and "census" in rows:
        assert rows["on"]["held"] == rows["census"]["held"], "the recorded fade is not the censused one"
        res["fade_equals_census"] = True
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps({k: val for k, val in res.items() if k != "legs"}))


if __name__ == "__main__":
    main()
