#!/usr/bin/env python3
"""Cost of the view-graph walks (gm_view_reach) at S-C size, beside the census and the view copy.

S-C as bench.py runs it: N = 16,777,216, V = 32, warm start at t0 = 8, 5 % per-entry loss on every
tick, RD_SEED 7, event keeping off. One context, three states:
  * a steady tick (9),
  * the tick after bench.py's 1 % crash (crash_set(N, N / 100, 42) after tick 10; tick 11),
  * a few ticks after a half-cluster crash (crash_set(N, N / 2, 42) after tick 14, on top of the
    1 %; tick 18).
On each state, host wall-clock around synced calls (gm_sync, then the call; every call measured returns
after its own copies), --reps calls each with every run listed:
  reach_{out,in}_{1,64}_ms  gm_view_reach from 1 source and from 64 (live nodes drawn by a seeded rng,
                            node 0 or the first live node first), seen = NULL, max_hops = GM_VIEW_HOPS;
                            with the hops run, the levels and the smallest / largest reach
  reach_in_64_seen_ms       the same with the seen words copied back (8 N bytes)
  census_norec_ms           gm_view_census with out = NULL: one pass over the live views (the yardstick)
  read_views_copy_ms        gm_read_views of all N nodes into one host buffer: the copy a host-side
                            BFS would need before its first hop (the other yardstick)
and what the walks say: summarize_reach of the 64-source pair.

  python scripts/view_reach_cost.py [--out profiles/view_reach/sc_cost.json]
"""
import argparse
import ctypes
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "distributed-membership_amd"))

import numpy as np  # noqa: E402

from membership import GM_MODE_PARTIAL, Simulator, crash_set, summarize_reach  # noqa: E402


def timed(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return r, [round(x, 3) for x in out]


def measure(sim, a, what, crashed, buf):
    n, t = sim.n, sim.time - 1
    live_nodes = np.flatnonzero(~crashed)
    rng = np.random.default_rng(1)
    src = live_nodes[rng.integers(0, len(live_nodes), size=64)].astype(np.int32)
    src[0] = live_nodes[0]
    sim.sync()
    row = {"what": what, "tick": t, "live": int(len(live_nodes))}
    walks = {}
    for d in ("out", "in"):
        for k in (1, 64):
            w, ms = timed(lambda: sim.view_reach(src[:k], d), a.reps)
            reached = w["counts"].sum(axis=0)
            assert w["live"] == len(live_nodes) and w["live_sources"] == k and not w["stopped"]
            assert (w["counts"][0] == 1).all() and (reached <= w["live"]).all()
            row[f"reach_{d}_{k}_ms"] = ms
            row[f"reach_{d}_{k}"] = {"hops": w["hops"], "reached_min": int(reached.min()), "reached_max": int(reached.max()),
                                     "levels_source0": [int(x) for x in w["counts"][:w["hops"] + 1, 0]]}
            walks[d, k] = w
    w, row["reach_in_64_seen_ms"] = timed(lambda: sim.view_reach(src, "in", seen=True), a.reps)
    assert np.array_equal(w["counts"], walks["in", 64]["counts"])
    assert not w["seen"][crashed].any() and (w["seen"][src] != 0).all()
    del w
    s = summarize_reach(walks["out", 64], walks["in", 64])
    row["strongly_connected"] = s["strongly_connected"]
    row["unreached_out"] = sorted({x["unreached"] for x in s["out"]["sources"]})[:8]
    row["unreached_in"] = sorted({x["unreached"] for x in s["in"]["sources"]})[:8]
    for d in ("out", "in"):  # over the sources that reach anybody
        md = [x["mean_distance"] for x in s[d]["sources"] if x["mean_distance"] is not None]
        row[f"mean_distance_{d}"] = round(float(np.mean(md)), 3) if md else None
    (_, hist, sizes), row["census_norec_ms"] = timed(lambda: sim.view_census(records=False), a.reps)
    assert int(sizes.sum()) == len(live_nodes)
    u64p = ctypes.POINTER(ctypes.c_uint64)

    def copy_all():
        assert sim.lib.gm_read_views(sim.h, 0, n, buf.ctypes.data_as(u64p)) == 0
    _, row["read_views_copy_ms"] = timed(copy_all, a.reps)
    hops = row["reach_in_64"]["hops"]
    row["in_64_over_hops_x_census"] = round(min(row["reach_in_64_ms"]) / (max(hops, 1) * min(row["census_norec_ms"])), 3)
    return row


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n", type=int, default=1 << 24)
    p.add_argument("--view", type=int, default=32)
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    n, v = a.n, a.view
    sim = Simulator(n, GM_MODE_PARTIAL, rd_seed=7, view=v, view_seed=5, init_mode=1, init_t0=8, init_seed=11,
                    drop_pct=5, drop_from=0, drop_to=1 << 20, drop_seed=42)
    sim.keep_events(0)
    crashes = {10: crash_set(n, int(round(n * 0.01)), 42), 14: crash_set(n, n // 2, 42)}
    crashed = np.zeros(n, dtype=bool)
    buf = np.zeros((n, v), dtype=np.uint64)
    names = {9: "steady", 11: "the tick after the 1 % crash", 18: "4 ticks after the half-cluster crash"}
    rows = []
    while sim.time <= max(names):
        t = sim.time
        sim.tick()
        if t in crashes:
            sim.set_failed(crashes[t])
            crashed[crashes[t]] = True
        if t in names:
            rows.append(measure(sim, a, names[t], crashed, buf))
            print(json.dumps(rows[-1]), flush=True)
    assert sim.tick_stats()["err"] == 0
    sim.close()
    res = {"n": n, "view": v, "reps": a.reps, "stored_view_bytes": n * v * 8, "word_array_bytes": n * 8, "measured": rows}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
