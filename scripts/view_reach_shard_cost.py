#!/usr/bin/env python3
"""Cost of the view-graph walk across row shards (gm_view_reach_loopback) at S-C size, beside the
single-context walk (gm_view_reach) on the same state in the same run.

S-C as bench.py runs it: N = 16,777,216, V = 32, warm start at t0 = 8, 5 % per-entry loss on every
tick, RD_SEED 7, event keeping off. One context and a loopback group of --shards row shards (8) on one
device, ticked side by side through the three states of profiles/view_reach/sc_cost.json:
  * a steady tick (9),
  * the tick after bench.py's 1 % crash (crash_set(N, N / 100, 42) after tick 10; tick 11),
  * four ticks after a half-cluster crash (crash_set(N, N / 2, 42) after tick 14, on top of the 1 %;
    tick 18).
On each state, host wall-clock around synced calls, --reps calls each with every run listed, 64 sources
(view_reach_cost.py's: live nodes drawn by a seeded rng, the first live node first), seen = NULL,
max_hops = GM_VIEW_HOPS:
  group_{out,in}_ms   the walk of the group
  one_{out,in}_ms     the walk of the single context
and, from one more call of each with the seen words copied back, the check that counts, the numbers
and seen are identical. levels: the levels run; exchange_bytes_per_level: what one member receives per
level (8 bytes per node of the other shards: the gathered front slices going IN, its slice of every
other member's proposals going OUT) and the group's total.

A loopback group runs its shards one after the other on one device and copies where G devices would
run side by side and send: group time / G is a projection, not a measured G-GPU figure.

  python scripts/view_reach_shard_cost.py [--out profiles/view_reach/shard_cost.json]
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "distributed-membership_amd"))

import numpy as np  # noqa: E402

from membership import GM_MODE_PARTIAL, Simulator, crash_set, summarize_reach  # noqa: E402
from membership.abi import partial_loopback_tick, partial_loopback_view_reach  # noqa: E402


def timed(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return r, [round(x, 3) for x in out]


def measure(one, group, a, what, crashed):
    n, t, world = one.n, one.time - 1, len(group)
    live_nodes = np.flatnonzero(~crashed)
    rng = np.random.default_rng(1)
    src = live_nodes[rng.integers(0, len(live_nodes), size=64)].astype(np.int32)
    src[0] = live_nodes[0]
    for s in [one] + group:
        s.sync()
    row = {"what": what, "tick": t, "live": int(len(live_nodes)), "shards": world}
    walks = {}
    for d in ("out", "in"):
        g, row[f"group_{d}_ms"] = timed(lambda: partial_loopback_view_reach(group, src, d), a.reps)
        o, row[f"one_{d}_ms"] = timed(lambda: one.view_reach(src, d), a.reps)
        assert np.array_equal(g["counts"], o["counts"]), f"{what}, {d}: counts differ"
        gs, os_ = partial_loopback_view_reach(group, src, d, seen=True), one.view_reach(src, d, seen=True)
        for key in gs:
            assert np.array_equal(gs[key], os_[key]), f"{what}, {d}: {key} differs"
        assert not gs["seen"][crashed].any() and g["live"] == len(live_nodes) and not g["stopped"]
        del gs, os_
        row[f"levels_{d}"] = g["hops"]
        row[f"group_over_one_{d}"] = round(min(row[f"group_{d}_ms"]) / min(row[f"one_{d}_ms"]), 3)
        row[f"group_{d}_ms_over_shards"] = round(min(row[f"group_{d}_ms"]) / world, 3)
        walks[d] = g
    s = summarize_reach(walks["out"], walks["in"])
    row["strongly_connected"] = s["strongly_connected"]
    row["unreached_out"] = sorted({x["unreached"] for x in s["out"]["sources"]})[:8]
    row["unreached_in"] = sorted({x["unreached"] for x in s["in"]["sources"]})[:8]
    row["identical_to_one_context"] = True
    return row


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n", type=int, default=1 << 24)
    p.add_argument("--view", type=int, default=32)
    p.add_argument("--shards", type=int, default=8)
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    n, v, world = a.n, a.view, a.shards
    kw = dict(rd_seed=7, view=v, view_seed=5, init_mode=1, init_t0=8, init_seed=11, drop_pct=5, drop_from=0,
              drop_to=1 << 20, drop_seed=42)
    one = Simulator(n, GM_MODE_PARTIAL, **kw)
    group = [Simulator(n, GM_MODE_PARTIAL, shard_rank=g, shard_count=world, **kw) for g in range(world)]
    for s in [one] + group:
        s.keep_events(0)
    crashes = {10: crash_set(n, int(round(n * 0.01)), 42), 14: crash_set(n, n // 2, 42)}
    crashed = np.zeros(n, dtype=bool)
    names = {9: "steady", 11: "the tick after the 1 % crash", 18: "4 ticks after the half-cluster crash"}
    rows = []
    while one.time <= max(names):
        t = one.time
        one.tick()
        partial_loopback_tick(group)
        if t in crashes:
            for s in [one] + group:
                s.set_failed(crashes[t])
            crashed[crashes[t]] = True
        if t in names:
            rows.append(measure(one, group, a, names[t], crashed))
            print(json.dumps(rows[-1]), flush=True)
    if n == 1 << 24 and v == 32:  # what the single-context run found (profiles/view_reach/sc_cost.json)
        assert rows[-1]["unreached_out"] == [89] and rows[-1]["strongly_connected"] is False
    for s in [one] + group:
        assert s.tick_stats()["err"] == 0
    nloc = [s.shard_layout()[1] for s in group]
    per_member = [8 * (n - w) for w in nloc]  # IN: the other shards' front slices; OUT: G - 1 slices of its own size
    res = {"n": n, "view": v, "shards": world, "reps": a.reps, "word_array_bytes": n * 8,
           "exchange_bytes_per_level": {"per_member_in": per_member, "per_member_out": [8 * (world - 1) * w for w in nloc],
                                        "group": int(sum(per_member))},
           "scratch_bytes_per_member": [8 * (3 * w + n + max(n - w, (world - 1) * w) + 64 * 64 + 1) + 256 for w in nloc],
           "measured": rows}
    for s in [one] + group:
        s.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
