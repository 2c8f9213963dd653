#!/usr/bin/env python3
"""Cost of a full S-C save and restore (gm_read_views / gm_load_views_*), and its full-size self-check.

S-C as bench.py runs it: N = 16,777,216, V = 32, warm start at t0 = 8, 5 % per-entry loss on every
tick, 1 % of the nodes (crash_set(N, N / 100, 42)) crashed after tick 10, RD_SEED 7, event keeping
off. The source context runs to tick --at; then, host wall-clock around synced calls:
  read_views_ms     gm_read_views of all N nodes in staging-size blocks (256 MiB / 8V nodes) into one
                    host array (allocated and touched before): the save
  nodes_ms          gm_read_nodes + gm_read_targets
  begin_ms          gm_load_views_begin on a fresh context (settles, allocates the staging buffer)
  load_views_ms     gm_load_views of the same rows in the same blocks, with gm_set_timing on:
                    check_ms / store_ms are the two kernels by HIP events (gm_load_views_stats)
  commit_ms         gm_load_views_commit (node arrays staged, gm_pl_nodes twice, gm_pl_inbox)
  shards            the same state into G = --shards loopback row shards: their loads (sum), the first
                    tick (which replays the exchange of the tick before) and the second tick (plain);
                    replay_ms is their difference
Self-check: the restored context and the shards tick --follow ticks beside the source; the view census
(hist, sizes; the shards' summed) is equal after every tick and the views of the first --slice nodes
are equal at the end.

  python scripts/load_views_cost.py [--out profiles/load_views]
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "distributed-membership_amd"))

import numpy as np  # noqa: E402

from membership import GM_MODE_PARTIAL, Simulator, crash_set, state  # noqa: E402
from membership.abi import partial_loopback_tick  # noqa: E402


def ms(fn):
    t0 = time.perf_counter()
    r = fn()
    return r, round((time.perf_counter() - t0) * 1e3, 3)


def make(a, rank=0, world=1):
    sim = Simulator(a.n, GM_MODE_PARTIAL, rd_seed=7, view=a.view, view_seed=5, init_mode=1, init_t0=8, init_seed=11,
                    drop_pct=5, drop_from=0, drop_to=1 << 20, drop_seed=42, shard_rank=rank, shard_count=world)
    sim.keep_events(0)
    return sim


def census(sims):
    got = [s.view_census(records=False)[1:] for s in sims]
    return sum(g[0] for g in got), sum(g[1] for g in got)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n", type=int, default=1 << 24)
    p.add_argument("--view", type=int, default=32)
    p.add_argument("--at", type=int, default=13, help="the tick the state is taken before")
    p.add_argument("--shards", type=int, default=8)
    p.add_argument("--follow", type=int, default=3)
    p.add_argument("--slice", type=int, default=1 << 16)
    p.add_argument("--out", default=None, help="directory for cost.json and README.md")
    a = p.parse_args()
    n, v = a.n, a.view
    block = max(1, (256 << 20) // (8 * v))
    crash = crash_set(n, int(round(n * 0.01)), 42)
    src = make(a)
    while src.time < a.at:
        t = src.time
        src.tick()
        if t == 10:
            src.set_failed(crash)
    src.sync()
    views = np.zeros((n, v), dtype=np.uint64)  # touched: no page faults in the timed copies

    def read_all():
        for r0 in range(0, n, block):
            views[r0:r0 + block] = src.read_views(r0, min(block, n - r0))
    _, read_ms = ms(read_all)

    import ctypes
    u64p = ctypes.POINTER(ctypes.c_uint64)

    def read_all_inplace():  # without Simulator.read_views' own array per block
        for r0 in range(0, n, block):
            m = min(block, n - r0)
            src._call("gm_read_views", src.h, r0, m, views[r0:r0 + m].ctypes.data_as(u64p))
    _, read_inplace_ms = ms(read_all_inplace)
    nodes, nodes_ms = ms(lambda: state._nodes(src, view=True))
    snap = dict(nodes, views=views)

    dst = make(a)
    dst.set_timing(1)
    dst.sync()
    _, begin_ms = ms(lambda: dst._call("gm_load_views_begin", dst.h, snap["t"]))
    per_block = []
    for r0 in range(0, n, block):
        m = min(block, n - r0)
        _, b = ms(lambda: dst._call("gm_load_views", dst.h, r0, m, views[r0:r0 + m].ctypes.data_as(u64p)))
        per_block.append(b)
    i32p = ctypes.POINTER(ctypes.c_int32)
    arrs = [np.ascontiguousarray(snap[k], dtype=np.int32) for k in ("heartbeat", "failed", "targets", "counts")]
    st = dst.load_views_stats()
    _, commit_ms = ms(lambda: dst._call("gm_load_views_commit", dst.h, *[x.ctypes.data_as(i32p) for x in arrs]))
    dst.set_timing(0)
    load_ms = round(sum(per_block), 3)
    bytes_views = n * v * 8

    shards = [make(a, g, a.shards) for g in range(a.shards)]

    def load_shards():
        for s in shards:
            state.view_restore(s, state.slice_rows(snap, *s.shard_layout()))
    _, shards_load_ms = ms(load_shards)

    def shard_tick():
        partial_loopback_tick(shards)
        for s in shards:
            s.sync()
    _, first_ms = ms(shard_tick)
    _, second_ms = ms(shard_tick)
    for k in range(a.follow):  # the shards are two ticks ahead: they wait for the others
        src.tick()
        dst.tick()
        if k >= 2:
            shard_tick()
        want = census([src])
        for what, grp in (("restored context", [dst]), ("shards", shards)):
            if what == "shards" and k < 1:
                continue  # the shards are one tick ahead until the others have made their second tick
            got = census(grp)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (what, k)
    m = min(a.slice, n)
    assert np.array_equal(dst.read_views(0, m), src.read_views(0, m)), "views differ after the followed ticks"
    for s in [src, dst] + shards:
        assert s.tick_stats()["err"] == 0
    res = {"n": n, "view": v, "tick": snap["t"], "block_rows": block, "view_bytes": bytes_views,
           "read_views_ms": read_ms, "read_views_inplace_ms": read_inplace_ms, "nodes_ms": nodes_ms,
           "begin_ms": begin_ms, "load_views_ms": load_ms, "load_views_block_ms": per_block,
           "check_ms": round(st["check_ms"], 3), "store_ms": round(st["store_ms"], 3), "staging_bytes": st["staging_bytes"],
           "commit_ms": commit_ms, "load_GBps": round(bytes_views / (load_ms * 1e-3) / 1e9, 1),
           "read_GBps": round(bytes_views / (read_inplace_ms * 1e-3) / 1e9, 1),
           "kernel_share_pct": round(100 * (st["check_ms"] + st["store_ms"]) / load_ms, 2),
           "shards": {"G": a.shards, "load_ms": shards_load_ms, "first_tick_ms": first_ms, "second_tick_ms": second_ms,
                      "replay_ms": round(first_ms - second_ms, 3)}}
    print(json.dumps(res))
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "cost.json"), "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
        sh = res["shards"]
        with open(os.path.join(a.out, "README.md"), "w") as f:
            f.write(f"""# Save and restore of a PARTIAL view state (`scripts/load_views_cost.py`)

Measured on one MI355X: N = {n:,}, V = {v}, the state before tick {snap['t']} (1 % crashed after tick 10,
5 % loss), {bytes_views / 1e9:.2f} GB of views, blocks of {block:,} nodes (the staging buffer, {st['staging_bytes'] / 2**20:.0f} MiB).
Host wall-clock around synced calls, one run each, pageable host arrays; `cost.json` has every figure.

| step | ms | |
|---|---|---|
| `gm_read_views`, all nodes (`Simulator.read_views`, an array per block) | {read_ms} | |
| `gm_read_views`, all nodes, into the caller's array | {read_inplace_ms} | {res['read_GBps']} GB/s |
| `gm_read_nodes` + `gm_read_targets` | {nodes_ms} | |
| `gm_load_views_begin` | {begin_ms} | |
| `gm_load_views`, all nodes | {load_ms} | {res['load_GBps']} GB/s |
| of which `gm_pl_check` (HIP events) | {res['check_ms']} | |
| of which `gm_pl_store` (HIP events) | {res['store_ms']} | |
| `gm_load_views_commit` | {commit_ms} | |

The two kernels take {res['kernel_share_pct']} % of `gm_load_views`; the rest is the host-to-device copy of 8 V bytes
per node and the status read per block.

G = {sh['G']} loopback row shards on the same device: loading all shards {sh['load_ms']} ms; the first tick after
the load, which replays the exchange of the tick before, {sh['first_tick_ms']} ms against {sh['second_tick_ms']} ms for the
next one: the replay costs about {sh['replay_ms']} ms.

Self-check at this size: the restored context and the shards tick beside the source context; the view
census (histogram and sizes) is equal after every tick and the views of the first {m:,} nodes at the end.
""")


if __name__ == "__main__":
    main()
