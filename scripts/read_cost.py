#!/usr/bin/env python3
"""Cost of reading a SCALED state decoded on the device (gm_read_rows) at S-A size, beside the host
route it complements (gm_read_table).

S-A as bench.py runs it: N = 65,536, warm start at t0 = 8, 655 nodes (crash_set(N, 655, 42)) crashed
after tick 10, RD_SEED 7, event keeping off, ticked to --until (default 14: inside the crash window,
the crashed columns' entries in escape lists). In one context and one session:

  * gm_read_table of 256 rows, host wall clock (it copies and decodes the whole stored state whatever
    the row count is; the route is unchanged, so it is the baseline), and the same 256 rows through
    gm_read_rows, compared cell for cell;
  * gm_read_rows of 256 / 512 / 2048 / 8192 rows: the cost follows count, not n;
  * all N rows in --block-row calls (512: one 256 MiB staging block each) into ONE reused pair of host
    arrays (pageable numpy memory), gm_set_timing on: wall clock, the decode kernel's and the
    device-to-host copies' share (gm_read_rows_stats), GB/s of staged bytes (8 B per cell) over the
    wall clock and over the kernel time alone (the kernel reads 1 B and writes 8 B per cell);
  * the tick after a full read against ticks without one: windows of --steady ticks, each followed
    by gm_sync and timed on its own, alternately after nothing and after an (untimed) full read.

--sb: instead, one 128-row block (256 MiB) of a single S-B context (N = 262,144), where the host
route cannot run; the rows are checked against gm_read_row.

  python scripts/read_cost.py [--out profiles/read_rows/sa_read_cost.json]
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "distributed-membership_amd"))

import numpy as np  # noqa: E402

from membership import GM_MODE_SCALED, Simulator, crash_set  # noqa: E402


def wall(fn):
    t0 = time.perf_counter()
    r = fn()
    return r, (time.perf_counter() - t0) * 1e3


def run_to(sim, until, crash):
    while sim.time < until:
        t = sim.time
        sim.tick()
        if t == 10:
            sim.set_failed(crash)
    sim.sync()


def full_read(sim, buf, block):
    """all rows through one reused pair of host arrays; returns the wall clock in ms"""
    t0 = time.perf_counter()
    for r0 in range(0, sim.n, block):
        sim.read_rows(r0, min(block, sim.n - r0), out=buf)
    return (time.perf_counter() - t0) * 1e3


def timed_ticks(sim, k):
    out = []
    for _ in range(k):
        sim.sync()
        _, ms = wall(lambda: (sim.tick(), sim.sync()))
        out.append(round(ms, 3))
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n", type=int, default=65536)
    p.add_argument("--block", type=int, default=512, help="rows per gm_read_rows call of the full read")
    p.add_argument("--until", type=int, default=14)
    p.add_argument("--reps", type=int, default=3, help="full reads timed")
    p.add_argument("--steady", type=int, default=2, help="ticks per window of the next-tick comparison")
    p.add_argument("--windows", type=int, default=3)
    p.add_argument("--sb", action="store_true", help="one 128-row block at N = 262,144 instead")
    p.add_argument("--out", default=None)
    a = p.parse_args()
    kw = dict(rd_seed=7, init_t0=8, init_seed=11, init_mode=1)
    if a.sb:
        n = 262144
        sim, create_ms = wall(lambda: Simulator(n, GM_MODE_SCALED, **kw))
        sim.keep_events(0)
        run_to(sim, 12, crash_set(n, int(round(n * 0.01)), 42))
        sim.set_timing(1)
        rows = max(1, (256 << 20) // (8 * n))
        r0 = n // 3
        (hb, ts), first_ms = wall(lambda: sim.read_rows(r0, rows))  # allocates the staging buffer
        _, ms = wall(lambda: sim.read_rows(r0, rows, out=(hb, ts)))
        for r in (r0, r0 + rows - 1):
            h1, t1 = sim.read_row(r)
            assert np.array_equal(h1, hb[r - r0]) and np.array_equal(t1, ts[r - r0]), f"row {r} differs from gm_read_row"
        st = sim.read_rows_stats()
        res = {"n": n, "rows": rows, "state_tick": sim.time - 1, "create_ms": round(create_ms, 1),
               "first_call_ms": round(first_ms, 2), "read_rows_ms": round(ms, 2), "ms_per_row": round(ms / rows, 4),
               "stage_rows": st["stage_rows"], "staging_bytes": st["staging_bytes"],
               "decode_ms_two_calls": round(st["decode_ms"], 3), "copy_ms_two_calls": round(st["copy_ms"], 3),
               "checked": "first and last row of the block equal gm_read_row"}
    else:
        n = a.n
        sim = Simulator(n, GM_MODE_SCALED, **kw)
        sim.keep_events(0)
        crash = crash_set(n, int(round(n * 0.01)), 42)
        run_to(sim, a.until, crash)
        r0 = n // 3
        host_ms = []
        for _ in range(2):
            (hb_t, ts_t), ms = wall(lambda: sim.read_table(r0, 256))
            host_ms.append(round(ms, 1))
        (hb_r, ts_r), first_ms = wall(lambda: sim.read_rows(r0, 256))  # allocates the staging buffer
        assert np.array_equal(hb_r, hb_t) and np.array_equal(ts_r, ts_t), "read_rows differs from read_table"
        for r in (int(crash[0]), 0, n - 1):  # a crashed row decodes relative to its own tick
            (h1, t1), (h2, t2) = sim.read_row(r), sim.read_rows(r, 1)
            assert np.array_equal(h1, h2[0]) and np.array_equal(t1, t2[0]), f"row {r} differs from gm_read_row"
        by_count = {}
        for cnt in (c for c in (256, 512, 2048, 8192) if r0 + c <= n):
            buf = (np.empty((cnt, n), dtype=np.int32), np.empty((cnt, n), dtype=np.int32))
            sim.read_rows(r0, cnt, out=buf)  # touches the host pages
            by_count[cnt] = [round(wall(lambda: sim.read_rows(r0, cnt, out=buf))[1], 2) for _ in range(3)]
            del buf
        buf = (np.empty((a.block, n), dtype=np.int32), np.empty((a.block, n), dtype=np.int32))
        full_read(sim, buf, a.block)  # warm: host pages, code object
        sim.set_timing(1)
        full = []
        for _ in range(a.reps):
            s0 = sim.read_rows_stats()
            ms = full_read(sim, buf, a.block)
            s1 = sim.read_rows_stats()
            assert s1["rows"] - s0["rows"] == n
            full.append({"wall_ms": round(ms, 1), "decode_ms": round(s1["decode_ms"] - s0["decode_ms"], 2),
                         "copy_ms": round(s1["copy_ms"] - s0["copy_ms"], 1)})
        sim.set_timing(0)
        ticks = {"plain": [], "after_full_read": []}
        for _ in range(a.windows):  # alternating windows in one context
            ticks["plain"].append(timed_ticks(sim, a.steady))
            w = []
            for _ in range(a.steady):
                full_read(sim, buf, a.block)
                w += timed_ticks(sim, 1)
            ticks["after_full_read"].append(w)
        assert sim.tick_stats()["err"] == 0
        st = sim.read_rows_stats()
        best = min(full, key=lambda f: f["wall_ms"])
        staged = 8.0 * n * n
        res = {"n": n, "state_tick": a.until - 1, "block_rows": a.block, "stage_rows": st["stage_rows"],
               "staging_bytes": st["staging_bytes"], "staged_bytes_full_read": staged,
               "read_table_256_rows_ms": host_ms, "read_table_ms_per_row": round(min(host_ms) / 256, 3),
               "read_rows_first_call_256_rows_ms": round(first_ms, 2), "read_rows_ms_by_count": by_count,
               "read_rows_ms_per_row_at_256": round(min(by_count[256]) / 256, 4),
               "full_read": full, "full_read_ms_per_row": round(best["wall_ms"] / n, 4),
               "full_read_GBps_wall": round(staged / (best["wall_ms"] * 1e-3) / 1e9, 2),
               "decode_kernel_GBps_staged": round(staged / (best["decode_ms"] * 1e-3) / 1e9, 1),
               "decode_kernel_share_of_wall": round(best["decode_ms"] / best["wall_ms"], 4),
               "copy_share_of_wall": round(best["copy_ms"] / best["wall_ms"], 4),
               "factor_over_read_table_per_row": round((min(host_ms) / 256) / (best["wall_ms"] / n), 1),
               "tick_ms": ticks, "host_memory": "pageable (numpy)",
               "checked": "256 rows equal gm_read_table; a crashed, the first and the last row equal gm_read_row"}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
