#!/usr/bin/env python3
"""Cost of loading a SCALED state (gm_load_begin / gm_load_rows / gm_load_commit) at S-A size.

Context A is S-A as bench.py runs it (N = 65,536, warm start at t0 = 8, 655 nodes crashed after
tick 10, RD_SEED 7) ticked to --until (default 14: inside the crash window, so the crashed columns'
entries are in escape lists and the crashed rows are relative to an older tick). Its state goes to a
cold-created context B block by block (512 rows: 256 MiB of hb / ts), each block read with
gm_read_table and given to gm_load_rows at once, so the host never holds more than one block:

  * wall clock around each synced call: gm_read_table per block (every call copies and decodes the
    table's records and escape lists afresh, so this is the price of reading in blocks, not a copy
    rate) and gm_load_rows per block (two host-to-device copies of the staged block, the check
    kernel, the encode kernel);
  * HIP events (gm_set_timing on B): the check kernel and the encode kernel alone, per load
    (gm_load_stats), and the encode kernel's effective bytes/s: 8 B read per staged cell, about 2 B
    written (the stored byte, the payload nibbles of one parity, the record's share);
  * the copy's share: gm_load_rows' wall clock minus both kernels.

Then B is checked against A: a few rows read back equal, and both run --ticks more ticks with equal
event totals, targets and rows. The loader is expected to be bound by the host-to-device copy of
8 B per cell; the JSON shows the kernel time next to it.

  python scripts/load_cost.py [--n 65536] [--out profiles/load_state/sa_load_cost.json]
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
from membership.abi import _ptr  # noqa: E402


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n", type=int, default=65536)
    p.add_argument("--block", type=int, default=512, help="rows per gm_read_table / gm_load_rows call")
    p.add_argument("--until", type=int, default=14, help="A runs until this tick is next")
    p.add_argument("--ticks", type=int, default=4, help="ticks both contexts run after the load")
    p.add_argument("--out", default=None)
    a = p.parse_args()
    n, ncrash = a.n, int(round(a.n * 0.01))
    kw = dict(rd_seed=7, init_t0=8, init_seed=11)
    src = Simulator(n, GM_MODE_SCALED, init_mode=1, **kw)
    src.keep_events(0)
    crash = crash_set(n, ncrash, 42)
    while src.time < a.until:
        t = src.time
        src.tick()
        if t == 10:
            src.set_failed(crash)
    src.sync()
    dst = Simulator(n, GM_MODE_SCALED, init_mode=0, **kw)
    dst.keep_events(0)
    dst.set_timing(1)
    st = src.read_nodes()
    tg, cnt = src.read_targets()
    read_s, load_s = [], []
    t_all = time.perf_counter()
    dst._call("gm_load_begin", dst.h, src.time)
    for r0 in range(0, n, a.block):
        m = min(a.block, n - r0)
        t0 = time.perf_counter()
        hb, ts = src.read_table(r0, m)
        t1 = time.perf_counter()
        dst._call("gm_load_rows", dst.h, r0, m, _ptr(hb), _ptr(ts))  # (with timing on it waits for the encode)
        t2 = time.perf_counter()
        read_s.append(t1 - t0)
        load_s.append(t2 - t1)
        if (r0 // a.block) % 16 == 15:
            print(f"rows {r0 + m}/{n}: read {sum(read_s):.1f} s, load {sum(load_s):.1f} s", file=sys.stderr, flush=True)
    t0 = time.perf_counter()
    dst._call("gm_load_commit", dst.h, _ptr(np.ascontiguousarray(st[:, 3])), _ptr(np.ascontiguousarray(st[:, 2])),
              _ptr(tg), _ptr(cnt))
    commit_s = time.perf_counter() - t0
    total_s = time.perf_counter() - t_all
    ls = dst.load_stats()
    dst.set_timing(0)
    assert ls["rows"] == n and dst.time == src.time
    for r in (0, int(crash[0]), n // 2 + 1, n - 1):
        (ha, ta), (hb2, tb2) = src.read_row(r), dst.read_row(r)
        assert np.array_equal(ha, hb2) and np.array_equal(ta, tb2), f"row {r} differs after the load"
    base = src.event_totals()
    for _ in range(a.ticks):
        src.tick()
        dst.tick()
    assert src.tick_stats()["err"] == 0 and dst.tick_stats()["err"] == 0
    (ta, ca), (tb, cb) = src.read_targets(), dst.read_targets()
    assert np.array_equal(ca, cb) and np.array_equal(ta, tb), "targets differ after the load"
    tot_a, tot_b = src.event_totals(), dst.event_totals()
    assert all(tot_a[k] - base[k] == tot_b[k] for k in tot_a), (base, tot_a, tot_b)
    for r in (1, int(crash[-1]), n - 2):
        (ha, ta), (hb2, tb2) = src.read_row(r), dst.read_row(r)
        assert np.array_equal(ha, hb2) and np.array_equal(ta, tb2), f"row {r} differs {a.ticks} ticks after the load"
    cells = float(n) * n
    load_total, kern = float(np.sum(load_s)), (ls["check_ms"] + ls["encode_ms"]) / 1e3
    res = {"n": n, "block_rows": a.block, "blocks": len(load_s), "state_tick": int(dst.time) - a.ticks,
           "staged_bytes": 8 * cells, "staging_buffer_bytes": ls["staging_bytes"],
           "read_table_s": {"total": round(float(np.sum(read_s)), 3), "per_block_min": round(min(read_s), 4),
                            "per_block_max": round(max(read_s), 4)},
           "load_rows_s": {"total": round(load_total, 3), "per_block_min": round(min(load_s), 4),
                           "per_block_max": round(max(load_s), 4)},
           "load_rows_gbytes_per_s": round(8 * cells / load_total / 1e9, 2),
           "check_kernel_ms": round(ls["check_ms"], 3), "encode_kernel_ms": round(ls["encode_ms"], 3),
           "encode_kernel_gbytes_per_s": round(10 * cells / (ls["encode_ms"] / 1e3) / 1e9, 1),
           "copy_and_host_s": round(load_total - kern, 3), "kernel_share_of_load_rows": round(kern / load_total, 4),
           "commit_s": round(commit_s, 4), "begin_to_commit_s": round(total_s, 3),
           "checked": f"rows equal after the load; {a.ticks} ticks on both: targets, event totals, rows equal"}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
