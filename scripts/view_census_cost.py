#!/usr/bin/env python3
"""Cost of the view census (gm_view_census) at S-C size, and its full-size self-check.

S-C as bench.py runs it: N = 16,777,216, V = 32, warm start at t0 = 8, 5 % per-entry loss on every
tick, 1 % of the nodes (crash_set(N, N / 100, 42)) crashed after tick 10, RD_SEED 7, event keeping
off. Host wall-clock around synced calls (gm_sync, then the call; every call measured returns after
its own copies), --reps calls each with every run listed, at
  * a steady tick (9, before the crash),
  * the tick after the crash (11),
  * 4 ticks later (15).
Per tick:
  census_all_ms       gm_view_census with all three outputs (24 N bytes of records come back)
  census_norec_ms     gm_view_census with out = NULL (no flush kernel, 776 bytes come back)
  read_views_copy_ms  the route it replaces, the copy alone: gm_read_views of all N nodes into one
                      host buffer (allocated once; the first run also pays its page faults)
  slice_route_ms      the same route on a slice of --slice nodes with its reduction: gm_read_views of
                      the slice plus the census of the slice in vectorised NumPy (bincount /
                      minimum.at) on one thread
Beside each census time: the bytes of the live views (live nodes x V x 8) divided by it.

Unperturbed run: in one context, windows of --steady ticks, each tick followed by gm_sync and timed on
its own, in turn with nothing, with an (untimed) census with all outputs, with an (untimed) census
with out = NULL and with an (untimed) gm_read_views of all nodes between the ticks.

Self-check at full size at every measured tick: holders.sum() == hist.sum() == sum of s x sizes[s];
sizes.sum() == the live nodes; every live subject has a holder; nothing is in the crashed class
before the crash.

  python scripts/view_census_cost.py [--out profiles/view_census/sc_cost.json]
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

from membership import GM_MODE_PARTIAL, Simulator, crash_set, summarize_views  # noqa: E402
from membership.abi import GM_VIEW_SIZES  # noqa: E402

TFAIL = 5


def timed(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return r, [round(x, 3) for x in out]


def numpy_census(views, failed_obs, crashed, t, n):
    """the census of a slice of views on the host (what tests/view_census_ref.py specifies)"""
    e = views[failed_obs == 0]
    sizes = np.bincount((e != 0).sum(axis=1), minlength=GM_VIEW_SIZES)
    e = e[e != 0]
    j = (e >> np.uint64(32)).astype(np.int64) - 1
    hb = (e & np.uint64(0xFFFFFFFF)).astype(np.int64)
    age = t - (hb + 1) // 2
    holders = np.bincount(j, minlength=n)
    stale = np.bincount(j[age >= TFAIL], minlength=n)
    hb_sum = np.bincount(j, weights=hb.astype(np.float64), minlength=n)
    lo = np.full(n, np.iinfo(np.int64).max)
    hi = np.full(n, -1, dtype=np.int64)
    np.minimum.at(lo, j, hb)
    np.maximum.at(hi, j, hb)
    hist = np.bincount(crashed[j].astype(np.int64) * 32 + age, minlength=64)
    return holders, stale, hb_sum, lo, hi, hist, sizes


def measure(sim, a, what, crashed, buf):
    n, v, t = sim.n, a.view, sim.time - 1
    sim.sync()
    (rec, hist, sizes), all_ms = timed(sim.view_census, a.reps)
    (_, hist2, sizes2), norec_ms = timed(lambda: sim.view_census(records=False), a.reps)
    assert np.array_equal(hist, hist2) and np.array_equal(sizes, sizes2)
    live = n - int(crashed.sum())
    entries = int(rec["holders"].sum())
    assert entries == int(hist.sum()) == int((np.arange(GM_VIEW_SIZES) * sizes.astype(np.int64)).sum()), "sums"
    assert int(sizes.sum()) == live, "sizes.sum() is not the number of live nodes"
    assert (rec["holders"][~crashed] >= 1).all(), "a live subject without a holder"
    if not crashed.any():
        assert not hist[1].any(), "entries in the crashed class before the crash"
    view_bytes = live * v * 8
    row = {"what": what, "tick": t, "live": live, "entries": entries, "live_view_bytes": view_bytes,
           "census_all_ms": all_ms, "census_norec_ms": norec_ms,
           "views_GBps_all": round(view_bytes / (min(all_ms) * 1e-3) / 1e9, 1),
           "views_GBps_norec": round(view_bytes / (min(norec_ms) * 1e-3) / 1e9, 1)}
    u64p = ctypes.POINTER(ctypes.c_uint64)
    if not a.no_route:
        def copy_all():
            assert sim.lib.gm_read_views(sim.h, 0, n, buf.ctypes.data_as(u64p)) == 0
        _, row["read_views_copy_ms"] = timed(copy_all, a.reps)
        m = min(a.slice, n)
        failed_obs = crashed[:m].astype(np.int32)

        def slice_route():
            return numpy_census(sim.read_views(0, m), failed_obs, crashed, t, n)
        got, row["slice_route_ms"] = timed(slice_route, a.reps)
        row["slice_nodes"] = m
        if m == n:  # the whole cluster fits the slice: the host reduction must equal the device's
            assert np.array_equal(got[0], rec["holders"]) and np.array_equal(got[5].reshape(2, 32), hist)
    return rec, hist, sizes, row


def window(sim, ticks, between, buf=None):
    tot = 0.0
    for _ in range(ticks):
        t0 = time.perf_counter()
        sim.tick()
        sim.sync()
        tot += time.perf_counter() - t0
        if between == "read_views":
            assert sim.lib.gm_read_views(sim.h, 0, sim.n, buf.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))) == 0
        elif between:
            sim.view_census(records=between == "all")
    return tot * 1e3 / ticks


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n", type=int, default=1 << 24)
    p.add_argument("--view", type=int, default=32)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--slice", type=int, default=1 << 20, help="nodes of the host-reduction slice")
    p.add_argument("--steady", type=int, default=20, help="ticks per window of the unperturbed-run pairs")
    p.add_argument("--pairs", type=int, default=3)
    p.add_argument("--no-route", action="store_true", help="skip the read_views route")
    p.add_argument("--kernels-only", action="store_true",
                   help="for a kernel trace: run to tick 11, --reps censuses with all outputs, nothing else")
    p.add_argument("--out", default=None)
    a = p.parse_args()
    n, v, ncrash = a.n, a.view, int(round(a.n * 0.01))
    sim = Simulator(n, GM_MODE_PARTIAL, rd_seed=7, view=v, view_seed=5, init_mode=1, init_t0=8, init_seed=11,
                    drop_pct=5, drop_from=0, drop_to=1 << 20, drop_seed=42)
    sim.keep_events(0)
    crash = crash_set(n, ncrash, 42)
    crashed = np.zeros(n, dtype=bool)
    if a.kernels_only:
        while sim.time <= 11:
            t = sim.time
            sim.tick()
            if t == 10:
                sim.set_failed(crash)
        for _ in range(a.reps):
            sim.view_census()
        sim.close()
        return
    buf = None if a.no_route else np.zeros((n, v), dtype=np.uint64)
    rows, summaries = [], {}
    names = {9: "steady", 11: "the tick after the crash", 15: "4 ticks later"}
    while sim.time <= 15:
        t = sim.time
        sim.tick()
        if t == 10:
            sim.set_failed(crash)
            crashed[crash] = True
        if t in names:
            rec, hist, sizes, row = measure(sim, a, names[t], crashed, buf)
            rows.append(row)
            summaries[names[t]] = summarize_views(rec, hist, sizes, crashed, t, v)
            print(json.dumps(row), flush=True)
    pairs = []
    for _ in range(a.pairs):
        off = window(sim, a.steady, None)
        on = window(sim, a.steady, "all")
        norec = window(sim, a.steady, "norec")
        pairs.append({"plain_ms": round(off, 4), "with_census_ms": round(on, 4), "diff_ms": round(on - off, 4),
                      "with_census_norec_ms": round(norec, 4), "diff_norec_ms": round(norec - off, 4)})
        if buf is not None:  # the route the census replaces, between the ticks: its copy alone
            rv = window(sim, a.steady, "read_views", buf)
            pairs[-1].update({"with_read_views_ms": round(rv, 4), "diff_read_views_ms": round(rv - off, 4)})
    del buf
    assert sim.tick_stats()["err"] == 0
    sim.close()
    res = {"n": n, "view": v, "crashed": ncrash, "reps": a.reps, "stored_view_bytes": n * v * 8, "measured": rows,
           "unperturbed_pairs": pairs, "summaries": summaries}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps({k: val for k, val in res.items() if k not in ("summaries", "measured")}))


if __name__ == "__main__":
    main()
