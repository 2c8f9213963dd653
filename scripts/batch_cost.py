#!/usr/bin/env python3
"""Cost of a FAITHFUL ensemble: R independent clusters through gm_batch_tick against the same R
contexts ticked round-robin with gm_tick, and one context through gm_tick against another build.

Every run is the reference's schedule on every member: the `singlefailure` conf at N nodes
(SINGLE_FAILURE 1, no drops), seeds time_seed = rd_seed = 1..R, 700 ticks, Application::fail at
t = 100 (gm_rand + gm_set_failed per member), nothing drained in between. Wall clock from the first
tick to the end of a gm_sync of every member, so the work is done when the clock stops.

  (a) batch        membership.Batch: one gm_batch_tick per tick
  (b) round-robin  one gm_tick per member and tick, each context on its own stream

For every (N, R) the two paths alternate --reps times in one process, on fresh contexts each time.
Also recorded: context creation time and device bytes per member (hipMemGetInfo around the creation),
and the host time of a batch tick (50 ticks enqueued after a sync, the clock stopped before the next
sync). --solo times one context through gm_tick at every N, --reps times; with --other-lib PATH that
is run in child processes, --reps of them on that libgm.so (an earlier build) alternating with --reps
on this one, so both builds are timed under the same conditions. --only solo / ensembles runs one half.

  python scripts/batch_cost.py [--out profiles/batch/batch_cost.json] [--other-lib PATH]
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "distributed-membership_amd"))

from membership import GM_MODE_FAITHFUL, Params, Simulator  # noqa: E402
from membership.app import Log, fail_step  # noqa: E402

TICKS = 700
PLAN = {10: (1, 8, 64, 256), 70: (1, 8, 64)}


def free_bytes():
    hip = ctypes.CDLL("libamdhip64.so")
    free, total = ctypes.c_size_t(), ctypes.c_size_t()
    if hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) != 0:
        raise RuntimeError("hipMemGetInfo failed")
    return free.value


def make(n, r):
    """R contexts, seeds 1..R: (sims, creation ms per member, device bytes per member)"""
    f0 = free_bytes()
    t0 = time.perf_counter()
    sims = [Simulator(n, GM_MODE_FAITHFUL, 1, 0, 0.1, s, s) for s in range(1, r + 1)]
    ms = (time.perf_counter() - t0) * 1e3 / r
    return sims, ms, (f0 - free_bytes()) / r


def run(n, sims, batch):
    """700 ticks of every member with fail() at t = 100; wall ms, synced"""
    par = Params(n, 1, 0, 0.1)
    log = Log()
    for s in sims:
        s.sync()
    t0 = time.perf_counter()
    for t in range(TICKS):
        if batch is not None:
            batch.tick()
        else:
            for s in sims:
                s.tick()
        if t == 100:
            for s in sims:
                fail_step(par, s, log, t)
    for s in sims:
        s.sync()
    return (time.perf_counter() - t0) * 1e3


def host_tick_us(sims, batch):
    """host time of gm_batch_tick in the steady state: 50 ticks enqueued after a sync"""
    for s in sims:
        s.sync()
    t0 = time.perf_counter()
    for _ in range(50):
        batch.tick()
    us = (time.perf_counter() - t0) * 1e6 / 50
    for s in sims:
        s.sync()
    return us


def ensemble(n, r, reps):
    from membership import Batch
    out = {"n": n, "R": r, "batch_ms": [], "round_robin_ms": [], "create_ms_per_member": [],
           "device_bytes_per_member": [], "batch_host_us_per_tick": []}
    for _ in range(reps):
        for path in ("batch", "round_robin"):
            sims, cms, dbytes = make(n, r)
            out["create_ms_per_member"].append(round(cms, 3))
            out["device_bytes_per_member"].append(int(dbytes))
            batch = Batch(sims) if path == "batch" else None
            out[path + "_ms"].append(round(run(n, sims, batch), 3))
            if batch is not None:
                out["batch_host_us_per_tick"].append(round(host_tick_us(sims, batch), 2))
                batch.close()
            for s in sims:
                s.close()
    a, b = out["batch_ms"], out["round_robin_ms"]
    out["batch_spread_ms"] = round(max(a) - min(a), 3)
    out["round_robin_spread_ms"] = round(max(b) - min(b), 3)
    out["round_robin_over_batch"] = round((sum(b) / len(b)) / (sum(a) / len(a)), 3)
    out["batch_wins_beyond_spread"] = min(b) - max(a) > max(out["batch_spread_ms"], out["round_robin_spread_ms"])
    return out


def solo(reps):
    """one context through gm_tick: {N: [wall ms of 700 ticks] * reps}"""
    res = {}
    for n in PLAN:
        res[n] = []
        for _ in range(reps):
            sims, _, _ = make(n, 1)
            res[n].append(round(run(n, sims, None), 3))
            sims[0].close()
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--solo", action="store_true", help="only the single-context runs; prints their JSON")
    p.add_argument("--other-lib", default=None, help="another build's libgm.so for the single-context comparison")
    p.add_argument("--only", choices=("solo", "ensembles"), default=None, help="run one half of the measurement")
    p.add_argument("--out", default=None)
    a = p.parse_args()
    if a.solo:
        print(json.dumps(solo(a.reps)))
        return
    res = {"ticks": TICKS, "reps": a.reps, "ensembles": [], "solo_this_build": [], "solo_other_build": []}

    def child(lib):  # one context through gm_tick in a process of its own, on this build's library or another
        env = dict(os.environ, GM_AB_BUILD="1")
        if lib:
            env["GM_LIBRARY"] = os.path.abspath(lib)
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--solo", "--reps", str(a.reps)], env=env,
                             check=True, capture_output=True, text=True, timeout=300).stdout
        return json.loads(out.strip().splitlines()[-1])

    if a.only != "ensembles":
        for _ in range(a.reps if a.other_lib else 1):
            if a.other_lib:
                res["solo_other_build"].append(child(a.other_lib))
            res["solo_this_build"].append(child(None))
        print(json.dumps({k: res[k] for k in ("solo_other_build", "solo_this_build")}), flush=True)
    for n, rs in PLAN.items() if a.only != "solo" else ():
        for r in rs:
            e = ensemble(n, r, a.reps)
            res["ensembles"].append(e)
            print(json.dumps(e), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
