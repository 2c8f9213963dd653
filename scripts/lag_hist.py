#!/usr/bin/env python3
"""Diagnostics: distribution of a present cell's heartbeat lag split as lag = L0 + age (L0 = the
lag its heartbeat had when it was last raised, constant while the entry ages) through the S-A
schedule -- which byte code ranges the stored cells need. Over ALL rows: the membership census
(gm_census) reduces the table on the device. usage: lag_hist.py [n]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "distributed-membership_amd"))
from membership import GM_MODE_SCALED, Simulator, crash_set, summarize_census  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
sim = Simulator(n, GM_MODE_SCALED, rd_seed=7, init_mode=1, init_t0=8, init_seed=11)
sim.keep_events(0)
crash = crash_set(n, int(round(n * 0.01)), 42)
crashed = np.zeros(n, bool)
while sim.time <= 48:
    t = sim.time
    sim.tick()
    if t == 10:
        sim.set_failed(crash)
        crashed[crash] = True
    if t in (9, 12, 16, 20, 24, 28, 32, 36, 40, 44, 48):
        rec, hist = sim.census()
        s = summarize_census(rec, hist, crashed, t)
        for k, name in enumerate(("live", "crashed")):
            cells = int(hist[k].sum())
            if not cells:
                print(f"t={t} {name}: none", flush=True)
                continue
            l0 = s["l0"][name]
            lh = [l0.get(v, 0) for v in range(-1, max(l0) + 1)]
            print(f"t={t} {name}: cells {cells} L0 min {min(l0)} max {max(l0)} hist(L0=-1..) {lh} "
                  f"age max {len(s['age'][name]) - 1} hist {s['age'][name]} lag max {s['max_lag'][name]} "
                  f"clipped {s['clipped'][name]}", flush=True)
        print(f"t={t} coverage {s['coverage']} suspected_by {s['suspected_by']} headroom {s['headroom']}", flush=True)
