"""The oracle runs behind tests/golden/digest/traces.json: per-tick state digests (membership.digest, the
NumPy definition) of the project's CPU oracle. Shared by the generator (tests/golden/make_digest_golden.py)
and the tests that replay them; no GPU and nothing of the reference is involved."""
import json
import os

import oracle_py
from membership import digest

TRACES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "digest", "traces.json")
KW = dict(rd_seed=7, init_t0=8, init_seed=11)                 # tests/test_gpu_census.py
PKW = dict(rd_seed=7, view_seed=5, init_t0=8, init_seed=11)   # tests/test_gpu_partial.py
PLOSS = dict(drop_pct=5, drop_from=0, drop_to=1000, drop_seed=42)

# name -> (kind, oracle arguments, first tick, last tick)
CASES = {
    "scaled_n300_crash": ("scaled", dict(n=300, crash_tick=10, crash_count=3, crash_seed=42, init_mode=1, **KW), 9, 45),
    "scaled_n96_cold": ("scaled", dict(n=96, rd_seed=7, init_mode=0), 1, 6),
    "partial_n300_v32": ("partial", dict(n=300, v=32, crash_tick=10, crash_count=3, crash_seed=42, **PKW, **PLOSS), 9, 30),
    "partial_n300_v5": ("partial", dict(n=300, v=5, crash_tick=10, crash_count=3, crash_seed=42, **PKW, **PLOSS), 9, 30),
}


def make_oracle(name):
    kind, kw, _, _ = CASES[name]
    kw = dict(kw)
    n = kw.pop("n")
    return oracle_py.Oracle(n, oracle_py.OC_SCALED, **kw) if kind == "scaled" else oracle_py.PartialOracle(n, **kw)


def oracle_digest(name, ora):
    """the digest of the oracle's state as of its last tick"""
    tg, cnt = ora.targets()
    if CASES[name][0] == "scaled":
        hb, ts = ora.table()
        return digest.reference(hb, ts, ora.nodes(), tg, cnt)
    return digest.reference_views(ora.views(), ora.nodes(), tg, cnt)


def run(name):
    """{tick: {"table": hex, "nodes": hex}} over the case's ticks"""
    _, _, first, last = CASES[name]
    ora = make_oracle(name)
    out = {}
    while ora.time <= last:
        t = ora.time
        ora.tick()
        if t >= first:
            d = oracle_digest(name, ora)
            out[str(t)] = {"table": f"{d['table']:016x}", "nodes": f"{d['nodes']:016x}"}
    ora.close()
    return out


def load():
    with open(TRACES) as f:
        return json.load(f)
