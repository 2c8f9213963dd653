"""What the cluster believes at one tick, from the membership census (Simulator.census(),
gm_census_rec and the (class, lag, age) histogram of include/gm_abi.h): dissemination depth,
suspicion counts, how a crashed node fades from the views, and the headroom of the stored cell
formats. CPU only: plain NumPy over the census arrays, no GPU handle."""
import numpy as np

from .abi import CENSUS_DTYPE, GM_CENSUS_AGES, GM_CENSUS_LAGS

BYTE_LAG_MAX = 14   # the stored byte holds heartbeat lags up to 14 ticks
ERR_LAG_MAX = 125   # a present entry lagging more sets GM_ERR_LAG (gm_scaled.h lag_hmin)


def merge_shards(parts):
    """parts: (c0, rec, hist) of every column shard of one cluster at one tick, in any order.
    Returns (rec, hist) of the cluster: the records by global column, the histograms summed."""
    parts = sorted(parts, key=lambda p: p[0])
    at = 0
    for c0, rec, _ in parts:
        if c0 != at:
            raise ValueError(f"column shards do not tile the columns: a shard starts at {c0}, expected {at}")
        at += len(rec)
    rec = np.concatenate([np.asarray(p[1], dtype=CENSUS_DTYPE) for p in parts])
    hist = np.zeros((2, GM_CENSUS_LAGS, GM_CENSUS_AGES), dtype=np.uint64)
    for _, _, h in parts:
        hist += np.asarray(h, dtype=np.uint64).reshape(hist.shape)
    return rec, hist


def _marginal(h):
    h = np.asarray(h, dtype=np.int64)
    nz = np.flatnonzero(h)
    return h[:int(nz[-1]) + 1].tolist() if len(nz) else []


def summarize_census(rec, hist, failed, t):
    """rec, hist: Simulator.census() over ALL subjects of the cluster (column shards: merge_shards
    first); failed: per node, non-zero = crashed (read_nodes()[:, 2]); t: the tick of the census
    (Simulator.time - 1).

    Returns a dict:
      live_observers  nodes with failed == 0
      coverage        {"min", "mean"} of holders / live observers over the live subjects (None each
                      without live observers or live subjects)
      lag, age        per class ("live" / "crashed" subjects) the marginal counts of the joint
                      histogram, trimmed after the last non-empty bin; the last lag bin
                      (GM_CENSUS_LAGS - 1) also holds every larger lag
      l0              per class {L0: cells} with L0 = lag - age, the lag an entry's heartbeat had
                      when it was last raised (cells of the clipped lag bin are left out and
                      counted in "clipped")
      max_lag         per class the largest heartbeat lag (2t - hb_min) >> 1 over the subjects held
                      by anyone, exact (from the records, not clipped); None without entries
      suspected_by    {"subjects", "min", "mean", "max"}: per crashed subject the live observers
                      whose entry of it is stale (T - ts >= TFAIL), and "faded": crashed subjects
                      nobody holds any more
      headroom        {"byte_lag": BYTE_LAG_MAX - the live subjects' max lag (negative: such cells
                      escape), "err_lag": ERR_LAG_MAX / the largest lag of any subject}
    """
    rec = np.asarray(rec)
    hist = np.asarray(hist, dtype=np.int64).reshape(2, GM_CENSUS_LAGS, GM_CENSUS_AGES)
    crashed = np.asarray(failed) != 0
    if rec.ndim != 1 or rec.shape != crashed.shape:
        raise ValueError(f"records {rec.shape} and failed {crashed.shape} must be 1-D and of one length")
    live_obs = int((~crashed).sum())
    holders = rec["holders"].astype(np.int64)
    if int(holders.sum()) != int(hist.sum()):
        raise ValueError("records and histogram are not of one census: holders and cells differ")
    out = {"t": int(t), "live_observers": live_obs}
    cov = holders[~crashed] / live_obs if live_obs and (~crashed).any() else None
    out["coverage"] = {"min": None if cov is None else float(cov.min()), "mean": None if cov is None else float(cov.mean())}
    names = ("live", "crashed")
    out["lag"] = {nm: _marginal(hist[k].sum(axis=1)) for k, nm in enumerate(names)}
    out["age"] = {nm: _marginal(hist[k].sum(axis=0)) for k, nm in enumerate(names)}
    l0, clipped = {}, {}
    for k, nm in enumerate(names):
        d = {}
        for lag, age in zip(*np.nonzero(hist[k, :GM_CENSUS_LAGS - 1])):
            d[int(lag) - int(age)] = d.get(int(lag) - int(age), 0) + int(hist[k, lag, age])
        l0[nm] = dict(sorted(d.items()))
        clipped[nm] = int(hist[k, GM_CENSUS_LAGS - 1].sum())
    out["l0"], out["clipped"] = l0, clipped
    held = holders > 0
    lag_max = np.where(held, (2 * int(t) - rec["hb_min"].astype(np.int64)) >> 1, -1)
    out["max_lag"] = {nm: (int(lag_max[sel & held].max()) if (sel & held).any() else None)
                      for nm, sel in zip(names, (~crashed, crashed))}
    sus = rec["stale"].astype(np.int64)[crashed]
    out["suspected_by"] = {"subjects": int(crashed.sum()), "faded": int((holders[crashed] == 0).sum()),
                           "min": int(sus.min()) if len(sus) else None,
                           "mean": float(sus.mean()) if len(sus) else None,
                           "max": int(sus.max()) if len(sus) else None}
    ml, ma = out["max_lag"]["live"], max([v for v in out["max_lag"].values() if v is not None], default=None)
    out["headroom"] = {"byte_lag": None if ml is None else BYTE_LAG_MAX - ml,
                       "err_lag": None if not ma else ERR_LAG_MAX / ma}
    return out
