"""What the partial views hold at one tick, from the view census (Simulator.view_census(),
gm_view_rec and the histograms of include/gm_abi.h): in-degree, orphans, view fill, entry ages and
how a crashed node fades from the views. CPU only: plain NumPy over the census arrays, no GPU
handle."""
import numpy as np

from .abi import GM_VIEW_AGES, GM_VIEW_SIZES, VIEW_DTYPE


def merge_view_shards(parts):
    """parts: (rec, hist, sizes) of every row shard of one cluster at one tick, in any order; each
    shard reduced its own nodes' views over all subjects. Returns (rec, hist, sizes) of the cluster:
    holders / stale / hb_sum and the histograms add, hb_min / hb_max are the min / max over the
    shards that hold the subject (-1 = none)."""
    parts = list(parts)
    if not parts:
        raise ValueError("no shard census to merge")
    n = len(parts[0][0])
    rec = np.zeros(n, dtype=VIEW_DTYPE)
    rec["hb_min"] = rec["hb_max"] = -1
    hist = np.zeros((2, GM_VIEW_AGES), dtype=np.uint64)
    sizes = np.zeros(GM_VIEW_SIZES, dtype=np.uint64)
    for r, h, s in parts:
        r = np.asarray(r, dtype=VIEW_DTYPE)
        if r.shape != (n,):
            raise ValueError(f"shard records of different lengths: {r.shape} and {(n,)}")
        for f in ("holders", "stale", "hb_sum"):
            rec[f] += r[f]
        has, had = r["hb_min"] >= 0, rec["hb_min"] >= 0
        rec["hb_min"] = np.where(has & had, np.minimum(rec["hb_min"], r["hb_min"]), np.where(has, r["hb_min"], rec["hb_min"]))
        rec["hb_max"] = np.maximum(rec["hb_max"], r["hb_max"])
        hist += np.asarray(h, dtype=np.uint64).reshape(hist.shape)
        sizes += np.asarray(s, dtype=np.uint64).reshape(sizes.shape)
    return rec, hist, sizes


def _trim(h):
    h = np.asarray(h, dtype=np.int64)
    nz = np.flatnonzero(h)
    return h[:int(nz[-1]) + 1].tolist() if len(nz) else []


def summarize_views(rec, hist, sizes, failed, t, v):
    """rec, hist, sizes: Simulator.view_census() of the whole cluster (row shards: merge_view_shards
    first); failed: per node, non-zero = crashed; t: the tick of the census (Simulator.time - 1);
    v: the view capacity.

    Returns a dict:
      live_observers  sizes.sum()
      view_size       {"min", "mean", "full"}: over the live views; full = the share holding v entries
                      (None each without live observers)
      in_degree       over the live subjects, the holders other than the subject itself
                      (holders - 1): {"min", "mean", "max", "hist"}, hist the trimmed bincount
      orphans         live subjects nobody else holds
      age             per class ("live" / "crashed" subjects) the trimmed marginal of hist
      stale           per class the sum of rec["stale"]
      max_lag         per class the largest heartbeat lag (2t - 1 - hb_min) / 2, exact; None without
                      entries
      crashed         {"subjects", "held", "entries"}: crashed subjects, those some live view still
                      holds, and the entries of them
    """
    rec = np.asarray(rec)
    hist = np.asarray(hist, dtype=np.int64).reshape(2, GM_VIEW_AGES)
    sizes = np.asarray(sizes, dtype=np.int64).reshape(GM_VIEW_SIZES)
    crashed = np.asarray(failed) != 0
    if rec.ndim != 1 or rec.shape != crashed.shape:
        raise ValueError(f"records {rec.shape} and failed {crashed.shape} must be 1-D and of one length")
    holders = rec["holders"].astype(np.int64)
    entries = int((np.arange(GM_VIEW_SIZES) * sizes).sum())
    if int(holders.sum()) != int(hist.sum()):
        raise ValueError("records and histogram are not of one census: holders and entries differ")
    if int(hist.sum()) != entries:
        raise ValueError("histogram and view sizes are not of one census: entries differ")
    live_obs = int(sizes.sum())
    out = {"t": int(t), "live_observers": live_obs}
    held_sizes = np.flatnonzero(sizes)
    out["view_size"] = {"min": int(held_sizes[0]) if live_obs else None,
                        "mean": entries / live_obs if live_obs else None,
                        "full": float(sizes[v]) / live_obs if live_obs else None}
    deg = holders[~crashed] - 1  # a live subject's own entry is one of its holders
    if len(deg) and deg.min() < 0:
        raise ValueError("a live subject without its own entry: failed is not this census's crash set")
    out["in_degree"] = {"min": int(deg.min()) if len(deg) else None, "mean": float(deg.mean()) if len(deg) else None,
                        "max": int(deg.max()) if len(deg) else None, "hist": _trim(np.bincount(deg)) if len(deg) else []}
    out["orphans"] = int((deg == 0).sum())
    names = ("live", "crashed")
    out["age"] = {nm: _trim(hist[k]) for k, nm in enumerate(names)}
    stale = rec["stale"].astype(np.int64)
    out["stale"] = {nm: int(stale[sel].sum()) for nm, sel in zip(names, (~crashed, crashed))}
    held = holders > 0
    lag = np.where(held, (2 * int(t) - 1 - rec["hb_min"].astype(np.int64)) // 2, -1)
    out["max_lag"] = {nm: (int(lag[sel & held].max()) if (sel & held).any() else None)
                      for nm, sel in zip(names, (~crashed, crashed))}
    out["crashed"] = {"subjects": int(crashed.sum()), "held": int((held & crashed).sum()),
                      "entries": int(holders[crashed].sum())}
    return out
