"""What breadth-first walks of the view graph say about the overlay (Simulator.view_reach(),
gm_view_reach of include/gm_abi.h): how many live nodes every source reaches and in how many hops, and
whether the walks prove the overlay strongly connected. CPU only: plain NumPy over the walks' counts,
no GPU handle."""
import numpy as np


def _trim(h):
    nz = np.flatnonzero(h)
    return h[:int(nz[-1]) + 1].tolist() if len(nz) else []


def _per_source(walk):
    counts = np.asarray(walk["counts"], dtype=np.int64)
    if counts.ndim != 2:
        raise ValueError(f"counts of shape {counts.shape}: [hops, sources] expected")
    live = int(walk["live"])
    reached = counts.sum(axis=0)
    if (counts[0] > 1).any() or (reached > live).any() or (reached[counts[0] == 0] != 0).any():
        raise ValueError("counts are not those of a walk: level 0 holds the source alone, a crashed source reaches "
                         "nobody, nobody reaches more than the live nodes")
    if int((counts[0] == 1).sum()) != int(walk["live_sources"]):
        raise ValueError("counts and live_sources are not of one walk")
    return counts, live, reached


def summarize_reach(out, inn=None):
    """out: Simulator.view_reach(sources, "out"); inn: view_reach of the same sources and state with
    "in", or None.

    Returns a dict:
      live, live_sources  as the walk reports them
      stopped             a walk given ended because of max_hops: its figures are lower bounds
      out, in             per direction ("in": None without inn)
                            sources        one dict per source: {"live", "reached", "unreached" (= live
                                           nodes - reached), "eccentricity" (the last non-empty level),
                                           "mean_distance" (over the reached nodes other than the source;
                                           None when there is none)}; a crashed source: live False, 0
                                           reached, the rest None
                            hop_histogram  nodes per level summed over the sources, trimmed
                            hops           the last non-empty level over all sources
      strongly_connected  True iff some live source reaches all live nodes in `out` and is reached by
                          all of them in `inn`: one such node proves the view graph strongly connected.
                          False if a live source fails either. None without inn, when either walk was
                          stopped, and without a live source.
    """
    walks = {"out": out, "in": inn}
    res = {"live": int(out["live"]), "live_sources": int(out["live_sources"]),
           "stopped": bool(out["stopped"]) or (inn is not None and bool(inn["stopped"]))}
    full = {}
    for name, w in walks.items():
        if w is None:
            res[name] = None
            continue
        counts, live, reached = _per_source(w)
        if live != res["live"] or counts.shape[1] != np.asarray(out["counts"]).shape[1]:
            raise ValueError("the two walks are not of one state and one list of sources")
        if not np.array_equal(counts[0], np.asarray(out["counts"], dtype=np.int64)[0]):
            raise ValueError("the two walks are not of one list of sources")
        levels = np.arange(counts.shape[0])
        src = []
        for k in range(counts.shape[1]):
            if not counts[0, k]:
                src.append({"live": False, "reached": 0, "unreached": None, "eccentricity": None, "mean_distance": None})
                continue
            others = int(reached[k]) - 1
            src.append({"live": True, "reached": int(reached[k]), "unreached": live - int(reached[k]),
                        "eccentricity": int(np.flatnonzero(counts[:, k])[-1]),
                        "mean_distance": float((levels * counts[:, k]).sum()) / others if others else None})
        hist = _trim(counts.sum(axis=1))
        res[name] = {"sources": src, "hop_histogram": hist, "hops": max(len(hist) - 1, 0)}
        full[name] = (counts[0] == 1) & (reached == live)
    if inn is None or res["stopped"] or not res["live_sources"]:
        res["strongly_connected"] = None
    else:
        res["strongly_connected"] = bool((full["out"] & full["in"]).any())
    return res
