"""What the reference's grader asks of a run -- completeness, accuracy, detection latency -- from
the detection records (Simulator.detect(), gm_detect_rec of include/gm_abi.h), and what a
partial-view run is asked instead -- how its crashed nodes fade from the views -- from the PARTIAL
records (Simulator.view_detect(), gm_view_detect_rec). CPU only: plain NumPy over the records, no
GPU handle."""
import numpy as np


def summarize(records, failed_mask):
    """records: the structured array of Simulator.detect() over ALL subjects of the cluster (column
    shards: their arrays concatenated by rank); failed_mask: bool per subject, the crashed nodes.

    Returns {"completeness", "false_removals", "latency"}:
      completeness    share of crashed subjects that every non-crashed node removed, i.e. whose
                      removals - false_removals equals the number of non-crashed nodes (1.0 when
                      nothing crashed)
      false_removals  removals logged while the subject was alive, over all subjects
      latency         {"min", "mean", "max"} in ticks after the crash, over the crashed subjects
                      that were removed at all: the smallest first_removed - fail_tick, the mean of
                      removed_tick_sum / removals - fail_tick, the largest last_removed - fail_tick
                      (None each when no crashed subject was removed)
    """
    rec = np.asarray(records)
    crashed = np.asarray(failed_mask, dtype=bool)
    if rec.shape != crashed.shape or rec.ndim != 1:
        raise ValueError(f"records {rec.shape} and failed_mask {crashed.shape} must be 1-D and of one length")
    live = int((~crashed).sum())
    true_rem = rec["removals"].astype(np.int64) - rec["false_removals"].astype(np.int64)
    ncrashed = int(crashed.sum())
    complete = int((true_rem[crashed] == live).sum())
    seen = crashed & (rec["removals"] > 0)
    lat = {"min": None, "mean": None, "max": None}
    if seen.any():
        r = rec[seen]
        ft = r["fail_tick"].astype(np.int64)
        lat["min"] = int((r["first_removed"].astype(np.int64) - ft).min())
        lat["mean"] = float((r["removed_tick_sum"].astype(np.float64) / r["removals"] - ft).mean())
        lat["max"] = int((r["last_removed"].astype(np.int64) - ft).max())
    return {"completeness": complete / ncrashed if ncrashed else 1.0,
            "false_removals": int(rec["false_removals"].astype(np.int64).sum()),
            "latency": lat}


def merge_view_detect_shards(parts):
    """The cluster's PARTIAL detection records from the row shards' parts (Simulator.view_detect() of
    every shard, each over all n subjects): removals, false_removals, late_joins, removed_tick_sum and
    held_sum add; first_removed is the minimum over the parts that have one (-1 = none);
    last_removed and last_held are the maximum; fail_tick must be the same in every part (every
    shard is given the whole crash set), else ValueError. The shards' timelines simply add."""
    parts = [np.asarray(p) for p in parts]
    if not parts or any(p.shape != parts[0].shape or p.dtype != parts[0].dtype or p.ndim != 1 for p in parts):
        raise ValueError("merge_view_detect_shards: the parts must be 1-D record arrays of one length")
    out = parts[0].copy()
    for p in parts[1:]:
        if not np.array_equal(p["fail_tick"], out["fail_tick"]):
            raise ValueError("merge_view_detect_shards: the parts disagree on fail_tick (not one crash set)")
        for f in ("removals", "false_removals", "late_joins", "removed_tick_sum", "held_sum"):
            out[f] += p[f]
        a, b = out["first_removed"], p["first_removed"]
        out["first_removed"] = np.where(a < 0, b, np.where(b < 0, a, np.minimum(a, b)))
        for f in ("last_removed", "last_held"):
            out[f] = np.maximum(out[f], p[f])
    return out


def summarize_view_detect(records, failed_mask, timeline=None):
    """What a partial-view run is asked about its crashed nodes, from the PARTIAL detection records
    (Simulator.view_detect(), gm_view_detect_rec of include/gm_abi.h; row shards: merged).
    records: one per subject of the cluster; failed_mask: bool per subject, the crashed nodes;
    timeline: Simulator.view_detect_timeline(t) up to the last tick run, uint64 [t, 5], or None.

    Returns
      extinct               share of crashed subjects no live observer holds any more: last_held below
                            the last tick (1.0 when nothing crashed). The last tick is the timeline's
                            last row; without a timeline it is the latest tick any record names, so a
                            subject held then counts as still held
      forget_latency        {"min", "mean", "max"} of last_held + 1 - fail_tick, the ticks from the
                            crash to the extinction of the last entry, over the crashed subjects that
                            were ever held while crashed (None each when there is none)
      stale_observer_ticks  the sum of held_sum: observer-ticks of belief in a crashed node
      late_joins            JOINED records naming a subject that was crashed: entries still spreading
      removals              REMOVED records (TREMOVE; evictions leave no record)
      false_removals        {"total", "crashed_later", "never_crashed"}: those logged while the subject
                            was alive, split by whether the subject is in failed_mask
      fade                  the timeline's held column, int64 [t] (None without a timeline)
    """
    rec = np.asarray(records)
    crashed = np.asarray(failed_mask, dtype=bool)
    if rec.shape != crashed.shape or rec.ndim != 1:
        raise ValueError(f"records {rec.shape} and failed_mask {crashed.shape} must be 1-D and of one length")
    tl = None if timeline is None else np.asarray(timeline)
    if tl is not None and (tl.ndim != 2 or tl.shape[1] != 5 or tl.shape[0] < 1):
        raise ValueError(f"timeline {tl.shape} must be [t, 5] with t >= 1")
    last_held = rec["last_held"].astype(np.int64)
    if tl is not None:
        last_tick = tl.shape[0] - 1
    else:
        last_tick = int(max(last_held.max(initial=-1), rec["last_removed"].astype(np.int64).max(initial=-1)))
    ncrashed = int(crashed.sum())
    ever = crashed & (last_held >= 0)
    lat = {"min": None, "mean": None, "max": None}
    if ever.any():
        d = last_held[ever] + 1 - rec["fail_tick"][ever].astype(np.int64)
        lat = {"min": int(d.min()), "mean": float(d.mean()), "max": int(d.max())}
    false = rec["false_removals"].astype(np.int64)
    return {"extinct": int((last_held[crashed] < last_tick).sum()) / ncrashed if ncrashed else 1.0,
            "forget_latency": lat,
            "stale_observer_ticks": int(rec["held_sum"].astype(np.int64).sum()),
            "late_joins": int(rec["late_joins"].astype(np.int64).sum()),
            "removals": int(rec["removals"].astype(np.int64).sum()),
            "false_removals": {"total": int(false.sum()), "crashed_later": int(false[crashed].sum()),
                               "never_crashed": int(false[~crashed].sum())},
            "fade": None if tl is None else tl[:, 3].astype(np.int64)}
