"""What the reference's grader asks of a run -- completeness, accuracy, detection latency -- from
the detection records (Simulator.detect(), gm_detect_rec of include/gm_abi.h). CPU only: plain
NumPy over the records, no GPU handle."""
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
