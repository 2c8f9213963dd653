"""The SCALED state between two ticks as plain arrays: take it from a context, keep it, move it.

A snapshot is a dict of
  t          the next tick to run
  hb, ts     int32 [n][w]: every row's entries over the context's columns, -1 = absent (read_table)
  heartbeat  int32 [n]: the heartbeat counters; failed int32 [n]: the crash flags (read_nodes)
  targets    int32 [n][5], counts int32 [n]: the gossip targets drawn in the last tick (read_targets)
which is everything gm_load_begin / gm_load_rows / gm_load_commit take (Simulator.load_state) and
everything the oracle's load_state takes. It is independent of the layout: a snapshot of a context
of one band width restores into another, a single context's snapshot slices into column shards
(slice_columns with each shard's shard_layout()) and the shards' snapshots join back (join_columns).
A column shard's snapshot holds its own columns and the same node arrays as every other shard's,
except that a shard bumps the heartbeat counters of the nodes whose columns it holds only: its
`heartbeat` is current for those nodes (which is all a load into that shard checks and uses), and
join_columns takes each node's counter from the shard that holds its column.
"""
import numpy as np

KEYS = ("t", "hb", "ts", "heartbeat", "failed", "targets", "counts")


def snapshot(sim):
    """The state of a SCALED context between two ticks (a column shard: its own columns)."""
    hb, ts = sim.read_table()
    st = sim.read_nodes()
    tg, cnt = sim.read_targets()
    return {"t": int(sim.time), "hb": hb, "ts": ts, "heartbeat": st[:, 3].copy(), "failed": st[:, 2].copy(),
            "targets": tg, "counts": cnt}


def restore(sim, snap, chunk_rows=None):
    """Load a snapshot into a SCALED context (created with init_mode 0 or 1); tick snap["t"] runs next."""
    sim.load_state(snap["t"], snap["hb"], snap["ts"], snap["heartbeat"], snap["failed"], snap["targets"],
                   snap["counts"], chunk_rows=chunk_rows)


def save(snap, path):
    """Write a snapshot with np.savez (one .npz file; `path` is used as given)."""
    with open(path, "wb") as f:
        np.savez(f, **{k: np.asarray(snap[k], dtype=np.int32) for k in KEYS})


def load(path):
    with np.load(path) as z:
        snap = {k: z[k].copy() for k in KEYS}
    snap["t"] = int(snap["t"])
    return snap


def slice_columns(snap, layout):
    """A full-width snapshot cut to a column shard: layout = the shard's shard_layout() = (c0, w)."""
    c0, w = layout
    n = snap["hb"].shape[0]
    if snap["hb"].shape[1] != n or c0 < 0 or w <= 0 or c0 + w > n:
        raise ValueError(f"columns [{c0}, {c0 + w}) of a snapshot of shape {snap['hb'].shape}")
    out = dict(snap)
    out["hb"] = np.ascontiguousarray(snap["hb"][:, c0:c0 + w])
    out["ts"] = np.ascontiguousarray(snap["ts"][:, c0:c0 + w])
    return out


def join_columns(snaps):
    """The shards' snapshots (in rank order) as one full-width snapshot."""
    first = snaps[0]
    for s in snaps[1:]:
        if s["t"] != first["t"] or any(not np.array_equal(s[k], first[k]) for k in ("failed", "targets", "counts")):
            raise ValueError("the shards' snapshots are not of one tick of one cluster")
    out = dict(first)
    out["hb"] = np.concatenate([s["hb"] for s in snaps], axis=1)
    out["ts"] = np.concatenate([s["ts"] for s in snaps], axis=1)
    if out["hb"].shape[0] != out["hb"].shape[1]:
        raise ValueError(f"the shards' columns do not add up to the rows: {out['hb'].shape}")
    c0 = np.cumsum([0] + [s["hb"].shape[1] for s in snaps])
    out["heartbeat"] = np.concatenate([s["heartbeat"][c0[g]:c0[g + 1]] for g, s in enumerate(snaps)])
    return out
