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

At the sizes the project is built for, the tables do not fit a host's memory comfortably (S-A: two
17 GB arrays), and read_table copies the whole stored state to the host to decode it there.
snapshot(device=True) reads through read_rows instead (decoded on the device, block by block);
save_dir streams a state to a directory block by block, and load_dir returns it with hb / ts
memory-mapped, which restore loads block by block: the whole table is never in memory.
"""
import os

import numpy as np

KEYS = ("t", "hb", "ts", "heartbeat", "failed", "targets", "counts")
NODE_KEYS = ("t", "heartbeat", "failed", "targets", "counts")  # everything but the tables (save_dir's nodes.npz)


def _chunk_rows(w, chunk_rows):
    """rows per block: as given, else about 64 MiB of (hb, ts) (Simulator.load_state's default)"""
    return max(1, int(chunk_rows)) if chunk_rows is not None else max(1, (64 << 20) // (8 * w))


def _read_blocks(sim, hb, ts, chunk_rows):
    """rows [0, n) through read_rows into hb / ts [n][w], block by block"""
    n, w = hb.shape
    m = min(n, _chunk_rows(w, chunk_rows))
    buf = (np.empty((m, w), dtype=np.int32), np.empty((m, w), dtype=np.int32))
    for r0 in range(0, n, m):
        k = min(m, n - r0)
        bh, bt = sim.read_rows(r0, k, out=buf)
        hb[r0:r0 + k] = bh
        ts[r0:r0 + k] = bt


def _nodes(sim):
    st = sim.read_nodes()
    tg, cnt = sim.read_targets()
    return {"t": int(sim.time), "heartbeat": st[:, 3].copy(), "failed": st[:, 2].copy(), "targets": tg, "counts": cnt}


def snapshot(sim, device=False, chunk_rows=None):
    """The state of a SCALED context between two ticks (a column shard: its own columns).
    device=True: the tables are decoded on the device and read in blocks of chunk_rows rows
    (read_rows); the default reads them through read_table."""
    if device:
        w = sim.shard_layout()[1]
        hb, ts = np.empty((sim.n, w), dtype=np.int32), np.empty((sim.n, w), dtype=np.int32)
        _read_blocks(sim, hb, ts, chunk_rows)
    else:
        hb, ts = sim.read_table()
    return dict(_nodes(sim), hb=hb, ts=ts)


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


def save_dir(sim, path, chunk_rows=None):
    """Stream the state of a SCALED context to the directory `path`: hb.npy / ts.npy (int32 [n][w], written
    block by block through read_rows, chunk_rows rows at a time) and nodes.npz (t, heartbeat, failed,
    targets, counts)."""
    os.makedirs(path, exist_ok=True)
    w = sim.shard_layout()[1]
    planes = [np.lib.format.open_memmap(os.path.join(path, name), mode="w+", dtype=np.int32, shape=(sim.n, w))
              for name in ("hb.npy", "ts.npy")]
    _read_blocks(sim, planes[0], planes[1], chunk_rows)
    for p in planes:
        p.flush()
    del planes
    nodes = _nodes(sim)
    with open(os.path.join(path, "nodes.npz"), "wb") as f:
        np.savez(f, **{k: np.asarray(nodes[k], dtype=np.int32) for k in NODE_KEYS})


def load_dir(path):
    """The snapshot save_dir wrote, hb / ts memory-mapped read-only (restore loads them block by block)."""
    with np.load(os.path.join(path, "nodes.npz")) as z:
        snap = {k: z[k].copy() for k in NODE_KEYS}
    snap["t"] = int(snap["t"])
    snap["hb"] = np.load(os.path.join(path, "hb.npy"), mmap_mode="r")
    snap["ts"] = np.load(os.path.join(path, "ts.npy"), mmap_mode="r")
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
