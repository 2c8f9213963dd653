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

from . import digest as _digest
from .abi import default_chunk_rows

KEYS = ("t", "hb", "ts", "heartbeat", "failed", "targets", "counts")
NODE_KEYS = ("t", "heartbeat", "failed", "targets", "counts")  # everything but the tables (save_dir's nodes.npz)


def _chunk_rows(width, chunk_rows):
    """rows per block: as given, else about 64 MiB of (hb, ts) or views (the loads' default)"""
    return max(1, int(chunk_rows)) if chunk_rows is not None else default_chunk_rows(width)


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


def _nodes(sim, view=False, failed=None):
    """Everything of a snapshot but the tables. view: of a PARTIAL context (a view snapshot) -- with n0,
    and `failed` the flags of the whole cluster: the caller's (default 0), this context's own nodes' read."""
    st = sim.read_nodes()
    tg, cnt = sim.read_targets()
    out = {"t": int(sim.time), "heartbeat": st[:, 3].copy(), "failed": st[:, 2].copy(), "targets": tg, "counts": cnt}
    if view:
        n0, nloc = sim.shard_layout()
        cluster = np.zeros(sim.n, dtype=np.int32) if failed is None else np.array(failed, dtype=np.int32).reshape(sim.n)
        cluster[n0:n0 + nloc] = out["failed"]
        out.update(n0=n0, failed=cluster)
    return out


def _save_dir(path, names, dtype, shape, fill, nodes, keys):
    """The directory form of a state: the tables `names` (.npy, dtype [rows][width] = shape, created
    memory-mapped and written by fill(*tables)) and nodes.npz (the `keys` of `nodes`, int32)."""
    os.makedirs(path, exist_ok=True)
    tables = [np.lib.format.open_memmap(os.path.join(path, name + ".npy"), mode="w+", dtype=dtype, shape=shape)
              for name in names]
    fill(*tables)
    for a in tables:
        a.flush()
    del tables
    with open(os.path.join(path, "nodes.npz"), "wb") as f:
        np.savez(f, **{k: np.asarray(nodes[k], dtype=np.int32) for k in keys})


def _load_dir(path, names, keys):
    """What _save_dir wrote as a snapshot: the tables memory-mapped read-only, t and n0 as int."""
    with np.load(os.path.join(path, "nodes.npz")) as z:
        missing = [k for k in keys if k not in z.files]
        if missing:
            raise ValueError(f"{path}: nodes.npz lacks {missing}")
        snap = {k: int(z[k]) if k in ("t", "n0") else z[k].copy() for k in keys}
    for name in names:
        snap[name] = np.load(os.path.join(path, name + ".npy"), mmap_mode="r")
    return snap


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


def verify(sim, snap):
    """Does the SCALED context hold the snapshot's state? Compares sim.digest(), computed where the state
    lives, with the snapshot's (membership.digest.of_snapshot, block by block over memory-mapped tables):
    the check after a restore that reads no table back. snap is full-width or already cut to the
    context's columns; returns the node indices whose row word or node word differ (empty: equal)."""
    c0, w = sim.shard_layout()
    if snap["hb"].shape[1] != w:
        snap = slice_columns(snap, (c0, w))
    return _digest.diff(sim.digest(), _digest.of_snapshot(snap, c0))


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
    _save_dir(path, ("hb", "ts"), np.int32, (sim.n, sim.shard_layout()[1]),
              lambda hb, ts: _read_blocks(sim, hb, ts, chunk_rows), _nodes(sim), NODE_KEYS)


def load_dir(path):
    """The snapshot save_dir wrote, hb / ts memory-mapped read-only (restore loads them block by block)."""
    return _load_dir(path, ("hb", "ts"), NODE_KEYS)


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


# ---------------------------------------------------------------------------- PARTIAL view states
# A view snapshot is a dict of
#   t          the next tick to run
#   n0         the first node the snapshot covers (a row shard's n0; 0 for a cluster snapshot)
#   views      uint64 [nloc][V]: the nodes' final views of tick t - 1 (read_views: id << 32 | hb, 0 = empty)
#   heartbeat  int32 [nloc];  failed int32 [n]: the crash flags of the WHOLE cluster, in every snapshot
#   targets    int32 [nloc][5], counts int32 [nloc]: the targets drawn in tick t - 1 (read_targets)
# which is everything gm_load_views_begin / gm_load_views / gm_load_views_commit take
# (Simulator.load_views). It does not depend on the layout: a cluster snapshot cuts into row shards'
# snapshots (slice_rows with each shard's shard_layout()) and the shards' snapshots join back
# (join_rows). A row shard knows its own nodes' flags only, so view_snapshot of a shard takes the
# cluster's flags from the caller (`failed`), or leaves the other nodes' flags 0 for join_rows to fill.
VIEW_KEYS = ("t", "n0", "views", "heartbeat", "failed", "targets", "counts")
VIEW_NODE_KEYS = ("t", "n0", "heartbeat", "failed", "targets", "counts")  # view_save_dir's nodes.npz


def _check_view_snap(snap):
    missing = [k for k in VIEW_KEYS if k not in snap]
    if missing:
        raise ValueError(f"not a view snapshot: keys {missing} missing")
    views = snap["views"]
    if views.ndim != 2 or views.dtype != np.uint64:
        raise ValueError(f"views must be uint64 [nloc][V], not {views.dtype} {views.shape}")
    nloc, n, n0 = views.shape[0], len(snap["failed"]), int(snap["n0"])
    shapes = {"heartbeat": (nloc,), "counts": (nloc,), "targets": (nloc, 5)}
    for k, want in shapes.items():
        if tuple(np.shape(snap[k])) != want:
            raise ValueError(f"{k} of shape {np.shape(snap[k])}, the views cover {nloc} nodes")
    if n0 < 0 or n0 + nloc > n:
        raise ValueError(f"nodes [{n0}, {n0 + nloc}) of a cluster of {n}")
    return n0, nloc, n


def view_snapshot(sim, failed=None):
    """The state of a PARTIAL context between two ticks (a row shard: its own nodes). failed: the crash
    flags of the whole cluster for a row shard's snapshot (its own nodes' flags are read from it)."""
    n0, nloc = sim.shard_layout()
    return dict(_nodes(sim, True, failed), views=sim.read_views(n0, nloc))


def view_restore(sim, snap, chunk_rows=None):
    """Load a view snapshot into a PARTIAL context that owns exactly its nodes; tick snap["t"] runs next."""
    n0, nloc, n = _check_view_snap(snap)
    if (n0, nloc) != tuple(sim.shard_layout()) or n != sim.n:
        raise ValueError(f"a snapshot of nodes [{n0}, {n0 + nloc}) of {n} for a context of "
                         f"{tuple(sim.shard_layout())} of {sim.n}: cut it with slice_rows")
    sim.load_views(snap["t"], snap["views"], snap["heartbeat"], snap["failed"], snap["targets"], snap["counts"],
                   chunk_rows=chunk_rows)


def view_verify(sim, snap):
    """Does the PARTIAL context hold the view snapshot's state (cut to the context's own nodes where it
    covers more)? Returns the global node indices whose row word or node word differ (empty: equal)."""
    n0, nloc = sim.shard_layout()
    if (int(snap["n0"]), snap["views"].shape[0]) != (n0, nloc):
        snap = slice_rows(snap, n0, nloc)
    return _digest.diff(sim.digest(), _digest.of_view_snapshot(snap))


def slice_rows(snap, n0, nloc):
    """A snapshot cut to the nodes [n0, n0 + nloc) (a row shard's shard_layout()); failed stays the cluster's."""
    s0, sl, _ = _check_view_snap(snap)
    if nloc <= 0 or n0 < s0 or n0 + nloc > s0 + sl:
        raise ValueError(f"nodes [{n0}, {n0 + nloc}) of a snapshot of nodes [{s0}, {s0 + sl})")
    a, b = n0 - s0, n0 - s0 + nloc
    out = dict(snap)
    out["n0"] = int(n0)
    for k in ("views", "heartbeat", "targets", "counts"):
        out[k] = np.ascontiguousarray(snap[k][a:b])
    return out


def join_rows(snaps):
    """The row shards' snapshots (ascending, adjacent node ranges) as one snapshot. Each node's crash flag
    is taken from the snapshot that covers it; nodes no snapshot covers keep the first one's flag."""
    lay = [_check_view_snap(s) for s in snaps]
    first = snaps[0]
    for s, (n0, _, n), (p0, pl, _) in zip(snaps[1:], lay[1:], lay[:-1]):
        if s["t"] != first["t"] or n != lay[0][2] or n0 != p0 + pl or s["views"].shape[1] != first["views"].shape[1]:
            raise ValueError("the snapshots are not adjacent row ranges of one tick of one cluster")
    out = dict(first)
    for k in ("views", "heartbeat", "targets", "counts"):
        out[k] = np.concatenate([s[k] for s in snaps])
    failed = np.array(first["failed"], dtype=np.int32)
    for s, (n0, nloc, _) in zip(snaps, lay):
        failed[n0:n0 + nloc] = np.asarray(s["failed"])[n0:n0 + nloc]
    out["failed"] = failed
    return out


def view_save_dir(sim, path, chunk_rows=None, failed=None):
    """Stream the state of a PARTIAL context to the directory `path`: views.npy (uint64 [nloc][V], written
    block by block through read_views, chunk_rows nodes at a time) and nodes.npz (the other keys)."""
    n0, nloc = sim.shard_layout()
    v = sim.cfg.view or 32

    def fill(views):
        m = min(nloc, _chunk_rows(v, chunk_rows))
        for r0 in range(0, nloc, m):
            k = min(m, nloc - r0)
            views[r0:r0 + k] = sim.read_views(n0 + r0, k)
    _save_dir(path, ("views",), np.uint64, (nloc, v), fill, _nodes(sim, True, failed), VIEW_NODE_KEYS)


def view_load_dir(path):
    """The snapshot view_save_dir wrote, views memory-mapped read-only (view_restore loads them block by block)."""
    snap = _load_dir(path, ("views",), VIEW_NODE_KEYS)
    _check_view_snap(snap)
    return snap
