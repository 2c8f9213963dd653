"""Layout-independent digests of the state between two ticks: the definition of include/gm_abi.h
(GM_DIGEST_VERSION 1) in NumPy.

This module is the specification the device kernels (gm_digest, Simulator.digest) are tested against:
nothing here calls the library. All arithmetic is mod 2^64 (uint64 arrays wrap).

    kcol(c)         = mix(KCOL ^ c)                         c = global subject index (id - 1)
    cell(c, hb, ts) = mix(kcol(c) ^ (hb << 32 | ts))
    rows[r]         = sum of cell over the present entries (hb >= 0) of observer r
    knode(r)        = mix(KNODE ^ r)
    nodes[r]        = mix(knode(r) ^ (heartbeat << 8 | count << 3 | failed << 2 | inGroup << 1 | inited))
                      + sum over q < count of mix(mix(knode(r) + q + 1) ^ target_q)
    fold(r, x)      = mix(mix(KROW ^ r) ^ x)
    table = sum of fold(r, rows[r]),  nodes = sum of fold(r, node_words[r])

A digest is a dict of `table`, `nodes` (ints), `rows`, `node_words` (uint64 arrays) and `r0`, the global
index of the first node the arrays cover. A SCALED column shard's words cover its own columns (node
words 0 outside them) and add up over the shards (merge_columns); a PARTIAL row shard's arrays cover
its own nodes and concatenate (merge_rows).
"""
import numpy as np

VERSION = 1
KCOL = np.uint64(0x6D656D6265727368)
KNODE = np.uint64(0x6E6F646573746174)
KROW = np.uint64(0x726F77666F6C6421)
_M1, _M2 = np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)
_S30, _S27, _S31, _S32 = np.uint64(30), np.uint64(27), np.uint64(31), np.uint64(32)
BLOCK_ROWS = 256  # rows hashed at a time by the snapshot digests


def _u64(a):
    """integers as uint64, negative ones sign-extended (as a C cast does)"""
    return np.asarray(a).astype(np.int64).astype(np.uint64)


def mix(z):
    """splitmix64's finalizer (gm_mix64) over a uint64 array"""
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> _S30)) * _M1
        z = (z ^ (z >> _S27)) * _M2
    return z ^ (z >> _S31)


def _sum(a, axis=None):
    return np.add.reduce(np.asarray(a, dtype=np.uint64), axis=axis, dtype=np.uint64)


def kcol(c):
    return mix(KCOL ^ _u64(c))


def row_words(hb, ts, c0=0):
    """rows[r] of the dense block hb / ts [rows][w] over the columns [c0, c0 + w); -1 = absent"""
    hb, ts = np.asarray(hb), np.asarray(ts)
    k = kcol(c0 + np.arange(hb.shape[1]))
    v = mix(k[None, :] ^ ((_u64(hb) << _S32) | (_u64(ts) & np.uint64(0xFFFFFFFF))))
    return _sum(np.where(hb >= 0, v, np.uint64(0)), axis=1)


def view_words(views):
    """rows[r] of raw views uint64 [rows][V] (id << 32 | hb, 0 = empty): c = id - 1, ts = (hb + 1) / 2"""
    views = np.asarray(views, dtype=np.uint64)
    ident, hb = views >> _S32, views & np.uint64(0xFFFFFFFF)
    with np.errstate(over="ignore"):
        v = mix(mix(KCOL ^ (ident - np.uint64(1))) ^ ((hb << _S32) | ((hb + np.uint64(1)) >> np.uint64(1))))
    return _sum(np.where(views != 0, v, np.uint64(0)), axis=1)


def node_words(state4, targets, counts, r0=0):
    """nodes[r] of the nodes [r0, r0 + len): state4 [.][4] = inited, inGroup, failed, heartbeat
    (read_nodes), targets [.][5] in draw order and counts (read_targets); slots >= count are not read"""
    st, tg, cnt = _u64(state4).reshape(-1, 4), _u64(targets).reshape(-1, 5), np.asarray(counts).reshape(-1)
    kn = mix(KNODE ^ _u64(r0 + np.arange(len(cnt))))
    word = (st[:, 3] << np.uint64(8)) | (_u64(cnt) << np.uint64(3)) | (st[:, 2] << np.uint64(2)) \
        | (st[:, 1] << np.uint64(1)) | st[:, 0]
    out = mix(kn ^ word)
    with np.errstate(over="ignore"):
        for q in range(5):
            out = out + np.where(cnt > q, mix(mix(kn + np.uint64(q + 1)) ^ tg[:, q]), np.uint64(0))
    return out


def fold(words, r0=0):
    """sum of fold(r0 + i, words[i]) as an int"""
    words = np.asarray(words, dtype=np.uint64)
    return int(_sum(mix(mix(KROW ^ _u64(r0 + np.arange(len(words)))) ^ words)))


def _digest(rows, nodes, r0=0):
    return {"table": fold(rows, r0), "nodes": fold(nodes, r0), "rows": rows, "node_words": nodes, "r0": int(r0)}


def reference(hb, ts, state4, targets, counts, c0=0, block_rows=BLOCK_ROWS):
    """The digest of a SCALED state: hb / ts int32 [n][w] over the columns [c0, c0 + w) (-1 = absent), the
    node arrays over all n nodes. The node words are 0 outside [c0, c0 + w), as a column shard's. The
    table is hashed block_rows rows at a time, so memory-mapped tables never load whole."""
    n, w = hb.shape
    rows = np.zeros(n, dtype=np.uint64)
    for r in range(0, n, block_rows):
        rows[r:r + block_rows] = row_words(hb[r:r + block_rows], ts[r:r + block_rows], c0)
    nodes = node_words(state4, targets, counts)
    own = np.zeros(n, dtype=bool)
    own[c0:c0 + w] = True
    return _digest(rows, np.where(own, nodes, np.uint64(0)))


def reference_views(views, state4, targets, counts, n0=0, block_rows=BLOCK_ROWS):
    """The digest of a PARTIAL state: views uint64 [nloc][V] and the node arrays of the nodes [n0, n0 + nloc)"""
    nloc = views.shape[0]
    rows = np.zeros(nloc, dtype=np.uint64)
    for r in range(0, nloc, block_rows):
        rows[r:r + block_rows] = view_words(views[r:r + block_rows])
    return _digest(rows, node_words(state4, targets, counts, n0), n0)


def _snap_state4(snap, lo, hi):
    """read_nodes' words of a snapshot's nodes: loadable states have every node started and in the group"""
    st = np.ones((hi - lo, 4), dtype=np.int64)
    st[:, 2] = np.asarray(snap["failed"])[lo:hi]
    st[:, 3] = np.asarray(snap["heartbeat"])
    return st


def of_snapshot(snap, c0=0, block_rows=BLOCK_ROWS):
    """The digest of a SCALED snapshot (membership.state: snapshot / load_dir dicts, memory-mapped tables
    included) whose tables cover the columns [c0, c0 + w)"""
    n = snap["hb"].shape[0]
    return reference(snap["hb"], snap["ts"], _snap_state4(snap, 0, n), snap["targets"], snap["counts"], c0, block_rows)


def of_view_snapshot(snap, block_rows=BLOCK_ROWS):
    """The digest of a PARTIAL view snapshot (membership.state: view_snapshot / view_load_dir dicts)"""
    n0, nloc = int(snap["n0"]), snap["views"].shape[0]
    return reference_views(snap["views"], _snap_state4(snap, n0, n0 + nloc), snap["targets"], snap["counts"], n0,
                           block_rows)


def merge_columns(parts):
    """The cluster's digest from its column shards': the words add up, the sums are folded from them"""
    with np.errstate(over="ignore"):
        rows = np.add.reduce([np.asarray(p["rows"], dtype=np.uint64) for p in parts], dtype=np.uint64)
        nodes = np.add.reduce([np.asarray(p["node_words"], dtype=np.uint64) for p in parts], dtype=np.uint64)
    return _digest(rows, nodes)


def merge_rows(parts):
    """The cluster's digest from its row shards' (ascending node ranges): the words concatenate, the sums add"""
    mask = (1 << 64) - 1
    out = _digest(np.concatenate([p["rows"] for p in parts]), np.concatenate([p["node_words"] for p in parts]),
                  parts[0].get("r0", 0))
    out["table"] = sum(int(p["table"]) for p in parts) & mask
    out["nodes"] = sum(int(p["nodes"]) for p in parts) & mask
    return out


def diff(a, b):
    """The node indices (global) whose row word or node word differ between two digests of equal cover"""
    if len(a["rows"]) != len(b["rows"]) or a.get("r0", 0) != b.get("r0", 0):
        raise ValueError("digests of different node ranges")
    bad = (np.asarray(a["rows"]) != np.asarray(b["rows"])) | (np.asarray(a["node_words"]) != np.asarray(b["node_words"]))
    return np.flatnonzero(bad) + int(a.get("r0", 0))
