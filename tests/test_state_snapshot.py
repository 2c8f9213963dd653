"""membership.state without a context: snapshots on disk, and a full snapshot cut to column shards."""
import numpy as np
import pytest

from membership import state

# gm_shard_layout of the three column shards of N = 21 (n < 8 G: c0 = n g / G), as the contexts of
# tests/test_gpu_detect.py's (21, 3) case report it
LAYOUT_21_3 = [(0, 7), (7, 7), (14, 7)]


def _snapshot(n, seed=3):
    rng = np.random.default_rng(seed)
    ts = rng.integers(-1, 40, size=(n, n)).astype(np.int32)
    hb = np.where(ts < 0, -1, 2 * ts - 1 - rng.integers(0, 3, size=(n, n))).astype(np.int32)
    counts = rng.integers(0, 6, size=n).astype(np.int32)
    targets = rng.integers(0, n, size=(n, 5)).astype(np.int32)
    targets[np.arange(5)[None, :] >= counts[:, None]] = 0
    return {"t": 41, "hb": hb, "ts": ts, "heartbeat": rng.integers(0, 80, size=n).astype(np.int32),
            "failed": rng.integers(0, 2, size=n).astype(np.int32), "targets": targets, "counts": counts}


def test_save_load_round_trip_bit_for_bit(tmp_path):
    snap = _snapshot(21)
    path = tmp_path / "state.npz"
    state.save(snap, path)
    got = state.load(path)
    assert set(got) == set(state.KEYS) and got["t"] == 41 and isinstance(got["t"], int)
    for k in state.KEYS[1:]:
        assert got[k].dtype == np.int32 and got[k].shape == snap[k].shape
        assert got[k].tobytes() == snap[k].tobytes(), k


def test_slice_columns_follows_the_shard_layout():
    n, world = 21, 3
    snap = _snapshot(n)
    assert [(n * g // world, n * (g + 1) // world - n * g // world) for g in range(world)] == LAYOUT_21_3
    parts = [state.slice_columns(snap, lay) for lay in LAYOUT_21_3]
    for (c0, w), p in zip(LAYOUT_21_3, parts):
        assert p["hb"].shape == (n, w) and p["hb"].flags["C_CONTIGUOUS"]
        assert np.array_equal(p["hb"], snap["hb"][:, c0:c0 + w]) and np.array_equal(p["ts"], snap["ts"][:, c0:c0 + w])
        for k in ("t", "heartbeat", "failed", "targets", "counts"):  # the node arrays are every shard's
            assert np.array_equal(p[k], snap[k])
    joined = state.join_columns(parts)
    for k in state.KEYS:
        assert np.array_equal(joined[k], snap[k]), k
    with pytest.raises(ValueError):
        state.slice_columns(snap, (14, 8))  # past the last column
    with pytest.raises(ValueError):
        state.slice_columns(parts[0], (0, 7))  # not a full-width snapshot
    parts[1]["failed"] = 1 - parts[1]["failed"]
    with pytest.raises(ValueError):
        state.join_columns(parts)
