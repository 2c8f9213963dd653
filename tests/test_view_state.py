"""membership.state's PARTIAL view snapshots without a GPU: slice_rows / join_rows between a cluster
snapshot and its row shards', view_save_dir / view_load_dir block by block and memory-mapped, and the
validation of keys and shapes."""
import numpy as np
import pytest

from membership import Simulator, state


def _view_snapshot(n=23, v=8, t=15, seed=3):
    """a well-formed view state of n nodes: own entry + sorted peers, targets out of the view"""
    rng = np.random.default_rng(seed)
    views = np.zeros((n, v), dtype=np.uint64)
    targets = np.zeros((n, 5), dtype=np.int32)
    counts = np.zeros(n, dtype=np.int32)
    for i in range(n):
        peers = rng.choice([j for j in range(n) if j != i], size=v - 2, replace=False)
        ids = np.sort(np.append(peers, i)) + 1
        hb = np.where(ids == i + 1, 2 * (t - 1) - 1, 2 * (t - 2) - 1)
        views[i, :len(ids)] = (ids.astype(np.uint64) << np.uint64(32)) | hb.astype(np.uint64)
        counts[i] = i % 6
        targets[i, :counts[i]] = peers[:counts[i]]
    failed = np.zeros(n, dtype=np.int32)
    failed[[2, 17]] = 1
    return {"t": t, "n0": 0, "views": views, "heartbeat": np.full(n, 2 * (t - 1), dtype=np.int32), "failed": failed,
            "targets": targets, "counts": counts}


class FakeViewSim:
    """what state.view_snapshot / view_save_dir / view_restore use of a Simulator, over a snapshot's arrays"""

    def __init__(self, snap, view=8):
        self.snap = snap
        self.n = len(snap["failed"])
        self.n0, self.nloc = snap["n0"], snap["views"].shape[0]
        self.time = snap["t"]
        self.cfg = type("Cfg", (), {"view": view})()
        self.asked = []
        self.loaded = None

    def shard_layout(self):
        return self.n0, self.nloc

    def read_views(self, r0, count):
        self.asked.append((r0, count))
        assert self.n0 <= r0 and r0 + count <= self.n0 + self.nloc
        return self.snap["views"][r0 - self.n0:r0 - self.n0 + count].copy()

    def read_nodes(self):
        st = np.zeros((self.nloc, 4), dtype=np.int32)
        st[:, 2] = self.snap["failed"][self.n0:self.n0 + self.nloc]
        st[:, 3] = self.snap["heartbeat"]
        return st

    def read_targets(self):
        return self.snap["targets"].copy(), self.snap["counts"].copy()

    def load_views(self, t, views, heartbeat, failed, targets, counts, chunk_rows=None):
        self.loaded = dict(t=t, views=views, heartbeat=heartbeat, failed=failed, targets=targets, counts=counts,
                           chunk_rows=chunk_rows)


def _same(a, b):
    assert set(a) == set(b) == set(state.VIEW_KEYS)
    assert a["t"] == b["t"] and a["n0"] == b["n0"]
    for k in state.VIEW_KEYS[2:]:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("world", [1, 2, 3, 5])
def test_slice_rows_and_join_rows_are_inverses(world):
    snap = _view_snapshot()
    n = 23
    cuts = [n * g // world for g in range(world + 1)]
    parts = [state.slice_rows(snap, cuts[g], cuts[g + 1] - cuts[g]) for g in range(world)]
    for g, p in enumerate(parts):
        assert p["n0"] == cuts[g] and p["views"].shape == (cuts[g + 1] - cuts[g], 8) and p["views"].flags["C_CONTIGUOUS"]
        assert np.array_equal(p["failed"], snap["failed"]), "failed stays the whole cluster's"
        assert np.array_equal(p["targets"], snap["targets"][cuts[g]:cuts[g + 1]])
    _same(state.join_rows(parts), snap)
    # a slice of a slice, and a join of part of the cluster
    if world >= 3:
        mid = state.join_rows(parts[1:3])
        assert mid["n0"] == cuts[1] and mid["views"].shape[0] == cuts[3] - cuts[1]
        _same(state.slice_rows(mid, cuts[2], cuts[3] - cuts[2]), parts[2])


def test_join_rows_takes_each_nodes_flag_from_its_own_shard():
    """a row shard knows its own nodes' flags only: view_snapshot leaves the others 0, join_rows fills them in"""
    snap = _view_snapshot()
    shards = [FakeViewSim(state.slice_rows(snap, a, b - a)) for a, b in ((0, 7), (7, 15), (15, 23))]
    got = [state.view_snapshot(s) for s in shards]
    assert [int(g["failed"].sum()) for g in got] == [1, 0, 1]
    _same(state.join_rows(got), snap)
    full = state.view_snapshot(shards[1], failed=snap["failed"])
    assert np.array_equal(full["failed"], snap["failed"])


def test_join_rows_rejects_what_is_not_one_cluster_state():
    snap = _view_snapshot()
    a, b, c = (state.slice_rows(snap, lo, hi - lo) for lo, hi in ((0, 7), (7, 15), (15, 23)))
    with pytest.raises(ValueError):
        state.join_rows([a, c])  # not adjacent
    with pytest.raises(ValueError):
        state.join_rows([b, a])  # not ascending
    with pytest.raises(ValueError):
        state.join_rows([a, dict(b, t=16)])
    with pytest.raises(ValueError):
        state.join_rows([a, dict(b, views=np.zeros((8, 4), dtype=np.uint64))])  # another view width


def test_key_and_shape_validation():
    snap = _view_snapshot()
    for k in state.VIEW_KEYS:
        bad = dict(snap)
        del bad[k]
        with pytest.raises(ValueError, match=k):
            state.slice_rows(bad, 0, 5)
    with pytest.raises(ValueError):
        state.slice_rows(dict(snap, views=snap["views"].astype(np.int64)), 0, 5)
    with pytest.raises(ValueError):
        state.slice_rows(dict(snap, heartbeat=snap["heartbeat"][:-1]), 0, 5)
    with pytest.raises(ValueError):
        state.slice_rows(dict(snap, targets=snap["targets"][:, :4]), 0, 5)
    with pytest.raises(ValueError):
        state.slice_rows(dict(snap, failed=snap["failed"][:10]), 0, 5)  # nodes past the cluster
    for n0, nloc in ((-1, 3), (20, 4), (5, 0)):
        with pytest.raises(ValueError):
            state.slice_rows(snap, n0, nloc)
    part = state.slice_rows(snap, 7, 8)
    with pytest.raises(ValueError):
        state.slice_rows(part, 0, 8)  # outside the part
    with pytest.raises(ValueError):
        state.view_restore(FakeViewSim(snap), part)  # a shard's snapshot for a whole-cluster context
    dst = FakeViewSim(part)
    state.view_restore(dst, part, chunk_rows=3)
    assert dst.loaded["t"] == 15 and dst.loaded["chunk_rows"] == 3 and dst.loaded["views"] is part["views"]


@pytest.mark.parametrize("chunk_rows", [3, 8, 100, None])
def test_view_save_dir_streams_blocks_and_view_load_dir_maps_them(tmp_path, chunk_rows):
    snap = state.slice_rows(_view_snapshot(), 7, 8)
    sim = FakeViewSim(snap)
    path = tmp_path / "views"
    state.view_save_dir(sim, path, chunk_rows=chunk_rows, failed=snap["failed"])
    assert sorted(p.name for p in path.iterdir()) == ["nodes.npz", "views.npy"]
    cap = 8 if chunk_rows is None else min(chunk_rows, 8)
    assert all(0 < c <= cap for _, c in sim.asked), sim.asked
    assert sorted(r for r0, c in sim.asked for r in range(r0, r0 + c)) == list(range(7, 15)), "every node once"
    a = np.load(path / "views.npy")
    assert a.dtype == np.uint64 and a.shape == (8, 8) and a.tobytes() == snap["views"].tobytes()
    with np.load(path / "nodes.npz") as z:
        assert sorted(z.files) == sorted(state.VIEW_NODE_KEYS)
    got = state.view_load_dir(path)
    assert isinstance(got["views"], np.memmap) and got["views"].dtype == np.uint64 and got["views"].flags["C_CONTIGUOUS"]
    assert isinstance(got["t"], int) and isinstance(got["n0"], int)
    _same(got, snap)
    dst = FakeViewSim(snap)
    state.view_restore(dst, got, chunk_rows=5)
    assert dst.loaded["views"] is got["views"] and dst.loaded["chunk_rows"] == 5


class _LoadLib:
    """gm_load_views_* of libgm, recording what Simulator.load_views hands over"""

    def __init__(self, v):
        self.v, self.blocks, self.t, self.commit = v, [], None, None

    def gm_load_views_begin(self, h, t):
        self.t = t
        return 0

    def gm_load_views(self, h, r0, m, views):
        self.blocks.append((r0, m, np.ctypeslib.as_array(views, shape=(m, self.v)).copy()))
        return 0

    def gm_load_views_commit(self, h, hb, failed, targets, counts):
        self.commit = (np.ctypeslib.as_array(hb, shape=(8,)).copy(), np.ctypeslib.as_array(failed, shape=(23,)).copy(),
                       np.ctypeslib.as_array(targets, shape=(8, 5)).copy(), np.ctypeslib.as_array(counts, shape=(8,)).copy())
        return 0


def test_load_views_feeds_mapped_views_block_by_block(tmp_path):
    snap = state.slice_rows(_view_snapshot(), 7, 8)
    state.view_save_dir(FakeViewSim(snap), tmp_path / "s", failed=snap["failed"])
    got = state.view_load_dir(tmp_path / "s")
    sim = object.__new__(Simulator)  # no context: the library calls are recorded
    sim.lib, sim.h, sim.n = _LoadLib(8), None, 23
    sim.cfg = type("Cfg", (), {"view": 8})()
    sim.shard_layout = lambda: (7, 8)
    state.view_restore(sim, got, chunk_rows=3)
    lib = sim.lib
    assert lib.t == 15 and [(r0, m) for r0, m, _ in lib.blocks] == [(7, 3), (10, 3), (13, 2)]  # global node indices
    assert np.array_equal(np.concatenate([b[2] for b in lib.blocks]), snap["views"])
    for got_a, k in zip(lib.commit, ("heartbeat", "failed", "targets", "counts")):
        assert np.array_equal(got_a, snap[k]), k
    with pytest.raises(ValueError):
        sim.load_views(15, snap["views"][:, :4], snap["heartbeat"], snap["failed"], snap["targets"], snap["counts"])
