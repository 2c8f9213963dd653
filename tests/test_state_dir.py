"""membership.state's directory form without a GPU: save_dir streams a context's state block by block
(read_rows), load_dir hands it back with the tables memory-mapped, and restore / Simulator.load_state
feed such tables to gm_load_rows block by block without copying them whole."""
import numpy as np
import pytest

from membership import Simulator, state
from test_state_snapshot import _snapshot


class FakeSim:
    """what state.snapshot / save_dir use of a Simulator, over a snapshot's arrays (a column shard's: w < n)"""

    def __init__(self, snap):
        self.snap = snap
        self.n, self.w = snap["hb"].shape
        self.time = snap["t"]
        self.asked = []   # (r0, count) of every read_rows call
        self.loaded = None

    def shard_layout(self):
        return 0, self.w

    def read_table(self):
        raise AssertionError("the directory route must not read the whole table")

    def read_rows(self, r0=0, count=None, out=None):
        count = self.n - r0 if count is None else count
        self.asked.append((r0, count))
        hb, ts = self.snap["hb"][r0:r0 + count], self.snap["ts"][r0:r0 + count]
        if out is None:
            return hb.copy(), ts.copy()
        got = tuple(a.reshape(-1)[:count * self.w].reshape(count, self.w) for a in out)
        got[0][:], got[1][:] = hb, ts
        return got

    def read_nodes(self):
        st = np.zeros((self.n, 4), dtype=np.int32)
        st[:, 2], st[:, 3] = self.snap["failed"], self.snap["heartbeat"]
        return st

    def read_targets(self):
        return self.snap["targets"].copy(), self.snap["counts"].copy()

    def load_state(self, t, hb, ts, heartbeat, failed, targets, counts, chunk_rows=None):
        self.loaded = dict(t=t, hb=hb, ts=ts, heartbeat=heartbeat, failed=failed, targets=targets, counts=counts,
                           chunk_rows=chunk_rows)


def _shard_snapshot(n=21, w=7):
    snap = _snapshot(n)
    return state.slice_columns(snap, (7, w))


@pytest.mark.parametrize("chunk_rows", [4, 21, 100, None])
def test_save_dir_streams_blocks_and_load_dir_maps_them(tmp_path, chunk_rows):
    snap = _shard_snapshot()
    sim = FakeSim(snap)
    path = tmp_path / "state"
    state.save_dir(sim, path, chunk_rows=chunk_rows)
    assert sorted(p.name for p in path.iterdir()) == ["hb.npy", "nodes.npz", "ts.npy"]
    cap = 21 if chunk_rows is None else min(chunk_rows, 21)
    assert all(0 < c <= cap for _, c in sim.asked), sim.asked
    rows = sorted(r for r0, c in sim.asked for r in range(r0, r0 + c))
    assert rows == list(range(21)), "every row exactly once"
    for name in ("hb", "ts"):  # plain .npy files of the table's shape
        a = np.load(path / f"{name}.npy")
        assert a.dtype == np.int32 and a.shape == (21, 7) and a.tobytes() == snap[name].tobytes()
    with np.load(path / "nodes.npz") as z:
        assert sorted(z.files) == sorted(state.NODE_KEYS)
        for k in state.NODE_KEYS:
            assert z[k].dtype == np.int32 and z[k].shape == np.asarray(snap[k]).shape, k
    got = state.load_dir(path)
    assert set(got) == set(state.KEYS) and got["t"] == 41 and isinstance(got["t"], int)
    for name in ("hb", "ts"):
        assert isinstance(got[name], np.memmap) and got[name].dtype == np.int32 and got[name].flags["C_CONTIGUOUS"]
    for k in state.KEYS[1:]:
        assert np.array_equal(got[k], snap[k]), k
    dst = FakeSim(snap)
    state.restore(dst, got, chunk_rows=5)
    assert dst.loaded["chunk_rows"] == 5 and dst.loaded["hb"] is got["hb"] and dst.loaded["t"] == 41


def test_device_snapshot_reads_blocks():
    snap = _shard_snapshot()
    sim = FakeSim(snap)
    got = state.snapshot(sim, device=True, chunk_rows=8)
    assert sim.asked == [(0, 8), (8, 8), (16, 5)]
    assert set(got) == set(state.KEYS)
    for k in state.KEYS:
        assert np.array_equal(got[k], snap[k]), k
    assert got["hb"].dtype == np.int32 and got["hb"].flags["C_CONTIGUOUS"] and got["hb"].shape == (21, 7)


class _LoadLib:
    """gm_load_begin / gm_load_rows / gm_load_commit of libgm, recording what Simulator.load_state hands over"""

    def __init__(self, w):
        self.w, self.blocks, self.t, self.committed = w, [], None, False

    def gm_load_begin(self, h, t):
        self.t = t
        return 0

    def gm_load_rows(self, h, r0, m, hb, ts):
        self.blocks.append((r0, m, np.ctypeslib.as_array(hb, shape=(m, self.w)).copy(),
                            np.ctypeslib.as_array(ts, shape=(m, self.w)).copy()))
        return 0

    def gm_load_commit(self, h, *arrays):
        self.committed = True
        return 0


def test_load_state_feeds_a_mapped_table_block_by_block(tmp_path):
    snap = _shard_snapshot()
    state.save_dir(FakeSim(snap), tmp_path / "s")
    got = state.load_dir(tmp_path / "s")
    # load_state's conversion of a mapped int32 table is a view: nothing is read before its block is
    assert np.shares_memory(np.ascontiguousarray(got["hb"], dtype=np.int32), got["hb"])
    sim = object.__new__(Simulator)  # no context: the library calls are recorded
    sim.lib, sim.h, sim.n = _LoadLib(7), None, 21
    sim.shard_layout = lambda: (7, 7)
    state.restore(sim, got, chunk_rows=8)
    lib = sim.lib
    assert lib.t == 41 and lib.committed and [(r0, m) for r0, m, _, _ in lib.blocks] == [(0, 8), (8, 8), (16, 5)]
    assert np.array_equal(np.concatenate([b[2] for b in lib.blocks]), snap["hb"])
    assert np.array_equal(np.concatenate([b[3] for b in lib.blocks]), snap["ts"])
