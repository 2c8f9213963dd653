"""membership.digest, the NumPy definition of the state digest (GM_DIGEST_VERSION 1), without a GPU.

 1. a known answer: a hand-written 3 x 3 state, its words and sums as constants (computed with plain Python
    integers from the definition in include/gm_abi.h)
 2. the oracle's runs reproduce tests/golden/digest/traces.json
 3. what must change the digest changes it, and only the words of the row it touches
 4. column slices add up (merge_columns), row slices concatenate (merge_rows)
 5. of_snapshot over a save_dir-format directory, read in 7-row blocks
"""
import os

import numpy as np
import pytest

import digest_cases
from membership import digest, state

U64 = np.uint64


# ---- 1. a known answer
KAT_HB = np.array([[5, -1, 0], [3, 7, 9], [1, 2, 11]], dtype=np.int32)  # row 0: one absent cell, one {0, 0}
KAT_TS = np.array([[3, -1, 0], [2, 4, 5], [1, 1, 6]], dtype=np.int32)
KAT_ST = np.array([[1, 1, 0, 6], [1, 1, 1, 8], [1, 0, 0, 12]], dtype=np.int32)
KAT_TG = np.array([[9, 9, 9, 9, 9], [2, 0, 7, 7, 7], [0, 1, 2, 1, 0]], dtype=np.int32)  # slots >= count: anything
KAT_CNT = np.array([0, 2, 5], dtype=np.int32)
KAT_ROWS = [0x5C22CA12A8A9F457, 0x1BDAAC0142B6B6EF, 0x9748078E2814A978]
KAT_NODES = [0x16FBFB6652E01308, 0x8673019365FBB5F5, 0x425E9C745F0D81F6]
KAT_SUMS = (0x0C97F6ABC0F81A48, 0x50F9CB7D8B5310E0)


def test_known_answer():
    assert digest.VERSION == 1
    assert int(digest.mix(U64(0))) == 0 and int(digest.mix(U64(1))) == 0x5692161D100B05E5  # splitmix64's finalizer
    d = digest.reference(KAT_HB, KAT_TS, KAT_ST, KAT_TG, KAT_CNT)
    assert [int(x) for x in d["rows"]] == KAT_ROWS
    assert [int(x) for x in d["node_words"]] == KAT_NODES
    assert (d["table"], d["nodes"]) == KAT_SUMS
    assert digest.fold(d["rows"]) == KAT_SUMS[0] and digest.fold(d["node_words"]) == KAT_SUMS[1]
    # the same entries as views (ts = (hb + 1) / 2 there): row 1 of a 3-node PARTIAL state
    hb = np.array([3, 7, 9], dtype=np.int64)
    views = ((np.arange(1, 4, dtype=np.uint64) << U64(32)) | hb.astype(np.uint64))[None, :]
    want = digest.row_words(hb[None, :], (hb[None, :] + 1) // 2)
    assert np.array_equal(digest.view_words(views), want)
    assert np.array_equal(digest.view_words(np.concatenate([views, np.zeros((1, 2), dtype=np.uint64)], axis=1)), want)


# ---- 2. the committed traces
@pytest.mark.parametrize("name", sorted(digest_cases.CASES))
def test_oracle_reproduces_the_traces(name):
    golden = digest_cases.load()
    assert golden["version"] == digest.VERSION and sorted(golden["cases"]) == sorted(digest_cases.CASES)
    got = digest_cases.run(name)
    _, _, first, last = digest_cases.CASES[name]
    assert sorted(map(int, got)) == list(range(first, last + 1))
    assert got == golden["cases"][name]
    assert len({(v["table"], v["nodes"]) for v in got.values()}) == len(got), "two ticks with one digest"


# ---- 3. sensitivity
def _random_state(n, w=None, seed=3, t=40):
    rng = np.random.default_rng(seed)
    w = n if w is None else w
    hb = rng.integers(2 * t - 30, 2 * t, size=(n, w)).astype(np.int32)
    ts = (t - rng.integers(0, 15, size=(n, w))).astype(np.int32)
    absent = rng.random((n, w)) < 0.1
    hb[absent] = ts[absent] = -1
    st = np.stack([np.ones(n), np.ones(n), rng.random(n) < 0.1, np.full(n, 2 * t)], axis=1).astype(np.int32)
    cnt = rng.integers(0, 6, size=n).astype(np.int32)
    tg = rng.integers(0, n, size=(n, 5)).astype(np.int32)
    return hb, ts, st, tg, cnt


def _only_row(a, b, r, rows=True, nodes=False):
    """digests a and b differ in the sums named and in exactly row r's word of those arrays"""
    for on, word, total in ((rows, "rows", "table"), (nodes, "node_words", "nodes")):
        bad = np.flatnonzero(a[word] != b[word])
        assert list(bad) == ([r] if on else []), (word, bad)
        assert (a[total] != b[total]) == on, total
    assert list(digest.diff(a, b)) == [r]


def test_what_must_change_the_digest_does():
    n, r = 40, 17
    hb, ts, st, tg, cnt = _random_state(n)
    hb[r, 3:9], ts[r, 3:9] = [60, 62, 64, -1, 66, 0], [33, 34, 35, -1, 36, 0]  # col 6 absent, col 8 {0, 0}
    cnt[r], tg[r], st[r, 2] = 5, [1, 2, 3, 4, 5], 0
    base = digest.reference(hb, ts, st, tg, cnt)

    def table(edit):
        h, t = hb.copy(), ts.copy()
        edit(h, t)
        return digest.reference(h, t, st, tg, cnt)

    def node(edit):
        s, g, c = st.copy(), tg.copy(), cnt.copy()
        edit(s, g, c)
        return digest.reference(hb, ts, s, g, c)

    def bump_hb(h, t):
        h[r, 3] += 2

    def older_ts(h, t):
        t[r, 3] -= 1

    def moved(h, t):  # the value of column 5 moves to the absent column 6
        h[r, 6], t[r, 6], h[r, 5], t[r, 5] = h[r, 5], t[r, 5], -1, -1

    def swapped(h, t):
        h[r, [3, 4]], t[r, [3, 4]] = h[r, [4, 3]], t[r, [4, 3]]

    def cold_to_absent(h, t):
        h[r, 8] = t[r, 8] = -1

    for edit in (bump_hb, older_ts, moved, swapped, cold_to_absent):
        _only_row(base, table(edit), r)

    def swap_targets(s, g, c):
        g[r, [0, 1]] = g[r, [1, 0]]

    def drop_count(s, g, c):  # count 5 -> 4, the fifth slot left in place
        c[r] = 4

    def flip_failed(s, g, c):
        s[r, 2] ^= 1

    for edit in (swap_targets, drop_count, flip_failed):
        _only_row(base, node(edit), r, rows=False, nodes=True)
    # a slot past the count is not read
    past = node(lambda s, g, c: (c.__setitem__(r, 4), g.__setitem__((r, 4), 33)))
    assert past["nodes"] == node(drop_count)["nodes"]


# ---- 4. shards
def test_column_slices_add_up_and_row_slices_concatenate():
    n = 600
    hb, ts, st, tg, cnt = _random_state(n, seed=5)
    full = digest.reference(hb, ts, st, tg, cnt)
    cuts = [0, 200, 450, n]
    parts = [digest.reference(hb[:, a:b], ts[:, a:b], st, tg, cnt, c0=a) for a, b in zip(cuts, cuts[1:])]
    for (a, b), p in zip(zip(cuts, cuts[1:]), parts):
        own = np.zeros(n, dtype=bool)
        own[a:b] = True
        assert not p["node_words"][~own].any() and np.array_equal(p["node_words"][own], full["node_words"][own])
        assert p["table"] != full["table"]
    merged = digest.merge_columns(parts)
    assert np.array_equal(merged["rows"], full["rows"]) and np.array_equal(merged["node_words"], full["node_words"])
    assert (merged["table"], merged["nodes"]) == (full["table"], full["nodes"])
    assert not len(digest.diff(merged, full))

    rng = np.random.default_rng(9)
    v = 20
    ids = np.sort(np.stack([rng.permutation(n)[:v] + 1 for _ in range(n)]), axis=1).astype(np.uint64)
    views = (ids << U64(32)) | rng.integers(40, 80, size=(n, v)).astype(np.uint64) * U64(2) + U64(1)
    views[rng.random((n, v)) < 0.2] = 0
    whole = digest.reference_views(views, st, tg, cnt)
    pieces = [digest.reference_views(views[a:b], st[a:b], tg[a:b], cnt[a:b], n0=a) for a, b in zip(cuts, cuts[1:])]
    joined = digest.merge_rows(pieces)
    assert np.array_equal(joined["rows"], whole["rows"]) and np.array_equal(joined["node_words"], whole["node_words"])
    assert (joined["table"], joined["nodes"]) == (whole["table"], whole["nodes"])
    other = np.where(np.arange(250) == 4, 5 - cnt[200:450], cnt[200:450])  # node 204: another count
    edited = digest.reference_views(views[200:450], st[200:450], tg[200:450], other, n0=200)
    assert list(digest.diff(pieces[1], edited)) == [204]  # global indices


# ---- 5. a state directory
def test_of_snapshot_over_a_state_directory(tmp_path):
    name = "scaled_n96_cold"
    ora = digest_cases.make_oracle(name)
    while ora.time <= 4:
        ora.tick()
    hb, ts = ora.table()
    st = ora.nodes()
    tg, cnt = ora.targets()
    want = digest.reference(hb, ts, st, tg, cnt)
    assert st[:, :2].all()  # a loadable state: every node started and in the group
    path = os.path.join(tmp_path, "state")
    os.makedirs(path)
    np.save(os.path.join(path, "hb.npy"), hb)
    np.save(os.path.join(path, "ts.npy"), ts)
    np.savez(os.path.join(path, "nodes.npz"), t=np.int32(ora.time), heartbeat=st[:, 3], failed=st[:, 2], targets=tg,
             counts=cnt)
    snap = state.load_dir(path)
    assert isinstance(snap["hb"], np.memmap)
    got = digest.of_snapshot(snap, block_rows=7)
    assert not len(digest.diff(got, want)) and (got["table"], got["nodes"]) == (want["table"], want["nodes"])
    assert got["table"] == int(digest_cases.load()["cases"][name][str(ora.time - 1)]["table"], 16)
    # a column shard's cut of it
    part = digest.of_snapshot(state.slice_columns(snap, (32, 40)), c0=32, block_rows=7)
    assert np.array_equal(part["rows"], digest.row_words(hb[:, 32:72], ts[:, 32:72], 32))
