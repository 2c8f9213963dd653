"""PARTIAL states built to sit on the edges of the node tick (gm_partial_node.h p_node): plain NumPy plus the
oracle's op_evict_key, no GPU code. Every builder returns a cluster view snapshot (membership.state
VIEW_KEYS form: t, n0 = 0, views, heartbeat, failed, targets, counts) that satisfies the load contract --
own entry 2(t - 1) - 1, every target in the sender's view, ids ascending, ages below GM_VIEW_AGES -- plus
a key "roles": {name: [node, ...]}, the nodes each case was built on (telemetry for the tests' messages
and the coverage conditions; the loads ignore it).

Ages are "as of tick t", the tick the state runs next: an entry of age A has heartbeat 2(t - A) - 1. A
node's own entry has age 1; a sender's list carries its entries of age <= TFAIL (fresh at t - 1, so an
entry of age TFAIL arrives already stale); the sweep removes at age >= TREMOVE; eviction class = age.
Nodes without a role hold a full view of fresh peers and sent nothing at t - 1."""
import numpy as np

import oracle_py

TFAIL, TREMOVE, FANOUT, VIEW_AGES = 5, 20, 5, 32
DEPTHS = (0, 1, 12, 13, 16, 17, 62, 63)  # around P_KSMALL = 12, P_KP = 16 and the inbox capacity 63


def hb_at(t, age):
    return 2 * (t - age) - 1


class _State:
    def __init__(self, n, v, t, seed):
        if not (2 <= v <= 32 and v <= n and t >= 6 + VIEW_AGES):
            raise ValueError(f"n = {n}, v = {v}, t = {t}: v in 2..32, t >= {6 + VIEW_AGES} (ages up to {VIEW_AGES})")
        self.n, self.v, self.t = n, v, t
        self.rng = np.random.default_rng(seed)
        self.free = [int(x) for x in self.rng.permutation(n)]  # nodes without a role, spread over the cluster
        self.peers = {}    # node -> {peer node: age}
        self.targets = {}  # node -> [node, ...] in draw order
        self.roles = {}

    def take(self, k, role=None):
        if k > len(self.free):
            raise ValueError("the cluster is too small for these cases")
        out, self.free = self.free[:k], self.free[k:]
        if role is not None:
            self.roles.setdefault(role, []).extend(out)
        return out

    def ages(self, k, lo=2, hi=4):
        return [int(a) for a in self.rng.integers(lo, hi + 1, size=k)]

    def set_view(self, i, peers, targets=()):
        assert i not in peers and len(peers) <= self.v - 1 and all(1 <= a <= VIEW_AGES for a in peers.values())
        assert all(d in peers for d in targets) and len(set(targets)) == len(targets) <= FANOUT
        self.peers[i] = dict(peers)
        self.targets[i] = list(targets)

    def others(self, exclude):
        """the nodes outside `exclude`, shuffled"""
        ex = set(exclude)
        return [int(x) for x in self.rng.permutation(self.n) if int(x) not in ex]

    def deliver(self, r, cands, role, senders_min=0, own_max=None):
        """Receiver r (a role of its own) ends the merge of tick t with exactly the candidates `cands`
        ({node: age}) plus one entry of age 1 per sender. Its own view takes the stale candidates (a list
        carries none older than TFAIL) and then others up to own_max (default V - 1) peers; senders outside
        the candidates carry the rest, at most V - 2 each next to themselves and r. Returns the senders."""
        v = self.v
        own_max = v - 1 if own_max is None else own_max
        order = sorted(cands, key=lambda j: (cands[j] <= TFAIL, j))  # stale first
        own, rest = order[:own_max], order[own_max:]
        assert all(cands[j] <= TFAIL for j in rest), "more stale candidates than a view holds"
        k = max(senders_min, -(-len(rest) // max(v - 2, 1)) if rest else 0)
        assert (v > 2 or not rest) and (senders_min == 0 or k == senders_min), "the case counts on its senders"
        senders = []
        for x in self.free:
            if len(senders) == k:
                break
            if x != r and x not in cands:
                senders.append(x)
        assert len(senders) == k, "no free node left for a sender"
        self.free = [x for x in self.free if x not in senders]
        self.roles.setdefault(role + ":senders", []).extend(senders)
        self.set_view(r, {j: cands[j] for j in own})
        for q, s in enumerate(senders):
            carried = rest[q::k]
            self.set_view(s, {**{j: cands[j] for j in carried}, r: self.ages(1)[0]}, [r])
        return senders

    def snapshot(self):
        n, v, t = self.n, self.v, self.t
        views = np.zeros((n, v), dtype=np.uint64)
        targets = np.zeros((n, FANOUT), dtype=np.int32)
        counts = np.zeros(n, dtype=np.int32)
        for i in range(n):
            if i not in self.peers:  # no role: a full view of fresh peers, nothing sent
                peers = [int(x) for x in self.rng.choice(n - 1, size=v - 1, replace=False)]
                self.peers[i] = dict(zip([j + (j >= i) for j in peers], self.ages(v - 1)))
                self.targets[i] = []
            ent = {**{j: hb_at(t, a) for j, a in self.peers[i].items()}, i: hb_at(t, 1)}
            ids = np.array(sorted(ent), dtype=np.uint64)
            hbs = np.array([ent[int(j)] for j in ids], dtype=np.uint64)
            views[i, :len(ids)] = ((ids + np.uint64(1)) << np.uint64(32)) | hbs
            counts[i] = len(self.targets[i])
            targets[i, :counts[i]] = self.targets[i]
        return {"t": t, "n0": 0, "views": views, "heartbeat": np.full(n, 2 * (t - 1), dtype=np.int32),
                "failed": np.zeros(n, dtype=np.int32), "targets": targets, "counts": counts,
                "roles": {k: list(x) for k, x in self.roles.items()}}


def snapshot_ages(snap):
    """int [n][V]: every entry's age as of tick snap["t"], -1 for an empty slot"""
    hb = (snap["views"] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    return np.where(snap["views"] != 0, snap["t"] - (hb + 1) // 2, -1)


# ------------------------------------------------------------------ inbox depth and table load
def deep_inbox(n, v, t, depths=DEPTHS, seed=1):
    """One receiver per entry of `depths` ("depth<d>") with that many lists delivered at tick t. The views
    of a receiver and its senders are disjoint apart from the receiver and the sender itself as far as
    the cluster reaches (32 + 31 d ids at V = 32: 404 / 528 / 1985 at d = 12 / 16 / 63); where it does
    not, the pool wraps and the lists overlap with different heartbeats. Carried entries have ages
    2..TFAIL, so some arrive stale. Up to V = 8 a sender holds the receiver at age TFAIL (drawn at t - 1,
    stale at t): with numpot <= FANOUT + 2 nearly every sender would draw it again at t, and the 63 lists
    of t + 1 plus a few natural ones would overflow the receiver's inbox, which the HIP path refuses
    (GM_ERR_INBOX) and the oracle does not model."""
    st = _State(n, v, t, seed)
    hold = (lambda: TFAIL) if v <= 8 else (lambda: st.ages(1)[0])
    for d in depths:
        (r,) = st.take(1, f"depth{d}")
        senders = st.take(d, f"depth{d}:senders")
        pool = st.others([r] + senders)
        assert len(pool) >= v - 1
        cur = 0

        def draw(k):
            nonlocal cur
            out = [pool[(cur + q) % len(pool)] for q in range(k)]
            cur += k
            return out
        st.set_view(r, dict(zip(draw(v - 1), st.ages(v - 1))))
        for s in senders:
            st.set_view(s, {**dict(zip(draw(v - 2), st.ages(v - 2, 2, TFAIL))), r: hold()}, [r])
    return st.snapshot()


# ------------------------------------------------------------------ eviction
def _key_groups(view_seed, t, r, nodes):
    """{key >> 26: [node, ...]} of the eviction keys observer r gives these nodes at tick t"""
    L = oracle_py.lib()
    groups = {}
    for j in nodes:
        groups.setdefault(int(L.op_evict_key(view_seed, t, r, j + 1)) >> 26, []).append(j)
    return groups


def eviction_cases(n, v, t, view_seed=5, seed=2, deep=True):
    """Receivers whose size after the sweep and whose heartbeat classes (= ages) are chosen; need = V - 1
    candidates are kept next to the node itself, every sender is a candidate of age 1:
      fit          size V: no eviction             over1        size V + 1
      first_part   V + 8 senders: the cut falls in the first class, in part
      first_whole  V - 1 senders: the first class is exactly what is needed
      class_whole  the cut class (age 3) is taken whole, an older class is left
      group_whole  the cut class in part, its cut key group (key >> 26) whole, a later group left
      group_part   the cut class is one key group, as large as the cluster gives (40 of ~64 ids at
                   n = 4096), taken in part: the exact min-selection runs needc rounds
      late         the cut falls in age TFAIL, after four fresher classes
      stale        the cut falls in age TREMOVE - 1, the oldest class there is
      big_part / huge_part (deep)  group_part with 14 / 20 senders: the big and the huge table"""
    st = _State(n, v, t, seed)
    need = v - 1

    def receiver(role):
        (r,) = st.take(1, role)
        return r, st.others([r])

    def spread(pool, sizes_ages):
        out, cur = {}, 0
        for k, a in sizes_ages:
            out.update({j: a for j in pool[cur:cur + k]})
            cur += k
        return out

    r, pool = receiver("fit")
    st.deliver(r, dict(zip(pool[:v - 2], st.ages(v - 2))), "fit", senders_min=1, own_max=max(v - 4, 0))
    r, pool = receiver("over1")
    st.deliver(r, dict(zip(pool[:v - 1], st.ages(v - 1))), "over1", senders_min=1)
    r, pool = receiver("first_part")
    st.deliver(r, dict(zip(pool[:v - 1], st.ages(v - 1))), "first_part", senders_min=v + 8)
    r, pool = receiver("first_whole")
    st.deliver(r, dict(zip(pool[:v - 1], st.ages(v - 1))), "first_whole", senders_min=v - 1)
    if v >= 12:
        a2 = (v - 2) // 3
        r, pool = receiver("class_whole")
        st.deliver(r, spread(pool, [(a2, 2), (need - 1 - a2, 3), (8, 4)]), "class_whole", senders_min=1)

        # the cut class (age 3) over chosen key groups; one sender, so 1 + a2 candidates are fresher
        def grouped(role, a2, senders):
            r, pool = receiver(role)
            groups = _key_groups(view_seed, t, r, pool)
            g = max(groups, key=lambda x: (16 <= x < 48, len(groups[x])))  # the fullest group of the middle
            return r, groups, g, need - senders - a2

        r, groups, g, needb = grouped("group_whole", a2, 1)
        y = max(1, min(len(groups[g]), needb - 1))
        below = [j for x in sorted(groups) if x < g for j in groups[x]][:needb - y]
        above = [j for x in sorted(groups) if x > g for j in groups[x]][:6]
        assert len(below) == needb - y and above
        cut = below + groups[g][:y] + above
        rest = [j for j in pool if j not in set(cut)]
        st.deliver(r, {**spread(rest, [(a2, 2)]), **{j: 3 for j in cut}}, "group_whole", senders_min=1)

        cases = [("group_part", 1)] + ([("big_part", 14), ("huge_part", 20)] if deep and v >= 26 else [])
        for role, senders in cases:
            r, groups, g, _ = grouped(role, 0, senders)
            cut = groups[g][:40]
            needb = min(len(cut) // 2, need - senders)  # 20 of 40 where the cluster gives them
            a2s = need - senders - needb
            assert len(cut) > needb >= 1, f"{role}: the fullest key group holds {len(cut)} ids"
            rest = [j for j in pool if j not in set(cut)]
            st.deliver(r, {**spread(rest, [(a2s, 2)]), **{j: 3 for j in cut}}, role, senders_min=senders,
                       own_max=None if senders == 1 else 4)
        r, pool = receiver("late")
        st.deliver(r, spread(pool, [(2, 2), (2, 3), (2, 4), (v, TFAIL)]), "late", senders_min=1)
        r, pool = receiver("stale")
        st.deliver(r, spread(pool, [(2, 2), (4, 3), (2, 7), (2, 12), (v - 7, TREMOVE - 1)]), "stale", senders_min=1)
    return st.snapshot()


# ------------------------------------------------------------------ sweep
def sweep_cases(n, v, t, seed=3):
    """age4 / age5 / age19 / age20  one peer at TFAIL - 1, TFAIL, TREMOVE - 1, TREMOVE, the others fresh
    all_gone      all V - 1 peers expire (ages 20..32) while two lists bring V new ids: V - 1 REMOVE and
                  V - 1 JOINED events in the 2V-slot event row, and an eviction of one
    all_gone_fit  the same with one list of V - 1 new ids: size V, no eviction
    refresh       peers of age TREMOVE - 1 and TREMOVE that a list refreshes (nothing removed), next to
                  a carried entry of age TFAIL (stale on arrival)
    starved       removals that make numpot <= 0 although fresh peers remain: `removed` counts into
                  numfailed (the reference's quirk, MP1Node.cpp:426-447), so nothing is sent"""
    st = _State(n, v, t, seed)
    for a in (TFAIL - 1, TFAIL, TREMOVE - 1, TREMOVE):
        (r,) = st.take(1, f"age{a}")
        pool = st.others([r])
        st.set_view(r, dict(zip(pool[:v - 1], [a] + st.ages(v - 2, 2, 3))))
    old = [TREMOVE, TREMOVE + 1, TREMOVE + 5, VIEW_AGES]
    for role, extra in (("all_gone", 1), ("all_gone_fit", 0)):
        (r,) = st.take(1, role)
        pool = st.others([r])
        gone, new = pool[:v - 1], pool[v - 1:]
        senders = []
        for x in st.free:  # senders outside the expiring peers
            if len(senders) < 1 + extra and x != r and x not in gone:
                senders.append(x)
        st.free = [x for x in st.free if x not in senders]
        st.roles[role + ":senders"] = senders
        new = [j for j in new if j not in senders][:v - 2]
        st.set_view(r, {j: old[q % len(old)] for q, j in enumerate(gone)})
        st.set_view(senders[0], {**dict(zip(new, st.ages(v - 2))), r: 2}, [r])
        if extra:
            st.set_view(senders[1], {r: 3}, [r])
    if v >= 4:
        (r,) = st.take(1, "refresh")
        (s,) = st.take(1, "refresh:senders")
        pool = st.others([r, s])
        x, y, z, w = pool[:4]
        st.set_view(r, {**dict(zip(pool[4:4 + v - 3], st.ages(v - 3))), x: TREMOVE - 1, y: TREMOVE})
        carried = {r: 2, x: 3, y: 4, z: TFAIL, w: TFAIL + 1}
        st.set_view(s, dict(list(carried.items())[:v - 1]), [r])
    (r,) = st.take(1, "starved")
    pool = st.others([r])
    nrem = -(-(v - 1) * 2 // 3)
    fresh = v - 1 - nrem
    st.set_view(r, dict(zip(pool[:v - 1], [old[q % 3] for q in range(nrem)] + st.ages(fresh))))
    return st.snapshot()


# ------------------------------------------------------------------ gossip draw
def draw_cases(n, v, t, seed=4, replicas=6):
    """fresh<f>  full views with f fresh peers (numpot = f: 0..5 and 8) and the others stale, ages
                 TFAIL..TREMOVE - 1: few draws are accepted, so the draw runs past the 16 precomputed S2
                 outputs into the lazy generator's first and later batches; `replicas` nodes each
    size2 / size3  views of 2 and 3 fresh entries: the node itself and repeats dominate the draws"""
    st = _State(n, v, t, seed)
    for f in (0, 1, 2, 3, 4, 5, 8):
        if f > v - 1 or (f == v - 1 and f > 0):
            continue
        for r in st.take(replicas, f"fresh{f}"):
            pool = st.others([r])
            st.set_view(r, dict(zip(pool[:v - 1], st.ages(f) + st.ages(v - 1 - f, TFAIL, TREMOVE - 1))))
    for size in (2, 3):
        if size > v:
            continue
        for r in st.take(replicas, f"size{size}"):
            pool = st.others([r])
            st.set_view(r, dict(zip(pool[:size - 1], st.ages(size - 1))))
    return st.snapshot()
