"""ctypes binding of include/gm_abi.h (libgm.so)."""
import ctypes
import os

import numpy as np

GM_ABI_VERSION = 2
GM_MODE_FAITHFUL, GM_MODE_SCALED, GM_MODE_PARTIAL = 0, 1, 2
GM_EV_JOINED, GM_EV_REMOVED, GM_EV_START_GROUP, GM_EV_TRY_JOIN, GM_EV_TIME_MARK = 1, 2, 3, 4, 5
GM_OK, GM_ERANGE = 0, -4
GM_EINVAL, GM_ESTATE, GM_EUNSUPPORTED = -1, -5, -6

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def lib_path():
    return os.environ.get("GM_LIBRARY", os.path.join(_PKG, "lib", "libgm.so"))


class GmConfig(ctypes.Structure):
    _fields_ = [("abi_version", ctypes.c_int32), ("mode", ctypes.c_int32), ("n", ctypes.c_int32),
                ("single_failure", ctypes.c_int32), ("drop_msg", ctypes.c_int32), ("drop_prob", ctypes.c_double),
                ("time_seed", ctypes.c_uint32), ("rd_seed", ctypes.c_uint64),
                ("drop_pct", ctypes.c_int32), ("drop_from", ctypes.c_int32), ("drop_to", ctypes.c_int32),
                ("drop_seed", ctypes.c_uint64),
                ("device", ctypes.c_int32), ("shard_rank", ctypes.c_int32), ("shard_count", ctypes.c_int32),
                ("init_mode", ctypes.c_int32), ("init_t0", ctypes.c_int32), ("init_seed", ctypes.c_uint64),
                ("band", ctypes.c_int32), ("view", ctypes.c_int32), ("view_seed", ctypes.c_uint64),
                ("device_share", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class GmEvent(ctypes.Structure):
    _fields_ = [("t", ctypes.c_int32), ("logger", ctypes.c_int32), ("kind", ctypes.c_int32),
                ("subject", ctypes.c_int32)]


class GmDetectRec(ctypes.Structure):
    _fields_ = [("fail_tick", ctypes.c_int32), ("first_removed", ctypes.c_int32), ("last_removed", ctypes.c_int32),
                ("removals", ctypes.c_uint32), ("false_removals", ctypes.c_uint32), ("joins", ctypes.c_uint32),
                ("removed_tick_sum", ctypes.c_uint64)]


# gm_detect_rec as a NumPy structured dtype (32 bytes, the field names of include/gm_abi.h)
DETECT_DTYPE = np.dtype([("fail_tick", "<i4"), ("first_removed", "<i4"), ("last_removed", "<i4"),
                         ("removals", "<u4"), ("false_removals", "<u4"), ("joins", "<u4"),
                         ("removed_tick_sum", "<u8")])
assert DETECT_DTYPE.itemsize == ctypes.sizeof(GmDetectRec) == 32

class GmCensusRec(ctypes.Structure):
    _fields_ = [("hb_min", ctypes.c_int32), ("hb_max", ctypes.c_int32), ("ts_min", ctypes.c_int32),
                ("ts_max", ctypes.c_int32), ("holders", ctypes.c_uint32), ("stale", ctypes.c_uint32),
                ("hb_sum", ctypes.c_uint64), ("ts_sum", ctypes.c_uint64)]


# gm_census_rec as a NumPy structured dtype (40 bytes, the field names of include/gm_abi.h)
GM_CENSUS_LAGS, GM_CENSUS_AGES = 64, 32
CENSUS_DTYPE = np.dtype([("hb_min", "<i4"), ("hb_max", "<i4"), ("ts_min", "<i4"), ("ts_max", "<i4"),
                         ("holders", "<u4"), ("stale", "<u4"), ("hb_sum", "<u8"), ("ts_sum", "<u8")])
assert CENSUS_DTYPE.itemsize == ctypes.sizeof(GmCensusRec) == 40

class GmViewRec(ctypes.Structure):
    _fields_ = [("hb_min", ctypes.c_int32), ("hb_max", ctypes.c_int32), ("holders", ctypes.c_uint32),
                ("stale", ctypes.c_uint32), ("hb_sum", ctypes.c_uint64)]


# gm_view_rec as a NumPy structured dtype (24 bytes, the field names of include/gm_abi.h)
GM_VIEW_AGES, GM_VIEW_SIZES = 32, 33
VIEW_DTYPE = np.dtype([("hb_min", "<i4"), ("hb_max", "<i4"), ("holders", "<u4"), ("stale", "<u4"), ("hb_sum", "<u8")])
assert VIEW_DTYPE.itemsize == ctypes.sizeof(GmViewRec) == 24

# gm_view_reach: levels and sources of one walk, the two directions
GM_VIEW_HOPS, GM_REACH_SOURCES = 64, 64
GM_REACH_OUT, GM_REACH_IN = 0, 1


class GmViewDetectRec(ctypes.Structure):
    _fields_ = [("fail_tick", ctypes.c_int32), ("first_removed", ctypes.c_int32), ("last_removed", ctypes.c_int32),
                ("removals", ctypes.c_uint32), ("false_removals", ctypes.c_uint32), ("last_held", ctypes.c_int32),
                ("late_joins", ctypes.c_uint32), ("reserved", ctypes.c_uint32),
                ("removed_tick_sum", ctypes.c_uint64), ("held_sum", ctypes.c_uint64)]


# gm_view_detect_rec as a NumPy structured dtype (48 bytes, the field names of include/gm_abi.h)
GM_VIEW_DETECT_COLS = 5  # timeline columns: joins, removals, false_removals, held, late_joins
VIEW_DETECT_DTYPE = np.dtype([("fail_tick", "<i4"), ("first_removed", "<i4"), ("last_removed", "<i4"),
                              ("removals", "<u4"), ("false_removals", "<u4"), ("last_held", "<i4"),
                              ("late_joins", "<u4"), ("reserved", "<u4"),
                              ("removed_tick_sum", "<u8"), ("held_sum", "<u8")])
assert VIEW_DETECT_DTYPE.itemsize == ctypes.sizeof(GmViewDetectRec) == 48

_P = ctypes.POINTER
_ctx, _i32, _i64, _u64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64
_f64, _sz = ctypes.c_double, ctypes.c_size_t
_load4 = [_ctx, _P(_i32), _P(_i32), _P(_i32), _P(_i32)]  # a load's commit: heartbeat, failed, targets, counts

# Every entry point of include/gm_abi.h that returns a status: its argument types. A new entry point
# is declared in the header and listed here (tests/test_abi.py compares the two).
SIGNATURES = {
    "gm_parse_conf": [ctypes.c_char_p, _P(GmConfig)],
    "gm_create": [_P(GmConfig), _P(_ctx)],
    "gm_destroy": [_ctx], "gm_tick": [_ctx], "gm_sync": [_ctx],
    "gm_time": [_ctx, _P(_i32)], "gm_rand": [_ctx, _P(_i32)],
    "gm_set_failed": [_ctx, _P(_i32), _i32], "gm_set_dropmsg": [_ctx, _i32],
    "gm_drain_events": [_ctx, _P(GmEvent), _sz, _P(_sz)],
    "gm_event_counts": [_ctx, _P(_u64)], "gm_event_totals": [_ctx, _P(_u64)],
    "gm_keep_events": [_ctx, _i32], "gm_shard_stub": [_ctx, _i32], "gm_read_views": [_ctx, _i32, _i32, _P(_u64)],
    "gm_msgcount": [_ctx, _i32, _P(_i32), _P(_i32)],
    "gm_msgcount_record": [_ctx, _i32],
    "gm_detect_record": [_ctx, _i32], "gm_detect": [_ctx, _P(GmDetectRec)],
    "gm_detect_timeline": [_ctx, _i32, _P(_u64)],
    "gm_read_row": [_ctx, _i32, _i32, _i32, _P(_i32), _P(_i32)],
    "gm_read_table": [_ctx, _i32, _i32, _P(_i32), _P(_i32)],
    "gm_read_nodes": [_ctx, _P(_i32)], "gm_read_targets": [_ctx, _P(_i32), _P(_i32)],
    "gm_dump_tables": [_ctx, ctypes.c_char_p, _sz, _P(_sz)],
    "gm_tick_stats": [_ctx, _P(_i64)], "gm_pool_info": [_ctx, _P(_i64)],
    "gm_set_timing": [_ctx, _i32], "gm_last_kernel_ms": [_ctx, _P(ctypes.c_float)],
    "gm_crash_set": [_i32, _i32, _u64, _P(_i32)],
    "gm_comm_unique_id": [ctypes.c_char_p],
    "gm_comm_init": [_ctx, ctypes.c_char_p, _i32, _i32],
    "gm_comm_info": [_ctx, _P(_i32)],
    "gm_shard_export": [_ctx, _i32, _i32, ctypes.c_void_p, _sz, _P(_sz)],
    "gm_shard_import": [_ctx, _i32, _i32, ctypes.c_void_p, _sz],
    "gm_shard_layout": [_ctx, _P(_i32), _P(_i32)],
    "gm_shard_loopback": [_P(_ctx), _i32, _i32, _i32],
    "gm_partial_loopback_tick": [_P(_ctx), _i32], "gm_shard_loopback_tick": [_P(_ctx), _i32],
    "gm_shard_exchange_bytes": [_ctx, _P(_i64)],
    "gm_shard_merge": [_ctx], "gm_shard_draw": [_ctx, _i32, _i32],
    "gm_shard_accept": [_ctx, _i32, _P(_i32)], "gm_shard_end_tick": [_ctx],
    "gm_load_begin": [_ctx, _i32], "gm_load_rows": [_ctx, _i32, _i32, _P(_i32), _P(_i32)],
    "gm_load_commit": _load4, "gm_load_stats": [_ctx, _P(_f64)],
    "gm_census": [_ctx, _P(GmCensusRec), _P(_u64)],
    "gm_view_census": [_ctx, _P(GmViewRec), _P(_u64), _P(_u64)],
    "gm_view_reach": [_ctx, _P(_i32), _i32, _i32, _i32, _P(_u64), _P(_u64), _P(_i64)],
    "gm_view_reach_loopback": [_P(_ctx), _i32, _P(_i32), _i32, _i32, _i32, _P(_u64), _P(_u64), _P(_i64)],
    "gm_view_detect_record": [_ctx, _i32], "gm_view_detect": [_ctx, _P(GmViewDetectRec)],
    "gm_view_detect_timeline": [_ctx, _i32, _P(_u64)],
    "gm_read_rows": [_ctx, _i32, _i32, _P(_i32), _P(_i32)], "gm_read_rows_stats": [_ctx, _P(_f64)],
    "gm_digest": [_ctx, _P(_u64), _P(_u64), _P(_u64)], "gm_digest_record": [_ctx, _i32],
    "gm_digest_trace": [_ctx, _i32, _P(_u64)],
    "gm_load_views_begin": [_ctx, _i32], "gm_load_views": [_ctx, _i32, _i32, _P(_u64)],
    "gm_load_views_commit": _load4, "gm_load_views_stats": [_ctx, _P(_f64)],
    "gm_batch_create": [_P(_ctx), _i32, _P(_ctx)], "gm_batch_tick": [_ctx], "gm_batch_destroy": [_ctx],
}
EXPORTS = list(SIGNATURES) + ["gm_strerror"]  # the one entry point that returns no status

_lib = None


class GmError(RuntimeError):
    def __init__(self, code, what):
        self.code = code
        super().__init__(f"{what}: {load_library().gm_strerror(code).decode()} ({code})")


def load_library():
    """Load libgm.so (built in-tree by `make` / __graft_entry__.build()); raises if absent."""
    global _lib
    if _lib is not None:
        return _lib
    path = lib_path()
    if not os.path.exists(path):
        raise FileNotFoundError(f"libgm.so not built: {path} (run `make` at the repo root)")
    lib = ctypes.CDLL(path)
    # GM_AB_BUILD=1 (A/B scripts only): an older measurement build may lack newer entry points, which
    # are then left unbound. Otherwise every entry point must be present, whatever library GM_LIBRARY
    # names, so a stale libgm fails here and not at its first call of a missing symbol
    ab_build = os.environ.get("GM_AB_BUILD") == "1"
    for name, args in SIGNATURES.items():
        if ab_build and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = ctypes.c_int
    lib.gm_strerror.argtypes = [ctypes.c_int]
    lib.gm_strerror.restype = ctypes.c_char_p
    _lib = lib
    return lib


def _ptr(a, ct=ctypes.c_int32):
    return a.ctypes.data_as(ctypes.POINTER(ct))


def default_chunk_rows(width):
    """rows per block of a state load or save when none is given: about 64 MiB at 8 * width bytes per row"""
    return max(1, (64 << 20) // (8 * width))


def crash_set(n, count, seed):
    lib = load_library()
    out = np.zeros(max(count, 1), dtype=np.int32)
    rc = lib.gm_crash_set(n, count, seed, _ptr(out))
    if rc:
        raise GmError(rc, "gm_crash_set")
    return out[:count]


class Simulator:
    """One libgm context: the whole cluster's MP1Node/EmulNet state on one GPU (or shard)."""

    def __init__(self, n, mode=GM_MODE_FAITHFUL, single_failure=1, drop_msg=0, drop_prob=0.1, time_seed=0,
                 rd_seed=0, drop_pct=0, drop_from=0, drop_to=0, drop_seed=0, device=0, shard_rank=0, shard_count=1,
                 init_mode=0, init_t0=0, init_seed=0, band=0, view=0, view_seed=0, device_share=0):
        self.lib = load_library()
        cfg = GmConfig()
        cfg.abi_version = GM_ABI_VERSION
        cfg.mode, cfg.n = mode, n
        cfg.single_failure, cfg.drop_msg, cfg.drop_prob = single_failure, drop_msg, drop_prob
        cfg.time_seed, cfg.rd_seed = time_seed & 0xFFFFFFFF, rd_seed
        cfg.drop_pct, cfg.drop_from, cfg.drop_to, cfg.drop_seed = drop_pct, drop_from, drop_to, drop_seed
        cfg.device, cfg.shard_rank, cfg.shard_count = device, shard_rank, shard_count
        cfg.init_mode, cfg.init_t0, cfg.init_seed = init_mode, init_t0, init_seed
        cfg.band = band
        cfg.view, cfg.view_seed = view, view_seed
        cfg.device_share = device_share
        self.cfg = cfg
        self.n = n
        self.mode = mode
        h = ctypes.c_void_p()
        self._call("gm_create", ctypes.byref(cfg), ctypes.byref(h))
        self.h = h

    def _call(self, name, *args):
        rc = getattr(self.lib, name)(*args)
        if rc != GM_OK:
            raise GmError(rc, name)
        return rc

    def close(self):
        if getattr(self, "_batch", None) is not None:
            self._batch.close()  # a member cannot be destroyed (GM_ESTATE): its batch goes first
        if getattr(self, "h", None):
            self.lib.gm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def tick(self):
        self._call("gm_tick", self.h)

    def sync(self):
        self._call("gm_sync", self.h)

    @property
    def time(self):
        t = ctypes.c_int32()
        self._call("gm_time", self.h, ctypes.byref(t))
        return t.value

    def rand(self):
        v = ctypes.c_int32()
        self._call("gm_rand", self.h, ctypes.byref(v))
        return v.value

    def set_failed(self, idx):
        a = np.ascontiguousarray(np.asarray(idx, dtype=np.int32))
        self._call("gm_set_failed", self.h, _ptr(a), len(a))

    def set_dropmsg(self, on):
        self._call("gm_set_dropmsg", self.h, 1 if on else 0)

    def drain_events(self):
        n = ctypes.c_size_t()
        rc = self.lib.gm_drain_events(self.h, None, 0, ctypes.byref(n))
        if rc == GM_OK:
            return []
        if rc != GM_ERANGE:
            raise GmError(rc, "gm_drain_events")
        buf = (GmEvent * n.value)()
        self._call("gm_drain_events", self.h, buf, n.value, ctypes.byref(n))
        return [(e.t, e.logger, e.kind, e.subject) for e in buf[:n.value]]

    def drain_events_np(self):
        """gm_drain_events into an int32 array [n, 4] of (t, logger, kind, subject)."""
        n = ctypes.c_size_t()
        rc = self.lib.gm_drain_events(self.h, None, 0, ctypes.byref(n))
        if rc == GM_OK:
            return np.zeros((0, 4), dtype=np.int32)
        if rc != GM_ERANGE:
            raise GmError(rc, "gm_drain_events")
        buf = np.empty((n.value, 4), dtype=np.int32)
        self._call("gm_drain_events", self.h, buf.ctypes.data_as(ctypes.POINTER(GmEvent)), n.value, ctypes.byref(n))
        return buf[:n.value]

    def keep_events(self, on):
        self._call("gm_keep_events", self.h, 1 if on else 0)

    def event_total(self):
        c = (ctypes.c_uint64 * 6)()
        self._call("gm_event_counts", self.h, c)
        return int(c[0])

    def event_counts(self):
        """Records of the last tick: [total, joined, removed, ...] (per kind where the mode has it)."""
        c = (ctypes.c_uint64 * 6)()
        self._call("gm_event_counts", self.h, c)
        return [int(x) for x in c]

    def event_totals(self):
        """Records since gm_create: {kind: count} (FAITHFUL, SCALED)."""
        c = (ctypes.c_uint64 * 6)()
        self._call("gm_event_totals", self.h, c)
        return {"total": int(c[0]), "joined": int(c[GM_EV_JOINED]), "removed": int(c[GM_EV_REMOVED])}

    def read_views(self, r0, count):
        """PARTIAL: raw views (id << 32 | hb, 0 = empty) of nodes [r0, r0 + count), uint64 [count, V]."""
        v = self.cfg.view or 32
        out = np.zeros((count, v), dtype=np.uint64)
        self._call("gm_read_views", self.h, r0, count, _ptr(out, ctypes.c_uint64))
        return out

    def msgcount_record(self, tmax):
        """SCALED / PARTIAL: record per-node entry counts for ticks < tmax (before the first tick)"""
        self._call("gm_msgcount_record", self.h, tmax)
        self._mc_tmax = tmax

    def msgcount_recording(self, t):
        return t < getattr(self, "_mc_tmax", 0)

    def msgcount(self, t, rows=None):
        """[rows][t] sent / recv entry messages per node and tick (rows: this context's nodes)"""
        rows = self.n if rows is None else rows
        sent = np.zeros((rows, t), dtype=np.int32)
        recv = np.zeros((rows, t), dtype=np.int32)
        self._call("gm_msgcount", self.h, t, _ptr(sent), _ptr(recv))
        return sent, recv

    def detect_record(self, tmax):
        """FAITHFUL / SCALED: record detection statistics from the next tick on, for ticks < tmax"""
        self._call("gm_detect_record", self.h, tmax)

    def detect(self):
        """One gm_detect_rec per subject this context owns (a SCALED column shard: its columns), as a
        structured array with the fields fail_tick, first_removed, last_removed, removals,
        false_removals, joins, removed_tick_sum."""
        rows = self.shard_layout()[1] if self.mode == GM_MODE_SCALED else self.n
        out = np.zeros(rows, dtype=DETECT_DTYPE)
        self._call("gm_detect", self.h, out.ctypes.data_as(ctypes.POINTER(GmDetectRec)))
        return out

    def detect_timeline(self, t):
        """uint64 [t, 3]: joins, removals, false removals recorded in each tick < t"""
        out = np.zeros((t, 3), dtype=np.uint64)
        self._call("gm_detect_timeline", self.h, t, _ptr(out, ctypes.c_uint64))
        return out

    def census(self, records=True, hist=True):
        """SCALED: the membership census of the state as of the last tick, reduced on the device
        (gm_census). Returns (rec, hist): rec a CENSUS_DTYPE array, one record per subject column of
        this context (holders, stale, hb / ts min, max and sums over the live observers' entries);
        hist uint64 [2, 64, 32], the live observers' cells by (subject's crash flag, heartbeat lag
        clipped to 63, age). The half not asked for is None."""
        rec = np.zeros(self.shard_layout()[1], dtype=CENSUS_DTYPE) if records else None
        h = np.zeros((2, GM_CENSUS_LAGS, GM_CENSUS_AGES), dtype=np.uint64) if hist else None
        self._call("gm_census", self.h, rec.ctypes.data_as(ctypes.POINTER(GmCensusRec)) if records else None,
                   _ptr(h, ctypes.c_uint64) if hist else None)
        return rec, h

    def view_census(self, records=True):
        """PARTIAL: the census of the stored views as of the last tick, reduced on the device
        (gm_view_census). Returns (rec, hist, sizes): rec a VIEW_DTYPE array, one record per subject
        node of the whole cluster (holders, stale, hb min / max / sum over the live observers'
        entries; a row shard counts its own nodes' views), or None with records=False; hist uint64
        [2, GM_VIEW_AGES], the live observers' entries by (subject's crash flag, age); sizes uint64
        [GM_VIEW_SIZES], the live observers by view size."""
        rec = np.zeros(self.n, dtype=VIEW_DTYPE) if records else None
        hist = np.zeros((2, GM_VIEW_AGES), dtype=np.uint64)
        sizes = np.zeros(GM_VIEW_SIZES, dtype=np.uint64)
        self._call("gm_view_census", self.h, rec.ctypes.data_as(ctypes.POINTER(GmViewRec)) if records else None,
                   _ptr(hist, ctypes.c_uint64), _ptr(sizes, ctypes.c_uint64))
        return rec, hist, sizes

    def view_reach(self, sources, direction="out", max_hops=None, seen=False):
        """PARTIAL: breadth-first walks of the view graph as of the last tick, on the device
        (gm_view_reach). On one context holding the whole cluster, or on an RCCL rank (comm_init), where
        the call is a collective every rank makes with the same arguments: counts and the numbers are
        the cluster's, seen covers the rank's own nodes (shard_layout). Row shards of one device:
        partial_loopback_view_reach. The graph: the live nodes, an edge i -> j where the stored view of i names j.
        sources: up to GM_REACH_SOURCES node indices, walked independently; direction "out": the paths
        source -> x (who hears from the source), "in": the paths x -> source (whose gossip reaches it);
        max_hops (default GM_VIEW_HOPS): levels 0 .. max_hops - 1 are walked. Returns a dict: counts
        uint64 [GM_VIEW_HOPS, nsrc], counts[h, k] = live nodes at distance h of source k (a crashed
        source's column is 0); live, the live nodes; hops, the last non-empty level; stopped, True when
        the walk ended because of max_hops; live_sources; seen uint64 [n], bit k set where source k's
        distance is below max_hops, or None when not asked for."""
        rows = self.shard_layout()[1] if self.mode == GM_MODE_PARTIAL else self.n  # an RCCL rank: its own nodes
        return _view_reach(lambda *a: self._call("gm_view_reach", self.h, *a), rows, sources, direction, max_hops, seen)

    def view_detect_record(self, tmax):
        """PARTIAL: record how crashed nodes fade from the views, from the next tick on, for ticks < tmax
        (gm_view_detect_record)"""
        self._call("gm_view_detect_record", self.h, tmax)

    def view_detect(self):
        """PARTIAL: one gm_view_detect_rec per subject node of the whole cluster, as a VIEW_DETECT_DTYPE
        array of n records (fail_tick, first_removed, last_removed, removals, false_removals, last_held,
        late_joins, removed_tick_sum, held_sum). A row shard returns the part its own observers
        recorded (membership.merge_view_detect_shards adds the parts up)."""
        out = np.zeros(self.n, dtype=VIEW_DETECT_DTYPE)
        self._call("gm_view_detect", self.h, out.ctypes.data_as(ctypes.POINTER(GmViewDetectRec)))
        return out

    def view_detect_timeline(self, t):
        """uint64 [t, 5]: joins, removals, false removals, held entries of crashed subjects, late joins
        recorded in each tick < t (a row shard: of its own observers)"""
        out = np.zeros((t, GM_VIEW_DETECT_COLS), dtype=np.uint64)
        self._call("gm_view_detect_timeline", self.h, t, _ptr(out, ctypes.c_uint64))
        return out

    def digest(self, rows=True, nodes=True):
        """SCALED / PARTIAL: the layout-independent digest of the state as of the last tick, computed on
        the device (gm_digest; membership.digest restates the definition in NumPy). Returns a dict of
        table, nodes (ints: the two sums), rows, node_words (uint64 arrays, one word per observer row
        and per node of this context -- n for SCALED, a row shard's own nodes for PARTIAL -- or None
        where not asked for) and r0, the global index of the arrays' first node."""
        part = self.mode == GM_MODE_PARTIAL
        r0, count = self.shard_layout() if part else (0, self.n)
        sums = np.zeros(2, dtype=np.uint64)
        rw = np.zeros(count, dtype=np.uint64) if rows else None
        nw = np.zeros(count, dtype=np.uint64) if nodes else None
        self._call("gm_digest", self.h, _ptr(sums, ctypes.c_uint64), _ptr(rw, ctypes.c_uint64) if rows else None,
                   _ptr(nw, ctypes.c_uint64) if nodes else None)
        return {"table": int(sums[0]), "nodes": int(sums[1]), "rows": rw, "node_words": nw, "r0": r0}

    def digest_record(self, tmax):
        """SCALED (one context) / PARTIAL: record the digest's two sums after every tick < tmax, from the
        next tick on, on the device (gm_digest_record)"""
        self._call("gm_digest_record", self.h, tmax)

    def digest_trace(self, t):
        """uint64 [t, 2]: (table, nodes) as digest() would have returned them right after each tick < t;
        a tick that was not recorded is (0, 0). A row shard records its own nodes: the shards' traces add up."""
        out = np.zeros((t, 2), dtype=np.uint64)
        self._call("gm_digest_trace", self.h, t, _ptr(out, ctypes.c_uint64))
        return out

    def read_row(self, r, c0=0, length=None):
        length = self.n if length is None else length
        hb = np.zeros(length, dtype=np.int32)
        ts = np.zeros(length, dtype=np.int32)
        self._call("gm_read_row", self.h, r, c0, length, _ptr(hb), _ptr(ts))
        return hb, ts

    def read_table(self, r0=0, count=None):
        """(hb, ts) int32 [count][w] of rows [r0, r0 + count) over this context's columns, -1 = absent."""
        count = self.n - r0 if count is None else count
        w = self.shard_layout()[1] if self.mode == GM_MODE_SCALED else self.n
        hb = np.zeros((count, w), dtype=np.int32)
        ts = np.zeros((count, w), dtype=np.int32)
        self._call("gm_read_table", self.h, r0, count, _ptr(hb), _ptr(ts))
        return hb, ts

    def read_rows(self, r0=0, count=None, out=None):
        """SCALED: what read_table returns -- (hb, ts) int32 [count][w] of rows [r0, r0 + count) over this
        context's columns, -1 = absent -- decoded on the device (gm_read_rows): only the rows asked
        for cross to the host. out = (hb, ts): C-contiguous int32 arrays of at least count * w elements
        each to decode into (a caller reading block by block reuses one pair); the returned arrays are
        views of their first count rows."""
        count = self.n - r0 if count is None else count
        w = self.shard_layout()[1] if self.mode == GM_MODE_SCALED else self.n
        if out is None:
            hb = np.zeros((max(count, 0), w), dtype=np.int32)
            ts = np.zeros((max(count, 0), w), dtype=np.int32)
        else:
            hb, ts = out
            for a in (hb, ts):
                if a.dtype != np.int32 or not a.flags["C_CONTIGUOUS"] or a.size < max(count, 0) * w:
                    raise ValueError("read_rows: out arrays must be C-contiguous int32 of at least count * w elements")
        self._call("gm_read_rows", self.h, r0, count, _ptr(hb), _ptr(ts))
        if out is not None:
            hb, ts = (a.reshape(-1)[:count * w].reshape(count, w) for a in (hb, ts))
        return hb, ts

    def _stage_stats(self, name, spans):
        """a staged call's stats (gm_*_stats): rows, the staging block's bytes and the ms in its two timed
        spans, named by `spans` (the times only while set_timing is on)"""
        v = (ctypes.c_double * 4)()
        self._call(name, self.h, v)
        return {"rows": int(v[0]), "staging_bytes": int(v[1]), spans[0]: float(v[2]), spans[1]: float(v[3])}

    def read_rows_stats(self):
        """{"rows", "staging_bytes", "stage_rows", "decode_ms", "copy_ms"} of read_rows since the context
        was created (the times only while set_timing is on); stage_rows: rows per decode launch"""
        st = self._stage_stats("gm_read_rows_stats", ("decode_ms", "copy_ms"))
        return dict(st, stage_rows=st["staging_bytes"] // (8 * self.shard_layout()[1]))

    def read_nodes(self):
        rows = self.shard_layout()[1] if self.mode == GM_MODE_PARTIAL else self.n  # a row shard: its own nodes
        st = np.zeros((rows, 4), dtype=np.int32)
        self._call("gm_read_nodes", self.h, _ptr(st))
        return st

    def read_targets(self):
        """SCALED: (targets int32 [n][5], counts int32 [n]) of the last tick (gm_read_targets).
        PARTIAL: the same for this context's own nodes, [nloc][5] global node indices and [nloc]."""
        rows = self.shard_layout()[1] if self.mode == GM_MODE_PARTIAL else self.n
        tg = np.zeros((rows, 5), dtype=np.int32)
        cnt = np.zeros(rows, dtype=np.int32)
        self._call("gm_read_targets", self.h, _ptr(tg), _ptr(cnt))
        return tg, cnt

    def _load(self, calls, t, row0, tables, chunk_rows, heartbeat, failed, targets, counts):
        """One state load: calls = the begin / rows / commit entry points; tables = the [rows][width]
        arrays of the rows call, this context's rows from the cluster's row0 on, given chunk_rows at a
        time (default: about 64 MiB); the node arrays cover the same rows, failed the whole cluster."""
        rows, width = tables[0].shape
        nodes = [np.ascontiguousarray(a, dtype=np.int32).reshape(shape) for a, shape in
                 ((heartbeat, rows), (failed, self.n), (targets, (rows, 5)), (counts, rows))]
        if chunk_rows is None:
            chunk_rows = default_chunk_rows(width)
        begin, give, commit = calls
        self._call(begin, self.h, int(t))
        for r0 in range(0, rows, chunk_rows):
            m = min(chunk_rows, rows - r0)
            block = [np.ascontiguousarray(a[r0:r0 + m]) for a in tables]  # of a memory-mapped table: read here
            self._call(give, self.h, row0 + r0, m, *[_ptr(a, np.ctypeslib.as_ctypes_type(a.dtype)) for a in block])
        self._call(commit, self.h, *[_ptr(a) for a in nodes])

    def load_state(self, t, hb, ts, heartbeat, failed, targets, counts, chunk_rows=None):
        """SCALED: replace the whole state between two ticks (gm_load_begin / gm_load_rows /
        gm_load_commit; the argument order of the oracle's load_state). hb / ts are int32 [n][w]
        over this context's columns (a shard: its own), -1 = absent, as read_table returns them;
        heartbeat / failed [n]; targets [n][5] and counts [n] as read_targets returns them; t is the
        next tick to run. Rows go to the device in blocks of chunk_rows (default: about 64 MiB)."""
        w = self.shard_layout()[1]
        hb = np.ascontiguousarray(hb, dtype=np.int32).reshape(self.n, w)
        ts = np.ascontiguousarray(ts, dtype=np.int32).reshape(self.n, w)
        self._load(("gm_load_begin", "gm_load_rows", "gm_load_commit"), t, 0, (hb, ts), chunk_rows,
                   heartbeat, failed, targets, counts)

    def load_stats(self):
        """{"rows", "staging_bytes", "check_ms", "encode_ms"} of the last load (kernel times only
        while set_timing is on)"""
        return self._stage_stats("gm_load_stats", ("check_ms", "encode_ms"))

    def load_views(self, t, views, heartbeat, failed, targets, counts, chunk_rows=None):
        """PARTIAL: replace the whole state between two ticks (gm_load_views_begin / gm_load_views /
        gm_load_views_commit). views uint64 [nloc][V] as read_views returns them for this context's
        own nodes; heartbeat [nloc]; failed [n], the crash flags of the WHOLE cluster; targets
        [nloc][5] and counts [nloc] as read_targets returns them; t is the next tick to run. The
        views go to the device in blocks of chunk_rows nodes (default: about 64 MiB)."""
        n0, nloc = self.shard_layout()
        v = self.cfg.view or 32
        vw = np.ascontiguousarray(views, dtype=np.uint64)  # a view of a memory-mapped array: read block by block
        if vw.shape != (nloc, v):
            raise ValueError(f"load_views: views of shape {vw.shape}, this context holds [{nloc}][{v}]")
        self._load(("gm_load_views_begin", "gm_load_views", "gm_load_views_commit"), t, n0, (vw,), chunk_rows,
                   heartbeat, failed, targets, counts)

    def load_views_stats(self):
        """{"rows", "staging_bytes", "check_ms", "store_ms"} of the last view load (kernel times only
        while set_timing is on)"""
        return self._stage_stats("gm_load_views_stats", ("check_ms", "store_ms"))

    def dump_tables(self):
        n = ctypes.c_size_t()
        rc = self.lib.gm_dump_tables(self.h, None, 0, ctypes.byref(n))
        if rc not in (GM_OK, GM_ERANGE):
            raise GmError(rc, "gm_dump_tables")
        buf = ctypes.create_string_buffer(n.value + 1)
        self._call("gm_dump_tables", self.h, buf, n.value + 1, ctypes.byref(n))
        return buf.raw[:n.value]

    def tick_stats(self):
        s = (ctypes.c_int64 * 4)()
        self._call("gm_tick_stats", self.h, s)
        return {"lists": int(s[0]), "live": int(s[1]), "max_inbox": int(s[2]), "err": int(s[3])}

    def pool_info(self):
        """SCALED escape storage as sized at create (gm_pool_info)"""
        v = (ctypes.c_int64 * 4)()
        self._call("gm_pool_info", self.h, v)
        return {"dense": bool(v[0]), "table_pool_entries": int(v[1]), "payload_pool_slots": int(v[2]),
                "event_spill_records": int(v[3])}

    def set_timing(self, on):
        self._call("gm_set_timing", self.h, 1 if on else 0)

    def last_kernel_ms(self):
        v = ctypes.c_float()
        self._call("gm_last_kernel_ms", self.h, ctypes.byref(v))
        return float(v.value)

    # ---- column shards (SCALED multi-GPU; see membership.sharded)
    def comm_init(self, uid, nranks, rank):
        self._call("gm_comm_init", self.h, uid, nranks, rank)

    def comm_info(self):
        """{"ranks", "rank", "rccl_device", "device"} of the attached RCCL communicator (ranks 0: none)"""
        v = (ctypes.c_int32 * 4)()
        self._call("gm_comm_info", self.h, v)
        return {"ranks": v[0], "rank": v[1], "rccl_device": v[2], "device": v[3]}

    def shard_layout(self):
        c0, w = ctypes.c_int32(), ctypes.c_int32()
        self._call("gm_shard_layout", self.h, ctypes.byref(c0), ctypes.byref(w))
        return c0.value, w.value

    def shard_merge(self):
        self._call("gm_shard_merge", self.h)

    def shard_draw(self, rnd, d):
        self._call("gm_shard_draw", self.h, rnd, d)

    def shard_accept(self, d):
        v = ctypes.c_int32()
        self._call("gm_shard_accept", self.h, d, ctypes.byref(v))
        return v.value

    def exchange_bytes(self):
        v = ctypes.c_int64()
        self._call("gm_shard_exchange_bytes", self.h, ctypes.byref(v))
        return v.value

    def shard_stub(self, on):
        """Diagnostics: tick this column shard alone on its device (gm_shard_stub)."""
        self._call("gm_shard_stub", self.h, 1 if on else 0)

    def shard_export(self, what, d=0):
        """the phase exchange buffer `what` of this shard (gm_shard_export) as a flat int32 array"""
        nb = ctypes.c_size_t()
        self._call("gm_shard_export", self.h, what, d, None, 0, ctypes.byref(nb))
        out = np.empty(nb.value // 4, dtype=np.int32)
        self._call("gm_shard_export", self.h, what, d, out.ctypes.data_as(ctypes.c_void_p), nb.value, ctypes.byref(nb))
        return out

    def shard_import(self, what, arr, d=0):
        a = np.ascontiguousarray(arr, dtype=np.int32)
        self._call("gm_shard_import", self.h, what, d, a.ctypes.data_as(ctypes.c_void_p), a.nbytes)

    def shard_end_tick(self):
        self._call("gm_shard_end_tick", self.h)


def _view_reach(call, rows, sources, direction, max_hops, seen):
    """one walk through `call` (the entry point, bound to its contexts), seen over `rows` nodes: the dict
    Simulator.view_reach documents"""
    if direction not in ("out", "in"):
        raise ValueError("view_reach: direction is 'out' or 'in'")
    src = np.ascontiguousarray(np.asarray(sources, dtype=np.int32).reshape(-1))
    counts = np.zeros((GM_VIEW_HOPS, GM_REACH_SOURCES), dtype=np.uint64)
    words = np.zeros(rows, dtype=np.uint64) if seen else None
    info = (ctypes.c_int64 * 4)()
    call(_ptr(src), len(src), GM_REACH_OUT if direction == "out" else GM_REACH_IN,
         GM_VIEW_HOPS if max_hops is None else int(max_hops), _ptr(counts, ctypes.c_uint64),
         _ptr(words, ctypes.c_uint64) if seen else None, info)
    return {"counts": np.ascontiguousarray(counts[:, :len(src)]), "live": int(info[0]), "hops": int(info[1]),
            "stopped": bool(info[2]), "live_sources": int(info[3]), "seen": words}


class Batch:
    """R FAITHFUL Simulators of one device ticked together (gm_batch_*): tick() is one tick() of every
    member in one launch set. Every other call stays the member's own, with its usual meaning, also
    between batch ticks. The batch keeps its members alive; close() gives them back (a member's
    close() closes its batch first)."""

    def __init__(self, sims):
        self.lib = load_library()
        self.sims = list(sims)
        arr = (ctypes.c_void_p * len(self.sims))(*[s.h for s in self.sims])
        h = ctypes.c_void_p()
        rc = self.lib.gm_batch_create(arr, len(self.sims), ctypes.byref(h))
        if rc != GM_OK:
            raise GmError(rc, "gm_batch_create")
        self.h = h
        for s in self.sims:
            s._batch = self

    def tick(self):
        rc = self.lib.gm_batch_tick(self.h)
        if rc != GM_OK:
            raise GmError(rc, "gm_batch_tick")

    def close(self):
        if getattr(self, "h", None):
            self.lib.gm_batch_destroy(self.h)
            self.h = None
            for s in self.sims:
                s._batch = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def comm_unique_id():
    """ncclGetUniqueId (RCCL) as 128 bytes, to broadcast to every rank."""
    buf = ctypes.create_string_buffer(128)
    rc = load_library().gm_comm_unique_id(buf)
    if rc:
        raise GmError(rc, "gm_comm_unique_id")
    return buf.raw


def shard_loopback(sims, what, d=0):
    arr = (ctypes.c_void_p * len(sims))(*[s.h for s in sims])
    rc = load_library().gm_shard_loopback(arr, len(sims), what, d)
    if rc:
        raise GmError(rc, "gm_shard_loopback")


def shard_loopback_tick(sims):
    """One column-shard tick of G contexts on one device in the pipelined tick's chunk order."""
    arr = (ctypes.c_void_p * len(sims))(*[s.h for s in sims])
    rc = load_library().gm_shard_loopback_tick(arr, len(sims))
    if rc:
        raise GmError(rc, "gm_shard_loopback_tick")


def partial_loopback_tick(sims):
    """One PARTIAL tick of G row-shard contexts on one device (exchange by device copies)."""
    arr = (ctypes.c_void_p * len(sims))(*[s.h for s in sims])
    rc = load_library().gm_partial_loopback_tick(arr, len(sims))
    if rc:
        raise GmError(rc, "gm_partial_loopback_tick")


def partial_loopback_view_reach(sims, sources, direction="out", max_hops=None, seen=False):
    """Simulator.view_reach over the G row-shard contexts of one cluster on one device
    (gm_view_reach_loopback, the frontier exchanged by device copies): the same dict, of the whole
    cluster; seen uint64 [n], the shards' parts in node order."""
    arr = (ctypes.c_void_p * len(sims))(*[s.h for s in sims])

    def call(*a):
        rc = load_library().gm_view_reach_loopback(arr, len(sims), *a)
        if rc:
            raise GmError(rc, "gm_view_reach_loopback")

    return _view_reach(call, sims[0].n if sims else 0, sources, direction, max_hops, seen)
