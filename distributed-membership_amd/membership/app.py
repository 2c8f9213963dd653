"""Reference-shaped driver in Python (Application.cpp:27-202, Params.cpp, Log.cpp).

`Application(conf).run()` produces the same dbg.log / msgcount.log / stdout
bytes as the C++ ./Application and as the reference, in memory.
"""
import struct

from .abi import (GM_EV_JOINED, GM_EV_REMOVED, GM_EV_START_GROUP, GM_EV_TIME_MARK, GM_EV_TRY_JOIN,
                  GM_MODE_FAITHFUL, Batch, Simulator)

TOTAL_RUNNING_TIME = 700  # Application.h:27


class Params:
    """Params::setparams (Params.cpp:19-40): MAX_NNB, SINGLE_FAILURE, DROP_MSG, MSG_DROP_PROB."""

    def __init__(self, MAX_NNB=10, SINGLE_FAILURE=1, DROP_MSG=0, MSG_DROP_PROB=0.1):
        self.MAX_NNB = self.EN_GPSZ = MAX_NNB
        self.SINGLE_FAILURE, self.DROP_MSG, self.MSG_DROP_PROB = SINGLE_FAILURE, DROP_MSG, MSG_DROP_PROB
        self.STEP_RATE = 0.25
        self.MAX_MSG_SIZE = 4000

    @classmethod
    def from_conf_text(cls, text):
        vals = {}
        for line in text.splitlines():
            if ":" in line:
                k, v = line.split(":", 1)
                vals[k.strip()] = v.strip()
        return cls(int(vals["MAX_NNB"]), int(vals["SINGLE_FAILURE"]), int(vals["DROP_MSG"]),
                   float(vals["MSG_DROP_PROB"]))

    @classmethod
    def from_conf(cls, path):
        with open(path) as f:
            return cls.from_conf_text(f.read())


def log_addr(i):
    """%d.%d.%d.%d:%d over the signed-char address bytes (Log.cpp:73)."""
    b = struct.unpack("4b", struct.pack("<i", i))
    return f"{b[0]}.{b[1]}.{b[2]}.{b[3]}:0"


class Log:
    def __init__(self):
        self.parts = []
        self.opened = False
        self.first = False

    def LOG(self, node_id, t, text):
        prefix = ""
        if not self.opened:
            self.opened = True
        else:
            prefix = log_addr(node_id) + " "
        if not self.first:
            self.parts.append("%x\n" % sum(map(ord, "CS425")))
            self.first = True
        self.parts.append(f"\n {prefix}[{t}] {text}")

    def logNodeAdd(self, logger_id, added_id, t):
        self.LOG(logger_id, t, f"Node {log_addr(added_id)} joined at time {t}")

    def logNodeRemove(self, logger_id, removed_id, t):
        self.LOG(logger_id, t, f"Node {log_addr(removed_id)} removed at time {t}")

    def data(self):
        return "".join(self.parts).encode()


def format_msgcount(sent, recv):
    """EmulNet::ENcleanup (EmulNet.cpp:184-220), node 67 special-cased."""
    n, T = sent.shape
    out = []
    for i in range(1, n + 1):
        out.append("node %3d " % i)
        st = rt = 0
        for j in range(T):
            s, r = int(sent[i - 1, j]), int(recv[i - 1, j])
            st += s
            rt += r
            if i != 67:
                out.append(" (%4d, %4d)" % (s, r))
                if j % 10 == 9:
                    out.append("\n         ")
            else:
                out.append("special %4d %4d %4d\n" % (j, s, r))
        out.append("\n")
        out.append("node %3d sent_total %6u  recv_total %6u\n\n" % (i, st, rt))
    return "".join(out).encode()


def log_events(log, events):
    """the tick records of one cluster (gm_drain_events order) as dbg.log lines"""
    for (t, logger, kind, subject) in events:
        nid = logger + 1
        if kind == GM_EV_JOINED:
            log.logNodeAdd(nid, subject, t)
        elif kind == GM_EV_REMOVED:
            log.logNodeRemove(nid, subject, t)
        elif kind == GM_EV_START_GROUP:
            log.LOG(nid, t, "Starting up group...")
        elif kind == GM_EV_TRY_JOIN:
            log.LOG(nid, t, "Trying to join...")
        elif kind == GM_EV_TIME_MARK:
            log.LOG(nid, t, f"@@time={t}")


def introduced_lines(par, t, stdout):
    """mp1Run's stdout lines of tick t (Application.cpp:143-148)"""
    for i in range(par.EN_GPSZ - 1, -1, -1):
        if t == int(par.STEP_RATE * i):
            stdout.append(f"{i}-th introduced node is assigned with the address: {i + 1}:0\n")


def fail_due(par, t):
    """whether Application::fail does anything at tick t: the t = 50 / 100 / 300 schedule"""
    return t == 100 or (par.DROP_MSG and t in (50, 300))


def fail_step(par, sim, log, t):
    """Application::fail at tick t (Application.cpp:172-202) on one cluster; the caller has logged the
    cluster's records up to tick t (the "Node failed" lines follow them in dbg.log)"""
    n = par.EN_GPSZ
    if par.DROP_MSG and t == 50:
        sim.set_dropmsg(1)
    if par.SINGLE_FAILURE and t == 100:
        removed = sim.rand() % n
        log.LOG(removed + 1, t, f"Node failed at time={t}")
        sim.set_failed([removed])
    elif t == 100:
        removed = (sim.rand() % n) // 2
        idx = list(range(removed, removed + n // 2))
        for i in idx:
            log.LOG(i + 1, t, f"Node failed at time = {t}")
        sim.set_failed(idx)
    if par.DROP_MSG and t == 300:
        sim.set_dropmsg(0)


def new_cluster(par, time_seed, rd_seed, device):
    """what Application::Application sets up for one run: the log with its APP lines, the context"""
    log = Log()
    n = par.EN_GPSZ
    for i in range(n):
        log.LOG(i + 1, 0, "APP")  # Application.cpp:66
    sim = Simulator(n, GM_MODE_FAITHFUL, par.SINGLE_FAILURE, par.DROP_MSG, par.MSG_DROP_PROB, time_seed, rd_seed,
                    device=device)
    return log, sim


class Application:
    def __init__(self, params, time_seed=0, rd_seed=0, device=0, ticks=TOTAL_RUNNING_TIME, dump_tables=False):
        self.par = params if isinstance(params, Params) else Params.from_conf(params)
        self.ticks = ticks
        self.stdout = []
        self.dumps = [] if dump_tables else None
        self.log, self.sim = new_cluster(self.par, time_seed, rd_seed, device)
        self.t = 0

    def mp1Run(self):
        self.sim.tick()
        log_events(self.log, self.sim.drain_events())
        introduced_lines(self.par, self.t, self.stdout)

    def fail(self):
        fail_step(self.par, self.sim, self.log, self.t)

    def run(self):
        for self.t in range(self.ticks):
            self.mp1Run()
            self.fail()
            if self.dumps is not None:
                self.dumps.append(self.sim.dump_tables())
        self.t = self.ticks
        sent, recv = self.sim.msgcount(self.ticks)
        self.msgcount = format_msgcount(sent, recv)
        self.dbg = self.log.data()
        self.out = "".join(self.stdout).encode()
        return self


class BatchResult:
    """one member's run of a BatchApplication: dbg, msgcount, out, dumps as Application has them"""

    def __init__(self, par, log, sim, dump):
        self.par, self.log, self.sim = par, log, sim
        self.stdout = []
        self.dumps = [] if dump else None
        self.dbg = self.msgcount = self.out = None


class BatchApplication:
    """R independent Application runs as one batch (abi.Batch): every tick of all of them is one
    launch set. cases: a list of (Params or conf path, time_seed, rd_seed); dump_tables: the indices
    of the members whose tables are dumped after every tick. run() returns one result per member
    with the bytes a solo Application(...).run() of that case produces.

    A member's records stay on the device until the log needs them, so a tick waits for no member:
    they are drained before fail() writes its "Node failed" lines (t = 100, where gm_rand settles the
    member anyway), at the end, and every tick only for the members whose tables are dumped. Records
    carry their tick and come back in the reference's order across ticks."""

    def __init__(self, cases, ticks=TOTAL_RUNNING_TIME, dump_tables=(), device=0):
        self.ticks = ticks
        self.members = []
        dump = set(dump_tables)
        for k, (params, time_seed, rd_seed) in enumerate(cases):
            par = params if isinstance(params, Params) else Params.from_conf(params)
            log, sim = new_cluster(par, time_seed, rd_seed, device)
            self.members.append(BatchResult(par, log, sim, k in dump))
        self.batch = Batch([m.sim for m in self.members])

    def run(self):
        for t in range(self.ticks):
            self.batch.tick()
            for m in self.members:
                introduced_lines(m.par, t, m.stdout)
                if m.dumps is not None or fail_due(m.par, t):
                    log_events(m.log, m.sim.drain_events())
                    fail_step(m.par, m.sim, m.log, t)
                if m.dumps is not None:
                    m.dumps.append(m.sim.dump_tables())
        for m in self.members:
            log_events(m.log, m.sim.drain_events())
            sent, recv = m.sim.msgcount(self.ticks)
            m.msgcount = format_msgcount(sent, recv)
            m.dbg = m.log.data()
            m.out = "".join(m.stdout).encode()
        return self.members

    def close(self):
        self.batch.close()
        for m in self.members:
            m.sim.close()
