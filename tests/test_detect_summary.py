"""membership.detect.summarize on hand-made detection records (no GPU), and the recorder's three
entry points in the binding list and the header."""
import os
import re

import numpy as np
import pytest

import membership
from membership import abi
from membership.detect import summarize

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gm_detect_record", "gm_detect", "gm_detect_timeline")


def _records():
    """Five nodes; 0 and 1 crashed after tick 10, so three observers stay alive."""
    rec = np.zeros(5, dtype=abi.DETECT_DTYPE)
    rec["fail_tick"] = rec["first_removed"] = rec["last_removed"] = -1
    # node 0: removed by all three live observers, at ticks 30, 31, 32
    rec[0] = (10, 30, 32, 3, 0, 0, 30 + 31 + 32)
    # node 1: one observer never removed it (ticks 31, 33)
    rec[1] = (10, 31, 33, 2, 0, 0, 31 + 33)
    # node 2: alive, removed by mistake twice (ticks 20, 25) and re-joined
    rec[2] = (-1, 20, 25, 2, 2, 2, 20 + 25)
    return rec, np.array([True, True, False, False, False])


def test_summarize_hand_made_records():
    rec, crashed = _records()
    got = summarize(rec, crashed)
    assert got["completeness"] == 0.5
    assert got["false_removals"] == 2
    # min: first_removed - fail_tick; mean: removed_tick_sum / removals - fail_tick; max: last_removed - fail_tick
    assert got["latency"] == {"min": 20, "mean": (21.0 + 22.0) / 2, "max": 23}
    assert set(got) == {"completeness", "false_removals", "latency"}


def test_summarize_edge_cases():
    rec, crashed = _records()
    none = summarize(rec[2:], crashed[2:])  # nothing crashed: nothing to detect, the mistakes still count
    assert none == {"completeness": 1.0, "false_removals": 2, "latency": {"min": None, "mean": None, "max": None}}
    # a false removal of a node that crashed later does not count towards its detection
    rec[1]["removals"], rec[1]["false_removals"] = 3, 1
    assert summarize(rec, crashed)["completeness"] == 0.5
    with pytest.raises(ValueError):
        summarize(rec, crashed[:4])
    assert membership.summarize is summarize


def test_record_layout_is_the_headers():
    assert abi.DETECT_DTYPE.itemsize == 32
    assert [f[0] for f in abi.GmDetectRec._fields_] == list(abi.DETECT_DTYPE.names)
    text = open(os.path.join(REPO, "include", "gm_abi.h")).read()
    body = re.search(r"typedef struct gm_detect_rec \{(.*?)\} gm_detect_rec;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+);", body) == list(abi.DETECT_DTYPE.names)


def test_entry_points_are_bound_and_declared():
    text = open(os.path.join(REPO, "include", "gm_abi.h")).read()
    for name in NAMES:
        assert name in abi.EXPORTS
        assert re.search(rf"^int {name}\(gm_ctx \*ctx", text, re.M), name
    for m in ("detect_record", "detect", "detect_timeline"):
        assert callable(getattr(abi.Simulator, m))
