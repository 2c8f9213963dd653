"""The FAITHFUL batch entry points at the C-ABI boundary, without a GPU: gm_batch_create / gm_batch_tick /
gm_batch_destroy are declared in include/gm_abi.h, bound in membership.abi and exported by libgm.so, and
gm_batch_create refuses malformed arguments before it touches a device."""
import ctypes
import os
import re

import pytest

from membership import abi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gm_batch_create", "gm_batch_tick", "gm_batch_destroy")


@pytest.mark.parametrize("name", NAMES)
def test_batch_entry_points_declared_bound_and_exported(name):
    text = open(os.path.join(REPO, "include", "gm_abi.h")).read()
    assert re.search(r"^int\s+" + name + r"\(", text, re.M), "not declared in gm_abi.h"
    assert name in abi.SIGNATURES
    assert hasattr(abi.load_library(), name), "not exported by libgm.so"


def test_batch_handle_is_an_opaque_type():
    text = open(os.path.join(REPO, "include", "gm_abi.h")).read()
    assert "typedef struct gm_batch gm_batch;" in text


def test_batch_create_rejects_bad_arguments_without_a_device():
    lib = abi.load_library()
    one = (ctypes.c_void_p * 1)(None)
    out = ctypes.c_void_p()
    assert lib.gm_batch_create(None, 1, ctypes.byref(out)) == abi.GM_EINVAL  # ctxs NULL
    assert lib.gm_batch_create(one, 1, None) == abi.GM_EINVAL                # out NULL
    assert lib.gm_batch_create(one, 0, ctypes.byref(out)) == abi.GM_EINVAL   # R < 1
    assert lib.gm_batch_create(one, -3, ctypes.byref(out)) == abi.GM_EINVAL
    assert lib.gm_batch_create(one, 65536, ctypes.byref(out)) == abi.GM_EINVAL  # R over the grid's y limit
    assert lib.gm_batch_create(one, 1, ctypes.byref(out)) == abi.GM_EINVAL   # a NULL member
    assert not out.value
    assert lib.gm_batch_tick(None) == abi.GM_EINVAL
    assert lib.gm_batch_destroy(None) == abi.GM_EINVAL
