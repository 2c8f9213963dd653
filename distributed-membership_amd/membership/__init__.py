"""Python host surface of the MI355X gossip-membership simulator.

Mirrors the reference's driver interface (Application / Params / Log,
Application.cpp:27-202, Params.cpp:19-40, Log.cpp:44-131) over the C ABI of
include/gm_abi.h (libgm.so: hand-written HIP kernels for gfx950). There is no
CPU fallback: constructing a Simulator without the built library, or without a
GPU, raises.
"""
from .abi import (GM_EV_JOINED, GM_EV_REMOVED, GM_EV_START_GROUP, GM_EV_TIME_MARK, GM_EV_TRY_JOIN,  # noqa: F401
                  GM_MODE_FAITHFUL, GM_MODE_PARTIAL, GM_MODE_SCALED, Batch, GmError, Simulator, crash_set, lib_path,
                  load_library)
from .app import Application, BatchApplication, Params, format_msgcount, log_addr  # noqa: F401
from .detect import merge_view_detect_shards, summarize, summarize_view_detect  # noqa: F401
from .census import merge_shards, summarize_census  # noqa: F401
from .views import merge_view_shards, summarize_views  # noqa: F401
from .reach import summarize_reach  # noqa: F401
from . import digest, state  # noqa: F401
