"""The reference-side binding compiles against the reference itself.

tests/integration/Application_gm.cpp is the reference's Application.cpp as a maintainer would
rewrite it over gm_abi.h (INTEGRATION.md quotes it). Here it is compiled with g++ against the
reference's OWN headers (Application.h, Params.h, Log.h, Member.h, stdincludes.h under
/root/reference, read in place) together with the reference's unmodified Log.cpp, Params.cpp
and Member.cpp, and linked to the in-tree libgm.so -- so a wrong field name, a missing include or
a signature drift in the documented seam fails here. Skipped where /root/reference is absent (the
GPU box); tests/test_gpu_faithful.py::test_reference_binding runs the binary built by
oracle/Makefile.ref there against the golden dbg.log / msgcount.log / stdout."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
SRC = os.path.join(REPO, "tests", "integration", "Application_gm.cpp")
LIB = os.path.join(REPO, "distributed-membership_amd", "lib")

@pytest.mark.skipif(not os.path.isdir(REF) or not shutil.which("g++"),
                    reason="the reference sources are in the build container only")
def test_binding_compiles_against_reference_headers_and_links_libgm(tmp_path):
    if not os.path.exists(os.path.join(LIB, "libgm.so")):
        pytest.skip("libgm.so not built")
    exe = tmp_path / "Application_gm"
    srcs = [SRC] + [os.path.join(REF, f) for f in ("Log.cpp", "Params.cpp", "Member.cpp")]
    cmd = ["g++", "-std=c++11", "-O0", "-w", f"-I{REF}", f"-I{os.path.join(REPO, 'include')}", "-o", str(exe)] + \
        srcs + [f"-L{LIB}", "-lgm", f"-Wl,-rpath,{LIB}", "-Wl,--no-undefined"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    # the binding calls through the C ABI: its undefined symbols are libgm's entry points
    nm = subprocess.run(["nm", "-u", str(exe)], capture_output=True, text=True, check=True).stdout
    used = {ln.split()[-1] for ln in nm.splitlines() if " gm_" in f" {ln.split()[-1]}"}
    assert {"gm_create", "gm_tick", "gm_drain_events", "gm_rand", "gm_set_failed", "gm_set_dropmsg",
            "gm_msgcount", "gm_destroy", "gm_strerror"} <= used, used
    # and nothing of MP1Node / EmulNet (no longer compiled) is referenced
    assert "MP1Node" not in nm and "EmulNet" not in nm


def test_binding_uses_only_reference_headers():
    """The binding includes the reference's Application.h and gm_abi.h -- no header of this build's
    own app/ (which would hide drift against the reference's classes)."""
    text = open(SRC).read()
    incs = [ln.split()[1] for ln in text.splitlines() if ln.startswith("#include")]
    assert '"Application.h"' in incs and '"gm_abi.h"' in incs
    assert not any("app/" in i for i in incs)
