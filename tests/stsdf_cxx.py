"""Builds tests/cxx/stsdf_example.cpp against libteaser_hip.so (as tsdf_cxx.py builds its example)."""
import os
import subprocess

import pytest

from util import ROOT

SRC = os.path.join(ROOT, "tests", "cxx", "stsdf_example.cpp")
EXE = os.path.join(ROOT, "tests", "cxx", "stsdf_example")
LIBDIR = os.path.join(ROOT, "teaser-plusplus_amd")


def build_stsdf_example():
    """Builds the example (without Eigen, like the other examples); returns the executable."""
    if not os.path.exists(os.path.join(LIBDIR, "libteaser_hip.so")):
        pytest.fail("libteaser_hip.so not built (run __graft_entry__.build())")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), SRC,
                           "-o", EXE, "-L" + LIBDIR, "-lteaser_hip", "-Wl,-rpath," + LIBDIR,
                           "-Wl,-rpath,/opt/rocm/lib"])
    return EXE
