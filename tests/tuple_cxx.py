"""Builds tests/cxx/tuple_example.cpp against libteaser_hip.so (as knn_cxx.py builds its example)."""
import os
import subprocess

import pytest

from util import ROOT

SRC = os.path.join(ROOT, "tests", "cxx", "tuple_example.cpp")
EXE = os.path.join(ROOT, "tests", "cxx", "tuple_example")
LIBDIR = os.path.join(ROOT, "teaser-plusplus_amd")
EIGEN_STUB = os.path.join(ROOT, "tests", "cxx", "eigen_stub")


def build_tuple_example(eigen=False):
    """Builds the example (with -DTEASER_HIP_USE_EIGEN and the Eigen stub when eigen=True); returns the executable."""
    if not os.path.exists(os.path.join(LIBDIR, "libteaser_hip.so")):
        pytest.skip("libteaser_hip.so not built (run __graft_entry__.build())")
    exe = EXE + ("_eigen" if eigen else "")
    flags = ["-DTEASER_HIP_USE_EIGEN", "-I" + EIGEN_STUB] if eigen else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror"] + flags +
                          ["-I" + os.path.join(ROOT, "include"), SRC, "-o", exe, "-L" + LIBDIR, "-lteaser_hip",
                           "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"])
    return exe
