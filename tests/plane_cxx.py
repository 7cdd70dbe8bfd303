"""Builds tests/cxx/plane_example.cpp against libteaser_hip.so (as tests/ransac_cxx.py builds its example), and writes
the problem file it reads."""
import os
import subprocess

from util import ROOT

SRC = os.path.join(ROOT, "tests", "cxx", "plane_example.cpp")
EXE = os.path.join(ROOT, "tests", "cxx", "plane_example")
LIBDIR = os.path.join(ROOT, "teaser-plusplus_amd")


def build_plane_example():
    if not os.path.exists(os.path.join(LIBDIR, "libteaser_hip.so")):
        raise RuntimeError("libteaser_hip.so is not built: run __graft_entry__.build() first")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), SRC,
                           "-o", EXE, "-L" + LIBDIR, "-lteaser_hip", "-Wl,-rpath," + LIBDIR,
                           "-Wl,-rpath,/opt/rocm/lib"])
    return EXE


def write_problem_file(path, P, d, ransac_n, num_iterations, probability, seed):
    with open(path, "w") as f:
        f.write("%d %.17g %d %d %.17g %d\n" % (len(P), d, ransac_n, num_iterations, probability, seed))
        for p in P:
            f.write("%.17g %.17g %.17g\n" % tuple(p))
