"""Builds tests/cxx/fgr_example.cpp against libteaser_hip.so (as tests/ransac_cxx.py builds its example), and writes
the problem file it reads."""
import os
import subprocess

from util import ROOT

SRC = os.path.join(ROOT, "tests", "cxx", "fgr_example.cpp")
EXE = os.path.join(ROOT, "tests", "cxx", "fgr_example")
LIBDIR = os.path.join(ROOT, "teaser-plusplus_amd")


def build_fgr_example():
    if not os.path.exists(os.path.join(LIBDIR, "libteaser_hip.so")):
        raise RuntimeError("libteaser_hip.so is not built: run __graft_entry__.build() first")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), SRC,
                           "-o", EXE, "-L" + LIBDIR, "-lteaser_hip", "-Wl,-rpath," + LIBDIR,
                           "-Wl,-rpath,/opt/rocm/lib"])
    return EXE


def write_problem_file(path, P, Q, corr, option):
    with open(path, "w") as f:
        f.write("%d %d %d %.17g %d %d %.17g %d %.17g %d %d\n" % (
            len(P), len(Q), len(corr), option.division_factor, option.use_absolute_scale, option.decrease_mu,
            option.maximum_correspondence_distance, option.iteration_number, option.tuple_scale, option.tuple_test,
            option.seed))
        for cloud in (P, Q):
            for p in cloud:
                f.write("%.17g %.17g %.17g\n" % tuple(p))
        for i, j in corr:
            f.write("%d %d\n" % (i, j))
