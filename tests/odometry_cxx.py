"""What the odometry tests build once per session: the host driver (tests/odometry_host_driver.cpp, under AddressSanitizer
and UndefinedBehaviorSanitizer, a stand-alone program) and the C++ example (tests/cxx/odometry_example.cpp against the
library)."""
import os
import subprocess
import tempfile

from test_search_host import compile_driver
from util import ROOT

_driver = None


def host_driver():
    """The path of the compiled host driver."""
    global _driver
    if _driver is None:
        import pathlib
        _driver = compile_driver("odometry_host_driver", pathlib.Path(tempfile.mkdtemp(prefix="odometry_driver_")))
    return _driver


def build_odometry_example():
    """Compiles tests/cxx/odometry_example.cpp against include/teaser/odometry.h and the library; returns the program."""
    libdir = os.path.join(ROOT, "teaser-plusplus_amd")
    exe = os.path.join(ROOT, "tests", "cxx", "odometry_example")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cxx", "odometry_example.cpp"), "-o", exe, "-L" + libdir,
                           "-lteaser_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe
