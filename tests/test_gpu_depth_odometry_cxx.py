"""include/teaser/odometry.h's depth odometry on the MI355X: tests/cxx/depth_odometry_example.cpp computes two pairs of
depth frames given by formulas in one call and one by one, and one pair as float32 metres; the record it prints
(successes, counts, measures and hashes of the matrices' bytes) must be the one the Python calls give on the same arrays.
Without a GPU the program must compile (trackFrameToModel for both volume classes included) and exit with code 77."""
import importlib
import os
import subprocess

import numpy as np
import pytest

from util import ROOT

tp = importlib.import_module("teaser-plusplus_amd")


def build_example():
    libdir = os.path.join(ROOT, "teaser-plusplus_amd")
    exe = os.path.join(ROOT, "tests", "cxx", "depth_odometry_example")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cxx", "depth_odometry_example.cpp"), "-o", exe, "-L" + libdir,
                           "-lteaser_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def fnv(a):
    h = 1469598103934665603
    for b in np.ascontiguousarray(a).tobytes():
        h = ((h ^ b) * 1099511628211) % (1 << 64)
    return "%016x" % h


def frames():
    w, h, padded, out = 48, 36, 52, []
    i, j = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    for k in range(3):
        d = np.full((h, padded), 9, dtype=np.uint16)
        d[:, :w] = 1500 + 3 * i + 2 * (j + k) + (i * i + (j + k) * (j + k)) % 97
        out.append(d[:, :w])
    return out


def line(name, k, r):
    return "%s %d success %d count %d iterations %d converged %d fitness %s rmse %s transformation %s information %s" % (
        name, k, r.success, r.count, r.iterations, r.converged_levels, float(r.fitness).hex(), float(r.inlier_rmse).hex(),
        fnv(r.transformation), fnv(r.information))


def test_the_cxx_header_compiles_and_fails_loudly_without_a_gpu():
    exe = build_example()
    if tp.device_count() == 0:
        assert subprocess.call([exe], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL) == 77


@pytest.mark.gpu
def test_the_cxx_header_gives_the_bits_of_the_python_calls():
    if tp.device_count() < 1:
        pytest.fail("the GPU suite needs an MI355X")
    out = subprocess.run([build_example()], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "checks 1" in out.stdout, out.stdout + out.stderr
    f = frames()
    K = tp.PinholeCameraIntrinsic(48, 36, 40.0, 40.0, 23.5, 17.5)
    opt = tp.DepthOdometryOption([4, 3, 2])
    res = tp.compute_depth_odometry_batch(f[:2], f[1:], K, option=opt)
    want = [line("pair", k, r) for k, r in enumerate(res)]
    m = [a.astype(np.float32) / np.float32(1000.0) for a in f[:2]]
    want.append(line("metres", 0, tp.compute_depth_odometry(m[0], m[1], K, option=opt)))
    got = out.stdout.strip().split("\n")[:3]
    # C's %a and Python's float.hex() spell the same double differently: compare the values
    def parse(s):
        w = s.split()
        return [float.fromhex(x) if x.startswith(("0x", "-0x")) else x for x in w]
    assert [parse(s) for s in got] == [parse(s) for s in want], (out.stdout, want)
    assert res[0].count > 0
