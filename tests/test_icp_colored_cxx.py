"""The C++ facade of Colored ICP (include/teaser/icp.h: TransformationEstimationForColoredICP, registrationColoredICP,
ICP::estimateColorGradients) through tests/cxx/colored_icp_example.cpp: it compiles with -Wall -Werror, fails loudly
without a device, and on the textured scene gives the bits of the Python call."""
import importlib
import subprocess

import numpy as np
import pytest

from icp_colored_cases import scene
from icp_colored_cxx import build_colored_icp_example

tp = importlib.import_module("teaser-plusplus_amd")


def test_cxx_colored_icp_example_exits_77_without_device():
    exe = build_colored_icp_example()
    rc = subprocess.call([exe], stdout=subprocess.DEVNULL, timeout=120)
    assert rc == (0 if tp.device_count() > 0 else 77)


@pytest.mark.gpu
def test_cxx_facade_gives_the_python_calls_bits_on_the_scene(tmp_path):
    exe = build_colored_icp_example()
    s = scene()
    for name, key in (("src", "source"), ("dst", "target"), ("src_colors", "source_colors"),
                      ("dst_colors", "target_colors"), ("dst_normals", "target_normals")):
        np.ascontiguousarray(s[key], dtype=np.float64).tofile(str(tmp_path / (name + ".bin")))
    out = subprocess.run([exe, str(tmp_path), repr(s["r"]), "50"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = dict(line.split(" ", 1) for line in out.stdout.strip().splitlines())
    py = tp.registration_colored_icp(s["source"], s["target"], s["r"], criteria=tp.ICPConvergenceCriteria(max_iteration=50),
                                     source_colors=s["source_colors"], target_colors=s["target_colors"],
                                     target_normals=s["target_normals"])
    T = np.array([float(x) for x in lines["T"].split()]).reshape(4, 4)
    assert T.tobytes() == py.transformation.tobytes()
    assert float(lines["fitness"]) == py.fitness and float(lines["rmse"]) == py.inlier_rmse
    assert int(lines["iterations"]) == py.iterations >= 2
    assert int(lines["correspondences"]) == len(py.correspondence_set)
    g = tp.estimate_color_gradients(s["target"], s["target_normals"], s["target_colors"], 2 * s["r"])
    assert np.array([float(x) for x in lines["gradients"].split()]).tobytes() == g[:3].tobytes()
