"""The C++ facade of Fast Global Registration (include/teaser/fgr.h) through the C ABI: tests/cxx/fgr_example.cpp
recovers its planted pose, refuses an empty cloud by name, and on a fixture case -- with and without the tuple test --
returns the record the Python call returns, bit for bit."""
import importlib
import os
import subprocess

import numpy as np
import pytest

from fgr_cxx import build_fgr_example, write_problem_file
from util import ROOT

tp = importlib.import_module("teaser-plusplus_amd")

pytestmark = pytest.mark.gpu
G = np.load(os.path.join(ROOT, "tests", "golden", "fgr_golden.npz"))


def test_cxx_facade_returns_the_python_calls_record(tmp_path):
    exe = build_fgr_example()
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    name = "c256"
    P, Q, corr = G[name + "/P"], G[name + "/Q"], G[name + "/corr"]
    for o in (tp.FastGlobalRegistrationOption(maximum_correspondence_distance=0.3, tuple_test=False),
              tp.FastGlobalRegistrationOption(maximum_correspondence_distance=0.3, tuple_test=True, tuple_scale=0.9,
                                              seed=23)):
        pfile, rfile = str(tmp_path / "problem.txt"), str(tmp_path / "result.txt")
        write_problem_file(pfile, P, Q, corr, o)
        out = subprocess.run([exe, pfile, rfile], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        want = tp.registration_fgr_based_on_correspondence(P, Q, corr, o)
        lines = open(rfile).read().splitlines()
        head = lines[0].split()
        f = want.fgr
        assert [int(v) for v in head[:5]] == [f["iterations"], f["n_corr"], f["failed_solves"], f["flags"],
                                              len(want.correspondence_set)]
        assert (float(head[5]), float(head[6]), float(head[7])) == (want.fitness, want.inlier_rmse, f["final_mu"])
        T = np.array([float(v) for v in lines[1].split()]).reshape(4, 4)
        assert T.tobytes() == want.transformation.tobytes() and f["iterations"] == 64
        pairs = np.array([[int(v) for v in ln.split()] for ln in lines[2:]], dtype=np.int32).reshape(-1, 2)
        assert np.array_equal(pairs, want.correspondence_set) and len(pairs) > 3
        if o.tuple_test:
            assert 10 <= f["n_corr"] < len(corr)
