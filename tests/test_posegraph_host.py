"""The host side of pose-graph optimisation without a GPU: csrc/posegraph.hip compiled by g++ against the HIP stand-in
header with a stand-in for the launcher (tests/posegraph_host_driver.cpp), under AddressSanitizer and
UndefinedBehaviorSanitizer, as a stand-alone program.  Every refusal and its message, the buffer sizes, the CSR and the
pair lists against brute force (duplicate and reversed pairs included), the unpacking, and that a refusal leaves the
outputs untouched.  Then the Python surface: names, argument validation, NotImplementedError for other methods and the
in-place semantics of global_optimization on a stubbed result."""
import importlib
import os
import subprocess

import numpy as np
import pytest

from util import ROOT

tp = importlib.import_module("teaser-plusplus_amd")


def test_posegraph_entry_checks_indexes_sizes_and_unpacks(tmp_path):
    exe = str(tmp_path / "posegraph_host_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-ffp-contract=off", "-x", "c++", "-I" + os.path.join(ROOT, "tests", "hip_stub"),
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "teaser-plusplus_amd", "csrc"),
                           os.path.join(ROOT, "tests", "posegraph_host_driver.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "mismatches 0" in out.stdout, out.stdout + out.stderr[-4000:]


def test_python_surface_names_and_structs():
    names = ["PoseGraph", "PoseGraphNode", "PoseGraphEdge", "GlobalOptimizationOption",
             "GlobalOptimizationConvergenceCriteria", "GlobalOptimizationLevenbergMarquardt", "global_optimization",
             "global_optimization_batch", "linearize_pose_graph"]
    for name in names:
        assert name in tp.__all__ and hasattr(tp, name), name
    o = tp.posegraph.PoseGraphOptionC()
    assert tp.lib().teaser_hip_posegraph_option_default(o) == 0
    import posegraph_reference as G
    assert {k: getattr(o, k) for k in G.DEFAULTS} == G.DEFAULTS
    crit, opt = tp.GlobalOptimizationConvergenceCriteria(), tp.GlobalOptimizationOption()
    c = tp.posegraph._option_c(crit, opt)
    assert {k: getattr(c, k) for k in G.DEFAULTS} == G.DEFAULTS
    assert [getattr(tp.posegraph, n) for n in tp.posegraph.STATUS_NAMES] == list(range(7))
    e = tp.PoseGraphEdge()
    assert e.source_node_id == -1 and e.confidence == 1.0 and not e.uncertain and np.array_equal(e.information, np.eye(6))


def test_python_argument_validation():
    pg = tp.PoseGraph([tp.PoseGraphNode(), tp.PoseGraphNode()], [tp.PoseGraphEdge(1, 0)])
    with pytest.raises(NotImplementedError, match="GaussNewton"):
        tp.global_optimization(pg, tp.GlobalOptimizationGaussNewton())
    with pytest.raises(NotImplementedError):
        tp.global_optimization_batch([pg], object())
    with pytest.raises(TypeError, match="criteria"):
        tp.global_optimization_batch([pg], None, tp.GlobalOptimizationOption())
    with pytest.raises(TypeError, match="option"):
        tp.global_optimization_batch([pg], None, None, 3)
    with pytest.raises(TypeError, match="pose graph 0"):
        tp.global_optimization_batch([[1, 2]])
    with pytest.raises(ValueError, match="2 values for 1 pose graphs"):
        tp.global_optimization_batch([pg], None, [None, None])
    with pytest.raises(ValueError, match="trace"):
        tp.global_optimization_batch([pg], trace=-1)
    pg.nodes[1].pose = np.eye(3)
    with pytest.raises(ValueError, match="pose of node 1 must be 4 x 4"):
        tp.global_optimization_batch([pg])
    pg.nodes[1].pose = np.eye(4)
    pg.edges[0].information = np.eye(5)
    with pytest.raises(ValueError, match="information of edge 0 must be 6 x 6"):
        tp.global_optimization_batch([pg])
    assert tp.global_optimization_batch([]) == []  # no graphs: no device needed


def test_global_optimization_applies_a_result_in_place(monkeypatch):
    nodes = [tp.PoseGraphNode(np.eye(4)) for _ in range(3)]
    edges = [tp.PoseGraphEdge(1, 0), tp.PoseGraphEdge(2, 1), tp.PoseGraphEdge(2, 0, uncertain=True)]
    pg = tp.PoseGraph(nodes, edges)
    rec = tp.posegraph.PoseGraphResultC()
    rec.status, rec.F0, rec.F = tp.posegraph.RESIDUAL, 2.0, 1.0
    poses = np.stack([np.eye(4) * (i + 1) for i in range(3)])
    stub = tp.posegraph.PoseGraphOptimizationResult(poses, np.array([1.0, 1.0, 0.1]), np.array([False, False, True]), rec, [])
    seen = {}

    def fake(pose_graphs, method, criteria, option, device=-1, trace=0):
        seen["args"] = (pose_graphs, method, criteria, option, device)
        return [stub]

    monkeypatch.setattr(tp.posegraph, "global_optimization_batch", fake)
    method, crit, opt = tp.GlobalOptimizationLevenbergMarquardt(), tp.GlobalOptimizationConvergenceCriteria(), tp.GlobalOptimizationOption()
    res = tp.global_optimization(pg, method, crit, opt)
    assert res is stub and seen["args"] == ([pg], method, crit, opt, -1) and res.status_name == "RESIDUAL"
    assert all(a is b for a, b in zip(pg.nodes, nodes)) and len(pg.nodes) == 3 and all(np.array_equal(n.pose, T) for n, T in zip(nodes, poses))
    assert pg.edges == edges[:2] and [e.confidence for e in edges] == [1.0, 1.0, 0.1]
