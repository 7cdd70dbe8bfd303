"""Pose-graph optimisation on the GPU against the numpy restatement (tests/posegraph_reference.py) on the scenarios of
tests/posegraph_cases.py: the decisions (status, iterations, trials, accept / factorise flags, pruned set) EQUAL the
restatement's; the numbers are compared with the longdouble restatement under the rule of posegraph_cases.tolerance
(16 x the restatement's own float64-against-longdouble noise), and the measured ratio is printed per quantity and case.
Then the batch: every output bit-identical to the same graph alone, in two orders, and run to run."""
import importlib

import numpy as np
import pytest

import posegraph_cases as PC
import posegraph_reference as G

tp = importlib.import_module("teaser-plusplus_amd")

pytestmark = pytest.mark.gpu
TRACE = 64  # rows of room per graph: more than any scenario's trials


def pose_graph(name):
    p = PC.packed(name)
    nodes = [tp.PoseGraphNode(T) for T in p["poses"]]
    edges = [tp.PoseGraphEdge(int(s), int(t), X, L, bool(u)) for s, t, X, L, u in
             zip(p["source"], p["target"], p["transformation"], p["information"], p["uncertain"])]
    return tp.PoseGraph(nodes, edges)


def objects(opt):
    crit = tp.GlobalOptimizationConvergenceCriteria(**{k: opt[k] for k in (
        "max_iteration", "max_iteration_lm", "min_relative_increment", "min_relative_residual_increment",
        "min_right_term", "min_residual", "upper_scale_factor", "lower_scale_factor")})
    option = tp.GlobalOptimizationOption(**{k: opt[k] for k in (
        "max_correspondence_distance", "edge_prune_threshold", "preference_loop_closure", "reference_node")})
    return crit, option


def as_got(res):
    flags, lam = [[], []], [[], []]
    for row in res.trace:
        flags[row["pass"]].append((row["accepted"], row["factorised"]))
        lam[row["pass"]].append(row["lam"])
    return dict(status=res.status, iterations=res.iterations, trials=res.trials, flags=flags, lam=lam, pruned=res.pruned,
                poses=res.poses, confidence=res.confidence, F0=res.F0, F=res.F, mu=res.mu)


_alone = {}


def alone(name):
    """The graph optimised in a call of its own, once per process."""
    if name not in _alone:
        crit, option = objects(PC.build(name)[2])
        _alone[name] = tp.global_optimization_batch([pose_graph(name)], tp.GlobalOptimizationLevenbergMarquardt(),
                                                    crit, option, trace=TRACE)[0]
    return _alone[name]


def bits(res):
    """Everything a call returns for one graph, as bytes."""
    rows = [(r["pass"], r["lam"], r["rho"], r["F_new"], r["accepted"], r["factorised"]) for r in res.trace]
    return (res.poses.tobytes(), res.confidence.tobytes(), res.pruned.tobytes(),
            np.array([res.F0, res.F] + res.mu).tobytes(), tuple(res.iterations), tuple(res.trials), res.status,
            res.n_trace, np.array(rows, dtype=np.float64).tobytes())


@pytest.mark.parametrize("name", list(PC.CASES))
def test_optimize_takes_the_restatements_decisions_and_agrees_within_its_noise(name):
    assert PC.WIDE
    res = alone(name)
    assert res.n_trace == len(res.trace) <= TRACE
    PC.check_against_reference(name, as_got(res))
    start, edges, _ = PC.build(name)
    if name == "multi_edge":
        assert np.array_equal(res.poses[5], start[5])  # the node without an edge
    if name == "negative_information":
        assert np.array_equal(res.poses, start)
    if name in PC.TRIVIAL:
        assert np.array_equal(res.poses, start) and res.status == tp.posegraph.TRIVIAL


@pytest.mark.parametrize("name", PC.LINEARIZE_CASES)
def test_linearize_agrees_with_the_restatement(name):
    assert PC.WIDE
    start, edges, opt = PC.build(name)
    got = tp.linearize_pose_graph(pose_graph(name), objects(opt)[1])
    l64, lld = G.linearize(start, edges, opt, np.float64), G.linearize(start, edges, opt, np.longdouble)
    ratios = {k: PC.ratio(got[k], l64[k], lld[k]) for k in ("e", "r", "l", "mu", "F", "H", "g")}
    print("posegraph linearize %-12s ratio to the restatement's noise: " % name +
          " ".join("%s %.3g" % kv for kv in ratios.items()))
    assert max(ratios.values()) <= 16.0, ratios
    H = got["H"]
    assert np.array_equal(H, H.T)
    ref = max(opt["reference_node"], 0)
    assert not H[6 * ref:6 * ref + 6].any() and not H[:, 6 * ref:6 * ref + 6].any() and not got["g"][6 * ref:6 * ref + 6].any()


def test_batch_of_zero_graphs_is_valid():
    assert tp.global_optimization_batch([]) == []
    L = tp.lib()
    h, lock = tp.posegraph._cache.get(-1)
    with lock:
        assert L.teaser_hip_posegraph_optimize_batch(h, 0, None, None, None, None, None, None, None, None, None, None,
                                                     None, None, None, None, None) == 0


def test_a_mixed_batch_gives_each_graph_the_bits_it_gets_alone():
    names = ["n2_m1", "consistent", "gross_chord", "far_start", "size_128", "negative_information",
             "trivial_one_node", "trivial_no_edge"] * 2 + ["far_start", "consistent"]
    assert len(names) >= 16
    rng = np.random.default_rng(5)
    first = None
    for order in (list(range(len(names))), list(rng.permutation(len(names)))):
        batch = [names[i] for i in order]
        built = [objects(PC.build(n)[2]) for n in batch]
        for rep in range(2 if order == list(range(len(names))) else 1):
            out = tp.global_optimization_batch([pose_graph(n) for n in batch], None, [b[0] for b in built],
                                               [b[1] for b in built], trace=TRACE)
            for name, res in zip(batch, out):
                assert bits(res) == bits(alone(name)), name
            if first is None:
                first = [bits(r) for r in out]
            elif rep == 1:
                assert [bits(r) for r in out] == first  # the same call twice: the same bits


def test_global_optimization_works_in_place_like_open3d():
    pg = pose_graph("gross_chord")
    crit, option = objects(PC.build("gross_chord")[2])
    res = tp.global_optimization(pg, tp.GlobalOptimizationLevenbergMarquardt(), crit, option)
    want = alone("gross_chord")
    assert len(pg.edges) == 9 and all(not (e.source_node_id, e.target_node_id) == (5, 1) for e in pg.edges)
    assert np.array_equal(np.stack([n.pose for n in pg.nodes]), want.poses)
    assert [e.confidence for e in pg.edges] == [c for c, gone in zip(want.confidence, want.pruned) if not gone]
    assert res.status == want.status and res.pruned.tolist() == want.pruned.tolist()
    with pytest.raises(NotImplementedError):
        tp.global_optimization(pg, tp.GlobalOptimizationGaussNewton())


def test_refusals_name_the_argument_and_leave_the_graph_alone():
    pg = pose_graph("consistent")
    pg.edges[3].source_node_id = 7
    before = [n.pose.copy() for n in pg.nodes]
    with pytest.raises(tp.TeaserHipError, match="edge_source.*edge 3.*problem 0"):
        tp.global_optimization(pg)
    assert all(np.array_equal(a, n.pose) for a, n in zip(before, pg.nodes)) and len(pg.edges) == 10
    pg = pose_graph("consistent")
    pg.nodes[2].pose[0, 0] = np.nan
    with pytest.raises(tp.TeaserHipError, match="poses.*node 2"):
        tp.global_optimization(pg)
    with pytest.raises(tp.TeaserHipError, match="max_iteration"):
        tp.global_optimization(pose_graph("consistent"), criteria=tp.GlobalOptimizationConvergenceCriteria(max_iteration=1001))
    with pytest.raises(tp.TeaserHipError, match="reference_node"):
        tp.global_optimization(pose_graph("consistent"), option=tp.GlobalOptimizationOption(reference_node=7))


def test_cxx_facade_reproduces_python(tmp_path):
    import subprocess

    from posegraph_cxx import build_posegraph_example
    from test_posegraph_emulation import read_result
    exe = build_posegraph_example()
    assert subprocess.run([exe], capture_output=True, timeout=120).returncode == 0
    gfile, rfile = str(tmp_path / "graph.txt"), str(tmp_path / "result.txt")
    PC.write_graph_file(gfile, "gross_chord")
    out = subprocess.run([exe, gfile, rfile], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    got, want = read_result(rfile, 7, 10), as_got(alone("gross_chord"))
    for key in ("status", "iterations", "trials", "flags", "lam", "F0", "F", "mu"):
        assert got[key] == want[key], key
    assert got["pruned"] == want["pruned"].astype(int).tolist()
    assert got["poses"].tobytes() == want["poses"].tobytes() and got["confidence"].tobytes() == want["confidence"].tobytes()


def test_multiway_example_prunes_the_wrong_closure_and_matches_the_restatement():
    """examples/teaser_python_multiway.py with K = 5: ICP of all pairs, their information matrices, one injected wrong
    loop closure, global_optimization -- then the restatement on the graph the device pipeline produced, after the
    margin conditions on that graph."""
    import os
    import sys

    from util import ROOT
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import teaser_python_multiway as mw
    out = mw.run(mw.read_ply_xyz(os.path.join(ROOT, "tests", "golden", "bun_zipper_res3.ply")), views=5, seed=3)
    res, wrong, before = out["result"], out["wrong"], out["before"]
    assert np.flatnonzero(res.pruned).tolist() == [wrong] and len(out["graph"].edges) == len(before.edges) - 1
    assert res.F <= res.F0
    start = np.stack([n.pose for n in before.nodes])
    edges = [(e.source_node_id, e.target_node_id, e.transformation, e.information, e.uncertain) for e in before.edges]
    o, c = out["option"], out["criteria"]
    opt = {k: getattr(c if hasattr(c, k) else o, k) for k in G.DEFAULTS}
    refs = PC.reference_of(start, edges, opt)
    assert PC.margin_problems("multiway", refs[0], refs[1], opt, edges) == []
    traced = tp.global_optimization_batch([before], None, c, o, trace=TRACE)[0]
    assert bits(traced)[:4] == (res.poses.tobytes(), res.confidence.tobytes(), res.pruned.tobytes(),
                                np.array([res.F0, res.F] + res.mu).tobytes())
    PC.check_against_reference("multiway", as_got(traced), graph=(start, edges, opt), refs=refs)
    rot, trans = mw.pose_error(out["truth"], traced.poses)
    print("multiway: pose error against the truth %.3g rad %.3g m" % (rot, trans))
