#!/usr/bin/env python3
"""Open3D's multiway-registration tutorial without Open3D, everything on the MI355X: K views of one model ->
pairwise ICP of ALL pairs in one call (registration_icp_batch) -> their information matrices in one call
(get_information_matrix_from_point_clouds_batch) -> a pose graph whose odometry edges (i + 1 -> i) are certain and
whose loop closures are uncertain, plus ONE injected wrong loop closure -> global_optimization (Levenberg-Marquardt
with a line process; the wrong closure is pruned after the first pass).  Usage:

    python examples/teaser_python_multiway.py [model.ply] [--views 5] [--seed 1] [--distance 0.01]

The views are random subsets (70 %) of the model under known poses, so the result can be compared with the truth; the
start poses are the truth perturbed by a few degrees and millimetres.  Without a file argument the model is
tests/golden/bun_zipper_res3.ply."""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
tp = importlib.import_module("teaser-plusplus_amd")

from examples.teaser_python_fpfh import read_ply_xyz  # noqa: E402


def rigid(axis, angle, t):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K
    T[:3, 3] = t
    return T


def inverse(T):
    out = np.eye(4)
    out[:3, :3] = T[:3, :3].T
    out[:3, 3] = -T[:3, :3].T @ T[:3, 3]
    return out


def make_views(model, views, seed):
    """K clouds, each a random 70 % of the model in its own frame; truth[i] maps view i's frame to the model's;
    start[i] is truth[i] perturbed (view 0 is the reference and is not)."""
    rng = np.random.default_rng(seed)
    extent = float(np.linalg.norm(model.max(0) - model.min(0)))
    centre = model.mean(0)
    clouds, truth, start = [], [], []
    for i in range(views):
        T = rigid([0.1, 1.0, 0.2], 0.35 * i, 0.0 * centre) if i else np.eye(4)
        T[:3, 3] = centre - T[:3, :3] @ centre + (0.1 * extent * rng.normal(0, 1, 3) if i else 0)
        keep = rng.random(len(model)) < 0.7
        clouds.append((model[keep] - T[:3, 3]) @ T[:3, :3])  # R^T (p - t)
        truth.append(T)
        noise = rigid(rng.normal(0, 1, 3), 0.03 * rng.normal(), 0.01 * extent * rng.normal(0, 1, 3))
        start.append(noise @ T if i else T.copy())
    return clouds, np.stack(truth), np.stack(start)


def build_pose_graph(clouds, truth, start, distance, device=-1):
    """All pairs s > t registered and weighted in two batched calls; returns the PoseGraph and the index of the
    injected wrong closure."""
    views = len(clouds)
    pairs = [(s, t) for t in range(views) for s in range(t + 1, views)]
    inits = [inverse(start[t]) @ start[s] for s, t in pairs]
    icp = tp.registration_icp_batch([clouds[s] for s, _ in pairs], [clouds[t] for _, t in pairs], distance, inits,
                                    tp.ICPConvergenceCriteria(max_iteration=50), device=device)
    infos = tp.get_information_matrix_from_point_clouds_batch(
        [clouds[s] for s, _ in pairs], [clouds[t] for _, t in pairs], distance, [r.transformation for r in icp],
        device=device)
    pg = tp.PoseGraph([tp.PoseGraphNode(T) for T in start])
    for (s, t), r, info in zip(pairs, icp, infos):
        pg.edges.append(tp.PoseGraphEdge(s, t, r.transformation, info, uncertain=(s != t + 1)))
    # the wrong closure: the last view against the first, 30 degrees and a tenth of the model off
    s, t = views - 1, 0
    wrong = inverse(truth[t]) @ truth[s] @ rigid([1.0, -0.5, 0.3], np.deg2rad(30.0), 0.1 * np.ptp(clouds[0], axis=0))
    pg.edges.append(tp.PoseGraphEdge(s, t, wrong, infos[pairs.index((s, t))], uncertain=True))
    return pg, len(pg.edges) - 1


def pose_error(a, b):
    """Largest rotation angle (radians) and translation distance between corresponding poses."""
    rot = trans = 0.0
    for x, y in zip(a, b):
        d = inverse(x) @ y
        rot = max(rot, float(np.arccos(np.clip((np.trace(d[:3, :3]) - 1) / 2, -1, 1))))
        trans = max(trans, float(np.linalg.norm(d[:3, 3])))
    return rot, trans


def run(model, views=5, seed=1, distance=0.01, device=-1):
    clouds, truth, start = make_views(np.asarray(model, dtype=np.float64), views, seed)
    pg, wrong = build_pose_graph(clouds, truth, start, distance, device)
    option = tp.GlobalOptimizationOption(max_correspondence_distance=distance, edge_prune_threshold=0.25, reference_node=0)
    criteria = tp.GlobalOptimizationConvergenceCriteria()
    before = tp.PoseGraph([tp.PoseGraphNode(n.pose) for n in pg.nodes],
                          [tp.PoseGraphEdge(e.source_node_id, e.target_node_id, e.transformation, e.information,
                                            e.uncertain) for e in pg.edges])
    result = tp.global_optimization(pg, tp.GlobalOptimizationLevenbergMarquardt(), criteria, option, device=device)
    return dict(graph=pg, before=before, wrong=wrong, result=result, truth=truth, start=start, option=option,
                criteria=criteria)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("model", nargs="?", default=os.path.join(ROOT, "tests", "golden", "bun_zipper_res3.ply"))
    ap.add_argument("--views", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--distance", type=float, default=0.01, help="max_correspondence_distance of ICP and of the graph")
    a = ap.parse_args()
    if tp.device_count() < 1:
        sys.exit("this example needs an MI355X: no HIP device visible")
    out = run(read_ply_xyz(a.model), a.views, a.seed, a.distance)
    res = out["result"]
    print("%d views, %d edges, wrong closure = edge %d" % (a.views, len(res.pruned), out["wrong"]))
    print("status %s, iterations %s, trials %s, F %.6g -> %.6g" % (res.status_name, res.iterations, res.trials, res.F0, res.F))
    print("pruned edges:", np.flatnonzero(res.pruned).tolist(), " confidence of the wrong closure: %.3g" % res.confidence[out["wrong"]])
    print("pose error against the truth (rad, m): start %.3g %.3g -> optimised %.3g %.3g" % (
        pose_error(out["truth"], out["start"]) + pose_error(out["truth"], [n.pose for n in out["graph"].nodes])))


if __name__ == "__main__":
    main()
