#!/usr/bin/env python3
"""Pose-graph optimisation on the MI355X: what one batched call buys.

Per size n (default 64; also 8 and 128): `--graphs` graphs (default 64) of n nodes, each a ring of certain edges plus
3 n uncertain chords between random node pairs, a fifth of them gross (30 degrees, 1 m off), start poses perturbed;
every graph has its own seed.
  (a) global_optimization_batch: all graphs in ONE call (a workgroup per graph, one synchronisation);
  (b) the same graphs one call after the other;
  (c) the numpy restatement (tests/posegraph_reference.py, float64) of ONE graph on the same host -- the only baseline
      there is -- and its largest pose difference from the device result.

Every timing is a host clock around a call that ends in a device synchronise, after `--warmup` untimed calls, median and
spread of `--reps`.  Needs an MI355X: there is no CPU path.

    python scripts/bench_posegraph.py --reps 5 --warmup 1 --out profiles/posegraph/bench_posegraph.json"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
tp = importlib.import_module("teaser-plusplus_amd")


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t))
    return dict(median_ms=float(np.median(ts)), min_ms=float(min(ts)), max_ms=float(max(ts)), reps=reps)


def make_graph(n, seed):
    import posegraph_cases as PC
    rng = np.random.default_rng(1000 + seed)
    chords = []
    while len(chords) < 3 * n:
        a, b = (int(v) for v in rng.integers(0, n, 2))
        if a != b and (a + 1) % n != b and (b + 1) % n != a:
            chords.append((a, b))
    gross = tuple(int(k) for k in rng.choice(3 * n, size=(3 * n) // 5, replace=False))
    return PC.graph(seed, n=n, chords=tuple(chords), gross=gross, angle=0.02, shift=0.02)


def as_pose_graph(start, edges):
    return tp.PoseGraph([tp.PoseGraphNode(T) for T in start],
                        [tp.PoseGraphEdge(s, t, X, L, u) for s, t, X, L, u in edges])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--graphs", type=int, default=64)
    ap.add_argument("--sizes", default="64,8,128")
    ap.add_argument("--no-host-ref", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "posegraph", "bench_posegraph.json"))
    a = ap.parse_args()
    if tp.device_count() < 1:
        sys.exit("bench_posegraph.py needs an MI355X")
    out = dict(graphs=a.graphs, sizes={})
    for n in (int(v) for v in a.sizes.split(",")):
        raw = [make_graph(n, seed) for seed in range(1, a.graphs + 1)]
        pgs = [as_pose_graph(*g) for g in raw]
        res = tp.global_optimization_batch(pgs)
        row = dict(nodes=n, edges=len(raw[0][1]), unknowns=6 * (n - 1),
                   status=sorted(set(r.status_name for r in res)),
                   trials=[int(np.min([sum(r.trials) for r in res])), int(np.max([sum(r.trials) for r in res]))],
                   pruned=[int(np.min([r.pruned.sum() for r in res])), int(np.max([r.pruned.sum() for r in res]))])
        row["batch_one_call"] = timed(lambda: tp.global_optimization_batch(pgs), a.reps, a.warmup)
        row["single_calls"] = timed(lambda: [tp.global_optimization_batch([g]) for g in pgs], a.reps, a.warmup)
        row["one_graph"] = timed(lambda: tp.global_optimization_batch(pgs[:1]), a.reps, a.warmup)
        if not a.no_host_ref:
            import posegraph_reference as G
            t = time.perf_counter()
            ref = G.global_optimization(*raw[0])
            row["numpy_one_graph_ms"] = 1e3 * (time.perf_counter() - t)
            row["numpy_agrees"] = dict(status=int(ref["status"]) == res[0].status,
                                       pruned=ref["pruned"].tolist() == res[0].pruned.tolist(),
                                       largest_pose_difference=float(np.abs(ref["poses"] - res[0].poses).max()))
        out["sizes"][str(n)] = row
        print(json.dumps({str(n): row}), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
