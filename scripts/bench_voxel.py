#!/usr/bin/env python3
"""Measures the batched voxel down-sampling (teaser-plusplus_amd.voxel_down_sample / voxel_down_sample_batch) and
prints ONE JSON object (and writes it to --out when given):
  single      one 313 395-point scan-like cloud (tests/voxel_reference.py scan_like, the size of the tutorial's
              cloud_bin_4), voxel 0.05: wall clock of the call (host checks + H2D + kernels + D2H), and the same with
              return_counts / return_trace
  batch64     64 clouds of 40 k points (scan-like, different seeds) in one call, against the same 64 as sequential
              single calls
  host_ref    the numpy restatement (tests/voxel_reference.py) and the fixture generator's np.add.reduceat form on
              the same host and cloud, single-threaded Python
Wall-clock medians over --reps calls after --warmup calls (every call is synchronous).  Usage:
    python scripts/bench_voxel.py [--reps 20] [--warmup 3] [--no-host-ref] [--out profiles/voxel/bench_voxel.json]"""
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
import voxel_reference as R  # noqa: E402

tp = importlib.import_module("teaser-plusplus_amd")


def timed(fn, reps, warmup):
    for _ in range(warmup):
        out = fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), out


def reduceat_form(p, voxel):
    """tests/golden/make_config5_golden.py's down-sampling (the form that made config5_clouds.npz)."""
    lo = p.min(0) - voxel * 0.5
    idx = np.floor((p - lo) / voxel).astype(np.int64)
    key = (idx[:, 0] * (1 << 42)) + (idx[:, 1] * (1 << 21)) + idx[:, 2]
    order = np.argsort(key, kind="stable")
    key, q = key[order], p[order]
    start = np.flatnonzero(np.concatenate([[True], key[1:] != key[:-1]]))
    sums = np.add.reduceat(q, start, axis=0)
    cnt = np.diff(np.concatenate([start, [len(q)]]))[:, None]
    return sums / cnt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-host-ref", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if tp.device_count() < 1:
        sys.exit("bench_voxel.py needs an MI355X")
    v = 0.05
    P = R.scan_like()
    res = {"workload": "voxel down-sampling, voxel %.2f: one %d-point cloud; 64 x 40 k points" % (v, len(P))}

    t, o = timed(lambda: tp.voxel_down_sample(P, v), a.reps, a.warmup)
    tt, _ = timed(lambda: tp.voxel_down_sample(P, v, return_counts=True, return_trace=True), a.reps, a.warmup)
    res["single"] = dict(points=len(P), voxels=len(o), ms=1e3 * t, ms_with_counts_and_trace=1e3 * tt,
                         input_MB=P.nbytes / 1e6)

    clouds = [R.scan_like(seed=1000 + k, n=40000) for k in range(64)]
    tb, ob = timed(lambda: tp.voxel_down_sample_batch(clouds, v), a.reps, a.warmup)
    ts, _ = timed(lambda: [tp.voxel_down_sample(c, v) for c in clouds], max(a.reps // 4, 3), 1)
    res["batch64"] = dict(points=int(sum(len(c) for c in clouds)), voxels=int(sum(len(x) for x in ob)),
                          batch_ms=1e3 * tb, sequential_ms=1e3 * ts, speedup=ts / tb)

    if not a.no_host_ref:
        th, ref = timed(lambda: R.voxel_down_sample(P, v), 3, 1)
        tr, _ = timed(lambda: reduceat_form(P, v), 5, 1)
        cores = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else os.cpu_count()
        res["host_ref"] = dict(restatement_ms=1e3 * th, reduceat_ms=1e3 * tr, python_threads=1,
                               cores_available=cores, speedup_vs_reduceat=tr / t,
                               same_bits=ref[0].tobytes() == o.tobytes())
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
