#!/usr/bin/env python3
"""Information matrices on the MI355X: what one batched call buys.

  (a) get_information_matrix_from_point_clouds_batch for 64 config-5-sized pairs (the pair of
      tests/golden/config5_clouds.npz under its committed pose, 64 jittered copies) in ONE call, against the same pairs
      one call after the other;
  (b) the numpy form (tests/information_reference.py: cKDTree correspondences + vectorised sums) of one pair on the same
      host -- the only baseline there is;
  (c) evaluate_registration_batch on the same pairs, i.e. the call without the reduction: their difference is what the
      two reduction launches and the copy of 36 doubles per pair cost.

Every timing is a host clock around a call that ends in a device synchronise, after `--warmup` untimed calls, median and
spread of `--reps`.  Needs an MI355X: there is no CPU path.

    python scripts/bench_information.py --reps 10 --warmup 2 --out profiles/information/bench_information.json"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--no-host-ref", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "information", "bench_information.json"))
    a = ap.parse_args()
    if tp.device_count() < 1:
        sys.exit("bench_information.py needs an MI355X")
    import icp_reference as R
    P, Q, vox, T = R.config5_problem()
    r = 1.5 * vox
    rng = np.random.default_rng(1)
    Ps = [P + 0.05 * vox * rng.standard_normal(P.shape) for _ in range(a.pairs)]
    Qs = [Q] * a.pairs
    info, res = tp.get_information_matrix_from_point_clouds_batch(Ps, Qs, r, T, return_results=True)
    out = dict(points=[len(P), len(Q)], pairs=a.pairs, max_correspondence_distance=r,
               correspondences=[len(x.correspondence_set) for x in res][:4])
    out["a"] = dict(
        batch_one_call=timed(lambda: tp.get_information_matrix_from_point_clouds_batch(Ps, Qs, r, T), a.reps, a.warmup),
        single_calls=timed(lambda: [tp.get_information_matrix_from_point_clouds(p, Q, r, T) for p in Ps], a.reps, a.warmup),
        one_pair=timed(lambda: tp.get_information_matrix_from_point_clouds(Ps[0], Q, r, T), a.reps, a.warmup))
    if not a.no_host_ref:
        import information_reference as I

        def host():
            cs = R.registration_icp(Ps[0], Q, r, T, 0)["correspondence_set"]
            return I.information_vectorised(Q, cs[:, 1])[0]
        t = time.perf_counter()
        ref = host()
        out["b"] = dict(numpy_one_pair_ms=1e3 * (time.perf_counter() - t),
                        largest_relative_difference=float(np.abs(ref - info[0]).max() / np.abs(ref).max()))
    out["c"] = dict(evaluate_registration_batch=timed(lambda: tp.evaluate_registration_batch(Ps, Qs, r, T), a.reps, a.warmup))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
