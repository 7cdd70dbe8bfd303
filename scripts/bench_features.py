#!/usr/bin/env python3
"""Measures the correspondence front-end (teaser-plusplus_amd.correspondences_batch / compute_fpfh_batch /
match_features_batch) against one call per pair in the same process and run, and prints ONE JSON object.  One call per
pair (FPFHEstimation.computeFPFHFeatures x 2 + Matcher.calculateCorrespondences) is the same implementation with
batch = 1, so those rows measure what a call costs by itself: three calls, five host synchronisations and the
features' round trip through host memory per pair.
  single_pair   one config-5 pair (tests/golden/config5_clouds.npz, radii 2 and 5 voxels): one call per pair vs
                correspondences_batch with batch = 1
  batch64       64 perturbed config-5 pairs (the generator of bench.py's config-5 workload): correspondences_batch in
                one call vs the same 64 pairs with one call per pair, one after the other
  stages64      compute_fpfh_batch (128 clouds) and match_features_batch (64 pairs) separately on the same 64
  fixture       the object / scene pair of tests/golden/features_golden.npz (1 000 / 60 865 points, radii 0.02 and
                0.04 as the reference's matcher test), both ways: one call per pair, twice, vs one call of two pairs
  knn           (with --knn these workloads only) match_features_knn_batch with k = 1, 4 and 16, mutual, on the FPFH
                features of the config-5 pair alone and of the 64 perturbed pairs, beside match_features_batch (the 1-NN
                path) on the same features in the same run: the baseline the k-NN times are divided by
  tuple         (with --tuple this workload only) the tuple test of the 64 perturbed pairs' correspondences -- after the
                1-NN matcher, and after k = 8 mutual matching -- by tuple_test_batch in one call against the per-pair
                host loop it replaces (tp.tuple_test for every pair, same seeds, same machine), after asserting that
                the two give the same pairs; also written to profiles/features/tuple_test.json
The object also records the board's name, the ROCm version and the commit (None outside a git checkout).
Wall-clock medians over --reps synchronous calls after --warmup calls; ms_min / ms_max give the spread.  Usage:
    python scripts/bench_features.py [--reps 20] [--warmup 3] [--knn | --tuple]"""
import argparse
import ctypes
import importlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from features_batch_cases import config5_pairs  # noqa: E402

tp = importlib.import_module("teaser-plusplus_amd")


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return dict(ms=1e3 * float(np.median(ts)), ms_min=1e3 * min(ts), ms_max=1e3 * max(ts), reps=reps)


def board_and_rocm():
    """(device name and architecture as the HIP runtime reports them, ROCm version of the installation the runtime was loaded from)."""
    name = ctypes.create_string_buffer(256)
    try:
        hip = ctypes.CDLL("libamdhip64.so")
        board = name.value.decode() if hip.hipDeviceGetName(name, 256, 0) == 0 else ""
    except OSError:
        board = ""
    try:  # (the marketing name is empty where the driver's id table is missing: the architecture then)
        import torch
        arch = torch.cuda.get_device_properties(0).gcnArchName.split(":")[0]
        board = ("%s (%s)" % (board, arch)) if board else arch
    except Exception:
        pass
    board = board or None
    rocm = None
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            root = os.path.dirname(os.path.dirname(os.path.realpath(line.split()[-1])))
            try:
                rocm = open(os.path.join(root, ".info", "version")).read().strip()
            except OSError:
                pass
            break
    return board, rocm


def knn_workloads(res, A, B, src, dst, rn, rf, reps, warmup):
    """res["knn"]: per workload the 1-NN matcher's time and the k-NN matcher's for k = 1, 4, 16 (mutual), the ratio to
    the 1-NN time, and the number of pairs found."""
    fa, fb = tp.compute_fpfh_batch([A, B], rn, rf)
    feats = tp.compute_fpfh_batch(src + dst, rn, rf)
    res["knn"] = {}
    for name, fs, fd in (("single_pair", [fa], [fb]), ("batch64", feats[:64], feats[64:])):
        base = timed(lambda: tp.match_features_batch(fs, fd), reps, warmup)
        row = dict(match_features_batch=base, pairs_1nn=sum(len(p) for p in tp.match_features_batch(fs, fd)))
        for k in (1, 4, 16):
            t = timed(lambda: tp.match_features_knn_batch(fs, fd, k, True), reps, warmup)
            t["over_match_features_batch"] = t["ms"] / base["ms"]
            t["pairs"] = sum(len(p) for p in tp.match_features_knn_batch(fs, fd, k, True))
            row["knn_k%d_mutual" % k] = t
        res["knn"][name] = row


def tuple_workloads(res, src, dst, rn, rf, reps, warmup, scale=0.9):
    """res["tuple"]: per matcher the batched call's time, the per-pair host loop's, their ratio and the counts."""
    res["tuple"] = dict(tuple_scale=scale, seeds="1 .. 64")
    seeds = np.arange(1, len(src) + 1, dtype=np.uint64)
    for name, corr in (("after_1nn", tp.correspondences_batch(src, dst, rn, rf)),
                       ("after_knn_k8_mutual", tp.correspondences_knn_batch(src, dst, rn, rf, 8, True))):
        def host_loop():
            return [tp.tuple_test(src[k], dst[k], corr[k], scale, int(seeds[k])) for k in range(len(src))]

        def batched():
            return tp.tuple_test_batch(src, dst, corr, scale, seeds)
        want, got = host_loop(), batched()
        assert all([tuple(r) for r in g.tolist()] == w for g, w in zip(got, want)), name
        row = dict(tuple_test_batch=timed(batched, reps, warmup), host_loop=timed(host_loop, max(reps // 4, 3), 1),
                   pairs_in=sum(len(c) for c in corr), pairs_in_max=max(len(c) for c in corr),
                   pairs_out=sum(len(g) for g in got), trials=100 * sum(len(c) for c in corr))
        row["host_loop_over_tuple_test_batch"] = row["host_loop"]["ms"] / row["tuple_test_batch"]["ms"]
        row["host_loop_ns_per_trial"] = 1e6 * row["host_loop"]["ms"] / row["trials"]
        res["tuple"][name] = row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--knn", action="store_true", help="the k-NN matching workloads only")
    ap.add_argument("--tuple", action="store_true", help="the tuple-test workload only")
    a = ap.parse_args()
    if tp.device_count() < 1:
        sys.exit("bench_features.py needs an MI355X")
    src, dst, vox = config5_pairs(64)
    rn, rf = 2 * vox, 5 * vox
    est, matcher = tp.FPFHEstimation(), tp.Matcher()

    def single(s, d, rn=rn, rf=rf):  # one call per pair
        fa = est.computeFPFHFeatures(s, rn, rf)
        fb = est.computeFPFHFeatures(d, rn, rf)
        return matcher.calculateCorrespondences(s, d, fa, fb, False, True, False, 0)

    C5 = np.load(os.path.join(ROOT, "tests", "golden", "config5_clouds.npz"))
    A, B = C5["cloud_bin_0"], C5["cloud_bin_4"]
    res = {"workload": "FPFH (radii 2 and 5 voxels) + mutual nearest neighbours, config-5 pairs (%d / %d points)"
                       % (len(A), len(B))}
    res["board"], res["rocm_version"] = board_and_rocm()
    try:
        res["commit"] = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True,
                                       text=True).stdout.strip() or None
    except OSError:
        res["commit"] = None
    if a.knn:
        res["workload"] = "k-NN matching (k = 1, 4, 16, mutual) of config-5 FPFH features (%d / %d points)" % (len(A), len(B))
        knn_workloads(res, A, B, src, dst, rn, rf, a.reps, a.warmup)
        print(json.dumps(res))
        return
    if a.tuple:
        res["workload"] = ("tuple test (scale 0.9) of the correspondences of 64 config-5 pairs (%d / %d points): "
                           "tuple_test_batch vs the per-pair host loop" % (len(A), len(B)))
        tuple_workloads(res, src, dst, rn, rf, a.reps, a.warmup)
        out = os.path.join(ROOT, "profiles", "features", "tuple_test.json")
        with open(out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        print(json.dumps(res))
        return
    one = timed(lambda: single(A, B), a.reps, a.warmup)
    b1 = timed(lambda: tp.correspondences_batch([A], [B], rn, rf), a.reps, a.warmup)
    res["single_pair"] = dict(one_call_per_pair=one, batch1=b1, batch1_over_one_call_per_pair=b1["ms"] / one["ms"],
                              batch1_minus_one_call_per_pair_ms=b1["ms"] - one["ms"],
                              one_call_per_pair_spread_ms=one["ms_max"] - one["ms_min"])
    seq = timed(lambda: [single(s, d) for s, d in zip(src, dst)], a.reps, a.warmup)
    bat = timed(lambda: tp.correspondences_batch(src, dst, rn, rf), a.reps, a.warmup)
    res["batch64"] = dict(one_call_per_pair=seq, batched=bat, speedup=seq["ms"] / bat["ms"],
                          saved_ms=seq["ms"] - bat["ms"], one_call_per_pair_spread_ms=seq["ms_max"] - seq["ms_min"],
                          one_call_per_pair_ms_per_pair=seq["ms"] / 64, batched_ms_per_pair=bat["ms"] / 64)
    feats = tp.compute_fpfh_batch(src + dst, rn, rf)
    res["stages64"] = dict(fpfh_batch_128_clouds=timed(lambda: tp.compute_fpfh_batch(src + dst, rn, rf), a.reps, a.warmup),
                           match_batch_64_pairs=timed(lambda: tp.match_features_batch(feats[:64], feats[64:]), a.reps,
                                                      a.warmup))
    G = np.load(os.path.join(ROOT, "tests", "golden", "features_golden.npz"))
    obj, scene = G["matcher_object"], G["matcher_scene"]
    reps = max(a.reps // 4, 3)
    frn, frf = 0.02, 0.04
    res["fixture"] = dict(points=[len(obj), len(scene)], radii=[frn, frf],
                          one_call_per_pair=timed(lambda: (single(obj, scene, frn, frf), single(scene, obj, frn, frf)), reps, 1),
                          batched=timed(lambda: tp.correspondences_batch([obj, scene], [scene, obj], frn, frf), reps, 1))
    res["fixture"]["speedup"] = res["fixture"]["one_call_per_pair"]["ms"] / res["fixture"]["batched"]["ms"]
    knn_workloads(res, A, B, src, dst, rn, rf, a.reps, a.warmup)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
