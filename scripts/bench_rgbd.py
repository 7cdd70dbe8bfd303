#!/usr/bin/env python3
"""The depth-frame calls (create_point_cloud_from_rgbd_image, project_to_rgbd_image on the ICP handle) on the MI355X:
what a call costs, and how much of it is kernels.

  (1) one 640 x 480 uint16 frame with an RGB image (points and colours out);
  (2) 16 such frames in ONE call and as 16 calls;
  (3) a cloud of 300 000 coloured points projected into 640 x 480 (depth and colour out);
  (4) the numpy restatement (tests/rgbd_reference.py) of (1) and (3), and whether the device's bits equal it.

Call times are a host clock around a Python call that ends in a device synchronise, after `--warmup` untimed calls:
median, minimum and maximum of `--reps` (at least nine; the restatement: two).  A call includes the host's checks and
packing, the uploads, the launches, the one copy back and the scatter into the caller's arrays.

Kernel time comes from a run of its own: `--profile-workload` runs three calls each of (1), (2, one call) and (3) and
writes nothing; `rocprofv3 --kernel-trace --memory-copy-trace --stats` is pointed at it.  `--kernel-stats CSV [--copy-stats
CSV]` then folds that run's tables into the JSON: per kernel the mean time per launch, the bytes the contract moves (the
functions below) over that time, and that rate as a share of the 8 TB/s HBM peak -- for the launches of workload (2) and
(3), which the kernel names and call counts identify.  Needs an MI355X: there is no CPU path.

    python scripts/bench_rgbd.py --reps 9 --warmup 2 --out profiles/rgbd/bench_rgbd.json"""
import argparse
import csv
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
import rgbd_reference as R  # noqa: E402

W, H, FRAMES, POINTS = 640, 480, 16, 300000
HBM_PEAK = 8.0e12


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t))
    return dict(median_ms=float(np.median(ts)), min_ms=float(min(ts)), max_ms=float(max(ts)), reps=reps)


def frame(seed):
    """A 640 x 480 frame: a slanted surface between 0.8 and 2.8 m with ripples, a fifth of the samples 0, and an RGB
    image."""
    rng = np.random.default_rng(seed)
    i, j = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    z = 1800 + 900 * np.sin(i / 97.0 + seed) * np.cos(j / 131.0) + 100 * rng.random((H, W))
    d = z.astype(np.uint16)
    d[rng.random((H, W)) < 0.2] = 0
    return d, rng.integers(0, 256, size=(H, W, 3)).astype(np.uint8)


def cloud(seed):
    rng = np.random.default_rng(seed)
    z = 0.8 + 2.0 * rng.random(POINTS)
    xy = (rng.random((POINTS, 2)) - 0.5) * [1.3, 1.0] * z[:, None]
    return np.column_stack([xy, z]), rng.random((POINTS, 3))


def unproject_bytes(n_vis, n_rows, colour):
    """The bytes the contract moves per launch: the count pass reads the depth and writes a count per tile; the write pass
    reads the depth again (and the colour of the rows it emits) and writes 24 bytes per row and output."""
    tiles = -(-n_vis // 256)
    return dict(rgbd_count_kernel=2 * n_vis + 4 * tiles,
                rgbd_scan_kernel=12 * tiles,
                rgbd_write_kernel=2 * n_vis + 4 * tiles + (3 + 24 if colour else 0) * n_rows + 24 * n_rows)


def project_bytes(n, px, n_hit, colour):
    """The fill writes a key per pixel; the scatter reads a point and updates a key per landed point; the resolve reads a
    key per pixel and a colour per hit and writes depth (and colour)."""
    return dict(fill=8 * px, rgbd_scatter_kernel=24 * n + 16 * n, rgbd_resolve_kernel=8 * px + 4 * px +
                ((24 * n_hit + 12 * px) if colour else 0))


def fold_kernel_stats(out, path, copy_path):
    """Per kernel of the profiled run: launches, mean microseconds, and for the kernels of this feature the rate."""
    rows = list(csv.DictReader(open(path)))
    table = {}
    for r in rows:
        name = r["Name"]
        short = next((k for k in ("rgbd_count_kernel", "rgbd_scan_kernel", "rgbd_write_kernel", "rgbd_scatter_kernel",
                                  "rgbd_resolve_kernel", "fillBuffer", "copyBuffer") if k in name), name[:60])
        table[short] = dict(calls=int(r["Calls"]), total_us=float(r["TotalDurationNs"]) / 1e3,
                            mean_us=float(r["AverageNs"]) / 1e3, min_us=float(r["MinNs"]) / 1e3, max_us=float(r["MaxNs"]) / 1e3)
    out["profiled_run"] = dict(kernels=table, note="three calls each of workloads (1), (2, one call) and (3); the longest "
                               "launch of an unprojection kernel (max_us) is the 16-frame call's")
    u16 = out["bytes_moved"]["unproject_16_frames"]
    pj = out["bytes_moved"]["project_300k"]
    shares = {}
    for k, b in list(u16.items()) + [(k, v) for k, v in pj.items() if k != "fill"]:
        if k in table and table[k]["max_us"] > 0:
            t = table[k]["max_us"] if k in u16 else table[k]["mean_us"]
            shares[k] = dict(bytes=b, us=t, GB_per_s=b / t / 1e3, share_of_hbm_peak=b / (t * 1e-6) / HBM_PEAK)
    out["profiled_run"]["hbm"] = shares
    if copy_path:
        out["profiled_run"]["copies"] = {r["Name"]: dict(calls=int(r["Calls"]), total_us=float(r["TotalDurationNs"]) / 1e3)
                                         for r in csv.DictReader(open(copy_path))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-host", action="store_true", help="skip the numpy restatement")
    ap.add_argument("--profile-workload", action="store_true", help="three calls of each workload, nothing else")
    ap.add_argument("--kernel-stats", default="", metavar="CSV", help="fold a rocprofv3 kernel_stats table into --out")
    ap.add_argument("--copy-stats", default="", metavar="CSV", help="with --kernel-stats: the memory_copy_stats table")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rgbd", "bench_rgbd.json"))
    a = ap.parse_args()
    if a.kernel_stats:  # no device needed: arithmetic on two files
        out = json.load(open(a.out))
        fold_kernel_stats(out, a.kernel_stats, a.copy_stats)
        json.dump(out, open(a.out, "w"), indent=1)
        print(json.dumps(out["profiled_run"]))
        return
    if a.reps < 9:
        sys.exit("at least nine runs")
    if tp.device_count() < 1:
        sys.exit("bench_rgbd.py needs an MI355X")
    K = tp.PinholeCameraIntrinsic(W, H, 525.0, 525.0, 319.5, 239.5)
    frames = [frame(s) for s in range(FRAMES)]
    depths, colors = [f[0] for f in frames], [f[1] for f in frames]
    P, C = cloud(7)
    one = lambda k=0: tp.create_point_cloud_from_rgbd_image(colors[k], depths[k], K, convert_rgb_to_intensity=False)  # noqa: E731
    many = lambda: tp.create_point_cloud_from_rgbd_image_batch(colors, depths, K, convert_rgb_to_intensity=False)  # noqa: E731
    proj = lambda: tp.project_to_rgbd_image(P, C, W, H, K)  # noqa: E731
    if a.profile_workload:
        for _ in range(3):
            one(), many(), proj()
        return
    out = dict(reps=a.reps, warmup=a.warmup, width=W, height=H, frames=FRAMES, points=POINTS)
    pts, cols = one()
    out["one_frame"] = dict(valid_pixels=len(pts), bytes_in=2 * W * H + 3 * W * H, bytes_back=W * H * 48 + 8,
                            one_call=timed(one, a.reps, a.warmup))
    print("one", out["one_frame"], file=sys.stderr, flush=True)
    res = many()
    out["sixteen_frames"] = dict(valid_pixels=int(sum(len(p) for p, _ in res)), bytes_back=FRAMES * W * H * 48 + 64,
                                 one_call=timed(many, a.reps, a.warmup),
                                 single_calls=timed(lambda: [one(k) for k in range(FRAMES)], a.reps, a.warmup),
                                 same_bits=bool(all(one(k)[0].tobytes() == res[k][0].tobytes() for k in range(FRAMES))))
    print("sixteen", out["sixteen_frames"], file=sys.stderr, flush=True)
    d, c = proj()
    n_hit = int((d > 0).sum())
    out["project_300k"] = dict(n_hit=n_hit, bytes_in=48 * POINTS, bytes_back=W * H * 16 + 8,
                               one_call=timed(proj, a.reps, a.warmup),
                               depth_only=timed(lambda: tp.project_to_depth_image(P, W, H, K), a.reps, a.warmup))
    print("project", out["project_300k"], file=sys.stderr, flush=True)
    out["bytes_moved"] = dict(unproject_one_frame=unproject_bytes(W * H, len(pts), True),
                              unproject_16_frames=unproject_bytes(FRAMES * W * H, out["sixteen_frames"]["valid_pixels"], True),
                              project_300k=project_bytes(POINTS, W * H, n_hit, True))
    if not a.no_host:
        f = R.Frame(K.fx, K.fy, K.cx, K.cy, depth_scale=1000.0, depth_trunc=3.0)
        host_u = lambda: R.unproject(depths[0], colors[0], f)  # noqa: E731
        _, hp, hc, _ = host_u()
        cam = R.Camera(W, H, K.fx, K.fy, K.cx, K.cy, None, 1000.0, 3.0)
        host_p = lambda: R.project(P, C, cam)  # noqa: E731
        hd, hci, _, _ = host_p()
        out["numpy_restatement"] = dict(
            unproject_one_frame=dict(timed(host_u, 2, 0), equal_to_device=bool(hp.tobytes() == pts.tobytes() and
                                                                                hc.tobytes() == cols.tobytes())),
            project_300k=dict(timed(host_p, 2, 0), equal_to_device=bool(hd.tobytes() == d.tobytes() and
                                                                        hci.tobytes() == c.tobytes())))
        print("numpy", out["numpy_restatement"], file=sys.stderr, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
