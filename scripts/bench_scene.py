#!/usr/bin/env python3
"""The ray-casting scene (RaycastingScene) on the MI355X on the 512-voxel meshes of scripts/bench_tsdf.py: the 64-frame
scene fused into the dense and into the scalable volume at R = 512 and extracted as triangle meshes.

  (1) the build: add_triangles (host: conversion to float32 and the gather of nine floats per triangle) and commit (the
      upload, bounds, Morton keys, sort, hierarchy and refit, ending in a synchronise), a fresh scene every repetition;
  (2) one 640 x 480 view (cast_views, rays generated on the device) with the depth alone and with all maps;
  (3) the same rays through cast_rays (24 bytes per ray go up);
  (4) 300 000 closest-point queries (points of the volume's own cloud, moved by up to two voxels), all maps and the
      distance alone;
  (5) for context, in the same process: UniformTSDFVolume.ray_cast of the same view, depth alone and all maps.

Call times are a host clock around a Python call that ends in a device synchronise, after `--warmup` untimed calls:
median, minimum and maximum of `--reps`, all in one process.  No hardware counter is read and the copies are not timed
on their own.  Needs an MI355X: there is no CPU path.

    python scripts/bench_scene.py --reps 5 --warmup 1 --out profiles/scene/bench_scene.json"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "examples"))
tp = importlib.import_module("teaser-plusplus_amd")
bt = importlib.import_module("bench_tsdf")

QUERIES = 300000


def build_times(mesh, reps, warmup):
    add, commit = [], []
    for k in range(warmup + reps):
        with tp.RaycastingScene() as s:
            t0 = time.perf_counter()
            s.add_triangles(mesh)
            t1 = time.perf_counter()
            s.commit()
            t2 = time.perf_counter()
        if k >= warmup:
            add.append(1e3 * (t1 - t0)), commit.append(1e3 * (t2 - t1))
    stat = lambda ts: dict(median_ms=float(np.median(ts)), min_ms=float(min(ts)), max_ms=float(max(ts)), reps=reps)
    return dict(add_triangles=stat(add), commit=stat(commit))


def run_mesh(name, mesh, cloud, K, E, voxel, reps, warmup):
    res = dict(mesh=name, vertices=len(mesh.vertices), triangles=len(mesh.triangles))
    res["build"] = build_times(mesh, reps, warmup)
    rng = np.random.default_rng(11)
    pick = rng.integers(0, len(cloud), QUERIES)
    pts = (cloud[pick] + rng.uniform(-2.0 * voxel, 2.0 * voxel, (QUERIES, 3))).astype(np.float32)
    with tp.RaycastingScene() as s:
        s.add_triangles(mesh)
        s.commit()
        depth = s.cast_views(K, [E], bt.W, bt.H, pixel_offset=0.0, ids=False, uvs=False, normals=False)[0]["t_hit"]
        res["view_hits"] = int(np.isfinite(depth).sum())
        res["cast_views_depth"] = bt.timed(lambda: s.cast_views(K, [E], bt.W, bt.H, pixel_offset=0.0, ids=False, uvs=False, normals=False), reps, warmup)
        res["cast_views_all_maps"] = bt.timed(lambda: s.cast_views(K, [E], bt.W, bt.H, pixel_offset=0.0), reps, warmup)
        rays = tp.create_rays_pinhole(K, E, bt.W, bt.H, 0.0)
        same = s.cast_rays(rays)["t_hit"]
        res["cast_rays_equals_cast_views"] = bool(same.tobytes() == depth.tobytes())
        res["cast_rays_all_maps"] = bt.timed(lambda: s.cast_rays(rays), reps, warmup)
        d = s.compute_distance(pts)
        res["closest_queries"] = QUERIES
        res["closest_distance_median_voxels"] = float(np.median(d) / voxel)
        res["closest_points_all_maps"] = bt.timed(lambda: s.compute_closest_points(pts), reps, warmup)
        res["compute_distance"] = bt.timed(lambda: s.compute_distance(pts), reps, warmup)
        res["same_bits_twice"] = bool(s.compute_distance(pts).tobytes() == d.tobytes())
    return res, depth


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene", "bench_scene.json"))
    a = ap.parse_args()
    if tp.device_count() < 1:
        sys.exit("bench_scene.py needs an MI355X: no HIP device visible")
    K, d, e, _ = bt.workload()
    view = e[3]
    out = dict(width=bt.W, height=bt.H, frames=len(d), resolution=a.size, meshes=[])
    with bt.make(a.size, False) as vol:
        bt.one_call(vol, K, d, e, None)
        voxel = vol.voxel_length
        dense_mesh = vol.extract_triangle_mesh()
        cloud = vol.extract_point_cloud(normals=False).points
        model = vol.ray_cast(K, view, bt.W, bt.H, depth_max=6.0, vertex_map=False, normal_map=False)
        out["tsdf_ray_cast_depth"] = bt.timed(lambda: vol.ray_cast(K, view, bt.W, bt.H, depth_max=6.0, vertex_map=False, normal_map=False), a.reps, a.warmup)
        out["tsdf_ray_cast_all_maps"] = bt.timed(lambda: vol.ray_cast(K, view, bt.W, bt.H, depth_max=6.0), a.reps, a.warmup)
        out["tsdf_ray_cast_hits"] = int(model.hits)
    with bt.make_scalable(a.size, False) as svol:
        svol.integrate_batch(d, K, e, None, 1000.0, 6.0)
        scalable_mesh = svol.extract_mesh()
    for name, mesh in (("dense", dense_mesh), ("scalable", scalable_mesh)):
        res, depth = run_mesh(name, mesh, cloud, K, view, voxel, a.reps, a.warmup)
        both = np.isfinite(depth) & (model.depth > 0)
        res["median_depth_difference_to_tsdf_ray_cast_voxels"] = float(np.median(np.abs(depth[both] - model.depth[both])) / voxel)
        out["meshes"].append(res)
        print(json.dumps(res))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: v for k, v in out.items() if k != "meshes"}))


if __name__ == "__main__":
    main()
