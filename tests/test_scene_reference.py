"""The restatement of the ray-casting scene (tests/scene_reference.py) against cases whose answers are known by hand: a
unit right triangle hit at a known t, u, v from both sides, a ray in the triangle's plane, an origin on the surface, rays
without a direction and with non-finite components, every one of Ericson's seven regions of the closest point, ties
decided by the global index, DEAD triangles, the pinhole formulas at pixel_offset 0 and 0.5, and the names and defaults
of the Python layer."""
import importlib
import inspect

import numpy as np

import scene_reference as R

tp = importlib.import_module("teaser-plusplus_amd")

UNIT = [(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], dtype=np.float32), np.array([[0, 1, 2]], dtype=np.uint32))]
INVALID = 0xFFFFFFFF


def test_unit_triangle_from_both_sides():
    rays = np.array([[0.25, 0.5, 2, 0, 0, -1], [0.25, 0.5, -3, 0, 0, 1], [0.25, 0.5, -3, 0, 0, 2], [0.25, 0.5, 2, 0, 0, 1],
                     [0.75, 0.75, 2, 0, 0, -1], [0.5, 0.5, 1, 0, 0, -1], [0, 0, 1, 0, 0, -1], [1, 0, 1, 0, 0, -1]], dtype=np.float32)
    r = R.cast_rays(UNIT, rays)
    assert r["t_hit"].tolist() == [2.0, 3.0, 1.5, np.inf, np.inf, 1.0, 1.0, 1.0]      # t counts in units of |d|
    assert r["primitive_uvs"][:3].tolist() == [[0.25, 0.5]] * 3 and r["primitive_uvs"][3].tolist() == [0, 0]
    assert r["primitive_uvs"][5:].tolist() == [[0.5, 0.5], [0, 0], [1, 0]]           # the hypotenuse and two vertices are inside
    assert r["primitive_normals"][:3].tolist() == [[0, 0, 1]] * 3                   # the normal of the winding, whichever side is hit
    assert r["geometry_ids"].tolist() == [0, 0, 0, INVALID, INVALID, 0, 0, 0] and r["primitive_ids"][3] == INVALID
    assert r["t_hit"].dtype == np.float32 and r["geometry_ids"].dtype == np.uint32
    assert R.test_occlusions(UNIT, rays).tolist() == [1, 1, 1, 0, 0, 1, 1, 1]
    assert R.test_occlusions(UNIT, rays, 2.0, 2.0).tolist() == [1, 0, 0, 0, 0, 0, 0, 0]  # tnear <= t <= tfar, both ends inside
    assert R.test_occlusions(UNIT, rays, 2.5, np.inf).tolist() == [0, 1, 0, 0, 0, 0, 0, 0]


def test_in_plane_on_surface_and_rays_that_take_no_part():
    rays = np.array([[-1, 0.25, 0, 1, 0, 0], [0.25, 0.25, 0, 0, 0, 1], [0.25, 0.25, 0, 0, 0, -1], [0.25, 0.25, 0, 1, 1, 1],
                     [0.25, 0.25, 1, 0, 0, 0], [0.25, 0.25, 1, 0, 0, np.nan], [np.inf, 0.25, 1, 0, 0, -1], [0.25, 0.25, 1, 0, -np.inf, -1]],
                    dtype=np.float32)
    r = R.cast_rays(UNIT, rays)
    assert r["t_hit"].tolist() == [np.inf, 0.0, 0.0, 0.0, np.inf, np.inf, np.inf, np.inf]   # det == 0 misses; t = 0 hits
    assert r["primitive_ids"].tolist() == [INVALID, 0, 0, 0] + [INVALID] * 4


def test_ties_go_to_the_smallest_global_index_and_dead_triangles_are_skipped():
    v, t = UNIT[0]
    dead = (np.array([[0, 0, 0], [1, 1, 0], [2, 2, 0], [0.5, 0.5, 0]], dtype=np.float32), np.array([[0, 1, 2], [3, 3, 3], [0, 0, 1]], dtype=np.uint32))
    geoms = [dead, (v, np.array([[0, 1, 2], [1, 2, 0]], dtype=np.uint32)), (v + np.float32([0, 0, 1]), t)]
    T = R.Triangles(geoms)
    assert T.dead.tolist() == [True, True, True, False, False, False]
    r = R.cast_rays(geoms, np.array([[0.25, 0.25, 0.5, 0, 0, -1], [0.25, 0.25, 0.5, 0, 0, 1], [0.5, 0.5, 3, 0, 0, -1]], dtype=np.float32))
    assert r["geometry_ids"].tolist() == [1, 2, 2] and r["primitive_ids"].tolist() == [0, 0, 0] and r["t_hit"].tolist() == [0.5, 0.5, 2.0]
    c = R.closest_points(geoms, np.array([[0.5, 0.5, 0.0], [0.5, 0.5, 0.5], [0.5, 0.5, 0.75]], dtype=np.float32))
    assert c["geometry_ids"].tolist() == [1, 1, 2] and c["primitive_ids"].tolist() == [0, 0, 0]   # a DEAD triangle holds (0.5, 0.5, 0) too
    assert c["distance"].tolist() == [0.0, 0.5, 0.25]
    none = R.closest_points([dead], np.zeros((2, 3), dtype=np.float32))
    assert np.isinf(none["distance"]).all() and (none["geometry_ids"] == INVALID).all() and not none["points"].any()


def test_every_region_of_the_closest_point():
    pts = np.array([[-1, -1, 1], [2, -0.5, 0], [0.5, -1, 2], [-0.5, 2, 0], [-1, 0.5, 0], [1, 1, 3], [0.25, 0.25, -2]], dtype=np.float32)
    T = R.Triangles(UNIT)
    _, _, _, _, region, live = R.closest_point_pairs(T, pts)
    assert region[:, 0].tolist() == [0, 1, 2, 3, 4, 5, 6] and live.all()    # A, B, AB, C, AC, BC, face -- the order of the book
    c = R.closest_points(UNIT, pts)
    assert c["points"].tolist() == [[0, 0, 0], [1, 0, 0], [0.5, 0, 0], [0, 1, 0], [0, 0.5, 0], [0.5, 0.5, 0], [0.25, 0.25, 0]]
    assert c["primitive_uvs"].tolist() == [[0, 0], [1, 0], [0.5, 0], [0, 1], [0, 0.5], [0.5, 0.5], [0.25, 0.25]]
    assert np.array_equal(c["distance"], np.sqrt(np.array([3, 1.25, 5, 1.25, 1, 9.5, 4])).astype(np.float32))
    assert (c["primitive_normals"] == [0, 0, 1]).all() and (c["geometry_ids"] == 0).all()
    bad = R.closest_points(UNIT, np.array([[np.nan, 0, 0], [0, np.inf, 0]], dtype=np.float32))
    assert np.isinf(bad["distance"]).all() and (bad["primitive_ids"] == INVALID).all()


def test_pinhole_formulas_at_both_offsets():
    K = np.array([[4.0, 0, 1.0], [0, 2.0, 0.5], [0, 0, 1]])
    E = np.eye(4)
    E[:3, 3] = [1.0, -2.0, 3.0]
    for fn in (R.create_rays_pinhole, tp.create_rays_pinhole, tp.RaycastingScene.create_rays_pinhole):
        r = fn(K, E, 3, 2, 0.0)
        assert r.shape == (2, 3, 6) and r.dtype == np.float32
        assert (r[..., :3] == [-1.0, 2.0, -3.0]).all()                         # the centre: -R^T t
        assert r[..., 3].tolist() == [[-0.25, 0, 0.25]] * 2 and r[..., 4].tolist() == [[-0.25] * 3, [0.25] * 3] and (r[..., 5] == 1).all()
        h = fn(K, E, 3, 2)
        assert h[..., 3].tolist() == [[-0.125, 0.125, 0.375]] * 2 and h[..., 4].tolist() == [[0.0] * 3, [0.5] * 3]
    c, s = np.cos(0.7), np.sin(0.7)
    E2 = np.array([[c, -s, 0, 0.3], [s, c, 0, -0.2], [0, 0, 1, 0.9], [0, 0, 0, 1]])
    a = tp.create_rays_pinhole(tp.PinholeCameraIntrinsic(7, 5, 9.0, 8.0, 3.2, 2.1), E2, 7, 5, 0.5)
    assert a.tobytes() == R.create_rays_pinhole(np.array([[9.0, 0, 3.2], [0, 8.0, 2.1], [0, 0, 1]]), E2, 7, 5, 0.5).tobytes()
    d = a[2, 4, 3:].astype(np.float64)
    assert np.allclose(E2[:3, :3] @ d, [(4.5 - 3.2) / 9.0, (2.5 - 2.1) / 8.0, 1.0], atol=1e-6)   # the camera sees it at the pixel, z = 1
    assert tp.create_rays_pinhole(K, E, 0, 0).shape == (0, 0, 6)


def test_names_and_defaults_of_the_python_layer():
    S = tp.RaycastingScene
    for name in ("add_triangles", "commit", "triangle_count", "cast_rays", "test_occlusions", "compute_closest_points", "compute_distance",
                 "cast_views", "render_depth", "create_rays_pinhole", "fill_scratch", "close"):
        assert callable(getattr(S, name)), name
    assert S.INVALID_ID == INVALID and "RaycastingScene" in tp.__all__ and "create_rays_pinhole" in tp.__all__
    assert "scene" not in tp.SCRATCH_KINDS
    sig = inspect.signature
    assert sig(tp.create_rays_pinhole).parameters["pixel_offset"].default == 0.5
    assert list(sig(tp.create_rays_pinhole).parameters) == ["intrinsic_matrix", "extrinsic_matrix", "width_px", "height_px", "pixel_offset"]
    occ = sig(S.test_occlusions).parameters
    assert occ["tnear"].default == 0.0 and occ["tfar"].default == float("inf")
    assert list(sig(S.render_depth).parameters) == ["self", "intrinsic", "extrinsic", "width", "height", "depth_max"]
    assert sig(S.render_depth).parameters["depth_max"].default is None and sig(S.cast_views).parameters["pixel_offset"].default == 0.5
