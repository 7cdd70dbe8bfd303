"""The ray-casting scene on the MI355X against the restatement (tests/scene_reference.py, pinned in
tests/test_scene_reference.py): every output must be EQUAL -- the bits of the float32 values, the integers as they are.
The restatement is a brute force over all triangles, so equality says that the search structure cut nothing off: scenes of
0, 1, 2 and 3 triangles; 0, 1, 63, 64, 65 and 257 rays; 200 copies of one triangle (equal Morton codes, the smallest index
wins every tie); 300 triangles on a line; the 9 x 9 lattice sheet with rays through vertices and along edges (six-way
ties), axis-parallel rays, rays in the plane, origins on the sheet and closest points on vertices, edges, between two
triangles and 10^4 sheet widths away; axis-aligned triangles (flat boxes) with grazing rays; the sheet offset by
(10^4, -10^4, 10^4); sizes 10^-3 and 10^3 in one scene; DEAD triangles; geometries added in several calls with a rebuild;
2 000 random triangles against 4 096 rays and points; occlusions with tnear == t exactly; views of two sizes in one call
at both pixel offsets; grouping; the scratch fill."""
import importlib

import numpy as np
import pytest

import scene_reference as R

pytestmark = pytest.mark.gpu
tp = importlib.import_module("teaser-plusplus_amd")

RAY_KEYS = ("t_hit", "geometry_ids", "primitive_ids", "primitive_uvs", "primitive_normals")
POINT_KEYS = ("distance", "points", "geometry_ids", "primitive_ids", "primitive_uvs", "primitive_normals")


@pytest.fixture(autouse=True)
def needs_gpu():
    if tp.device_count() < 1:
        pytest.fail("the GPU suite needs an MI355X")


def scene_of(geoms):
    s = tp.RaycastingScene()
    for k, (vert, tri) in enumerate(geoms):
        assert s.add_triangles(vert, tri) == k
    return s


def equal(got, ref, keys, what):
    for k in keys:
        g, r = np.asarray(got[k]), np.asarray(ref[k]).reshape(np.asarray(got[k]).shape)
        assert g.dtype == r.dtype, (what, k, g.dtype, r.dtype)
        bad = np.flatnonzero((g.view(np.uint32) != r.view(np.uint32)).reshape(len(g), -1).any(axis=1)) if g.size else []
        assert len(bad) == 0, (what, k, len(bad), bad[:5], g[bad[:3]], r[bad[:3]])


@pytest.mark.parametrize("name", list(R.cases()))
def test_rays_and_points_equal_the_restatement(name):
    geoms, rays, pts, _ = R.cases()[name]
    hit, near = R.expected(name)
    if name not in ("small0",):
        assert np.isfinite(hit["t_hit"]).any() and np.isfinite(near["distance"]).any(), name
    if name not in ("small0", "duplicates", "line"):
        assert np.isinf(hit["t_hit"]).any(), name
    with scene_of(geoms) as s:
        assert s.triangle_count() == sum(len(t) for _, t in geoms)
        equal(s.cast_rays(rays), hit, RAY_KEYS, name)
        equal(s.compute_closest_points(pts), near, POINT_KEYS, name)
        assert s.compute_distance(pts).tobytes() == near["distance"].tobytes()


def test_the_cases_are_what_they_say():
    hit, near = R.expected("lattice")
    geoms, rays, pts, _ = R.cases()["lattice"]
    T = R.Triangles(geoms)
    h, t, _, _ = R._ray_pairs(T, rays)
    ties = (h & (t == np.where(h, t, np.inf).min(axis=1, keepdims=True))).sum(axis=1)
    assert ties.max() == 6 and (ties == 2).any()                              # six triangles share a lattice vertex
    assert (hit["t_hit"] == 0).sum() >= 5 and np.isinf(hit["t_hit"][-16:-8]).sum() >= 4    # on the sheet; in its plane
    assert (near["distance"] == 0).sum() >= 81 and near["distance"].max() > 7e4
    d = R.expected("dead")
    dead = np.flatnonzero(R.Triangles(R.cases()["dead"][0]).dead)
    assert len(dead) >= 5 and not np.isin(d[0]["primitive_ids"], dead).any() and not np.isin(d[1]["primitive_ids"], dead).any()
    dup = R.expected("duplicates")
    assert (dup[0]["primitive_ids"][np.isfinite(dup[0]["t_hit"])] == 0).all() and (dup[1]["primitive_ids"] == 0).all()
    g = R.Triangles(R.cases()["axis_aligned"][0])
    assert ((g.v0 == g.v1) & (g.v1 == g.v2)).any(axis=1).all()                  # every box has zero thickness


@pytest.mark.parametrize("count", [0, 1, 63, 64, 65, 257])
def test_ray_counts(count):
    geoms, rays, pts, _ = R.cases()["small3"]
    hit, near = R.expected("small3")
    with scene_of(geoms) as s:
        got = s.cast_rays(rays[:count])
        equal(got, {k: v[:count] for k, v in hit.items()}, RAY_KEYS, count)
        assert got["t_hit"].shape == (count,) and got["primitive_normals"].shape == (count, 3)
        n = min(count, len(pts))
        equal(s.compute_closest_points(pts[:n]), {k: v[:n] for k, v in near.items()}, POINT_KEYS, count)
        assert s.test_occlusions(rays[:count]).shape == (count,)


def test_geometries_added_in_several_calls_and_a_rebuild():
    geoms, rays, pts, _ = R.cases()["two_geometries"]
    with tp.RaycastingScene() as s:
        assert s.add_triangles(*geoms[0]) == 0 and s.add_triangles(*geoms[1]) == 1
        s.commit()
        two = geoms[:2]
        equal(s.cast_rays(rays), R.cast_rays(two, rays), RAY_KEYS, "two")
        equal(s.compute_closest_points(pts), R.closest_points(two, pts), POINT_KEYS, "two")
        assert s.add_triangles(*geoms[2]) == 2 and s.triangle_count() == 110
        hit, near = R.expected("two_geometries")
        got = s.cast_rays(rays)  # builds first
        equal(got, hit, RAY_KEYS, "three")
        equal(s.compute_closest_points(pts), near, POINT_KEYS, "three")
        assert set(np.unique(got["geometry_ids"])) == {0, 2, 0xFFFFFFFF} and got["primitive_ids"][got["geometry_ids"] == 2].max() < 70


@pytest.mark.parametrize("name", ["lattice", "random", "axis_aligned", "mixed_sizes"])
def test_occlusions(name):
    geoms, rays, _, _ = R.cases()[name]
    t = R.expected(name)[0]["t_hit"]
    T = R.Triangles(geoms)
    f = np.sort(t[np.isfinite(t)])
    with scene_of(geoms) as s:
        assert np.array_equal(s.test_occlusions(rays), np.isfinite(t))
        for tnear, tfar in ((float(f[len(f) // 2]), np.inf), (0.0, float(f[len(f) // 2])), (float(f[len(f) // 4]), float(f[3 * len(f) // 4])),
                            (float(f[-1]), float(f[-1])), (2.0, 1.0), (-np.inf, np.inf)):
            ref = R.test_occlusions(T, rays, tnear, tfar).astype(bool)
            assert np.array_equal(s.test_occlusions(rays, tnear, tfar), ref), (name, tnear, tfar)
        if name == "lattice":  # tnear == t exactly: t = 5 for the rays through the lattice vertices
            assert (t[:81] == 5.0).all() and s.test_occlusions(rays[:81], 5.0, 5.0).all()
            assert not s.test_occlusions(rays[:81], np.nextafter(5.0, 6.0), 9.0).any()
        with pytest.raises(tp.TeaserHipError, match="tnear must not be NaN"):
            s.test_occlusions(rays, float("nan"), 1.0)


@pytest.mark.parametrize("name", ["lattice", "random"])
def test_views_equal_cast_rays_on_the_pinhole_rays(name):
    geoms = R.cases()[name][0]
    T = R.Triangles(geoms)
    views = R.views_case()
    with scene_of(geoms) as s:
        for off in (0.5, 0.0):
            got = s.cast_views([K for K, _, _, _ in views], [E for _, E, _, _ in views], [w for _, _, w, _ in views],
                               [h for _, _, _, h in views], pixel_offset=off)
            for b, (K, E, w, h) in enumerate(views):
                rays = tp.create_rays_pinhole(K, E, w, h, off)
                assert rays.tobytes() == R.create_rays_pinhole(K, E, w, h, off).tobytes() and rays.shape == (h, w, 6)
                equal(got[b], s.cast_rays(rays), RAY_KEYS, (name, off, b))
                equal({k: v.reshape((h * w,) + v.shape[2:]) for k, v in got[b].items()}, R.cast_rays(T, rays.reshape(-1, 6)), RAY_KEYS,
                      (name, off, b, "restatement"))
            assert got[2]["t_hit"].shape == (0, 0)
            if name == "lattice":
                assert np.isfinite(got[1]["t_hit"]).any() and np.isinf(got[1]["t_hit"]).any()
        some = s.cast_views(views[1][0], [views[1][1], views[0][1]], 64, 48, ids=False, normals=False)  # only some maps
        assert sorted(some[0]) == ["primitive_uvs", "t_hit"]
        full = s.cast_views(views[1][0], [views[1][1], views[0][1]], 64, 48)
        for b in range(2):
            equal(some[b], full[b], ("t_hit", "primitive_uvs"), "some maps")
        depth = s.render_depth(tp.PinholeCameraIntrinsic(64, 48, 40.0, 42.0, 31.5, 23.5), views[1][1], depth_max=1e9)
        t = s.cast_views(views[1][0], [views[1][1]], 64, 48, pixel_offset=0.0)[0]["t_hit"]
        assert depth.dtype == np.float32 and np.array_equal(depth, np.where(np.isfinite(t), t, np.float32(0)))


def test_grouping_and_scratch_do_not_change_a_bit():
    geoms, rays, pts, _ = R.cases()["random"]
    hit, near = R.expected("random")
    with scene_of(geoms) as s:
        whole = s.cast_rays(rays)
        assert s.fill_scratch(0xA5) > 0
        parts = [s.cast_rays(rays[a:a + 1000]) for a in range(0, len(rays), 1000)]
        equal({k: np.concatenate([p[k] for p in parts]) for k in RAY_KEYS}, whole, RAY_KEYS, "chunks")
        s.fill_scratch(0x5A)
        back = s.cast_rays(rays[::-1])
        equal({k: v[::-1] for k, v in back.items()}, whole, RAY_KEYS, "reversed")
        equal(whole, hit, RAY_KEYS, "restatement")
        s.fill_scratch(0xA5)
        equal(s.compute_closest_points(pts[::-1]), {k: v[::-1] for k, v in near.items()}, POINT_KEYS, "points reversed")
        shaped = s.cast_rays(rays[:4000].reshape(40, 100, 6))
        assert shaped["t_hit"].shape == (40, 100) and shaped["primitive_uvs"].shape == (40, 100, 2)


def test_refusals_leave_the_scene_usable():
    vert, tri = R.sheet(3)
    with tp.RaycastingScene() as s:
        bad = vert.copy()
        bad[2, 1] = np.inf
        with pytest.raises(tp.TeaserHipError, match=r"non-finite entry \(vertex 2\)"):
            s.add_triangles(bad, tri)
        with pytest.raises(tp.TeaserHipError, match=r"index >= n_vertices \(triangle 0\)"):
            s.add_triangles(vert[:4], tri)
        assert s.triangle_count() == 0 and np.isinf(s.cast_rays(np.array([[1, 1, 1, 0, 0, -1.0]]))["t_hit"]).all()
        assert s.add_triangles(vert, tri) == 0
        assert s.cast_rays(np.array([[1.25, 0.5, 1, 0, 0, -1.0]]))["t_hit"][0] == 1.0
        assert s.add_triangles(np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int64)) == 1  # an empty mesh is a geometry
