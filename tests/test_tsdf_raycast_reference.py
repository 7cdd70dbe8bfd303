"""The restatement of the ray cast (tests/tsdf_raycast_reference.py) pinned by hand: a volume of two voxels a side with
voxels of length 1 and a truncation of 1.5, cameras whose rays are small exact numbers, and every t0, t1, sample, step
size and t* worked out here in the comments and asserted.  Then the rules one by one -- the slab test of an axis the ray
does not move along, the weight threshold at and just below a voxel's weight, a first sample that is negative, a surface
met from unobserved space, a sample outside the volume after the clip, the colour rule with a corner that does not count
and with none that does, a missed pixel -- and a sanity case against geometry."""
import numpy as np

import tsdf_mesh_reference as M
import tsdf_raycast_reference as RC
import tsdf_reference as T

f32 = np.float32


def volume(values, weights=None, color_type=T.NONE):
    """R = 2, vl = 1, trunc = 1.5, origin 0; values: {(x, y, z): tsdf}; every weight 3 unless given."""
    vol = T.Volume(2.0, 2, 1.5, color_type)
    vol.weight[:] = f32(3)
    for at, f in values.items():
        vol.tsdf[at] = f32(f)
    for at, w in (weights or {}).items():
        vol.weight[at] = f32(w)
    return vol


def one_ray(vol, o, d, wthr=3.0, dmin=0.1, dmax=10.0):
    """(t0, t1, ok, hit, t, t_prev, f, f_prev, steps, the samples as (t, voxel or None)) of one ray."""
    o, d = np.array(o, dtype=f32), np.array([d], dtype=f32)
    t0, t1, ok = RC.clip(o, d, f32(vol.length), f32(dmin), f32(dmax))
    trace = []
    hit, t, t_prev, f, f_prev, steps = RC.march(vol, o, d, t0, t1, ok, f32(wthr), trace)
    samples = [(float(ts[0]), tuple(int(x) for x in q[0]) if inside[0] else None) for ts, q, inside, active in trace if active[0]]
    return (float(t0[0]), float(t1[0]), bool(ok[0]), bool(hit[0]), float(t[0]), float(t_prev[0]), float(f[0]), float(f_prev[0]),
            int(steps[0]), samples)


O, Z = (0.5, 0.5, -1.0), (0.0, 0.0, 1.0)  # a camera one voxel in front of the volume looking along z through column (0, 0)


def test_a_ray_along_z_by_hand():
    # z slab: lo = (0 - -1) / 1 = 1, hi = (2 - -1) / 1 = 3; x and y do not move and 0.5 lies in [0, 2): t0 = 1, t1 = 3.
    # t = 1: p = (.5, .5, 0), voxel (0, 0, 0), f = .5: no hit (f_prev = -1); delta = .5 * 1.5 = .75 < vl: the step is vl = 1.
    # t = 2: p_z = 1, voxel (0, 0, 1), f = -.25, w = 3 >= 3, f_prev = .5 > 0: HIT.
    # t* = (2 * .5 - 1 * -.25) / (.5 - -.25) = 1.25 / .75
    vol = volume({(0, 0, 0): 0.5, (0, 0, 1): -0.25})
    t0, t1, ok, hit, t, t_prev, f, f_prev, steps, samples = one_ray(vol, O, Z)
    assert (t0, t1, ok, hit) == (1.0, 3.0, True, True)
    assert samples == [(1.0, (0, 0, 0)), (2.0, (0, 0, 1))] and steps == 2
    assert (t, t_prev, f, f_prev) == (2.0, 1.0, -0.25, 0.5)
    # a value of 1: delta = 1.5 > vl, the step is 1.5; t = 2.5 samples p_z = 1.5, still voxel (0, 0, 1)
    # t* = (2.5 * 1 - 1 * -.25) / 1.25 = 2.75 / 1.25
    vol = volume({(0, 0, 0): 1.0, (0, 0, 1): -0.25})
    t0, t1, ok, hit, t, t_prev, f, f_prev, steps, samples = one_ray(vol, O, Z)
    assert hit and samples == [(1.0, (0, 0, 0)), (2.5, (0, 0, 1))] and (t, t_prev, f, f_prev) == (2.5, 1.0, -0.25, 1.0)


def test_the_whole_call_by_hand():
    """The camera of the ray above as an extrinsic, a 3 x 2 view with fx = fy = 1 and the principal point on pixel (0, 0):
    pixel (0, 0) is the ray above, pixel (0, 1) has d = (1, 0, 1), pixel (0, 2) has d = (2, 0, 1)."""
    vol = volume({(0, 0, 0): 0.5, (0, 0, 1): -0.25, (1, 0, 0): 0.5, (1, 0, 1): 0.5}, color_type=T.RGB8)
    vol.color[:] = 51.0
    vol.origin[:] = (10.0, 20.0, 30.0)  # the volume moved: the camera moves with it
    E = np.eye(4)
    E[:3, 3] = -(np.array(O) + vol.origin)
    o, Rt = RC.camera(vol, E)
    assert o.tolist() == [0.5, 0.5, -1.0] and Rt.tolist() == np.eye(3).tolist()
    d = RC.rays((1.0, 1.0, 0.0, 0.0), Rt, 3, 2)
    assert d[0, 0].tolist() == [0, 0, 1] and d[0, 1].tolist() == [1, 0, 1] and d[0, 2].tolist() == [2, 0, 1] and d[1, 0].tolist() == [0, 1, 1]
    r = RC.ray_cast(vol, (1.0, 1.0, 0.0, 0.0), E, 3, 2, 0.1, 10.0, 3.0)
    ts = f32(1.25) / f32(0.75)
    assert r.depth[0, 0] == ts and r.hits == int(r.hit.sum()) and r.hit[0, 0]
    q = np.array([0.5, 0.5, -1.0 + float(ts)])
    assert r.vertex[0, 0].tolist() == (q + vol.origin).astype(f32).tolist()
    # the normal is the point cloud's rule at q, the colour that of eight equal corners
    g = 0.99 * vol.vl
    n = np.array([vol.trilinear((q + g * e)[None])[0] - vol.trilinear((q - g * e)[None])[0] for e in np.eye(3)])
    n = n / np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
    assert r.normal[0, 0].tolist() == n.astype(f32).tolist() and n[2] < 0  # the surface faces the camera
    assert r.color[0, 0].tolist() == [f32(51.0 / 255.0)] * 3
    # pixel (0, 1), d = (1, 0, 1): x slab lo = -.5, hi = 1.5; z slab lo = 1, hi = 3: t0 = 1, t1 = 1.5.
    # t = 1: p = (1.5, .5, 0), voxel (1, 0, 0), f = .5, the step is 1; t = 2 > t1: MISS -- all outputs 0
    assert not r.hit[0, 1] and r.steps[0, 1] == 1
    for m in (r.depth, r.vertex, r.normal, r.color):
        assert not m[0, 1].any()
    # pixel (0, 2), d = (2, 0, 1): x slab hi = .75 < the z slab's lo = 1: t0 = 1 > t1 = .75, no sample at all
    assert not r.hit[0, 2] and r.steps[0, 2] == 0


def test_an_axis_the_ray_does_not_move_along():
    vol = volume({(0, 0, 0): 0.5, (0, 0, 1): -0.25})
    assert one_ray(vol, O, Z)[2:4] == (True, True)                       # inside the slab
    assert one_ray(vol, (-0.5, 0.5, -1.0), Z)[2:4] == (False, False)     # outside it: a miss without a sample
    assert one_ray(vol, (-0.5, 0.5, -1.0), Z)[8] == 0
    assert one_ray(vol, (2.0, 0.5, -1.0), Z)[2] is False                 # o_k = L is outside [0, L)
    assert one_ray(vol, (0.0, 0.5, -1.0), Z)[2] is True                  # o_k = 0 is inside
    # the same start with a ray that does move along x comes in: d = (1, 0, 1), x slab lo = .5, hi = 2.5, z slab 1 .. 3
    t0, t1, ok, hit, *_ = one_ray(vol, (-0.5, 0.5, -1.0), (1.0, 0.0, 1.0))
    assert (t0, t1, ok) == (1.0, 2.5, True)


def test_cameras_outside_inside_and_past_the_box():
    vol = volume({(0, 0, 0): 0.5, (0, 0, 1): -0.25})
    assert one_ray(vol, O, Z)[:2] == (1.0, 3.0)                                         # outside: t0 is the box's face
    t0, t1, ok, hit, t, t_prev, f, f_prev, steps, samples = one_ray(vol, (0.5, 0.5, 0.25), Z, dmin=0.125)
    # inside: lo = -.25 < depth_min: t0 = .125, t1 = 1.75; t = .125: p_z = .375, voxel (0, 0, 0); t = 1.125: p_z = 1.375: HIT
    assert (t0, t1, hit) == (0.125, 1.75, True) and samples == [(0.125, (0, 0, 0)), (1.125, (0, 0, 1))]
    # past the box: d = (5, 0, 1) from O: x slab lo = -.1, hi = .3; z slab lo = 1: t0 = 1 > t1 = .3
    t0, t1, ok, hit, *_, steps, samples = one_ray(vol, O, (5.0, 0.0, 1.0))
    assert (t0, float(f32(t1)), ok, hit, steps) == (1.0, float(f32(1.5) / f32(5.0)), True, False, 0)
    # depth_max in front of the box, and depth_min behind the surface
    assert one_ray(vol, O, Z, dmax=0.5)[3] is False and one_ray(vol, O, Z, dmax=0.5)[8] == 0
    assert one_ray(vol, O, Z, dmin=2.0)[3] is False  # starts in the negative voxel: f_prev = -1


def test_the_weight_threshold():
    below = float(np.nextafter(f32(3), f32(0)))
    assert one_ray(volume({(0, 0, 0): 0.5, (0, 0, 1): -0.25}, {(0, 0, 1): 3.0}), O, Z)[3] is True      # exactly at it
    assert one_ray(volume({(0, 0, 0): 0.5, (0, 0, 1): -0.25}, {(0, 0, 1): below}), O, Z)[3] is False   # just below
    assert one_ray(volume({(0, 0, 0): 0.5, (0, 0, 1): -0.25}, {(0, 0, 1): below}), O, Z, wthr=below)[3] is True
    # the weight of the positive voxel in front does not matter
    assert one_ray(volume({(0, 0, 0): 0.5, (0, 0, 1): -0.25}, {(0, 0, 0): 1.0}), O, Z)[3] is True


def test_no_hit_from_behind_or_from_unobserved_space():
    # the first sample is negative: f_prev = -1, and then f_prev = -.5: no hit; t = 1, 2, 3 are sampled, t = 4 > t1
    t0, t1, ok, hit, *_, steps, samples = one_ray(volume({(0, 0, 0): -0.5, (0, 0, 1): -0.25}), O, Z)
    assert not hit and [s[0] for s in samples] == [1.0, 2.0, 3.0]
    # an unobserved voxel (f = 0, w = 0) in front of a negative one: f_prev = 0 is not > 0
    assert one_ray(volume({(0, 0, 0): 0.0, (0, 0, 1): -0.25}, {(0, 0, 0): 0.0}), O, Z)[3] is False
    # ... and a zero of an observed voxel is a hit after a positive one: f <= 0
    assert one_ray(volume({(0, 0, 0): 0.5, (0, 0, 1): 0.0}), O, Z)[3] is True
    assert one_ray(volume({(0, 0, 0): 0.5, (0, 0, 1): -0.0}), O, Z)[3] is True


def test_a_sample_outside_the_volume_after_the_clip():
    # both voxels positive: t = 1, 2, then t = 3 = t1 passes step 1 and samples p_z = 2.0: q_z = 2 = R is outside, f = w = 0
    vol = volume({(0, 0, 0): 0.5, (0, 0, 1): 0.5})
    t0, t1, ok, hit, *_, steps, samples = one_ray(vol, O, Z)
    assert not hit and samples == [(1.0, (0, 0, 0)), (2.0, (0, 0, 1)), (3.0, None)]
    # with the threshold 0 that sample ends the ray: f_prev = .5 > 0, 0 >= 0, 0 <= 0; t* = (3 * .5 - 2 * 0) / .5 = 3
    t0, t1, ok, hit, t, t_prev, f, f_prev, steps, samples = one_ray(vol, O, Z, wthr=0.0)
    assert hit and (t, t_prev, f, f_prev) == (3.0, 2.0, 0.0, 0.5) and samples[-1] == (3.0, None)
    r = RC.ray_cast(vol, (1.0, 1.0, 0.0, 0.0), np.array([[1, 0, 0, -0.5], [0, 1, 0, -0.5], [0, 0, 1, 1.0], [0, 0, 0, 1.0]]), 1, 1, 0.1, 10.0, 0.0)
    assert r.hits == 1 and r.depth[0, 0] == 3.0 and r.vertex[0, 0].tolist() == [0.5, 0.5, 2.0]


def test_the_colour_rule():
    vol = volume({}, color_type=T.RGB8)
    for x in range(2):
        for y in range(2):
            for z in range(2):
                vol.color[x, y, z] = 8.0 * (4 * x + 2 * y + z)
    q = np.array([[1.0, 1.0, 1.0]])  # a = .5: idx = 0, r = .5: every corner inside with omega = .125
    assert RC.color_at(vol, q)[0].tolist() == [(8.0 * 28 / 8) / 255.0] * 3
    vol.weight[1, 1, 1] = 0  # corner 111 no longer counts: num = .125 * 8 * 21 = 21, den = .875: 24
    assert RC.color_at(vol, q)[0].tolist() == [24.0 / 255.0] * 3
    # at the volume's corner only voxel (0, 0, 0) is inside: q = .25: a = -.25, idx = -1, r = .75
    vol.color[0, 0, 0] = 100.0
    assert RC.color_at(vol, np.array([[0.25, 0.25, 0.25]]))[0].tolist() == [100.0 / 255.0] * 3
    vol.weight[:] = 0  # no corner counts
    assert RC.color_at(vol, q)[0].tolist() == [0.0, 0.0, 0.0]
    gray = volume({}, color_type=T.GRAY32)
    gray.color[:] = 0.5
    gray.color[1, 1, 1] = np.nan
    c = RC.to_f32(RC.color_at(gray, q))
    assert c.view(np.uint32).tolist() == [[0x7fc00000] * 3]  # THE quiet NaN; no division by 255
    gray.weight[1, 1, 1] = 0
    assert RC.color_at(gray, q)[0].tolist() == [0.5] * 3


def test_a_sphere_seen_from_inside_the_volume():
    """Geometry: the analytic sphere of tsdf_mesh_reference.sphere_volume at R = 64 with a radius of 10 voxels (truncation
    3 voxels, every weight 1), an 80 x 60 view from (0.5, 0.5, 0.05) inside the volume along z, threshold 1.  Measured on
    this restatement: 2272 hits; all 1288 pixels whose analytic ray passes at least two voxels inside the silhouette hit,
    with a depth error of at most 0.7232584717505226 voxel (median 0.32); over all hits whose analytic ray meets the
    sphere the error is at most 1.8156670747688537 voxels (grazing rays); no pixel whose ray passes more than a voxel
    outside the silhouette hits; at most 27 steps per ray.  The assertions are those maxima plus 0.05 and 0.1 voxel."""
    R, radius, w, h = 64, 10.0, 80, 60
    vol = M.sphere_volume(R, radius)
    K = T.camera(w, h)
    c = np.array([0.5, 0.5, 0.05])
    E = np.eye(4)
    E[:3, 3] = -c
    r = RC.ray_cast(vol, K, E, w, h, 0.01, 3.0, 1.0)
    i, j = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    d = np.stack([(j - K[2]) / K[0], (i - K[3]) / K[1], np.ones_like(i)], axis=2)
    oc = c - 0.5
    A, B, C0 = (d * d).sum(axis=2), 2.0 * (d @ oc), oc @ oc - (radius * vol.vl) ** 2
    disc = B * B - 4.0 * A * C0
    t = (-B - np.sqrt(np.maximum(disc, 0.0))) / (2.0 * A)  # d_z = 1: t is the z-depth
    dist = np.linalg.norm(np.cross(d, np.broadcast_to(-oc, d.shape)), axis=2) / np.sqrt(A)
    inner, outer = dist <= (radius - 2.0) * vol.vl, dist > (radius + 1.0) * vol.vl
    err = np.abs(r.depth.astype(np.float64) - t) / vol.vl
    print("hits", r.hits, "inner", int(inner.sum()), "inner max", err[inner].max(), "all max", err[r.hit & (disc > 0)].max(), "steps", r.steps.max())
    assert inner.sum() > 1000 and r.hit[inner].all() and not r.hit[outer].any() and 0 < r.hits < w * h
    assert err[inner].max() <= 0.7232584717505226 + 0.05
    assert err[r.hit & (disc > 0)].max() <= 1.8156670747688537 + 0.1
    assert r.steps.max() < np.sqrt(3.0) * R + 1
    # the normals of the inner pixels point from the centre to the vertex, against the ray
    v = r.vertex[inner].astype(np.float64) - 0.5
    cosine = (r.normal[inner].astype(np.float64) * v).sum(axis=1) / np.linalg.norm(v, axis=1)
    assert cosine.min() > 0.99
