"""The restatement of the scalable volume's ray cast (tests/stsdf_raycast_reference.py) pinned by hand and against two
independent references.  By hand: voxels of 1/16, blocks of side 1 and a truncation of 1/4, so that every t, t_exit and
t* is a short binary fraction, worked out in the comments and asserted.  Against the dense restatement
(tests/tsdf_raycast_reference.py): eight open blocks that hold a dense volume, cameras inside the box.  Against
geometry: an analytic sphere stored only in the blocks near its surface."""
import numpy as np
import pytest

import stsdf_raycast_reference as SR
import tsdf_raycast_reference as RC
import tsdf_reference as T

f32 = np.float32
U = SR.U
VL, TRUNC = 1.0 / 16.0, 0.25
C = 0.53125  # the centre of voxel 8 of block 0: the rays below run along a row of voxel centres


def plane_block(axis, surface, side):
    """The tsdf of a block whose surface is the plane coordinate[axis] = surface (local, in [0, 1]); side = +1: the free
    space (positive values) lies below the plane.  clamp(side (surface - centre) / trunc): exact in float32 for these."""
    c = (np.arange(U) + 0.5) * VL
    f = np.clip(side * (surface - c) / TRUNC, -1.0, 1.0).astype(f32)
    shape = [1, 1, 1]
    shape[axis] = U
    return np.broadcast_to(f.reshape(shape), (U, U, U)).copy()


def volume(blocks, weight=5.0, color_type=T.NONE):
    """blocks: key -> tsdf array; every weight `weight`."""
    return SR.volume_of_blocks(VL, TRUNC, color_type, {b: (f, np.full((U, U, U), weight, dtype=f32), None) for b, f in blocks.items()})


def one_ray(vol, o, d, wthr=3.0, dmin=0.0625, dmax=10.0, n_cap=None, skip=True):
    """(hit, t, t_prev, f, f_prev, the steps as (t, block, open, t_exit or None)) of one ray."""
    trace = []
    cap = n_cap if n_cap is not None else SR.step_cap(vol, dmin, dmax)
    hit, t, t_prev, f, f_prev, steps = SR.march(vol, np.array(o, dtype=f32), np.array([d], dtype=f32), dmin, dmax, wthr, cap, skip, trace)
    rows = [(float(s.t[0]), tuple(int(x) for x in s.B[0]), bool(s.open[0]), None if s.open[0] or np.isnan(s.t_exit[0]) else float(s.t_exit[0]))
            for s in trace if s.active[0]]
    assert len(rows) == steps[0]
    return bool(hit[0]), float(t[0]), float(t_prev[0]), float(f[0]), float(f_prev[0]), rows


def t_star(t, t_prev, f, f_prev):
    return float((f32(t) * f32(f_prev) - f32(t_prev) * f32(f)) / (f32(f_prev) - f32(f)))


# voxel z: 0..3 -> 1, 4 -> .875, 5 -> .625, 6 -> .375, 7 -> .125, 8 -> -.125, 9 -> -.375, ...: the plane z = .5 seen from below
PLANE_Z = {(0, 0, 0): plane_block(2, 0.5, +1)}


def test_one_open_block_with_a_plane_through_it():
    # o = (C, C, 0), d = (0, 0, 1), t0 = 1/32.
    # t = .03125: g_z = floor(.5) = 0, f = 1, f_prev = -1: no hit; delta = 1 * .25: t = .28125
    # t = .28125: g_z = floor(4.5) = 4, f = .875: no hit; delta = .21875: t = .5
    # t = .5: g_z = 8, f = -.125, w = 5 >= 3, f_prev = .875: HIT.  t* = (.5 * .875 + .28125 * .125) / 1 = .47265625
    vol = volume(PLANE_Z)
    assert vol.blocks[(0, 0, 0)].tsdf[3, 3, 4] == f32(0.875) and vol.blocks[(0, 0, 0)].tsdf[0, 0, 8] == f32(-0.125)
    hit, t, t_prev, f, f_prev, rows = one_ray(vol, (C, C, 0.0), (0, 0, 1), dmin=0.03125)
    assert hit and rows == [(0.03125, (0, 0, 0), True, None), (0.28125, (0, 0, 0), True, None), (0.5, (0, 0, 0), True, None)]
    assert (t, t_prev, f, f_prev) == (0.5, 0.28125, -0.125, 0.875) and t_star(t, t_prev, f, f_prev) == 0.47265625


def test_the_weight_threshold_at_and_just_below_a_weight():
    vol = volume(PLANE_Z)
    assert one_ray(vol, (C, C, 0.0), (0, 0, 1), wthr=5.0, dmin=0.03125)[0]
    above = float(np.nextafter(f32(5), f32(6)))
    hit, _, _, _, _, rows = one_ray(vol, (C, C, 0.0), (0, 0, 1), wthr=above, dmin=0.03125, dmax=2.0)
    # the crossing at t = .5 is passed (f_prev becomes -.125) and nothing behind it is a hit; the ray leaves the block at
    # t = 1 and skips block (0, 0, 1) whole: t_exit = (2 - 0) / 1 = 2, the last sample
    assert not hit and rows[2] == (0.5, (0, 0, 0), True, None) and rows[-1][1:] == ((0, 0, 2), False, 3.0) and rows[-2] == (1.0, (0, 0, 1), False, 2.0)


def test_from_an_absent_block_along_plus_x_with_negative_indices():
    # The block (-2, 0, 0) = [-2, -1) with the plane x = -1.5 seen from -x; o = (-3.5, C, C), d = (1, 0, 0): two d_k are 0,
    # so t_exit is the x face alone.
    # t = .0625: p_x = -3.4375, g = -55, B = floor(-55 / 16) = -4 (l = 9): absent.  face = -3, t_exit = .5 > .125: t = .5
    # t = .5: p_x = -3, g = -48, B = -3 (l = 0): absent; the landing is exactly on the face.  face = -2, t_exit = 1.5: t = 1.5
    # t = 1.5: p_x = -2, g = -32, B = -2, l = 0: open, f = 1, f_prev = 0: no hit; t = 1.75
    # t = 1.75: g = -28, l = 4, f = .875; t = 1.96875
    # t = 1.96875: p_x = -1.53125, g = floor(-24.5) = -25, l = 7, f = .125; delta < vl: t = 2.03125
    # t = 2.03125: p_x = -1.46875, g = -24, l = 8, f = -.125: HIT.  t* = (2.03125 * .125 + 1.96875 * .125) / .25 = 2
    vol = volume({(-2, 0, 0): plane_block(0, 0.5, +1)})
    hit, t, t_prev, f, f_prev, rows = one_ray(vol, (-3.5, C, C), (1, 0, 0))
    assert hit and rows == [(0.0625, (-4, 0, 0), False, 0.5), (0.5, (-3, 0, 0), False, 1.5), (1.5, (-2, 0, 0), True, None),
                            (1.75, (-2, 0, 0), True, None), (1.96875, (-2, 0, 0), True, None), (2.03125, (-2, 0, 0), True, None)]
    assert (t, t_prev, f, f_prev) == (2.03125, 1.96875, -0.125, 0.125) and t_star(t, t_prev, f, f_prev) == 2.0


def test_along_minus_x_a_landing_on_a_face_takes_one_more_voxel():
    # The same block with the plane seen from +x: voxel 7 -> -.125, 8 -> .125, 9 -> .375, 10 -> .625, 11 -> .875, 12.. -> 1.
    # o = (.5, C, C), d = (-1, 0, 0).
    # t = .0625: p_x = .4375, g = 7, B = 0: absent.  d_x < 0: face = B ul = 0, t_exit = (0 - .5) / -1 = .5: t = .5
    # t = .5: p_x = 0, g = 0, B = 0 still: the ray lies ON the face it left by.  t_exit = .5 is not > t_next = .5625: t = .5625
    # t = .5625: p_x = -.0625, g = -1, B = -1 (l = 15): absent.  face = -1, t_exit = 1.5: t = 1.5
    # t = 1.5: p_x = -1, g = -16, B = -1 (l = 0): absent; again one voxel more: t = 1.5625
    # t = 1.5625: g = -17, B = -2, l = 15: open, f = 1, f_prev = 0: no hit; t = 1.8125
    # t = 1.8125: p_x = -1.3125, g = -21, l = 11, f = .875; t = 2.03125
    # t = 2.03125: p_x = -1.53125, g = -25, l = 7, f = -.125: HIT.  t* = 2.03125 * .875 + 1.8125 * .125 = 2.00390625
    vol = volume({(-2, 0, 0): plane_block(0, 0.5, -1)})
    hit, t, t_prev, f, f_prev, rows = one_ray(vol, (0.5, C, C), (-1, 0, 0))
    assert hit and rows == [(0.0625, (0, 0, 0), False, 0.5), (0.5, (0, 0, 0), False, 0.5), (0.5625, (-1, 0, 0), False, 1.5),
                            (1.5, (-1, 0, 0), False, 1.5), (1.5625, (-2, 0, 0), True, None), (1.8125, (-2, 0, 0), True, None),
                            (2.03125, (-2, 0, 0), True, None)]
    assert (t, t_prev, f, f_prev) == (2.03125, 1.8125, -0.125, 0.875) and t_star(t, t_prev, f, f_prev) == 2.00390625
    # without the skip the same hit, after 1.5 / vl steps more
    assert one_ray(vol, (0.5, C, C), (-1, 0, 0), skip=False)[:5] == (hit, t, t_prev, f, f_prev)


def test_a_landing_that_rounds_short_of_the_face():
    # The block (0, 0, 0) with the plane x = .5 seen from -x; o_x = fl(-0.21) = -0x1.ae147ap-3, d = (fl(0.7), 0, 0) with
    # fl(0.7) = 0x1.666666p-1.  Block (-1, 0, 0) is not open; its exit face is x = 0.
    # t = .0625: p_x = -.16625, g = -3, B = -1: absent.  t_exit = fl(0.21f / 0.7f) = 0x1.333332p-2 = .29999998 (one ulp
    #   below 0.3) > t_next = .125: t = .29999998
    # t = .29999998: p_x = fl(o + t d) = -2^-26 < 0, SHORT of the face: g = -1, B = -1 again, absent.  t_exit is the same
    #   number and not > t_next = fl(.29999998 + .0625) = 0x1.733332p-2 = .36249998: t = .36249998, one voxel more
    # t = .36249998: p_x = .04375, g = 0: block (0, 0, 0), open, voxel 0, f = 1, f_prev = 0: no hit; then steps of
    #   max(vl, f trunc) through voxels 3 (f = 1), 6 (.375) and 7 (.125) to voxel 8 (f = -.125): HIT near x = .5
    vol = volume({(0, 0, 0): plane_block(0, 0.5, +1)})
    o, d = (f32(-0.21), f32(C), f32(C)), (f32(0.7), 0, 0)
    e, t2 = float.fromhex("0x1.333332p-2"), float.fromhex("0x1.733332p-2")
    assert float((f32(0) - o[0]) / d[0]) == e and float(o[0] + f32(e) * d[0]) == -(2.0 ** -26) and float(f32(e) + f32(VL)) == t2
    hit, t, t_prev, f, f_prev, rows = one_ray(vol, o, d)
    assert rows[:3] == [(0.0625, (-1, 0, 0), False, e), (e, (-1, 0, 0), False, e), (t2, (0, 0, 0), True, None)]
    assert hit and len(rows) == 7 and all(r[1:] == ((0, 0, 0), True, None) for r in rows[2:])
    x = [float(o[0] + f32(r[0]) * d[0]) for r in rows[2:]]  # the samples in the open block: voxels 0, 3, 6, 7, 8
    assert [int(np.floor(v / VL)) for v in x] == [0, 3, 6, 7, 8]
    assert (f, f_prev) == (-0.125, 0.125) and t == rows[6][0] and t_prev == rows[5][0]
    assert abs(float(o[0]) + t_star(t, t_prev, f, f_prev) * float(d[0]) - 0.5) < 0.5 * VL
    # without the skip the ray walks block -1 a voxel at a time and meets the same surface
    assert one_ray(vol, o, d, skip=False)[0]


def test_a_ray_through_a_block_corner():
    # o = (-.5, -.5, -.5), d = (1, 1, 1): t = .0625 lies in block (-1, -1, -1); the three faces give t_exit = .5 each and the
    # first wins; t = .5 is the corner (0, 0, 0), which belongs to block (0, 0, 0).
    vol = volume({(0, 0, 0): np.ones((U, U, U), dtype=f32)})
    hit, _, _, _, _, rows = one_ray(vol, (-0.5, -0.5, -0.5), (1, 1, 1), dmax=1.0)
    assert not hit and rows[:2] == [(0.0625, (-1, -1, -1), False, 0.5), (0.5, (0, 0, 0), True, None)]
    assert [r[0] for r in rows[1:]] == [0.5, 0.75, 1.0]  # f = 1: steps of trunc


def test_f_prev_from_one_block_and_the_hit_in_the_next():
    # two open blocks along z with the plane z = 1.03125 (the centre of global voxel 16): voxel 15 holds .25, voxel 16 holds 0
    c = (np.arange(2 * U) + 0.5) * VL
    f = np.clip((1.03125 - c) / TRUNC, -1.0, 1.0).astype(f32)
    lo, hi = (np.broadcast_to(x.reshape(1, 1, U), (U, U, U)).copy() for x in (f[:U], f[U:]))
    assert lo[0, 0, 15] == f32(0.25) and hi[0, 0, 0] == 0
    vol = volume({(0, 0, 0): lo, (0, 0, 1): hi})
    # o_z = .90625 (voxel 14, f = .5), t0 = 1/16 -> voxel 15: f = .25, f_prev = -1: no hit; delta = .0625 = vl: t = .125
    # t = .125: p_z = 1.03125: voxel 16 = voxel 0 of block (0, 0, 1), f = 0 <= 0, f_prev = .25: HIT, t* = t
    hit, t, t_prev, f, f_prev, rows = one_ray(vol, (C, C, 0.90625), (0, 0, 1))
    assert hit and rows == [(0.0625, (0, 0, 0), True, None), (0.125, (0, 0, 1), True, None)]
    assert (t, t_prev, f, f_prev) == (0.125, 0.0625, 0.0, 0.25) and t_star(t, t_prev, f, f_prev) == 0.125


def test_no_hit_after_absent_space_from_behind_or_in_an_absent_block():
    # the first sample after absent space has f_prev = 0
    inside = volume({(0, 0, 0): np.full((U, U, U), -0.5, dtype=f32)})
    hit, _, _, _, _, rows = one_ray(inside, (C, C, -0.5), (0, 0, 1), dmax=3.0)
    assert not hit and rows[1] == (0.5, (0, 0, 0), True, None) and sum(r[2] for r in rows) == 16
    # from behind: the values rise along the ray
    hit, _, _, _, _, rows = one_ray(volume(PLANE_Z), (C, C, 0.96875), (0, 0, -1), dmax=3.0)
    assert not hit and len(rows) > 5
    # out of a positive voxel into a block that is not open: no hit even with the threshold 0 (DEPARTURE from the dense rule)
    hit, _, _, _, _, rows = one_ray(volume({(0, 0, 0): np.ones((U, U, U), dtype=f32)}), (C, C, 0.5), (0, 0, 1), wthr=0.0, dmax=3.0)
    assert not hit and rows[-1][2] is False


def test_a_sample_outside_the_index_range_ends_the_ray():
    vol = volume(PLANE_Z)
    edge = float(2 ** 24) * VL  # g = 2^24 is the first index outside
    hit, _, _, _, _, rows = one_ray(vol, (edge - 0.125, C, C), (1, 0, 0), dmax=5.0)
    # t = .0625: g = 2^24 - 1, block 2^20 - 1: absent, t_exit = .125; t = .125: g = 2^24: the ray ends before any look-up
    assert not hit and rows == [(0.0625, (2 ** 20 - 1, 0, 0), False, 0.125)]
    hit, _, _, _, _, rows = one_ray(vol, (-edge - 0.125, C, C), (1, 0, 0), dmin=0.0, dmax=5.0)
    assert not hit and rows == []  # g = -2^24 - 2 at the first sample (float32 has no -2^24 - 1)
    assert one_ray(vol, (-edge, C, C), (1, 0, 0), dmin=0.0, dmax=0.5)[5][0] == (0.0, (-2 ** 20, 0, 0), False, 1.0)  # -2^24 is inside
    assert one_ray(vol, (np.nan, C, C), (1, 0, 0))[5] == [] and one_ray(vol, (np.inf, C, C), (1, 0, 0))[5] == []


def test_the_step_cap_ends_a_ray_whose_t_cannot_advance():
    # t = 2^21 has an ulp of 1/4: t + vl_f == t.  o = -2^21 + .5 on every axis and d = (1, 1, 1): the sample is (.5, .5, .5)
    # in the open block, f = -.125 (f_prev = -1: no hit), delta < vl_f, and t stays.  dmin = dmax: n_cap = 0 + 2.
    vol = volume(PLANE_Z)
    X = float(2 ** 21)
    assert SR.step_cap(vol, X, X) == 2 and f32(X) + f32(VL) == f32(X)
    hit, _, _, _, _, rows = one_ray(vol, (0.5 - X,) * 3, (1, 1, 1), dmin=X, dmax=X)
    assert not hit and rows == [(X, (0, 0, 0), True, None)] * 2
    assert SR.step_cap(vol, 0.1, 3.0) == int(np.floor((float(f32(3.0)) - float(f32(0.1))) / VL)) + 2
    assert SR.step_cap(SR.S.ScalableVolume(1e-6, 1e-5), 0.0, 1e6) == 2 ** 20


def test_an_empty_volume():
    vol = SR.S.ScalableVolume(VL, TRUNC, T.RGB8)
    r = SR.ray_cast(vol, T.camera(5, 4), np.eye(4), 5, 4)
    assert r.hits == 0 and not r.depth.any() and not r.vertex.any() and not r.normal.any() and not r.color.any() and not r.steps.any()


def test_the_colour_rule_with_a_corner_in_an_absent_block_and_near():
    col = np.zeros((U, U, U, 3))
    col[...] = (200.0, 100.0, 50.0)
    one = np.full((U, U, U), 5, dtype=f32)
    vol = SR.volume_of_blocks(VL, TRUNC, T.RGB8, {(0, 0, 0): (plane_block(2, 0.5, +1), one, col)})
    lat = SR.Lattice(vol)
    q = np.array([[0.01, 0.3, 0.5]])  # x below the first voxel centre: four corners lie in block (-1, 0, 0), which is not open
    got = SR.color_at(vol, lat, q)
    # the four counting corners share one colour: num / den is that colour up to the rounding of the sums
    assert np.allclose(got, np.array([[200.0, 100.0, 50.0]]) / 255.0, rtol=1e-15, atol=0)
    # the same block opened with weights 0 changes nothing; opened with a weight and black voxels it darkens the value
    unseen = SR.volume_of_blocks(VL, TRUNC, T.RGB8, {(0, 0, 0): (plane_block(2, 0.5, +1), one, col),
                                                     (-1, 0, 0): (np.zeros((U, U, U), dtype=f32), 0 * one, 0 * col)})
    assert (SR.color_at(unseen, SR.Lattice(unseen), q) == got).all()
    seen = SR.volume_of_blocks(VL, TRUNC, T.RGB8, {(0, 0, 0): (plane_block(2, 0.5, +1), one, col),
                                                   (-1, 0, 0): (np.zeros((U, U, U), dtype=f32), one, 0 * col)})
    r = (0.01 / VL - 0.5) - np.floor(0.01 / VL - 0.5)  # the weight of the corners in block (0, 0, 0)
    assert np.allclose(SR.color_at(seen, SR.Lattice(seen), q), got * r, rtol=1e-12)
    # no corner counts: 0
    assert (SR.color_at(vol, lat, np.array([[5.0, 5.0, 5.0]])) == 0).all()
    # NEAR: |q_k| <= (2^24 + 2) vl = 1048576.125; a hit beyond it keeps its depth and vertex and has normal and colour 0
    for x, near in ((1048576.125, True), (1048576.25, False), (-1048576.25, False)):
        ts, vertex, normal, color, is_near = SR.finish(vol, lat, np.zeros(3, dtype=f32), np.array([[np.sign(x), 0, 0]], dtype=f32),
                                                       np.array([abs(x)], dtype=f32), np.array([abs(x)], dtype=f32),
                                                       np.array([-1], dtype=f32), np.array([1], dtype=f32))
        assert ts[0] == f32(abs(x)) and vertex[0, 0] == f32(x) and bool(is_near[0]) == near and not normal.any() and not color.any()
    # a hit in the block: the normal of the plane z = .5 seen from below points against the ray
    ts, vertex, normal, color, is_near = SR.finish(vol, lat, np.array([C, C, 0], dtype=f32), np.array([[0, 0, 1]], dtype=f32),
                                                   np.array([0.5], dtype=f32), np.array([0.28125], dtype=f32),
                                                   np.array([-0.125], dtype=f32), np.array([0.875], dtype=f32))
    assert ts[0] == f32(0.47265625) and (vertex[0] == np.array([C, C, 0.47265625], dtype=f32)).all() and is_near[0]
    assert (normal[0] == np.array([0, 0, -1], dtype=f32)).all() and np.allclose(color[0], np.array([200, 100, 50]) / 255.0, rtol=1e-6)


# ---- the dense identity ----------------------------------------------------------------------------------------------
def dense_and_blocks(seed, color_type):
    """A dense volume of R = 32 with voxels of 1/16 at the origin, its outermost voxel layer unobserved, and the eight
    blocks of [0, 2)^3 that hold the same voxels."""
    rng = np.random.default_rng(seed)
    R = 2 * U
    vol = T.Volume(2.0, R, TRUNC, color_type)
    assert vol.vl == VL and vol.vl_f == f32(VL)
    # a smooth surface (so that rays hit) with noise on it
    x = (np.arange(R) + 0.5) * VL
    X, Y, Z = np.meshgrid(x, x, x, indexing="ij")
    d = np.sqrt((X - 1.0) ** 2 + (Y - 1.1) ** 2 + (Z - 1.6) ** 2) - 0.45
    vol.tsdf[:] = np.clip(d / TRUNC + rng.uniform(-0.2, 0.2, d.shape), -1.0, 1.0).astype(f32)
    vol.weight[:] = (rng.random((R, R, R)) >= 0.2).astype(f32) * f32(3)
    for k in range(3):
        for side in (0, R - 1):
            at = [slice(None)] * 3
            at[k] = side
            vol.weight[tuple(at)] = 0
    if color_type == T.RGB8:
        vol.color[:] = rng.integers(0, 256, (R, R, R, 3)).astype(np.float64)
    elif color_type == T.GRAY32:
        vol.color[:] = np.repeat(rng.random((R, R, R, 1)), 3, axis=3)
        vol.color[rng.random((R, R, R)) < 0.05] = np.nan
    blocks = {}
    for b in np.ndindex(2, 2, 2):
        at = tuple(slice(U * k, U * k + U) for k in b)
        blocks[b] = (vol.tsdf[at], vol.weight[at], vol.color[at] if color_type != T.NONE else None)
    return vol, SR.volume_of_blocks(VL, TRUNC, color_type, blocks)


@pytest.mark.parametrize("color_type", (T.NONE, T.RGB8, T.GRAY32))
def test_eight_blocks_are_the_dense_volume_they_hold(color_type):
    """With the camera strictly inside the box the dense clip leaves t0 = dmin, and outside the box there is nothing
    observed in either volume; the outermost layer is unobserved so that a sample the dense clip cuts off at the box's
    face cannot be a hit.  Thresholds above 0: at 0 the dense rule ends a ray that leaves the box (see the DEPARTURE)."""
    dense, vol = dense_and_blocks(5 + color_type, color_type)
    lat = SR.Lattice(vol)
    hits = 0
    for (w, h), E, thr in (((33, 17), T.extrinsic(0.1, -0.15, 0.2, (-1.0, -0.9, -0.4)), 3.0), ((1, 1), T.extrinsic(0.0, 0.0, 0.0, (-1.0, -1.1, -0.3)), 1.0),
                           ((33, 17), T.extrinsic(-0.3, 0.4, 0.0, (-0.9, -1.0, -0.7)), 1.0)):
        K = T.camera(w, h)
        a = RC.ray_cast(dense, K, E, w, h, 0.05, 3.0, thr)
        b = SR.ray_cast(vol, K, E, w, h, 0.05, 3.0, thr, lat=lat)
        hits += a.hits
        assert a.hits == b.hits and (a.hit == b.hit).all()
        for m in ("depth", "vertex", "normal") + (("color",) if color_type != T.NONE else ()):
            assert getattr(a, m).tobytes() == getattr(b, m).tobytes(), m
    assert hits > 150  # both outcomes occur


# ---- the analytic sphere ---------------------------------------------------------------------------------------------
RADIUS = 10.0  # voxels
# Measured on this restatement (the test prints the figures): the largest depth error against the analytic sphere over
# the pixels whose ray passes at least two voxels inside the silhouette is 1.034615505280847 voxels from outside (640
# pixels, all hit; 1.855924523424214 over all hits, grazing rays included; at most 26 steps, 13.8 on average against 70.9
# without the skip) and 0.5906307854521682 voxel from the centre (4800 pixels, all hit; at most 5 steps).  The bounds are
# those maxima rounded up to the next 0.05 voxel.
SPHERE_MEASURED = {"outside": 1.05, "centre": 0.60}


def sphere_volume(cavity):
    """A sphere of 10 voxels around the world origin (a block corner, so that the blocks have negative indices), stored
    in only the blocks that have a voxel within sdf_trunc (3 voxels) of the surface.  cavity: the free space is inside."""
    trunc = 3.0 * VL
    blocks = {}
    for b in np.ndindex(4, 4, 4):
        b = tuple(k - 2 for k in b)
        c = [(b[k] * U + np.arange(U) + 0.5) * VL for k in range(3)]
        X, Y, Z = np.meshgrid(*c, indexing="ij")
        d = np.sqrt(X * X + Y * Y + Z * Z) - RADIUS * VL
        if (np.abs(d) <= trunc).any():
            f = np.clip((-d if cavity else d) / trunc, -1.0, 1.0).astype(f32)
            blocks[b] = (f, np.full((U, U, U), 1, dtype=f32), None)
    return SR.volume_of_blocks(VL, trunc, T.NONE, blocks)


@pytest.mark.parametrize("where", ("outside", "centre"))
def test_an_analytic_sphere_in_the_blocks_near_its_surface(where):
    """Geometry, not code: the depth against the analytic sphere, 80 x 60.  From outside (40 voxels in front of the
    centre) the sphere is solid, from its centre it is a cavity -- the values are positive on the camera's side, as
    integration leaves them.  Every pixel whose ray passes two voxels or more inside the silhouette hits, none further
    than a voxel outside it does, and no ray takes more steps than without the skip.  Measured against the analytic
    sphere (not against any code): the largest depth error inside the silhouette is 1.034615505280847 voxels from
    outside and 0.5906307854521682 voxel from the centre; the bounds are 1.05 and 0.60, those maxima rounded up to the
    next 0.05 voxel (SPHERE_MEASURED).  The dense ray cast's figure on its own sphere scene was 0.72."""
    w, h = 80, 60
    cavity = where == "centre"
    vol = sphere_volume(cavity)
    assert len(vol.blocks) == 8  # of the 64 around the centre
    K = T.camera(w, h)
    c = np.array([0.0, 0.0, 0.0 if cavity else -40.0 * VL])
    E = np.eye(4)
    E[:3, 3] = -c
    lat = SR.Lattice(vol)
    r = SR.ray_cast(vol, K, E, w, h, 0.01, 6.0, 1.0, lat=lat)
    slow = SR.ray_cast(vol, K, E, w, h, 0.01, 6.0, 1.0, lat=lat, skip=False)
    assert (r.steps <= slow.steps).all()
    if not cavity:  # from the centre every sample lies in one of the eight open blocks
        assert 2 * r.steps.sum() < slow.steps.sum()
    i, j = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    d = np.stack([(j - K[2]) / K[0], (i - K[3]) / K[1], np.ones_like(i)], axis=2)
    A, B, C0 = (d * d).sum(axis=2), 2.0 * (d @ c), c @ c - (RADIUS * VL) ** 2
    disc = B * B - 4.0 * A * C0
    root = np.sqrt(np.maximum(disc, 0.0))
    t = ((-B + root) if cavity else (-B - root)) / (2.0 * A)  # d_z = 1: t is the z-depth
    dist = np.linalg.norm(np.cross(d, np.broadcast_to(-c, d.shape)), axis=2) / np.sqrt(A)
    inner, outer = dist <= (RADIUS - 2.0) * VL, dist > (RADIUS + 1.0) * VL
    err = np.abs(r.depth.astype(np.float64) - t) / VL
    print(where, "hits", r.hits, "inner", int(inner.sum()), "inner max", err[inner].max(), "all max", err[r.hit & (disc > 0)].max(),
          "steps", r.steps.max(), "mean", r.steps.mean(), "without skip", slow.steps.mean())
    assert inner.sum() > (4000 if cavity else 300) and r.hit[inner].all() and not r.hit[outer].any()
    assert err[inner].max() <= SPHERE_MEASURED[where]
    assert err[inner].max() < 2.0  # the dense figures were 0.72 inside the silhouette: above 2 is a bug, not a bound
    v = r.vertex[inner].astype(np.float64)
    cosine = (r.normal[inner].astype(np.float64) * v).sum(axis=1) / np.linalg.norm(v, axis=1)
    assert (cosine.max() < -0.99) if cavity else (cosine.min() > 0.99)
