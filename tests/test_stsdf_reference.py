"""The restatement of the scalable TSDF volume (tests/stsdf_reference.py) pinned by hand: the touched set of one point,
with a negative block index and a point exactly on a block face; a surface row across a block face; a normal whose
trilinear corners span two blocks, one of them absent; the closed-form inverse of the extrinsic.  And the conditions the
fixture scenes must meet for the GPU comparison to exercise the new rules, asserted here on the restatement alone."""
import numpy as np
import pytest

import stsdf_reference as S
import tsdf_reference as T

f32 = np.float32


def box(x, y, z):
    return {(a, b, c) for a in x for b in y for c in z}


def test_the_touched_set_of_one_point_by_hand():
    # ul = 1, sdf_trunc = 1/4.  p = (-0.1, -0.9, 2.0): x - 1/4 = -0.35 -> -1, x + 1/4 = 0.15 -> 0; y: -1.15 -> -2, -0.65 -> -1;
    # z lies exactly on the face between blocks 1 and 2: 1.75 -> 1, 2.25 -> 2
    blocks, oor = S.touched_by_points(np.array([[-0.1, -0.9, 2.0]]), 0.25, 1.0)
    assert blocks == box((-1, 0), (-2, -1), (1, 2)) and oor == 0
    # the lower end exactly on a face: (2 - 1) / 1 = 1 belongs to block 1, not to block 0
    blocks, _ = S.touched_by_points(np.array([[0.5, 0.5, 2.0]]), 1.0, 1.0)
    assert blocks == box((-1, 0, 1), (-1, 0, 1), (1, 2, 3))
    # a point well inside a block with a small truncation touches that block alone
    assert S.touched_by_points(np.array([[-0.5, 0.5, 7.5]]), 0.25, 1.0)[0] == {(-1, 0, 7)}
    # a component that is not finite touches nothing and counts nothing
    assert S.touched_by_points(np.array([[np.inf, 0.0, 0.0], [0.0, np.nan, 0.0]]), 0.25, 1.0) == (set(), 0)
    # the ends of the index range: block 2^20 - 1 is the last one, and the point that reaches past it is counted once
    top = float(2 ** 20)
    blocks, oor = S.touched_by_points(np.array([[top - 0.1, 0.5, 0.5], [-top - 0.1, 0.5, 0.5], [3 * top, 0.5, 0.5]]), 0.25, 1.0)
    assert blocks == {(2 ** 20 - 1, 0, 0), (-2 ** 20, 0, 0)} and oor == 3


def test_a_one_pixel_frame_touches_the_blocks_of_its_point():
    # voxels of 1/16: ul = 1.  One pixel at the principal point with depth 2 m: the camera point (0, 0, 2); the extrinsic
    # moves the world by (0.1, 0.9, 0), so the world point is (-0.1, -0.9, 2.0): the first case above
    vol = S.ScalableVolume(0.0625, 0.25, stride=1)
    E = np.eye(4)
    E[:3, 3] = [0.1, 0.9, 0.0]
    f = T.frame(np.array([[2.0]], dtype=f32), (1.0, 1.0, 0.0, 0.0), E)
    assert vol.touch(f) == (box((-1, 0), (-2, -1), (1, 2)), 0)
    assert vol.touch(T.frame(np.array([[0.0]], dtype=f32), (1.0, 1.0, 0.0, 0.0), E)) == (set(), 0)
    assert vol.touch(T.frame(np.array([[2000]], dtype=np.uint16), (1.0, 1.0, 0.0, 0.0), E, depth_trunc=3.0))[0] == box((-1, 0), (-2, -1), (1, 2))
    assert vol.touch(T.frame(np.array([[2000]], dtype=np.uint16), (1.0, 1.0, 0.0, 0.0), E, depth_trunc=2.0)) == (set(), 0)


def test_the_closed_form_inverse():
    E = T.extrinsic(0.3, -0.2, 0.5, (0.4, -1.5, 2.25))
    M = S.camera_pose(E)
    assert np.allclose(M @ E, np.eye(4), atol=1e-15) and np.allclose(M, np.linalg.inv(E), atol=1e-15)
    E = np.eye(4)
    E[:3, 3] = [0.5, -0.25, 4.0]
    assert S.camera_pose(E).tolist() == [[1, 0, 0, -0.5], [0, 1, 0, 0.25], [0, 0, 1, -4.0], [0, 0, 0, 1]]
    E = np.diag([2.0, 4.0, 0.5, 1.0])  # not a rotation: the adjugate form inverts it all the same
    assert S.camera_pose(E).tolist() == [[0.5, 0, 0, 0], [0, 0.25, 0, 0], [0, 0, 2.0, 0], [0, 0, 0, 1]]


def two_blocks(present=True, ctype=S.RGB8):
    """Voxels of 1/4 (ul = 4): voxel (15, 3, 4) of block (-1, 0, 0) and its neighbour across the face, voxel (0, 3, 4) of
    block (0, 0, 0)."""
    vol = S.ScalableVolume(0.25, 1.0, ctype)
    for b in ((-1, 0, 0), (0, 0, 0)) if present else ((-1, 0, 0),):
        vol.blocks[b] = T.Volume(4.0, 16, 1.0, ctype, tuple(4.0 * k for k in b))
    a = vol.blocks[(-1, 0, 0)]
    a.tsdf[15, 3, 4], a.weight[15, 3, 4], a.color[15, 3, 4] = 0.5, 1.0, (30.0, 60.0, 90.0)
    if present:
        b = vol.blocks[(0, 0, 0)]
        b.tsdf[0, 3, 4], b.weight[0, 3, 4], b.color[0, 3, 4] = -0.25, 2.0, (60.0, 0.0, 30.0)
    return vol


def test_a_surface_row_across_a_block_face_by_hand():
    points, normals, colors, crossing = two_blocks().extract_point_cloud()
    # p0_x = (1/8 + 15/4) - 4 = -1/8;  r0 = 1/2, r1 = 1/4:  p_x = (-1/8 1/4 + 1/8 1/2) / (3/4) = (1/32) / (3/4)
    assert points.tolist() == [[0.03125 / 0.75, 0.125 + 0.75, 0.125 + 1.0]]
    # (30 1/4 + 60 1/2) / (3/4) = 50;  (60 1/4 + 0) / (3/4) = 20;  (90 1/4 + 30 1/2) / (3/4) = 50
    assert colors.tolist() == [[50.0 / 255.0, 20.0 / 255.0, 50.0 / 255.0]]
    assert crossing.tolist() == [[0, 1]]
    # the same voxel with the next block absent gives no row; neither do the two usable voxels in the other directions
    assert len(two_blocks(present=False).extract_point_cloud()[0]) == 0
    # the voxel cloud: both voxels, the block (-1, 0, 0) first
    vp, vc = two_blocks().extract_voxel_point_cloud()
    assert vp.tolist() == [[-0.125, 0.875, 1.125], [0.125, 0.875, 1.125]] and vc.tolist() == [[0.75] * 3, [0.375] * 3]


def corner_case(present):
    """A row inside block (-1, 0, 0), one voxel from its face: the trilinear corners of its normal reach voxel 0 of block
    (0, 0, 0), which is absent or holds 0.8 there (with weight 0: it gives no row)."""
    vol = S.ScalableVolume(0.25, 1.0, S.NONE)
    a = vol.blocks[(-1, 0, 0)] = T.Volume(4.0, 16, 1.0, S.NONE, (-4.0, 0.0, 0.0))
    a.tsdf[14, 3, 4], a.weight[14, 3, 4] = 0.5, 1.0
    a.tsdf[15, 3, 4], a.weight[15, 3, 4] = -0.5, 1.0
    a.tsdf[15, 4, 4] = 0.25  # weight 0: not usable, but a corner of T
    if present:
        b = vol.blocks[(0, 0, 0)] = T.Volume(4.0, 16, 1.0, S.NONE, (0.0, 0.0, 0.0))
        b.tsdf[0, 3, 4] = 0.8
    return vol


def test_a_normal_whose_corners_span_two_blocks_by_hand():
    # p0_x = (1/8 + 14/4) - 4 = -3/8, r0 = r1 = 1/2: p = (-1/4, 7/8, 9/8); a = p / vl - 1/2 = (-1.5, 3, 4): on the lattice in y, z
    # x + g: a_x = -0.51: g = -1, r = 0.49: voxel -1 (local 15 of block -1: -0.5) and voxel 0 (block 0: absent or 0.8)
    # x - g: a_x = -2.49: g = -3, r = 0.51: voxel -3 (0) and voxel -2 (local 14: 0.5)
    # y + g: a_y = 3.99: voxels y = 3 (weight 0.01) and 4 (0.99) at x = -2 (r = 0.5: 0.5 and nothing) and x = -1 (-0.5 and 0.25)
    # y - g: a_y = 2.01: y = 3 with weight 0.01: 0.5 0.01 0.5 + 0.5 0.01 (-0.5) = 0;  z: the same cancellation
    for present, v in ((False, 0.0), (True, float(f32(0.8)))):  # the voxel holds the float32 nearest to 0.8
        points, normals, _, _ = corner_case(present).extract_point_cloud()
        assert points.tolist() == [[-0.25, 0.875, 1.125]]
        nx = (0.51 * -0.5 + 0.49 * v) - 0.51 * 0.5
        ny = 0.5 * 0.99 * 0.25 + (0.5 * 0.01 * 0.5 + 0.5 * 0.01 * -0.5)
        want = np.array([nx, ny, 0.0]) / np.sqrt(nx * nx + ny * ny)
        assert normals.shape == (1, 3) and normals[0, 2] == 0.0
        assert np.abs(normals[0] - want).max() < 1e-13, (normals, want)
    assert abs(corner_case(False).extract_point_cloud()[1][0, 0] - corner_case(True).extract_point_cloud()[1][0, 0]) > 0.2


def test_floor_division_of_negative_lattice_indices():
    vol = corner_case(True)
    G = np.array([[-1, 3, 4], [-2, 3, 4], [0, 3, 4], [-16, 3, 4], [-17, 3, 4], [16, 3, 4]], dtype=np.int64)
    assert vol.tsdf_at(G).tolist() == [-0.5, 0.5, f32(0.8), 0.0, 0.0, 0.0]


# ---- the fixture scenes --------------------------------------------------------------------------------------------
def test_every_scene_stays_small():
    for name in S.cases():
        assert len(S.result(name).keys) <= 100, name
    assert len(S.result("identity").keys) <= 30


def test_blocks_with_negative_indices_on_every_axis():
    assert any((S.result(n).keys < 0).any(axis=0).all() and (S.result(n).keys >= 0).any() for n in S.cases() if len(S.result(n).keys))
    assert (S.result("rgb_64").keys < 0).any(axis=0).all()


@pytest.mark.parametrize("name", ["rgb_64", "none_7"])
def test_surface_rows_cross_block_faces_along_every_axis(name):
    c = S.result(name).crossing
    for i in range(3):
        assert ((c[:, 0] == i) & (c[:, 1] == 1)).any(), i


@pytest.mark.parametrize("name", ["rgb_64", "none_7", "split_17", "identity"])
def test_a_later_frame_opens_blocks_and_a_middle_frame_skips_some(name):
    log = [set(x) for x in S.result(name).vol.log]
    seen, later = set(log[0]), False
    for k in range(1, len(log)):
        later |= bool(log[k] - seen)
        seen |= log[k]
    assert later                                                    # a block no earlier frame touched
    assert any(log[a] & log[c] - log[b] for a in range(len(log)) for b in range(a + 1, len(log)) for c in range(b + 1, len(log)))


def test_the_counts_and_the_splits_of_the_restatement():
    r = S.result("split_17")
    assert r.touched == sum(len(x) for x in r.vol.log) and r.opened == len(r.keys) and r.out_of_range == 0
    far = S.result("far")
    assert far.out_of_range > 0 and 0 < len(far.keys) and len(far.vol.log[1]) == 0
    assert (far.keys[:, 0].max(), far.keys[:, 0].min()) == (2 ** 20 - 1, -2 ** 20)
    assert len(S.result("nothing").keys) == 0 and len(S.result("rgb_7_wide_stride").vol.log[0]) <= 8
