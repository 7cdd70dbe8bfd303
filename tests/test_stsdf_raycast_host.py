"""The host side of the ray cast of the scalable TSDF volume without a GPU: csrc/stsdf.hip and csrc/stsdf_raycast.hip
compiled by g++ against the HIP stand-in header with a CPU stand-in for the launcher, which calls stsdf_ray_thread of
csrc/stsdf_raycast_device.h -- the text the kernel compiles -- for every thread of every block
(tests/stsdf_raycast_host_driver.cpp).  Built with -ffp-contract=off under AddressSanitizer and UndefinedBehaviorSanitizer
and run as a stand-alone program.  The entry checks, the view records with their step caps, the block map, the
directory's upload after every growth, the output layout for mixed view sizes, NULL arrays and NULL entries and every
refusal with its text run for real; depth, vertex, normal and colour maps are compared bit for bit, and the hit counts,
with the restatement's (tests/stsdf_raycast_reference.py): the plane volumes of the hand cases seen along the axes, the
other hand-worked rays (a block corner, f_prev across two blocks, the index range, the step cap), random
sets of five blocks from [-2, 2)^3 with the thresholds 0, 1 and 3 in the three colour types, and an empty volume."""
import subprocess

import numpy as np

import stsdf_raycast_reference as SR
import tsdf_raycast_reference as RC
import tsdf_reference as T
from test_outlier_host import hexes, ints
from test_search_host import compile_driver

f32 = np.float32
U = SR.U


def bits(a):
    return ints(np.ascontiguousarray(a, dtype=np.float32).view(np.uint32))


def looking_along(axis, sign, centre):
    """World to camera with exact entries: the camera at `centre` looks along sign e_axis."""
    Rt = np.zeros((3, 3))
    Rt[axis, 2] = sign
    Rt[(axis + 1) % 3, 0] = 1.0
    Rt[(axis + 2) % 3, 1] = sign
    E = np.eye(4)
    E[:3, :3] = Rt.T
    E[:3, 3] = -Rt.T @ np.asarray(centre, dtype=np.float64)
    return E


def hand_cases():
    """The volumes of tests/test_stsdf_raycast_reference.py seen along every axis in both directions by a 3 x 2 view whose
    pixel (0, 0) is the ray along the axis, and by a 5 x 4 view with a wide angle."""
    VL, TRUNC, C = 1.0 / 16.0, 0.25, 0.53125
    c = (np.arange(U) + 0.5) * VL
    out = []
    for axis in range(3):
        for side in (+1, -1):
            f = np.clip(side * (0.5 - c) / TRUNC, -1.0, 1.0).astype(f32)
            shape = [1, 1, 1]
            shape[axis] = U
            tsdf = np.broadcast_to(f.reshape(shape), (U, U, U)).copy()
            key = [0, 0, 0]
            key[axis] = -2
            vol = SR.volume_of_blocks(VL, TRUNC, T.NONE, {tuple(key): (tsdf, np.full((U, U, U), 5, dtype=f32), None)})
            centre = [C, C, C]
            centre[axis] = -3.5 if side > 0 else 0.5
            E = looking_along(axis, float(side), centre)
            views = [RC.view(3, 2, E, K=(1.0, 1.0, 0.0, 0.0), depth_min=0.0625, depth_max=10.0),
                     RC.view(5, 4, E, K=(2.0, 2.0, 2.0, 1.5), depth_min=0.0625, depth_max=10.0, weight_threshold=5.0),
                     RC.view(1, 1, E, K=(1.0, 1.0, 0.0, 0.0), depth_min=0.0625, depth_max=1.0)]
            out.append((vol, views))
    return out


def more_hand_cases():
    """The other rays of tests/test_stsdf_raycast_reference.py, each as pixel (1, 1) or (0, 0) of a 3 x 2 view with
    fx = fy = 1 and the principal point on pixel (0, 0), so that pixel (v, u) has the camera direction (u, v, 1): the ray
    through a block corner, f_prev from one block and the hit in the next, samples outside the index range on either
    side, and the ray whose t cannot advance, which the step cap ends."""
    VL, TRUNC, C = 1.0 / 16.0, 0.25, 0.53125
    K = (1.0, 1.0, 0.0, 0.0)
    five = np.full((U, U, U), 5, dtype=f32)

    def along_z(f):
        return np.broadcast_to(f.reshape(1, 1, U), (U, U, U)).copy()

    def at(centre):
        E = np.eye(4)
        E[:3, 3] = -np.asarray(centre, dtype=np.float64)
        return E
    c = (np.arange(2 * U) + 0.5) * VL
    plane = along_z(np.clip((0.5 - c[:U]) / TRUNC, -1.0, 1.0).astype(f32))
    one = SR.volume_of_blocks(VL, TRUNC, T.NONE, {(0, 0, 0): (plane, five, None)})
    f = np.clip((1.03125 - c) / TRUNC, -1.0, 1.0).astype(f32)
    two = SR.volume_of_blocks(VL, TRUNC, T.NONE, {(0, 0, 0): (along_z(f[:U]), five, None), (0, 0, 1): (along_z(f[U:]), five, None)})
    edge, X = float(2 ** 24) * VL, float(2 ** 21)
    out = [(one, [RC.view(3, 2, at((-0.5, -0.5, -0.5)), K=K, depth_min=0.0625, depth_max=2.0)]),           # pixel (1, 1): the corner
           (two, [RC.view(3, 2, at((C, C, 0.90625)), K=K, depth_min=0.0625, depth_max=10.0)]),             # pixel (0, 0)
           (one, [RC.view(3, 2, looking_along(0, 1.0, (edge - 0.125, C, C)), K=K, depth_min=0.0625, depth_max=5.0),
                  RC.view(3, 2, looking_along(0, 1.0, (-edge - 0.125, C, C)), K=K, depth_min=0.0, depth_max=5.0),
                  RC.view(3, 2, looking_along(0, 1.0, (-edge, C, C)), K=K, depth_min=0.0, depth_max=0.5)]),
           (one, [RC.view(3, 2, at((0.5 - X,) * 3), K=K, depth_min=X, depth_max=X)])]                      # pixel (1, 1): t + vl_f == t
    # what the hand cases say of these rays, on the restatement: the corner ray and the ray across the blocks hit, the
    # others miss
    assert SR.cast(one, out[0][1][0]).hit[1, 1] and SR.cast(two, out[1][1][0]).hit[0, 0]
    assert not any(SR.cast(one, w).hits for w in out[2][1]) and SR.cast(one, out[3][1][0]).hits == 0
    assert SR.cast(one, out[3][1][0]).steps[1, 1] == 2  # the cap: floor(0 / vl) + 2
    return out


def case_lines(vol, views):
    ctype = vol.color_type
    keys = vol.keys()
    lines = [str(ctype), hexes([vol.vl, vol.sdf_trunc]), str(len(keys)), ints(keys), hexes(vol.block_tsdf_weight()) if len(keys) else "",
             hexes(vol.block_colors()) if ctype and len(keys) else "", str(len(views))]
    lat = SR.Lattice(vol)
    hit = miss = 0
    for w in views:
        r = SR.cast(vol, w, lat)
        hit, miss = hit + r.hits, miss + w.width * w.height - r.hits
        lines += ["%d %d" % (w.width, w.height), hexes(w.K), hexes(w.E), hexes([w.depth_min, w.depth_max, w.weight_threshold]),
                  str(r.hits), bits(r.depth), bits(r.vertex), bits(r.normal), bits(r.color) if ctype else ""]
    return lines, hit, miss


def host_cases():
    out = hand_cases()
    for seed, ctype, thr, weight in SR.RANDOM_SETS:
        vol = SR.random_blocks(seed, ctype, weight)
        out.append((vol, SR.views_of(vol, thr)))
    out += more_hand_cases()
    empty = SR.S.ScalableVolume(0.02, 0.06, T.RGB8)
    out.append((empty, [RC.view(5, 3, np.eye(4)), RC.view(0, 0, np.eye(4))]))
    return out


def test_host_code_is_clean_and_equal_to_the_restatement(tmp_path):
    cases = host_cases()
    assert {v.color_type for v, _ in cases} == {T.NONE, T.RGB8, T.GRAY32}
    assert {w.weight_threshold for v, views in cases[6:12] for w in views} == {0.0, 1.0, 3.0}
    lines = [str(len(cases))]
    hits = []
    for vol, views in cases:
        text, hit, miss = case_lines(vol, views)
        lines += text
        hits.append((hit, miss))
    # the plane volumes and the random sets must show both outcomes, or equality would say little; the empty volume misses
    assert all(h > 0 and m > 0 for h, m in hits[:12]) and hits[-1][0] == 0, hits
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    exe = compile_driver("stsdf_raycast_host_driver", tmp_path)
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "mismatches 0" in out.stdout, out.stdout + out.stderr[-4000:]
