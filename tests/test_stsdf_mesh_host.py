"""The host side of the triangle mesh of the scalable TSDF volume without a GPU: csrc/stsdf.hip and csrc/stsdf_mesh.hip
compiled by g++ against the HIP stand-in header with CPU stand-ins for the launchers, which call the functions of
csrc/stsdf_mesh_device.h -- the text the kernels compile -- for every column of every open block
(tests/stsdf_mesh_host_driver.cpp).  Built with -ffp-contract=off under AddressSanitizer and UndefinedBehaviorSanitizer
and run as a stand-alone program.  The entry checks, the scratch layout and its growth with the directory, the output
layout, the counts alone, the capacity rule per array, the launch counts and every refusal with its text run for real;
counts, vertices, colours, normals and triangles are compared for equality with the restatement's
(tests/stsdf_mesh_reference.py) on the blocks of the host cases' scenes, on random block sets (one block, a pair along z,
2 x 2 x 2, the L shape with its corner block missing; zeroed weights, NaN Gray32 colours, negative block indices) and on
the one cube whose eight corners lie in eight blocks."""
import subprocess

import numpy as np

import stsdf_mesh_reference as R
import stsdf_reference as S
import tsdf_reference as T
from test_outlier_host import hexes, ints
from test_search_host import compile_driver

SCENES = ("none_7", "gray_7", "rgb_7_wide_stride", "far", "nothing", "empty")
SETS = ("one", "pair_z", "cube_2", "l_shape")


def case_lines(vol, m):
    ctype = vol.color_type
    keys = vol.keys()
    return [str(ctype), hexes([vol.vl, vol.sdf_trunc]), str(len(keys)), ints(keys), hexes(vol.block_tsdf_weight()) if len(keys) else "",
            hexes(vol.block_colors()) if ctype and len(keys) else "", str(len(m.vertices)), hexes(m.vertices), hexes(m.normals),
            hexes(m.colors) if ctype else "", str(len(m.triangles)), ints(m.triangles)]


def host_cases():
    out = [(R.volume(name), R.result(name)) for name in SCENES + SETS]
    for pattern, missing, ctype in ((0x69, None, T.RGB8), (0x17, None, T.NONE), (0x17, (0, -1, 0), T.NONE)):
        vol = R.corner_cube_volume(pattern, missing, ctype)
        out.append((vol, R.extract_triangle_mesh(vol, normals=True)))
    return out


def test_host_code_is_clean_and_equal_to_the_restatement(tmp_path):
    cases = host_cases()
    assert {v.color_type for v, _ in cases} == {T.NONE, T.RGB8, T.GRAY32}
    assert all(S.cases()[name].host for name in SCENES)
    # the scenes and the larger sets meet the hard cases, or equality would say little
    for vol, m in cases[:4] + cases[8:10]:
        blocks, cubes, crossing, differ = R.face_statistics(vol)
        assert crossing >= 1 and differ >= 1 and len(m.vertices) > 100
    assert len(cases[4][1].vertices) == 0 and len(cases[5][1].vertices) == 0 and len(cases[-1][1].vertices) == 0
    assert any(np.isnan(m.colors).any() for _, m in cases if m.colors is not None)
    lines = [str(len(cases))]
    for vol, m in cases:
        lines += case_lines(vol, m)
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    exe = compile_driver("stsdf_mesh_host_driver", tmp_path)
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "mismatches 0" in out.stdout, out.stdout + out.stderr[-4000:]
