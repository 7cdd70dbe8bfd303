"""The host side of the triangle mesh of the TSDF volume without a GPU: csrc/tsdf.hip and csrc/tsdf_mesh.hip compiled by
g++ against the HIP stand-in header with CPU stand-ins for the launchers, which call the column functions of
csrc/tsdf_mesh_device.h -- the text the kernels compile -- (tests/tsdf_mesh_host_driver.cpp).  Built with
-ffp-contract=off under AddressSanitizer and UndefinedBehaviorSanitizer and run as a stand-alone program.  The entry
checks, the scratch and output layouts, the capacity rule of either array, the counts-only call and every refusal run
for real; counts, vertices, colours, normals and triangles are compared for equality with the restatement's
(tests/tsdf_mesh_reference.py): the `host` cases of tsdf_reference.cases(), random volumes of 2, 3 and 6 voxels a side with
zeroed weights and the three colour types, and the analytic sphere."""
import subprocess

import numpy as np

import tsdf_mesh_reference as M
import tsdf_reference as T
from test_outlier_host import hexes, ints
from test_search_host import compile_driver


def volume_lines(vol, mesh):
    ctype = vol.color_type
    return ["%d %d" % (vol.R, ctype), hexes([vol.length, vol.sdf_trunc]) + " " + hexes(vol.origin), hexes(vol.tsdf_weight()),
            hexes(vol.colors()) if ctype else "", str(len(mesh.vertices)), hexes(mesh.vertices), hexes(mesh.normals),
            hexes(mesh.colors) if ctype else "", str(len(mesh.triangles)), ints(mesh.triangles)]


def test_host_code_is_clean_and_equal_to_the_restatement(tmp_path):
    names = [c.name for c in T.cases().values() if c.host]
    vols = [(T.result(n).vol, M.result(n)) for n in names]
    assert {v.color_type for v, _ in vols} == {T.NONE, T.RGB8, T.GRAY32} and sum(len(m.triangles) > 0 for _, m in vols) >= 4
    for R, seed, ctype, zeroed in ((3, 21, T.RGB8, 0.1), (6, 2, T.GRAY32, 1.0 / 3.0), (6, 29, T.NONE, 0.1), (2, 4, T.RGB8, 0.0)):
        v = M.random_volume(R, seed, ctype, zero_weights=zeroed)
        vols.append((v, M.extract_triangle_mesh(v, normals=True)))
        assert len(vols[-1][1].triangles) > 0
    sphere = M.sphere_volume(12, 4.0)
    vols.append((sphere, M.extract_triangle_mesh(sphere, normals=True)))
    lines = [str(len(vols))]
    for v, m in vols:
        lines += volume_lines(v, m)
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    exe = compile_driver("tsdf_mesh_host_driver", tmp_path)
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "mismatches 0" in out.stdout, out.stdout + out.stderr[-4000:]
