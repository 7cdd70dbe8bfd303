"""The host side of the ray-casting scene without a GPU: csrc/scene.hip compiled by g++ against the HIP stand-in header
with CPU stand-ins for the launchers, which call the functions of csrc/scene_device.h -- the text the kernels compile --
(tests/scene_host_driver.cpp): the hierarchy node by node, the refit pass by pass and both traversals lane by lane.
Built with -ffp-contract=off under AddressSanitizer and UndefinedBehaviorSanitizer and run as a stand-alone program.
Validation, every refusal with its text, the layouts, the rebuild after a further geometry and equality of every output
with the restatement run for real; nothing is loaded into Python under a sanitizer."""
import pathlib
import struct
import subprocess
import tempfile

import numpy as np

import scene_reference as R
from test_search_host import compile_driver


def bits(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.float32:
        a = a.view(np.uint32)
    return " ".join(str(int(x)) for x in a.astype(np.uint32).ravel())


def real(x):
    hi, lo = struct.unpack(">II", struct.pack(">d", float(x)))
    return "%d %d" % (hi, lo)


def maps(r, key, closest=False):
    out = [bits(r[key]), bits(r["geometry_ids"]), bits(r["primitive_ids"]), bits(r["primitive_uvs"]), bits(r["primitive_normals"])]
    if closest:
        out.append(bits(r["points"]))
    return out


def case_lines(name, views):
    geoms, rays, pts, _ = R.cases()[name]
    T = R.Triangles(geoms)
    hit, near = R.expected(name)
    lines = [str(len(geoms))]
    for vert, tri in geoms:
        lines += ["%d %d" % (len(vert), len(tri)), bits(np.asarray(vert, dtype=np.float32)), bits(np.asarray(tri, dtype=np.uint32))]
    lines += [str(len(rays)), bits(rays)] + maps(hit, "t_hit")
    t = hit["t_hit"][np.isfinite(hit["t_hit"])]
    tnear, tfar = (float(np.median(t)), float(np.max(t))) if len(t) else (0.0, 1.0)  # tnear == t exactly for one ray at least
    lines += [real(tnear) + " " + real(tfar), bits(R.test_occlusions(T, rays, tnear, tfar).astype(np.uint32))]
    lines += [str(len(pts)), bits(pts)] + maps(near, "distance", closest=True)
    lines.append(str(len(views)))
    for b, (K, E, w, h) in enumerate(views):
        off = 0.5 if b % 2 == 0 else 0.0
        lines.append("%d %d %s %s" % (w, h, " ".join(real(x) for x in (K[0, 0], K[1, 1], K[0, 2], K[1, 2])),
                                      " ".join(real(x) for x in np.asarray(E).ravel())) + " " + real(off))
        lines += maps(R.cast_rays(T, R.create_rays_pinhole(K, E, w, h, off).reshape(-1, 6)), "t_hit")
    return lines


def test_host_code_is_clean_and_equal_to_the_restatement(tmp_path):
    names = [n for n, c in R.cases().items() if c[3]]
    assert {"small0", "small1", "duplicates", "line", "lattice", "offset", "axis_aligned", "dead", "mixed_sizes"} <= set(names)
    hit, near = R.expected("lattice")
    assert np.isinf(hit["t_hit"]).any() and (hit["t_hit"] == 0).any() and (near["distance"] == 0).any()
    lines = [str(len(names))]
    for n in names:
        lines += case_lines(n, R.views_case() if n in ("lattice", "small0") else [])
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    exe = compile_driver("scene_host_driver", pathlib.Path(tempfile.mkdtemp(prefix="scene_driver_")))
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "mismatches 0" in out.stdout, out.stdout + out.stderr[-4000:]
