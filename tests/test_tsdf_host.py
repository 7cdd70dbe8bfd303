"""The host side of the TSDF volume without a GPU: csrc/tsdf.hip compiled by g++ against the HIP stand-in header with CPU
stand-ins for the launchers, which call the functions of csrc/tsdf_device.h -- the text the kernels compile --
(tests/tsdf_host_driver.cpp).  Built with -ffp-contract=off under AddressSanitizer and UndefinedBehaviorSanitizer and run
as a stand-alone program.  Validation, frame records, the packing of padded rows, the chunks of frames, the z segments,
the device layout, download and upload, the extraction buffers, the capacity rule and every refusal run for real; voxels,
counts, points, normals and colours are compared for equality with the restatement's."""
import subprocess

import numpy as np

import tsdf_reference as T
from test_outlier_host import hexes, ints
from test_search_host import compile_driver


def image_numbers(a):
    if a is None or a.size == 0:
        return ""
    return ints(a) if a.dtype.kind == "u" else hexes(a)


def row_padding(a, pixel_bytes):
    return 0 if a is None or a.size == 0 else a.strides[0] - a.shape[1] * pixel_bytes


def case_lines(cs):
    length, R, trunc, ctype, origin = cs.vol
    r = T.result(cs.name)
    lines = ["%d %d %d" % (R, ctype, len(cs.frames)), hexes([length, trunc]) + " " + hexes(origin)]
    for f in cs.frames:
        h, w = f.depth.shape
        cfmt = {T.NONE: 0, T.RGB8: 1, T.GRAY32: 2}[ctype]
        lines += ["%d %d %d %d %d %d" % (w, h, 0 if f.depth.dtype == np.uint16 else 1, cfmt,
                                         row_padding(f.depth, f.depth.itemsize), row_padding(f.color, {0: 0, 1: 3, 2: 4}[cfmt])),
                  hexes(f.K) + " " + hexes(f.E) + " " + hexes([f.depth_scale, f.depth_trunc]),
                  image_numbers(f.depth), image_numbers(f.color)]
    lines += [hexes(r.tw), hexes(r.color) if ctype else "", str(len(r.points)), hexes(r.points), hexes(r.normals),
              hexes(r.colors) if ctype else "", str(len(r.vpoints)), hexes(r.vpoints), hexes(r.vcolors)]
    return lines


def test_host_code_is_clean_and_equal_to_the_restatement(tmp_path):
    cs = [c for c in T.cases().values() if c.host]
    assert {c.vol[3] for c in cs} == {T.NONE, T.RGB8, T.GRAY32} and any(len(c.frames) > T.CHUNK for c in cs)
    lines = [str(len(cs))]
    for c in cs:
        lines += case_lines(c)
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    exe = compile_driver("tsdf_host_driver", tmp_path)
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "mismatches 0" in out.stdout, out.stdout + out.stderr[-4000:]
