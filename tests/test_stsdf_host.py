"""The host side of the scalable TSDF volume without a GPU: csrc/stsdf.hip compiled by g++ against the HIP stand-in header
with CPU stand-ins for the launchers, which call the functions of csrc/stsdf_device.h and csrc/tsdf_device.h -- the text
the kernels compile -- (tests/stsdf_host_driver.cpp).  Built with -ffp-contract=off under AddressSanitizer and
UndefinedBehaviorSanitizer and run as a stand-alone program.  Validation, the inverse of the extrinsic, the touch
records, the expansion of the candidates, the directory merge, the slabs and their growth, the passes and their frame
masks, download and upload of blocks, the capacity rule, max_blocks and every refusal run for real; keys, voxels,
counts, points, normals and colours are compared for equality with the restatement's."""
import subprocess

import numpy as np

import stsdf_reference as S
from test_outlier_host import hexes, ints
from test_search_host import compile_driver
from test_tsdf_host import image_numbers, row_padding


def case_lines(cs):
    r = S.result(cs.name)
    ctype = cs.ctype
    lines = ["%d %d %d" % (ctype, cs.stride, len(cs.frames)), hexes([cs.vl, cs.trunc])]
    for f in cs.frames:
        h, w = f.depth.shape
        cfmt = {S.NONE: 0, S.RGB8: 1, S.GRAY32: 2}[ctype]
        color = f.color if ctype else None
        lines += ["%d %d %d %d %d %d" % (w, h, 0 if f.depth.dtype == np.uint16 else 1, cfmt,
                                         row_padding(f.depth, f.depth.itemsize), row_padding(color, {0: 0, 1: 3, 2: 4}[cfmt])),
                  hexes(f.K) + " " + hexes(f.E) + " " + hexes([f.depth_scale, f.depth_trunc]),
                  image_numbers(f.depth), image_numbers(color)]
    lines += [str(len(r.keys)), ints(r.keys), hexes(r.tw), hexes(r.color) if ctype else "", str(len(r.points)), hexes(r.points),
              hexes(r.normals), hexes(r.colors) if ctype else "", str(len(r.vpoints)), hexes(r.vpoints), hexes(r.vcolors),
              "%d %d %d" % (r.touched, r.opened, r.out_of_range)]
    return lines


def test_host_code_is_clean_and_equal_to_the_restatement(tmp_path):
    cs = [c for c in S.cases().values() if c.host]
    assert {c.ctype for c in cs} == {S.NONE, S.RGB8, S.GRAY32} and any(len(c.frames) > S.CHUNK for c in cs)
    assert any(S.result(c.name).out_of_range > 0 for c in cs) and any(len(S.result(c.name).keys) == 0 for c in cs)
    lines = [str(len(cs))]
    for c in cs:
        lines += case_lines(c)
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    exe = compile_driver("stsdf_host_driver", tmp_path)
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "mismatches 0" in out.stdout, out.stdout + out.stderr[-4000:]
