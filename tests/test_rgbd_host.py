"""The host side of the depth-frame calls without a GPU: csrc/icp_rgbd.hip compiled by g++ against the HIP stand-in
header with CPU stand-ins for the two launchers, which call the functions of csrc/icp_rgbd_device.h -- the text the
kernels compile -- (tests/rgbd_host_driver.cpp).  Built with -ffp-contract=off under AddressSanitizer and
UndefinedBehaviorSanitizer and run as a stand-alone program.  Validation, descriptors, the packing of padded rows, the
tile and block maps, the output layouts, the optional outputs, the empty frames, the copy back and every refusal run for
real; points, colours, pixels, counts and the three images are compared for equality with the restatement's."""
import subprocess

import numpy as np

import rgbd_reference as R
from test_outlier_host import hexes, ints
from test_search_host import compile_driver


def image_numbers(a):
    if a is None or a.size == 0:
        return ""
    return ints(a) if a.dtype.kind == "u" else hexes(a)


def row_padding(a, pixel_bytes):
    return 0 if a is None or a.size == 0 else a.strides[0] - a.shape[1] * pixel_bytes


def unproject_lines(depth, color, f):
    h, w = depth.shape
    fmt = R.color_format(color)
    count, P, C, pix = R.unproject(depth, color, f)
    assert P.shape == (count, 3) and pix.shape == (count,) and (C is None or C.shape == (count, 3))
    head = "%d %d %d %d %d %d %d %d %d" % (w, h, 0 if depth.dtype == np.uint16 else 1, fmt, f.intensity, f.stride,
                                          f.valid_only, row_padding(depth, depth.itemsize),
                                          row_padding(color, {0: 0, 1: 3, 2: 4, 3: 12}[fmt]))
    cam = hexes([f.fx, f.fy, f.cx, f.cy]) + " " + hexes(f.pose) + " " + hexes([f.depth_scale, f.depth_trunc])
    return [head, cam, image_numbers(depth), image_numbers(color), str(count), hexes(P), hexes(C) if fmt else "", ints(pix)]


def project_lines(P, C, cam):
    depth, cimg, index, n_hit = R.project(P, C, cam)
    assert depth.shape == index.shape == (cam.height, cam.width)
    head = "%d %d %d %d" % (len(P), int(C is not None), cam.width, cam.height)
    rec = hexes([cam.fx, cam.fy, cam.cx, cam.cy]) + " " + hexes(cam.extrinsic) + " " + hexes([cam.depth_scale, cam.depth_max])
    return [head, rec, hexes(P), hexes(C) if C is not None else "", str(n_hit), hexes(depth), ints(index),
            hexes(cimg) if C is not None else ""]


def test_host_code_is_clean_and_equal_to_the_restatement(tmp_path):
    us, ps = R.unproject_cases(), R.project_cases()
    lines = ["%d %d" % (len(us), len(ps))]
    for _, depth, color, f in us:
        lines += unproject_lines(depth, color, f)
    for _, P, C, cam in ps:
        lines += project_lines(P, C, cam)
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    exe = compile_driver("rgbd_host_driver", tmp_path)
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "mismatches 0" in out.stdout, out.stdout + out.stderr[-4000:]
