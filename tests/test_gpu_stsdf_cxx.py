"""tests/cxx/stsdf_example.cpp on the MI355X: teaser::ScalableTSDFVolume of include/teaser/tsdf.h on two frames given by
formulas, and the record the example prints -- counts and FNV-1a hashes of the bytes of every output -- against the numpy
restatement (tests/stsdf_reference.py) on the same frames."""
import re
import subprocess

import numpy as np
import pytest

import stsdf_reference as S
import tsdf_reference as T
from stsdf_cxx import build_stsdf_example
from test_gpu_tsdf_cxx import fixture_frames, fnv, tp

pytestmark = pytest.mark.gpu


def test_cxx_example_prints_the_record_of_the_restatement():
    if tp.device_count() < 1:
        pytest.fail("the GPU suite needs an MI355X")
    exe = build_stsdf_example()
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "checks 1" in out.stdout, out.stdout + out.stderr
    rec = dict(re.findall(r"^(\w+) (\w+)$", out.stdout, flags=re.M))
    depths, colors, K, E = fixture_frames()
    vol = S.ScalableVolume(0.0625, 0.15, S.RGB8, 4)
    for d, c, e in zip(depths, colors, E):
        vol.integrate(T.frame(d, (K.fx, K.fy, K.cx, K.cy), e, c))
    points, normals, pcolors, _ = vol.extract_point_cloud()
    vpoints, vcolors = vol.extract_voxel_point_cloud()
    assert len(vol.blocks) > 1 and len(points) > 0
    want = dict(blocks=str(len(vol.blocks)), touched=str(vol.touched), opened=str(vol.opened), keys=fnv(vol.keys()),
                count=str(len(points)), points=fnv(points), normals=fnv(normals), colors=fnv(pcolors), vcount=str(len(vpoints)),
                vpoints=fnv(vpoints), vcolors=fnv(vcolors), checks="1")
    assert rec == want, (rec, want)
