"""examples/teaser_python_raycast.py --scalable on the MI355X at a small size: eight 160 x 120 frames of the analytic
wall-and-balls scene, all but the last integrated into a Gray32 ScalableTSDFVolume with the voxels of the 64^3 cube, the
model ray-cast at the second-to-last pose and odometry of that model frame against the held-out last frame.

The bounds on the model's depth against the analytically rendered depth of the same pose were not picked: the numpy
restatements (tests/stsdf_reference.py and tests/stsdf_raycast_reference.py), whose bits the GPU must return, were run on
the same frames on a CPU and gave 54 blocks and 17695 hit pixels of 19200, all of which the analytic frame sees too, with
a median error of 0.23321533203125 voxel, a 95th percentile of 0.7457880655924469 voxel and a maximum of 5.12 voxels (the
far pixels sit on the balls' silhouettes, where model and frame see different surfaces; the maximum is therefore not
asserted).  As for the dense example (tests/test_gpu_tsdf_raycast_example.py), whose renderer this one shares, the
assertions are the restatement's median plus 0.05 voxel, its 95th percentile plus a quarter voxel and its hit count
within a twentieth.  Frame-to-model odometry must succeed and land nearer the truth than the identity guess."""
import os
import re
import subprocess
import sys

import pytest

from util import ROOT

pytestmark = pytest.mark.gpu
EXAMPLE = os.path.join(ROOT, "examples", "teaser_python_raycast.py")
RESTATEMENT_BLOCKS, RESTATEMENT_HITS, RESTATEMENT_MEDIAN, RESTATEMENT_P95 = 54, 17695, 0.23321533203125, 0.7457880655924469


def test_the_scalable_model_frame_matches_the_scene_and_tracks_the_next_frame():
    out = subprocess.run([sys.executable, EXAMPLE, "--width", "160", "--height", "120", "--resolution", "64", "--frames", "8", "--scalable"],
                         capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stdout + out.stderr
    print(out.stdout)
    blocks = re.search(r"integration: 7 frames of 160 x 120 into (\d+) blocks of 16\^3 voxels", out.stdout)
    hits = re.search(r"ray cast at pose 6: (\d+) of 19200 pixels hit", out.stdout)
    err = re.search(r"model depth against the analytic depth: (\d+) pixels, median ([\d.e+-]+), 95th percentile ([\d.e+-]+),", out.stdout)
    model = re.search(r"frame-to-model odometry: success (\d), rotation error ([\d.e+-]+) deg, translation error ([\d.e+-]+) m", out.stdout)
    frame = re.search(r"frame-to-frame odometry: success (\d),", out.stdout)
    guess = re.search(r"identity guess: rotation error ([\d.]+) deg, translation error ([\d.]+) m", out.stdout)
    assert blocks and hits and err and model and frame and guess, out.stdout
    assert abs(int(blocks.group(1)) - RESTATEMENT_BLOCKS) <= 2, out.stdout  # a millimetre rounded otherwise may touch a block more
    assert abs(int(hits.group(1)) - RESTATEMENT_HITS) < RESTATEMENT_HITS // 20, out.stdout
    assert int(err.group(1)) > RESTATEMENT_HITS * 19 // 20, out.stdout
    assert float(err.group(2)) <= RESTATEMENT_MEDIAN + 0.05 and float(err.group(3)) <= RESTATEMENT_P95 + 0.25, out.stdout
    assert model.group(1) == "1" and frame.group(1) == "1", out.stdout
    assert float(model.group(2)) < float(guess.group(1)) and float(model.group(3)) < float(guess.group(2)), out.stdout
