"""examples/teaser_python_slam.py on five small frames, dense and scalable: every tracked pose must EQUAL the pose the
numpy restatement of depth odometry (tests/depth_odometry_reference.py) gives for the same frame against the device's own
ray-cast map, chained from the first frame's true pose -- so the drift the example prints is the restatement's drift --
and the script prints one drift line per tracked frame."""
import importlib
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

import depth_odometry_reference as R
from util import ROOT

pytestmark = pytest.mark.gpu
tp = importlib.import_module("teaser-plusplus_amd")
sys.path.insert(0, os.path.join(ROOT, "examples"))

W, H, FRAMES, RES = 96, 72, 5, 64


@pytest.fixture(autouse=True)
def needs_gpu():
    if tp.device_count() < 1:
        pytest.fail("the GPU suite needs an MI355X")


@pytest.mark.parametrize("scalable", [False, True])
def test_the_loop_tracks_five_frames_with_the_restatement_s_poses(scalable, capsys):
    slam = importlib.import_module("teaser_python_slam")
    K, truth, depths, _ = slam.odo.sequence(W, H, FRAMES)
    poses, tracked = slam.track_sequence(K, depths, truth[0], RES, scalable)
    assert len(poses) == FRAMES and len(tracked) == FRAMES - 1
    want = [np.array(truth[0], dtype=np.float64)]
    for k in range(1, FRAMES):
        frame = depths[k].astype(np.float32) / np.float32(1000.0)
        pair = SimpleNamespace(K=(K.fx, K.fy, K.cx, K.cy), source_depth=frame, target_depth=tracked[k - 1].model_depth,
                               depth_scale=1000.0, init=np.eye(4))
        r = R.compute(pair, R.option((10, 5, 3), depth_max=slam.DEPTH_MAX))
        assert r.success and tracked[k - 1].result.iterations == r.iterations
        assert np.array_equal(tracked[k - 1].result.transformation.view(np.uint64), r.transformation.view(np.uint64)), k
        want.append(poses[k - 1] @ r.transformation)   # the loop goes on from the tracked pose
        assert np.array_equal(poses[k].view(np.uint64), want[k].view(np.uint64)), k
        assert slam.drift(poses[k], truth[k]) == slam.drift(want[k], truth[k])
    capsys.readouterr()
    slam.main(["--width", str(W), "--height", str(H), "--frames", str(FRAMES), "--resolution", str(RES)] + (["--scalable"] if scalable else []))
    out = capsys.readouterr().out
    lines = [ln for ln in out.splitlines() if ln.startswith("frame ")]
    assert len(lines) == FRAMES - 1 and all("drift" in ln and "untracked" in ln for ln in lines), out
    for k, ln in enumerate(lines, start=1):   # the printed drift is that of the poses above
        dr, dt = slam.drift(poses[k], truth[k])
        assert ln.startswith("frame %d: drift %.6f deg %.6f m" % (k, dr, dt)), (ln, dr, dt)
    print(out)
