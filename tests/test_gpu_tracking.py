"""track_frame_to_model on the MI355X: a frame of the analytic scene tracked against a dense volume of 64^3 voxels and
against the same scene in a scalable volume.  The device's own ray-cast depth map is handed to the numpy restatement of
depth odometry (tests/depth_odometry_reference.py) with the frame as source and the identity as init: the result must
EQUAL it, and the pose must be camera_to_world_init @ T.  A Gray32 volume and a volume without colour are tracked
against -- the photometric route (as_rgbd_image) needs a colour the second one does not have."""
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

W, H, RES = 96, 72, 64
_scene = None


@pytest.fixture(autouse=True)
def needs_gpu():
    if tp.device_count() < 1:
        pytest.fail("the GPU suite needs an MI355X")


def scene():
    """(the example module, intrinsic, true poses, depth frames, intensity frames), rendered once."""
    global _scene
    if _scene is None:
        slam = importlib.import_module("teaser_python_slam")
        _scene = (slam,) + tuple(slam.odo.sequence(W, H, 3))
    return _scene


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def restated(frame_u16, model_depth, K, option):
    """The restatement's result for the frame (as the float32 metres the call forms) against the device's model view."""
    frame = frame_u16.astype(np.float32) / np.float32(1000.0)
    pair = SimpleNamespace(K=(K.fx, K.fy, K.cx, K.cy), source_depth=frame, target_depth=model_depth, depth_scale=1000.0, init=np.eye(4))
    return R.compute(pair, R.option((10, 5, 3), depth_max=option.depth_max))


@pytest.mark.parametrize("scalable", [False, True])
@pytest.mark.parametrize("color_type", ["NoColor", "Gray32"])
def test_the_tracked_pose_is_init_times_the_restatement_s_motion(scalable, color_type):
    slam, K, truth, depths, paints = scene()
    ct = getattr(tp.TSDFVolumeColorType, color_type)
    length, res, trunc, origin = slam.fusion.volume_settings(RES)
    vol = tp.ScalableTSDFVolume(length / res, trunc, ct) if scalable else tp.UniformTSDFVolume(length, res, trunc, ct, origin)
    option = slam.tracking_option()
    with vol:
        vol.integrate_batch(depths[:2], K, [np.linalg.inv(p) for p in truth[:2]], paints[:2] if color_type == "Gray32" else None,
                            depth_scale=1000.0, depth_trunc=slam.DEPTH_MAX)
        init = truth[1]
        tr = tp.track_frame_to_model(vol, depths[2], K, init, option, weight_threshold=1.0)
        if color_type == "NoColor":  # the photometric route has nothing to track against
            with pytest.raises(ValueError, match="no colour"):
                tp.ray_cast(vol, K, np.linalg.inv(init), W, H, depth_max=slam.DEPTH_MAX, weight_threshold=1.0).as_rgbd_image()
    assert tr.model_depth.shape == (H, W) and tr.model_depth.dtype == np.float32 and (tr.model_depth > 0).sum() > W * H // 2
    want = restated(depths[2], tr.model_depth, K, option)
    got = tr.result
    assert (got.success, got.count, got.iterations, got.converged_levels) == (bool(want.success), want.count, want.iterations, want.converged_levels)
    assert np.array_equal(bits(got.transformation), bits(want.transformation))
    assert np.array_equal(bits(got.information), bits(want.information))
    assert got.fitness == want.fitness and got.inlier_rmse == want.inlier_rmse
    assert got.success and tr.success
    # the pose: camera_to_world_init @ T, T taking the frame's camera to the camera of the initial pose
    assert np.array_equal(bits(tr.camera_to_world), bits(np.array(init, dtype=np.float64) @ want.transformation))
    d_tracked, d_held = slam.drift(tr.camera_to_world, truth[2]), slam.drift(init, truth[2])
    print("scalable %d %s: drift %.6f deg %.6f m, untracked %.6f deg %.6f m, %d iterations" %
          ((scalable, color_type) + d_tracked + d_held + (got.iterations,)))
