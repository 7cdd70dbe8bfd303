"""RGB-D odometry on the MI355X against the numpy restatement (tests/odometry_reference.py, pinned by hand in
tests/test_odometry_reference.py): for EVERY case of the shared list the pyramid stage's images, the trace record by
record, success, the transformation, the information matrix and the counts must be EQUAL, compared as integer views.
The same pair gives the same bits alone, first, in the middle and last in a batch of mixed sizes that also holds the
failing pair and the pair without correspondences, and in a second run; the failing pair leaves its neighbours' bits
untouched."""
import importlib

import numpy as np
import pytest

import odometry_reference as R

pytestmark = pytest.mark.gpu
tp = importlib.import_module("teaser-plusplus_amd")


@pytest.fixture(autouse=True)
def needs_gpu():
    if tp.device_count() < 1:
        pytest.fail("the GPU suite needs an MI355X")


def images(pair):
    return (tp.RGBDImage(pair.source_color, pair.source_depth, pair.depth_scale, pair.depth_trunc),
            tp.RGBDImage(pair.target_color, pair.target_depth, pair.depth_scale, pair.depth_trunc))


def option(opt):
    return tp.OdometryOption(opt.iterations, opt.depth_diff_max, opt.depth_min, opt.depth_max)


def jacobian(pair):
    return tp.RGBDOdometryJacobianFromHybridTerm if pair.jacobian == R.HYBRID else tp.RGBDOdometryJacobianFromColorTerm


def intrinsic(pair):
    h, w = pair.source_depth.shape
    return tp.PinholeCameraIntrinsic(w, h, *pair.K)


def run(names, return_trace=True):
    """The cases `names` (which share their options) in one call."""
    cs = [R.cases()[n] for n in names]
    src, tgt = zip(*[images(c.pair) for c in cs])
    return tp.compute_rgbd_odometry_batch(list(src), list(tgt), [intrinsic(c.pair) for c in cs], [c.pair.odo_init for c in cs],
                                          [jacobian(c.pair) for c in cs], option(cs[0].opt), return_trace=return_trace)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def check_result(got, name, trace=True):
    r = R.result(name)
    assert got.success == bool(r.success) and got.count == r.count and got.iterations == r.iterations, \
        (name, got.success, got.count, got.iterations, r.success, r.count, r.iterations)
    if trace:
        assert len(got.trace) == len(r.trace), name
        for k, t in enumerate(r.trace):  # record by record: the first difference names the iteration where it starts
            where = (name, "iteration", k, "level", t["level"])
            assert (got.trace.level[k], got.trace.executed[k], got.trace.count[k], got.trace.failed[k]) == \
                (t["level"], t["executed"], t["count"], t["failed"]), where
            assert same(got.trace.e[k], np.float64(t["e"])), where + ("e", got.trace.e[k], t["e"])
            assert same(got.trace.A[k], t["A"]) and same(got.trace.g[k], t["g"]), where + ("sums",)
            assert same(got.trace.pose[k].ravel(), t["pose"]), where + ("pose",)
    assert same(got.transformation, r.transformation), (name, got.transformation, r.transformation)
    assert same(got.information, r.information), (name, got.information, r.information)


@pytest.mark.parametrize("name", list(R.cases()))
def test_the_pyramid_stage_equals_the_restatement(name):
    cs = R.cases()[name]
    src, tgt = images(cs.pair)
    levels = tp.rgbd_odometry_pyramid_batch([src], [tgt], intrinsic(cs.pair), cs.pair.odo_init, option(cs.opt))[0]
    ref = R.result(name).levels
    assert len(levels) == len(ref)
    for l, (got, want) in enumerate(zip(levels, ref)):
        for plane in ("I_s", "I_t", "D_s", "D_t", "I_t_dx", "I_t_dy", "D_t_dx", "D_t_dy"):
            bad = np.flatnonzero(bits(got[plane]).ravel() != bits(want[plane]).ravel())
            assert len(bad) == 0, (name, l, plane, len(bad), bad[:5], got[plane].ravel()[bad[:5]], want[plane].ravel()[bad[:5]])
        assert same(got["XYZ"], np.stack([want["X"], want["Y"], want["Z"]], axis=2)), (name, l, "XYZ")


@pytest.mark.parametrize("name", list(R.cases()))
def test_a_pair_alone_equals_the_restatement(name):
    check_result(run([name])[0], name)


# cases that share the options (3, 2, 2): mixed sizes, formats and Jacobians
MIXED = ["37x29", "8x8", "no_correspondence", "f32_specials", "4x4", "big_init"]


def test_the_same_bits_at_any_position_of_a_batch_and_run_after_run():
    assert len({R.cases()[n].opt.iterations for n in MIXED}) == 1
    for order in (MIXED, MIXED[::-1], MIXED[2:] + MIXED[:2]):
        for _ in range(2):
            for got, name in zip(run(order), order):
                check_result(got, name)
    # without the trace the results are the same
    for got, name in zip(run(MIXED, return_trace=False), MIXED):
        assert got.trace is None
        check_result(got, name, trace=False)


def test_a_failing_pair_leaves_its_neighbours_untouched():
    """The textureless pair (singular under the colour term) in front of, between and behind two pairs that succeed."""
    for order in (["block", "singular", "block-1"], ["singular", "block-1", "block"], ["block-1", "block", "singular"]):
        res = run(order)
        for got, name in zip(res, order):
            check_result(got, name)
    failed = run(["block", "singular", "block-1"])[1]
    assert not failed.success and same(failed.transformation, np.eye(4)) and not failed.information.any()
    assert failed.trace.failed[0] == 1 and not failed.trace.executed[1:].any()


def test_no_iteration_returns_the_initial_pose_with_its_information():
    got = run(["no_iteration"])[0]
    cs = R.cases()["no_iteration"]
    assert got.success and got.iterations == 0 and len(got.trace) == 0 and same(got.transformation, cs.pair.odo_init)
    assert got.count > 0 and got.information[3, 3] == got.count
    check_result(got, "no_iteration")


def test_the_single_pair_call_and_the_refusals():
    cs = R.cases()["37x29"]
    src, tgt = images(cs.pair)
    ok, trans, info = tp.compute_rgbd_odometry(src, tgt, intrinsic(cs.pair), cs.pair.odo_init, jacobian(cs.pair), option(cs.opt))
    r = R.result("37x29")
    assert ok and same(trans, r.transformation) and same(info, r.information)
    assert tp.compute_rgbd_odometry_batch([], [], intrinsic(cs.pair)) == []
    K = np.array([[0.0, 0, 1], [0, 1.0, 1], [0, 0, 1]])
    with pytest.raises(ValueError, match="fx and fy"):
        tp.compute_rgbd_odometry(src, tgt, K)
    # the C entry's own refusal, with the pair named, and the handle usable afterwards
    from importlib import import_module
    odo = import_module("teaser-plusplus_amd.odometry")
    b, recs, opt, ptrs, keep = odo._pairs([src, src], [tgt, tgt], intrinsic(cs.pair), None, tp.RGBDOdometryJacobianFromHybridTerm, option(cs.opt))
    recs[1].target_width += 1
    res = (odo.OdometryResultC * 2)()
    with pytest.raises(tp.TeaserHipError, match=r"differ in size \(pair 1\)"):
        odo._handle(-1).call(tp.lib().teaser_hip_icp_rgbd_odometry_batch, 2, recs, opt, *ptrs, res, None)
    check_result(run(["37x29"])[0], "37x29")
