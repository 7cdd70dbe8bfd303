"""Depth odometry on the MI355X against the numpy restatement (tests/depth_odometry_reference.py, pinned by hand in
tests/test_depth_odometry_reference.py): for EVERY case of the shared list -- pixel counts at the block edge (255, 256,
257), at the group edge (64 blocks of 256 less one row, exactly, plus one row), more than eight groups for the finishing
kernel's slots, a last level of 2 x 1, both depth formats, padded rows -- every plane of the pyramid stage, the trace
record by record, success, the transformation, the information matrix, the measures and the counts must be EQUAL,
compared as integer views.  The same pair gives the same bits alone, at any position of a batch of mixed sizes that also
holds the pair that fails at count 0 and the pair that converges early, run after run, in a call of 320 pairs, and
whatever the handle's scratch held before."""
import ctypes as C
import importlib

import numpy as np
import pytest

import depth_odometry_reference as R

pytestmark = pytest.mark.gpu
tp = importlib.import_module("teaser-plusplus_amd")
odo = importlib.import_module("teaser-plusplus_amd.odometry")


@pytest.fixture(autouse=True)
def needs_gpu():
    if tp.device_count() < 1:
        pytest.fail("the GPU suite needs an MI355X")


def option(opt, depth_scale=1000.0):
    crit = [tp.OdometryConvergenceCriteria(n, opt.relative_rmse, opt.relative_fitness) for n in opt.iterations]
    return tp.DepthOdometryOption(crit, tp.OdometryLossParams(opt.trunc, opt.delta), depth_scale, opt.depth_min, opt.depth_max)


def intrinsic(pair):
    h, w = pair.source_depth.shape
    return tp.PinholeCameraIntrinsic(w, h, *pair.K)


def run(names, return_trace=True):
    """The cases `names` (which share their options) in one call."""
    cs = [R.cases()[n] for n in names]
    assert len({(c.opt.iterations, c.opt.trunc, c.opt.delta, c.opt.depth_min, c.opt.depth_max, c.opt.relative_rmse,
                 c.opt.relative_fitness) for c in cs}) == 1
    return tp.compute_depth_odometry_batch([c.pair.source_depth for c in cs], [c.pair.target_depth for c in cs],
                                           [intrinsic(c.pair) for c in cs], [c.pair.init for c in cs], option(cs[0].opt),
                                           return_trace=return_trace)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def check_result(got, name, trace=True):
    r = R.result(name)
    assert (got.success, got.count, got.iterations, got.converged_levels) == (bool(r.success), r.count, r.iterations, r.converged_levels), \
        (name, got.success, got.count, got.iterations, got.converged_levels, r.success, r.count, r.iterations, r.converged_levels)
    if trace:
        assert len(got.trace) == len(r.trace), name
        for k, t in enumerate(r.trace):  # record by record: the first difference names the iteration where it starts
            where = (name, "iteration", k, "level", t["level"])
            assert (got.trace.level[k], got.trace.executed[k], got.trace.count[k], got.trace.failed[k], got.trace.converged[k]) == \
                (t["level"], t["executed"], t["count"], t["failed"], t["converged"]), where
            assert same(got.trace.e[k], np.float64(t["e"])), where + ("e", got.trace.e[k], t["e"])
            assert same(got.trace.A[k], t["A"]) and same(got.trace.g[k], t["g"]), where + ("sums",)
            assert same(got.trace.pose[k].ravel(), t["pose"]), where + ("pose",)
    assert same(got.transformation, r.transformation), (name, got.transformation, r.transformation)
    assert same(got.information, r.information), (name, got.information, r.information)
    assert same(np.float64(got.fitness), np.float64(r.fitness)) and same(np.float64(got.inlier_rmse), np.float64(r.inlier_rmse)), \
        (name, got.fitness, r.fitness, got.inlier_rmse, r.inlier_rmse)


def flat_levels(levels):
    out = []
    for lev in levels:
        out += [lev["D_s"].ravel(), lev["D_t"].ravel()]
        for name in ("source_vertex", "target_vertex", "target_normal"):
            out += [lev[name][:, :, c].ravel() for c in range(3)]
    return np.concatenate(out)


@pytest.mark.parametrize("name", list(R.cases()))
def test_the_pyramid_call_alone_equals_the_restatement(name):
    cs = R.cases()[name]
    levels = tp.depth_odometry_pyramid_batch([cs.pair.source_depth], [cs.pair.target_depth], intrinsic(cs.pair), option(cs.opt))[0]
    ref = R.result(name).levels
    assert len(levels) == len(ref)
    got, want = flat_levels(levels), R.pyramid(name)
    at = 0
    for l, lev in enumerate(ref):   # plane by plane: the first difference names the level and the plane
        n = lev["D_s"].size
        for plane in R.PLANES:
            bad = np.flatnonzero(bits(got[at:at + n]) != bits(want[at:at + n]))
            assert len(bad) == 0, (name, l, plane, len(bad), bad[:5], got[at:at + n][bad[:5]], want[at:at + n][bad[:5]])
            at += n
    assert at == len(got) == len(want)


@pytest.mark.parametrize("name", list(R.cases()))
def test_a_pair_alone_equals_the_restatement(name):
    check_result(run([name])[0], name)


# cases that share the options (3, 2, 2): mixed sizes and formats, padded rows, the pair that fails at count 0
MIXED = ["37x29", "8x8", "all_invalid", "f32_specials", "37x29"]


def test_the_same_bits_at_any_position_of_a_batch_and_run_after_run():
    first = None
    for order in (MIXED, MIXED[::-1], MIXED[2:] + MIXED[:2]):
        for _ in range(2):
            res = run(order)
            for got, name in zip(res, order):
                check_result(got, name)
            if order is MIXED:
                raw = [(bits(g.transformation).copy(), bits(g.information).copy(), bits(g.trace.A).copy()) for g in res]
                assert first is None or all(np.array_equal(x, y) for a, b in zip(first, raw) for x, y in zip(a, b))
                first = raw
    for got, name in zip(run(MIXED, return_trace=False), MIXED):
        assert got.trace is None
        check_result(got, name, trace=False)


def test_a_pair_that_fails_at_count_zero_leaves_its_neighbours_untouched():
    for order in (["37x29", "all_invalid", "8x8"], ["all_invalid", "8x8", "37x29"], ["8x8", "37x29", "all_invalid"]):
        for got, name in zip(run(order), order):
            check_result(got, name)
    failed = run(["37x29", "all_invalid", "8x8"])[1]
    assert not failed.success and failed.count == 0 and same(failed.transformation, np.eye(4)) and not failed.information.any()
    assert failed.trace.failed[0] == 1 and not failed.trace.executed[1:].any()


def test_a_pair_that_converges_early_beside_one_that_does_not():
    """A moving pair, the still pair (identical images: its rmse is 0, and 0 <= threshold x 0 holds for any threshold)
    and the moving pair again share a call of (3, 3, 3) iterations, first under the thresholds 10 and 10, which any two
    iterations meet, then under a negative relative_rmse, which no moving pair meets: there the still pair stops at every
    level's second iteration between two neighbours that run all nine."""
    cs = R.cases()
    early, never = cs["converges_early"], cs["never_converges"]
    for o in (early.opt, never.opt):
        pairs = [early.pair, cs["converges"].pair, early.pair]
        res = tp.compute_depth_odometry_batch([p.source_depth for p in pairs], [p.target_depth for p in pairs],
                                              [intrinsic(p) for p in pairs], None, option(o), return_trace=True)
        want = [R.compute(p, o) for p in pairs]
        for g, w in zip(res, want):
            assert (g.success, g.count, g.iterations, g.converged_levels) == (bool(w.success), w.count, w.iterations, w.converged_levels)
            assert list(g.trace.executed) == [t["executed"] for t in w.trace]
            assert list(g.trace.converged) == [t["converged"] for t in w.trace]
            assert same(g.transformation, w.transformation) and same(g.information, w.information)
    # under the negative threshold the moving pair ran all nine iterations beside the still pair, which stopped early
    assert res[0].iterations == 9 and res[0].converged_levels == 0 and res[1].iterations == 6 and res[1].converged_levels == 7
    check_result(run(["converges_early"])[0], "converges_early")
    check_result(run(["never_converges"])[0], "never_converges")
    check_result(run(["converges"])[0], "converges")


def test_320_tiny_pairs_in_one_call():
    cycle = ("8x8", "37x29", "all_invalid", "f32_specials")
    names = [cycle[i % len(cycle)] for i in range(320)]
    res = run(names, return_trace=False)
    assert len(res) == 320
    for i, (got, name) in enumerate(zip(res, names)):
        check_result(got, name, trace=False)


@pytest.mark.parametrize("byte", [0x00, 0xFF, 0x3F])
def test_the_call_does_not_read_what_its_scratch_held(byte):
    """Every buffer of the ICP handle filled with one byte in front of the call: a small call
    after a larger one, so that the buffers are larger than the call needs."""
    run(["group+1"], return_trace=False)
    assert tp.fill_scratch("icp", byte) > 0
    for got, name in zip(run(MIXED), MIXED):
        check_result(got, name)
    assert tp.fill_scratch("icp", byte) > 0
    cs = R.cases()["9x5"]
    levels = tp.depth_odometry_pyramid_batch([cs.pair.source_depth], [cs.pair.target_depth], intrinsic(cs.pair), option(cs.opt))[0]
    assert np.array_equal(bits(flat_levels(levels)), bits(R.pyramid("9x5")))


def test_the_single_pair_call_and_the_refusals():
    cs = R.cases()["37x29"]
    r = R.result("37x29")
    got = tp.compute_depth_odometry(cs.pair.source_depth, cs.pair.target_depth, intrinsic(cs.pair), cs.pair.init, option(cs.opt))
    ok, trans, info, fitness, rmse = got
    assert ok and same(trans, r.transformation) and same(info, r.information) and fitness == r.fitness and rmse == r.inlier_rmse
    assert tp.compute_depth_odometry_batch([], [], intrinsic(cs.pair)) == []
    # the C entry's own refusal, with the pair named, and the handle usable afterwards
    s, t = cs.pair.source_depth, cs.pair.target_depth
    b, recs, opt, ptrs, keep = odo._depth_pairs([s, s], [t, t], intrinsic(cs.pair), None, option(cs.opt))
    recs[1].depth_format = 2
    res = (odo.DepthOdometryResultC * 2)()
    with pytest.raises(tp.TeaserHipError, match=r"depth_format must be 0 \(uint16\) or 1 \(float32\) \(pair 1\)"):
        odo._handle(-1).call(tp.lib().teaser_hip_icp_depth_odometry_pairs, 2, recs, C.byref(opt), *ptrs, res, None)
    recs[1].depth_format = 0
    opt.depth_huber_delta = 0.0
    with pytest.raises(tp.TeaserHipError, match="depth_huber_delta must be finite and > 0"):
        odo._handle(-1).call(tp.lib().teaser_hip_icp_depth_odometry_pairs, 2, recs, C.byref(opt), *ptrs, res, None)
    check_result(run(["37x29"])[0], "37x29")
