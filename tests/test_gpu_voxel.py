"""Batched voxel down-sampling on the MI355X against the numpy restatement of the contract (tests/voxel_reference.py):
bit-identical means, counts and voxel_of_point for every case; a problem inside a batch gives the same bits as alone
and as the last run; invalid arguments are refused with the argument named and leave the handle usable."""
import ctypes as C
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import voxel_reference as R
from util import ROOT

pytestmark = pytest.mark.gpu
tp = importlib.import_module("teaser-plusplus_amd")
CROP = os.path.join(ROOT, "tests", "golden", "voxel_crop.npz")


@pytest.fixture(scope="module", autouse=True)
def _device():
    if tp.device_count() < 1:
        pytest.fail("the GPU suite needs an MI355X")


def gpu(points, v):
    return tp.voxel_down_sample(points, v, return_counts=True, return_trace=True)


def assert_bits(got, ref):
    means, counts, trace = got
    assert means.shape == ref[0].shape
    assert means.tobytes() == ref[0].tobytes()
    assert np.array_equal(counts, ref[1])
    assert np.array_equal(trace, ref[2])


def check(points, v):
    points = np.asarray(points, dtype=np.float64)
    got = gpu(points, v)
    assert_bits(got, R.voxel_down_sample(points, v))
    return got


def test_crop_fixture():
    g = np.load(CROP)
    got = check(g["points"].astype(np.float64), float(g["voxel_size"]))
    assert_bits(got, (g["means"], g["counts"], g["trace"]))


def test_scan_like_cloud():
    p = R.scan_like()
    means, counts, _ = check(p, 0.05)
    assert 2000 < len(means) < 100000 and counts.max() > 64  # both summation paths run


def test_uniform_cloud():
    check(np.random.default_rng(2).uniform(-1, 1, size=(200000, 3)), 0.05)


def test_far_from_the_origin():
    """At 1e5 the rounding of p - lo decides voxels: the GPU must round exactly as the contract does."""
    check(R.scan_like(seed=9, n=100000, offset=1e5), 0.05)
    check(np.random.default_rng(3).uniform(1e5, 1e5 + 1, size=(50000, 3)), 0.01)


def test_points_exactly_on_faces():
    v = 0.5
    rng = np.random.default_rng(4)
    # min_bound 0 -> lo = -0.25: every x = 0.25 + 0.5 k is a face; mix faces, centres and random coordinates
    faces = 0.25 + 0.5 * rng.integers(0, 20, size=(20000, 3))
    centres = 0.5 * rng.integers(0, 20, size=(20000, 3))
    mixed = np.where(rng.random((20000, 3)) < 0.5, faces, rng.uniform(0, 10, size=(20000, 3)))
    p = np.concatenate([[[0.0, 0.0, 0.0]], faces, centres, mixed])
    idx = R.voxel_indices(p, v)
    assert np.array_equal(idx[1:20001], (faces + 0.25) / 0.5)  # the faces land in the upper voxel
    check(p, v)


def test_one_voxel_holds_100k_points():
    p = np.random.default_rng(6).uniform(0, 0.49, size=(100000, 3))
    means, counts, trace = check(p, 1.0)
    assert counts.tolist() == [100000] and not trace.any()


def test_every_point_in_its_own_voxel():
    rng = np.random.default_rng(7)
    g = rng.permutation(np.stack(np.meshgrid(np.arange(40), np.arange(40), np.arange(40), indexing="ij"), -1)
                        .reshape(-1, 3))
    p = g.astype(np.float64) + rng.uniform(-0.2, 0.2, size=g.shape)
    means, counts, trace = check(p, 1.0)
    assert len(means) == len(p) and (counts == 1).all()


def test_empty_and_single_point():
    means, counts, trace = gpu(np.zeros((0, 3)), 0.05)
    assert means.shape == (0, 3) and len(counts) == 0 and len(trace) == 0
    p = np.array([[1.2345678901234567, -9.87654321e-3, 4.5e7]])
    means, counts, trace = check(p, 0.05)
    assert means.tobytes() == p.tobytes()


def test_wide_grid_takes_the_second_sort_pass():
    """More than 2^21 voxels per axis: 3 x 22 bits of key do not fit in 64, so the sort runs a second LSD pass."""
    rng = np.random.default_rng(8)
    p = rng.uniform(0, 5e6, size=(30000, 3))
    p[:10000] = p[:10000].round()  # exact faces among them
    p = np.concatenate([p, p[:5000] + 0.25])  # voxels with two points
    assert (R.voxel_indices(p, 1.0).max(0) >= 2 ** 21).all()
    means, counts, _ = check(p, 1.0)
    assert counts.max() == 2
    # inside a batch too, with problem bits above the widest problem
    res = tp.voxel_down_sample_batch([p, p[:100], np.zeros((0, 3)), p[::-1]], [1.0, 1.0, 1.0, 0.5],
                                     return_counts=True, return_trace=True)
    for q, v, r in zip([p, p[:100], np.zeros((0, 3)), p[::-1]], [1.0, 1.0, 1.0, 0.5], res):
        assert_bits(r, R.voxel_down_sample(q, v))


def test_key_width_edges():
    """The key at the word boundary: 64 bits in one pass, 65 with one bit for the second pass, a voxel index and the
    problem index straddling bit 64, the problem index alone in the high word and at the top of the low word."""
    tiny, empty = np.array([[0.0, 0.0, 0.0], [1.0, 2.0, 3.0], [1.2, 2.1, 3.1]]), np.zeros((0, 3))

    def run(clouds, bits, x_shift, prob_shift):
        got_bits, shifts, got_prob_shift = R.key_bits(clouds, 1.0)
        assert (got_bits, shifts[0][0], got_prob_shift) == (bits, x_shift, prob_shift)
        refs = [R.voxel_down_sample(c, 1.0) for c in clouds]
        assert refs[0][1].max() >= 2 and (refs[0][1] == 1).any()
        res = tp.voxel_down_sample_batch(clouds, 1.0, return_counts=True, return_trace=True)
        for r, ref in zip(res, refs):
            assert_bits(r, ref)

    w64 = R.corner_cloud(22, 21, 21, 31)
    run([w64], 64, 42, 64)                              # one pass, end_bit 64, no high word
    run([w64, w64[::-1]], 65, 42, 64)                   # the problem bit alone in the high word: a 1-bit second pass
    w65 = R.corner_cloud(22, 22, 21, 32)
    run([w65], 65, 43, 65)                              # i_x (22 bits at 43) straddles bit 64
    w62 = R.corner_cloud(21, 21, 20, 33)
    run([w62, tiny, empty, w62[::-1]], 64, 41, 62)      # the problem field is bits 62 and 63, nothing above
    w63 = R.corner_cloud(21, 21, 21, 34)
    run([w63, tiny, empty, w63[::-1]], 65, 42, 63)      # the problem field straddles bit 64


RUN_LENGTHS = (1, 2, 63, 64, 65, 66, 127, 128, 129, 191, 192, 193, 256, 257)


def test_run_lengths_at_the_lane_and_chunk_edges():
    """Runs of 64 points stay with the lane kernel, 65 go to the wave kernel; its 64-point chunks end at 128, 192, 256."""
    lengths = RUN_LENGTHS * 3
    p = R.line_of_runs(lengths, 41)
    ref = R.voxel_down_sample(p, 1.0)
    assert ref[1].tolist() == list(lengths)
    assert_bits(gpu(p, 1.0), ref)
    # between two clouds: long runs on both sides of both problem boundaries
    first, third = R.line_of_runs((3, 70, 130), 42), R.line_of_runs((200, 5, 64), 43)
    refs = [R.voxel_down_sample(c, 1.0) for c in (first, p, third)]
    assert refs[0][1][-1] > 64 and refs[1][1][-1] > 64 and refs[2][1][0] > 64
    for r, ref in zip(tp.voxel_down_sample_batch([first, p, third], 1.0, return_counts=True, return_trace=True), refs):
        assert_bits(r, ref)


def test_more_long_runs_than_waves():
    """16 400 voxels of 65 points: more runs for the wave kernel than the 16 384 waves of its grid, so the last ones are
    reached by the grid stride; a tail of 100 one-point voxels for the lane kernel in the same call.  The restatement
    of this 1.07 M-point cloud takes 0.7 s on the CPU."""
    long_runs, tail = 16400, 100
    assert long_runs > 4096 * 4  # kVoxLongBlocks blocks of 4 waves
    p = R.many_runs(long_runs, 65, tail, 51)
    ref = R.voxel_down_sample(p, 1.0)
    assert (ref[1] == 65).sum() == long_runs and (ref[1] == 1).sum() == tail and len(ref[1]) == long_runs + tail
    assert_bits(gpu(p, 1.0), ref)


def test_int_max_guard():
    ok = np.array([[0.0, 0.0, 0.0], [2147483646.0, 0.0, 0.0]])
    check(ok, 1.0)
    with pytest.raises(tp.TeaserHipError, match="voxel_size is too small"):
        gpu(np.array([[0.0, 0.0, 0.0], [2147483647.0, 0.0, 0.0]]), 1.0)


def test_mixed_batch_equals_problems_alone():
    rng = np.random.default_rng(10)
    clouds, sizes = [], []
    for k in range(64):
        kind = k % 8
        n = 0 if kind == 0 else int(rng.integers(1, 3000)) if kind < 6 else int(rng.integers(20000, 60000))
        clouds.append(R.scan_like(seed=100 + k, n=n, offset=float(rng.uniform(-50, 50))) if n >= 6 else
                      rng.uniform(-1, 1, size=(n, 3)))
        sizes.append(float(rng.choice([0.02, 0.05, 0.1, 0.3])))
    clouds[5] = np.full((5000, 3), 0.125)  # one voxel, long run, next to short ones
    res = tp.voxel_down_sample_batch(clouds, sizes, return_counts=True, return_trace=True)
    for c, v, r in zip(clouds, sizes, res):
        assert_bits(r, gpu(c, v))
        assert_bits(r, R.voxel_down_sample(c, v))
    # one voxel size for all clouds
    res1 = tp.voxel_down_sample_batch(clouds[:8], 0.05)
    for c, r in zip(clouds[:8], res1):
        assert r.tobytes() == R.voxel_down_sample(c, 0.05)[0].tobytes()


def test_two_runs_give_the_same_bits():
    p = R.scan_like(seed=12, n=150000)
    a, b = gpu(p, 0.05), gpu(p, 0.05)
    assert_bits(a, b)


def test_refusals_name_the_argument_and_keep_the_handle():
    p = R.scan_like(seed=13, n=5000)
    ref = R.voxel_down_sample(p, 0.05)
    for v in (0.0, -0.05, np.nan, np.inf):
        with pytest.raises(tp.TeaserHipError, match="voxel_size") as e:
            gpu(p, v)
        assert e.value.status == 1
        assert_bits(gpu(p, 0.05), ref)
    q = p.copy()
    q[17, 1] = np.inf
    with pytest.raises(tp.TeaserHipError, match="points"):
        gpu(q, 0.05)
    assert_bits(gpu(p, 0.05), ref)
    with pytest.raises(tp.TeaserHipError, match="problem 1"):
        tp.voxel_down_sample_batch([p, q], 0.05)
    assert_bits(gpu(p, 0.05), ref)
    # NULL pointers where n > 0, straight through the C ABI
    L = tp.lib()
    h = C.c_void_p()
    assert L.teaser_hip_voxel_create(-1, C.byref(h)) == 0
    try:
        out = np.empty((len(p), 3))
        n_out = C.c_int64(-1)
        dp = C.POINTER(C.c_double)
        assert L.teaser_hip_voxel_down_sample(h, None, len(p), 0.05, out.ctypes.data_as(dp), C.byref(n_out), None,
                                              None) == 1
        assert b"points" in L.teaser_hip_voxel_last_error(h)
        assert L.teaser_hip_voxel_down_sample(h, p.ctypes.data_as(dp), len(p), 0.05, None, C.byref(n_out), None,
                                              None) == 1
        assert b"out" in L.teaser_hip_voxel_last_error(h)
        assert L.teaser_hip_voxel_down_sample(h, p.ctypes.data_as(dp), len(p), 0.05, out.ctypes.data_as(dp), None,
                                              None, None) == 1
        assert b"n_out" in L.teaser_hip_voxel_last_error(h)
        assert L.teaser_hip_voxel_down_sample(h, None, 0, 0.05, None, C.byref(n_out), None, None) == 0
        assert n_out.value == 0
        assert L.teaser_hip_voxel_down_sample(h, p.ctypes.data_as(dp), len(p), 0.05, out.ctypes.data_as(dp),
                                              C.byref(n_out), None, None) == 0
        assert out[:n_out.value].tobytes() == ref[0].tobytes()
    finally:
        L.teaser_hip_voxel_destroy(h)


def test_cxx_facade_agrees_with_python(tmp_path):
    from voxel_cxx import build_voxel_example
    p = np.load(CROP)["points"].astype(np.float64)
    p.tofile(str(tmp_path / "points.bin"))
    ref = gpu(p, 0.05)
    for eigen in (False, True):
        exe = build_voxel_example(eigen)
        out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stdout + out.stderr
        out = subprocess.run([exe, str(tmp_path), "0.05"], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stdout + out.stderr
        assert np.fromfile(str(tmp_path / "means.bin")).tobytes() == ref[0].tobytes()
        assert np.array_equal(np.fromfile(str(tmp_path / "counts.bin"), dtype=np.int32), ref[1])
        assert np.array_equal(np.fromfile(str(tmp_path / "trace.bin"), dtype=np.int32), ref[2])


def write_ply(path, p):
    p = np.asarray(p, dtype=np.float32)
    with open(path, "wb") as f:
        f.write(("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\n"
                 "property float z\nend_header\n" % len(p)).encode())
        f.write(p.tobytes())


def test_example_down_samples_ply_inputs_on_the_gpu(tmp_path):
    """examples/teaser_python_fpfh.py with two PLY files: the GPU down-sampling feeds the rest of the pipeline."""
    g = np.load(CROP)
    p = g["points"]
    write_ply(str(tmp_path / "a.ply"), p)
    write_ply(str(tmp_path / "b.ply"), p[::2])
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "teaser_python_fpfh.py"),
                          str(tmp_path / "a.ply"), str(tmp_path / "b.ply")], capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "voxel down-sampling: %d / %d -> %d / " % (len(p), len(p[::2]), len(g["means"])) in out.stdout
    assert "down-sampling" in out.stdout and " ms, front-end" in out.stdout
