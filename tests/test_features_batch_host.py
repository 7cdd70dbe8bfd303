"""The batched correspondence front-end without a GPU: creation fails loudly (never a CPU fallback), the Python
argument normalisation, and the C++ facade example compiles (it runs on the GPU: test_gpu_features_batch_cxx.py)."""
import ctypes as C
import importlib
import subprocess

import numpy as np
import pytest

tp = importlib.import_module("teaser-plusplus_amd")
feat = importlib.import_module("teaser-plusplus_amd.features")


def test_no_device_is_a_loud_error():
    if tp.device_count() > 0:
        return  # on the GPU box test_gpu_features_batch.py covers creation
    h = C.c_void_p()
    assert tp.lib().teaser_hip_features_create(0, C.byref(h)) == 3 and not h  # TEASER_HIP_ERR_NO_DEVICE
    pts = np.zeros((8, 3), dtype=np.float32)
    f = np.zeros((8, 33), dtype=np.float32)
    for call in (lambda: tp.compute_fpfh_batch([pts], 0.03, 0.05), lambda: tp.match_features_batch([f], [f]),
                 lambda: tp.correspondences_batch([pts], [pts], 0.03, 0.05)):
        with pytest.raises(tp.TeaserHipError, match="NO_DEVICE"):
            call()


def test_the_budget_hook_is_not_a_setting():
    """The list budget is a constant of the source with a per-handle test hook: no set_option row, no environment."""
    with pytest.raises(tp.TeaserHipError):
        tp.get_option("features_list_budget")
    assert tp.lib().teaser_hip_features_set_budgets(None, 1, 1) != 0  # (needs a handle)


def test_clouds_are_coerced_to_float32_n_by_3():
    a = feat._clouds([[[0, 0, 0], [1, 2, 3]], np.zeros((0, 3)), [], np.ones((4, 3), dtype=np.float64)[::2]])
    assert [x.shape for x in a] == [(2, 3), (0, 3), (0, 3), (2, 3)]
    assert all(x.dtype == np.float32 and x.flags.c_contiguous for x in a)
    assert a[0].tolist() == [[0, 0, 0], [1, 2, 3]]
    with pytest.raises(ValueError, match=r"clouds\[1\]"):
        feat._clouds([np.zeros((2, 3)), np.zeros((3, 2))])
    with pytest.raises(ValueError, match=r"src_clouds\[0\]"):
        feat._clouds([np.zeros(6)], "src_clouds")


def test_radii_are_a_scalar_or_one_per_problem():
    assert feat._radii(0.05, 3, "r").tolist() == [0.05] * 3
    assert feat._radii([0.1, 0.2, 0.3], 3, "r").tolist() == [0.1, 0.2, 0.3] and feat._radii(np.float32(0.5), 2, "r").dtype == np.float64
    assert len(feat._radii(0.05, 0, "r")) == 1 and len(feat._radii([], 0, "r")) == 1  # (an address for an empty batch)
    with pytest.raises(ValueError, match="normal_radius"):
        feat._radii([0.1, 0.2], 3, "normal_radius")
    with pytest.raises(ValueError, match="fpfh_radius"):
        feat._radii([[0.1, 0.2, 0.3]], 3, "fpfh_radius")


def test_features_share_one_dim_and_lists_one_length():
    a, dim = feat._features([np.zeros((4, 33)), np.zeros((0, 33)), []], "src_feats")
    assert dim == 33 and [x.shape[0] for x in a] == [4, 0, 0] and all(x.dtype == np.float32 for x in a)
    assert feat._features([[], np.zeros((0, 5))], "f")[1] is None
    with pytest.raises(ValueError, match=r"src_feats\[1\] has dim 32"):
        feat._features([np.zeros((4, 33)), np.zeros((2, 32))], "src_feats")
    with pytest.raises(ValueError, match="n x dim"):
        feat._features([np.zeros(33)], "f")
    # mismatched list lengths / dims are refused before any device is needed
    with pytest.raises(ValueError, match="same length"):
        tp.match_features_batch([np.zeros((4, 33))], [])
    with pytest.raises(ValueError, match="same length"):
        tp.correspondences_batch([np.zeros((4, 3))] * 2, [np.zeros((4, 3))], 0.03, 0.05)
    with pytest.raises(ValueError, match="dim 33.*dim 16"):
        tp.match_features_batch([np.zeros((4, 33))], [np.zeros((4, 16))])
    with pytest.raises(ValueError, match="normal_radius"):
        tp.compute_fpfh_batch([np.zeros((4, 3))] * 2, [0.03], 0.05)


def test_ragged_lists_are_packed_as_pointer_and_count_arrays():
    clouds = feat._clouds([np.zeros((5, 3)), np.zeros((0, 3)), np.ones((2, 3))])
    n = feat._counts(clouds)
    assert n.dtype == np.int32 and n.tolist() == [5, 0, 2] and feat._counts([]).tolist() == [0]
    p = feat._ptrs(clouds, feat._fp)
    assert len(p) == 3 and p[2][0] == 1.0 and len(feat._ptrs([], feat._fp)) == 1
    cap, bufs, cnt = feat._pair_buffers(np.array([5, 0, 2]), np.array([3, 4, 0]), 3)
    assert cap.dtype == np.int64 and cap.tolist() == [8, 4, 2] and [b.shape for b in bufs] == [(8, 2), (4, 2), (2, 2)]
    assert cnt.dtype == np.int64 and len(cnt) == 3 and all(b.dtype == np.int32 for b in bufs)


@pytest.mark.parametrize("eigen", [False, True])
def test_cxx_batch_example_builds_and_fails_loudly_without_device(eigen):
    from fpfh_batch_cxx import build_fpfh_batch_example
    exe = build_fpfh_batch_example(eigen)
    if tp.device_count() == 0:
        assert subprocess.call([exe], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL) == 77
