"""The wide batches of tests/test_gpu_wide_batches.py without a GPU: every builder is called, so that what it asserts
from the sizes alone holds here; every numpy restatement is run over its batch and timed (the times stand in the GPU
tests' docstrings and in profiles/wide_batches/README.md), and together they must stay under 90 s; and a table maps
every batched entry point of the C ABI either to the wide test that calls it with more than 256 problems or to an
exemption with its reason, so that a front-end added without a wide test fails here."""
import ast
import importlib
import os
import time

import pytest

import wide_batch_cases as W
from util import ROOT

tp = importlib.import_module("teaser-plusplus_amd")

RESTATEMENTS = ["plane", "ransac", "fgr", "posegraph", "information", "colored", "search", "fpfh", "boundary", "dbscan",
                "fps", "rgbd", "odometry"]
BUDGET = 90.0  # seconds for all restatements together on the machine that runs the CPU suite
_seconds = {}


@pytest.mark.parametrize("name", RESTATEMENTS)
def test_builder_asserts_hold_and_the_restatement_runs(name):
    fn = getattr(W, name)
    fn.cache_clear()
    t0 = time.perf_counter()
    out = fn()
    _seconds[name] = time.perf_counter() - t0
    print("restatement of the wide %s batch: %.2f s" % (name, _seconds[name]))
    batch = out[0]
    size = len(batch["clouds"] if name == "plane" else batch["P"] if name == "ransac" else
               batch["data"] if name == "search" else batch)
    assert size == 320


def test_the_restatements_together_stay_inside_the_budget():
    missing = [n for n in RESTATEMENTS if n not in _seconds]
    for n in missing:  # run alone or in another order: time what the test above has not
        t0 = time.perf_counter()
        getattr(W, n).cache_clear()
        getattr(W, n)()
        _seconds[n] = time.perf_counter() - t0
    total = sum(_seconds.values())
    print("restatements of the wide batches: %.1f s in all" % total)
    assert total < BUDGET, _seconds


def test_margins_and_regimes_that_come_from_the_restatements():
    """What the GPU tests assert from the restatement (not from the sizes) before they call the device."""
    assert W.colored_margins_hold(W.colored()[3])
    total = [len(r[0]) for r in W.search()[5]]
    assert sum(total) > 0 and sum(t == 0 for t in total) >= 50
    assert not any(total[250:255]) and all(total[255:258]) and not any(total[258:263])
    found = [r["best_trial"] >= 0 for r in W.plane()[2]]
    assert any(found) and not all(found)
    done = sorted(r["trials"] for r in W.ransac()[1])
    assert done[-1] == 13000 and done[-4] == 5000 and sum(64 < t < 4096 for t in done) >= 10
    names, refs = W.posegraph()
    assert len({refs[n][0]["status"] for n in set(names) - {"size_128"}}) >= 2


# ---- the coverage guard ---------------------------------------------------------------------------------------------
WIDTH, WIDE = "tests/test_gpu_batch_width.py", "tests/test_gpu_wide_batches.py"
SOLVER = "the solver handle: tests/test_gpu_parity.py and tests/test_gpu_long_n.py cover its batches"
FEATURES = ("the features handle predates both wide files and its grids step through the pairs in slices of 65 535 "
            "(kernels_features.hip); it has no wide test yet")
# every *_batch symbol of the ABI list -> (file, test function) that calls it with more than 256 problems, or a reason
COVERAGE = {
    "teaser_hip_solve_batch": SOLVER,
    "teaser_hip_solve_batch_device": SOLVER,
    "teaser_hip_submit_batch": SOLVER,
    "teaser_hip_multi_solve_batch": SOLVER,
    "teaser_hip_icp_batch": (WIDTH, "test_registration_icp_batch_with_300_problems"),
    "teaser_hip_icp_batch_ex": (WIDTH, "test_registration_icp_batch_with_300_problems"),
    "teaser_hip_icp_batch_cov": (WIDTH, "test_registration_icp_batch_with_300_problems"),
    "teaser_hip_icp_covariances_batch": (WIDTH, "test_registration_icp_batch_with_300_problems"),
    "teaser_hip_icp_normals_batch": (WIDTH, "test_estimate_normals_batch"),
    "teaser_hip_icp_batch_auto": (WIDE, "test_icp_with_normals_estimated_inside_the_call"),
    "teaser_hip_icp_self_knn_batch": (WIDTH, "test_self_knn_batch_with_both_list_capacities_and_both_routes"),
    "teaser_hip_icp_remove_statistical_outliers_batch": (WIDTH, "test_remove_statistical_outlier_batch"),
    "teaser_hip_icp_remove_radius_outliers_batch": (WIDTH, "test_remove_radius_outlier_batch"),
    "teaser_hip_icp_knn_search_batch": (WIDE, "test_two_cloud_search"),
    "teaser_hip_icp_hybrid_search_batch": (WIDE, "test_two_cloud_search"),
    "teaser_hip_icp_radius_search_batch": (WIDE, "test_two_cloud_search"),
    "teaser_hip_icp_fpfh_batch": (WIDE, "test_fpfh_open3d_form"),
    "teaser_hip_icp_boundary_points_batch": (WIDE, "test_boundary_points"),
    "teaser_hip_icp_unproject_depth_batch": (WIDE, "test_rgbd_unprojection_and_projection"),
    "teaser_hip_icp_project_depth_batch": (WIDE, "test_rgbd_unprojection_and_projection"),
    "teaser_hip_icp_iss_keypoints_batch": (WIDTH, "test_compute_iss_keypoints_batch"),
    "teaser_hip_icp_cluster_dbscan_batch": (WIDE, "test_dbscan"),
    "teaser_hip_icp_farthest_point_down_sample_batch": (WIDE, "test_farthest_point_down_sampling"),
    "teaser_hip_icp_information_batch": (WIDE, "test_information_matrices"),
    "teaser_hip_icp_batch_color": (WIDE, "test_colored_icp_gradients_and_registration"),
    "teaser_hip_icp_color_gradients_batch": (WIDE, "test_colored_icp_gradients_and_registration"),
    "teaser_hip_voxel_down_sample_batch": (WIDTH, "test_voxel_down_sample_batch"),
    "teaser_hip_features_fpfh_batch": FEATURES,
    "teaser_hip_features_match_batch": FEATURES,
    "teaser_hip_features_correspondences_batch": FEATURES,
    "teaser_hip_features_knn_batch": FEATURES,
    "teaser_hip_features_match_knn_batch": FEATURES,
    "teaser_hip_features_correspondences_knn_batch": FEATURES,
    "teaser_hip_features_tuple_test_batch": FEATURES,
    "teaser_hip_posegraph_optimize_batch": (WIDE, "test_pose_graph_optimisation"),
    "teaser_hip_posegraph_linearize_batch": "a stage call for tests: the Python front-end linearises one graph per call",
    "teaser_hip_ransac_correspondence_batch": (WIDE, "test_ransac_on_correspondences_with_one_to_four_chunks_in_a_group"),
    "teaser_hip_ransac_trials_batch": (WIDE, "test_ransac_on_correspondences_with_one_to_four_chunks_in_a_group"),
    "teaser_hip_fgr_correspondence_batch": (WIDE, "test_fgr_on_correspondences_by_both_routes"),
    "teaser_hip_fgr_iterations_batch": (WIDE, "test_fgr_on_correspondences_by_both_routes"),
    "teaser_hip_plane_segment_batch": (WIDE, "test_plane_segmentation"),
    "teaser_hip_plane_trials_batch": (WIDE, "test_plane_segmentation"),
    "teaser_hip_tsdf_integrate_batch": "one volume per call: its batch is the frames, tested at 2 * CHUNK + 1",
    "teaser_hip_icp_rgbd_odometry_batch": (WIDE, "test_rgbd_odometry_and_its_pyramid_stage"),
    "teaser_hip_icp_rgbd_odometry_pyramid_batch": (WIDE, "test_rgbd_odometry_and_its_pyramid_stage"),
}


def wide_test_functions_of(path):
    tree = ast.parse(open(os.path.join(ROOT, path)).read())
    return {node.name for node in tree.body if isinstance(node, ast.FunctionDef) and node.name.startswith("test_")}


def coverage_problems(symbols, table):
    """Every way in which `table` fails to cover the batched symbols: a list of sentences, empty when it does."""
    batched = [s for s in symbols if "_batch" in s]
    bad = ["%s is a batched entry point without a wide test or an exemption" % s for s in batched if s not in table]
    bad += ["%s is in the table but not in the ABI list" % s for s in table if s not in batched]
    for sym, entry in table.items():
        if isinstance(entry, str):
            if not entry.strip() or "\n" in entry:
                bad.append("%s: an exemption needs a one-line reason" % sym)
            continue
        path, name = entry
        if path not in (WIDTH, WIDE):
            bad.append("%s: %s is not one of the two wide test files" % (sym, path))
        elif name not in wide_test_functions_of(path):
            bad.append("%s: %s has no test function %s" % (sym, path, name))
    return bad


def test_every_batched_entry_point_has_a_wide_test_or_an_exemption():
    assert coverage_problems(tp.EXPORTED_SYMBOLS, COVERAGE) == []


def test_the_coverage_guard_catches_gaps():
    assert any("teaser_hip_new_front_end_batch" in p for p in
               coverage_problems(list(tp.EXPORTED_SYMBOLS) + ["teaser_hip_new_front_end_batch"], COVERAGE))
    renamed = dict(COVERAGE, teaser_hip_plane_segment_batch=(WIDE, "test_no_such_function"))
    assert any("test_no_such_function" in p for p in coverage_problems(tp.EXPORTED_SYMBOLS, renamed))
    assert coverage_problems(tp.EXPORTED_SYMBOLS, dict(COVERAGE, teaser_hip_tsdf_integrate_batch="")) != []
    assert coverage_problems(tp.EXPORTED_SYMBOLS, {k: v for k, v in COVERAGE.items() if "dbscan" not in k}) != []
