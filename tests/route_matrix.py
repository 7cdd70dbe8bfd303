"""The route switches and tuning knobs of teaser_hip_set_option as data (no GPU needed to import this module).

include/teaser_hip.h promises that no value of a route option changes a result.  tests/test_gpu_route_switches.py runs
every (option, value) of ROUTES and every combination of COMBOS against the default route and the oracle;
tests/test_abi_symbols.py checks that ROUTES, ALREADY_TESTED and DIAGNOSTIC together cover the settings table of
csrc/solver.hip exactly, so an option added without a route test fails there."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOLVER_HIP = os.path.join(ROOT, "teaser-plusplus_amd", "csrc", "solver.hip")

# option -> the values under test (each list holds the option's lo and hi from kSettingRows)
ROUTES = {
    # K1 FP64 fix-up: grid of tim_fixup_group_kernel (1 is clamped to 4 workgroups; 65536 is far more than regions)
    "fixup_wgs": [0, 1, 5, 65536],
    # heuristic: workgroups sharing a problem's 16-start queue
    "heu_blocks": [0, 1, 2, 5, 16],
    # heuristic: 1 is admissible and neither 256 nor 512 (the 256-thread kernel)
    "greedy_threads": [0, 1, 256, 512],
    # the all-starts greedy of graphs of at most 768 vertices off
    "greedy_small": [0, 1],
    # degree closure: workgroups per problem of the row launch
    "deg_closure_wgs": [0, 1, 2, 64],
    # exact search: LDS stack bytes (1000 is not a multiple of 16; 65536 does not fit and falls back to 0)
    "k4_lds_stack": [0, 16, 1000, 2048, 65536],
    "k4_donate": [0, 1],
    "k4_donate_after": [-1, 0, 1, 1048576],
    "k4_hungry": [-1, 0, 1, 1048576],
    # 8 is clamped to kTaskPrefix - 1 = 7 passes
    "k4_expand": [-1, 0, 1, 2, 8],
    "k4_waves": [0, 1, 64, 1048576],
    # scale stage: one problem at a time / no shared sort for mid-size problems
    "scale_batch": [0, 1],
    "scale_mid_batch": [0, 1],
    # asynchronous schedule (read at handle creation; copy_stream at the first host-input batch of a handle)
    "depth": [1, 3, 16],
    "stagger": [0, 2, 3],
    "k1_stream": [0, 1, 2],
    "tail_cus": [0, 1, 8, 255],
    "tail_cu_block": [0, 1],
    "copy_stream": [0, 1, 2],
    "h2d_kernel": [0, 1],
}

# stress combinations (applied together; "batch" is a workload hint, not an option)
COMBOS = {
    "max_donation_traffic": {"k4_donate_after": 0, "k4_hungry": 1048576, "k4_expand": 0, "k4_waves": 64},
    "hbm_records_no_donation": {"k4_lds_stack": 0, "k4_donate": 0},
    "wide_heuristic_64": {"heu_blocks": 16, "greedy_threads": 512},
}

# options that are allowed to change results
DIAGNOSTIC = {
    "k4_debug": "prints diagnostics on stderr and traces the heuristic's starts; used by the route tests as evidence",
    "k4_lb_bonus": "starts the exact search above the incumbent to price a better heuristic: may miss the maximum clique",
    "tail_skip": "timing probe that leaves stages out behind K1: results are wrong by design",
    "reference_snapshot_semantics": "emulates the reference snapshot's binary (PMC_EXACT + CHAIN), not a route switch",
}

# options with a route test elsewhere: option -> "<module>::<test function>"
ALREADY_TESTED = {
    "k1_fp64": "test_gpu_parity::test_k1_matrix_core_filter_matches_the_fp64_kernel",
    "fused_estimators": "test_gpu_parity::test_fused_estimators_match_the_separate_kernels",
    "scale_sort64": "test_gpu_parity::test_scale_float_key_sort_matches_the_64_bit_sort",
    "scale_hull": "test_gpu_parity::test_scale_hull_matches_the_full_sort",
    "scale_hull_sync": "test_gpu_parity::test_scale_hull_matches_the_full_sort",
    "colour_persistent": "test_gpu_parity::test_colouring_rounds_in_one_launch_match_the_launch_per_round_route",
    "colour_mis": "test_gpu_parity::test_colour_centric_bound_matches_the_vertex_centric_route",
    "colour_mis_any": "test_gpu_parity::test_colour_centric_bound_on_supplied_graphs",
    "deg_closure": "test_gpu_parity::test_degree_closure_matches_the_greedy_route_on_50_seeds",
    "heu_skip_closed": "test_gpu_parity::test_degree_closure_switches_the_heuristic_launches_off_and_on",
    "spec_bounds": "test_gpu_parity::test_async_paths_agree_across_host_modes",
    "finisher": "test_gpu_parity::test_async_paths_agree_across_host_modes",
}

# options read when a handle is created (depth .. tail_cu_block) or when it sets up its copy stream: a test needs a
# handle created after set_option
HANDLE_TIME = ("depth", "stagger", "k1_stream", "tail_cus", "tail_cu_block", "copy_stream")


def setting_rows(path=SOLVER_HIP):
    """kSettingRows of csrc/solver.hip: name -> (env, default, lo, hi)."""
    text = open(path).read()
    body = text[text.index("const SettingRow kSettingRows[S_COUNT] = {"):]
    body = body[:body.index("\n};")]
    rows = {}
    for name, env, d, lo, hi in re.findall(r'\{"([a-z0-9_]+)",\s*"([A-Z0-9_]+)",\s*(-?\d+),\s*(-?\d+),\s*(-?\d+)\}', body):
        assert name not in rows, name
        rows[name] = (env, int(d), int(lo), int(hi))
    return rows
