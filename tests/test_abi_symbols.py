"""The C-ABI library loads on a box without a GPU and exports every entry point include/teaser_hip.h
declares (no compute calls here); creating a solver without a device fails loudly."""
import ctypes as C
import importlib
import os
import re

import pytest

from util import ROOT

tp = importlib.import_module("teaser-plusplus_amd")


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "teaser_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"TEASER_HIP_API\s+[A-Za-z0-9_\s\*]*?\b(teaser_hip_[a-z0-9_]+)\s*\(", text)))


def test_every_declared_entry_point_is_exported():
    names = declared_symbols()
    assert len(names) >= 25
    L = tp.lib()
    for name in names:
        assert getattr(L, name) is not None, name
    assert sorted(tp.EXPORTED_SYMBOLS) == names
    assert L.teaser_hip_abi_version() == 1


def test_fill_scratch_is_declared_for_every_handle_kind_but_the_solvers():
    """The diagnostic teaser_hip_<kind>_fill_scratch(handle, int32 byte, int64* bytes_out): exported, declared in the
    header with exactly these arguments, and given its ctypes signature where the kind's other entries get theirs."""
    kinds = ["icp", "voxel", "features", "posegraph", "ransac", "fgr", "plane", "tsdf"]
    assert sorted(tp.SCRATCH_KINDS + ("tsdf",)) == sorted(kinds)  # a TSDF volume is its own handle: UniformTSDFVolume.fill_scratch
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "teaser_hip.h")).read(), flags=re.S)
    L = tp.lib()
    for kind in kinds:
        name = "teaser_hip_%s_fill_scratch" % kind
        assert name in tp.EXPORTED_SYMBOLS
        assert re.search(r"TEASER_HIP_API int32_t %s\(teaser_hip_%s\* \w+, int32_t byte, int64_t\* bytes_out\);" % (name, kind),
                         text), name
        fn = getattr(L, name)
        assert fn.argtypes == [C.c_void_p, C.c_int32, C.POINTER(C.c_int64)], name
        filled = C.c_int64(7)
        assert fn(None, 0, C.byref(filled)) != 0 and filled.value == 7  # no handle: refused, nothing written
    assert callable(tp.fill_scratch) and callable(tp.UniformTSDFVolume.fill_scratch)
    with pytest.raises(ValueError):
        tp.fill_scratch("solver", 0)


def test_no_device_is_a_loud_error():
    if tp.device_count() > 0:
        return  # on the GPU box the parity tests cover creation
    h = C.c_void_p()
    rc = tp.lib().teaser_hip_solver_create(None, 0, C.byref(h))
    assert rc == 3 and not h  # TEASER_HIP_ERR_NO_DEVICE: never a CPU fallback
    try:
        tp.RobustRegistrationSolver()
    except tp.TeaserHipError as e:
        assert "NO_DEVICE" in str(e) or "no MI355X" in str(e)
    else:
        raise AssertionError("constructing a solver without a GPU must raise")


def test_product_does_not_import_the_oracle():
    """oracle/ is test infrastructure: nothing under teaser-plusplus_amd/ or include/ may reference it."""
    bad = []
    for base in ("teaser-plusplus_amd", "include", "teaserpp_python"):
        for dirpath, _, files in os.walk(os.path.join(ROOT, base)):
            for f in files:
                if f.endswith((".py", ".hip", ".h", ".cpp")):
                    txt = open(os.path.join(dirpath, f), errors="ignore").read()
                    if re.search(r"^\s*(from\s+oracle\b|import\s+oracle\b)|#\s*include[^\n]*oracle|"
                                 r"libteaser_oracle|dlopen[^\n]*oracle", txt, flags=re.M):
                        bad.append(os.path.join(dirpath, f))
    assert not bad, bad


def test_bench_cli_parses_without_gpu():
    """bench.py --help must work (argparse help strings) and, without a GPU, the run must stop with the
    explicit no-device message rather than a traceback from deep inside."""
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--depth" in r.stdout and "--batch" in r.stdout and "--gpus" in r.stdout
    if tp.device_count() == 0:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")], capture_output=True, text=True)
        assert r.returncode != 0 and "needs an MI355X" in (r.stderr + r.stdout)


def test_bench_roofline_object():
    """The roofline arithmetic of bench.py (64 x N = 10 k per launch, 0.80 ms): executed-pipe fractions, the largest
    one at the top level, none above 1; the FP64-equivalent ratio nested (it MAY exceed 1)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    pairs = 64 * 10000 * 9999 // 2
    byts = 64 * (48 * 10000 + 8 * 10000 * 157)
    issue = dict(valu_insts_per_1024_pairs=77.6, source="profiles/x/k1_sq_counters.json")
    r = bench.roofline_object(k1_ms=20 * 0.80, k1_launches=20, k1_bytes=20 * byts, k1_pairs=20 * pairs,
                              k1_aux_ms=20 * 0.15, traffic=1.78e9, traffic_src="profiles/x", issue=issue)
    assert set(r["pipes"]) == {"valu", "mfma", "hbm"}
    assert r["bound"] == "valu" and r["unit"] == "G wave-instructions/s" and r["peak"] == 1024 * 2.4 / 4
    assert abs(r["avg_launch_ms"] - 0.80) < 1e-9 and r["launches"] == 20
    assert abs(r["achieved"] - 77.6 * pairs / 1024 / 0.80e-3 / 1e9) < 1e-6 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12
    assert r["frac"] == max(p["frac"] for p in r["pipes"].values()) and all(0 <= p["frac"] <= 1 for p in r["pipes"].values())
    assert abs(r["pipes"]["mfma"]["achieved"] - 128 * pairs / 0.80e-3 / 1e12) < 1e-6 and r["pipes"]["mfma"]["peak"] == 2500.0
    assert abs(r["pipes"]["hbm"]["achieved"] - byts / 0.80e-3 / 1e9) < 1e-6 and r["traffic"] == 1.78e9
    f = r["fp64_equivalent"]
    assert abs(f["achieved"] - 20 * pairs / 0.80e-3 / 1e12) < 1e-6 and f["peak"] == 78.6 and f["ratio"] > 1.0
    # a counter pass that also holds the vector-memory instruction count adds the vector-L1 pipe (1 KB per instruction)
    r1 = bench.roofline_object(20 * 0.80, 20, 20 * byts, 20 * pairs, 0.0, None, None,
                               issue=dict(issue, vmem_insts_per_1024_pairs=3.04, ta_busy_frac=0.65))
    assert set(r1["pipes"]) == {"valu", "mfma", "hbm", "l1"} and r1["pipes"]["l1"]["peak"] == 256 * 64 * 2.4
    assert abs(r1["pipes"]["l1"]["achieved"] - 3.04 * pairs / 0.80e-3 / 1e9) < 1e-6 and 0 < r1["pipes"]["l1"]["frac"] < 1
    r0 = bench.roofline_object(20 * 0.80, 20, 20 * byts, 20 * pairs, 0.0, None, None)  # no counter pass committed
    assert r0["pipes"]["valu"]["valu_insts_per_1024_pairs"] == bench.K1_VALU_PER_1024_STATIC
    z = bench.roofline_object(0.0, 0, 0, 0, 0.0, None, None)  # no launches: no division by zero
    assert z["achieved"] == 0.0 and z["traffic"] is None


def test_bench_dump_outputs_writes_the_last_steps_results(tmp_path):
    """bench.py --dump-outputs: the gathered result records and the index lists of the last timed step become
    float64 .npy files (rotation [P, 3, 3], translation [P, 3], per-problem scalars, -1-padded index lists)."""
    import importlib.util
    import types

    import numpy as np
    spec = importlib.util.spec_from_file_location("bench_mod3", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    assert bench.parse(["--full"]).full is True and bench.parse([]).full is False
    assert bench.parse(["--dump-outputs", "d"]).dump_outputs == "d"
    sols = []
    for b in range(3):
        s = tp.SolutionC()
        s.valid, s.scale, s.n, s.clique_size, s.num_edges = 1, 1.0, 100 + b, 5 + b, 40 + b
        s.rotation[:] = list(np.eye(3).ravel() * (b + 1))
        s.translation[:] = [b, 2 * b, 3 * b]
        sols.append(s)
    rec = tp.batched.pack_records(sols)
    lists = {0: [1, 2], 1: [], 2: [0, 4, 7]}
    solver = types.SimpleNamespace(getInlierMaxClique=lambda b: lists[b], getRotationInliers=lambda b: lists[b][:1],
                                   getTranslationInliers=lambda b: lists[b][::-1])
    bench.dump_outputs(str(tmp_path / "out"), tp, solver, rec, 3)
    got = {p.stem: np.load(p) for p in (tmp_path / "out").iterdir()}
    assert all(a.dtype == np.float64 for a in got.values())
    assert got["rotation"].shape == (3, 3, 3) and np.array_equal(got["rotation"][2], 3 * np.eye(3))
    assert np.array_equal(got["translation"][1], [1, 2, 3]) and got["clique_size"].tolist() == [5, 6, 7]
    assert got["num_edges"].tolist() == [40, 41, 42] and got["n"].tolist() == [100, 101, 102]
    assert got["max_clique"].tolist() == [[1, 2, -1], [-1, -1, -1], [0, 4, 7]]
    assert got["translation_inliers"][2].tolist() == [7, 4, 0]


def test_roofline_flat_copies_and_measured_valu_peak():
    """A record that keeps scalars only must still carry the pipe fractions, the traffic ratio and BOTH VALU peaks:
    the assumed one (4 cycles per wave64 instruction at 2.4 GHz) and the one measured for K1's instruction mix
    (scripts/probe/valu_rate weighted by scripts/k1_isa_stats.py, both committed under profiles/)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod2", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    pairs = 64 * 10000 * 9999 // 2
    byts = 64 * (48 * 10000 + 8 * 10000 * 157)
    r = bench.roofline_object(20 * 0.75, 20, 20 * byts, 20 * pairs, 0.0, 1.7e9, "profiles/x",
                              issue=dict(valu_insts_per_1024_pairs=69.4, vmem_insts_per_1024_pairs=2.5, source="profiles/x"))
    for k in ("frac_valu", "frac_mfma", "frac_hbm", "frac_l1"):
        assert r[k] == r["pipes"][k[5:]]["frac"]
    assert abs(r["traffic_over_algorithmic"] - 1.7e9 / byts) < 1e-9
    m = r["valu_peak_measurement"]
    assert m is not None and m["timed_share_of_mix"] > 0.8 and 2.0 < m["cycles_per_valu_inst_at_assumed_ghz"] < 6.0
    assert r["valu_peak_assumed"] == 1024 * 2.4 / 4 and abs(r["valu_peak_measured"] - 1024 * m["assumed_ghz"] / m["cycles_per_valu_inst_at_assumed_ghz"]) < 0.1
    assert abs(r["frac_valu_at_measured_peak"] - r["pipes"]["valu"]["achieved"] / r["valu_peak_measured"]) < 1e-12


def test_set_option_validates_names_and_ranges():
    """teaser_hip_set_option needs no device: unknown names and values outside an option's range answer BAD_ARG and
    leave the table untouched (round-5 advice: a negative k4_lds_stack used to be masked and used)."""
    L = tp.lib()
    assert L.teaser_hip_set_option(None, b"no_such_option", 1) != 0
    assert L.teaser_hip_set_option(None, b"k4_lds_stack", -16) != 0
    assert L.teaser_hip_set_option(None, b"depth", 0) != 0 and L.teaser_hip_set_option(None, b"depth", 17) != 0
    assert L.teaser_hip_set_option(None, b"deg_closure", 2) != 0
    for name, v in ((b"depth", 2), (b"deg_closure", 1), (b"greedy_small", 1), (b"k4_lds_stack", 16384)):
        assert L.teaser_hip_set_option(None, name, v) == 0
    with pytest.raises(tp.TeaserHipError):
        tp.set_option("fused_estimators", 7)
    # the keyword-only device: Params followed by a positional argument is refused loudly (round-5 advice)
    with pytest.raises(TypeError, match="device"):
        tp.RobustRegistrationSolver._params_from_ctor_args((tp.RobustRegistrationSolver.Params(), 0), {})


def test_every_documented_option_exists_with_its_default():
    """INTEGRATION.md's settings table against the library's: every option a row names is accepted with the default the
    row states (a renamed or dropped option fails here; the call also leaves the table at its defaults), and the options
    this round added check their ranges."""
    L = tp.lib()
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    table = text[text.index("| option | env | default | meaning |"):]
    table = table[:table.index("\n\n")]
    seen = set()
    for line in table.splitlines()[2:]:
        cols = [c.strip() for c in line.strip().strip("|").split("|")]
        names = re.findall(r"`([a-z0-9_]+)`", cols[0])
        defaults = [int(x) for x in re.findall(r"-?\d+", cols[2].replace("\u2212", "-").replace(" ", ""))]
        assert names and defaults, line[:80]
        if len(defaults) == 1:
            defaults = defaults * len(names)
        assert len(defaults) == len(names), (names, defaults)
        for name, default in zip(names, defaults):
            assert L.teaser_hip_set_option(None, name.encode(), default) == 0, (name, default)
            seen.add(name)
    assert len(seen) >= 30 and {"colour_mis", "colour_mis_any", "colour_persistent", "deg_closure", "scale_hull"} <= seen, sorted(seen)
    assert L.teaser_hip_set_option(None, b"colour_mis", 65537) != 0 and L.teaser_hip_set_option(None, b"colour_mis_any", 2) != 0


def test_get_option_reads_back_what_set_option_stored():
    """teaser_hip_get_option (no device needed): the value set_option stored, BAD_ARG for an unknown name, and the
    previous value restored."""
    before = tp.get_option("colour_mis")
    try:
        tp.set_option("colour_mis", 4096)
        assert tp.get_option("colour_mis") == 4096
        tp.set_option("colour_mis", 0)
        assert tp.get_option("colour_mis") == 0
    finally:
        tp.set_option("colour_mis", before)
    assert tp.get_option("colour_mis") == before
    with pytest.raises(tp.TeaserHipError):
        tp.get_option("no_such_option")
    v = C.c_int64(7)
    assert tp.lib().teaser_hip_get_option(b"no_such_option", C.byref(v)) != 0 and v.value == 7


def _integration_option_names():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    table = text[text.index("| option | env | default | meaning |"):]
    table = table[:table.index("\n\n")]
    names = []
    for line in table.splitlines()[2:]:
        names += re.findall(r"`([a-z0-9_]+)`", line.strip().strip("|").split("|")[0])
    return names


def _header_option_comment():
    text = open(os.path.join(ROOT, "include", "teaser_hip.h")).read()
    end = text.index("TEASER_HIP_API int32_t teaser_hip_set_option(")
    return text[text.rindex("/*", 0, end):end]


def route_matrix_problems(rows, routes, combos, already, diagnostic, integration, header, test_sources):
    """Every way in which the route matrix (tests/route_matrix.py) fails to cover the settings table: a list of
    messages, empty when complete."""
    bad = []
    names = set(rows)
    if set(integration) != names or len(integration) != len(set(integration)):
        bad.append("INTEGRATION.md table %s != kSettingRows %s" % (sorted(set(integration) ^ names), sorted(names)))
    parts = (set(routes), set(already), set(diagnostic))
    for a, b in ((0, 1), (0, 2), (1, 2)):
        if parts[a] & parts[b]:
            bad.append("classified twice: %s" % sorted(parts[a] & parts[b]))
    union = parts[0] | parts[1] | parts[2]
    if union != names:
        bad.append("not classified: %s; not an option: %s" % (sorted(names - union), sorted(union - names)))
    for name, values in routes.items():
        if name not in rows:
            continue
        lo, hi = rows[name][2], rows[name][3]
        if not values or any(not lo <= v <= hi for v in values):
            bad.append("%s: values %s outside [%d, %d]" % (name, values, lo, hi))
        if lo not in values or hi not in values:
            bad.append("%s: values %s miss lo %d or hi %d" % (name, values, lo, hi))
    for combo, opts in combos.items():
        for name, v in opts.items():
            if name not in rows or not rows[name][2] <= v <= rows[name][3]:
                bad.append("combo %s: %s = %s" % (combo, name, v))
    for name, test in already.items():
        module, func = test.split("::")
        if not re.search(r"^def %s\(" % re.escape(func), test_sources.get(module, ""), flags=re.M):
            bad.append("%s: no test %s" % (name, test))
    for name in names:
        if '"%s"' % name not in header:
            bad.append("teaser_hip.h's set_option comment omits %s" % name)
    for name in diagnostic:
        if name in header and '"%s"' % name not in header[header.index("DIAGNOSTIC"):]:
            bad.append("teaser_hip.h does not mark %s diagnostic" % name)
    return bad


def _route_matrix_inputs():
    import route_matrix as rm
    sources = {}
    for test in rm.ALREADY_TESTED.values():
        module = test.split("::")[0]
        sources[module] = open(os.path.join(ROOT, "tests", module + ".py")).read()
    return dict(rows=rm.setting_rows(), routes=rm.ROUTES, combos=rm.COMBOS, already=rm.ALREADY_TESTED,
                diagnostic=rm.DIAGNOSTIC, integration=_integration_option_names(), header=_header_option_comment(),
                test_sources=sources)


def test_every_option_is_route_tested_or_diagnostic():
    """The settings table of csrc/solver.hip, INTEGRATION.md's table, teaser_hip.h's set_option comment and the route
    matrix (tests/route_matrix.py) name the same options; every option is route-tested (ROUTES, or a test named in
    ALREADY_TESTED that exists) or classified DIAGNOSTIC, exactly once; every value under test is in range and the
    ranges' ends are tested.  An option added without a route test fails here."""
    inp = _route_matrix_inputs()
    assert len(inp["rows"]) == 36
    assert route_matrix_problems(**inp) == []


def test_route_matrix_guard_catches_gaps(tmp_path):
    """The guard above fails for a row added to a copy of the settings table and for an entry dropped from ROUTES."""
    import route_matrix as rm
    inp = _route_matrix_inputs()
    src = open(rm.SOLVER_HIP).read()
    fake = tmp_path / "solver.hip"
    fake.write_text(src.replace('{"k1_fp64", ', '{"fake_route", "TEASER_FAKE_ROUTE", 0, 0, 1},\n    {"k1_fp64", ', 1))
    assert "fake_route" in route_matrix_problems(**dict(inp, rows=rm.setting_rows(str(fake))))[0]
    routes = dict(rm.ROUTES)
    del routes["k4_hungry"]
    assert any("k4_hungry" in m for m in route_matrix_problems(**dict(inp, routes=routes)))
    routes = dict(rm.ROUTES, depth=[1, 17])
    assert any(m.startswith("depth:") for m in route_matrix_problems(**dict(inp, routes=routes)))
    assert any("no test" in m for m in route_matrix_problems(**dict(inp, already=dict(rm.ALREADY_TESTED, k1_fp64="test_gpu_parity::test_gone"))))
