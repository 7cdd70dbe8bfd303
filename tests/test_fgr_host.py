"""The host side of Fast Global Registration without a GPU: csrc/fgr.hip compiled by g++ against the HIP stand-in
header with stand-in launchers that run the one-lane functions of csrc/fgr_device.h on the CPU
(tests/fgr_host_driver.cpp), under AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone program: the
packing and offsets of a mixed batch, the route of every problem at resident_max_corr 0, the default and the bound, the
full call and the stage call against the contract written out in the driver, and every refusal.  Then the Python
surface: names, defaults and the argument errors that need no device."""
import importlib
import os
import subprocess

import numpy as np
import pytest

from util import ROOT

tp = importlib.import_module("teaser-plusplus_amd")


def test_fgr_packs_routes_steps_and_refuses(tmp_path):
    exe = str(tmp_path / "fgr_host_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-ffp-contract=off", "-x", "c++", "-I" + os.path.join(ROOT, "tests", "hip_stub"),
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "teaser-plusplus_amd", "csrc"),
                           os.path.join(ROOT, "tests", "fgr_host_driver.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "mismatches 0" in out.stdout, out.stdout + out.stderr[-4000:]


def test_python_surface_names_and_defaults():
    names = ["FastGlobalRegistrationOption", "registration_fgr_based_on_correspondence",
             "registration_fgr_based_on_correspondence_batch", "registration_fgr_based_on_feature_matching",
             "fgr_iterations_batch"]
    for name in names:
        assert name in tp.__all__ and hasattr(tp, name), name
    for name in tp.EXPORTED_SYMBOLS:
        if name.startswith("teaser_hip_fgr_"):
            assert hasattr(tp.lib(), name), name
    p = tp.fgr.FgrParamsC()
    assert tp.lib().teaser_hip_fgr_params_default(p) == 0
    assert (p.division_factor, p.maximum_correspondence_distance) == (1.4, 0.025)
    assert (p.use_absolute_scale, p.decrease_mu, p.iteration_number) == (0, 1, 64)
    o = tp.FastGlobalRegistrationOption()
    assert (o.division_factor, o.use_absolute_scale, o.decrease_mu, o.maximum_correspondence_distance) == (1.4, False, True, 0.025)
    assert (o.iteration_number, o.tuple_scale, o.maximum_tuple_count, o.tuple_test, o.seed) == (64, 0.95, 1000, True, 0)
    assert "maximum_tuple_count is NOT applied" in tp.FastGlobalRegistrationOption.__doc__
    q = tp.fgr._params(tp.FastGlobalRegistrationOption(2.0, True, False, 0.5, 7))
    assert (q.division_factor, q.use_absolute_scale, q.decrease_mu) == (2.0, 1, 0)
    assert (q.maximum_correspondence_distance, q.iteration_number) == (0.5, 7)


def test_python_argument_errors_need_no_device():
    P, corr = np.zeros((12, 3)), np.zeros((12, 2), dtype=np.int32)
    call = tp.registration_fgr_based_on_correspondence
    with pytest.raises(TypeError, match="FastGlobalRegistrationOption"):
        call(P, P, corr, option=0.025)
    with pytest.raises(ValueError, match="corres 0 must be an n x 2"):
        call(P, P, np.zeros((4, 3), dtype=np.int32))
    with pytest.raises(ValueError, match="source 0 must be an n x 3"):
        call(np.zeros((4, 2)), P, corr)
    with pytest.raises(ValueError, match="2 values for 1 problems"):
        tp.registration_fgr_based_on_correspondence_batch([P], [P], [corr], [tp.FastGlobalRegistrationOption()] * 2)
    with pytest.raises(ValueError, match="option: 2 values for 1 problems"):  # an array holds one per problem too
        tp.registration_fgr_based_on_correspondence_batch([P], [P], [corr],
                                                          np.array([tp.FastGlobalRegistrationOption()] * 2, dtype=object))
    with pytest.raises(ValueError, match="differ in length"):
        tp.registration_fgr_based_on_correspondence_batch([P], [P, P], [corr])
    H = importlib.import_module("teaser-plusplus_amd._handles")  # one copy of the argument helpers
    assert tp.fgr._pairs is H._pairs and tp.ransac._pairs is H._pairs
    assert tp.fgr._per_problem is H._per_problem and tp.ransac._per_problem is H._per_problem
    assert tp.plane._per_problem is H._per_problem
    assert tp.registration_fgr_based_on_correspondence_batch([], [], []) == []  # no problems: no device needed
    assert tp.fgr_iterations_batch([], [], [], 3) == []
