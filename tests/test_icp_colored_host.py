"""The host side of Colored ICP without a GPU: csrc/icp.hip and csrc/icp_color.hip compiled by g++ against the HIP
stand-in header, with the source of the colour-gradient kernel run one lane at a time and a stand-in for the mode-3
iteration launcher that reads every row the kernel would (tests/icp_colored_host_driver.cpp), under AddressSanitizer and
UndefinedBehaviorSanitizer, as a stand-alone program.  The plan of the gradient stage, the packing of intensities and
{gradient, intensity} records, the uploads, the launch arguments and the unpacking of the results run for real."""
import os
import subprocess

from util import ROOT


def test_colour_stage_sizes_packs_and_hands_over_cleanly(tmp_path):
    exe = str(tmp_path / "icp_colored_host_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-ffp-contract=off", "-x", "c++", "-I" + os.path.join(ROOT, "tests", "hip_stub"),
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "teaser-plusplus_amd", "csrc"),
                           os.path.join(ROOT, "tests", "icp_colored_host_driver.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "mismatches 0" in out.stdout, out.stdout + out.stderr[-4000:]
