"""The host side of the information matrices without a GPU: csrc/icp_information.hip compiled by g++ against the HIP
stand-in header with stand-ins for the kernel launchers that walk the block map and touch every row the kernels would
(tests/icp_information_host_driver.cpp), under AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone
program.  Buffer sizing, packing, the uploads, the launch arguments, the unpacking and every entry check run for real."""
import os
import subprocess

from util import ROOT


def test_information_entry_sizes_packs_unpacks_and_refuses_cleanly(tmp_path):
    exe = str(tmp_path / "icp_information_host_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-ffp-contract=off", "-x", "c++", "-I" + os.path.join(ROOT, "tests", "hip_stub"),
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "teaser-plusplus_amd", "csrc"),
                           os.path.join(ROOT, "tests", "icp_information_host_driver.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "mismatches 0" in out.stdout, out.stdout + out.stderr[-4000:]
