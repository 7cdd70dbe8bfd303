"""examples/teaser_python_fpfh.py --fps K on BASELINE config 5: the single pair matches at exactly K samples per cloud
and maps its pairs back to cloud indices; --batch gives every cloud of every pair exactly min(K, n) samples from one
call; --fps with --iss is refused before anything runs."""
import os
import re
import subprocess
import sys

import pytest

from util import ROOT

pytestmark = pytest.mark.gpu
EXAMPLE = os.path.join(ROOT, "examples", "teaser_python_fpfh.py")


def example(*args):
    return subprocess.run([sys.executable, EXAMPLE] + list(args), capture_output=True, text=True, timeout=600, cwd=ROOT)


def test_single_pair_matches_at_k_samples():
    out = example("--fps", "1500")
    assert out.returncode == 0, out.stdout + out.stderr
    m = re.search(r"farthest-point samples: (\d+) of (\d+) / (\d+) of (\d+) points", out.stdout)
    assert m, out.stdout
    ka, na, kb, nb = map(int, m.groups())
    assert ka == kb == 1500 and na > 1500 and nb > 1500
    m = re.search(r"(\d+) / (\d+) points, (\d+) correspondences, max clique (\d+)", out.stdout)
    assert m, out.stdout
    assert (int(m.group(1)), int(m.group(2))) == (na, nb)  # the solver sees the clouds, the pairs index them
    assert 3 <= int(m.group(3)) <= 1500


def test_batch_gives_every_cloud_exactly_k_samples():
    out = example("--batch", "2", "--fps", "800", "--icp-iterations", "5")
    assert out.returncode == 0, out.stdout + out.stderr
    assert "farthest-point samples: 800 .. 800 per cloud (--fps 800, one call for all 4 clouds)" in out.stdout, out.stdout
    big = example("--batch", "2", "--fps", "1000000", "--icp-iterations", "5")  # K above n: every cloud keeps its n points
    assert big.returncode == 0, big.stdout + big.stderr
    m = re.search(r"(\d+) \.\. (\d+) points after down-sampling", big.stdout)
    s = re.search(r"farthest-point samples: (\d+) \.\. (\d+) per cloud", big.stdout)
    assert m and s and m.groups() == s.groups(), big.stdout


def test_fps_and_iss_together_are_an_error():
    out = example("--fps", "100", "--iss")
    assert out.returncode == 2 and "--fps and --iss" in out.stderr
