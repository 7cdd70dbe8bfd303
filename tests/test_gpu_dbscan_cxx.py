"""The C++ facade of DBSCAN clustering (include/teaser/cluster.h: teaser::DBSCANParams, clusterDBSCAN, teaser::DBSCAN)
through tests/cxx/dbscan_example.cpp: the contested-border scene of tests/dbscan_reference.py in both index orders with
literal expectations (the same ones tests/test_dbscan_reference.py works out), single and batched."""
import importlib
import subprocess

import pytest

from dbscan_cxx import build_dbscan_example

pytestmark = pytest.mark.gpu
tp = importlib.import_module("teaser-plusplus_amd")


def test_cxx_facade_clusters_the_contested_scene():
    if tp.device_count() < 1:
        pytest.fail("the GPU suite needs an MI355X")
    exe = build_dbscan_example()
    own = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert own.returncode == 0 and "checks 1" in own.stdout, own.stderr
