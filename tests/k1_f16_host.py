"""Builds and calls tests/k1_f16_consts_main.cpp (the host program over csrc/k1_consts.h) for the K1 fp16 tests."""
import functools
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("C", "K2", "K0", "eps_u", "eps_w")


@functools.lru_cache(maxsize=None)
def program():
    out = os.path.join(tempfile.mkdtemp(prefix="k1consts"), "k1_f16_consts_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I" + os.path.join(ROOT, "teaser-plusplus_amd", "csrc"),
                           os.path.join(ROOT, "tests", "k1_f16_consts_main.cpp"), "-o", out])
    return out


def host_consts(cases):
    """cases: [(beta, shift, r2 as np.float32)] -> list of dicts like the model's consts()"""
    args = []
    for beta, s, r2 in cases:
        args += [float(beta).hex(), str(int(s)), str(int(np.float32(r2).view(np.uint32)))]
    lines = subprocess.check_output([program()] + args, text=True).split("\n")
    res = []
    for l in lines[:len(cases)]:
        t = l.split()
        d = {k: np.float32(float.fromhex(v)) for k, v in zip(FIELDS, t)}
        d["kexp"], d["use_mfma"] = int(t[5]), int(t[6])
        res.append(d)
    return res


def host_shift(H):
    return int(subprocess.check_output([program(), "shift", float(H).hex()], text=True))
