"""The host side of the ray cast of the TSDF volume without a GPU: csrc/tsdf.hip and csrc/tsdf_raycast.hip compiled by
g++ against the HIP stand-in header with a CPU stand-in for the launcher, which calls tsdf_ray_thread of
csrc/tsdf_raycast_device.h -- the text the kernel compiles -- for every thread of every block
(tests/tsdf_raycast_host_driver.cpp).  Built with -ffp-contract=off under AddressSanitizer and UndefinedBehaviorSanitizer
and run as a stand-alone program.  The entry checks, the view records, the block map, the output layout for mixed view
sizes, NULL arrays and NULL entries and every refusal with its text run for real; depth, vertex, normal and colour maps
are compared bit for bit, and the hit counts, with the restatement's (tests/tsdf_raycast_reference.py): the `host` cases
of tsdf_reference.cases() and random volumes of 2, 3 and 6 voxels a side in the three colour types."""
import subprocess

import numpy as np

import tsdf_raycast_reference as RC
import tsdf_reference as T
from test_outlier_host import hexes, ints
from test_search_host import compile_driver


def bits(a):
    return ints(np.ascontiguousarray(a, dtype=np.float32).view(np.uint32))


def case_lines(vol, views):
    ctype = vol.color_type
    lines = ["%d %d" % (vol.R, ctype), hexes([vol.length, vol.sdf_trunc]) + " " + hexes(vol.origin), hexes(vol.tsdf_weight()),
             hexes(vol.colors()) if ctype else "", str(len(views))]
    hit = miss = 0
    for w in views:
        r = RC.cast(vol, w)
        hit, miss = hit + r.hits, miss + w.width * w.height - r.hits
        lines += ["%d %d" % (w.width, w.height), hexes(w.K), hexes(w.E), hexes([w.depth_min, w.depth_max, w.weight_threshold]),
                  str(r.hits), bits(r.depth), bits(r.vertex), bits(r.normal), bits(r.color) if ctype else ""]
    return lines, hit, miss


def host_cases():
    """(volume, views): three views of different sizes and a 0 x 0 one per volume."""
    out = []
    for cs in T.cases().values():
        if not cs.host:
            continue
        vol = T.result(cs.name).vol
        thr = 1.0 if len(cs.frames) < 3 else 3.0
        views = [RC.view(9, 7, np.eye(4), weight_threshold=thr), RC.view(17, 5, T.extrinsic(0.05, -0.1, 0.3, (0.02, -0.01, 0.1)), weight_threshold=thr),
                 RC.view(0, 0, np.eye(4)), RC.view(3, 18, RC.look_at_volume(vol, 0.2, 0.1, 1.1), weight_threshold=0.0)]
        out.append((vol, views))
    for R, seed, ctype, thr, weight in ((2, 4, T.RGB8, 1.0, 2.0), (3, 21, T.GRAY32, 0.0, 2.0), (6, 2, T.NONE, 3.0, 4.0), (6, 24, T.RGB8, 1.0, 2.0),
                                        (3, 22, T.NONE, 1.0, 2.0), (6, 30, T.GRAY32, 3.0, 4.0)):
        vol = RC.random_volume(R, seed, ctype, weight)
        out.append((vol, RC.views_around(vol, thr, ((8, 8), (17, 9), (0, 5), (33, 17)))))
    return out


def test_host_code_is_clean_and_equal_to_the_restatement(tmp_path):
    cases = host_cases()
    assert {v.color_type for v, _ in cases} == {T.NONE, T.RGB8, T.GRAY32}
    lines = [str(len(cases))]
    hits = []
    for vol, views in cases:
        text, hit, miss = case_lines(vol, views)
        lines += text
        hits.append((hit, miss))
    # most cases must show both outcomes, or equality would say little; the empty volume can only miss
    assert sum(h > 0 and m > 0 for h, m in hits) >= len(cases) - 3, hits
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    exe = compile_driver("tsdf_raycast_host_driver", tmp_path)
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "mismatches 0" in out.stdout, out.stdout + out.stderr[-4000:]
