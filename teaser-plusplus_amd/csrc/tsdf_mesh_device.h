// tsdf_mesh_device.h -- the per-cube rules of the triangle mesh of the TSDF volume (include/teaser_hip.h, "TSDF volume",
// the triangle mesh; kernels: kernels_tsdf_mesh.hip, host side: tsdf_mesh.hip, design: DESIGN.md section 34): the
// marching-cubes tables, the byte of a cube, which cube creates the vertex of a lattice edge, what a column counts, and
// the vertex and triangle rows a column writes.  Nothing here uses a wave operation or LDS, so
// tests/tsdf_mesh_host_driver.cpp runs this very source in serial loops.
//
// The tables are namespace-scope constants: the compiler places them in the constant address space of the code object,
// and every index into them is a load from there, never from a private array.
#pragma once

#include "tsdf_device.h"

namespace thip {

// tri_table[256][16]: Paul Bourke's public-domain "polygonise" table, edge numbers, -1 terminated.
constexpr int8_t kTsdfTriTable[256 * 16] = {
    -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
    0, 8, 3, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
    0, 1, 9, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
    1, 8, 3, 9, 8, 1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
    1, 2, 10, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
    0, 8, 3, 1, 2, 10, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
    9, 2, 10, 0, 2, 9, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
    2, 8, 3, 2, 10, 8, 10, 9, 8, -1, -1, -1, -1, -1, -1, -1,
    3, 11, 2, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
    0, 11, 2, 8, 11, 0, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
    1, 9, 0, 2, 3, 11, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
    1, 11, 2, 1, 9, 11, 9, 8, 11, -1, -1, -1, -1, -1, -1, -1,
    3, 10, 1, 11, 10, 3, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
    0, 10, 1, 0, 8, 10, 8, 11, 10, -1, -1, -1, -1, -1, -1, -1,
    3, 9, 0, 3, 11, 9, 11, 10, 9, -1, -1, -1, -1, -1, -1, -1,
    9, 8, 10, 10, 8, 11, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
    4, 7, 8, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
    4, 3, 0, 7, 3, 4, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
    0, 1, 9, 8, 4, 7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
    4, 1, 9, 4, 7, 1, 7, 3, 1, -1, -1, -1, -1, -1, -1, -1,
    1, 2, 10, 8, 4, 7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
    3, 4, 7, 3, 0, 4, 1, 2, 10, -1, -1, -1, -1, -1, -1, -1,
    9, 2, 10, 9, 0, 2, 8, 4, 7, -1, -1, -1, -1, -1, -1, -1,
    2, 10, 9, 2, 9, 7, 2, 7, 3, 7, 9, 4, -1, -1, -1, -1,
    8, 4, 7, 3, 11, 2, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
    11, 4, 7, 11, 2, 4, 2, 0, 4, -1, -1, -1, -1, -1, -1, -1,
    9, 0, 1, 8, 4, 7, 2, 3, 11, -1, -1, -1, -1, -1, -1, -1,
    4, 7, 11, 9, 4, 11, 9, 11, 2, 9, 2, 1, -1, -1, -1, -1,
    3, 10, 1, 3, 11, 10, 7, 8, 4, -1, -1, -1, -1, -1, -1, -1,
    1, 11, 10, 1, 4, 11, 1, 0, 4, 7, 11, 4, -1, -1, -1, -1,
    4, 7, 8, 9, 0, 11, 9, 11, 10, 11, 0, 3, -1, -1, -1, -1,
    4, 7, 11, 4, 11, 9, 9, 11, 10, -1, -1, -1, -1, -1, -1, -1,
    9, 5, 4, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
    9, 5, 4, 0, 8, 3, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
    0, 5, 4, 1, 5, 0, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
    8, 5, 4, 8, 3, 5, 3, 1, 5, -1, -1, -1, -1, -1, -1, -1,
    1, 2, 10, 9, 5, 4, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
    3, 0, 8, 1, 2, 10, 4, 9, 5, -1, -1, -1, -1, -1, -1, -1,
    5, 2, 10, 5, 4, 2, 4, 0, 2, -1, -1, -1, -1, -1, -1, -1,
    2, 10, 5, 3, 2, 5, 3, 5, 4, 3, 4, 8, -1, -1, -1, -1,
    9, 5, 4, 2, 3, 11, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
    0, 11, 2, 0, 8, 11, 4, 9, 5, -1, -1, -1, -1, -1, -1, -1,
    0, 5, 4, 0, 1, 5, 2, 3, 11, -1, -1, -1, -1, -1, -1, -1,
    2, 1, 5, 2, 5, 8, 2, 8, 11, 4, 8, 5, -1, -1, -1, -1,
    10, 3, 11, 10, 1, 3, 9, 5, 4, -1, -1, -1, -1, -1, -1, -1,
    4, 9, 5, 0, 8, 1, 8, 10, 1, 8, 11, 10, -1, -1, -1, -1,
    5, 4, 0, 5, 0, 11, 5, 11, 10, 11, 0, 3, -1, -1, -1, -1,
    5, 4, 8, 5, 8, 10, 10, 8, 11, -1, -1, -1, -1, -1, -1, -1,
    9, 7, 8, 5, 7, 9, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
    9, 3, 0, 9, 5, 3, 5, 7, 3, -1, -1, -1, -1, -1, -1, -1,
    0, 7, 8, 0, 1, 7, 1, 5, 7, -1, -1, -1, -1, -1, -1, -1,
    1, 5, 3, 3, 5, 7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
    9, 7, 8, 9, 5, 7, 10, 1, 2, -1, -1, -1, -1, -1, -1, -1,
    10, 1, 2, 9, 5, 0, 5, 3, 0, 5, 7, 3, -1, -1, -1, -1,
    8, 0, 2, 8, 2, 5, 8, 5, 7, 10, 5, 2, -1, -1, -1, -1,
    2, 10, 5, 2, 5, 3, 3, 5, 7, -1, -1, -1, -1, -1, -1, -1,
    7, 9, 5, 7, 8, 9, 3, 11, 2, -1, -1, -1, -1, -1, -1, -1,
    9, 5, 7, 9, 7, 2, 9, 2, 0, 2, 7, 11, -1, -1, -1, -1,
    2, 3, 11, 0, 1, 8, 1, 7, 8, 1, 5, 7, -1, -1, -1, -1,
    11, 2, 1, 11, 1, 7, 7, 1, 5, -1, -1, -1, -1, -1, -1, -1,
    9, 5, 8, 8, 5, 7, 10, 1, 3, 10, 3, 11, -1, -1, -1, -1,
    5, 7, 0, 5, 0, 9, 7, 11, 0, 1, 0, 10, 11, 10, 0, -1,
    11, 10, 0, 11, 0, 3, 10, 5, 0, 8, 0, 7, 5, 7, 0, -1,
    11, 10, 5, 7, 11, 5, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
    10, 6, 5, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
    0, 8, 3, 5, 10, 6, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
    9, 0, 1, 5, 10, 6, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
    1, 8, 3, 1, 9, 8, 5, 10, 6, -1, -1, -1, -1, -1, -1, -1,
    1, 6, 5, 2, 6, 1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
    1, 6, 5, 1, 2, 6, 3, 0, 8, -1, -1, -1, -1, -1, -1, -1,
    9, 6, 5, 9, 0, 6, 0, 2, 6, -1, -1, -1, -1, -1, -1, -1,
    5, 9, 8, 5, 8, 2, 5, 2, 6, 3, 2, 8, -1, -1, -1, -1,
    2, 3, 11, 10, 6, 5, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
    11, 0, 8, 11, 2, 0, 10, 6, 5, -1, -1, -1, -1, -1, -1, -1,
    0, 1, 9, 2, 3, 11, 5, 10, 6, -1, -1, -1, -1, -1, -1, -1,
    5, 10, 6, 1, 9, 2, 9, 11, 2, 9, 8, 11, -1, -1, -1, -1,
    6, 3, 11, 6, 5, 3, 5, 1, 3, -1, -1, -1, -1, -1, -1, -1,
    0, 8, 11, 0, 11, 5, 0, 5, 1, 5, 11, 6, -1, -1, -1, -1,
    3, 11, 6, 0, 3, 6, 0, 6, 5, 0, 5, 9, -1, -1, -1, -1,
    6, 5, 9, 6, 9, 11, 11, 9, 8, -1, -1, -1, -1, -1, -1, -1,
    5, 10, 6, 4, 7, 8, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
    4, 3, 0, 4, 7, 3, 6, 5, 10, -1, -1, -1, -1, -1, -1, -1,
    1, 9, 0, 5, 10, 6, 8, 4, 7, -1, -1, -1, -1, -1, -1, -1,
    10, 6, 5, 1, 9, 7, 1, 7, 3, 7, 9, 4, -1, -1, -1, -1,
    6, 1, 2, 6, 5, 1, 4, 7, 8, -1, -1, -1, -1, -1, -1, -1,
    1, 2, 5, 5, 2, 6, 3, 0, 4, 3, 4, 7, -1, -1, -1, -1,
    8, 4, 7, 9, 0, 5, 0, 6, 5, 0, 2, 6, -1, -1, -1, -1,
    7, 3, 9, 7, 9, 4, 3, 2, 9, 5, 9, 6, 2, 6, 9, -1,
    3, 11, 2, 7, 8, 4, 10, 6, 5, -1, -1, -1, -1, -1, -1, -1,
    5, 10, 6, 4, 7, 2, 4, 2, 0, 2, 7, 11, -1, -1, -1, -1,
    0, 1, 9, 4, 7, 8, 2, 3, 11, 5, 10, 6, -1, -1, -1, -1,
    9, 2, 1, 9, 11, 2, 9, 4, 11, 7, 11, 4, 5, 10, 6, -1,
    8, 4, 7, 3, 11, 5, 3, 5, 1, 5, 11, 6, -1, -1, -1, -1,
    5, 1, 11, 5, 11, 6, 1, 0, 11, 7, 11, 4, 0, 4, 11, -1,
    0, 5, 9, 0, 6, 5, 0, 3, 6, 11, 6, 3, 8, 4, 7, -1,
    6, 5, 9, 6, 9, 11, 4, 7, 9, 7, 11, 9, -1, -1, -1, -1,
    10, 4, 9, 6, 4, 10, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
    4, 10, 6, 4, 9, 10, 0, 8, 3, -1, -1, -1, -1, -1, -1, -1,
    10, 0, 1, 10, 6, 0, 6, 4, 0, -1, -1, -1, -1, -1, -1, -1,
    8, 3, 1, 8, 1, 6, 8, 6, 4, 6, 1, 10, -1, -1, -1, -1,
    1, 4, 9, 1, 2, 4, 2, 6, 4, -1, -1, -1, -1, -1, -1, -1,
    3, 0, 8, 1, 2, 9, 2, 4, 9, 2, 6, 4, -1, -1, -1, -1,
    0, 2, 4, 4, 2, 6, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
    8, 3, 2, 8, 2, 4, 4, 2, 6, -1, -1, -1, -1, -1, -1, -1,
    10, 4, 9, 10, 6, 4, 11, 2, 3, -1, -1, -1, -1, -1, -1, -1,
    0, 8, 2, 2, 8, 11, 4, 9, 10, 4, 10, 6, -1, -1, -1, -1,
    3, 11, 2, 0, 1, 6, 0, 6, 4, 6, 1, 10, -1, -1, -1, -1,
    6, 4, 1, 6, 1, 10, 4, 8, 1, 2, 1, 11, 8, 11, 1, -1,
    9, 6, 4, 9, 3, 6, 9, 1, 3, 11, 6, 3, -1, -1, -1, -1,
    8, 11, 1, 8, 1, 0, 11, 6, 1, 9, 1, 4, 6, 4, 1, -1,
    3, 11, 6, 3, 6, 0, 0, 6, 4, -1, -1, -1, -1, -1, -1, -1,
    6, 4, 8, 11, 6, 8, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
    7, 10, 6, 7, 8, 10, 8, 9, 10, -1, -1, -1, -1, -1, -1, -1,
    0, 7, 3, 0, 10, 7, 0, 9, 10, 6, 7, 10, -1, -1, -1, -1,
    10, 6, 7, 1, 10, 7, 1, 7, 8, 1, 8, 0, -1, -1, -1, -1,
    10, 6, 7, 10, 7, 1, 1, 7, 3, -1, -1, -1, -1, -1, -1, -1,
    1, 2, 6, 1, 6, 8, 1, 8, 9, 8, 6, 7, -1, -1, -1, -1,
    2, 6, 9, 2, 9, 1, 6, 7, 9, 0, 9, 3, 7, 3, 9, -1,
    7, 8, 0, 7, 0, 6, 6, 0, 2, -1, -1, -1, -1, -1, -1, -1,
    7, 3, 2, 6, 7, 2, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
    2, 3, 11, 10, 6, 8, 10, 8, 9, 8, 6, 7, -1, -1, -1, -1,
    2, 0, 7, 2, 7, 11, 0, 9, 7, 6, 7, 10, 9, 10, 7, -1,
    1, 8, 0, 1, 7, 8, 1, 10, 7, 6, 7, 10, 2, 3, 11, -1,
    11, 2, 1, 11, 1, 7, 10, 6, 1, 6, 7, 1, -1, -1, -1, -1,
    8, 9, 6, 8, 6, 7, 9, 1, 6, 11, 6, 3, 1, 3, 6, -1,
    0, 9, 1, 11, 6, 7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
    7, 8, 0, 7, 0, 6, 3, 11, 0, 11, 6, 0, -1, -1, -1, -1,
    7, 11, 6, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
    7, 6, 11, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
    3, 0, 8, 11, 7, 6, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
    0, 1, 9, 11, 7, 6, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
    8, 1, 9, 8, 3, 1, 11, 7, 6, -1, -1, -1, -1, -1, -1, -1,
    10, 1, 2, 6, 11, 7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
    1, 2, 10, 3, 0, 8, 6, 11, 7, -1, -1, -1, -1, -1, -1, -1,
    2, 9, 0, 2, 10, 9, 6, 11, 7, -1, -1, -1, -1, -1, -1, -1,
    6, 11, 7, 2, 10, 3, 10, 8, 3, 10, 9, 8, -1, -1, -1, -1,
    7, 2, 3, 6, 2, 7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
    7, 0, 8, 7, 6, 0, 6, 2, 0, -1, -1, -1, -1, -1, -1, -1,
    2, 7, 6, 2, 3, 7, 0, 1, 9, -1, -1, -1, -1, -1, -1, -1,
    1, 6, 2, 1, 8, 6, 1, 9, 8, 8, 7, 6, -1, -1, -1, -1,
    10, 7, 6, 10, 1, 7, 1, 3, 7, -1, -1, -1, -1, -1, -1, -1,
    10, 7, 6, 1, 7, 10, 1, 8, 7, 1, 0, 8, -1, -1, -1, -1,
    0, 3, 7, 0, 7, 10, 0, 10, 9, 6, 10, 7, -1, -1, -1, -1,
    7, 6, 10, 7, 10, 8, 8, 10, 9, -1, -1, -1, -1, -1, -1, -1,
    6, 8, 4, 11, 8, 6, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
    3, 6, 11, 3, 0, 6, 0, 4, 6, -1, -1, -1, -1, -1, -1, -1,
    8, 6, 11, 8, 4, 6, 9, 0, 1, -1, -1, -1, -1, -1, -1, -1,
    9, 4, 6, 9, 6, 3, 9, 3, 1, 11, 3, 6, -1, -1, -1, -1,
    6, 8, 4, 6, 11, 8, 2, 10, 1, -1, -1, -1, -1, -1, -1, -1,
    1, 2, 10, 3, 0, 11, 0, 6, 11, 0, 4, 6, -1, -1, -1, -1,
    4, 11, 8, 4, 6, 11, 0, 2, 9, 2, 10, 9, -1, -1, -1, -1,
    10, 9, 3, 10, 3, 2, 9, 4, 3, 11, 3, 6, 4, 6, 3, -1,
    8, 2, 3, 8, 4, 2, 4, 6, 2, -1, -1, -1, -1, -1, -1, -1,
    0, 4, 2, 4, 6, 2, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
    1, 9, 0, 2, 3, 4, 2, 4, 6, 4, 3, 8, -1, -1, -1, -1,
    1, 9, 4, 1, 4, 2, 2, 4, 6, -1, -1, -1, -1, -1, -1, -1,
    8, 1, 3, 8, 6, 1, 8, 4, 6, 6, 10, 1, -1, -1, -1, -1,
    10, 1, 0, 10, 0, 6, 6, 0, 4, -1, -1, -1, -1, -1, -1, -1,
    4, 6, 3, 4, 3, 8, 6, 10, 3, 0, 3, 9, 10, 9, 3, -1,
    10, 9, 4, 6, 10, 4, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
    4, 9, 5, 7, 6, 11, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
    0, 8, 3, 4, 9, 5, 11, 7, 6, -1, -1, -1, -1, -1, -1, -1,
    5, 0, 1, 5, 4, 0, 7, 6, 11, -1, -1, -1, -1, -1, -1, -1,
    11, 7, 6, 8, 3, 4, 3, 5, 4, 3, 1, 5, -1, -1, -1, -1,
    9, 5, 4, 10, 1, 2, 7, 6, 11, -1, -1, -1, -1, -1, -1, -1,
    6, 11, 7, 1, 2, 10, 0, 8, 3, 4, 9, 5, -1, -1, -1, -1,
    7, 6, 11, 5, 4, 10, 4, 2, 10, 4, 0, 2, -1, -1, -1, -1,
    3, 4, 8, 3, 5, 4, 3, 2, 5, 10, 5, 2, 11, 7, 6, -1,
    7, 2, 3, 7, 6, 2, 5, 4, 9, -1, -1, -1, -1, -1, -1, -1,
    9, 5, 4, 0, 8, 6, 0, 6, 2, 6, 8, 7, -1, -1, -1, -1,
    3, 6, 2, 3, 7, 6, 1, 5, 0, 5, 4, 0, -1, -1, -1, -1,
    6, 2, 8, 6, 8, 7, 2, 1, 8, 4, 8, 5, 1, 5, 8, -1,
    9, 5, 4, 10, 1, 6, 1, 7, 6, 1, 3, 7, -1, -1, -1, -1,
    1, 6, 10, 1, 7, 6, 1, 0, 7, 8, 7, 0, 9, 5, 4, -1,
    4, 0, 10, 4, 10, 5, 0, 3, 10, 6, 10, 7, 3, 7, 10, -1,
    7, 6, 10, 7, 10, 8, 5, 4, 10, 4, 8, 10, -1, -1, -1, -1,
    6, 9, 5, 6, 11, 9, 11, 8, 9, -1, -1, -1, -1, -1, -1, -1,
    3, 6, 11, 0, 6, 3, 0, 5, 6, 0, 9, 5, -1, -1, -1, -1,
    0, 11, 8, 0, 5, 11, 0, 1, 5, 5, 6, 11, -1, -1, -1, -1,
    6, 11, 3, 6, 3, 5, 5, 3, 1, -1, -1, -1, -1, -1, -1, -1,
    1, 2, 10, 9, 5, 11, 9, 11, 8, 11, 5, 6, -1, -1, -1, -1,
    0, 11, 3, 0, 6, 11, 0, 9, 6, 5, 6, 9, 1, 2, 10, -1,
    11, 8, 5, 11, 5, 6, 8, 0, 5, 10, 5, 2, 0, 2, 5, -1,
    6, 11, 3, 6, 3, 5, 2, 10, 3, 10, 5, 3, -1, -1, -1, -1,
    5, 8, 9, 5, 2, 8, 5, 6, 2, 3, 8, 2, -1, -1, -1, -1,
    9, 5, 6, 9, 6, 0, 0, 6, 2, -1, -1, -1, -1, -1, -1, -1,
    1, 5, 8, 1, 8, 0, 5, 6, 8, 3, 8, 2, 6, 2, 8, -1,
    1, 5, 6, 2, 1, 6, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
    1, 3, 6, 1, 6, 10, 3, 8, 6, 5, 6, 9, 8, 9, 6, -1,
    10, 1, 0, 10, 0, 6, 9, 5, 0, 5, 6, 0, -1, -1, -1, -1,
    0, 3, 8, 5, 6, 10, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
    10, 5, 6, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
    11, 5, 10, 7, 5, 11, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
    11, 5, 10, 11, 7, 5, 8, 3, 0, -1, -1, -1, -1, -1, -1, -1,
    5, 11, 7, 5, 10, 11, 1, 9, 0, -1, -1, -1, -1, -1, -1, -1,
    10, 7, 5, 10, 11, 7, 9, 8, 1, 8, 3, 1, -1, -1, -1, -1,
    11, 1, 2, 11, 7, 1, 7, 5, 1, -1, -1, -1, -1, -1, -1, -1,
    0, 8, 3, 1, 2, 7, 1, 7, 5, 7, 2, 11, -1, -1, -1, -1,
    9, 7, 5, 9, 2, 7, 9, 0, 2, 2, 11, 7, -1, -1, -1, -1,
    7, 5, 2, 7, 2, 11, 5, 9, 2, 3, 2, 8, 9, 8, 2, -1,
    2, 5, 10, 2, 3, 5, 3, 7, 5, -1, -1, -1, -1, -1, -1, -1,
    8, 2, 0, 8, 5, 2, 8, 7, 5, 10, 2, 5, -1, -1, -1, -1,
    9, 0, 1, 5, 10, 3, 5, 3, 7, 3, 10, 2, -1, -1, -1, -1,
    9, 8, 2, 9, 2, 1, 8, 7, 2, 10, 2, 5, 7, 5, 2, -1,
    1, 3, 5, 3, 7, 5, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
    0, 8, 7, 0, 7, 1, 1, 7, 5, -1, -1, -1, -1, -1, -1, -1,
    9, 0, 3, 9, 3, 5, 5, 3, 7, -1, -1, -1, -1, -1, -1, -1,
    9, 8, 7, 5, 9, 7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
    5, 8, 4, 5, 10, 8, 10, 11, 8, -1, -1, -1, -1, -1, -1, -1,
    5, 0, 4, 5, 11, 0, 5, 10, 11, 11, 3, 0, -1, -1, -1, -1,
    0, 1, 9, 8, 4, 10, 8, 10, 11, 10, 4, 5, -1, -1, -1, -1,
    10, 11, 4, 10, 4, 5, 11, 3, 4, 9, 4, 1, 3, 1, 4, -1,
    2, 5, 1, 2, 8, 5, 2, 11, 8, 4, 5, 8, -1, -1, -1, -1,
    0, 4, 11, 0, 11, 3, 4, 5, 11, 2, 11, 1, 5, 1, 11, -1,
    0, 2, 5, 0, 5, 9, 2, 11, 5, 4, 5, 8, 11, 8, 5, -1,
    9, 4, 5, 2, 11, 3, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
    2, 5, 10, 3, 5, 2, 3, 4, 5, 3, 8, 4, -1, -1, -1, -1,
    5, 10, 2, 5, 2, 4, 4, 2, 0, -1, -1, -1, -1, -1, -1, -1,
    3, 10, 2, 3, 5, 10, 3, 8, 5, 4, 5, 8, 0, 1, 9, -1,
    5, 10, 2, 5, 2, 4, 1, 9, 2, 9, 4, 2, -1, -1, -1, -1,
    8, 4, 5, 8, 5, 3, 3, 5, 1, -1, -1, -1, -1, -1, -1, -1,
    0, 4, 5, 1, 0, 5, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
    8, 4, 5, 8, 5, 3, 9, 0, 5, 0, 3, 5, -1, -1, -1, -1,
    9, 4, 5, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
    4, 11, 7, 4, 9, 11, 9, 10, 11, -1, -1, -1, -1, -1, -1, -1,
    0, 8, 3, 4, 9, 7, 9, 11, 7, 9, 10, 11, -1, -1, -1, -1,
    1, 10, 11, 1, 11, 4, 1, 4, 0, 7, 4, 11, -1, -1, -1, -1,
    3, 1, 4, 3, 4, 8, 1, 10, 4, 7, 4, 11, 10, 11, 4, -1,
    4, 11, 7, 9, 11, 4, 9, 2, 11, 9, 1, 2, -1, -1, -1, -1,
    9, 7, 4, 9, 11, 7, 9, 1, 11, 2, 11, 1, 0, 8, 3, -1,
    11, 7, 4, 11, 4, 2, 2, 4, 0, -1, -1, -1, -1, -1, -1, -1,
    11, 7, 4, 11, 4, 2, 8, 3, 4, 3, 2, 4, -1, -1, -1, -1,
    2, 9, 10, 2, 7, 9, 2, 3, 7, 7, 4, 9, -1, -1, -1, -1,
    9, 10, 7, 9, 7, 4, 10, 2, 7, 8, 7, 0, 2, 0, 7, -1,
    3, 7, 10, 3, 10, 2, 7, 4, 10, 1, 10, 0, 4, 0, 10, -1,
    1, 10, 2, 8, 7, 4, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
    4, 9, 1, 4, 1, 7, 7, 1, 3, -1, -1, -1, -1, -1, -1, -1,
    4, 9, 1, 4, 1, 7, 0, 8, 1, 8, 7, 1, -1, -1, -1, -1,
    4, 0, 3, 7, 4, 3, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
    4, 8, 7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
    9, 10, 8, 10, 11, 8, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
    3, 0, 9, 3, 9, 11, 11, 9, 10, -1, -1, -1, -1, -1, -1, -1,
    0, 1, 10, 0, 10, 8, 8, 10, 11, -1, -1, -1, -1, -1, -1, -1,
    3, 1, 10, 11, 3, 10, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
    1, 2, 11, 1, 11, 9, 9, 11, 8, -1, -1, -1, -1, -1, -1, -1,
    3, 0, 9, 3, 9, 11, 1, 2, 9, 2, 11, 9, -1, -1, -1, -1,
    0, 2, 11, 8, 0, 11, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
    3, 2, 11, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
    2, 3, 8, 2, 8, 10, 10, 8, 9, -1, -1, -1, -1, -1, -1, -1,
    9, 10, 2, 0, 9, 2, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
    2, 3, 8, 2, 8, 10, 0, 1, 8, 1, 10, 8, -1, -1, -1, -1,
    1, 10, 2, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
    1, 3, 8, 9, 1, 8, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
    0, 9, 1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
    0, 3, 8, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
    -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
};

// edge_to_vert[12][2]: the corners of an edge, the base voxel first.
constexpr int8_t kTsdfEdgeCorner[12][2] = {{0, 1}, {1, 2}, {3, 2}, {0, 3}, {4, 5}, {5, 6},
                                           {7, 6}, {4, 7}, {0, 4}, {1, 5}, {2, 6}, {3, 7}};
constexpr int8_t kTsdfEdgeAxis[12] = {0, 1, 0, 1, 0, 1, 0, 1, 2, 2, 2, 2};

// The cubes that contain edge i of a cube and come before that cube in (x, y, z) order, themselves in that order: the
// offset to the cube and the number the edge has there.  Edges 5, 6 and 10 have none.
constexpr int8_t kTsdfEarlierCount[12] = {3, 1, 1, 3, 2, 0, 0, 2, 3, 1, 0, 2};
constexpr int8_t kTsdfEarlier[12][3][4] = {
    {{0, -1, -1, 6}, {0, -1, 0, 2}, {0, 0, -1, 4}},   // 0
    {{0, 0, -1, 5}, {0, 0, 0, 0}, {0, 0, 0, 0}},      // 1
    {{0, 0, -1, 6}, {0, 0, 0, 0}, {0, 0, 0, 0}},      // 2
    {{-1, 0, -1, 5}, {-1, 0, 0, 1}, {0, 0, -1, 7}},   // 3
    {{0, -1, 0, 6}, {0, -1, 1, 2}, {0, 0, 0, 0}},     // 4
    {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}},       // 5
    {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}},       // 6
    {{-1, 0, 0, 5}, {-1, 0, 1, 1}, {0, 0, 0, 0}},     // 7
    {{-1, -1, 0, 10}, {-1, 0, 0, 9}, {0, -1, 0, 11}}, // 8
    {{0, -1, 0, 10}, {0, 0, 0, 0}, {0, 0, 0, 0}},     // 9
    {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}},       // 10
    {{-1, 0, 0, 10}, {-1, 1, 0, 9}, {0, 0, 0, 0}},    // 11
};

// shift[8]: the offset of corner i.
__host__ __device__ __forceinline__ int tsdf_corner_x(int i) { return (i ^ (i >> 1)) & 1; }
__host__ __device__ __forceinline__ int tsdf_corner_y(int i) { return (i >> 1) & 1; }
__host__ __device__ __forceinline__ int tsdf_corner_z(int i) { return (i >> 2) & 1; }

// edge_table[cube_index]: bit i is set when the two corners of edge i differ in sign.  Edges 0 .. 3 run round the lower
// face, 4 .. 7 round the upper one, 8 .. 11 join them.
__host__ __device__ __forceinline__ int tsdf_edge_mask(int cube_index) {
  const int lo = cube_index & 15, hi = cube_index >> 4;
  const int ring_lo = (lo ^ ((lo >> 1) | (lo << 3))) & 15, ring_hi = (hi ^ ((hi >> 1) | (hi << 3))) & 15;
  return ring_lo | (ring_hi << 4) | ((lo ^ hi) << 8);
}

// The triangles of a cube: a third of the length of its row of the table.
__host__ __device__ __forceinline__ int tsdf_cube_triangles(int cube_index) {
  int t = 0;
  while (t < 5 && kTsdfTriTable[cube_index * 16 + 3 * t] >= 0) ++t;
  return t;
}

// Layer z of the four voxel columns round cube column (x, y), in the order of corners 0 .. 3: bits 0 .. 3 tsdf < 0.0f,
// bits 4 .. 7 weight != 0.  x, y < R - 1 and z < R.
__host__ __device__ __forceinline__ int tsdf_mesh_layer(const TsdfGrid& g, const TsdfFields& v, int x, int y, int z) {
  int bits = 0;
  for (int i = 0; i < 4; ++i) {
    const int64_t at = tsdf_index(g.R, x + tsdf_corner_x(i), y + tsdf_corner_y(i), z);
    bits |= (v.tsdf[at] < 0.0f ? 1 : 0) << i;
    bits |= (v.weight[at] != 0.0f ? 16 : 0) << i;
  }
  return bits;
}

// The byte of a cube from its two layers: cube_index when the cube is ACTIVE, else 0.
__host__ __device__ __forceinline__ unsigned char tsdf_cube_byte(int lower, int upper) {
  const int cube_index = (lower & 15) | ((upper & 15) << 4);
  const bool active = ((lower & upper) >> 4) == 15 && cube_index != 0 && cube_index != 255;
  return (unsigned char)(active ? cube_index : 0);
}

// Pass A of column (x, y): the bytes of its cubes.  A column with x or y = R - 1 has no cube and writes nothing.
__host__ __device__ __forceinline__ void tsdf_mesh_column_cubes(const TsdfGrid& g, const TsdfFields& v, int x, int y,
                                                                unsigned char* cubes) {
  if (x >= g.R - 1 || y >= g.R - 1) return;
  int lower = tsdf_mesh_layer(g, v, x, y, 0);
  for (int z = 0; z < g.R - 1; ++z) {
    const int upper = tsdf_mesh_layer(g, v, x, y, z + 1);
    cubes[tsdf_index(g.R, x, y, z)] = tsdf_cube_byte(lower, upper);
    lower = upper;
  }
}

// Whether (x, y, z) is a cube and ACTIVE.
__host__ __device__ __forceinline__ bool tsdf_cube_active(const unsigned char* cubes, int R, int x, int y, int z) {
  if (x < 0 || y < 0 || z < 0 || x >= R - 1 || y >= R - 1 || z >= R - 1) return false;
  return cubes[tsdf_index(R, x, y, z)] != 0;
}

// The slots the ACTIVE cube (x, y, z) creates: the crossed edges no earlier ACTIVE cube contains.
__host__ __device__ __forceinline__ int tsdf_cube_created(const unsigned char* cubes, int R, int x, int y, int z,
                                                          int cube_index) {
  const int crossed = tsdf_edge_mask(cube_index);
  int created = 0;
  for (int i = 0; i < 12; ++i) {
    if (!((crossed >> i) & 1)) continue;
    bool first = true;
    for (int k = 0; k < kTsdfEarlierCount[i]; ++k) {
      const int8_t* e = kTsdfEarlier[i][k];
      if (tsdf_cube_active(cubes, R, x + e[0], y + e[1], z + e[2])) first = false;
    }
    if (first) created |= 1 << i;
  }
  return created;
}

// The count pass of column (x, y): per ACTIVE cube the record (created slots << 16) | (vertices the column's earlier
// cubes create, at most 12 (R - 1) < 65536); *n_vertices and *n_triangles are the column's sums.
__host__ __device__ __forceinline__ void tsdf_mesh_column_count(const unsigned char* cubes, int R, int x, int y,
                                                                uint32_t* records, int32_t* n_vertices,
                                                                int32_t* n_triangles) {
  int32_t nv = 0, nt = 0;
  if (x < R - 1 && y < R - 1)
    for (int z = 0; z < R - 1; ++z) {
      const int64_t at = tsdf_index(R, x, y, z);
      const int cube_index = cubes[at];
      if (cube_index == 0) continue;
      const int created = tsdf_cube_created(cubes, R, x, y, z, cube_index);
      records[at] = ((uint32_t)created << 16) | (uint32_t)nv;
      nv += __builtin_popcount((unsigned)created);
      nt += tsdf_cube_triangles(cube_index);
    }
  *n_vertices = nv;
  *n_triangles = nt;
}

// The vertex on edge i of cube (x, y, z): position and, where the pointers are given, colour and normal.
__host__ __device__ __forceinline__ void tsdf_mesh_vertex(const TsdfGrid& g, const TsdfFields& v, int x, int y, int z,
                                                          int i, double* vertex, double* color, double* normal) {
  const int a = kTsdfEdgeCorner[i][0], b = kTsdfEdgeCorner[i][1], axis = kTsdfEdgeAxis[i];
  const int bx = x + tsdf_corner_x(a), by = y + tsdf_corner_y(a), bz = z + tsdf_corner_z(a);
  const int64_t at0 = tsdf_index(g.R, bx, by, bz);
  const int64_t at1 = tsdf_index(g.R, x + tsdf_corner_x(b), y + tsdf_corner_y(b), z + tsdf_corner_z(b));
  const double f0 = __builtin_fabs((double)v.tsdf[at0]), f1 = __builtin_fabs((double)v.tsdf[at1]);
  const double den = f0 + f1;
  double p[3] = {g.half + g.vl * (double)bx, g.half + g.vl * (double)by, g.half + g.vl * (double)bz};
  const double step = (f0 * g.vl) / den;
  for (int k = 0; k < 3; ++k)
    if (k == axis) p[k] = p[k] + step;
  for (int k = 0; k < 3; ++k) vertex[k] = p[k] + g.origin[k];
  if (color)
    for (int k = 0; k < 3; ++k) {
      double c0 = v.color[k * v.n + at0], c1 = v.color[k * v.n + at1];
      if (g.color_type == 1) c0 = c0 / 255.0, c1 = c1 / 255.0;
      const double c = (f1 * c0 + f0 * c1) / den;
      color[k] = g.color_type == 2 ? rgbd_canonical(c) : c;
    }
  if (normal) tsdf_normal_at(g, v, p, normal);
}

// Whether rows may be written: both totals fit their capacities and a vertex index fits int32.
__host__ __device__ __forceinline__ bool tsdf_mesh_fits(const int64_t* totals, int64_t vertex_capacity,
                                                        int64_t triangle_capacity) {
  return totals[0] <= vertex_capacity && totals[1] <= triangle_capacity && totals[0] <= 2147483647;
}

// The vertex pass of column (x, y): its created vertices from vertex_offsets[column], cubes by z, slots ascending.
__host__ __device__ __forceinline__ void tsdf_mesh_column_vertices(const TsdfGrid& g, const TsdfFields& v,
                                                                   const unsigned char* cubes, const uint32_t* records,
                                                                   const int64_t* vertex_offsets, int x, int y,
                                                                   double* vertices, double* colors, double* normals) {
  if (x >= g.R - 1 || y >= g.R - 1) return;
  const int64_t column = (int64_t)x * g.R + y;
  if (vertex_offsets[column] == vertex_offsets[column + 1]) return;
  for (int z = 0; z < g.R - 1; ++z) {
    const int64_t at = tsdf_index(g.R, x, y, z);
    if (cubes[at] == 0) continue;
    const uint32_t record = records[at];
    int64_t row = vertex_offsets[column] + (int64_t)(record & 0xffffu);
    for (int i = 0; i < 12; ++i) {
      if (!((record >> (16 + i)) & 1u)) continue;
      tsdf_mesh_vertex(g, v, x, y, z, i, vertices + 3 * row, colors ? colors + 3 * row : nullptr,
                       normals ? normals + 3 * row : nullptr);
      ++row;
    }
  }
}

// The index of the vertex on edge i (crossed) of the ACTIVE cube (x, y, z): the creator is the first ACTIVE cube among
// the earlier ones that contain the edge, else the cube itself; the index is the creator column's offset, the creator's
// count within its column and the rank of the slot among the slots the creator creates.
__host__ __device__ __forceinline__ int32_t tsdf_mesh_vertex_index(const unsigned char* cubes, const uint32_t* records,
                                                                   const int64_t* vertex_offsets, int R, int x, int y,
                                                                   int z, int i) {
  int cx = x, cy = y, cz = z, slot = i;
  for (int k = kTsdfEarlierCount[i] - 1; k >= 0; --k) {  // backwards: the earliest ACTIVE one is kept
    const int8_t* e = kTsdfEarlier[i][k];
    if (tsdf_cube_active(cubes, R, x + e[0], y + e[1], z + e[2])) cx = x + e[0], cy = y + e[1], cz = z + e[2], slot = e[3];
  }
  const uint32_t record = records[tsdf_index(R, cx, cy, cz)];
  const uint32_t before = (record >> 16) & ((1u << slot) - 1u);
  return (int32_t)(vertex_offsets[(int64_t)cx * R + cy] + (int64_t)(record & 0xffffu) + __builtin_popcount(before));
}

// The triangle pass of column (x, y): the rows of its cubes by z from triangle_offsets[column], each row
// (v[T[t]], v[T[t + 2]], v[T[t + 1]]).
__host__ __device__ __forceinline__ void tsdf_mesh_column_triangles(const unsigned char* cubes, const uint32_t* records,
                                                                    const int64_t* vertex_offsets,
                                                                    const int64_t* triangle_offsets, int R, int x, int y,
                                                                    int32_t* triangles) {
  if (x >= R - 1 || y >= R - 1) return;
  const int64_t column = (int64_t)x * R + y;
  int64_t row = triangle_offsets[column];
  if (row == triangle_offsets[column + 1]) return;
  for (int z = 0; z < R - 1; ++z) {
    const int cube_index = cubes[tsdf_index(R, x, y, z)];
    if (cube_index == 0) continue;
    const int8_t* T = kTsdfTriTable + cube_index * 16;
    for (int t = 0; t < 15 && T[t] >= 0; t += 3) {
      triangles[3 * row] = tsdf_mesh_vertex_index(cubes, records, vertex_offsets, R, x, y, z, T[t]);
      triangles[3 * row + 1] = tsdf_mesh_vertex_index(cubes, records, vertex_offsets, R, x, y, z, T[t + 2]);
      triangles[3 * row + 2] = tsdf_mesh_vertex_index(cubes, records, vertex_offsets, R, x, y, z, T[t + 1]);
      ++row;
    }
  }
}

// ---- launchers (kernels_tsdf_mesh.hip; tests/tsdf_mesh_host_driver.cpp has serial stand-ins) ----
// Scratch of a mesh call, all on the handle: one byte and one 32-bit record per voxel (5 bytes per voxel), and per
// column two int32 sums and two int64 offsets.
// cubes[(z R + x) R + y] = the byte of cube (x, y, z).
void launch_tsdf_mesh_cubes(hipStream_t s, const TsdfGrid& g, const TsdfFields& v, unsigned char* d_cubes);
// The records of the ACTIVE cubes, the sums of the columns (d_counts: R R vertex sums, then R R triangle sums), their
// exclusive sums (d_offsets: R R + 1 vertex offsets, then R R + 1 triangle offsets) and d_totals[0 .. 1] = the vertices
// and the triangles of the mesh.
void launch_tsdf_mesh_count(hipStream_t s, const TsdfGrid& g, const unsigned char* d_cubes, uint32_t* d_records,
                            int32_t* d_counts, int64_t* d_offsets, int64_t* d_totals);
// The vertex rows and the triangle rows, unless tsdf_mesh_fits says no (then nothing is written).  d_colors and
// d_normals may be NULL.
void launch_tsdf_mesh_vertices(hipStream_t s, const TsdfGrid& g, const TsdfFields& v, const unsigned char* d_cubes,
                               const uint32_t* d_records, const int64_t* d_offsets, const int64_t* d_totals,
                               int64_t vertex_capacity, int64_t triangle_capacity, double* d_vertices, double* d_colors,
                               double* d_normals);
void launch_tsdf_mesh_triangles(hipStream_t s, const TsdfGrid& g, const unsigned char* d_cubes, const uint32_t* d_records,
                                const int64_t* d_offsets, const int64_t* d_totals, int64_t vertex_capacity,
                                int64_t triangle_capacity, int32_t* d_triangles);

}  // namespace thip
