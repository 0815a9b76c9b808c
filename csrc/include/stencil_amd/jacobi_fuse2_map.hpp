// Integer bookkeeping of jacobi_kernel_fuse2 (csrc/src/jacobi.hip): which
// cells the one gathered load of a wave fetches. Host and device share it,
// so the table is checked on the host over whole grids (bindings.cpp,
// tests/test_jacobi_fuse2_gather_cpu.py) without a launch.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace stencil_amd {

// a mod n for n > 0, in [0, n)
__host__ __device__ inline int32_t f2_pmod(int32_t a, int32_t n) {
  const int32_t m = a % n;
  return m < 0 ? m + n : m;
}

// Extended x indices (cells from the row's first vector) of the true cells
// just outside a tile of 64 vectors that starts at vector `ub`, wrapped at
// the row's ends: `under` is the row's first true cell, `last` its last one
// (in vector body4 - 1).
__host__ __device__ inline int32_t f2_edge_left(int32_t ub, int32_t last) {
  return ub == 0 ? last : ub * 4 - 1;
}
__host__ __device__ inline int32_t f2_edge_right(int32_t ub, int32_t body4, int32_t under) {
  return ub + 63 >= body4 - 1 ? under : (ub + 64) * 4;
}

// The gathered load: per row and plane a wave needs ten scalars from outside
// its tile, five per edge cell e (eL, eR): the t values of e's four x / y
// neighbours and of e itself. Lane 2 j + side holds quantity j of edge
// `side` (0 = eL, 1 = eR):
//   j = 0: +x   1: -x   2: +y   3: -y   4: e itself
// so that lane `side` finds quantity j 2 j lanes above itself. Lanes from 10
// on repeat lane 9. (e's z neighbours are e itself in the planes before and
// after, loaded by the same lane in other iterations.)
constexpr int F2_GATHER_LANES = 10;
constexpr int F2_GATHER_SELF = 8; // first lane of quantity 4

// Byte offset of lane `lane`'s scalar from the cell (extended index 0, row 0)
// of the plane: yo / ym / yp are the wave's own row and the wrapped rows
// below and above it. Every offset addresses a TRUE cell of the plane (x in
// [under, last], row in [0, extY)), for every lane, so no lane holds an
// address outside the allocation; it is below the plane stride, which the
// launcher bounds to 31 bits.
__host__ __device__ inline uint32_t f2_gather_offset(int32_t lane, int32_t eL, int32_t eR,
                                                     int32_t under, int32_t last, int32_t yo,
                                                     int32_t ym, int32_t yp, uint32_t pitch) {
  const int32_t k = lane < F2_GATHER_LANES ? lane : F2_GATHER_LANES - 1;
  const int32_t e = (k & 1) ? eR : eL;
  const int32_t j = k >> 1;
  int32_t x = e, y = yo;
  if (j == 0)
    x = e == last ? under : e + 1;
  else if (j == 1)
    x = e == under ? last : e - 1;
  else if (j == 2)
    y = yp;
  else if (j == 3)
    y = ym;
  return (uint32_t)y * pitch + (uint32_t)x * 4u;
}

} // namespace stencil_amd
