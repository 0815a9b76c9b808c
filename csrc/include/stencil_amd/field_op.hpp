// What the operators on pitched quantities share (csrc/src/vector_ops.hip,
// grid_transfer.hip, diffusion_op.hip, stencil_op.hip, jacobi.hip): the
// 16 B strip of the row kernels and the argument checks every entry point
// makes before it launches or allocates anything. Internal: not part of
// ops.hpp's API.
//
// Every check takes the op's name for its message and throws
// std::invalid_argument.
#pragma once

#include <algorithm>
#include <cstdint>
#include <initializer_list>
#include <stdexcept>
#include <string>

#include "stencil_amd/domain.hpp"
#include "stencil_amd/engine.hpp"

namespace stencil_amd {

//// device: one 16 B strip of a row
typedef float F4 __attribute__((ext_vector_type(4)));
typedef double D2 __attribute__((ext_vector_type(2)));
template <typename T> struct Strip;
template <> struct Strip<float> {
  static constexpr int N = 4;
  typedef F4 vec;
};
template <> struct Strip<double> {
  static constexpr int N = 2;
  typedef D2 vec;
};

//// host
inline bool rect_inside(const Rect3 &r, const Rect3 &full) {
  return r.lo.x >= full.lo.x && r.lo.y >= full.lo.y && r.lo.z >= full.lo.z &&
         r.hi.x <= full.hi.x && r.hi.y <= full.hi.y && r.hi.z <= full.hi.z;
}

// blocks of a linearised grid-stride walk over `total` cells
inline uint32_t grid_for(int64_t total, int block) {
  int64_t g = (total + block - 1) / block;
  // cap: 256 CUs x 16 blocks keeps the chip full while bounding launch size
  g = std::min<int64_t>(g, 256 * 16);
  return (uint32_t)std::max<int64_t>(g, 1);
}

// cells from ptr to the next 16 B-aligned ADDRESS (the allocation pad shifts
// the base, so index-aligned strips would be misaligned)
inline int64_t head_cells(const void *ptr, int64_t elemSize) {
  return (int64_t)((16 - ((uintptr_t)ptr & 15)) & 15) / elemSize;
}

inline LocalDomain &checked_domain(const char *op, ExchangeEngine &eng, int dom,
                                   const char *what = "domain") {
  if (dom < 0 || dom >= eng.num_domains())
    throw std::invalid_argument(std::string(op) + ": no such " + what + " " + std::to_string(dom));
  return eng.domain(dom);
}

// one buffer of a quantity
struct Operand {
  int64_t q;
  bool next;
};

// The element size the operands share: each a quantity of d, of 4 or 8
// bytes (want != 0: of `want` bytes), and `common` (from operands checked
// before, 0: none) the size of all.
inline int64_t checked_elem_size(const char *op, const LocalDomain &d,
                                 std::initializer_list<Operand> operands, int64_t want = 0,
                                 int64_t common = 0) {
  for (const Operand &o : operands) {
    if (o.q < 0 || o.q >= d.num_data()) throw std::invalid_argument(std::string(op) + ": no such quantity");
    const int64_t es = d.elem_size(o.q);
    if (want != 0 ? es != want : (es != 4 && es != 8))
      throw std::invalid_argument(std::string(op) + ": " +
                                  (want != 0 ? std::to_string(want) + "-byte"
                                             : std::string("float32/float64")) +
                                  " quantities only (element size " + std::to_string(es) + ")");
    if (common != 0 && es != common)
      throw std::invalid_argument(std::string(op) + ": operands differ in element size");
    common = es;
  }
  return common;
}

// false: an empty region, which every op takes as a no-op
inline bool checked_extent(const char *op, const Rect3 &region,
                           int64_t limit = 0x7fffffff) {
  const Vec3 ext = region.extent();
  if (ext.x <= 0 || ext.y <= 0 || ext.z <= 0) return false;
  if (ext.x > limit || ext.y > limit || ext.z > limit)
    throw std::invalid_argument(std::string(op) + ": region extent exceeds " + std::to_string(limit));
  return true;
}

// r, grown by `apron` cells on every side, lies inside the allocation
inline void check_inside(const char *op, const char *what, const Rect3 &r,
                         const Rect3 &full, int64_t apron = 0) {
  const Vec3 a(apron, apron, apron);
  if (!rect_inside(Rect3(r.lo - a, r.hi + a), full))
    throw std::invalid_argument(std::string(op) + ": " + what + " " + r.str() +
                                (apron ? " plus its " + std::to_string(apron) + "-cell apron" : "") +
                                " leaves the allocation " + full.str());
}

// The region's first cell in every operand's buffer, `pos` being the
// region's lo in allocation coordinates; the buffers share one layout.
struct RegionCells {
  static constexpr int kMax = 6;
  int64_t pitch = 0, plane = 0; // byte strides, the same for every operand
  int n = 0;
  char *ptr[kMax] = {};
};
inline RegionCells region_cells(const char *op, const LocalDomain &d,
                                std::initializer_list<Operand> operands, const Vec3 &pos,
                                int64_t elemSize) {
  RegionCells c;
  const Pitched &first = d.curr(operands.begin()->q);
  c.pitch = first.pitch;
  c.plane = first.plane();
  for (const Operand &o : operands) {
    const Pitched &pp = o.next ? d.next(o.q) : d.curr(o.q);
    if (pp.pitch != first.pitch || pp.ysize != first.ysize)
      throw std::invalid_argument(std::string(op) + ": operand layouts differ");
    c.ptr[c.n++] = pp.ptr + pos.z * pp.plane() + pos.y * pp.pitch + pos.x * elemSize;
  }
  return c;
}

} // namespace stencil_amd
