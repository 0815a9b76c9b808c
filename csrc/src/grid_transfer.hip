// Grid transfer on cell-centred 2:1 coarsening for gfx950: the restriction
// (mean of the 8 children of alpha a + beta b) and the piecewise-constant
// prolongation (dst(p) += src(p >> 1)), the two kernels that move data
// between the levels of a geometric multigrid hierarchy. Pure streaming:
// every fine cell of the region is read once (prolongation: and written
// once), every coarse cell once.
//
// Contract (the vector operations'): nothing outside the region is written
// in any buffer, and no cell outside the region (restriction: outside the
// children of the region) is even loaded, so halos may hold NaN.
//
// Fine and coarse allocations differ in pitch, plane and x alignment, so
// both geometries are kernel arguments. The children (2c, 2c + 1) of a
// coarse cell start at allocation index 2 (c - origin) + radius: with the
// common radius 1 that is an odd index, and a 16 B strip aligned by ADDRESS
// would split every pair. The strips here are therefore aligned to PAIRS,
// not to 16 B: they start at the first fine cell of the region, whatever
// its address. gfx950 executes dwordx4 / dwordx2 global accesses at element
// alignment, and with 64 consecutive lanes on consecutive 16 B the wave
// still touches each cache line once. That leaves no head lanes at all and
// one tail lane in fp32 (a region with an odd number of coarse cells).
//
// Two walks over the coarse region, chosen on the host (plan):
//   strips: one thread = 16 B of a fine row pair = 8 B of the coarse row
//     (fp32: 4 fine / 2 coarse cells, fp64: 2 fine / 1 coarse cell),
//     marching zc coarse planes in z. 64 x 4 threads: one wave per coarse
//     row. No division per cell. Needs a region at least 4 coarse cells wide.
//   cells: linearised grid-stride, one coarse cell (a fine pair per row) per
//     lane and step, for the narrow regions.
// No atomics, no LDS. The coarse row of the restriction is written with a
// nontemporal store (write-only, as the star kernel's output); the
// prolongation's fine row is read and written in place with plain accesses.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <initializer_list>
#include <stdexcept>
#include <string>

#include "stencil_amd/domain.hpp"
#include "stencil_amd/engine.hpp"
#include "stencil_amd/field_op.hpp"
#include "stencil_amd/hip_check.hpp"
#include "stencil_amd/ops.hpp"

namespace stencil_amd {

namespace {

constexpr int kBx = 64, kBy = 4;      // strip block: one wave per coarse row, 4 rows
constexpr int kMinZc = 4;             // coarse planes per thread, when the region has them
constexpr int64_t kMaxGridYZ = 65535; // HIP's limit on gridDim.y and gridDim.z
constexpr int64_t kMaxCellBlocks = 1 << 16;

typedef float F2 __attribute__((ext_vector_type(2))); // next to field_op.hpp's F4 and D2
// the same vectors as memory operands at ELEMENT alignment
typedef F2 F2e __attribute__((aligned(4)));
typedef F4 F4e __attribute__((aligned(4)));
typedef D2 D2e __attribute__((aligned(8)));

// NC coarse cells and their 2 NC fine children per row
template <typename T, int NC> struct Xfer;
template <> struct Xfer<float, 2> {
  typedef F4 fine;
  typedef F4e fineMem;
  typedef F2 coarse;
  typedef F2e coarseMem;
};
template <> struct Xfer<float, 1> {
  typedef F2 fine;
  typedef F2e fineMem;
  typedef float coarse;
  typedef float coarseMem;
};
template <> struct Xfer<double, 1> {
  typedef D2 fine;
  typedef D2e fineMem;
  typedef double coarse;
  typedef double coarseMem;
};

// fine row sums -> coarse cells: the pair sums times 1/8
__device__ __forceinline__ float fold(F2 s) { return (s[0] + s[1]) * 0.125f; }
__device__ __forceinline__ double fold(D2 s) { return (s[0] + s[1]) * 0.125; }
__device__ __forceinline__ F2 fold(F4 s) {
  F2 r = {s[0] + s[1], s[2] + s[3]};
  return r * 0.125f;
}
// coarse cells -> fine row: every coarse cell twice
__device__ __forceinline__ F2 spread(float c) { return F2{c, c}; }
__device__ __forceinline__ D2 spread(double c) { return D2{c, c}; }
__device__ __forceinline__ F4 spread(F2 c) { return F4{c[0], c[0], c[1], c[1]}; }

struct Geom {
  int64_t fPitch, fPlane; // byte strides of the fine operands
  int64_t cPitch, cPlane; // and of the coarse one
  int32_t extX, extY, extZ; // the COARSE region
  int32_t zc;               // coarse planes per thread (strips)
};

// a, b: the first child of the coarse cell(s); out: the coarse cell(s)
template <typename T> struct RestrictF {
  const char *a, *b;
  char *out;
  T alpha, beta;
  template <int NC>
  __device__ __forceinline__ void at(const Geom &g, int64_t foff, int64_t coff) const {
    typedef Xfer<T, NC> X;
    typename X::fine s = {};
#pragma unroll
    for (int dz = 0; dz < 2; ++dz)
#pragma unroll
      for (int dy = 0; dy < 2; ++dy) {
        const int64_t o = foff + dz * g.fPlane + dy * g.fPitch;
        const typename X::fine va = *(const typename X::fineMem *)(a + o);
        const typename X::fine vb = *(const typename X::fineMem *)(b + o);
        s += alpha * va + beta * vb;
      }
    __builtin_nontemporal_store(fold(s), (typename X::coarseMem *)(out + coff));
  }
};

template <typename T> struct ProlongF {
  const char *src;
  char *dst;
  template <int NC>
  __device__ __forceinline__ void at(const Geom &g, int64_t foff, int64_t coff) const {
    typedef Xfer<T, NC> X;
    const typename X::coarse c = *(const typename X::coarseMem *)(src + coff);
    const typename X::fine add = spread(c);
#pragma unroll
    for (int dz = 0; dz < 2; ++dz)
#pragma unroll
      for (int dy = 0; dy < 2; ++dy) {
        typename X::fineMem *p = (typename X::fineMem *)(dst + foff + dz * g.fPlane + dy * g.fPitch);
        const typename X::fine v = *p;
        *p = v + add;
      }
  }
};

// f.at<NC>(g, foff, coff) handles NC coarse cells at byte offset coff from
// the coarse operand's first cell of the region and their children at foff
// from the fine operands' first cell.
template <typename T, typename F> __device__ __forceinline__ void walk_strips(const Geom &g, const F &f) {
  constexpr int NC = 8 / (int)sizeof(T); // coarse cells per strip
  constexpr int64_t ES = (int64_t)sizeof(T);
  const int32_t u = blockIdx.x * blockDim.x + threadIdx.x;
  const int32_t cy = blockIdx.y * blockDim.y + threadIdx.y;
  const int32_t cz0 = blockIdx.z * g.zc;
  const int64_t cx = (int64_t)u * NC;
  if (cy >= g.extY || cx >= g.extX) return;
  const int32_t zEnd = min(cz0 + g.zc, g.extZ);
  int64_t coff = (int64_t)cz0 * g.cPlane + (int64_t)cy * g.cPitch + cx * ES;
  int64_t foff = 2 * ((int64_t)cz0 * g.fPlane + (int64_t)cy * g.fPitch + cx * ES);
  if (cx + NC <= g.extX) {
#pragma unroll 2
    for (int32_t cz = cz0; cz < zEnd; ++cz, coff += g.cPlane, foff += 2 * g.fPlane)
      f.template at<NC>(g, foff, coff);
  } else { // fp32 only: the last coarse cell of an odd row
    for (int32_t cz = cz0; cz < zEnd; ++cz, coff += g.cPlane, foff += 2 * g.fPlane)
      f.template at<1>(g, foff, coff);
  }
}

template <typename T, typename I, typename F>
__device__ __forceinline__ void walk_cells_i(const Geom &g, const F &f) {
  const I total = (I)g.extX * (I)g.extY * (I)g.extZ;
  const I stride = (I)gridDim.x * (I)blockDim.x;
  for (I i = (I)blockIdx.x * (I)blockDim.x + (I)threadIdx.x; i < total; i += stride) {
    const I cx = i % (I)g.extX;
    const I t = i / (I)g.extX;
    const I cy = t % (I)g.extY;
    const I cz = t / (I)g.extY;
    const int64_t coff = (int64_t)cz * g.cPlane + (int64_t)cy * g.cPitch + (int64_t)cx * (int64_t)sizeof(T);
    const int64_t foff =
        2 * ((int64_t)cz * g.fPlane + (int64_t)cy * g.fPitch + (int64_t)cx * (int64_t)sizeof(T));
    f.template at<1>(g, foff, coff);
  }
}

template <typename T, bool STRIPS, typename F>
__device__ __forceinline__ void walk(const Geom &g, const F &f) {
  if constexpr (STRIPS) {
    walk_strips<T>(g, f);
  } else {
    if ((int64_t)g.extX * g.extY * g.extZ <= 0x7fffffffLL)
      walk_cells_i<T, uint32_t>(g, f);
    else
      walk_cells_i<T, int64_t>(g, f);
  }
}

template <typename T, bool STRIPS>
__global__ void __launch_bounds__(256)
    grid_restrict_kernel(Geom g, const char *a, const char *b, char *out, T alpha, T beta) {
  const RestrictF<T> f{a, b, out, alpha, beta};
  walk<T, STRIPS>(g, f);
}

template <typename T, bool STRIPS>
__global__ void __launch_bounds__(256)
    grid_prolong_add_kernel(Geom g, const char *src, char *dst) {
  const ProlongF<T> f{src, dst};
  walk<T, STRIPS>(g, f);
}

//// host ////

struct Launch {
  LocalDomain *fd = nullptr, *cd = nullptr;
  bool empty = false;
  bool strips = false;
  int64_t es = 0;
  Geom g{};
  dim3 grid, block;
  RegionCells f, c; // each operand's first cell of its region
};

// Validate and shape one op. Throws std::invalid_argument before anything
// is launched.
Launch plan(const char *op, ExchangeEngine &fine, int fdom, std::initializer_list<Operand> fops,
            ExchangeEngine &coarse, int cdom, std::initializer_list<Operand> cops,
            const Rect3 &region) {
  Launch l;
  l.fd = &checked_domain(op, fine, fdom, "fine domain");
  l.cd = &checked_domain(op, coarse, cdom, "coarse domain");
  l.es = checked_elem_size(op, *l.fd, fops);
  l.es = checked_elem_size(op, *l.cd, cops, 0, l.es);
  if (l.fd->gpu() != l.cd->gpu())
    throw std::invalid_argument(std::string(op) + ": the fine domain is on device " +
                                std::to_string(l.fd->gpu()) + ", the coarse one on device " +
                                std::to_string(l.cd->gpu()));
  if (!checked_extent(op, region, 0x3fffffff)) { // the fine extent is twice this one
    l.empty = true;
    return l;
  }
  const Vec3 ext = region.extent();
  const Rect3 cfull = l.cd->full_region(), ffull = l.fd->full_region();
  check_inside(op, "coarse region", region, cfull);
  const Rect3 fregion(Vec3(2 * region.lo.x, 2 * region.lo.y, 2 * region.lo.z),
                      Vec3(2 * region.hi.x, 2 * region.hi.y, 2 * region.hi.z));
  check_inside(op, "fine region", fregion, ffull);
  l.f = region_cells(op, *l.fd, fops, fregion.lo - ffull.lo, l.es);
  l.c = region_cells(op, *l.cd, cops, region.lo - cfull.lo, l.es);
  l.g.fPitch = l.f.pitch;
  l.g.fPlane = l.f.plane;
  l.g.cPitch = l.c.pitch;
  l.g.cPlane = l.c.plane;
  l.g.extX = (int32_t)ext.x;
  l.g.extY = (int32_t)ext.y;
  l.g.extZ = (int32_t)ext.z;

  const int64_t nc = 8 / l.es;
  const int64_t units = (ext.x + nc - 1) / nc;
  const int64_t gx = (units + kBx - 1) / kBx, gy = (ext.y + kBy - 1) / kBy;
  if (ext.x >= 4 && gy <= kMaxGridYZ) {
    const int64_t zc = std::max<int64_t>((ext.z + kMaxGridYZ - 1) / kMaxGridYZ,
                                         std::min<int64_t>(kMinZc, ext.z));
    l.strips = true;
    l.g.zc = (int32_t)zc;
    l.block = dim3(kBx, kBy, 1);
    l.grid = dim3((uint32_t)gx, (uint32_t)gy, (uint32_t)((ext.z + zc - 1) / zc));
    return l;
  }
  const int64_t total = ext.flatten();
  l.block = dim3(256, 1, 1);
  l.grid = dim3((uint32_t)std::min<int64_t>((total + 255) / 256, kMaxCellBlocks), 1, 1);
  return l;
}

#define GRID_TRANSFER_LAUNCH(T, l, KERNEL, stream, ...)                                           \
  do {                                                                                             \
    if ((l).strips)                                                                                \
      hipLaunchKernelGGL((KERNEL<T, true>), (l).grid, (l).block, 0, stream, __VA_ARGS__);          \
    else                                                                                           \
      hipLaunchKernelGGL((KERNEL<T, false>), (l).grid, (l).block, 0, stream, __VA_ARGS__);         \
    STENCIL_HIP(hipGetLastError());                                                                \
  } while (0)

} // namespace

void grid_restrict(ExchangeEngine &fine, int fdom, double alpha, int64_t a, bool aNext,
                   double beta, int64_t b, bool bNext, ExchangeEngine &coarse, int cdom,
                   int64_t out, bool outNext, const Rect3 &coarseRegion, int streamId) {
  const Launch l = plan("grid_restrict", fine, fdom, {{a, aNext}, {b, bNext}}, coarse, cdom,
                        {{out, outNext}}, coarseRegion);
  if (l.empty) return;
  STENCIL_HIP(hipSetDevice(l.cd->gpu()));
  hipStream_t stream = coarse.compute_stream(cdom, streamId);
  if (l.es == 4) {
    const float al = (float)alpha, be = (float)beta; // the one rounding to the quantity's type
    GRID_TRANSFER_LAUNCH(float, l, grid_restrict_kernel, stream, l.g, (const char *)l.f.ptr[0],
                         (const char *)l.f.ptr[1], l.c.ptr[0], al, be);
  } else {
    GRID_TRANSFER_LAUNCH(double, l, grid_restrict_kernel, stream, l.g, (const char *)l.f.ptr[0],
                         (const char *)l.f.ptr[1], l.c.ptr[0], alpha, beta);
  }
}

void grid_prolong_add(ExchangeEngine &coarse, int cdom, int64_t src, bool srcNext,
                      ExchangeEngine &fine, int fdom, int64_t dst, bool dstNext,
                      const Rect3 &coarseRegion, int streamId) {
  const Launch l = plan("grid_prolong_add", fine, fdom, {{dst, dstNext}}, coarse, cdom,
                        {{src, srcNext}}, coarseRegion);
  if (l.empty) return;
  STENCIL_HIP(hipSetDevice(l.fd->gpu()));
  hipStream_t stream = fine.compute_stream(fdom, streamId);
  if (l.es == 4)
    GRID_TRANSFER_LAUNCH(float, l, grid_prolong_add_kernel, stream, l.g, (const char *)l.c.ptr[0],
                         l.f.ptr[0]);
  else
    GRID_TRANSFER_LAUNCH(double, l, grid_prolong_add_kernel, stream, l.g,
                         (const char *)l.c.ptr[0], l.f.ptr[0]);
}

} // namespace stencil_amd
