// Generic constant-coefficient linear stencil operator for gfx950:
//   next[dstQ](p) = sum_k w_k * curr[srcQ](p + o_k)   for p in region.
//
// Contract (stricter than jacobi_step's row extension): nothing outside
// `region` is written in any buffer, and only cells of `region (+) offsets`
// enter the arithmetic. Addresses: beyond those cells the kernels touch at
// most the rest of a 16 B line that holds one of them and the cells of
// `region` itself, all inside the allocation.
//
// Two kernels, chosen on the host (launch_stencil):
//   stencil_star_kernel<T, R>: every tap on an axis, max radius <= R <= 4,
//     region at least 8 cells wide. The design is jacobi_kernel_v4's: 16 B
//     x strips (float4 / double2) aligned by ADDRESS with scalar head and
//     tail lanes, a z march that keeps the centre-strip planes in
//     registers, nontemporal stores. The per-axis weights, tap masks and
//     the actual per-side radii are kernel arguments (wave-uniform, scalar
//     registers). A side beyond its actual radius is never addressed: the
//     load's offset is clamped to the nearest row/strip/plane the stencil
//     does read, and the tap mask selects 0 instead of the value, so an
//     asymmetric allocation (no downwind halo) is legal. The y rows come
//     through L1/L2; an LDS-staged variant was not built.
//     Strip loads fetch whole 16 B lines: the cells of a line that no tap
//     needs are loaded (same row, inside the allocation because the line
//     holds a cell that is) but never enter the arithmetic.
//   stencil_taps_kernel<T>: any tap set (<= 128). A table of precomputed
//     byte offsets dz*plane + dy*pitch + dx*sizeof(T) and weights travels
//     by value in the kernel arguments; cells are linearised grid-stride
//     like jacobi_kernel, so thin exterior slabs stay coalesced. Star
//     stencils on regions narrower than 8 cells take this path too.
//
// Knobs (read once): STENCIL_OP_BLOCK=BXxBY (BX*BY == 256, default 64x4)
// and STENCIL_OP_ZC=<z chunk> (default 32) shape the star launch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <string>

#include "stencil_amd/domain.hpp"
#include "stencil_amd/engine.hpp"
#include "stencil_amd/field_op.hpp"
#include "stencil_amd/hip_check.hpp"
#include "stencil_amd/ops.hpp"

namespace stencil_amd {

namespace {

constexpr int kMaxTaps = 128;
constexpr int kStarMaxR = 4;
constexpr int kDefaultZc = 32;

//// general path ////

template <typename T> struct Tap {
  int64_t off; // bytes from the cell itself
  T w;
};

template <typename T> struct TapsParams {
  const char *src;
  char *dst;
  int64_t pitch, plane; // byte strides (same for curr/next)
  int32_t extX, extY, extZ;
  int32_t ntaps;
  Tap<T> taps[kMaxTaps];
};
static_assert(sizeof(TapsParams<double>) < 4096, "tap table must fit the kernel arguments");

constexpr int kTapUnroll = 8; // the host pads the table to a multiple of this

// I = uint32_t when the region has fewer than 2^31 cells (the 64-bit
// divisions cost more than a 7-tap cell otherwise)
template <typename T, typename I> __device__ __forceinline__ void taps_cells(const TapsParams<T> &p) {
  const I total = (I)p.extX * (I)p.extY * (I)p.extZ;
  const I stride = (I)gridDim.x * (I)blockDim.x;
  for (I i = (I)blockIdx.x * (I)blockDim.x + (I)threadIdx.x; i < total; i += stride) {
    const I lx = i % (I)p.extX;
    const I t = i / (I)p.extX;
    const I ly = t % (I)p.extY;
    const I lz = t / (I)p.extY;
    // src/dst already point at the region's first cell
    const int64_t cell =
        (int64_t)lz * p.plane + (int64_t)ly * p.pitch + (int64_t)lx * (int64_t)sizeof(T);
    const char *c = p.src + cell;
    T acc = (T)0;
    // k is wave-uniform: the table is read with scalar loads. kTapUnroll
    // independent loads per wait; the padding entries repeat a real tap's
    // offset (a legal address) and are selected out, not multiplied by 0
    for (int32_t k = 0; k < p.ntaps; k += kTapUnroll) {
      T v[kTapUnroll];
#pragma unroll
      for (int u = 0; u < kTapUnroll; ++u) v[u] = *(const T *)(c + p.taps[k + u].off);
#pragma unroll
      for (int u = 0; u < kTapUnroll; ++u) acc += p.taps[k + u].w * (k + u < p.ntaps ? v[u] : (T)0);
    }
    *(T *)(p.dst + cell) = acc;
  }
}

template <typename T> __global__ void __launch_bounds__(256) stencil_taps_kernel(TapsParams<T> p) {
  if ((int64_t)p.extX * p.extY * p.extZ <= 0x7fffffffLL)
    taps_cells<T, uint32_t>(p);
  else
    taps_cells<T, int64_t>(p);
}

//// star path ////

template <typename T, int R> struct StarParams {
  const char *src; // the region's first cell
  char *dst;
  int64_t pitch, plane;
  int32_t extX, extY, extZ;
  int32_t zc;   // planes per thread
  int32_t head; // scalar cells before the first 16 B-aligned address
  // actual radii per side (<= R); nsl/nsr: side strips that exist
  int32_t rmx, rpx, rmy, rpy, rmz, rpz, nsl, nsr;
  // tap masks: bit j+R <-> offset j on x / y (centre bit never set);
  // mz in SLOT space (see the kernel), centre tap included
  uint32_t mx, my, mz, mzo;       // mzo: z taps and centre in offset space
  T wx[2 * R + 1], wy[2 * R + 1]; // index j+R
  T wzs[2 * R + 1];               // slot space
  T wzo[2 * R + 1];               // offset space (head / tail lanes)
};

// One thread = one 16 B x strip marching p.zc planes in z.
//   z: the last 2R+1 loaded centre strips live in registers, slot 2R the
//      newest (plane z + rpz), slot i plane z + rpz - (2R - i). The host
//      lays wzs/mz out in that slot order, so one new plane is loaded per
//      step whatever the per-side radii are.
//   x: the centre strip and NS aligned strips on either side form one
//      register row that the x taps index at compile-time offsets.
//   y: 2R row loads per step (L1/L2 hits: the neighbouring rows belong to
//      this block's other lanes or to the adjacent block).
// Lanes body .. body + head + tail - 1 do one head / tail cell each.
template <typename T, int R>
__global__ void __launch_bounds__(256) stencil_star_kernel(StarParams<T, R> p) {
  constexpr int N = Strip<T>::N;
  constexpr int NS = (R + N - 1) / N; // side strips that can hold an x tap
  constexpr int W = 2 * R + 1;
  constexpr int64_t ES = (int64_t)sizeof(T);
  typedef typename Strip<T>::vec vec;

  const int32_t u = blockIdx.x * blockDim.x + threadIdx.x;
  const int32_t ly = blockIdx.y * blockDim.y + threadIdx.y;
  const int32_t lz0 = blockIdx.z * p.zc;
  if (ly >= p.extY) return;
  const int32_t zEnd = min(lz0 + p.zc, p.extZ);
  const int32_t body = (p.extX - p.head) / N;
  const int32_t tail = p.extX - p.head - body * N;
  const int64_t rowOff = (int64_t)lz0 * p.plane + (int64_t)ly * p.pitch;

  if (u < body) {
    const int64_t xOff = ((int64_t)p.head + (int64_t)u * N) * ES;
    const char *col = p.src + rowOff + xOff;
    char *dcol = p.dst + rowOff + xOff;
    const int64_t newOff = (int64_t)p.rpz * p.plane;

    vec win[W];
    win[0] = (vec)(T)0; // shifted out before the first use
#pragma unroll
    for (int s = 1; s < W; ++s) {
      // plane offset this slot must hold before the first step's shift;
      // below -rmz the slot is masked: address the nearest plane read
      const int32_t jj = max(p.rpz - 1 - 2 * R + s, -p.rmz);
      win[s] = *(const vec *)(col + (int64_t)jj * p.plane);
    }

    // Every load of a step is unconditional and issued before the
    // arithmetic: a load under a (even wave-uniform) tap test makes hipcc
    // branch around it and wait for it alone, one memory round trip after
    // the other (measured 1.8x slower at R = 1). Taps that do not exist
    // are kept out of the sum by selecting 0 for the VALUE (their weight
    // is 0 too), never by 0 * value: the clamped address may hold a NaN.
    const vec zero = (vec)(T)0;
    for (int32_t lz = lz0; lz < zEnd; ++lz) {
      const vec newv = *(const vec *)(col + newOff);
      vec yv[2 * R], lv[NS], rv[NS];
#pragma unroll
      for (int i = 0; i < 2 * R; ++i) {
        const int j = i < R ? i - R : i - R + 1;
        const int32_t jc = min(max(j, -p.rmy), p.rpy);
        yv[i] = *(const vec *)(col + (int64_t)jc * p.pitch);
      }
#pragma unroll
      for (int s = 1; s <= NS; ++s) {
        lv[s - 1] = *(const vec *)(col - 16 * (int64_t)min(s, p.nsl));
        rv[s - 1] = *(const vec *)(col + 16 * (int64_t)min(s, p.nsr));
      }
#pragma unroll
      for (int s = 0; s < W - 1; ++s) win[s] = win[s + 1];
      win[W - 1] = newv;

      vec acc = zero;
#pragma unroll
      for (int s = 0; s < W; ++s) acc += p.wzs[s] * (((p.mz >> s) & 1u) ? win[s] : zero);
#pragma unroll
      for (int i = 0; i < 2 * R; ++i) {
        const int j = i < R ? i - R : i - R + 1;
        acc += p.wy[j + R] * (((p.my >> (j + R)) & 1u) ? yv[i] : zero);
      }

      // the centre strip sits rpz slots behind the newest
      vec cc = win[W - 1];
#pragma unroll
      for (int k = 1; k <= R; ++k)
        if (p.rpz == k) cc = win[W - 1 - k];
      T row[(2 * NS + 1) * N];
#pragma unroll
      for (int s = 1; s <= NS; ++s) {
#pragma unroll
        for (int c = 0; c < N; ++c) {
          row[(NS - s) * N + c] = lv[s - 1][c];
          row[(NS + s) * N + c] = rv[s - 1][c];
        }
      }
#pragma unroll
      for (int c = 0; c < N; ++c) row[NS * N + c] = cc[c];
#pragma unroll
      for (int j = -R; j <= R; ++j) {
        if (j == 0) continue;
        const bool on = (p.mx >> (j + R)) & 1u;
#pragma unroll
        for (int c = 0; c < N; ++c) acc[c] += p.wx[j + R] * (on ? row[NS * N + c + j] : (T)0);
      }

      // next is write-only this step: bypass cache pollution
      __builtin_nontemporal_store(acc, (vec *)dcol);
      col += p.plane;
      dcol += p.plane;
    }
  } else if (u < body + p.head + tail) {
    // one lane per head / tail cell; the same clamped unconditional loads
    const int32_t k = u - body;
    const int32_t lx = k < p.head ? k : p.extX - tail + (k - p.head);
    const char *c = p.src + rowOff + (int64_t)lx * ES;
    char *d = p.dst + rowOff + (int64_t)lx * ES;
    for (int32_t lz = lz0; lz < zEnd; ++lz) {
      T zv[W], yv[W], xv[W];
#pragma unroll
      for (int j = -R; j <= R; ++j) {
        zv[j + R] = *(const T *)(c + (int64_t)min(max(j, -p.rmz), p.rpz) * p.plane);
        yv[j + R] = *(const T *)(c + (int64_t)min(max(j, -p.rmy), p.rpy) * p.pitch);
        xv[j + R] = *(const T *)(c + (int64_t)min(max(j, -p.rmx), p.rpx) * ES);
      }
      T acc = (T)0;
#pragma unroll
      for (int j = -R; j <= R; ++j) {
        acc += p.wzo[j + R] * (((p.mzo >> (j + R)) & 1u) ? zv[j + R] : (T)0);
        acc += p.wy[j + R] * (((p.my >> (j + R)) & 1u) ? yv[j + R] : (T)0);
        acc += p.wx[j + R] * (((p.mx >> (j + R)) & 1u) ? xv[j + R] : (T)0);
      }
      *(T *)d = acc;
      c += p.plane;
      d += p.plane;
    }
  }
}

struct StarShape {
  int bx = 64, by = 4, zc = kDefaultZc;
};

const StarShape &star_shape() {
  static StarShape s = [] {
    StarShape r;
    if (const char *e = getenv("STENCIL_OP_BLOCK")) {
      int bx = 0, by = 0;
      if (sscanf(e, "%dx%d", &bx, &by) == 2 && bx > 0 && by > 0 && bx * by == 256 && bx % 64 == 0) {
        r.bx = bx;
        r.by = by;
      }
    }
    if (const char *e = getenv("STENCIL_OP_ZC")) {
      const int zc = atoi(e);
      if (zc >= 1 && zc <= 1024) r.zc = zc;
    }
    return r;
  }();
  return s;
}

template <typename T>
void launch_taps(const char *src, char *dst, int64_t pitch, int64_t plane, const Vec3 &ext,
                 const StencilTaps &taps, hipStream_t stream) {
  TapsParams<T> p{};
  p.src = src;
  p.dst = dst;
  p.pitch = pitch;
  p.plane = plane;
  p.extX = (int32_t)ext.x;
  p.extY = (int32_t)ext.y;
  p.extZ = (int32_t)ext.z;
  p.ntaps = (int32_t)taps.offsets.size();
  for (int k = 0; k < p.ntaps; ++k) {
    const Vec3 &o = taps.offsets[k];
    p.taps[k].off = o.z * plane + o.y * pitch + o.x * (int64_t)sizeof(T);
    p.taps[k].w = (T)taps.weights[k]; // the one rounding to the quantity's type
  }
  // padding up to the unroll width: a real tap's offset, weight 0
  for (int k = p.ntaps; k % kTapUnroll != 0; ++k) p.taps[k] = {p.taps[p.ntaps - 1].off, (T)0};
  hipLaunchKernelGGL(stencil_taps_kernel<T>, dim3(grid_for(ext.flatten(), 256)), dim3(256), 0,
                     stream, p);
}

template <typename T, int R>
void launch_star(const char *src, char *dst, int64_t pitch, int64_t plane, const Vec3 &ext,
                 const StencilTaps &taps, hipStream_t stream) {
  constexpr int N = Strip<T>::N;
  StarParams<T, R> p{};
  p.src = src;
  p.dst = dst;
  p.pitch = pitch;
  p.plane = plane;
  p.extX = (int32_t)ext.x;
  p.extY = (int32_t)ext.y;
  p.extZ = (int32_t)ext.z;
  const StarShape &shape = star_shape();
  p.zc = shape.zc;
  p.head = (int32_t)std::min<int64_t>(head_cells(src, sizeof(T)), ext.x);

  // per-axis tables in offset space, then z re-laid into slot space
  double wz[2 * R + 1] = {};
  uint32_t mzOff = 0;
  for (size_t k = 0; k < taps.offsets.size(); ++k) {
    const Vec3 &o = taps.offsets[k];
    const T w = (T)taps.weights[k]; // the one rounding to the quantity's type
    if (o.x != 0) {
      p.wx[o.x + R] = w;
      p.mx |= 1u << (o.x + R);
      p.rmx = std::max<int32_t>(p.rmx, (int32_t)-o.x);
      p.rpx = std::max<int32_t>(p.rpx, (int32_t)o.x);
    } else if (o.y != 0) {
      p.wy[o.y + R] = w;
      p.my |= 1u << (o.y + R);
      p.rmy = std::max<int32_t>(p.rmy, (int32_t)-o.y);
      p.rpy = std::max<int32_t>(p.rpy, (int32_t)o.y);
    } else { // z taps and the centre
      wz[o.z + R] = (double)w;
      mzOff |= 1u << (o.z + R);
      p.rmz = std::max<int32_t>(p.rmz, (int32_t)-o.z);
      p.rpz = std::max<int32_t>(p.rpz, (int32_t)o.z);
    }
  }
  p.nsl = (p.rmx + N - 1) / N;
  p.nsr = (p.rpx + N - 1) / N;
  p.mzo = mzOff;
  for (int s = 0; s < 2 * R + 1; ++s) p.wzo[s] = (T)wz[s];
  for (int s = 0; s < 2 * R + 1; ++s) {
    const int j = p.rpz - (2 * R - s); // offset held by slot s
    if (j >= -p.rmz && ((mzOff >> (j + R)) & 1u)) {
      p.wzs[s] = (T)wz[j + R];
      p.mz |= 1u << s;
    }
  }
  // strips + one lane per head/tail cell: x - head - body*N + head + body
  const int64_t units = ext.x - ((ext.x - p.head) / N) * (N - 1);
  dim3 block((uint32_t)shape.bx, (uint32_t)shape.by, 1);
  dim3 grid((uint32_t)((units + shape.bx - 1) / shape.bx),
            (uint32_t)((ext.y + shape.by - 1) / shape.by),
            (uint32_t)((ext.z + shape.zc - 1) / shape.zc));
  hipLaunchKernelGGL((stencil_star_kernel<T, R>), grid, block, 0, stream, p);
}

template <typename T>
void launch_star_r(int r, const char *src, char *dst, int64_t pitch, int64_t plane,
                   const Vec3 &ext, const StencilTaps &taps, hipStream_t stream) {
  switch (r) {
  case 0: // centre tap only
  case 1: launch_star<T, 1>(src, dst, pitch, plane, ext, taps, stream); break;
  case 2: launch_star<T, 2>(src, dst, pitch, plane, ext, taps, stream); break;
  case 3: launch_star<T, 3>(src, dst, pitch, plane, ext, taps, stream); break;
  default: launch_star<T, 4>(src, dst, pitch, plane, ext, taps, stream); break;
  }
}

template <typename T>
void launch_stencil(const char *src, char *dst, int64_t pitch, int64_t plane, const Vec3 &ext,
                    const StencilTaps &taps, hipStream_t stream) {
  bool star = true;
  int64_t maxR = 0;
  for (const Vec3 &o : taps.offsets) {
    star = star && ((o.x != 0) + (o.y != 0) + (o.z != 0) <= 1);
    maxR = std::max({maxR, std::abs(o.x), std::abs(o.y), std::abs(o.z)});
  }
  const StarShape &shape = star_shape();
  // the strip kernel needs curr and next equally aligned rows, and its
  // grid's y/z block counts within the launch limit
  const bool stripOk = ((uintptr_t)src & 15) == ((uintptr_t)dst & 15) && pitch % 16 == 0 &&
                       ((uintptr_t)src % sizeof(T)) == 0 &&
                       (ext.y + shape.by - 1) / shape.by <= 65535 &&
                       (ext.z + shape.zc - 1) / shape.zc <= 65535 && ext.x <= 0x7fffffff;
  if (star && maxR <= kStarMaxR && ext.x >= 8 && stripOk)
    launch_star_r<T>((int)maxR, src, dst, pitch, plane, ext, taps, stream);
  else
    launch_taps<T>(src, dst, pitch, plane, ext, taps, stream);
}

} // namespace

void stencil_apply(ExchangeEngine &eng, int dom, int64_t srcQ, int64_t dstQ, const Rect3 &region,
                   const StencilTaps &taps, StencilType type, int streamId) {
  const char *op = "stencil_apply";
  LocalDomain &d = checked_domain(op, eng, dom);
  const int64_t es = type == StencilType::F32 ? 4 : 8; // the stencil type's
  checked_elem_size(op, d, {{srcQ, false}, {dstQ, true}}, es);
  const size_t ntaps = taps.offsets.size();
  if (ntaps != taps.weights.size())
    throw std::invalid_argument("stencil_apply: offsets and weights differ in length");
  if (ntaps == 0 || ntaps > (size_t)kMaxTaps)
    throw std::invalid_argument("stencil_apply: want 1.." + std::to_string(kMaxTaps) +
                                " taps, got " + std::to_string(ntaps));
  if (!checked_extent(op, region)) return; // empty region: no-op
  const Vec3 ext = region.extent();
  const Rect3 full = d.full_region();
  for (const Vec3 &o : taps.offsets)
    if (!rect_inside(Rect3(region.lo + o, region.hi + o), full))
      throw std::invalid_argument("stencil_apply: tap " + o.str() + " over region " +
                                  region.str() + " reads outside the allocation " + full.str());
  // a tap-free cell of the region itself must be allocated too (it is written)
  check_inside(op, "region", region, full);
  const RegionCells c = region_cells(op, d, {{srcQ, false}, {dstQ, true}}, region.lo - full.lo, es);
  STENCIL_HIP(hipSetDevice(d.gpu()));
  hipStream_t stream = eng.compute_stream(dom, streamId);
  if (type == StencilType::F32)
    launch_stencil<float>(c.ptr[0], c.ptr[1], c.pitch, c.plane, ext, taps, stream);
  else
    launch_stencil<double>(c.ptr[0], c.ptr[1], c.pitch, c.plane, ext, taps, stream);
  STENCIL_HIP(hipGetLastError());
}

} // namespace stencil_amd
