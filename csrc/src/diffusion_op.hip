// Variable-coefficient diffusion operator for gfx950:
//   next[dstQ](p) = sigma u(p) + sum over a in {x,y,z}, s in {-1,+1} of
//                   h_a * 0.5 (k(p) + k(p + s e_a)) * (u(p) - u(p + s e_a))
//   diag(p)       = sigma + sum over a, s of h_a * 0.5 (k(p) + k(p + s e_a))
// with u = curr[srcQ], k = curr[kQ], h_a = 1 / spacing_a^2, for p in region.
//
// Contract (stencil_apply's): nothing outside `region` is written in any
// buffer, and only the cells of `region` and their six face neighbours, in
// u and in k, enter the arithmetic: no edge or corner cell does. Addresses:
// beyond those cells the strip kernel touches at most the rest of a 16 B
// line that holds one of them (same row, inside the allocation because the
// line holds a cell that is); of the two side strips of a step only the
// one cell next to the centre strip is used.
//
// Two kernels, chosen on the host (launch_diffusion):
//   diffusion_strip_kernel<T>: stencil_star_kernel<T, 1>'s scheme. One
//     thread = one 16 B x strip (float4 / double2) aligned by ADDRESS,
//     marching zc planes in z with the last three centre strips of u and of
//     k in registers; lanes past the body do one head / tail cell each. A
//     step issues its 10 sixteen-byte loads (new z plane, y -+ 1 rows and
//     x -+ 1 strips, of u and of k; the star kernel issues 5) before any
//     arithmetic, unconditionally, and stores nontemporally. Needs a region
//     at least 8 cells wide and curr[src], curr[k], next[dst] rows equally
//     aligned modulo 16 B.
//   diffusion_cells_kernel<T>: linearised grid-stride, one cell per lane
//     and step, 14 scalar loads: thin exterior slabs, narrow regions and
//     unequal alignment. diffusion_inv_diagonal has this walk only (it runs
//     once per coefficient change).
//
// Arithmetic per face: kf = (0.5 h_a) * (k + k'), acc += kf * (u - u'), in
// the quantity's type; 0.5 h_a and sigma are rounded to it once on the host.
//
// Shape: block 64x4 and 4 planes per thread (DIFFUSION_OP_BLOCK and
// DIFFUSION_OP_ZC override, read once). Ideal traffic is 3 passes (u, k,
// out). Measured on the MI355X at 512^3, effective TB/s of the 3 passes
// (the star kernel's 2 passes ran at 3.1-3.5 fp32 and 3.0-3.1 fp64 in the
// same processes):
//   planes/thread    4     8     12    16    24    32    64    128
//   fp32 (64x4)     3.25  3.19  3.04  2.97  2.89  2.77  2.59  2.72
//   fp64 (64x4)     2.98  2.93  2.94  2.89  2.84  2.76  2.56  2.33
//   at 32 planes: block 128x2 1.79 / 2.75, block 256x1 2.16 / 1.53
// Short chunks win although each re-reads 2 planes of u and 2 of k; the
// star kernel's default of 32 planes costs this kernel 15 %. BASELINE.md,
// "variable-coefficient diffusion", has the runs and a FETCH_SIZE counter
// run: in fp64 the kernel fetches 1.24 x the bytes of u and k from beyond
// L2, so about half of the re-read planes miss it. Compiler resource report
// (-Rpass-analysis=kernel-resource-usage, gfx950, ROCm clang):
//   diffusion_strip_kernel<float>:  62 VGPRs, 42 SGPRs, no scratch, no LDS,
//                                   occupancy 8 waves/SIMD
//   diffusion_strip_kernel<double>: 66 VGPRs, 42 SGPRs, no scratch, no LDS,
//                                   occupancy 7 waves/SIMD (64 would give 8)
//   diffusion_cells_kernel: 42 (float) / 52 (double) VGPRs, occupancy 8.
// The six window strips, the eight loaded strips and the accumulator are
// 60 registers of the fp32 kernel: the windows cost no occupancy there and
// one wave per SIMD in fp64, so they were kept and nothing is staged
// through LDS. 7-8 waves x 10 loads in flight per wave are more
// outstanding lines per CU than the star kernel's 5 per wave.
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

struct StripShape {
  int bx = 64, by = 4; // strip block: one wave per row, 4 rows
  int zc = 4;          // planes per thread (see the sweep in the file header)
};

// DIFFUSION_OP_BLOCK=BXxBY (BX*BY == 256, BX a multiple of 64) and
// DIFFUSION_OP_ZC=<z chunk>, read once: the star kernel's knobs
const StripShape &strip_shape() {
  static StripShape s = [] {
    StripShape r;
    if (const char *e = getenv("DIFFUSION_OP_BLOCK")) {
      int bx = 0, by = 0;
      if (sscanf(e, "%dx%d", &bx, &by) == 2 && bx > 0 && by > 0 && bx * by == 256 && bx % 64 == 0) {
        r.bx = bx;
        r.by = by;
      }
    }
    if (const char *e = getenv("DIFFUSION_OP_ZC")) {
      const int zc = atoi(e);
      if (zc >= 1 && zc <= 1024) r.zc = zc;
    }
    return r;
  }();
  return s;
}

template <typename T> struct DiffParams {
  const char *u; // the region's first cell in curr[src]
  const char *k; // ... in curr[k]
  char *dst;     // ... in next[dst] (inv_diagonal: the chosen buffer of out)
  int64_t pitch, plane; // byte strides, the same for the three
  int32_t extX, extY, extZ;
  int32_t zc;   // planes per thread (strips)
  int32_t head; // scalar cells before the first 16 B-aligned address (strips)
  T hx, hy, hz; // 0.5 / spacing_a^2
  T sigma;
  T omega; // inv_diagonal only
};

// one face: V is T or the strip vector
template <typename T, typename V>
__device__ __forceinline__ void face(V &acc, T hh, V kc, V kn, V uc, V un) {
  acc += (hh * (kc + kn)) * (uc - un);
}

template <typename T>
__global__ void __launch_bounds__(256) diffusion_strip_kernel(DiffParams<T> p) {
  constexpr int N = Strip<T>::N;
  constexpr int64_t ES = (int64_t)sizeof(T);
  typedef typename Strip<T>::vec vec;

  const int32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  const int32_t ly = blockIdx.y * blockDim.y + threadIdx.y;
  const int32_t lz0 = blockIdx.z * p.zc;
  if (ly >= p.extY) return;
  const int32_t zEnd = min(lz0 + p.zc, p.extZ);
  const int32_t body = (p.extX - p.head) / N;
  const int32_t tail = p.extX - p.head - body * N;
  const int64_t rowOff = (int64_t)lz0 * p.plane + (int64_t)ly * p.pitch;

  if (s < body) {
    const int64_t xOff = ((int64_t)p.head + (int64_t)s * N) * ES;
    const char *uc = p.u + rowOff + xOff;
    const char *kc = p.k + rowOff + xOff;
    char *dc = p.dst + rowOff + xOff;

    // slots: 0 = plane z - 1, 1 = z, 2 = z + 1 after a step's shift
    vec u0, u1 = *(const vec *)(uc - p.plane), u2 = *(const vec *)uc;
    vec k0, k1 = *(const vec *)(kc - p.plane), k2 = *(const vec *)kc;

    for (int32_t lz = lz0; lz < zEnd; ++lz) {
      // every load of the step, unconditional, before the arithmetic
      const vec un = *(const vec *)(uc + p.plane), kn = *(const vec *)(kc + p.plane);
      const vec uym = *(const vec *)(uc - p.pitch), kym = *(const vec *)(kc - p.pitch);
      const vec uyp = *(const vec *)(uc + p.pitch), kyp = *(const vec *)(kc + p.pitch);
      const vec ul = *(const vec *)(uc - 16), kl = *(const vec *)(kc - 16);
      const vec ur = *(const vec *)(uc + 16), kr = *(const vec *)(kc + 16);
      u0 = u1, u1 = u2, u2 = un;
      k0 = k1, k1 = k2, k2 = kn;

      vec acc = p.sigma * u1;
      face<T, vec>(acc, p.hz, k1, k0, u1, u0);
      face<T, vec>(acc, p.hz, k1, k2, u1, u2);
      face<T, vec>(acc, p.hy, k1, kym, u1, uym);
      face<T, vec>(acc, p.hy, k1, kyp, u1, uyp);
      // x: of the side strips only the cell next to the centre strip
      T ux[N + 2], kx[N + 2];
      ux[0] = ul[N - 1], kx[0] = kl[N - 1];
      ux[N + 1] = ur[0], kx[N + 1] = kr[0];
#pragma unroll
      for (int c = 0; c < N; ++c) ux[c + 1] = u1[c], kx[c + 1] = k1[c];
#pragma unroll
      for (int c = 0; c < N; ++c) {
        T a = acc[c];
        face<T, T>(a, p.hx, kx[c + 1], kx[c], ux[c + 1], ux[c]);
        face<T, T>(a, p.hx, kx[c + 1], kx[c + 2], ux[c + 1], ux[c + 2]);
        acc[c] = a;
      }

      // next is write-only this step: bypass cache pollution
      __builtin_nontemporal_store(acc, (vec *)dc);
      uc += p.plane;
      kc += p.plane;
      dc += p.plane;
    }
  } else if (s < body + p.head + tail) {
    // one lane per head / tail cell
    const int32_t j = s - body;
    const int32_t lx = j < p.head ? j : p.extX - tail + (j - p.head);
    const char *uc = p.u + rowOff + (int64_t)lx * ES;
    const char *kc = p.k + rowOff + (int64_t)lx * ES;
    char *dc = p.dst + rowOff + (int64_t)lx * ES;
    for (int32_t lz = lz0; lz < zEnd; ++lz) {
      const T u1 = *(const T *)uc, k1 = *(const T *)kc;
      const T uzm = *(const T *)(uc - p.plane), kzm = *(const T *)(kc - p.plane);
      const T uzp = *(const T *)(uc + p.plane), kzp = *(const T *)(kc + p.plane);
      const T uym = *(const T *)(uc - p.pitch), kym = *(const T *)(kc - p.pitch);
      const T uyp = *(const T *)(uc + p.pitch), kyp = *(const T *)(kc + p.pitch);
      const T uxm = *(const T *)(uc - ES), kxm = *(const T *)(kc - ES);
      const T uxp = *(const T *)(uc + ES), kxp = *(const T *)(kc + ES);
      T acc = p.sigma * u1;
      face<T, T>(acc, p.hz, k1, kzm, u1, uzm);
      face<T, T>(acc, p.hz, k1, kzp, u1, uzp);
      face<T, T>(acc, p.hy, k1, kym, u1, uym);
      face<T, T>(acc, p.hy, k1, kyp, u1, uyp);
      face<T, T>(acc, p.hx, k1, kxm, u1, uxm);
      face<T, T>(acc, p.hx, k1, kxp, u1, uxp);
      *(T *)dc = acc;
      uc += p.plane;
      kc += p.plane;
      dc += p.plane;
    }
  }
}

// I = uint32_t when the region has fewer than 2^31 cells. DIAG: write
// omega / diag instead of A u (u is not read then).
template <typename T, typename I, bool DIAG>
__device__ __forceinline__ void diffusion_cells(const DiffParams<T> &p) {
  constexpr int64_t ES = (int64_t)sizeof(T);
  const I total = (I)p.extX * (I)p.extY * (I)p.extZ;
  const I stride = (I)gridDim.x * (I)blockDim.x;
  for (I i = (I)blockIdx.x * (I)blockDim.x + (I)threadIdx.x; i < total; i += stride) {
    const I lx = i % (I)p.extX;
    const I t = i / (I)p.extX;
    const I ly = t % (I)p.extY;
    const I lz = t / (I)p.extY;
    const int64_t cell = (int64_t)lz * p.plane + (int64_t)ly * p.pitch + (int64_t)lx * ES;
    const char *kc = p.k + cell;
    const T k1 = *(const T *)kc;
    const T kzm = *(const T *)(kc - p.plane), kzp = *(const T *)(kc + p.plane);
    const T kym = *(const T *)(kc - p.pitch), kyp = *(const T *)(kc + p.pitch);
    const T kxm = *(const T *)(kc - ES), kxp = *(const T *)(kc + ES);
    if constexpr (DIAG) {
      T diag = p.sigma;
      diag += p.hz * (k1 + kzm);
      diag += p.hz * (k1 + kzp);
      diag += p.hy * (k1 + kym);
      diag += p.hy * (k1 + kyp);
      diag += p.hx * (k1 + kxm);
      diag += p.hx * (k1 + kxp);
      *(T *)(p.dst + cell) = p.omega / diag;
    } else {
      const char *uc = p.u + cell;
      const T u1 = *(const T *)uc;
      const T uzm = *(const T *)(uc - p.plane), uzp = *(const T *)(uc + p.plane);
      const T uym = *(const T *)(uc - p.pitch), uyp = *(const T *)(uc + p.pitch);
      const T uxm = *(const T *)(uc - ES), uxp = *(const T *)(uc + ES);
      T acc = p.sigma * u1;
      face<T, T>(acc, p.hz, k1, kzm, u1, uzm);
      face<T, T>(acc, p.hz, k1, kzp, u1, uzp);
      face<T, T>(acc, p.hy, k1, kym, u1, uym);
      face<T, T>(acc, p.hy, k1, kyp, u1, uyp);
      face<T, T>(acc, p.hx, k1, kxm, u1, uxm);
      face<T, T>(acc, p.hx, k1, kxp, u1, uxp);
      *(T *)(p.dst + cell) = acc;
    }
  }
}

template <typename T, bool DIAG>
__global__ void __launch_bounds__(256) diffusion_cells_kernel(DiffParams<T> p) {
  if ((int64_t)p.extX * p.extY * p.extZ <= 0x7fffffffLL)
    diffusion_cells<T, uint32_t, DIAG>(p);
  else
    diffusion_cells<T, int64_t, DIAG>(p);
}

template <typename T>
void launch_diffusion(DiffParams<T> p, const Vec3 &ext, bool diag, hipStream_t stream) {
  constexpr int N = Strip<T>::N;
  if (diag) {
    hipLaunchKernelGGL((diffusion_cells_kernel<T, true>), dim3(grid_for(ext.flatten(), 256)),
                       dim3(256), 0, stream, p);
    return;
  }
  const StripShape &shape = strip_shape();
  const int kBx = shape.bx, kBy = shape.by, kZc = shape.zc;
  const uintptr_t au = (uintptr_t)p.u & 15;
  const bool stripOk = au == ((uintptr_t)p.k & 15) && au == ((uintptr_t)p.dst & 15) &&
                       p.pitch % 16 == 0 && ((uintptr_t)p.u % sizeof(T)) == 0 &&
                       (ext.y + kBy - 1) / kBy <= 65535 && (ext.z + kZc - 1) / kZc <= 65535;
  if (ext.x >= 8 && stripOk) {
    p.head = (int32_t)std::min<int64_t>(head_cells(p.u, sizeof(T)), ext.x);
    p.zc = kZc;
    // strips + one lane per head / tail cell
    const int64_t units = ext.x - ((ext.x - p.head) / N) * (N - 1);
    dim3 block(kBx, kBy, 1);
    dim3 grid((uint32_t)((units + kBx - 1) / kBx), (uint32_t)((ext.y + kBy - 1) / kBy),
              (uint32_t)((ext.z + kZc - 1) / kZc));
    hipLaunchKernelGGL((diffusion_strip_kernel<T>), grid, block, 0, stream, p);
  } else {
    hipLaunchKernelGGL((diffusion_cells_kernel<T, false>), dim3(grid_for(ext.flatten(), 256)),
                       dim3(256), 0, stream, p);
  }
}

// Validate and launch either op. uQ < 0: the inverse diagonal (no u).
void run(const char *op, ExchangeEngine &eng, int dom, int64_t uQ, int64_t kQ, int64_t outQ,
         bool outNext, const Rect3 &region, const double h[3], double sigma, double omega,
         int64_t wantEs, int streamId) {
  const bool diag = uQ < 0;
  LocalDomain &d = checked_domain(op, eng, dom);
  const std::initializer_list<Operand> operands = {{diag ? kQ : uQ, false}, {kQ, false}, {outQ, outNext}};
  const int64_t es = checked_elem_size(op, d, operands);
  if (wantEs != 0 && es != wantEs)
    throw std::invalid_argument(std::string(op) + ": element size of the quantities does not match the type");
  if (streamId != 0 && streamId != 1)
    throw std::invalid_argument(std::string(op) + ": stream id must be 0 or 1");
  if (!checked_extent(op, region)) return; // empty region: no-op
  const Vec3 ext = region.extent();
  const Rect3 full = d.full_region();
  check_inside(op, "region", region, full, 1); // the kernels read the six face neighbours
  const RegionCells c = region_cells(op, d, operands, region.lo - full.lo, es);
  STENCIL_HIP(hipSetDevice(d.gpu()));
  hipStream_t stream = eng.compute_stream(dom, streamId);
  auto fill = [&](auto &p) {
    typedef decltype(p.sigma) T;
    p.u = c.ptr[0];
    p.k = c.ptr[1];
    p.dst = c.ptr[2];
    p.pitch = c.pitch;
    p.plane = c.plane;
    p.extX = (int32_t)ext.x;
    p.extY = (int32_t)ext.y;
    p.extZ = (int32_t)ext.z;
    // the one rounding to the quantity's type (the halving is exact)
    p.hx = (T)(0.5 * h[0]);
    p.hy = (T)(0.5 * h[1]);
    p.hz = (T)(0.5 * h[2]);
    p.sigma = (T)sigma;
    p.omega = (T)omega;
  };
  if (es == 4) {
    DiffParams<float> p{};
    fill(p);
    launch_diffusion<float>(p, ext, diag, stream);
  } else {
    DiffParams<double> p{};
    fill(p);
    launch_diffusion<double>(p, ext, diag, stream);
  }
  STENCIL_HIP(hipGetLastError());
}

} // namespace

void diffusion_apply(ExchangeEngine &eng, int dom, int64_t srcQ, int64_t kQ, int64_t dstQ,
                     const Rect3 &region, const double h[3], double sigma, StencilType type,
                     int streamId) {
  if (srcQ < 0) throw std::invalid_argument("diffusion_apply: no such quantity");
  run("diffusion_apply", eng, dom, srcQ, kQ, dstQ, true, region, h, sigma, 0.0,
      type == StencilType::F32 ? 4 : 8, streamId);
}

void diffusion_inv_diagonal(ExchangeEngine &eng, int dom, int64_t kQ, int64_t outQ, bool outNext,
                            const Rect3 &region, const double h[3], double sigma, double omega,
                            int streamId) {
  run("diffusion_inv_diagonal", eng, dom, -1, kQ, outQ, outNext, region, h, sigma, omega, 0,
      streamId);
}

} // namespace stencil_amd
