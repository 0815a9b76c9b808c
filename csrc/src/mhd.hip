// 6th-order compressible resistive MHD solver kernels (fp64, radius 3,
// 8 coupled fields) -- the Astaroth-class workload (reference:
// astaroth/astaroth.cu, user_kernels.h). This is an independent
// implementation of the standard equations, not a port of Astaroth's
// DSL-generated code.
//
// Fields: lnrho (log density), uu (velocity, 3), aa (magnetic vector
// potential, 3), ss (specific entropy). Equations (mu0 = 1, isothermal
// base state with entropy coupling; nu/eta/chi constant):
//   D lnrho / Dt = -div(u)
//   D u / Dt     = -cs2 * grad(lnrho + ss/cp) + j x B / rho
//                  + nu * (lap(u) + (1/3) grad(div(u)))
//   d A / dt     = u x B + eta * lap(A)          (resistive gauge)
//   D ss / Dt    = chi * lap(ss)
// with B = curl(A), j = grad(div(A)) - lap(A), D/Dt = d/dt + u . grad.
//
// Time integration: Williamson (1980) low-storage RK3 in the two-buffer
// form the halo-exchange library provides (curr/next + swap per substep):
//   next = curr + beta_s * (alpha_s / beta_{s-1} * (curr - next) + dt * rhs(curr))
//
// 6th-order central derivative coefficients; cross derivatives compose the
// first-derivative stencils (36-point quadrant sum).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>

#include "stencil_amd/device_util.hpp"
#include "stencil_amd/domain.hpp"
#include "stencil_amd/engine.hpp"
#include "stencil_amd/hip_check.hpp"
#include "stencil_amd/ops.hpp"

namespace stencil_amd {

namespace {

struct MhdParams {
  // raw per-launch base pointers (kernarg > slot indirection; see jacobi)
  // quantities 0..7 = physics fields, 8 = div u, 9 = div A (auxiliary
  // exchanged fields of the separable-derivative scheme)
  const char *curr[10];
  char *next[10];
  int64_t pitch, plane; // byte strides (identical for all 8 fp64 fields)
  int64_t allocX, allocY, allocZ;
  int64_t loX, loY, loZ;
  int32_t extX, extY, extZ;
  double dsx, dsy, dsz; // grid spacing
  double dt;
  double cs2;    // sound speed squared
  double cp_inv; // 1/cp for the entropy pressure coupling
  double nu, eta, chi;
  double alpha_over_beta_prev; // alpha_s / beta_{s-1} (0 for substep 0)
  double beta;
  int32_t ychunk; // y-chunked dispatch order in BLOCKS (see ychunk_remap)
};

enum { LNRHO = 0, UUX = 1, UUY = 2, UUZ = 3, AAX = 4, AAY = 5, AAZ = 6, SS = 7, DIVU = 8, DIVA = 9 };

// first derivative: (c1 (f1 - f-1) + c2 (f2 - f-2) + c3 (f3 - f-3)) / ds
__constant__ double D1[3] = {3.0 / 4.0, -3.0 / 20.0, 1.0 / 60.0};
// second derivative: (l0 f0 + sum li (fi + f-i)) / ds^2
__constant__ double D2[4] = {-49.0 / 18.0, 3.0 / 2.0, -3.0 / 20.0, 1.0 / 90.0};

struct Vec3d {
  double x, y, z;
};
__device__ inline Vec3d operator+(Vec3d a, Vec3d b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ inline Vec3d operator-(Vec3d a, Vec3d b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ inline Vec3d operator*(double s, Vec3d a) { return {s * a.x, s * a.y, s * a.z}; }
__device__ inline double dot(Vec3d a, Vec3d b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ inline Vec3d cross(Vec3d a, Vec3d b) {
  return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}

// read field q at offset (i,j,k) from the cell
struct Stencil {
  const char *base[10]; // per-field curr pointer AT the cell
  char *out[10];        // per-field next pointer AT the cell
  int64_t pitch, plane;

  __device__ double f(int q, int i, int j, int k) const {
    return *(const double *)(base[q] + (int64_t)k * plane + (int64_t)j * pitch + (int64_t)i * 8);
  }
  __device__ double c(int q) const { return *(const double *)base[q]; }

  __device__ double dx(int q, double ids) const {
    return (D1[0] * (f(q, 1, 0, 0) - f(q, -1, 0, 0)) + D1[1] * (f(q, 2, 0, 0) - f(q, -2, 0, 0)) +
            D1[2] * (f(q, 3, 0, 0) - f(q, -3, 0, 0))) *
           ids;
  }
  __device__ double dy(int q, double ids) const {
    return (D1[0] * (f(q, 0, 1, 0) - f(q, 0, -1, 0)) + D1[1] * (f(q, 0, 2, 0) - f(q, 0, -2, 0)) +
            D1[2] * (f(q, 0, 3, 0) - f(q, 0, -3, 0))) *
           ids;
  }
  __device__ double dz(int q, double ids) const {
    return (D1[0] * (f(q, 0, 0, 1) - f(q, 0, 0, -1)) + D1[1] * (f(q, 0, 0, 2) - f(q, 0, 0, -2)) +
            D1[2] * (f(q, 0, 0, 3) - f(q, 0, 0, -3))) *
           ids;
  }
  __device__ double dxx(int q, double ids2) const {
    return (D2[0] * c(q) + D2[1] * (f(q, 1, 0, 0) + f(q, -1, 0, 0)) +
            D2[2] * (f(q, 2, 0, 0) + f(q, -2, 0, 0)) + D2[3] * (f(q, 3, 0, 0) + f(q, -3, 0, 0))) *
           ids2;
  }
  __device__ double dyy(int q, double ids2) const {
    return (D2[0] * c(q) + D2[1] * (f(q, 0, 1, 0) + f(q, 0, -1, 0)) +
            D2[2] * (f(q, 0, 2, 0) + f(q, 0, -2, 0)) + D2[3] * (f(q, 0, 3, 0) + f(q, 0, -3, 0))) *
           ids2;
  }
  __device__ double dzz(int q, double ids2) const {
    return (D2[0] * c(q) + D2[1] * (f(q, 0, 0, 1) + f(q, 0, 0, -1)) +
            D2[2] * (f(q, 0, 0, 2) + f(q, 0, 0, -2)) + D2[3] * (f(q, 0, 0, 3) + f(q, 0, 0, -3))) *
           ids2;
  }
  // cross derivatives: composed first-derivative stencils (quadrant sum)
  __device__ double dxy(int q, double idsx, double idsy) const {
    double s = 0;
#pragma unroll
    for (int i = 1; i <= 3; ++i)
#pragma unroll
      for (int j = 1; j <= 3; ++j)
        s += D1[i - 1] * D1[j - 1] *
             (f(q, i, j, 0) - f(q, i, -j, 0) - f(q, -i, j, 0) + f(q, -i, -j, 0));
    return s * idsx * idsy;
  }
  __device__ double dxz(int q, double idsx, double idsz) const {
    double s = 0;
#pragma unroll
    for (int i = 1; i <= 3; ++i)
#pragma unroll
      for (int k = 1; k <= 3; ++k)
        s += D1[i - 1] * D1[k - 1] *
             (f(q, i, 0, k) - f(q, i, 0, -k) - f(q, -i, 0, k) + f(q, -i, 0, -k));
    return s * idsx * idsz;
  }
  __device__ double dyz(int q, double idsy, double idsz) const {
    double s = 0;
#pragma unroll
    for (int j = 1; j <= 3; ++j)
#pragma unroll
      for (int k = 1; k <= 3; ++k)
        s += D1[j - 1] * D1[k - 1] *
             (f(q, 0, j, k) - f(q, 0, j, -k) - f(q, 0, -j, k) + f(q, 0, -j, -k));
    return s * idsy * idsz;
  }

  __device__ Vec3d grad(int q, double ix, double iy, double iz) const {
    return {dx(q, ix), dy(q, iy), dz(q, iz)};
  }
  __device__ double lap(int q, double ix, double iy, double iz) const {
    return dxx(q, ix * ix) + dyy(q, iy * iy) + dzz(q, iz * iz);
  }
};

// The solver is split into two kernels per substep: the monolithic form
// allocated 356 VGPR+AGPR (1 wave/SIMD) and latency-bound on its dependent
// cache loads. Split, each kernel fits >=2 waves/SIMD; the duplicated
// center reads are served by L1/L2.

// y-chunked dispatch (STENCIL_MHD_YCHUNK=<blocks>): iterate the block
// grid chunk-of-y-rows-major (for each y-chunk: all z, then y-in-chunk,
// then x) so a z-slab's working set per XCD shrinks by nby/C -- the
// momentum/scalar kernels refetch z-star planes ~3.4x because a 2-thick
// slab of 10 fp64 fields (~5 MB/XCD at 256^3) thrashes the 4 MB XCD L2.
// C must divide gridDim.y (host guarantees).
__device__ __forceinline__ void ychunk_remap(int32_t C, int32_t &bx, int32_t &by, int32_t &bz) {
  const int32_t flat = bx + gridDim.x * (by + gridDim.y * bz);
  const int32_t per = gridDim.x * C * gridDim.z;
  const int32_t chunk = flat / per, rem = flat % per;
  bz = rem / (gridDim.x * C);
  const int32_t rem2 = rem % (gridDim.x * C);
  by = chunk * C + rem2 / gridDim.x;
  bx = rem2 % gridDim.x;
}

// What every kernel starts from: decode this thread's cell from the block
// grid (in y-chunked order when p.ychunk is set) and point `st` at it in
// every field. False for threads outside the region.
__device__ __forceinline__ bool mhd_cell(const MhdParams &p, Stencil &st) {
  int32_t bx = blockIdx.x, by = blockIdx.y, bz = blockIdx.z;
  if (p.ychunk) ychunk_remap(p.ychunk, bx, by, bz);
  const int32_t lx = bx * blockDim.x + threadIdx.x;
  const int32_t ly = by * blockDim.y + threadIdx.y;
  const int32_t lz = bz * blockDim.z + threadIdx.z;
  if (lx >= p.extX || ly >= p.extY || lz >= p.extZ) return false;
  const int64_t ax = p.loX + lx - p.allocX;
  const int64_t ay = p.loY + ly - p.allocY;
  const int64_t az = p.loZ + lz - p.allocZ;
  const int64_t cellOff = az * p.plane + ay * p.pitch + ax * 8;
  st.pitch = p.pitch;
  st.plane = p.plane;
#pragma unroll
  for (int q = 0; q < 10; ++q) {
    st.base[q] = p.curr[q] + cellOff;
    st.out[q] = p.next[q] + cellOff;
  }
  return true;
}

__device__ __forceinline__ void write_rk3(const MhdParams &p, const Stencil &st, int q, double r) {
  char *out = st.out[q];
  const double cur = st.c(q);
  const double prev = *(const double *)out;
  *(double *)out = cur + p.beta * (p.alpha_over_beta_prev * (cur - prev) + p.dt * r);
}

// kernel 1: continuity + entropy + induction (lnrho, ss, aa). First and
// second derivatives only, no cross terms.
__global__ void __launch_bounds__(256) mhd_scalar_kernel(MhdParams p) {
  Stencil st;
  if (!mhd_cell(p, st)) return;
  const double ix = 1.0 / p.dsx, iy = 1.0 / p.dsy, iz = 1.0 / p.dsz;
  const Vec3d uu = {st.c(UUX), st.c(UUY), st.c(UUZ)};
  {
    const Vec3d glnrho = st.grad(LNRHO, ix, iy, iz);
    write_rk3(p, st, LNRHO, -dot(uu, glnrho) - st.c(DIVU));
  }
  {
    const Vec3d gss = st.grad(SS, ix, iy, iz);
    write_rk3(p, st, SS, -dot(uu, gss) + p.chi * st.lap(SS, ix, iy, iz));
  }
  const Vec3d B = {st.dy(AAZ, iy) - st.dz(AAY, iz), st.dz(AAX, iz) - st.dx(AAZ, ix),
                   st.dx(AAY, ix) - st.dy(AAX, iy)};
  const Vec3d uxB = cross(uu, B);
  write_rk3(p, st, AAX, uxB.x + p.eta * st.lap(AAX, ix, iy, iz));
  write_rk3(p, st, AAY, uxB.y + p.eta * st.lap(AAY, ix, iy, iz));
  write_rk3(p, st, AAZ, uxB.z + p.eta * st.lap(AAZ, ix, iy, iz));
}

// div pass: divu = div(u), divA = div(A), stored as exchanged auxiliary
// quantities. After their halos are exchanged, grad(div .) becomes three
// cheap 7-point first derivatives of ONE field instead of 36-point
// composed cross-derivative sums (separable formulation; identical order
// of accuracy, fp-rounding-level difference mirrored exactly in the NumPy
// reference).
__global__ void __launch_bounds__(256) mhd_div_kernel(MhdParams p) {
  Stencil st;
  if (!mhd_cell(p, st)) return;
  const double ix = 1.0 / p.dsx, iy = 1.0 / p.dsy, iz = 1.0 / p.dsz;
  // div fields live in the CURR buffers (consumed this substep, stale
  // after swap, recomputed next substep)
  *(double *)(const_cast<char *>(st.base[DIVU])) =
      st.dx(UUX, ix) + st.dy(UUY, iy) + st.dz(UUZ, iz);
  *(double *)(const_cast<char *>(st.base[DIVA])) =
      st.dx(AAX, ix) + st.dy(AAY, iy) + st.dz(AAZ, iz);
}

// momentum: j_i = D_i(divA) - lap(A_i); grad(div u) = grad of the divu field
__global__ void __launch_bounds__(256) mhd_momentum_kernel(MhdParams p) {
  Stencil st;
  if (!mhd_cell(p, st)) return;
  const double ix = 1.0 / p.dsx, iy = 1.0 / p.dsy, iz = 1.0 / p.dsz;
  const Vec3d uu = {st.c(UUX), st.c(UUY), st.c(UUZ)};
  const double rho_inv = exp(-st.c(LNRHO));

  const Vec3d j = {st.dx(DIVA, ix) - st.lap(AAX, ix, iy, iz),
                   st.dy(DIVA, iy) - st.lap(AAY, ix, iy, iz),
                   st.dz(DIVA, iz) - st.lap(AAZ, ix, iy, iz)};
  const Vec3d B = {st.dy(AAZ, iy) - st.dz(AAY, iz), st.dz(AAX, iz) - st.dx(AAZ, ix),
                   st.dx(AAY, ix) - st.dy(AAX, iy)};
  const Vec3d jxB = cross(j, B);

  {
    const double ugradu = uu.x * st.dx(UUX, ix) + uu.y * st.dy(UUX, iy) + uu.z * st.dz(UUX, iz);
    const double press = st.dx(LNRHO, ix) + p.cp_inv * st.dx(SS, ix);
    const double visc = p.nu * (st.lap(UUX, ix, iy, iz) + st.dx(DIVU, ix) / 3.0);
    write_rk3(p, st, UUX, -ugradu - p.cs2 * press + rho_inv * jxB.x + visc);
  }
  {
    const double ugradu = uu.x * st.dx(UUY, ix) + uu.y * st.dy(UUY, iy) + uu.z * st.dz(UUY, iz);
    const double press = st.dy(LNRHO, iy) + p.cp_inv * st.dy(SS, iy);
    const double visc = p.nu * (st.lap(UUY, ix, iy, iz) + st.dy(DIVU, iy) / 3.0);
    write_rk3(p, st, UUY, -ugradu - p.cs2 * press + rho_inv * jxB.y + visc);
  }
  {
    const double ugradu = uu.x * st.dx(UUZ, ix) + uu.y * st.dy(UUZ, iy) + uu.z * st.dz(UUZ, iz);
    const double press = st.dz(LNRHO, iz) + p.cp_inv * st.dz(SS, iz);
    const double visc = p.nu * (st.lap(UUZ, ix, iy, iz) + st.dz(DIVU, iz) / 3.0);
    write_rk3(p, st, UUZ, -ugradu - p.cs2 * press + rho_inv * jxB.z + visc);
  }
}

// STENCIL_MHD_YCHUNK=<blocks> (0 = off; default 32): largest divisor of
// the y-block count that is <= the request (C must divide gridDim.y for
// the in-kernel decode). Measured: +1.5% at 256^3, +21% at 640^3 (fixes
// the odd-size L2-thrash anomaly with the default block shape). Unlike the
// whole-grid per-XCD slab remap that measured 10% slower (removed;
// docs/DESIGN.md), this keeps the round-robin XCD spread WITHIN a chunk
// while bounding the z-slab working set that the chunk streams through
// the XCD L2s.
int32_t mhd_ychunk(int32_t nby) {
  static int ych = -1;
  if (ych < 0) {
    const char *e = getenv("STENCIL_MHD_YCHUNK");
    ych = e ? atoi(e) : 32;
  }
  if (ych <= 0) return 0;
  for (int32_t c = ych < nby ? ych : nby; c >= 1; --c)
    if (nby % c == 0) return c == nby ? 0 : c;
  return 0;
}

// STENCIL_MHD_BLOCK=<bx>x<by>x<bz>: any 256-thread shape (the kernels'
// launch bound); anything else falls back to the default
dim3 mhd_block() {
  // 64x2x2 measured best after the separable-derivative restructure
  // (block-shape sweep: 1649 vs 1608 Mcell/s at 32x4x2)
  static int bx = 0, by = 0, bz = 0;
  if (!bx) {
    bx = 64;
    by = 2;
    bz = 2;
    if (const char *e = getenv("STENCIL_MHD_BLOCK"))
      if (sscanf(e, "%dx%dx%d", &bx, &by, &bz) != 3 || bx * by * bz != 256) {
        bx = 64;
        by = 2;
        bz = 2;
      }
  }
  return dim3((uint32_t)bx, (uint32_t)by, (uint32_t)bz);
}

// One launch of the MHD kernels over `region`: kernargs built from the
// domain's CURRENT buffer parity, plus the launch shape. `step`/`dt` select
// the RK3 substep; the div pass reads neither.
struct MhdLaunch {
  MhdParams p;
  dim3 grid, block;
};

MhdLaunch mhd_launch(LocalDomain &d, const Rect3 &region, const MhdCoeffs &cf, int step = 0,
                     double dt = 0.0) {
  if (d.num_data() != 10 || d.elem_size(0) != 8)
    throw std::runtime_error("mhd: domain must have 10 fp64 quantities (8 fields + divu + divA)");
  MhdLaunch l{};
  MhdParams &p = l.p;
  for (int q = 0; q < 10; ++q) {
    p.curr[q] = d.curr(q).ptr;
    p.next[q] = d.next(q).ptr;
    if (d.curr(q).pitch != d.curr(0).pitch) throw std::runtime_error("mhd: field pitches differ");
  }
  p.pitch = d.curr(0).pitch;
  p.plane = d.curr(0).plane();
  const Rect3 full = d.full_region();
  p.allocX = full.lo.x;
  p.allocY = full.lo.y;
  p.allocZ = full.lo.z;
  p.loX = region.lo.x;
  p.loY = region.lo.y;
  p.loZ = region.lo.z;
  const Vec3 ext = region.extent();
  p.extX = (int32_t)ext.x;
  p.extY = (int32_t)ext.y;
  p.extZ = (int32_t)ext.z;
  p.dsx = cf.dsx;
  p.dsy = cf.dsy;
  p.dsz = cf.dsz;
  p.cs2 = cf.cs2;
  p.cp_inv = cf.cp_inv;
  p.nu = cf.nu;
  p.eta = cf.eta;
  p.chi = cf.chi;
  // Williamson (1980) coefficients
  static const double ALPHA[3] = {0.0, -5.0 / 9.0, -153.0 / 128.0};
  static const double BETA[3] = {1.0 / 3.0, 15.0 / 16.0, 8.0 / 15.0};
  p.dt = dt;
  p.alpha_over_beta_prev = (step == 0) ? 0.0 : ALPHA[step] / BETA[step - 1];
  p.beta = BETA[step];
  l.block = mhd_block();
  l.grid = dim3((uint32_t)((ext.x + l.block.x - 1) / l.block.x),
                (uint32_t)((ext.y + l.block.y - 1) / l.block.y),
                (uint32_t)((ext.z + l.block.z - 1) / l.block.z));
  p.ychunk = mhd_ychunk((int32_t)l.grid.y);
  return l;
}

void mhd_div_launch_on(LocalDomain &d, const Rect3 &region, const MhdCoeffs &cf,
                       hipStream_t stream) {
  if (region.extent().flatten() <= 0) return;
  const MhdLaunch l = mhd_launch(d, region, cf);
  hipLaunchKernelGGL(mhd_div_kernel, l.grid, l.block, 0, stream, l.p);
  STENCIL_HIP(hipGetLastError());
}

void mhd_substep_launch_on(LocalDomain &d, const Rect3 &region, int step, double dt,
                           const MhdCoeffs &cf, hipStream_t sScalar, hipStream_t sMomentum) {
  if (region.extent().flatten() <= 0) return;
  const MhdLaunch l = mhd_launch(d, region, cf, step, dt);
  // scalar (writes lnrho/ss/aa) and momentum (writes uu) touch disjoint
  // outputs and only read shared inputs: run them CONCURRENTLY on the two
  // streams (the caller joins them)
  hipLaunchKernelGGL(mhd_scalar_kernel, l.grid, l.block, 0, sScalar, l.p);
  STENCIL_HIP(hipGetLastError());
  hipLaunchKernelGGL(mhd_momentum_kernel, l.grid, l.block, 0, sMomentum, l.p);
  STENCIL_HIP(hipGetLastError());
}

} // namespace

void mhd_div_pass(ExchangeEngine &eng, int dom, const Rect3 &region, const MhdCoeffs &cf,
                  int streamId) {
  LocalDomain &d = eng.domain(dom);
  STENCIL_HIP(hipSetDevice(d.gpu()));
  mhd_div_launch_on(d, region, cf, eng.compute_stream(dom, streamId));
}

void mhd_substep(ExchangeEngine &eng, int dom, const Rect3 &region, int step, double dt,
                 const MhdCoeffs &cf, int streamId) {
  LocalDomain &d = eng.domain(dom);
  STENCIL_HIP(hipSetDevice(d.gpu()));
  mhd_substep_launch_on(d, region, step, dt, cf, eng.compute_stream(dom, streamId),
                        eng.compute_stream(dom, 1 - streamId));
}

// Whole-substep replay graphs for the single-process single-domain MHD
// path (the world=1 astaroth shape). Each RK3 substep s captures, per
// buffer parity: [X1 translates (field halos, group 0) -> div pass ->
// X2 translates (div halos, group 1) -> scalar || momentum (event-forked
// second stream) -> device-side table swap]. The host gap measured
// ~0.45 ms per substep at 256^3 (profiles/astaroth_256_kernel_stats.csv
// GPU-busy vs wall); replay costs one hipGraphLaunch.
std::unique_ptr<MhdStepGraph> mhd_graph_create(ExchangeEngine &eng, int dom, const Rect3 &region,
                                               double dt, const MhdCoeffs &cf) {
  return std::unique_ptr<MhdStepGraph>(new MhdStepGraph(eng, dom, region, dt, cf));
}

MhdStepGraph::MhdStepGraph(ExchangeEngine &eng, int dom, const Rect3 &region, double dt,
                           const MhdCoeffs &cf)
    : ReplayGraph(eng, dom, /*nSide=*/1, /*nEvents=*/2) {
  LocalDomain &d = domain();
  const hipStream_t stream2 = side_[0]; // momentum fork
  const hipEvent_t evFork = events_[0], evJoin = events_[1];
  for (int s = 0; s < 3; ++s) {
    for (int par = 0; par < 2; ++par) {
      exec_[s][par] = capture([&] {
        eng.launch_translates_plain_on((uintptr_t)stream_, 0); // X1: field halos
        mhd_div_launch_on(d, region, cf, stream_);
        eng.launch_translates_plain_on((uintptr_t)stream_, 1); // X2: div halos
        STENCIL_HIP(hipEventRecord(evFork, stream_));
        STENCIL_HIP(hipStreamWaitEvent(stream2, evFork, 0));
        mhd_substep_launch_on(d, region, s, dt, cf, stream_, stream2);
        STENCIL_HIP(hipEventRecord(evJoin, stream2));
        STENCIL_HIP(hipStreamWaitEvent(stream_, evJoin, 0));
        d.enqueue_table_swap(stream_);
      });
      d.swap(); // bake the other parity next
    }
  }
}

void MhdStepGraph::iter(int64_t nIters) {
  LocalDomain &d = domain();
  STENCIL_HIP(hipSetDevice(dev_));
  for (int64_t i = 0; i < nIters; ++i)
    for (int s = 0; s < 3; ++s) {
      STENCIL_HIP(hipGraphLaunch(exec_[s][parity_], stream_));
      parity_ ^= 1;
      d.swap_host_only();
    }
}

// Multi-rank substep graphs (one rank, one domain, cross-rank halos via
// IPC -- the 8-GPU single-node weak-scaling shape). Each RK3 substep
// splits at the TWO cross-rank barriers (field halos X1, div halos X2):
//   G1[par]    = [div(interior) || (translates g0 + staged packs g0)]
//   <barrier: every rank's field halos written>
//   G2[s][par] = [staged unpacks g0 -> div(exteriors) ->
//                 (translates g1 + staged packs g1) || substep(interior)]
//   <barrier: every rank's div halos written>
//   G3[s][par] = [staged unpacks g1 -> substep(exteriors) ->
//                 device table swap + view flips]
// The skew-safety argument is the jacobi one (JacobiMrStepGraph): each
// barrier bounds peers to one phase, staged buffers are double-buffered
// by parity, and direct writes land in halo rings disjoint from locally
// written compute cells.
std::unique_ptr<MhdMrStepGraph> mhd_mr_graph_create(ExchangeEngine &eng, int dom,
                                                    const Rect3 &interior,
                                                    const std::vector<Rect3> &exteriors,
                                                    double dt, const MhdCoeffs &cf) {
  return std::unique_ptr<MhdMrStepGraph>(
      new MhdMrStepGraph(eng, dom, interior, exteriors, dt, cf));
}

MhdMrStepGraph::MhdMrStepGraph(ExchangeEngine &eng, int dom, const Rect3 &interior,
                               const std::vector<Rect3> &exteriors, double dt,
                               const MhdCoeffs &cf)
    : ReplayGraph(eng, dom, /*nSide=*/2, /*nEvents=*/3) {
  LocalDomain &d = domain();
  const hipStream_t stream2 = side_[0], stream3 = side_[1];
  const hipEvent_t evF = events_[0], evJ2 = events_[1], evJ3 = events_[2];
  for (int par = 0; par < 2; ++par) {
    // G1: div(interior) concurrent with the outgoing field halos
    g1_[par] = capture([&] {
      STENCIL_HIP(hipEventRecord(evF, stream_));
      STENCIL_HIP(hipStreamWaitEvent(stream2, evF, 0));
      mhd_div_launch_on(d, interior, cf, stream_);
      eng.launch_translates_plain_on((uintptr_t)stream2, 0);
      eng.launch_packs_plain_on((uintptr_t)stream2, 1 + par);
      STENCIL_HIP(hipEventRecord(evJ2, stream2));
      STENCIL_HIP(hipStreamWaitEvent(stream_, evJ2, 0));
    });
    for (int s = 0; s < 3; ++s) {
      // G2: incoming field halos -> div(ext) -> div halos out || interior
      g2_[s][par] = capture([&] {
        eng.launch_unpacks_plain_on((uintptr_t)stream_, 1 + par);
        for (const Rect3 &box : exteriors) mhd_div_launch_on(d, box, cf, stream_);
        STENCIL_HIP(hipEventRecord(evF, stream_));
        STENCIL_HIP(hipStreamWaitEvent(stream2, evF, 0));
        STENCIL_HIP(hipStreamWaitEvent(stream3, evF, 0));
        eng.launch_translates_plain_on((uintptr_t)stream_, 1);
        eng.launch_packs_plain_on((uintptr_t)stream_, 4 + par); // 3*1+1+par
        mhd_substep_launch_on(d, interior, s, dt, cf, stream2, stream3);
        STENCIL_HIP(hipEventRecord(evJ2, stream2));
        STENCIL_HIP(hipEventRecord(evJ3, stream3));
        STENCIL_HIP(hipStreamWaitEvent(stream_, evJ2, 0));
        STENCIL_HIP(hipStreamWaitEvent(stream_, evJ3, 0));
      });
      // G3: incoming div halos -> exterior shells -> swap
      g3_[s][par] = capture([&] {
        eng.launch_unpacks_plain_on((uintptr_t)stream_, 4 + par);
        for (const Rect3 &box : exteriors)
          mhd_substep_launch_on(d, box, s, dt, cf, stream_, stream_);
        d.enqueue_table_swap(stream_);
        eng.enqueue_view_flips((uintptr_t)stream_);
      });
    }
    d.swap(); // bake the other parity's kernarg pointers next round
  }
}

void MhdMrStepGraph::phase1() { launch(g1_[parity_]); }

void MhdMrStepGraph::phase2() { launch(g2_[substep_][parity_]); }

void MhdMrStepGraph::phase3() {
  launch(g3_[substep_][parity_]);
  substep_ = (substep_ + 1) % 3;
  parity_ ^= 1;
  domain().swap_host_only(); // in-graph kernels flip the device state
  eng_.flip_views_host_only();
}

} // namespace stencil_amd
