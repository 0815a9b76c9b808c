// Vector operations on pitched quantities for gfx950: the inner product,
// out = alpha x + beta y, out = alpha x + beta y + gamma z, the diagonally
// scaled out = alpha x + d (beta y + gamma z), and the fused
// conjugate-gradient update. Pure
// streaming kernels: every cell of the region is read (and written) once.
// For singular problems (the constant null space, solvers/cg.py) also the
// sum of a field, the inner product together with both sums, the fused
// update together with sum r_new, and out = alpha x + beta y + c: the
// projection v - mean(v) rides on passes the iteration makes anyway.
// For non-symmetric problems (solvers/bicgstab.py) the three fused passes of
// a BiCGStab iteration: out = alpha x + beta y with sum out^2, the pair
// (a . b, a . a), and the update of x and r with (r . r, rhat . r).
//
// Contract (the stencil operator's): nothing outside `region` is written
// in any buffer, and no cell outside it enters the arithmetic. Unlike the
// star kernel these kernels never load a cell outside the region either:
// the 16 B strips cover aligned cells of the region only, the cells before
// the first and after the last aligned strip of a row get a lane each.
//
// Structure. An op is a functor: its operands' first cells of the region,
// its scalars in the quantity's type, and at<V>(off) for the cell(s) at
// byte offset `off`. Two kernel templates take it by value: field_kernel
// for the element-wise ops (axpbypcz_kernel stands in for one, see there),
// reduce_kernel for the functors that also
// declare NV and acc[NV], the values they sum. Two host helpers,
// run_field and begin_reduce, do the rest (plan, empty region, device and
// stream, the float / double dispatch with the one rounding of each scalar,
// launch, landing the partials), so a public op is its operand list and
// its functor.
//
// Two walks over the region, chosen on the host (plan_launch):
//   strips: the star kernel's row scheme. One thread = one 16 B x strip
//     (float4 / double2, aligned by ADDRESS) marching zc planes in z; lanes
//     body .. body + head + tail - 1 of a row do one head / tail cell each.
//     No division per cell. Needs a region at least 8 cells wide and every
//     operand's rows equally aligned.
//   cells: linearised grid-stride, one cell per lane and step, for the
//     thin slabs and the unequally aligned.
//
// Reductions are deterministic: fp64 accumulation per thread, cross-lane
// shuffles per wave, LDS per block, one partial per block and value written
// with an ordinary store, the partials summed in index order on the host.
// No atomics. The grid never exceeds ExchangeEngine::kReducePartials
// blocks; the engine's per-domain scratch holds kReduceValues times as many
// doubles, value-major (partials[v * blocks + b]), for the reductions that
// return up to three values from one pass.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <initializer_list>
#include <stdexcept>
#include <string>
#include <type_traits>

#include "stencil_amd/domain.hpp"
#include "stencil_amd/engine.hpp"
#include "stencil_amd/field_op.hpp"
#include "stencil_amd/hip_check.hpp"
#include "stencil_amd/ops.hpp"

namespace stencil_amd {

namespace {

constexpr int kBx = 64, kBy = 4; // strip block: one wave per row, 4 rows
constexpr int kMinZc = 4;        // planes per thread, when the region has them

struct Geom {
  int64_t pitch, plane; // byte strides, the same for every operand
  int32_t extX, extY, extZ;
  int32_t zc;   // planes per thread (strips)
  int32_t head; // scalar cells before the first 16 B-aligned address (strips)
};

// f.at<V>(off) handles the cell(s) at byte offset `off` from each operand's
// first cell of the region: V = the strip vector or T.
template <typename T, typename F> __device__ __forceinline__ void walk_strips(const Geom &g, F &f) {
  constexpr int N = Strip<T>::N;
  constexpr int64_t ES = (int64_t)sizeof(T);
  typedef typename Strip<T>::vec vec;
  const int32_t u = blockIdx.x * blockDim.x + threadIdx.x;
  const int32_t ly = blockIdx.y * blockDim.y + threadIdx.y;
  const int32_t lz0 = blockIdx.z * g.zc;
  if (ly >= g.extY) return; // back to the kernel: the thread still joins its block reduction
  const int32_t zEnd = min(lz0 + g.zc, g.extZ);
  const int32_t body = (g.extX - g.head) / N;
  const int32_t tail = g.extX - g.head - body * N;
  int64_t off = (int64_t)lz0 * g.plane + (int64_t)ly * g.pitch;
  if (u < body) {
    off += ((int64_t)g.head + (int64_t)u * N) * ES;
#pragma unroll 4
    for (int32_t lz = lz0; lz < zEnd; ++lz, off += g.plane) f.template at<vec>(off);
  } else if (u < body + g.head + tail) {
    const int32_t k = u - body;
    const int32_t lx = k < g.head ? k : g.extX - tail + (k - g.head);
    off += (int64_t)lx * ES;
    for (int32_t lz = lz0; lz < zEnd; ++lz, off += g.plane) f.template at<T>(off);
  }
}

template <typename T, typename I, typename F>
__device__ __forceinline__ void walk_cells_i(const Geom &g, F &f) {
  const I total = (I)g.extX * (I)g.extY * (I)g.extZ;
  const I stride = (I)gridDim.x * (I)blockDim.x;
  for (I i = (I)blockIdx.x * (I)blockDim.x + (I)threadIdx.x; i < total; i += stride) {
    const I lx = i % (I)g.extX;
    const I t = i / (I)g.extX;
    const I ly = t % (I)g.extY;
    const I lz = t / (I)g.extY;
    f.template at<T>((int64_t)lz * g.plane + (int64_t)ly * g.pitch +
                     (int64_t)lx * (int64_t)sizeof(T));
  }
}

template <typename T, bool STRIPS, typename F>
__device__ __forceinline__ void walk(const Geom &g, F &f) {
  if constexpr (STRIPS) {
    walk_strips<T>(g, f);
  } else {
    if ((int64_t)g.extX * g.extY * g.extZ <= 0x7fffffffLL)
      walk_cells_i<T, uint32_t>(g, f);
    else
      walk_cells_i<T, int64_t>(g, f);
  }
}

// acc += a * b in fp64, component after component
__device__ __forceinline__ void add_prod(double &acc, float a, float b) {
  acc += (double)a * (double)b;
}
__device__ __forceinline__ void add_prod(double &acc, double a, double b) { acc += a * b; }
__device__ __forceinline__ void add_prod(double &acc, F4 a, F4 b) {
#pragma unroll
  for (int c = 0; c < 4; ++c) add_prod(acc, a[c], b[c]);
}
__device__ __forceinline__ void add_prod(double &acc, D2 a, D2 b) {
#pragma unroll
  for (int c = 0; c < 2; ++c) add_prod(acc, a[c], b[c]);
}

// acc += a in fp64, component after component
__device__ __forceinline__ void add_val(double &acc, float a) { acc += (double)a; }
__device__ __forceinline__ void add_val(double &acc, double a) { acc += a; }
__device__ __forceinline__ void add_val(double &acc, F4 a) {
#pragma unroll
  for (int c = 0; c < 4; ++c) add_val(acc, a[c]);
}
__device__ __forceinline__ void add_val(double &acc, D2 a) {
#pragma unroll
  for (int c = 0; c < 2; ++c) add_val(acc, a[c]);
}

// Every thread of the 256-thread block calls this once (threads without a
// cell bring 0): per value, wave sums by shuffles, the 4 wave sums through
// LDS, one ordinary store per block: value v of block b lands in
// partials[v * blocks + b]. A fixed order: the same bits every time.
template <int NV>
__device__ __forceinline__ void block_store_sums(const double (&in)[NV], double *partials) {
  __shared__ double sWaves[NV][4];
  const int tid = threadIdx.y * blockDim.x + threadIdx.x;
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    double v = in[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if ((tid & 63) == 0) sWaves[k][tid >> 6] = v;
  }
  __syncthreads();
  if (tid == 0) {
    const int64_t blocks = (int64_t)gridDim.z * gridDim.y * gridDim.x;
    const int64_t b = ((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
#pragma unroll
    for (int k = 0; k < NV; ++k)
      partials[k * blocks + b] = ((sWaves[k][0] + sWaves[k][1]) + sWaves[k][2]) + sWaves[k][3];
  }
}

//// the ops ////

// a . b; SUMS: and sum a, sum b
template <bool SUMS> struct DotF {
  static constexpr int NV = SUMS ? 3 : 1;
  const char *a, *b;
  double acc[NV];
  template <typename V> __device__ __forceinline__ void at(int64_t off) {
    const V va = *(const V *)(a + off), vb = *(const V *)(b + off);
    add_prod(acc[0], va, vb);
    if constexpr (SUMS) {
      add_val(acc[1], va);
      add_val(acc[2], vb);
    }
  }
};

struct SumF {
  static constexpr int NV = 1;
  const char *a;
  double acc[NV];
  template <typename V> __device__ __forceinline__ void at(int64_t off) {
    add_val(acc[0], *(const V *)(a + off));
  }
};

// x += alpha p; r -= alpha ap; r_new . r_new; SUM: and sum r_new
template <typename T, bool SUM> struct CgF {
  static constexpr int NV = SUM ? 2 : 1;
  char *x;
  const char *p, *ap;
  char *r;
  T alpha;
  double acc[NV];
  template <typename V> __device__ __forceinline__ void at(int64_t off) {
    const V vp = *(const V *)(p + off), vap = *(const V *)(ap + off);
    const V vx = *(const V *)(x + off), vr = *(const V *)(r + off);
    const V rn = vr - alpha * vap;
    *(V *)(x + off) = vx + alpha * vp;
    *(V *)(r + off) = rn;
    add_prod(acc[0], rn, rn);
    if constexpr (SUM) add_val(acc[1], rn);
  }
};

template <typename T> struct AxpbyF {
  const char *x, *y;
  char *out;
  T alpha, beta;
  template <typename V> __device__ __forceinline__ void at(int64_t off) {
    const V vx = *(const V *)(x + off), vy = *(const V *)(y + off);
    *(V *)(out + off) = alpha * vx + beta * vy;
  }
};

template <typename T> struct AxpbycF {
  const char *x, *y;
  char *out;
  T alpha, beta, c;
  template <typename V> __device__ __forceinline__ void at(int64_t off) {
    const V vx = *(const V *)(x + off), vy = *(const V *)(y + off);
    *(V *)(out + off) = alpha * vx + beta * vy + c;
  }
};

template <typename T> struct AxpbypczF {
  const char *x, *y, *z;
  char *out;
  T alpha, beta, gamma;
  template <typename V> __device__ __forceinline__ void at(int64_t off) {
    const V vx = *(const V *)(x + off), vy = *(const V *)(y + off), vz = *(const V *)(z + off);
    *(V *)(out + off) = alpha * vx + beta * vy + gamma * vz;
  }
};

template <typename T> struct ScaledF {
  const char *x, *d, *y, *z;
  char *out;
  T alpha, beta, gamma;
  template <typename V> __device__ __forceinline__ void at(int64_t off) {
    const V vx = *(const V *)(x + off), vd = *(const V *)(d + off);
    const V vy = *(const V *)(y + off), vz = *(const V *)(z + off);
    *(V *)(out + off) = alpha * vx + vd * (beta * vy + gamma * vz);
  }
};

// The fused passes of BiCGStab (solvers/bicgstab.py).
//
// alpha x + beta y with the bits field_axpby writes. AxpbyF leaves the
// contraction to the compiler, which in field_kernel settles on
// fma(alpha, x, beta y) for the strips and for double, and on two rounded
// products and a sum for a float cell (it pairs the products into one
// packed multiply); tests/golden/vector_ops_bits.json pins that. In a
// reduction kernel the same expression contracts otherwise (the float cell
// gets an fma), so the forms are spelled out here.
__device__ __forceinline__ float axpby_bits(float alpha, float x, float beta, float y) {
  return __fadd_rn(__fmul_rn(alpha, x), __fmul_rn(beta, y));
}
__device__ __forceinline__ double axpby_bits(double alpha, double x, double beta, double y) {
  return __builtin_fma(alpha, x, __dmul_rn(beta, y));
}
__device__ __forceinline__ F4 axpby_bits(float alpha, F4 x, float beta, F4 y) {
  F4 o;
#pragma unroll
  for (int c = 0; c < 4; ++c) o[c] = __builtin_fmaf(alpha, x[c], __fmul_rn(beta, y[c]));
  return o;
}
__device__ __forceinline__ D2 axpby_bits(double alpha, D2 x, double beta, D2 y) {
  D2 o;
#pragma unroll
  for (int c = 0; c < 2; ++c) o[c] = axpby_bits(alpha, x[c], beta, y[c]);
  return o;
}

// out = alpha x + beta y; sum out^2, of the out that is stored
template <typename T> struct AxpbyNormF {
  static constexpr int NV = 1;
  const char *x, *y;
  char *out;
  T alpha, beta;
  double acc[NV];
  template <typename V> __device__ __forceinline__ void at(int64_t off) {
    const V vx = *(const V *)(x + off), vy = *(const V *)(y + off);
    const V vo = axpby_bits(alpha, vx, beta, vy);
    *(V *)(out + off) = vo;
    add_prod(acc[0], vo, vo);
  }
};

// (a . b, a . a)
struct DotPairF {
  static constexpr int NV = 2;
  const char *a, *b;
  double acc[NV];
  template <typename V> __device__ __forceinline__ void at(int64_t off) {
    const V va = *(const V *)(a + off), vb = *(const V *)(b + off);
    add_prod(acc[0], va, vb);
    add_prod(acc[1], va, va);
  }
};

// x += alpha y + omega z; r -= omega t; (r_new . r_new, rhat . r_new).
// z may be the buffer of r (no __restrict__ anywhere): every load of a cell
// stands before its stores.
template <typename T> struct BicgF {
  static constexpr int NV = 2;
  const char *y, *z;
  char *x, *r;
  const char *t, *rhat;
  T alpha, omega;
  double acc[NV];
  template <typename V> __device__ __forceinline__ void at(int64_t off) {
    const V vy = *(const V *)(y + off), vz = *(const V *)(z + off);
    const V vt = *(const V *)(t + off), vh = *(const V *)(rhat + off);
    const V vx = *(const V *)(x + off), vr = *(const V *)(r + off);
    const V rn = vr - omega * vt;
    *(V *)(x + off) = vx + alpha * vy + omega * vz;
    *(V *)(r + off) = rn;
    add_prod(acc[0], rn, rn);
    add_prod(acc[1], vh, rn);
  }
};

// Waves per SIMD a reduction is held to; 0: the compiler's choice.
// DotF<true> in float: the 4 x unrolled strip loop wants 74 VGPRs to keep
// its 8 loads in flight. Held to 64 (8 waves per SIMD) the scheduler
// serialises them, 2 in flight, and the kernel runs 5-6% behind DotF<false>;
// at 6 waves it batches them as DotF<false> does. double fits 8 waves as it
// is.
// DotPairF in float is the same case with the other outcome of the same
// pressure: left to the compiler it takes 26 VGPRs and waits after every
// pair of loads; at 6 waves it takes 72 and keeps the 8 loads in flight
// (0.24 ms at 512^3, DotF<false>'s time). double batches at 8 waves in 44.
// AxpbyNormF (32 VGPRs) and BicgF (70 in float, 7 waves; 62 in double) have
// no entry: their stores may alias the next plane's loads, so a plane's
// loads (2 and 6) are issued together and waited for before its stores, as
// in CgF, whatever the budget; they run at the rate of the storing kernels
// (BASELINE.md "BiCGStab").
template <typename F, typename T> constexpr int kWaves = 0;
template <typename T> constexpr int kWaves<DotF<true>, T> = sizeof(T) == 4 ? 6 : 8;
template <typename T> constexpr int kWaves<DotPairF, T> = sizeof(T) == 4 ? 6 : 8;

template <typename T, bool STRIPS, typename F>
__global__ void __launch_bounds__(256) field_kernel(Geom g, F f) {
  walk<T, STRIPS>(g, f);
}

template <typename T, bool STRIPS, typename F>
__global__ void __launch_bounds__(256)
    __attribute__((amdgpu_waves_per_eu(kWaves<F, T>, kWaves<F, T>)))
    reduce_kernel(Geom g, F f, double *partials) {
  // zeroed here: what the argument holds the compiler would have to load
#pragma unroll
  for (int k = 0; k < F::NV; ++k) f.acc[k] = 0.0;
  walk<T, STRIPS>(g, f);
  block_store_sums<F::NV>(f.acc, partials);
}

// AxpbypczF keeps a kernel with loose arguments. In float the bits of
// alpha x + beta y + gamma z depend on which product the compiler contracts
// into an fma first, and from this form it picks beta y (cells walk:
// fma(beta, y, alpha x) + gamma z), from field_kernel alpha x.
template <typename T, bool STRIPS>
__global__ void __launch_bounds__(256)
    axpbypcz_kernel(Geom g, const char *x, const char *y, const char *z, char *out, T alpha,
                    T beta, T gamma) {
  AxpbypczF<T> f{x, y, z, out, alpha, beta, gamma};
  walk<T, STRIPS>(g, f);
}

//// host ////

struct Launch {
  LocalDomain *d = nullptr;
  bool empty = false;
  bool strips = false;
  int64_t es = 0;
  Geom g{};
  dim3 grid, block;
  int blocks = 0;
  RegionCells c; // each operand's first cell of the region
};

// Validate and shape one op. Throws std::invalid_argument before anything
// is launched or allocated.
Launch plan_launch(const char *op, ExchangeEngine &eng, int dom,
                   std::initializer_list<Operand> operands, const Rect3 &region) {
  Launch l;
  l.d = &checked_domain(op, eng, dom);
  l.es = checked_elem_size(op, *l.d, operands);
  if (!checked_extent(op, region)) {
    l.empty = true;
    return l;
  }
  const Rect3 full = l.d->full_region();
  check_inside(op, "region", region, full);
  l.c = region_cells(op, *l.d, operands, region.lo - full.lo, l.es);
  const Vec3 ext = region.extent();
  l.g.pitch = l.c.pitch;
  l.g.plane = l.c.plane;
  l.g.extX = (int32_t)ext.x;
  l.g.extY = (int32_t)ext.y;
  l.g.extZ = (int32_t)ext.z;

  // strips: as launch_stencil's stripOk, over every operand pointer
  const int n = (int)(16 / l.es);
  bool ok = ext.x >= 8 && l.c.pitch % 16 == 0;
  for (int i = 0; i < l.c.n; ++i) {
    const uintptr_t p = (uintptr_t)l.c.ptr[i];
    ok = ok && (p & 15) == ((uintptr_t)l.c.ptr[0] & 15) && (p % l.es) == 0;
  }
  if (ok) {
    const int64_t head = head_cells(l.c.ptr[0], l.es);
    const int64_t units = ext.x - ((ext.x - head) / n) * (n - 1);
    const int64_t gx = (units + kBx - 1) / kBx, gy = (ext.y + kBy - 1) / kBy;
    if (gx * gy <= ExchangeEngine::kReducePartials) {
      // as many z chunks as the grid cap admits, each at least kMinZc planes
      const int64_t maxGz = ExchangeEngine::kReducePartials / (gx * gy);
      const int64_t zc = std::max<int64_t>((ext.z + maxGz - 1) / maxGz, std::min<int64_t>(kMinZc, ext.z));
      const int64_t gz = (ext.z + zc - 1) / zc;
      l.strips = true;
      l.g.head = (int32_t)head;
      l.g.zc = (int32_t)zc;
      l.block = dim3(kBx, kBy, 1);
      l.grid = dim3((uint32_t)gx, (uint32_t)gy, (uint32_t)gz);
      l.blocks = (int)(gx * gy * gz);
      return l;
    }
  }
  const int64_t total = ext.flatten();
  l.blocks = (int)std::min<int64_t>((total + 255) / 256, ExchangeEngine::kReducePartials);
  l.block = dim3(256, 1, 1);
  l.grid = dim3((uint32_t)l.blocks, 1, 1);
  return l;
}

// fn(T(), std::bool_constant<STRIPS>()) with the quantity's type and the walk
template <typename Fn> void dispatch(const Launch &l, Fn fn) {
  auto typed = [&](auto t) {
    if (l.strips)
      fn(t, std::true_type());
    else
      fn(t, std::false_type());
  };
  if (l.es == 4)
    typed(float());
  else
    typed(double());
  STENCIL_HIP(hipGetLastError());
}

template <typename T, bool STRIPS, typename F>
void launch_field(const Launch &l, hipStream_t stream, const F &f) {
  hipLaunchKernelGGL((field_kernel<T, STRIPS, F>), l.grid, l.block, 0, stream, l.g, f);
}
template <typename T, bool STRIPS>
void launch_field(const Launch &l, hipStream_t stream, const AxpbypczF<T> &f) {
  hipLaunchKernelGGL((axpbypcz_kernel<T, STRIPS>), l.grid, l.block, 0, stream, l.g, f.x, f.y, f.z,
                     f.out, f.alpha, f.beta, f.gamma);
}

// An element-wise op. make(T(), ptr) gives the functor over the operands'
// first cells ptr[i], T the quantity's type: the (T) it puts on a scalar is
// that scalar's one rounding.
template <typename Make>
void run_field(const char *op, ExchangeEngine &eng, int dom,
               std::initializer_list<Operand> operands, const Rect3 &region, int streamId,
               Make make) {
  const Launch l = plan_launch(op, eng, dom, operands, region);
  if (l.empty) return;
  STENCIL_HIP(hipSetDevice(l.d->gpu()));
  hipStream_t stream = eng.compute_stream(dom, streamId);
  dispatch(l, [&](auto t, auto strips) {
    launch_field<decltype(t), decltype(strips)::value>(l, stream, make(t, l.c.ptr));
  });
}

// Leave a reduction of `values` values and `count` partials each in flight;
// count > 0: the partials go to the pinned host buffer behind the kernel,
// reduction_end_n waits. count = 0 is the empty region.
void land(ExchangeEngine::ReduceScratch &sc, int count, int values, hipStream_t stream) {
  if (count > 0)
    STENCIL_HIP(hipMemcpyAsync(sc.host, sc.dev, (size_t)values * (size_t)count * sizeof(double),
                               hipMemcpyDeviceToHost, stream));
  sc.stream = stream;
  sc.count = count;
  sc.values = values;
  sc.pending = true;
}

// A reduction: run_field with a functor that has NV and acc[NV]. Throws
// std::runtime_error, launching nothing, while another is in flight.
template <typename Make>
void begin_reduce(const char *op, ExchangeEngine &eng, int dom,
                  std::initializer_list<Operand> operands, const Rect3 &region, int streamId,
                  Make make) {
  const Launch l = plan_launch(op, eng, dom, operands, region);
  ExchangeEngine::ReduceScratch &sc = eng.reduce_scratch(dom, !l.empty);
  if (sc.pending)
    throw std::runtime_error(std::string(op) + ": a reduction is already in flight on domain " +
                             std::to_string(dom) + " (call reduction_end first)");
  constexpr int NV = decltype(make(float(), l.c.ptr))::NV;
  if (l.empty) return land(sc, 0, NV, nullptr);
  STENCIL_HIP(hipSetDevice(l.d->gpu()));
  hipStream_t stream = eng.compute_stream(dom, streamId);
  dispatch(l, [&](auto t, auto strips) {
    auto f = make(t, l.c.ptr);
    typedef decltype(f) F;
    static_assert(F::NV == NV && NV <= ExchangeEngine::kReduceValues, "value count");
    hipLaunchKernelGGL((reduce_kernel<decltype(t), decltype(strips)::value, F>), l.grid, l.block, 0,
                       stream, l.g, f, sc.dev);
  });
  land(sc, l.blocks, NV, stream);
}

void check_distinct(const char *op, int64_t x, int64_t p, int64_t r) {
  if (x == p || x == r || p == r)
    throw std::invalid_argument(std::string(op) + ": x, p and r must be distinct quantities");
}

// bicgstab_update writes curr[x] and curr[r]: neither may be the other, nor
// a buffer the op only reads, except z, which may be r's (every cell is
// read before it is written)
void check_distinct_bicg(const char *op, int64_t x, int64_t r, const Operand &y, const Operand &t,
                         const Operand &rhat) {
  bool bad = x == r;
  for (const Operand *o : {&y, &t, &rhat}) bad = bad || (!o->next && (o->q == x || o->q == r));
  if (bad)
    throw std::invalid_argument(std::string(op) + ": x and r must be distinct from each other "
                                                  "and from y, t and rhat");
}

} // namespace

void field_axpby_norm2_begin(ExchangeEngine &eng, int dom, double alpha, int64_t x, bool xNext,
                             double beta, int64_t y, bool yNext, int64_t out, bool outNext,
                             const Rect3 &region, int streamId) {
  begin_reduce("field_axpby_norm2", eng, dom, {{x, xNext}, {y, yNext}, {out, outNext}}, region,
               streamId, [=](auto t, char *const *p) {
                 typedef decltype(t) T;
                 return AxpbyNormF<T>{p[0], p[1], p[2], (T)alpha, (T)beta, {}};
               });
}

void field_dot_pair_begin(ExchangeEngine &eng, int dom, int64_t a, bool aNext, int64_t b,
                          bool bNext, const Rect3 &region, int streamId) {
  begin_reduce("field_dot_pair", eng, dom, {{a, aNext}, {b, bNext}}, region, streamId,
               [](auto, char *const *p) { return DotPairF{p[0], p[1], {}}; });
}

// operands: y, z, curr[x], curr[r], t, rhat
void bicgstab_update_begin(ExchangeEngine &eng, int dom, double alpha, int64_t y, bool yNext,
                           double omega, int64_t z, bool zNext, int64_t x, int64_t r, int64_t t,
                           bool tNext, int64_t rhat, bool rhatNext, const Rect3 &region,
                           int streamId) {
  check_distinct_bicg("bicgstab_update", x, r, {y, yNext}, {t, tNext}, {rhat, rhatNext});
  begin_reduce("bicgstab_update", eng, dom,
               {{y, yNext}, {z, zNext}, {x, false}, {r, false}, {t, tNext}, {rhat, rhatNext}},
               region, streamId, [=](auto ty, char *const *q) {
                 typedef decltype(ty) T;
                 return BicgF<T>{q[0], q[1], q[2], q[3], q[4], q[5], (T)alpha, (T)omega, {}};
               });
}

double field_axpby_norm2(ExchangeEngine &eng, int dom, double alpha, int64_t x, bool xNext,
                         double beta, int64_t y, bool yNext, int64_t out, bool outNext,
                         const Rect3 &region, int streamId) {
  field_axpby_norm2_begin(eng, dom, alpha, x, xNext, beta, y, yNext, out, outNext, region,
                          streamId);
  return reduction_end(eng, dom);
}

std::array<double, 2> field_dot_pair(ExchangeEngine &eng, int dom, int64_t a, bool aNext,
                                     int64_t b, bool bNext, const Rect3 &region, int streamId) {
  field_dot_pair_begin(eng, dom, a, aNext, b, bNext, region, streamId);
  std::array<double, 2> out{};
  reduction_end_n(eng, dom, out.data(), 2);
  return out;
}

std::array<double, 2> bicgstab_update(ExchangeEngine &eng, int dom, double alpha, int64_t y,
                                      bool yNext, double omega, int64_t z, bool zNext, int64_t x,
                                      int64_t r, int64_t t, bool tNext, int64_t rhat,
                                      bool rhatNext, const Rect3 &region, int streamId) {
  bicgstab_update_begin(eng, dom, alpha, y, yNext, omega, z, zNext, x, r, t, tNext, rhat,
                        rhatNext, region, streamId);
  std::array<double, 2> out{};
  reduction_end_n(eng, dom, out.data(), 2);
  return out;
}

void field_dot_begin(ExchangeEngine &eng, int dom, int64_t a, bool aNext, int64_t b, bool bNext,
                     const Rect3 &region, int streamId) {
  begin_reduce("field_dot", eng, dom, {{a, aNext}, {b, bNext}}, region, streamId,
               [](auto, char *const *p) { return DotF<false>{p[0], p[1], {}}; });
}

void field_dot_sums_begin(ExchangeEngine &eng, int dom, int64_t a, bool aNext, int64_t b,
                          bool bNext, const Rect3 &region, int streamId) {
  begin_reduce("field_dot_sums", eng, dom, {{a, aNext}, {b, bNext}}, region, streamId,
               [](auto, char *const *p) { return DotF<true>{p[0], p[1], {}}; });
}

void field_sum_begin(ExchangeEngine &eng, int dom, int64_t a, bool aNext, const Rect3 &region,
                     int streamId) {
  begin_reduce("field_sum", eng, dom, {{a, aNext}}, region, streamId,
               [](auto, char *const *p) { return SumF{p[0], {}}; });
}

// operands of both: curr[x], curr[p], next[p] (= A p), curr[r]
void cg_update_begin(ExchangeEngine &eng, int dom, double alpha, int64_t x, int64_t p, int64_t r,
                     const Rect3 &region, int streamId) {
  check_distinct("cg_update", x, p, r);
  begin_reduce("cg_update", eng, dom, {{x, false}, {p, false}, {p, true}, {r, false}}, region,
               streamId, [=](auto t, char *const *q) {
                 typedef decltype(t) T;
                 return CgF<T, false>{q[0], q[1], q[2], q[3], (T)alpha, {}};
               });
}

void cg_update_sum_begin(ExchangeEngine &eng, int dom, double alpha, int64_t x, int64_t p,
                         int64_t r, const Rect3 &region, int streamId) {
  check_distinct("cg_update_sum", x, p, r);
  begin_reduce("cg_update_sum", eng, dom, {{x, false}, {p, false}, {p, true}, {r, false}}, region,
               streamId, [=](auto t, char *const *q) {
                 typedef decltype(t) T;
                 return CgF<T, true>{q[0], q[1], q[2], q[3], (T)alpha, {}};
               });
}

void reduction_end_n(ExchangeEngine &eng, int dom, double *out, int n) {
  checked_domain("reduction_end", eng, dom);
  if (out == nullptr || n < 1 || n > ExchangeEngine::kReduceValues)
    throw std::invalid_argument("reduction_end: want 1.." +
                                std::to_string(ExchangeEngine::kReduceValues) + " values, got " +
                                std::to_string(n));
  ExchangeEngine::ReduceScratch &sc = eng.reduce_scratch(dom, false);
  if (!sc.pending)
    throw std::runtime_error("reduction_end: no reduction in flight on domain " +
                             std::to_string(dom));
  if (sc.values != n) // it stays in flight
    throw std::runtime_error("reduction_end: the reduction in flight on domain " +
                             std::to_string(dom) + " has " + std::to_string(sc.values) +
                             " values, not " + std::to_string(n));
  sc.pending = false;
  for (int v = 0; v < n; ++v) out[v] = 0.0;
  if (sc.count == 0) return;
  STENCIL_HIP(hipSetDevice(eng.domain(dom).gpu()));
  STENCIL_HIP(hipStreamSynchronize(sc.stream));
  for (int v = 0; v < n; ++v) {
    const double *part = sc.host + (size_t)v * (size_t)sc.count;
    double sum = 0.0;
    for (int i = 0; i < sc.count; ++i) sum += part[i]; // index order
    out[v] = sum;
  }
}

double reduction_end(ExchangeEngine &eng, int dom) {
  double out = 0.0;
  reduction_end_n(eng, dom, &out, 1);
  return out;
}

double field_dot(ExchangeEngine &eng, int dom, int64_t a, bool aNext, int64_t b, bool bNext,
                 const Rect3 &region, int streamId) {
  field_dot_begin(eng, dom, a, aNext, b, bNext, region, streamId);
  return reduction_end(eng, dom);
}

double cg_update(ExchangeEngine &eng, int dom, double alpha, int64_t x, int64_t p, int64_t r,
                 const Rect3 &region, int streamId) {
  cg_update_begin(eng, dom, alpha, x, p, r, region, streamId);
  return reduction_end(eng, dom);
}

double field_sum(ExchangeEngine &eng, int dom, int64_t a, bool aNext, const Rect3 &region,
                 int streamId) {
  field_sum_begin(eng, dom, a, aNext, region, streamId);
  return reduction_end(eng, dom);
}

std::array<double, 3> field_dot_sums(ExchangeEngine &eng, int dom, int64_t a, bool aNext,
                                     int64_t b, bool bNext, const Rect3 &region, int streamId) {
  field_dot_sums_begin(eng, dom, a, aNext, b, bNext, region, streamId);
  std::array<double, 3> out{};
  reduction_end_n(eng, dom, out.data(), 3);
  return out;
}

std::array<double, 2> cg_update_sum(ExchangeEngine &eng, int dom, double alpha, int64_t x,
                                    int64_t p, int64_t r, const Rect3 &region, int streamId) {
  cg_update_sum_begin(eng, dom, alpha, x, p, r, region, streamId);
  std::array<double, 2> out{};
  reduction_end_n(eng, dom, out.data(), 2);
  return out;
}

void field_axpby(ExchangeEngine &eng, int dom, double alpha, int64_t x, bool xNext, double beta,
                 int64_t y, bool yNext, int64_t out, bool outNext, const Rect3 &region,
                 int streamId) {
  run_field("field_axpby", eng, dom, {{x, xNext}, {y, yNext}, {out, outNext}}, region, streamId,
            [=](auto t, char *const *p) {
              typedef decltype(t) T;
              return AxpbyF<T>{p[0], p[1], p[2], (T)alpha, (T)beta};
            });
}

void field_axpbyc(ExchangeEngine &eng, int dom, double alpha, int64_t x, bool xNext, double beta,
                  int64_t y, bool yNext, double c, int64_t out, bool outNext,
                  const Rect3 &region, int streamId) {
  run_field("field_axpbyc", eng, dom, {{x, xNext}, {y, yNext}, {out, outNext}}, region, streamId,
            [=](auto t, char *const *p) {
              typedef decltype(t) T;
              return AxpbycF<T>{p[0], p[1], p[2], (T)alpha, (T)beta, (T)c};
            });
}

void field_axpbypcz(ExchangeEngine &eng, int dom, double alpha, int64_t x, bool xNext,
                    double beta, int64_t y, bool yNext, double gamma, int64_t z, bool zNext,
                    int64_t out, bool outNext, const Rect3 &region, int streamId) {
  run_field("field_axpbypcz", eng, dom, {{x, xNext}, {y, yNext}, {z, zNext}, {out, outNext}},
            region, streamId, [=](auto t, char *const *p) {
              typedef decltype(t) T;
              return AxpbypczF<T>{p[0], p[1], p[2], p[3], (T)alpha, (T)beta, (T)gamma};
            });
}

void field_scaled_update(ExchangeEngine &eng, int dom, double alpha, int64_t x, bool xNext,
                         int64_t d, bool dNext, double beta, int64_t y, bool yNext, double gamma,
                         int64_t z, bool zNext, int64_t out, bool outNext, const Rect3 &region,
                         int streamId) {
  run_field("field_scaled_update", eng, dom,
            {{x, xNext}, {d, dNext}, {y, yNext}, {z, zNext}, {out, outNext}}, region, streamId,
            [=](auto t, char *const *p) {
              typedef decltype(t) T;
              return ScaledF<T>{p[0], p[1], p[2], p[3], p[4], (T)alpha, (T)beta, (T)gamma};
            });
}

} // namespace stencil_amd
