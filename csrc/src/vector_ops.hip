// Vector operations on pitched quantities for gfx950: the inner product,
// out = alpha x + beta y, out = alpha x + beta y + gamma z, the diagonally
// scaled out = alpha x + d (beta y + gamma z), and the fused
// conjugate-gradient update. Pure
// streaming kernels: every cell of the region is read (and written) once.
// For singular problems (the constant null space, solvers/cg.py) also the
// sum of a field, the inner product together with both sums, the fused
// update together with sum r_new, and out = alpha x + beta y + c: the
// projection v - mean(v) rides on passes the iteration makes anyway.
//
// Contract (the stencil operator's): nothing outside `region` is written
// in any buffer, and no cell outside it enters the arithmetic. Unlike the
// star kernel these kernels never load a cell outside the region either:
// the 16 B strips cover aligned cells of the region only, the cells before
// the first and after the last aligned strip of a row get a lane each.
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
// shuffles per wave, LDS per block, one partial per block written with an
// ordinary store, the partials summed in index order on the host. No
// atomics. The grid never exceeds ExchangeEngine::kReducePartials blocks;
// the engine's per-domain scratch holds kReduceValues times as many
// doubles, value-major (partials[v * blocks + b]), for the reductions that
// return up to three values from one pass.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <initializer_list>
#include <stdexcept>
#include <string>
#include <vector>

#include "stencil_amd/domain.hpp"
#include "stencil_amd/engine.hpp"
#include "stencil_amd/hip_check.hpp"
#include "stencil_amd/ops.hpp"

namespace stencil_amd {

namespace {

constexpr int kBx = 64, kBy = 4; // strip block: one wave per row, 4 rows
constexpr int kMinZc = 4;        // planes per thread, when the region has them

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

// Every thread of the 256-thread block calls this once (threads without a
// cell bring 0): wave sums by shuffles, the 4 wave sums through LDS, one
// ordinary store per block. A fixed order: the same bits every time.
__device__ __forceinline__ void block_sum_store(double v, double *partials) {
  __shared__ double sWave[4];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  const int tid = threadIdx.y * blockDim.x + threadIdx.x;
  if ((tid & 63) == 0) sWave[tid >> 6] = v;
  __syncthreads();
  if (tid == 0) {
    const int64_t b = ((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    partials[b] = ((sWave[0] + sWave[1]) + sWave[2]) + sWave[3];
  }
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

// block_sum_store for NV values at once: value v of block b lands in
// partials[v * blocks + b]. The same fixed order per value.
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

struct DotF {
  const char *a, *b;
  double acc;
  template <typename V> __device__ __forceinline__ void at(int64_t off) {
    add_prod(acc, *(const V *)(a + off), *(const V *)(b + off));
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

template <typename T> struct CgF {
  char *x, *r;
  const char *p, *ap;
  T alpha;
  double acc;
  template <typename V> __device__ __forceinline__ void at(int64_t off) {
    const V vp = *(const V *)(p + off), vap = *(const V *)(ap + off);
    const V vx = *(const V *)(x + off), vr = *(const V *)(r + off);
    const V rn = vr - alpha * vap;
    *(V *)(x + off) = vx + alpha * vp;
    *(V *)(r + off) = rn;
    add_prod(acc, rn, rn);
  }
};

struct SumF {
  const char *a;
  double acc;
  template <typename V> __device__ __forceinline__ void at(int64_t off) {
    add_val(acc, *(const V *)(a + off));
  }
};

struct DotSumsF {
  const char *a, *b;
  double ab, sa, sb;
  template <typename V> __device__ __forceinline__ void at(int64_t off) {
    const V va = *(const V *)(a + off), vb = *(const V *)(b + off);
    add_prod(ab, va, vb);
    add_val(sa, va);
    add_val(sb, vb);
  }
};

// CgF's arithmetic, statement for statement, plus sum r_new
template <typename T> struct CgSumF {
  char *x, *r;
  const char *p, *ap;
  T alpha;
  double acc, sum;
  template <typename V> __device__ __forceinline__ void at(int64_t off) {
    const V vp = *(const V *)(p + off), vap = *(const V *)(ap + off);
    const V vx = *(const V *)(x + off), vr = *(const V *)(r + off);
    const V rn = vr - alpha * vap;
    *(V *)(x + off) = vx + alpha * vp;
    *(V *)(r + off) = rn;
    add_prod(acc, rn, rn);
    add_val(sum, rn);
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

template <typename T, bool STRIPS>
__global__ void __launch_bounds__(256)
    dot_kernel(Geom g, const char *a, const char *b, double *partials) {
  DotF f{a, b, 0.0};
  walk<T, STRIPS>(g, f);
  block_sum_store(f.acc, partials);
}

template <typename T, bool STRIPS>
__global__ void __launch_bounds__(256)
    axpby_kernel(Geom g, const char *x, const char *y, char *out, T alpha, T beta) {
  AxpbyF<T> f{x, y, out, alpha, beta};
  walk<T, STRIPS>(g, f);
}

template <typename T, bool STRIPS>
__global__ void __launch_bounds__(256)
    axpbypcz_kernel(Geom g, const char *x, const char *y, const char *z, char *out, T alpha,
                    T beta, T gamma) {
  AxpbypczF<T> f{x, y, z, out, alpha, beta, gamma};
  walk<T, STRIPS>(g, f);
}

template <typename T, bool STRIPS>
__global__ void __launch_bounds__(256)
    scaled_update_kernel(Geom g, const char *x, const char *d, const char *y, const char *z,
                         char *out, T alpha, T beta, T gamma) {
  ScaledF<T> f{x, d, y, z, out, alpha, beta, gamma};
  walk<T, STRIPS>(g, f);
}

template <typename T, bool STRIPS>
__global__ void __launch_bounds__(256)
    cg_update_kernel(Geom g, char *x, const char *p, const char *ap, char *r, T alpha,
                     double *partials) {
  CgF<T> f{x, r, p, ap, alpha, 0.0};
  walk<T, STRIPS>(g, f);
  block_sum_store(f.acc, partials);
}

template <typename T, bool STRIPS>
__global__ void __launch_bounds__(256) sum_kernel(Geom g, const char *a, double *partials) {
  SumF f{a, 0.0};
  walk<T, STRIPS>(g, f);
  const double v[1] = {f.acc};
  block_store_sums<1>(v, partials);
}

// float: the 4 x unrolled strip loop wants 74 VGPRs to keep its 8 loads in
// flight. Held to 64 (8 waves per SIMD) the scheduler serialises them, 2 in
// flight, and the kernel runs 5-6% behind dot_kernel; at 6 waves it batches
// them as dot_kernel does. double fits 8 waves as it is.
template <typename T, bool STRIPS>
__global__ void __launch_bounds__(256)
    __attribute__((amdgpu_waves_per_eu(sizeof(T) == 4 ? 6 : 8, sizeof(T) == 4 ? 6 : 8)))
    dot_sums_kernel(Geom g, const char *a, const char *b, double *partials) {
  DotSumsF f{a, b, 0.0, 0.0, 0.0};
  walk<T, STRIPS>(g, f);
  const double v[3] = {f.ab, f.sa, f.sb};
  block_store_sums<3>(v, partials);
}

template <typename T, bool STRIPS>
__global__ void __launch_bounds__(256)
    cg_update_sum_kernel(Geom g, char *x, const char *p, const char *ap, char *r, T alpha,
                         double *partials) {
  CgSumF<T> f{x, r, p, ap, alpha, 0.0, 0.0};
  walk<T, STRIPS>(g, f);
  const double v[2] = {f.acc, f.sum};
  block_store_sums<2>(v, partials);
}

template <typename T, bool STRIPS>
__global__ void __launch_bounds__(256)
    axpbyc_kernel(Geom g, const char *x, const char *y, char *out, T alpha, T beta, T c) {
  AxpbycF<T> f{x, y, out, alpha, beta, c};
  walk<T, STRIPS>(g, f);
}

//// host ////

struct Operand {
  int64_t q;
  bool next;
};

struct Launch {
  LocalDomain *d = nullptr;
  bool empty = false;
  bool strips = false;
  int64_t es = 0;
  Geom g{};
  dim3 grid, block;
  int blocks = 0;
  std::vector<char *> ptr; // each operand's first cell of the region
};

// Validate and shape one op. Throws std::invalid_argument before anything
// is launched or allocated.
Launch plan_launch(const char *op, ExchangeEngine &eng, int dom,
                   std::initializer_list<Operand> operands, const Rect3 &region) {
  const std::string name(op);
  if (dom < 0 || dom >= eng.num_domains())
    throw std::invalid_argument(name + ": no such domain " + std::to_string(dom));
  Launch l;
  l.d = &eng.domain(dom);
  LocalDomain &d = *l.d;
  for (const Operand &o : operands) {
    if (o.q < 0 || o.q >= d.num_data()) throw std::invalid_argument(name + ": no such quantity");
    const int64_t es = d.elem_size(o.q);
    if (es != 4 && es != 8)
      throw std::invalid_argument(name + ": float32/float64 quantities only (element size " +
                                  std::to_string(es) + ")");
    if (l.es != 0 && es != l.es)
      throw std::invalid_argument(name + ": operands differ in element size");
    l.es = es;
  }
  const Vec3 ext = region.extent();
  if (ext.x <= 0 || ext.y <= 0 || ext.z <= 0) {
    l.empty = true;
    return l;
  }
  if (ext.x > 0x7fffffff || ext.y > 0x7fffffff || ext.z > 0x7fffffff)
    throw std::invalid_argument(name + ": region extent exceeds 2^31 - 1");
  const Rect3 full = d.full_region();
  if (region.lo.x < full.lo.x || region.lo.y < full.lo.y || region.lo.z < full.lo.z ||
      region.hi.x > full.hi.x || region.hi.y > full.hi.y || region.hi.z > full.hi.z)
    throw std::invalid_argument(name + ": region " + region.str() +
                                " is outside the allocation " + full.str());
  const Vec3 pos = region.lo - full.lo; // allocation coords
  const Pitched &first = d.curr(operands.begin()->q);
  for (const Operand &o : operands) {
    const Pitched &pp = o.next ? d.next(o.q) : d.curr(o.q);
    if (pp.pitch != first.pitch || pp.ysize != first.ysize)
      throw std::invalid_argument(name + ": operand layouts differ");
    l.ptr.push_back(pp.ptr + pos.z * pp.plane() + pos.y * pp.pitch + pos.x * l.es);
  }
  l.g.pitch = first.pitch;
  l.g.plane = first.plane();
  l.g.extX = (int32_t)ext.x;
  l.g.extY = (int32_t)ext.y;
  l.g.extZ = (int32_t)ext.z;

  // strips: as launch_stencil's stripOk, over every operand pointer
  const int n = (int)(16 / l.es);
  bool ok = ext.x >= 8 && first.pitch % 16 == 0;
  for (char *p : l.ptr)
    ok = ok && ((uintptr_t)p & 15) == ((uintptr_t)l.ptr[0] & 15) && ((uintptr_t)p % l.es) == 0;
  if (ok) {
    const int64_t head = (int64_t)((16 - ((uintptr_t)l.ptr[0] & 15)) & 15) / l.es;
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

#define VEC_OPS_LAUNCH(T, l, KERNEL, stream, ...)                                                 \
  do {                                                                                             \
    if ((l).strips)                                                                                \
      hipLaunchKernelGGL((KERNEL<T, true>), (l).grid, (l).block, 0, stream, __VA_ARGS__);          \
    else                                                                                           \
      hipLaunchKernelGGL((KERNEL<T, false>), (l).grid, (l).block, 0, stream, __VA_ARGS__);         \
    STENCIL_HIP(hipGetLastError());                                                                \
  } while (0)

ExchangeEngine::ReduceScratch &begin_reduction(const char *op, ExchangeEngine &eng, int dom,
                                               bool allocate) {
  ExchangeEngine::ReduceScratch &sc = eng.reduce_scratch(dom, allocate);
  if (sc.pending)
    throw std::runtime_error(std::string(op) + ": a reduction is already in flight on domain " +
                             std::to_string(dom) + " (call reduction_end first)");
  return sc;
}

// partials -> pinned host buffer behind the kernel; reduction_end waits
void land_partials(ExchangeEngine::ReduceScratch &sc, int blocks, hipStream_t stream) {
  STENCIL_HIP(hipMemcpyAsync(sc.host, sc.dev, (size_t)blocks * sizeof(double),
                             hipMemcpyDeviceToHost, stream));
  sc.stream = stream;
  sc.count = blocks;
  sc.pending = true;
}

// the n-valued form: value-major partials, n * blocks doubles in one copy
void land_partials_n(ExchangeEngine::ReduceScratch &sc, int blocks, int n, hipStream_t stream) {
  STENCIL_HIP(hipMemcpyAsync(sc.host, sc.dev, (size_t)n * (size_t)blocks * sizeof(double),
                             hipMemcpyDeviceToHost, stream));
  sc.stream = stream;
  sc.count = blocks;
  sc.values = n;
  sc.pending = true;
}

void land_empty_n(ExchangeEngine::ReduceScratch &sc, int n) {
  sc.count = 0;
  sc.values = n;
  sc.pending = true;
}

} // namespace

void field_dot_begin(ExchangeEngine &eng, int dom, int64_t a, bool aNext, int64_t b, bool bNext,
                     const Rect3 &region, int streamId) {
  const Launch l = plan_launch("field_dot", eng, dom, {{a, aNext}, {b, bNext}}, region);
  ExchangeEngine::ReduceScratch &sc = begin_reduction("field_dot", eng, dom, !l.empty);
  if (l.empty) {
    sc.count = 0;
    sc.pending = true;
    return;
  }
  STENCIL_HIP(hipSetDevice(l.d->gpu()));
  hipStream_t stream = eng.compute_stream(dom, streamId);
  if (l.es == 4)
    VEC_OPS_LAUNCH(float, l, dot_kernel, stream, l.g, (const char *)l.ptr[0],
                   (const char *)l.ptr[1], sc.dev);
  else
    VEC_OPS_LAUNCH(double, l, dot_kernel, stream, l.g, (const char *)l.ptr[0],
                   (const char *)l.ptr[1], sc.dev);
  land_partials(sc, l.blocks, stream);
}

void cg_update_begin(ExchangeEngine &eng, int dom, double alpha, int64_t x, int64_t p, int64_t r,
                     const Rect3 &region, int streamId) {
  // operands: curr[x], curr[p], next[p] (= A p), curr[r]
  const Launch l =
      plan_launch("cg_update", eng, dom, {{x, false}, {p, false}, {p, true}, {r, false}}, region);
  if (x == p || x == r || p == r)
    throw std::invalid_argument("cg_update: x, p and r must be distinct quantities");
  ExchangeEngine::ReduceScratch &sc = begin_reduction("cg_update", eng, dom, !l.empty);
  if (l.empty) {
    sc.count = 0;
    sc.pending = true;
    return;
  }
  STENCIL_HIP(hipSetDevice(l.d->gpu()));
  hipStream_t stream = eng.compute_stream(dom, streamId);
  if (l.es == 4) {
    const float al = (float)alpha; // the one rounding to the quantity's type
    VEC_OPS_LAUNCH(float, l, cg_update_kernel, stream, l.g, l.ptr[0], (const char *)l.ptr[1],
                   (const char *)l.ptr[2], l.ptr[3], al, sc.dev);
  } else {
    VEC_OPS_LAUNCH(double, l, cg_update_kernel, stream, l.g, l.ptr[0], (const char *)l.ptr[1],
                   (const char *)l.ptr[2], l.ptr[3], alpha, sc.dev);
  }
  land_partials(sc, l.blocks, stream);
}

double reduction_end(ExchangeEngine &eng, int dom) {
  if (dom < 0 || dom >= eng.num_domains())
    throw std::invalid_argument("reduction_end: no such domain " + std::to_string(dom));
  ExchangeEngine::ReduceScratch &sc = eng.reduce_scratch(dom, false);
  if (!sc.pending)
    throw std::runtime_error("reduction_end: no reduction in flight on domain " +
                             std::to_string(dom));
  if (sc.values != 1)
    throw std::runtime_error("reduction_end: the reduction in flight on domain " +
                             std::to_string(dom) + " has " + std::to_string(sc.values) +
                             " values (call reduction_end_n)");
  sc.pending = false;
  if (sc.count == 0) return 0.0;
  STENCIL_HIP(hipSetDevice(eng.domain(dom).gpu()));
  STENCIL_HIP(hipStreamSynchronize(sc.stream));
  double sum = 0.0;
  for (int i = 0; i < sc.count; ++i) sum += sc.host[i]; // index order
  return sum;
}

void reduction_end_n(ExchangeEngine &eng, int dom, double *out, int n) {
  if (dom < 0 || dom >= eng.num_domains())
    throw std::invalid_argument("reduction_end_n: no such domain " + std::to_string(dom));
  if (out == nullptr || n < 1 || n > ExchangeEngine::kReduceValues)
    throw std::invalid_argument("reduction_end_n: want 1.." +
                                std::to_string(ExchangeEngine::kReduceValues) + " values, got " +
                                std::to_string(n));
  ExchangeEngine::ReduceScratch &sc = eng.reduce_scratch(dom, false);
  if (!sc.pending)
    throw std::runtime_error("reduction_end_n: no reduction in flight on domain " +
                             std::to_string(dom));
  if (sc.values != n)
    throw std::runtime_error("reduction_end_n: the reduction in flight on domain " +
                             std::to_string(dom) + " has " + std::to_string(sc.values) +
                             " values, not " + std::to_string(n));
  sc.pending = false;
  sc.values = 1; // what the one-valued ops leave untouched
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

void field_sum_begin(ExchangeEngine &eng, int dom, int64_t a, bool aNext, const Rect3 &region,
                     int streamId) {
  const Launch l = plan_launch("field_sum", eng, dom, {{a, aNext}}, region);
  ExchangeEngine::ReduceScratch &sc = begin_reduction("field_sum", eng, dom, !l.empty);
  if (l.empty) return land_empty_n(sc, 1);
  STENCIL_HIP(hipSetDevice(l.d->gpu()));
  hipStream_t stream = eng.compute_stream(dom, streamId);
  if (l.es == 4)
    VEC_OPS_LAUNCH(float, l, sum_kernel, stream, l.g, (const char *)l.ptr[0], sc.dev);
  else
    VEC_OPS_LAUNCH(double, l, sum_kernel, stream, l.g, (const char *)l.ptr[0], sc.dev);
  land_partials_n(sc, l.blocks, 1, stream);
}

void field_dot_sums_begin(ExchangeEngine &eng, int dom, int64_t a, bool aNext, int64_t b,
                          bool bNext, const Rect3 &region, int streamId) {
  const Launch l = plan_launch("field_dot_sums", eng, dom, {{a, aNext}, {b, bNext}}, region);
  ExchangeEngine::ReduceScratch &sc = begin_reduction("field_dot_sums", eng, dom, !l.empty);
  if (l.empty) return land_empty_n(sc, 3);
  STENCIL_HIP(hipSetDevice(l.d->gpu()));
  hipStream_t stream = eng.compute_stream(dom, streamId);
  if (l.es == 4)
    VEC_OPS_LAUNCH(float, l, dot_sums_kernel, stream, l.g, (const char *)l.ptr[0],
                   (const char *)l.ptr[1], sc.dev);
  else
    VEC_OPS_LAUNCH(double, l, dot_sums_kernel, stream, l.g, (const char *)l.ptr[0],
                   (const char *)l.ptr[1], sc.dev);
  land_partials_n(sc, l.blocks, 3, stream);
}

void cg_update_sum_begin(ExchangeEngine &eng, int dom, double alpha, int64_t x, int64_t p,
                         int64_t r, const Rect3 &region, int streamId) {
  // operands: curr[x], curr[p], next[p] (= A p), curr[r]
  const Launch l = plan_launch("cg_update_sum", eng, dom,
                               {{x, false}, {p, false}, {p, true}, {r, false}}, region);
  if (x == p || x == r || p == r)
    throw std::invalid_argument("cg_update_sum: x, p and r must be distinct quantities");
  ExchangeEngine::ReduceScratch &sc = begin_reduction("cg_update_sum", eng, dom, !l.empty);
  if (l.empty) return land_empty_n(sc, 2);
  STENCIL_HIP(hipSetDevice(l.d->gpu()));
  hipStream_t stream = eng.compute_stream(dom, streamId);
  if (l.es == 4) {
    const float al = (float)alpha; // the one rounding to the quantity's type
    VEC_OPS_LAUNCH(float, l, cg_update_sum_kernel, stream, l.g, l.ptr[0], (const char *)l.ptr[1],
                   (const char *)l.ptr[2], l.ptr[3], al, sc.dev);
  } else {
    VEC_OPS_LAUNCH(double, l, cg_update_sum_kernel, stream, l.g, l.ptr[0],
                   (const char *)l.ptr[1], (const char *)l.ptr[2], l.ptr[3], alpha, sc.dev);
  }
  land_partials_n(sc, l.blocks, 2, stream);
}

double field_sum(ExchangeEngine &eng, int dom, int64_t a, bool aNext, const Rect3 &region,
                 int streamId) {
  field_sum_begin(eng, dom, a, aNext, region, streamId);
  double out[1];
  reduction_end_n(eng, dom, out, 1);
  return out[0];
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

void field_axpbyc(ExchangeEngine &eng, int dom, double alpha, int64_t x, bool xNext, double beta,
                  int64_t y, bool yNext, double c, int64_t out, bool outNext,
                  const Rect3 &region, int streamId) {
  const Launch l =
      plan_launch("field_axpbyc", eng, dom, {{x, xNext}, {y, yNext}, {out, outNext}}, region);
  if (l.empty) return;
  STENCIL_HIP(hipSetDevice(l.d->gpu()));
  hipStream_t stream = eng.compute_stream(dom, streamId);
  if (l.es == 4) {
    const float al = (float)alpha, be = (float)beta, cc = (float)c; // rounded once
    VEC_OPS_LAUNCH(float, l, axpbyc_kernel, stream, l.g, (const char *)l.ptr[0],
                   (const char *)l.ptr[1], l.ptr[2], al, be, cc);
  } else {
    VEC_OPS_LAUNCH(double, l, axpbyc_kernel, stream, l.g, (const char *)l.ptr[0],
                   (const char *)l.ptr[1], l.ptr[2], alpha, beta, c);
  }
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

void field_axpby(ExchangeEngine &eng, int dom, double alpha, int64_t x, bool xNext, double beta,
                 int64_t y, bool yNext, int64_t out, bool outNext, const Rect3 &region,
                 int streamId) {
  const Launch l =
      plan_launch("field_axpby", eng, dom, {{x, xNext}, {y, yNext}, {out, outNext}}, region);
  if (l.empty) return;
  STENCIL_HIP(hipSetDevice(l.d->gpu()));
  hipStream_t stream = eng.compute_stream(dom, streamId);
  if (l.es == 4) {
    const float al = (float)alpha, be = (float)beta; // the one rounding to the quantity's type
    VEC_OPS_LAUNCH(float, l, axpby_kernel, stream, l.g, (const char *)l.ptr[0],
                   (const char *)l.ptr[1], l.ptr[2], al, be);
  } else {
    VEC_OPS_LAUNCH(double, l, axpby_kernel, stream, l.g, (const char *)l.ptr[0],
                   (const char *)l.ptr[1], l.ptr[2], alpha, beta);
  }
}

void field_axpbypcz(ExchangeEngine &eng, int dom, double alpha, int64_t x, bool xNext,
                    double beta, int64_t y, bool yNext, double gamma, int64_t z, bool zNext,
                    int64_t out, bool outNext, const Rect3 &region, int streamId) {
  const Launch l = plan_launch("field_axpbypcz", eng, dom,
                               {{x, xNext}, {y, yNext}, {z, zNext}, {out, outNext}}, region);
  if (l.empty) return;
  STENCIL_HIP(hipSetDevice(l.d->gpu()));
  hipStream_t stream = eng.compute_stream(dom, streamId);
  if (l.es == 4) {
    const float al = (float)alpha, be = (float)beta, ga = (float)gamma; // rounded once
    VEC_OPS_LAUNCH(float, l, axpbypcz_kernel, stream, l.g, (const char *)l.ptr[0],
                   (const char *)l.ptr[1], (const char *)l.ptr[2], l.ptr[3], al, be, ga);
  } else {
    VEC_OPS_LAUNCH(double, l, axpbypcz_kernel, stream, l.g, (const char *)l.ptr[0],
                   (const char *)l.ptr[1], (const char *)l.ptr[2], l.ptr[3], alpha, beta, gamma);
  }
}

void field_scaled_update(ExchangeEngine &eng, int dom, double alpha, int64_t x, bool xNext,
                         int64_t d, bool dNext, double beta, int64_t y, bool yNext, double gamma,
                         int64_t z, bool zNext, int64_t out, bool outNext, const Rect3 &region,
                         int streamId) {
  const Launch l =
      plan_launch("field_scaled_update", eng, dom,
                  {{x, xNext}, {d, dNext}, {y, yNext}, {z, zNext}, {out, outNext}}, region);
  if (l.empty) return;
  STENCIL_HIP(hipSetDevice(l.d->gpu()));
  hipStream_t stream = eng.compute_stream(dom, streamId);
  if (l.es == 4) {
    const float al = (float)alpha, be = (float)beta, ga = (float)gamma; // rounded once
    VEC_OPS_LAUNCH(float, l, scaled_update_kernel, stream, l.g, (const char *)l.ptr[0],
                   (const char *)l.ptr[1], (const char *)l.ptr[2], (const char *)l.ptr[3],
                   l.ptr[4], al, be, ga);
  } else {
    VEC_OPS_LAUNCH(double, l, scaled_update_kernel, stream, l.g, (const char *)l.ptr[0],
                   (const char *)l.ptr[1], (const char *)l.ptr[2], (const char *)l.ptr[3],
                   l.ptr[4], alpha, beta, gamma);
  }
}

} // namespace stencil_amd
