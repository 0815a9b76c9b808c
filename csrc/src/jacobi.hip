// Jacobi-3D 7-point stencil kernels for gfx950 (the flagship app workload;
// reference: bin/jacobi3d.cu:18-85).
//
// The kernel is HBM-bandwidth-bound: per cell it reads the 6 face neighbors
// + writes one value; with y/z-neighbor rows served from L2/L3 the traffic
// floor is 4 B read + 4 B write per cell (PMC-verified: 1.64 GB fetched /
// 1.75 GB written per 750^3 step, profiles/jacobi_750_*_size.csv).
// Design choices for CDNA4, each A/B-measured via examples/jacobi_probe:
//   - float4 x-strips marching z with register-rolled center planes,
//     nontemporal stores (plain stores 9% slower),
//   - jacobi_kernel_v4_lds (the vecAll/graph path): y-neighbor rows
//     staged through 12 KB of ping-pong LDS, full 8 waves/SIMD — runs at
//     the mapping's copy roofline (540 Gcell/s @750^3),
//   - pure-vector full-rect launches (tail lanes cost 10%) with
//     address-based 16 B alignment,
//   - linearized scalar kernel for thin exterior slabs (any shape stays
//     coalesced), grid-stride with a capped grid,
//   - single-domain fully periodic runs (the bench shape): the whole-step
//     graph is jacobi_kernel_v4_lds<ZC, true> alone. It reads periodic
//     neighbours from the far side of the same buffer, so the per-step
//     halo copy (copy_batch, 59 us for 13.5 MB of strided faces) and the
//     in-graph table swap (4 us) are gone; the kernel itself costs 8 us
//     more (698 vs 689 us at 750^3). 0.714 vs 0.774 ms/step, median of 5
//     alternating runs (profiles/README.md). Halos are stale after steps
//     on this path until the next exchange(). STENCIL_JAC_WRAP=0 restores
//     the translate graph.
//   - the same runs, two steps at a time: run(n >= 2) replays
//     jacobi_kernel_fuse2, which reads time t and writes time t+2 with the
//     t+1 values held in LDS and registers only, so the field crosses HBM
//     once per two steps (the single-step kernel already streams within a
//     few percent of its copy roofline; the round trip between two steps
//     was the traffic left to remove). An odd n ends with one single step,
//     step() stays the single-step kernel. Its division is the 3-instruction
//     div6 of device_util.hpp, bit for bit the IEEE quotient; the
//     single-step kernels keep `/ 6.0f` (no measurable difference there:
//     they wait on memory at 8 waves/SIMD). 0.531 vs 0.722 ms/step, median
//     of 5 alternating runs (profiles/README.md). Its x neighbours come from
//     the neighbouring lanes' registers and everything from outside a tile
//     from one gathered load per wave and plane, on scalar bases with 32-bit
//     lane offsets: 78 instead of 122 VGPRs, a third block per CU, 0.393 vs
//     0.531 ms/step. STENCIL_JAC_FUSE2=0 forces single-step replays.
// Hot/cold sphere sources match the reference's behavior (truncated-int
// sqrtf distance, HOT=1/COLD=0 fixed cells) so results are comparable.
// What the kernels share is written once: the sphere rule (SpheresT), the
// scalar cell (scalar_cell), the six-neighbour sum in its fixed order with
// the periodic x-end selects (stencil_sum4, XEnds), and in device_util.hpp
// the nontemporal store, the lane shifts and the scalar-base addressing. On
// the host one function decides every launch (plan_jacobi -> JacobiLaunch)
// and one launches it (enqueue); the levers are in JacobiTuning.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#include "stencil_amd/device_util.hpp"
#include "stencil_amd/domain.hpp"
#include "stencil_amd/engine.hpp"
#include "stencil_amd/field_op.hpp"
#include "stencil_amd/hip_check.hpp"
#include "stencil_amd/jacobi_fuse2_map.hpp"
#include "stencil_amd/ops.hpp"

namespace stencil_amd {

namespace {

struct JacobiParams {
  // raw base pointers passed per launch (kernarg pointers get global
  // address-space inference + SGPR preload; slot-indirected bases cost
  // ~18% on this kernel -- measured with the jacobi_probe prod variant)
  const char *src;
  char *dst;
  int64_t pitch, plane;       // byte strides (same for curr/next)
  // global coordinate of allocation element (0,0,0)
  int64_t allocX, allocY, allocZ;
  // region to compute, global coords
  int64_t loX, loY, loZ;
  int32_t extX, extY, extZ;
  int32_t vecAll; // 1 = pure-vector launch (see plan_jacobi)
  // whole compute region (for the hot/cold spheres)
  int64_t cLoX, cLoY, cLoZ, cHiX, cHiY, cHiZ;
};

// kernargs of the WRAP instantiation of jacobi_kernel_v4_lds: the true x
// region, before the vecAll row extension moved loX/extX. A struct of its
// own, so the other kernels' kernarg layout (and code) stays as it was.
struct JacobiWrapParams : JacobiParams {
  int64_t trueLoX;
  int32_t trueExtX;
};

// The hot and cold sphere sources, one rule for every kernel: a cell whose
// truncated-int sqrtf distance from (hotX, cY, cZ) is at most srad holds 1,
// else one that close to (coldX, cY, cZ) holds 0. The truncation must match
// the reference bit for bit. I = int32_t in the vector kernels (grids are far
// below 2^31 per axis), int64_t in the scalar cells, which accept any shape.
template <typename I> struct SpheresT {
  I hotX, coldX, cY, cZ, srad;
  __device__ __forceinline__ explicit SpheresT(const JacobiParams &p) {
    const I cw = (I)(p.cHiX - p.cLoX);
    hotX = (I)p.cLoX + cw / 3;
    coldX = (I)p.cLoX + cw * 2 / 3;
    cY = (I)(p.cLoY + p.cHiY) / 2;
    cZ = (I)(p.cLoZ + p.cHiZ) / 2;
    srad = cw / 10;
  }
  __device__ __forceinline__ I yz2(I gy, I gz) const {
    const I dy = gy - cY, dz = gz - cZ;
    return dy * dy + dz * dz;
  }
  // the per-cell test: true, and `out` set, for a source cell
  __device__ __forceinline__ bool cell(I gx, I yz2, float &out) const {
    const I dxh = gx - hotX, dxc = gx - coldX;
    const bool hot = (I)__fsqrt_rn((float)(dxh * dxh + yz2)) <= srad;
    const bool cold = (I)__fsqrt_rn((float)(dxc * dxc + yz2)) <= srad;
    out = hot ? 1.0f : cold ? 0.0f : out;
    return hot || cold;
  }
  __device__ __forceinline__ bool cell(I gx, I gy, I gz, float &out) const {
    return cell(gx, yz2(gy, gz), out);
  }
  // the 4 cells from gx on. The common case costs two int compares: with the
  // truncated-int sqrt only yz2 >= (r+1)^2 guarantees exclusion
  __device__ __forceinline__ void cells4(I gx, I gy, I gz, float4 &out) const {
    const I q = yz2(gy, gz);
    if (q >= (srad + 1) * (srad + 1)) return;
#pragma unroll
    for (int i = 0; i < 4; ++i) cell(gx + i, q, (&out.x)[i]);
  }
};
using Spheres = SpheresT<int32_t>;

// One cell of the scalar paths (jacobi_kernel, head / tail lanes of
// jacobi_kernel_v4): the sphere value or the stencil, then the store. rowC /
// rowD are the cell's row in src / dst, ax its index in the row.
__device__ __forceinline__ void scalar_cell(const JacobiParams &p, const SpheresT<int64_t> &sph,
                                            const char *rowC, char *rowD, int64_t ax, int64_t gx,
                                            int64_t gy, int64_t gz) {
  float out = 0.0f;
  if (!sph.cell(gx, gy, gz, out)) {
    const float px = *(const float *)(rowC + (ax + 1) * 4);
    const float mx = *(const float *)(rowC + (ax - 1) * 4);
    const float py = *(const float *)(rowC + p.pitch + ax * 4);
    const float my = *(const float *)(rowC - p.pitch + ax * 4);
    const float pz = *(const float *)(rowC + p.plane + ax * 4);
    const float mz = *(const float *)(rowC - p.plane + ax * 4);
    out = (px + mx + py + my + pz + mz) / 6.0f;
  }
  *(float *)(rowD + ax * 4) = out;
}

// The x ends of a row of float4 vectors: leftOff / rightOff are where a lane
// finds the scalars across the ends of its vector, in bytes from the vector;
// wl_k / wr_k tell that this scalar, not the component next to it, is the
// -x / +x neighbour of component k.
// WRAP = false: the scalars are the cells next to the vector in memory and
// nothing is selected: compile-time constants, no select instruction.
// WRAP = true (periodic rows under the vecAll row extension): the true first
// cell is component `under` of the row's first vector (lane u == 0), the true
// last cell, extended index `last`, component last & 3 of its last vector
// (lane u == body4 - 1). Those two lanes load the periodic image of the row's
// other end, and the one component whose in-vector neighbour is an overshoot
// cell takes it.
template <bool WRAP> struct XEnds;
template <> struct XEnds<false> {
  static constexpr int32_t leftOff = -4, rightOff = 16;
  static constexpr bool wl1 = false, wl2 = false, wl3 = false;
  static constexpr bool wr0 = false, wr1 = false, wr2 = false;
  __device__ __forceinline__ XEnds() {}
  __device__ __forceinline__ XEnds(const JacobiParams &, int32_t, int32_t) {}
};
template <> struct XEnds<true> {
  int32_t under, last;
  int32_t leftOff = -4, rightOff = 16;
  bool wl1, wl2, wl3, wr0, wr1, wr2;
  __device__ __forceinline__ XEnds(const JacobiWrapParams &p, int32_t u, int32_t body4) {
    under = (int32_t)(p.trueLoX - p.loX); // 0..3
    last = under + p.trueExtX - 1;        // in vector body4-1
    const int32_t lastC = last & 3;       // 3 - over
    const bool first = u == 0, lastLane = u == body4 - 1;
    if (first) leftOff = last * 4;                // row start + last
    if (lastLane) rightOff = (under - 4 * u) * 4; // row start + under
    wl1 = first && under == 1;
    wl2 = first && under == 2;
    wl3 = first && under == 3;
    wr0 = lastLane && lastC == 0;
    wr1 = lastLane && lastC == 1;
    wr2 = lastLane && lastC == 2;
  }
};

// The six-neighbour sums of one vector, in the order every kernel and the
// NumPy oracle sum in: +x -x +y -y +z -z. c is the vector's own plane (x
// neighbours inside), l / r the scalars across its ends. Callers divide.
template <bool WRAP>
__device__ __forceinline__ float4 stencil_sum4(const XEnds<WRAP> &e, const float4 &c, float l,
                                               float r, const float4 &py, const float4 &my,
                                               const float4 &pz, const float4 &mz) {
  float4 s;
  s.x = (e.wr0 ? r : c.y) + l + py.x + my.x + pz.x + mz.x;
  s.y = (e.wr1 ? r : c.z) + (e.wl1 ? l : c.x) + py.y + my.y + pz.y + mz.y;
  s.z = (e.wr2 ? r : c.w) + (e.wl2 ? l : c.y) + py.z + my.z + pz.z + mz.z;
  s.w = r + (e.wl3 ? l : c.z) + py.w + my.w + pz.w + mz.w;
  return s;
}
// the single-step kernels' division (fuse2 divides with div6)
__device__ __forceinline__ float4 over6(const float4 &s) {
  return make_float4(s.x / 6.0f, s.y / 6.0f, s.z / 6.0f, s.w / 6.0f);
}

// Vectorized z-marching kernel for wide regions: each thread owns a
// 4-wide x strip (16 B aligned) and marches ZCHUNK cells in z, keeping the
// z-1 / z / z+1 center vectors in registers so the +-z neighbor planes are
// never re-loaded. Per 4 cells and z step: 3 aligned float4 loads (new
// center plane + y neighbors) + 2 scalar edge loads + 1 float4 store
// (~14 B/cell issued vs 28 for the scalar kernel). The hot/cold sphere
// test short-circuits on a 1D bounding check so the common case costs two
// int compares.
#define JAC_ZCHUNK 16

__global__ void __launch_bounds__(256) jacobi_kernel_v4(JacobiParams p) {
  // (an XCD-aware block remap was measured 9% SLOWER here: the row
  // working set is L3-resident, so the remap only disturbed dispatch)
  const int32_t u = blockIdx.x * blockDim.x + threadIdx.x; // x unit
  const int32_t ly = blockIdx.y * blockDim.y + threadIdx.y;
  const int32_t lz0 = blockIdx.z * JAC_ZCHUNK;
  if (ly >= p.extY) return;
  const char *srcBase = p.src;
  char *dstBase = p.dst;
  const int64_t gy = p.loY + ly;
  const int64_t ay = gy - p.allocY;
  const int32_t zEnd = min((int32_t)(lz0 + JAC_ZCHUNK), p.extZ);

  const Spheres sph(p);
  const SpheresT<int64_t> sph64(p);
  const XEnds<false> ends;

  auto cell = [&](int32_t lx, int32_t lz) {
    const int64_t gx = p.loX + lx;
    const int64_t gz = p.loZ + lz;
    const int64_t row = (gz - p.allocZ) * p.plane + ay * p.pitch;
    scalar_cell(p, sph64, srcBase + row, dstBase + row, gx - p.allocX, gx, gy, gz);
  };

  const int64_t a0 = p.loX - p.allocX;
  // vecAll: host pre-adjusted loX/extX (16B-aligned start, extX%4==0;
  // the launcher's row_extension guarantees that writes beyond the true
  // region land only in same-row halo / local-rect cells, which the next
  // exchange or a later kernel rewrites before any read, or in pitch-slack
  // bytes where the row has them) -- no scalar lanes.
  // Otherwise head = elements until the next 16 B-aligned ADDRESS (the
  // allocation pad shifts the base, so index-aligned units would issue
  // misaligned dwordx4 -- measured ~10% on gfx950); must match the
  // launcher's units formula.
  const int32_t headAl =
      (int32_t)((16 - (((uintptr_t)srcBase + (uintptr_t)(a0 * 4)) & 15)) & 15) >> 2;
  const int32_t head = p.vecAll ? 0 : (headAl > p.extX ? p.extX : headAl);
  const int32_t body4 = (p.extX - head) / 4;
  const int32_t tail = p.extX - head - body4 * 4;

  if (u < body4) {
    const int64_t ax = a0 + head + (int64_t)u * 4; // 4-aligned
    const int32_t gx = (int32_t)(ax + p.allocX);
    const int64_t az0 = p.loZ + lz0 - p.allocZ;
    const char *col = srcBase + az0 * p.plane + ay * p.pitch + ax * 4;
    char *dcol = dstBase + az0 * p.plane + ay * p.pitch + ax * 4;
    // rolling center vectors
    float4 cm = *(const float4 *)(col - p.plane);
    float4 cc = *(const float4 *)(col);
    for (int32_t lz = lz0; lz < zEnd; ++lz) {
      const float4 cp = *(const float4 *)(col + p.plane);
      const float left = *(const float *)(col - 4);
      const float right = *(const float *)(col + 16);
      const float4 py = *(const float4 *)(col + p.pitch);
      const float4 my = *(const float4 *)(col - p.pitch);
      float4 out = over6(stencil_sum4(ends, cc, left, right, py, my, cp, cm));
      sph.cells4(gx, (int32_t)gy, (int32_t)(p.loZ + lz), out);
      store4(dcol, out); // next is write-only this iteration
      cm = cc;
      cc = cp;
      col += p.plane;
      dcol += p.plane;
    }
  } else if (u == body4) {
    // (spreading these cells over one-lane-per-z-plane measured 10%
    // SLOWER overall -- the extra block column cost more than the
    // straggler lane; keep the compact form)
    for (int32_t lz = lz0; lz < zEnd; ++lz)
      for (int32_t lx = 0; lx < head; ++lx) cell(lx, lz);
  } else if (u == body4 + 1) {
    for (int32_t lz = lz0; lz < zEnd; ++lz)
      for (int32_t lx = p.extX - tail; lx < p.extX; ++lx) cell(lx, lz);
  }
}

// vecAll-only variant: y-neighbor rows staged through LDS. A 64x4 block
// marching z keeps the current plane's center vectors of its 4 rows + 2
// y-halo rows in ping-pong LDS buffers (one barrier per z-step), so the
// py/my global vector loads become LDS reads. Probe: 0.749 ms vs 0.839
// for the pure-global stencil at 752^3 -- at the mapping's copy roofline
// (examples/jacobi_probe.cpp full-ldsrows). Requires blockDim (64,4,1)
// and a vecAll launch (no scalar lanes; every lane's row exists because
// the region is the interior rect of a radius>=1 domain).
//
// WRAP = true (single-domain fully periodic whole-step graph, see
// jacobi_graph_create): the region is the whole domain and periodic on all
// three axes, so every neighbour outside [lo, lo+ext) is read from the far
// end of the same buffer instead of from a halo cell. No halo is read, so
// none has to be filled before the step. z: the -z plane of plane 0 is
// plane extZ-1 and the +z plane of plane extZ-1 is plane 0 (uniform per
// block / per iteration). y: the row staged below row 0 is row extY-1, the
// row staged above row extY-1 is row 0 (uniform per block; lanes past extY
// stage row 0, because the valid lane below reads their row as its +y
// neighbour). x: the vecAll extension puts the true first cell at
// component `under` of a row's first vector and the true last cell at
// component 3-`over` of its last vector; the first lane loads `left` from
// the row's last true cell, the last lane loads `right` from its first, and
// a per-lane select feeds that scalar to the one component whose in-vector
// neighbour is an overshoot cell. Overshoot components still compute and
// store garbage. The launcher only extends a row when every overshoot cell
// is an x-halo cell or a pitch-slack byte of that row (row_extension), which
// nothing on this path reads; a row without that room never gets here
// (plan_jacobi plans no WrapStep for it).
// gfx950 resource usage (-Rpass-analysis=kernel-resource-usage), the same
// for ZC = 16 and 32:
//   WRAP=false: 58 VGPRs, 54 SGPRs, 0 scratch, 8 waves/SIMD, 12288 B LDS
//   WRAP=true : 60 VGPRs, 58 SGPRs, 0 scratch, 8 waves/SIMD, 12288 B LDS
// (the row/plane selects and the six x-select lane masks live in scalar
// registers; WRAP=false has no select for the x ends, see XEnds)
template <int ZC, bool WRAP = false>
__global__ void __launch_bounds__(256)
jacobi_kernel_v4_lds(std::conditional_t<WRAP, JacobiWrapParams, JacobiParams> p) {
  __shared__ float4 tile[2][6][64];
  const int32_t tx = threadIdx.x;
  const int32_t ry = threadIdx.y;
  // no early returns (__syncthreads needs every lane): out-of-range lanes
  // clamp coordinates and skip only the store
  const int32_t u0 = blockIdx.x * 64 + tx;
  const int32_t ly0 = blockIdx.y * 4 + ry;
  const int32_t body4 = p.extX / 4; // vecAll: extX % 4 == 0
  const bool valid = u0 < body4 && ly0 < p.extY;
  const int32_t u = min(u0, body4 - 1);
  // clamp to extY (the +y halo row, which exists for radius >= 1): a
  // VALID lane ry-1 reads lane ry's staged row as its +y neighbor, so
  // lanes at ly0 == extY must stage the TRUE halo row, not a duplicate.
  // WRAP: that neighbour is row 0.
  const int32_t ly = WRAP ? (ly0 < p.extY ? ly0 : 0) : min(ly0, (int32_t)p.extY);
  const int32_t lz0 = blockIdx.z * ZC;
  const int32_t zEnd = min((int32_t)(lz0 + ZC), p.extZ);
  // byte offsets from a lane's own cell to the rows/planes it stages:
  //   myHalo: -y row staged by ry==0      pyHalo: +y row staged by ry==3
  //   mzOff : the initial -z plane        (+z plane: pzOff, in the loop)
  int64_t myHalo = -p.pitch, pyHalo, mzOff = -p.plane;
  if constexpr (WRAP) {
    // all three depend on blockIdx only: scalar registers
    const int32_t by0 = blockIdx.y * 4, by3 = by0 + 3;
    const int64_t ySpan = (int64_t)(p.extY - 1) * p.pitch;
    if (by0 == 0) myHalo = ySpan;
    // ry==3 at the last row wraps down to row 0; past it the lane already
    // sits on row 0 and any in-range row will do
    pyHalo = by3 < p.extY - 1 ? p.pitch : (by3 == p.extY - 1 ? -ySpan : 0);
    if (lz0 == 0) mzOff = (int64_t)(p.extZ - 1) * p.plane;
  } else {
    // one past its own row, clamped in-bounds
    pyHalo = (ly < p.extY) ? p.pitch : 0;
  }

  const int64_t gy = p.loY + ly;
  const int64_t ay = gy - p.allocY;
  const int64_t a0 = p.loX - p.allocX;
  const int64_t ax = a0 + (int64_t)u * 4;
  const int32_t gx = (int32_t)(ax + p.allocX);
  const int64_t az0 = p.loZ + lz0 - p.allocZ;
  const char *col = p.src + az0 * p.plane + ay * p.pitch + ax * 4;
  char *dcol = p.dst + az0 * p.plane + ay * p.pitch + ax * 4;

  const Spheres sph(p);
  const XEnds<WRAP> ends(p, u, body4);

  float4 cm = *(const float4 *)(col + mzOff);
  float4 cc = *(const float4 *)(col);
  tile[0][ry + 1][tx] = cc;
  if (ry == 0) tile[0][0][tx] = *(const float4 *)(col + myHalo);
  if (ry == 3) tile[0][5][tx] = *(const float4 *)(col + pyHalo);
  __syncthreads();
  int buf = 0;
  for (int32_t lz = lz0; lz < zEnd; ++lz) {
    // +z plane (WRAP: plane 0 after the last one, uniform per iteration) and
    // the -y row in it
    const int64_t pzOff =
        WRAP && lz == p.extZ - 1 ? -(int64_t)(p.extZ - 1) * p.plane : p.plane;
    const char *colP = col + pzOff, *colPmy = colP + myHalo;
    const float left = *(const float *)(col + ends.leftOff);
    const float right = *(const float *)(col + ends.rightOff);
    const float4 cp = *(const float4 *)colP;
    const float4 py = tile[buf][ry + 2][tx];
    const float4 my = tile[buf][ry][tx];
    float4 out = over6(stencil_sum4(ends, cc, left, right, py, my, cp, cm));
    sph.cells4(gx, (int32_t)gy, (int32_t)(p.loZ + lz), out);
    if (valid) store4(dcol, out);

    tile[buf ^ 1][ry + 1][tx] = cp;
    if (ry == 0) tile[buf ^ 1][0][tx] = *(const float4 *)colPmy;
    if (ry == 3) tile[buf ^ 1][5][tx] = *(const float4 *)(colP + pyHalo);
    __syncthreads();
    buf ^= 1;
    cm = cc;
    cc = cp;
    col += p.plane;
    dcol += p.plane;
  }
}

// Two time steps in one pass over memory, for the same launch the WRAP
// kernel above serves (whole domain, periodic on every axis, vecAll row
// extension): reads `src` at time t, writes time t+2 into `dst`; the t+1
// values exist only in LDS and registers, so the field makes one trip
// through HBM per TWO steps.
//
// Tiling: a 64 x NY block marches z. A wave is one row of the block: lane
// (tx, ry) owns the float4 at vector blockIdx.x*64+tx of row
// blockIdx.y*(NY-2)-1+ry, and everything that depends on the row alone (ry
// is read through readfirstlane) is scalar. Every lane computes stage 1
// (time t+1) of its vector, the inner NY-2 rows also compute stage 2 (time
// t+2) and store it: 2 of NY rows are redundant stage-1 work (25% at NY =
// 8), and there is NO x halo lane.
//   y: stage 1 reads the t rows above and below from tT (NY+2 rows: the
//      block's own, plus one halo row staged by ry==0 and one by ry==NY-1),
//      stage 2 reads the t+1 rows above and below from tS (NY rows). Both
//      are ping-pong pairs, one barrier per plane: a plane's reads all
//      precede the barrier after which the other half is overwritten.
//   z: the t planes z-1, z, z+1 and the t+1 planes z-2, z-1, z roll in
//      registers; iteration z computes stage 1 of plane z and stage 2 of
//      plane z-1. A block owns a chunk of planes [lz0, zEnd) and runs the
//      loop over lz0-1 .. zEnd: 2 extra stage-1 planes and 4 extra t planes
//      per chunk. Vector loads (own vector and halo row) run two planes
//      ahead of their use, the gathered load one (see the loop).
//   x: inside a vector the neighbours are components; across vectors they
//      are the neighbouring LANES' registers at both stages (cc / sc of lane
//      tx-1 and tx+1, one lane shift each): no load and no LDS read. Only
//      the two lanes at a tile's x edges need a value from outside the wave.
//      There the neighbour belongs to another block (or, at a row's end, is
//      the periodic image of the row's other end): edge cells eL and eR. At
//      stage 1 the edge lanes take the t values of eL / eR; at stage 2 they
//      need the t+1 values, which lanes 0 and 1 of each wave compute
//      themselves from the six t neighbours of eL / eR. All of that arrives
//      by ONE gathered global_load_dword per wave and plane (ten lanes
//      useful, table in jacobi_fuse2_map.hpp): the t values of e and of its
//      four x / y neighbours in the plane after stage 1's. The z neighbours
//      of e are e itself one plane later and earlier, so the last three
//      gathered registers are kept (g1, g2, g3) and lanes 0 / 1 sum
//      their six operands with row shifts, in the order every other cell
//      is summed in.
// Addresses: every load and the store is a wave-uniform 64-bit base (buffer
// + row + plane, scalar unit) plus a 32-bit lane offset that never changes
// (the global saddr + voffset form); the gathered offset is below the plane
// stride, which plan_jacobi bounds to 31 bits.
// Periodic wrap is a true modulo on every axis (rows and planes by index,
// x by the row's true first/last cell), so extents down to x=8, y=1, z=1
// are exact; the sphere override runs after each stage at the WRAPPED
// global coordinate of the cell it produced. Overshoot components of a
// row's first/last vector hold garbage at both stages and are stored, like
// the WRAP kernel's, only into cells row_extension mode 1 permits; no true
// cell ever reads one (the wl*/wr* selects replace exactly those
// neighbours, and a lane shift across vectors only ever delivers component
// 3 of a row's first or component 0 of its last vector, both true cells).
// Lanes past a row's last vector (tx > rl) hold garbage that no other lane
// reads: lane rl takes its right neighbours from the gathered values. No
// halo cell is read. No lane returns before a barrier: out-of-range lanes
// clamp or wrap their coordinates and skip the store.
// The division is div6 (device_util.hpp): 3 instructions per value instead
// of the IEEE expansion's 11, the same bits.
// gfx950 resource usage (-Rpass-analysis=kernel-resource-usage), NY = 8:
//   76 VGPRs, 84 SGPRs, 0 scratch, 6 waves/SIMD, 36864 B LDS: three blocks
//   (24 waves) per CU, bound by the VGPRs (80 is the most for 6 waves/SIMD;
//   78 / 78 while the sphere test was branches, now it is selects).
//   Before the lane shifts and the gathered load: 122 VGPRs, 82 SGPRs, two
//   blocks per CU.
// The loop body, two planes, every block of it counted (the IEEE-division
// fallback of div6 and the sphere tests included), before -> now:
//   global_load_dword 16 -> 2, global_load_dwordx4 4 -> 4, stores 2 -> 2,
//   ds_read 12 -> 8 (b128 only), ds_write_b128 6 -> 6, ds_bpermute 2 -> 0,
//   v_mad_u64_u32 12 -> 0, v_lshl_add_u64 14 -> 0, v_mov_b64 38 -> 26,
//   v_mov_b32 34 -> 72 (the lane shifts' operands and results among them),
//   v_mov_b32_dpp 0 -> 18, v_readlane_b32 0 -> 6. Every global access has the
//   saddr + voffset form. The load queue is still drained once per two
//   planes at the loop latch, where the register slots are copied.
//   (Since the sphere test is the shared select form instead of a branch per
//   cell the body is 941 instead of 1012 instructions, fewer moves among
//   them; every memory, LDS, DPP and readlane count above is unchanged.)
// Measured at 750^3 (profiles/README.md, "Fused two-step jacobi graph").
template <int NY>
__global__ void __launch_bounds__(64 * NY) jacobi_kernel_fuse2(JacobiWrapParams p) {
  __shared__ float4 tT[2][NY + 2][64];
  __shared__ float4 tS[2][NY][64];
  const int32_t tx = threadIdx.x;
  // blockDim.x is the wave size, so threadIdx.y is the same in all 64 lanes
  const int32_t ry = __builtin_amdgcn_readfirstlane((int32_t)threadIdx.y);
  const int32_t body4 = p.extX / 4; // vecAll: extX % 4 == 0
  const int32_t ub = blockIdx.x * 64;
  const int32_t u0 = ub + tx;
  const int32_t u = min(u0, body4 - 1);
  // rows: unwrapped yb, and the wrapped rows the wave touches
  const int32_t yb = (int32_t)blockIdx.y * (NY - 2) - 1 + ry;
  const int32_t yo = f2_pmod(yb, p.extY), ym = f2_pmod(yb - 1, p.extY),
                yp = f2_pmod(yb + 1, p.extY);
  const bool valid = u0 < body4 && ry >= 1 && ry <= NY - 2 && yb < p.extY;
  // planes: the chunk is derived from the grid, so the launcher alone
  // decides its length
  const int32_t zc = (p.extZ + (int32_t)gridDim.z - 1) / (int32_t)gridDim.z;
  const int32_t lz0 = blockIdx.z * zc;
  const int32_t zEnd = min(lz0 + zc, p.extZ);

  // cell (extended index 0, row 0, plane 0) of both buffers, and from there
  // the wave's rows: its own, and the halo row it stages into tT (ry == 0:
  // below, ry == NY-1: above; the other waves re-read their own)
  const int64_t a0 = p.loX - p.allocX;
  const int64_t org = (p.loZ - p.allocZ) * p.plane + (p.loY - p.allocY) * p.pitch + a0 * 4;
  const bool stagesHalo = ry == 0 || ry == NY - 1;
  const int32_t hrow = ry == 0 ? 0 : NY + 1;
  const char *src0 = p.src + org;
  const char *srcO = src0 + (int64_t)yo * p.pitch;
  const char *srcH = src0 + (int64_t)(ry == 0 ? ym : ry == NY - 1 ? yp : yo) * p.pitch;
  char *dstO = p.dst + org + (int64_t)yo * p.pitch;
  const uint32_t voff = (uint32_t)u * 16u; // the lane's vector within a row
  const int32_t gx = (int32_t)p.loX + u * 4;
  const int32_t gy = (int32_t)p.loY + yo;

  const Spheres sph(p);
  // x wrap of the row's true end cells: extended index ends.under is the
  // first true cell, ends.last the last one
  const XEnds<true> ends(p, u, body4);

  // tile x edges (uniform per block): rl is the last lane that holds a
  // vector of its own; eL / eR are the extended indices of the true cells
  // just outside the tile, wrapped at the row's ends. Lane 0 computes the
  // t+1 value of eL, lane 1 that of eR.
  const int32_t rl = min(63, body4 - 1 - ub);
  const int32_t eL = f2_edge_left(ub, ends.last), eR = f2_edge_right(ub, body4, ends.under);
  const int32_t gxE = (int32_t)p.loX + (tx == 0 ? eL : eR);
  const bool rightEdge = tx >= rl;
  // the lane's scalar of the gathered load, from cell 0 of row 0 of a plane
  const uint32_t goff =
      f2_gather_offset(tx, eL, eR, ends.under, ends.last, yo, ym, yp, (uint32_t)p.pitch);

  // wrapped plane indices of the rolling window: i0 is the plane stage 1
  // produces this iteration, iP3 the plane requested in it
  int32_t iM1 = f2_pmod(lz0 - 2, p.extZ), i0 = f2_pmod(lz0 - 1, p.extZ);
  int32_t iP1 = f2_pmod(lz0, p.extZ), iP2 = f2_pmod(lz0 + 1, p.extZ),
          iP3 = f2_pmod(lz0 + 2, p.extZ);
  // The plane index is uniform, so row + plane is a scalar base
  // (global_base) and the lane adds 32 bits.
  auto zoff = [&](int32_t i) { return (int64_t)i * p.plane; };
  auto ld4 = [&](const char *row, int32_t i) {
    const vfloat4 v = *(const __attribute__((address_space(1))) vfloat4 *)(
        global_base(row + zoff(i)) + lane_offset(voff));
    return make_float4(v.x, v.y, v.z, v.w);
  };
  auto gather = [&](int32_t i) {
    return *(const __attribute__((address_space(1))) float *)(global_base(src0 + zoff(i)) +
                                                              lane_offset(goff));
  };

  // Vector loads run TWO planes ahead of their use (one plane per wave in
  // flight cannot cover HBM latency at 4 waves/SIMD): plane zz+1 and zz+2
  // sit in the slot pairs (vA, hA) / (vB, hB), which alternate per iteration.
  // The loop is unrolled by two so that a slot is a fixed register set that
  // a load writes directly; copying an in-flight slot would wait for it.
  // (The compiler still copies the slots at the loop latch and drains the
  // load queue there once per two planes. A variant without that drain,
  // every wait in the loop partial, measured the same step time, 0.532 vs
  // 0.532 ms in alternating runs: not kept.)
  float4 cm = ld4(srcO, iM1);
  float4 cc = ld4(srcO, i0);
  // gathered registers: g1 holds plane i0, g2 plane i0-1, g3 plane i0-2.
  // Stage 1 needs g1 from the first iteration on; the first stage 2 (third
  // iteration) needs g3 of plane lz0-1, which is this load, g2 of plane lz0
  // and g1 of plane lz0+1, gathered in the first two iterations.
  float g1 = gather(i0), g2 = g1, g3 = g1;
  tT[0][ry + 1][tx] = cc;
  if (stagesHalo) tT[0][hrow][tx] = ld4(srcH, i0);
  float4 vA = ld4(srcO, iP1), hA = ld4(srcH, iP1);
  float4 vB = ld4(srcO, iP2), hB = ld4(srcH, iP2);
  float4 sm = make_float4(0.f, 0.f, 0.f, 0.f), sc = sm;
  __syncthreads();
  int tb = 0, sb = 0;
  // one plane: v / h hold plane zz+1 on entry and are re-requested with
  // plane zz+3
  auto iteration = [&](int32_t zz, float4 &v, float4 &h) {
    const float4 cp = v, hp = h;
    // Requests, every lane and wave alike (a wait counts loads in issue
    // order, and only straight-line code lets the compiler count exactly).
    // First what the NEXT iteration needs, in a plane already requested:
    // the gathered scalars of plane zz+1.
    const float gn = gather(iP1);
    // then plane zz+3, last: a wait for the scalars above leaves it in flight
    // (waves that stage no halo row re-read their own vector)
    v = ld4(srcO, iP3);
    h = ld4(srcH, iP3);

    // stage 1: time t+1 of plane zz. x neighbours across vectors: the
    // neighbouring lanes' cc, at the tile's edges the t values of eL / eR
    const float tL = lane_value(g1, F2_GATHER_SELF), tR = lane_value(g1, F2_GATHER_SELF + 1);
    // (shifts first, selects after: a shift inside a branch of the select
    // would run with the edge lanes switched off and miss their values)
    const float l = lane_below(cc.w, tL);
    const float ra = lane_above(cc.x);
    const float r = rightEdge ? tR : ra;
    float4 s = div6(stencil_sum4(ends, cc, l, r, tT[tb][ry + 2][tx], tT[tb][ry][tx], cp, cm));
    sph.cells4(gx, gy, (int32_t)p.loZ + i0, s);

    // stage 2: time t+2 of plane zz-1, from the t+1 planes zz-2 (sm),
    // zz-1 (sc, tS[sb^1]) and zz (s)
    if (zz > lz0) {
      // lanes 0 / 1: the six t neighbours of eL / eR in plane zz-1, summed
      // +x -x +y -y +z -z (all lanes run the shifts, two keep the result)
      const float e6 = ((((g2 + row_above<2>(g2)) + row_above<4>(g2)) + row_above<6>(g2)) +
                        row_above<F2_GATHER_SELF>(g1)) +
                       row_above<F2_GATHER_SELF>(g3);
      float e1 = 0.f;
      if (tx < 2) {
        e1 = div6(e6);
        sph.cell(gxE, gy, (int32_t)p.loZ + iM1, e1);
      }
      const float eRight = lane_value(e1, 1);
      const float l2 = lane_below(sc.w, e1);
      const float ra2 = lane_above(sc.x);
      const float r2 = rightEdge ? eRight : ra2;
      float4 out = div6(stencil_sum4(ends, sc, l2, r2, tS[sb ^ 1][min(ry + 1, NY - 1)][tx],
                                     tS[sb ^ 1][max(ry - 1, 0)][tx], s, sm));
      sph.cells4(gx, gy, (int32_t)p.loZ + iM1, out);
      if (valid) store4(global_base(dstO + zoff(iM1)) + lane_offset(voff), out);
    }

    tS[sb][ry][tx] = s;
    tT[tb ^ 1][ry + 1][tx] = cp;
    if (stagesHalo) tT[tb ^ 1][hrow][tx] = hp;
    __syncthreads();
    tb ^= 1;
    sb ^= 1;
    cm = cc;
    cc = cp;
    sm = sc;
    sc = s;
    g3 = g2;
    g2 = g1;
    g1 = gn;
    iM1 = i0;
    i0 = iP1;
    iP1 = iP2;
    iP2 = iP3;
    iP3 = iP3 + 1 == p.extZ ? 0 : iP3 + 1;
  };
  // planes lz0-1 .. zEnd: the count is uniform per block, so is the branch
  for (int32_t zz = lz0 - 1; zz <= zEnd; zz += 2) {
    iteration(zz, vA, hA);
    if (zz + 1 <= zEnd) iteration(zz + 1, vB, hB);
  }
}

__global__ void jacobi_kernel(JacobiParams p) {
  const char *srcBase = p.src;
  char *dstBase = p.dst;
  const SpheresT<int64_t> sph(p);
  const int64_t total = (int64_t)p.extX * p.extY * p.extZ;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int32_t lx = (int32_t)(i % p.extX);
    const int64_t t = i / p.extX;
    const int32_t ly = (int32_t)(t % p.extY);
    const int32_t lz = (int32_t)(t / p.extY);
    // global coords
    const int64_t gx = p.loX + lx, gy = p.loY + ly, gz = p.loZ + lz;
    // allocation-local element coords
    const int64_t ax = gx - p.allocX, ay = gy - p.allocY, az = gz - p.allocZ;
    const int64_t row = az * p.plane + ay * p.pitch;
    scalar_cell(p, sph, srcBase + row, dstBase + row, ax, gx, gy, gz);
  }
}

__global__ void fill_kernel(char *base, int64_t pitch, int64_t plane,
                            int32_t extX, int32_t extY, int32_t extZ, float value) {
  const int64_t total = (int64_t)extX * extY * extZ;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int32_t lx = (int32_t)(i % extX);
    const int64_t t = i / extX;
    const int32_t ly = (int32_t)(t % extY);
    const int64_t lz = t / extY;
    *(float *)(base + lz * plane + (int64_t)ly * pitch + (int64_t)lx * 4) = value;
  }
}

// The levers, all from the environment. The tuning values are read once per
// process. The two path switches are the A/B levers and the fallbacks: they
// are read at each graph creation, which is set-up and never on the step path.
struct JacobiTuning {
  bool lds = true;     // STENCIL_JAC_LDS=0 turns the LDS-rows kernel off
  int zc = 32;         // STENCIL_JAC_ZC=16: its planes per block (32 measured +1.8%)
  int bx = 64, by = 4; // STENCIL_JAC_BLOCK=<bx>x<by>, 256 threads: jacobi_kernel_v4's block
  int f2zc = 64;       // STENCIL_JAC_F2ZC=<n >= 1>: planes per block of the fused kernel

  static const JacobiTuning &get() {
    static const JacobiTuning tuning = [] {
      JacobiTuning t;
      t.lds = !is_zero("STENCIL_JAC_LDS");
      if (const char *e = getenv("STENCIL_JAC_ZC")) t.zc = atoi(e) == 16 ? 16 : 32;
      if (const char *e = getenv("STENCIL_JAC_BLOCK")) {
        int bx, by;
        if (sscanf(e, "%dx%d", &bx, &by) == 2 && bx * by == 256) t.bx = bx, t.by = by;
      }
      if (const char *e = getenv("STENCIL_JAC_F2ZC")) t.f2zc = atoi(e) >= 1 ? atoi(e) : 64;
      return t;
    }();
    return tuning;
  }
  // STENCIL_JAC_WRAP=0 forces the translate graph, STENCIL_JAC_FUSE2=0
  // single-step replays
  static bool wrap() { return !is_zero("STENCIL_JAC_WRAP"); }
  static bool fuse2() { return !is_zero("STENCIL_JAC_FUSE2"); }

private:
  static bool is_zero(const char *name) {
    const char *e = getenv(name);
    return e && e[0] == '0';
  }
};

// Argument check of every jacobi entry point, before anything is launched
// or captured: the kernels read a 1-cell apron around `region`, and all of
// it has to lie inside the allocation. An empty region is a no-op and valid.
LocalDomain &checked_jacobi_domain(ExchangeEngine &eng, int dom, int64_t qi, const char *name) {
  LocalDomain &d = checked_domain(name, eng, dom);
  checked_elem_size(name, d, {{qi, false}}, 4); // fp32
  return d;
}

void check_jacobi_region(const LocalDomain &d, const Rect3 &region, const char *name) {
  if (checked_extent(name, region)) check_inside(name, "region", region, d.full_region(), 1);
}

// Row extension of a pure-vector (vecAll) launch: the x range of `region`
// grown left by `under` cells to the previous 16 B-aligned ADDRESS and right
// by `over` cells to a multiple of 4, which removes the scalar head/tail
// lanes (the probe measured them at ~10% of the kernel). Returns false when
// the launch must stay as it is.
//   mode 1 (free): the extended cells are written with discardable values,
//     so each must be an x-halo cell or a local-rect cell of the SAME row,
//     or a pitch-slack byte. Rows are `pitch` apart and hold raw_size().x
//     cells: the extended range has to stay within [-slack, raw.x + slack)
//     of its own row, slack = pitch / 4 - raw.x. A row without slack
//     ((X + 2r) % 64 == 0) that would be overrun is NOT extended: the
//     overshoot would land in cells of the neighbouring rows, which other
//     lanes of the same launch (or nobody) own.
//   mode 2 (strict): no cell outside the region may be written; only a
//     region that is aligned already qualifies.
// Alignment is the same for both buffer parities (same pad, 256 B-aligned
// allocations), so the answer holds for every launch of the region.
bool row_extension(const LocalDomain &d, int64_t qi, const Rect3 &region, int mode,
                   int64_t &under, int64_t &over) {
  under = over = 0;
  const int64_t extX = region.extent().x;
  if (!mode || extX < 8) return false;
  const int64_t a0 = region.lo.x - d.full_region().lo.x;
  const uintptr_t addr0 = (uintptr_t)d.curr(qi).ptr + (uintptr_t)(a0 * 4);
  const int64_t u = (int64_t)((addr0 & 15) >> 2);
  const int64_t o = (4 - ((extX + u) & 3)) & 3;
  if (mode == 2) {
    if (u != 0 || o != 0) return false;
  } else {
    const int64_t rowCells = d.raw_size().x;
    const int64_t slack = d.curr(qi).pitch / 4 - rowCells;
    if (a0 - u < -slack || a0 + extX + o > rowCells + slack) return false;
  }
  under = u;
  over = o;
  return true;
}

// Rows per block of jacobi_kernel_fuse2 (6 of them useful). 8 rows are 8
// waves and 36 KB of LDS, so three blocks share a CU (two while the kernel
// held 122 VGPRs) and the others compute while one waits at its barrier; 14
// rows (12 useful, 14% instead of 25% redundant stage-1 rows, but one block
// per CU) measured 12% slower at 122 VGPRs.
constexpr int JAC_F2_NY = 8;

// One kernel launch, decided and parameterised: which kernel, its kernargs
// from the domain's CURRENT buffer parity (raw pointers: the whole-step
// graphs plan once and bake the pointers per parity, enqueue_current) and its
// launch shape.
struct JacobiLaunch {
  // None: nothing to launch (an empty region, or a Want that cannot be served)
  enum Kind { None, Scalar, Vec4, Lds, LdsWrap, Fuse2 };
  // Step: one step of any region. WrapStep / FusedPair: one / two steps of a
  // whole domain that is periodic on every axis, neighbours read from the far
  // side of the buffer (the caller vouches for the geometry); only ever the
  // LdsWrap / Fuse2 kernel.
  enum Want { Step, WrapStep, FusedPair };
  Kind kind = None;
  JacobiWrapParams p{}; // the non-wrap kernels take its JacobiParams base
  dim3 grid, block;
  int zc = 0; // planes per block, where it is a template argument (Lds, LdsWrap)
};

// mode: 0 = no row extension; 1 = free extension (single-process or RCCL-wire
// ranks: extended writes land in refresh-before-read halo/slack bytes or
// exterior cells a later same-stream kernel rewrites, never in a translate
// SOURCE, which is an interior cell); 2 = strict (IPC ranks: a fast peer
// writes our NEXT-buffer halos during our compute, so no extension is allowed
// -- the fast path engages only when the region is already aligned, which the
// allocation pad arranges for the overlap interior).
JacobiLaunch plan_jacobi(const LocalDomain &d, int64_t qi, const Rect3 &region,
                         const Rect3 &computeRegion, int mode,
                         JacobiLaunch::Want want = JacobiLaunch::Step) {
  JacobiLaunch l;
  const Vec3 ext = region.extent();
  if (ext.x <= 0 || ext.y <= 0 || ext.z <= 0) return l;
  const JacobiTuning &t = JacobiTuning::get();
  JacobiWrapParams &p = l.p;
  p.src = d.curr(qi).ptr;
  p.dst = d.next(qi).ptr;
  p.pitch = d.curr(qi).pitch;
  p.plane = d.curr(qi).plane();
  const Rect3 full = d.full_region();
  p.allocX = full.lo.x;
  p.allocY = full.lo.y;
  p.allocZ = full.lo.z;
  p.loX = p.trueLoX = region.lo.x;
  p.loY = region.lo.y;
  p.loZ = region.lo.z;
  p.extX = p.trueExtX = (int32_t)ext.x;
  p.extY = (int32_t)ext.y;
  p.extZ = (int32_t)ext.z;
  p.cLoX = computeRegion.lo.x;
  p.cLoY = computeRegion.lo.y;
  p.cLoZ = computeRegion.lo.z;
  p.cHiX = computeRegion.hi.x;
  p.cHiY = computeRegion.hi.y;
  p.cHiZ = computeRegion.hi.z;
  // pure-vector launch over the row-extended region (at least 8 cells wide)
  int64_t under, over;
  if (row_extension(d, qi, region, mode, under, over)) {
    p.loX -= under;
    p.extX += (int32_t)(under + over);
    p.vecAll = 1;
  }
  const uint32_t gridX = (uint32_t)((p.extX / 4 + 63) / 64); // 64 vectors per block row
  const bool lds = p.vecAll && t.lds;
  // LDS-staged y-rows variant (fixed 64x4 block); see jacobi_kernel_v4_lds
  auto lds_kernel = [&](JacobiLaunch::Kind kind) {
    l.kind = kind;
    l.zc = t.zc;
    l.block = dim3(64, 4, 1);
    l.grid = dim3(gridX, (uint32_t)((ext.y + 3) / 4), (uint32_t)((ext.z + t.zc - 1) / t.zc));
  };
  switch (want) {
  case JacobiLaunch::WrapStep:
    // a row that cannot be extended falls back to the translate graph
    if (lds && JacobiTuning::wrap()) lds_kernel(JacobiLaunch::LdsWrap);
    break;
  case JacobiLaunch::FusedPair: {
    // the fused kernel serves every geometry the WRAP kernel serves (the
    // wraps are true modulos); what remains are the grid limits and its
    // 32-bit lane offsets, which stay below one plane stride
    const int ny = JAC_F2_NY;
    l.block = dim3(64, ny, 1);
    l.grid = dim3(gridX, (uint32_t)((ext.y + ny - 3) / (ny - 2)),
                  (uint32_t)((ext.z + t.f2zc - 1) / t.f2zc));
    if (lds && JacobiTuning::wrap() && JacobiTuning::fuse2() && p.plane <= 0x7fffffff &&
        l.grid.y <= 65535 && l.grid.z <= 65535)
      l.kind = JacobiLaunch::Fuse2;
    break;
  }
  case JacobiLaunch::Step:
    if (lds) {
      lds_kernel(JacobiLaunch::Lds);
    } else if (p.extX >= 8 && ext.y <= 0x7fffffff) {
      // vectorized row-mapped kernel: the units formula must match the
      // kernel's head / body4 / tail
      const int64_t a0 = p.loX - full.lo.x;
      const int64_t headAl =
          (int64_t)((16 - (((uintptr_t)p.src + (uintptr_t)(a0 * 4)) & 15)) & 15) >> 2;
      const int64_t head = p.vecAll ? 0 : std::min<int64_t>(headAl, p.extX);
      const int64_t units = (p.extX - head) / 4 + (p.vecAll ? 0 : 2);
      l.kind = JacobiLaunch::Vec4;
      l.block = dim3((uint32_t)t.bx, (uint32_t)t.by, 1);
      l.grid = dim3((uint32_t)((units + t.bx - 1) / t.bx), (uint32_t)((ext.y + t.by - 1) / t.by),
                    (uint32_t)((ext.z + JAC_ZCHUNK - 1) / JAC_ZCHUNK));
    } else {
      // linearized, grid-stride with a capped grid
      l.kind = JacobiLaunch::Scalar;
      l.block = dim3(256);
      l.grid = dim3(grid_for(ext.flatten(), 256));
    }
    break;
  }
  return l;
}

void enqueue(const JacobiLaunch &l, hipStream_t stream) {
  const JacobiParams &base = l.p;
  switch (l.kind) {
  case JacobiLaunch::None:
    return;
  case JacobiLaunch::Scalar:
    hipLaunchKernelGGL(jacobi_kernel, l.grid, l.block, 0, stream, base);
    break;
  case JacobiLaunch::Vec4:
    hipLaunchKernelGGL(jacobi_kernel_v4, l.grid, l.block, 0, stream, base);
    break;
  case JacobiLaunch::Lds:
    if (l.zc == 32)
      hipLaunchKernelGGL(jacobi_kernel_v4_lds<32>, l.grid, l.block, 0, stream, base);
    else
      hipLaunchKernelGGL(jacobi_kernel_v4_lds<16>, l.grid, l.block, 0, stream, base);
    break;
  case JacobiLaunch::LdsWrap:
    if (l.zc == 32)
      hipLaunchKernelGGL((jacobi_kernel_v4_lds<32, true>), l.grid, l.block, 0, stream, l.p);
    else
      hipLaunchKernelGGL((jacobi_kernel_v4_lds<16, true>), l.grid, l.block, 0, stream, l.p);
    break;
  case JacobiLaunch::Fuse2:
    hipLaunchKernelGGL(jacobi_kernel_fuse2<JAC_F2_NY>, l.grid, l.block, 0, stream, l.p);
    break;
  }
  STENCIL_HIP(hipGetLastError());
}

// a plan made on either buffer parity, launched on the CURRENT one: only the
// two pointers differ (same pad and alignment, see row_extension)
void enqueue_current(JacobiLaunch l, const LocalDomain &d, int64_t qi, hipStream_t stream) {
  l.p.src = d.curr(qi).ptr;
  l.p.dst = d.next(qi).ptr;
  enqueue(l, stream);
}

// jacobi_step's argument checks, then its plan
JacobiLaunch checked_step_plan(ExchangeEngine &eng, int dom, int64_t qi, const Rect3 &region,
                               const Rect3 &computeRegion, int extendVec, const char *name) {
  LocalDomain &d = checked_jacobi_domain(eng, dom, qi, name);
  check_jacobi_region(d, region, name);
  if (extendVec < 0 || extendVec > 2)
    throw std::invalid_argument(std::string(name) + ": extend_vec must be 0, 1 or 2");
  return plan_jacobi(d, qi, region, computeRegion, extendVec);
}

} // namespace

void jacobi_step(ExchangeEngine &eng, int dom, int64_t qi, const Rect3 &region,
                 const Rect3 &computeRegion, int streamId, int extendVec) {
  const JacobiLaunch l =
      checked_step_plan(eng, dom, qi, region, computeRegion, extendVec, "jacobi_step");
  STENCIL_HIP(hipSetDevice(eng.domain(dom).gpu()));
  enqueue(l, eng.compute_stream(dom, streamId));
}

const char *jacobi_step_kernel(ExchangeEngine &eng, int dom, int64_t qi, const Rect3 &region,
                               const Rect3 &computeRegion, int extendVec) {
  const JacobiLaunch l =
      checked_step_plan(eng, dom, qi, region, computeRegion, extendVec, "jacobi_step_kernel");
  switch (l.kind) {
  case JacobiLaunch::Scalar:
    return "scalar";
  case JacobiLaunch::Vec4:
    return l.p.vecAll ? "vec4-all" : "vec4";
  case JacobiLaunch::Lds:
    return "lds";
  default:
    return "none"; // an empty region
  }
}

std::unique_ptr<JacobiStepGraph> jacobi_graph_create(ExchangeEngine &eng, int dom, int64_t qi,
                                                     const Rect3 &region,
                                                     const Rect3 &computeRegion) {
  LocalDomain &d = checked_jacobi_domain(eng, dom, qi, "jacobi_graph_create");
  check_jacobi_region(d, region, "jacobi_graph_create");
  return std::unique_ptr<JacobiStepGraph>(
      new JacobiStepGraph(eng, dom, qi, region, computeRegion));
}

// One graph per buffer parity: the jacobi kernargs are baked per parity
// (slot-indirecting the jacobi kernel itself was measured ~18% slower),
// while the translate jobs stay slot-indirect and an in-graph
// LocalDomain::enqueue_table_swap node flips the device tables.
JacobiStepGraph::JacobiStepGraph(ExchangeEngine &eng, int dom, int64_t qi, const Rect3 &region,
                                 const Rect3 &computeRegion)
    : ReplayGraph(eng, dom) {
  // whole-step replay graph: [translate copy_batch -> boundary fill (if
  // any axis is non-periodic) -> full-region jacobi -> device-side table
  // swap] captured once per buffer parity. Replay costs one hipGraphLaunch (~5 us) instead of the ~0.25 ms of host
  // orchestration measured per step at 750^3 (exchange + launches +
  // stream syncs + swap upload). Single-process single-domain only (the
  // periodic self-wrap bench shape): no wire/IPC machinery may exist.
  //
  // Fully periodic single domain (a WrapStep plan exists): every halo cell
  // is a copy of an interior cell of the same buffer, so the graph is the
  // WRAP stencil kernel ALONE -- it reads the wrapped neighbour itself, no
  // translate fills a halo (59 us/step of strided face copies at 750^3)
  // and nothing in the graph reads the device pointer tables, so the
  // table swap leaves the graph too (launch() hoists it).
  // Halos are STALE after steps taken on this path until the next
  // exchange(); interior cells are exact.
  LocalDomain &d = domain();
  // the wrap kernels serve exactly the single-domain fully periodic
  // whole-domain step
  const bool selfPeriodic = dom == 0 && eng.self_wrap_only(qi, 0) && d.elem_size(qi) == 4 &&
                            region == d.compute_region() && region == computeRegion;
  // planned once (the levers are read here, at graph creation); the captures
  // bake the pointers of their parity
  auto plan = [&](JacobiLaunch::Want want) {
    return plan_jacobi(d, qi, region, computeRegion, /*mode=*/1, want);
  };
  JacobiLaunch step = selfPeriodic ? plan(JacobiLaunch::WrapStep) : JacobiLaunch();
  wrap_ = step.kind == JacobiLaunch::LdsWrap;
  if (!wrap_) step = plan(JacobiLaunch::Step);
  for (int par = 0; par < 2; ++par) {
    exec_[par] = capture([&] {
      if (wrap_) {
        enqueue_current(step, d, qi, stream_);
      } else {
        eng.launch_translates_plain_on((uintptr_t)stream_, 0);
        // physical boundaries (no-op on a fully periodic domain): the fill
        // reads halos the translates delivered, same stream so ordered
        eng.launch_boundary_plain_on((uintptr_t)stream_, 0);
        // the graph's region is the whole interior rect: pure-vector launch
        // (scalar tail lanes measured ~10% of the kernel in the probe)
        enqueue_current(step, d, qi, stream_);
        d.enqueue_table_swap(stream_);
      }
    });
    d.swap(); // bake the other parity's kernarg pointers next round
  }
  // two swaps: host+device state is back where it started
  //
  // Fused pairs (a wrap graph with a FusedPair plan): a second graph per
  // parity holds jacobi_kernel_fuse2 alone, curr(t) -> next(t+2). A replay of
  // it is ONE buffer swap like a single step, so after it the buffer that was
  // `next` is current and holds t+2, while the new `next` still holds time t
  // (not t+1, which never reaches memory).
  const JacobiLaunch pair = wrap_ ? plan(JacobiLaunch::FusedPair) : JacobiLaunch();
  fused2_ = pair.kind == JacobiLaunch::Fuse2;
  if (fused2_) {
    for (int par = 0; par < 2; ++par) {
      exec2_[par] = capture([&] { enqueue_current(pair, d, qi, stream_); });
      d.swap();
    }
  }
}

void JacobiStepGraph::launch(int64_t nSteps) {
  LocalDomain &d = domain();
  STENCIL_HIP(hipSetDevice(dev_));
  // run(n >= 2) on a fused graph: n/2 two-step replays, then one single
  // step if n is odd. step() (n == 1) is always the single-step kernel.
  const int64_t nPairs = fused2_ ? nSteps / 2 : 0;
  const int64_t nSingle = nSteps - 2 * nPairs;
  for (int64_t i = 0; i < nPairs + nSingle; ++i) {
    STENCIL_HIP(hipGraphLaunch(i < nPairs ? exec2_[parity_] : exec_[parity_], stream_));
    parity_ ^= 1;
    d.swap_host_only(); // in-graph kernel flips the device tables
  }
  // the wrap graphs have no swap node (nothing in them reads the tables):
  // an even number of flips cancels, an odd one is ONE flip, enqueued behind
  // the replays so host and device state agree in stream order on return
  if (wrap_ && ((nPairs + nSingle) & 1)) d.enqueue_table_swap(stream_);
}

// Multi-rank whole-step graphs (one rank, one domain, cross-rank halos
// via IPC direct writes -- the 8-GPU single-node bench shape). The step
// splits at the cross-rank barrier:
//   A[par] = [interior jacobi -> translates (self + IPC views) ->
//             staged thin packs (parity)]
//   <barrier: all ranks' A complete -- RCCL all-reduce posted on the
//    SAME stream (fully stream-ordered), or a gloo host barrier with a
//    stream sync around it>
//   B[par] = [staged unpacks (parity) -> exterior slabs -> device table
//             swap -> device view flips]
// With the device barrier, steps queue back-to-back with ONE host sync
// per run(n): the eager path's ~0.21 ms/step of host orchestration
// (measured 0.989 vs 0.780 ms, profiles/r2/r2_gpu7_eager.log) collapses
// to two graph launches + one collective post per step.
std::unique_ptr<JacobiMrStepGraph>
jacobi_mr_graph_create(ExchangeEngine &eng, int dom, int64_t qi, const Rect3 &interior,
                       const Rect3 &computeRegion, const std::vector<Rect3> &exteriors,
                       int extendVec) {
  LocalDomain &d = checked_jacobi_domain(eng, dom, qi, "jacobi_mr_graph_create");
  check_jacobi_region(d, interior, "jacobi_mr_graph_create");
  for (const Rect3 &box : exteriors) check_jacobi_region(d, box, "jacobi_mr_graph_create");
  if (extendVec < 0 || extendVec > 2)
    throw std::invalid_argument("jacobi_mr_graph_create: extend_vec must be 0, 1 or 2");
  return std::unique_ptr<JacobiMrStepGraph>(
      new JacobiMrStepGraph(eng, dom, qi, interior, computeRegion, exteriors, extendVec));
}

JacobiMrStepGraph::JacobiMrStepGraph(ExchangeEngine &eng, int dom, int64_t qi,
                                     const Rect3 &interior, const Rect3 &computeRegion,
                                     const std::vector<Rect3> &exteriors, int extendVec)
    : ReplayGraph(eng, dom) {
  LocalDomain &d = domain();
  const JacobiLaunch inner = plan_jacobi(d, qi, interior, computeRegion, extendVec);
  std::vector<JacobiLaunch> slabs;
  for (const Rect3 &box : exteriors)
    slabs.push_back(plan_jacobi(d, qi, box, computeRegion, /*mode=*/0));
  for (int par = 0; par < 2; ++par) {
    // A: interior + outgoing halos
    execA_[par] = capture([&] {
      enqueue_current(inner, d, qi, stream_);
      eng.launch_translates_plain_on((uintptr_t)stream_, 0);
      eng.launch_packs_plain_on((uintptr_t)stream_, 1 + par); // staged parity
    });
    // B: incoming halos + exterior + swap
    execB_[par] = capture([&] {
      eng.launch_unpacks_plain_on((uintptr_t)stream_, 1 + par);
      for (const JacobiLaunch &slab : slabs) enqueue_current(slab, d, qi, stream_);
      d.enqueue_table_swap(stream_);
      eng.enqueue_view_flips((uintptr_t)stream_);
    });
    d.swap(); // bake the other parity's kernarg pointers next round
  }
}

void JacobiMrStepGraph::pre() { launch(execA_[parity_]); }

void JacobiMrStepGraph::post() {
  launch(execB_[parity_]);
  parity_ ^= 1;
  domain().swap_host_only(); // in-graph kernels flip the device state
  eng_.flip_views_host_only();
}

void fill_f32(ExchangeEngine &eng, int dom, int64_t qi, const Rect3 &region, float value,
              bool nextBuf) {
  LocalDomain &d = checked_jacobi_domain(eng, dom, qi, "fill_f32");
  if (!checked_extent("fill_f32", region)) return;
  const Vec3 ext = region.extent();
  const Rect3 full = d.full_region();
  check_inside("fill_f32", "region", region, full);
  const Vec3 pos = region.lo - full.lo; // allocation coords
  const Pitched &pp = d.curr(qi);
  const int64_t off = pos.z * pp.plane() + pos.y * pp.pitch + pos.x * 4;
  char *base = (nextBuf ? d.next(qi).ptr : d.curr(qi).ptr) + off;
  STENCIL_HIP(hipSetDevice(d.gpu()));
  hipLaunchKernelGGL(fill_kernel, dim3(grid_for(ext.flatten(), 256)), dim3(256), 0,
                     eng.compute_stream(dom), base, pp.pitch, pp.plane(), (int32_t)ext.x,
                     (int32_t)ext.y, (int32_t)ext.z, value);
  STENCIL_HIP(hipGetLastError());
}

namespace {

__global__ void div6_kernel(const float *in, float *out, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    out[i] = div6(in[i]);
}

} // namespace

void div6_f32(const float *in, float *out, int64_t n) {
  if (n <= 0) return;
  float *dIn = nullptr, *dOut = nullptr;
  STENCIL_HIP(hipMalloc(&dIn, n * sizeof(float)));
  if (hipMalloc(&dOut, n * sizeof(float)) != hipSuccess) {
    (void)hipFree(dIn);
    throw std::runtime_error("div6_f32: out of device memory");
  }
  hipError_t err = hipMemcpy(dIn, in, n * sizeof(float), hipMemcpyHostToDevice);
  if (err == hipSuccess) {
    hipLaunchKernelGGL(div6_kernel, dim3(grid_for(n, 256)), dim3(256), 0, nullptr, dIn, dOut, n);
    err = hipGetLastError();
  }
  if (err == hipSuccess) err = hipMemcpy(out, dOut, n * sizeof(float), hipMemcpyDeviceToHost);
  (void)hipFree(dIn);
  (void)hipFree(dOut);
  STENCIL_HIP(err);
}

} // namespace stencil_amd
