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
  int32_t vecAll; // 1 = pure-vector launch (see launch_jacobi_on)
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

__device__ __forceinline__ bool sphere_override(int64_t x, int64_t y, int64_t z,
                                                const JacobiParams &p, float &out) {
  const int64_t cw = p.cHiX - p.cLoX;
  const int64_t hotX = p.cLoX + cw / 3, coldX = p.cLoX + cw * 2 / 3;
  const int64_t cY = (p.cLoY + p.cHiY) / 2, cZ = (p.cLoZ + p.cHiZ) / 2;
  const int64_t r = cw / 10;
  {
    const int64_t dx = x - hotX, dy = y - cY, dz = z - cZ;
    const int64_t d = (int64_t)__fsqrt_rn((float)(dx * dx + dy * dy + dz * dz));
    if (d <= r) {
      out = 1.0f;
      return true;
    }
  }
  {
    const int64_t dx = x - coldX, dy = y - cY, dz = z - cZ;
    const int64_t d = (int64_t)__fsqrt_rn((float)(dx * dx + dy * dy + dz * dz));
    if (d <= r) {
      out = 0.0f;
      return true;
    }
  }
  return false;
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

  // sphere geometry (int32: grids are far below 2^31 per axis)
  const int32_t cw = (int32_t)(p.cHiX - p.cLoX);
  const int32_t hotX = (int32_t)p.cLoX + cw / 3, coldX = (int32_t)p.cLoX + cw * 2 / 3;
  const int32_t cY = (int32_t)(p.cLoY + p.cHiY) / 2, cZ = (int32_t)(p.cLoZ + p.cHiZ) / 2;
  const int32_t srad = cw / 10;

  auto sphere4 = [&](int32_t gx, int32_t gyy, int32_t gzz, float4 &out) {
    const int32_t dy = gyy - cY, dz = gzz - cZ;
    const int32_t yz2 = dy * dy + dz * dz;
    // truncated-int sqrt: only yz2 >= (r+1)^2 guarantees exclusion
    if (yz2 >= (srad + 1) * (srad + 1)) return;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int32_t dxh = gx + i - hotX, dxc = gx + i - coldX;
      if ((int32_t)__fsqrt_rn((float)(dxh * dxh + yz2)) <= srad)
        (&out.x)[i] = 1.0f;
      else if ((int32_t)__fsqrt_rn((float)(dxc * dxc + yz2)) <= srad)
        (&out.x)[i] = 0.0f;
    }
  };

  auto scalar_cell = [&](int32_t lx, int32_t lz) {
    const int64_t gx = p.loX + lx;
    const int64_t gz = p.loZ + lz;
    const int64_t ax = gx - p.allocX, az = gz - p.allocZ;
    const char *rowC = srcBase + az * p.plane + ay * p.pitch;
    float out;
    if (!sphere_override(gx, gy, gz, p, out)) {
      const float px = *(const float *)(rowC + (ax + 1) * 4);
      const float mx = *(const float *)(rowC + (ax - 1) * 4);
      const float py = *(const float *)(rowC + p.pitch + ax * 4);
      const float my = *(const float *)(rowC - p.pitch + ax * 4);
      const float pz = *(const float *)(rowC + p.plane + ax * 4);
      const float mz = *(const float *)(rowC - p.plane + ax * 4);
      out = (px + mx + py + my + pz + mz) / 6.0f;
    }
    *(float *)(dstBase + az * p.plane + ay * p.pitch + ax * 4) = out;
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
      float4 out;
      out.x = (cc.y + left + py.x + my.x + cp.x + cm.x) / 6.0f;
      out.y = (cc.z + cc.x + py.y + my.y + cp.y + cm.y) / 6.0f;
      out.z = (cc.w + cc.y + py.z + my.z + cp.z + cm.z) / 6.0f;
      out.w = (right + cc.z + py.w + my.w + cp.w + cm.w) / 6.0f;
      sphere4(gx, (int32_t)gy, (int32_t)(p.loZ + lz), out);
      // next is write-only this iteration: bypass cache pollution
      typedef float vfloat4 __attribute__((ext_vector_type(4)));
      vfloat4 ov = {out.x, out.y, out.z, out.w};
      __builtin_nontemporal_store(ov, (vfloat4 *)dcol);
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
      for (int32_t lx = 0; lx < head; ++lx) scalar_cell(lx, lz);
  } else if (u == body4 + 1) {
    for (int32_t lz = lz0; lz < zEnd; ++lz)
      for (int32_t lx = p.extX - tail; lx < p.extX; ++lx) scalar_cell(lx, lz);
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
// (jacobi_wrap_eligible answers false).
// gfx950 resource usage (-Rpass-analysis=kernel-resource-usage), the same
// for ZC = 16 and 32:
//   WRAP=false: 58 VGPRs, 54 SGPRs, 0 scratch, 8 waves/SIMD, 12288 B LDS
//   WRAP=true : 58 VGPRs, 58 SGPRs, 0 scratch, 8 waves/SIMD, 12288 B LDS
// (the row/plane selects and the six x-select lane masks live in scalar
// registers; the WRAP=false instruction stream is unchanged by the flag)
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
  //   mzOff : the initial -z plane        (+z plane: colP, in the loop)
  int64_t myHalo = 0, pyHalo, mzOff = 0;
  if constexpr (WRAP) {
    // all three depend on blockIdx only: scalar registers
    const int32_t by0 = blockIdx.y * 4, by3 = by0 + 3;
    const int64_t ySpan = (int64_t)(p.extY - 1) * p.pitch;
    myHalo = by0 == 0 ? ySpan : -p.pitch;
    // ry==3 at the last row wraps down to row 0; past it the lane already
    // sits on row 0 and any in-range row will do
    pyHalo = by3 < p.extY - 1 ? p.pitch : (by3 == p.extY - 1 ? -ySpan : 0);
    mzOff = lz0 == 0 ? (int64_t)(p.extZ - 1) * p.plane : -p.plane;
  } else {
    // +y halo row staged by ry==3: one past its own row, clamped in-bounds
    // (the -y row and -z plane are the fixed - p.pitch / - p.plane)
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

  const int32_t cw = (int32_t)(p.cHiX - p.cLoX);
  const int32_t hotX = (int32_t)p.cLoX + cw / 3, coldX = (int32_t)p.cLoX + cw * 2 / 3;
  const int32_t cY = (int32_t)(p.cLoY + p.cHiY) / 2, cZ = (int32_t)(p.cLoZ + p.cHiZ) / 2;
  const int32_t srad = cw / 10;
  auto sphere4 = [&](int32_t gzz, float4 &out) {
    const int32_t dy = (int32_t)gy - cY, dz = gzz - cZ;
    const int32_t yz2 = dy * dy + dz * dz;
    if (yz2 >= (srad + 1) * (srad + 1)) return;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int32_t dxh = gx + i - hotX, dxc = gx + i - coldX;
      if ((int32_t)__fsqrt_rn((float)(dxh * dxh + yz2)) <= srad)
        (&out.x)[i] = 1.0f;
      else if ((int32_t)__fsqrt_rn((float)(dxc * dxc + yz2)) <= srad)
        (&out.x)[i] = 0.0f;
    }
  };

  // WRAP x axis: where the first / last lane of a row find the periodic
  // neighbour of the row's true end cells, and which component takes it
  int32_t leftOff = -4, rightOff = 16;
  bool wl1 = false, wl2 = false, wl3 = false; // left -> -x of component k
  bool wr0 = false, wr1 = false, wr2 = false; // right -> +x of component k
  if constexpr (WRAP) {
    const int32_t under = (int32_t)(p.trueLoX - p.loX); // 0..3
    const int32_t last = under + p.trueExtX - 1;        // in vector body4-1
    const int32_t lastC = last & 3;                     // 3 - over
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

  float4 cm, cc;
  if constexpr (WRAP) {
    cm = *(const float4 *)(col + mzOff);
    cc = *(const float4 *)(col);
    tile[0][ry + 1][tx] = cc;
    if (ry == 0) tile[0][0][tx] = *(const float4 *)(col + myHalo);
  } else {
    cm = *(const float4 *)(col - p.plane);
    cc = *(const float4 *)(col);
    tile[0][ry + 1][tx] = cc;
    if (ry == 0) tile[0][0][tx] = *(const float4 *)(col - p.pitch);
  }
  if (ry == 3) tile[0][5][tx] = *(const float4 *)(col + pyHalo);
  __syncthreads();
  int buf = 0;
  for (int32_t lz = lz0; lz < zEnd; ++lz) {
    // +z plane and the -y row in it; WRAP: uniform per iteration
    const char *colP, *colPmy;
    float left, right;
    if constexpr (WRAP) {
      colP = col + (lz == p.extZ - 1 ? -(int64_t)(p.extZ - 1) * p.plane : p.plane);
      colPmy = colP + myHalo;
      left = *(const float *)(col + leftOff);
      right = *(const float *)(col + rightOff);
    } else {
      colP = col + p.plane;
      colPmy = col + p.plane - p.pitch;
      left = *(const float *)(col - 4);
      right = *(const float *)(col + 16);
    }
    const float4 cp = *(const float4 *)colP;
    const float4 py = tile[buf][ry + 2][tx];
    const float4 my = tile[buf][ry][tx];
    float4 out;
    if constexpr (WRAP) {
      out.x = ((wr0 ? right : cc.y) + left + py.x + my.x + cp.x + cm.x) / 6.0f;
      out.y = ((wr1 ? right : cc.z) + (wl1 ? left : cc.x) + py.y + my.y + cp.y + cm.y) / 6.0f;
      out.z = ((wr2 ? right : cc.w) + (wl2 ? left : cc.y) + py.z + my.z + cp.z + cm.z) / 6.0f;
      out.w = (right + (wl3 ? left : cc.z) + py.w + my.w + cp.w + cm.w) / 6.0f;
    } else {
      out.x = (cc.y + left + py.x + my.x + cp.x + cm.x) / 6.0f;
      out.y = (cc.z + cc.x + py.y + my.y + cp.y + cm.y) / 6.0f;
      out.z = (cc.w + cc.y + py.z + my.z + cp.z + cm.z) / 6.0f;
      out.w = (right + cc.z + py.w + my.w + cp.w + cm.w) / 6.0f;
    }
    sphere4((int32_t)(p.loZ + lz), out);
    if (valid) {
      typedef float vfloat4 __attribute__((ext_vector_type(4)));
      vfloat4 ov = {out.x, out.y, out.z, out.w};
      __builtin_nontemporal_store(ov, (vfloat4 *)dcol);
    }
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

// Lane shifts of one VGPR by data-parallel-primitive moves (no LDS, no
// memory). Every lane of the wave must be active where they are used.
//   lane_below: lane i gets v of lane i-1 of the wave, lane 0 gets `first`
//   lane_above: lane i gets v of lane i+1 of the wave, lane 63 keeps its own
//   row_above<N>: lane i gets lane i+N of its 16-lane row (0 past the row)
__device__ __forceinline__ float lane_below(float v, float first) {
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(first), __float_as_int(v),
                                                    0x138 /* wave_shr:1 */, 0xf, 0xf, false));
}
__device__ __forceinline__ float lane_above(float v) {
  const int i = __float_as_int(v);
  return __int_as_float(__builtin_amdgcn_update_dpp(i, i, 0x130 /* wave_shl:1 */, 0xf, 0xf, false));
}
template <int N> __device__ __forceinline__ float row_above(float v) {
  static_assert(N >= 1 && N <= 15, "row shift");
  return __int_as_float(
      __builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x100 + N /* row_shl:N */, 0xf, 0xf, true));
}
// A wave-uniform address as a scalar-register base in the GLOBAL address
// space: the loads and the store below then take the form scalar base +
// 32-bit lane offset. (Through a generic pointer they would become flat
// instructions, and without the pin the compiler folds the lane offset into a
// per-lane 64-bit pointer and multiplies per load.)
typedef float vfloat4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) char gchar;
__device__ __forceinline__ gchar *global_base(const void *p) {
  const uint64_t v = (uint64_t)p;
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
  return (gchar *)(((uint64_t)hi << 32) | lo);
}
// A loop-invariant 32-bit lane offset, made opaque at its use: the zero
// extension then stays next to the access, where instruction selection folds
// it into the scalar-base form; hoisted out of the loop it becomes a 64-bit
// register pair and a 64-bit vector add per access.
__device__ __forceinline__ uint32_t lane_offset(uint32_t o) {
  asm volatile("" : "+v"(o));
  return o;
}
__device__ __forceinline__ float lane_value(float v, int lane) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
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
// stride, which jacobi_fuse2_eligible bounds to 31 bits.
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
//   78 VGPRs, 78 SGPRs, 0 scratch, 6 waves/SIMD, 36864 B LDS: three blocks
//   (24 waves) per CU, bound by the VGPRs (80 is the most for 6 waves/SIMD).
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

  const int32_t cw = (int32_t)(p.cHiX - p.cLoX);
  const int32_t hotX = (int32_t)p.cLoX + cw / 3, coldX = (int32_t)p.cLoX + cw * 2 / 3;
  const int32_t cY = (int32_t)(p.cLoY + p.cHiY) / 2, cZ = (int32_t)(p.cLoZ + p.cHiZ) / 2;
  const int32_t srad = cw / 10;
  auto sphere4 = [&](int32_t gzz, float4 &out) {
    const int32_t dy = gy - cY, dz = gzz - cZ;
    const int32_t yz2 = dy * dy + dz * dz;
    if (yz2 >= (srad + 1) * (srad + 1)) return;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int32_t dxh = gx + i - hotX, dxc = gx + i - coldX;
      if ((int32_t)__fsqrt_rn((float)(dxh * dxh + yz2)) <= srad)
        (&out.x)[i] = 1.0f;
      else if ((int32_t)__fsqrt_rn((float)(dxc * dxc + yz2)) <= srad)
        (&out.x)[i] = 0.0f;
    }
  };

  // x wrap of the row's true end cells, as in the WRAP kernel: extended
  // index `under` is the first true cell, `last` the last one
  const int32_t under = (int32_t)(p.trueLoX - p.loX); // 0..3
  const int32_t last = under + p.trueExtX - 1;        // in vector body4-1
  const int32_t lastC = last & 3;                     // 3 - over
  const bool first = u == 0, lastLane = u == body4 - 1;
  const bool wl1 = first && under == 1, wl2 = first && under == 2, wl3 = first && under == 3;
  const bool wr0 = lastLane && lastC == 0, wr1 = lastLane && lastC == 1,
             wr2 = lastLane && lastC == 2;
  // one stencil evaluation of a vector: c its own plane (x neighbours
  // inside), l / r the scalars across its ends, then +y -y +z -z
  auto stencil4 = [&](const float4 &c, float l, float r, const float4 &py, const float4 &my,
                      const float4 &pz, const float4 &mz) {
    float4 s;
    s.x = ((wr0 ? r : c.y) + l + py.x + my.x + pz.x + mz.x);
    s.y = ((wr1 ? r : c.z) + (wl1 ? l : c.x) + py.y + my.y + pz.y + mz.y);
    s.z = ((wr2 ? r : c.w) + (wl2 ? l : c.y) + py.z + my.z + pz.z + mz.z);
    s.w = (r + (wl3 ? l : c.z) + py.w + my.w + pz.w + mz.w);
    return div6(s);
  };

  // tile x edges (uniform per block): rl is the last lane that holds a
  // vector of its own; eL / eR are the extended indices of the true cells
  // just outside the tile, wrapped at the row's ends. Lane 0 computes the
  // t+1 value of eL, lane 1 that of eR.
  const int32_t rl = min(63, body4 - 1 - ub);
  const int32_t eL = f2_edge_left(ub, last), eR = f2_edge_right(ub, body4, under);
  const int32_t gxE = (int32_t)p.loX + (tx == 0 ? eL : eR);
  const bool rightEdge = tx >= rl;
  // the lane's scalar of the gathered load, from cell 0 of row 0 of a plane
  const uint32_t goff = f2_gather_offset(tx, eL, eR, under, last, yo, ym, yp, (uint32_t)p.pitch);

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
    float4 s = stencil4(cc, l, r, tT[tb][ry + 2][tx], tT[tb][ry][tx], cp, cm);
    sphere4((int32_t)p.loZ + i0, s);

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
        const int32_t dy = gy - cY, dz = (int32_t)p.loZ + iM1 - cZ;
        const int32_t yz2 = dy * dy + dz * dz;
        const int32_t dxh = gxE - hotX, dxc = gxE - coldX;
        if ((int32_t)__fsqrt_rn((float)(dxh * dxh + yz2)) <= srad)
          e1 = 1.0f;
        else if ((int32_t)__fsqrt_rn((float)(dxc * dxc + yz2)) <= srad)
          e1 = 0.0f;
      }
      const float eRight = lane_value(e1, 1);
      const float l2 = lane_below(sc.w, e1);
      const float ra2 = lane_above(sc.x);
      const float r2 = rightEdge ? eRight : ra2;
      float4 out = stencil4(sc, l2, r2, tS[sb ^ 1][min(ry + 1, NY - 1)][tx],
                            tS[sb ^ 1][max(ry - 1, 0)][tx], s, sm);
      sphere4((int32_t)p.loZ + iM1, out);
      if (valid) {
        vfloat4 ov = {out.x, out.y, out.z, out.w};
        __builtin_nontemporal_store(
            ov, (__attribute__((address_space(1))) vfloat4 *)(global_base(dstO + zoff(iM1)) +
                                                             lane_offset(voff)));
      }
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
    const char *rowC = srcBase + az * p.plane + ay * p.pitch;
    float out;
    if (!sphere_override(gx, gy, gz, p, out)) {
      const float px = *(const float *)(rowC + (ax + 1) * 4);
      const float mx = *(const float *)(rowC + (ax - 1) * 4);
      const float py = *(const float *)(rowC + p.pitch + ax * 4);
      const float my = *(const float *)(rowC - p.pitch + ax * 4);
      const float pz = *(const float *)(rowC + p.plane + ax * 4);
      const float mz = *(const float *)(rowC - p.plane + ax * 4);
      out = (px + mx + py + my + pz + mz) / 6.0f;
    }
    *(float *)(dstBase + az * p.plane + ay * p.pitch + ax * 4) = out;
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

} // namespace

namespace {

// STENCIL_JAC_LDS=0 turns the LDS-rows kernel off (read once)
bool jac_use_lds() {
  static int useLds = -1;
  if (useLds < 0) {
    const char *e = getenv("STENCIL_JAC_LDS");
    useLds = (e && e[0] == '0') ? 0 : 1;
  }
  return useLds != 0;
}

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

// shared launch logic: builds params from the domain's CURRENT buffer
// parity and enqueues the right kernel variant onto `stream`. Also used
// by the whole-step hipGraph capture (pointers get baked per parity).
// fullRectVec: 0 = off; 1 = free extension (single-process or RCCL-wire
// ranks: extended writes land in refresh-before-read halo/slack bytes or
// exterior cells a later same-stream kernel rewrites); 2 = strict (IPC
// ranks: a fast peer writes our NEXT-buffer halos during our compute, so
// no extension is allowed -- the fast path engages only when the region
// is already aligned, which the allocation pad arranges for the overlap
// interior).
// wrap: launch the WRAP instantiation of jacobi_kernel_v4_lds (periodic
// neighbours read in-kernel): the caller guarantees that `region` is the
// whole domain and periodic on every axis (see jacobi_graph_create); throws
// if the LDS kernel would not be selected.
void launch_jacobi_on(LocalDomain &d, int64_t qi, const Rect3 &region,
                      const Rect3 &computeRegion, hipStream_t stream, int fullRectVec = 0,
                      bool wrap = false) {
  Vec3 ext = region.extent();
  if (ext.x <= 0 || ext.y <= 0 || ext.z <= 0) return;
  JacobiParams p{};
  p.src = d.curr(qi).ptr;
  p.dst = d.next(qi).ptr;
  p.pitch = d.curr(qi).pitch;
  p.plane = d.curr(qi).plane();
  const Rect3 full = d.full_region();
  p.allocX = full.lo.x;
  p.allocY = full.lo.y;
  p.allocZ = full.lo.z;
  p.loX = region.lo.x;
  p.loY = region.lo.y;
  p.loZ = region.lo.z;
  p.extX = (int32_t)ext.x;
  p.extY = (int32_t)ext.y;
  p.extZ = (int32_t)ext.z;
  p.cLoX = computeRegion.lo.x;
  p.cLoY = computeRegion.lo.y;
  p.cLoZ = computeRegion.lo.z;
  p.cHiX = computeRegion.hi.x;
  p.cHiY = computeRegion.hi.y;
  p.cHiZ = computeRegion.hi.z;
  // fullRectVec: pure-vector launch over the row-extended region where
  // row_extension allows it. The extended cells are x-halo cells, cells of
  // the local rect in the same row (a later same-stream kernel rewrites
  // them) or pitch-slack bytes: every one is rewritten by the next exchange
  // (or is padding) before any read, and never a translate SOURCE (sources
  // are interior cells).
  int64_t under, over;
  if (row_extension(d, qi, region, fullRectVec, under, over)) {
    p.loX = region.lo.x - under;
    p.extX = (int32_t)(ext.x + under + over);
    p.vecAll = 1;
    ext.x = p.extX;
  }
  const bool useLds = jac_use_lds();
  if (wrap && !(p.vecAll && useLds))
    throw std::runtime_error("jacobi: wrap launch needs the vecAll LDS kernel");
  if (p.vecAll && useLds && ext.x >= 8) {
    // LDS-staged y-rows variant (fixed 64x4 block); see jacobi_kernel_v4_lds
    static int zc = 0;
    if (!zc) {
      const char *e = getenv("STENCIL_JAC_ZC");
      zc = (e && atoi(e) == 16) ? 16 : 32; // 32 measured +1.8% (gpu35)
    }
    dim3 block(64, 4, 1);
    dim3 grid((uint32_t)((p.extX / 4 + 63) / 64), (uint32_t)((ext.y + 3) / 4),
              (uint32_t)((ext.z + zc - 1) / zc));
    if (wrap) {
      JacobiWrapParams wp{};
      static_cast<JacobiParams &>(wp) = p;
      wp.trueLoX = region.lo.x;
      wp.trueExtX = (int32_t)region.extent().x;
      if (zc == 32)
        hipLaunchKernelGGL((jacobi_kernel_v4_lds<32, true>), grid, block, 0, stream, wp);
      else
        hipLaunchKernelGGL((jacobi_kernel_v4_lds<16, true>), grid, block, 0, stream, wp);
    } else if (zc == 32)
      hipLaunchKernelGGL(jacobi_kernel_v4_lds<32>, grid, block, 0, stream, p);
    else
      hipLaunchKernelGGL(jacobi_kernel_v4_lds<16>, grid, block, 0, stream, p);
    STENCIL_HIP(hipGetLastError());
    return;
  }
  if (ext.x >= 8 && ext.y <= 0x7fffffff) {
    // vectorized row-mapped kernel; block shape tunable via env
    const int64_t a0 = p.loX - full.lo.x;
    const int64_t headAl =
        (int64_t)((16 - (((uintptr_t)p.src + (uintptr_t)(a0 * 4)) & 15)) & 15) >> 2;
    const int64_t head = p.vecAll ? 0 : std::min<int64_t>(headAl, ext.x);
    const int64_t units = (ext.x - head) / 4 + (p.vecAll ? 0 : 2);
    static int bx = 0, by = 0;
    if (!bx) {
      bx = 64;
      by = 4;
      if (const char *e = getenv("STENCIL_JAC_BLOCK")) {
        if (sscanf(e, "%dx%d", &bx, &by) != 2 || bx * by != 256) {
          bx = 64;
          by = 4;
        }
      }
    }
    dim3 block((uint32_t)bx, (uint32_t)by, 1);
    dim3 grid((uint32_t)((units + bx - 1) / bx), (uint32_t)((ext.y + by - 1) / by),
              (uint32_t)((ext.z + 15) / 16)); // 16 == JAC_ZCHUNK
    hipLaunchKernelGGL(jacobi_kernel_v4, grid, block, 0, stream, p);
  } else {
    hipLaunchKernelGGL(jacobi_kernel, dim3(grid_for(ext.flatten(), 256)), dim3(256), 0,
                       stream, p);
  }
  STENCIL_HIP(hipGetLastError());
}

} // namespace

void jacobi_step(ExchangeEngine &eng, int dom, int64_t qi, const Rect3 &region,
                 const Rect3 &computeRegion, int streamId, int extendVec) {
  LocalDomain &d = checked_jacobi_domain(eng, dom, qi, "jacobi_step");
  check_jacobi_region(d, region, "jacobi_step");
  if (extendVec < 0 || extendVec > 2)
    throw std::invalid_argument("jacobi_step: extend_vec must be 0, 1 or 2");
  STENCIL_HIP(hipSetDevice(d.gpu()));
  launch_jacobi_on(d, qi, region, computeRegion, eng.compute_stream(dom, streamId),
                   extendVec);
}

namespace {

// The wrap-reading graph serves exactly the single-domain fully periodic
// whole-domain step that launch_jacobi_on would give to
// jacobi_kernel_v4_lds. STENCIL_JAC_WRAP=0 forces the translate graph (the
// A/B lever and the fallback); it is read at each graph creation, which is
// set-up and never on the step path.
bool jacobi_wrap_eligible(ExchangeEngine &eng, int dom, int64_t qi, const Rect3 &region,
                          const Rect3 &computeRegion) {
  const char *e = getenv("STENCIL_JAC_WRAP");
  if (e && e[0] == '0') return false;
  if (dom != 0 || !eng.self_wrap_only(qi, 0)) return false;
  const LocalDomain &d = eng.domain(dom);
  if (d.elem_size(qi) != 4) return false;
  if (!(region == d.compute_region()) || !(region == computeRegion)) return false;
  // the wrap kernel is a vecAll launch: rows that cannot be extended
  // (row_extension) fall back to the translate graph
  int64_t under, over;
  return jac_use_lds() && row_extension(d, qi, region, /*mode=*/1, under, over);
}

// Rows per block of jacobi_kernel_fuse2 (6 of them useful). 8 rows are 8
// waves and 36 KB of LDS, so three blocks share a CU (two while the kernel
// held 122 VGPRs) and the others compute while one waits at its barrier; 14
// rows (12 useful, 14% instead of 25% redundant stage-1 rows, but one block
// per CU) measured 12% slower at 122 VGPRs.
constexpr int JAC_F2_NY = 8;

// planes per block of the fused kernel; STENCIL_JAC_F2ZC overrides (read once)
int jac_f2_zc() {
  static int zc = 0;
  if (!zc) {
    const char *e = getenv("STENCIL_JAC_F2ZC");
    const int v = e ? atoi(e) : 0;
    zc = v >= 1 ? v : 64;
  }
  return zc;
}

dim3 jac_f2_grid(int64_t extXvec, int64_t extY, int64_t extZ) {
  const int zc = jac_f2_zc(), ny = JAC_F2_NY;
  return dim3((uint32_t)((extXvec / 4 + 63) / 64), (uint32_t)((extY + ny - 3) / (ny - 2)),
              (uint32_t)((extZ + zc - 1) / zc));
}

// Whether a wrap graph may replay the fused two-step kernel. The kernel
// serves every geometry the WRAP kernel serves (the wraps are true modulos),
// so what remains is the switch and the grid limits. STENCIL_JAC_FUSE2=0
// forces single-step replays (the A/B lever); read at each graph creation.
bool jacobi_fuse2_eligible(bool wrap, const LocalDomain &d, int64_t qi, const Rect3 &region) {
  if (!wrap) return false;
  const char *e = getenv("STENCIL_JAC_FUSE2");
  if (e && e[0] == '0') return false;
  int64_t under, over;
  if (!row_extension(d, qi, region, /*mode=*/1, under, over)) return false;
  const Vec3 ext = region.extent();
  const dim3 g = jac_f2_grid(ext.x + under + over, ext.y, ext.z);
  // the kernel's lane offsets are 32-bit and stay below one plane stride
  if (d.curr(qi).plane() > 0x7fffffff) return false;
  return g.y <= 65535 && g.z <= 65535;
}

// the fused kernel over the whole (row-extended) domain, curr -> next
void launch_jacobi_fuse2_on(LocalDomain &d, int64_t qi, const Rect3 &region,
                            const Rect3 &computeRegion, hipStream_t stream) {
  const Vec3 ext = region.extent();
  int64_t under, over;
  if (!row_extension(d, qi, region, /*mode=*/1, under, over))
    throw std::runtime_error("jacobi: fused launch needs the row extension");
  JacobiWrapParams p{};
  p.src = d.curr(qi).ptr;
  p.dst = d.next(qi).ptr;
  p.pitch = d.curr(qi).pitch;
  p.plane = d.curr(qi).plane();
  const Rect3 full = d.full_region();
  p.allocX = full.lo.x;
  p.allocY = full.lo.y;
  p.allocZ = full.lo.z;
  p.loX = region.lo.x - under;
  p.loY = region.lo.y;
  p.loZ = region.lo.z;
  p.extX = (int32_t)(ext.x + under + over);
  p.extY = (int32_t)ext.y;
  p.extZ = (int32_t)ext.z;
  p.vecAll = 1;
  p.cLoX = computeRegion.lo.x;
  p.cLoY = computeRegion.lo.y;
  p.cLoZ = computeRegion.lo.z;
  p.cHiX = computeRegion.hi.x;
  p.cHiY = computeRegion.hi.y;
  p.cHiZ = computeRegion.hi.z;
  p.trueLoX = region.lo.x;
  p.trueExtX = (int32_t)ext.x;
  const dim3 grid = jac_f2_grid(p.extX, ext.y, ext.z);
  hipLaunchKernelGGL(jacobi_kernel_fuse2<JAC_F2_NY>, grid, dim3(64, JAC_F2_NY, 1), 0, stream, p);
  STENCIL_HIP(hipGetLastError());
}

} // namespace

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
  // any axis is non-periodic) -> full-region jacobi -> device-side table swap] captured once per buffer parity. Replay
  // costs one hipGraphLaunch (~5 us) instead of the ~0.25 ms of host
  // orchestration measured per step at 750^3 (exchange + launches +
  // stream syncs + swap upload). Single-process single-domain only (the
  // periodic self-wrap bench shape): no wire/IPC machinery may exist.
  //
  // Fully periodic single domain (jacobi_wrap_eligible): every halo cell
  // is a copy of an interior cell of the same buffer, so the graph is the
  // WRAP stencil kernel ALONE -- it reads the wrapped neighbour itself, no
  // translate fills a halo (59 us/step of strided face copies at 750^3)
  // and nothing in the graph reads the device pointer tables, so the
  // table swap leaves the graph too (launch() hoists it).
  // Halos are STALE after steps taken on this path until the next
  // exchange(); interior cells are exact.
  LocalDomain &d = domain();
  wrap_ = jacobi_wrap_eligible(eng, dom, qi, region, computeRegion);
  for (int par = 0; par < 2; ++par) {
    exec_[par] = capture([&] {
      if (wrap_) {
        launch_jacobi_on(d, qi, region, computeRegion, stream_, /*fullRectVec=*/1,
                         /*wrap=*/true);
      } else {
        eng.launch_translates_plain_on((uintptr_t)stream_, 0);
        // physical boundaries (no-op on a fully periodic domain): the fill
        // reads halos the translates delivered, same stream so ordered
        eng.launch_boundary_plain_on((uintptr_t)stream_, 0);
        // the graph's region is the whole interior rect: pure-vector launch
        // (scalar tail lanes measured ~10% of the kernel in the probe)
        launch_jacobi_on(d, qi, region, computeRegion, stream_, /*fullRectVec=*/1);
        d.enqueue_table_swap(stream_);
      }
    });
    d.swap(); // bake the other parity's kernarg pointers next round
  }
  // two swaps: host+device state is back where it started
  //
  // Fused pairs (jacobi_fuse2_eligible): a second graph per parity holds
  // jacobi_kernel_fuse2 alone, curr(t) -> next(t+2). A replay of it is ONE
  // buffer swap like a single step, so after it the buffer that was `next`
  // is current and holds t+2, while the new `next` still holds time t (not
  // t+1, which never reaches memory).
  fused2_ = jacobi_fuse2_eligible(wrap_, d, qi, region);
  if (fused2_) {
    for (int par = 0; par < 2; ++par) {
      exec2_[par] = capture([&] { launch_jacobi_fuse2_on(d, qi, region, computeRegion, stream_); });
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
  for (int par = 0; par < 2; ++par) {
    // A: interior + outgoing halos
    execA_[par] = capture([&] {
      launch_jacobi_on(d, qi, interior, computeRegion, stream_, extendVec);
      eng.launch_translates_plain_on((uintptr_t)stream_, 0);
      eng.launch_packs_plain_on((uintptr_t)stream_, 1 + par); // staged parity
    });
    // B: incoming halos + exterior + swap
    execB_[par] = capture([&] {
      eng.launch_unpacks_plain_on((uintptr_t)stream_, 1 + par);
      for (const Rect3 &box : exteriors)
        launch_jacobi_on(d, qi, box, computeRegion, stream_, /*fullRectVec=*/0);
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
