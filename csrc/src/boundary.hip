// Physical (non-periodic) boundary fill: job-table construction and the
// batched fill kernel. See engine.hpp (Boundary, FillJob) for the API.
//
// Semantics: the halo of a subdomain that points out of the global domain
// on a non-periodic axis holds what padding the global array one axis at a
// time, x then y then z, would produce (constant / edge / symmetric /
// negated symmetric per face). The kernel implements the equivalent
// single-pass rule: walk the axes z, y, x; on each non-periodic axis where
// the region lies outside [0, N) apply the face's map. FIXED ends the walk
// with the constant times the accumulated sign; CLAMP / MIRROR / ANTIMIRROR
// map the coordinate back inside (ANTIMIRROR flips the sign); OPEN ends the
// walk: unwritten if nothing was mapped yet, else a copy from the source
// mapped so far. A whole region shares one treatment per axis, so the walk
// is resolved on the host into a per-job affine source map.
//
// Race freedom (why ONE launch with no ordering among jobs is enough): the
// final source cell is outside the global domain on no non-periodic axis
// that the walk mapped, and the walk only stops early at an OPEN face whose
// cells no job writes. So a source is an interior cell, a halo cell the
// exchange delivered, or a user-owned OPEN cell -- never the destination of
// any fill job. Every job reads only cells no job writes.
#include "stencil_amd/device_util.hpp"
#include "stencil_amd/engine.hpp"
#include "stencil_amd/hip_check.hpp"

#include <roctracer/roctx.h>

#include <algorithm>
#include <cstring>
#include <stdexcept>

namespace stencil_amd {

namespace {

constexpr int kBlock = 256;

struct alignas(16) W16 {
  uint64_t a, b;
};

__global__ void boundary_fill_kernel(const FillJob *__restrict__ jobs,
                                     const int64_t *__restrict__ prefix, int nJobs) {
  // binary-search the job that owns this block (as copy_batch_kernel)
  const int64_t b = blockIdx.x;
  int lo = 0, hi = nJobs - 1;
  while (lo < hi) {
    const int mid = (lo + hi) / 2;
    if (prefix[mid + 1] <= b) {
      lo = mid + 1;
    } else {
      hi = mid;
    }
  }
  const FillJob j = jobs[lo];
  char *base = uniform_ptr(*j.slot);
  char *dst = base + j.dstOff;
  const char *src = base + j.srcOff;

  const int64_t jobBlocks = prefix[lo + 1] - prefix[lo];
  const int64_t stride = jobBlocks * blockDim.x;
  for (int64_t w = (b - prefix[lo]) * blockDim.x + threadIdx.x; w < j.nWords; w += stride) {
    const int32_t wx = (int32_t)(w % j.extXw);
    const int64_t t = w / j.extXw;
    const int32_t wy = (int32_t)(t % j.extY);
    const int64_t wz = t / j.extY;
    char *d = dst + wz * j.plane + (int64_t)wy * j.pitch + (int64_t)wx * j.wordBytes;
    const char *s = src + wz * j.srcSz + (int64_t)wy * j.srcSy + (int64_t)wx * j.srcSx;
    // broadcast jobs never dereference s; copy jobs XOR the sign mask
    // (zero unless an ANTIMIRROR face was crossed an odd number of times)
    switch (j.wordBytes) {
    case 16: {
      W16 v{j.pat[0], j.pat[1]};
      if (!j.broadcast) {
        const W16 in = *reinterpret_cast<const W16 *>(s);
        v.a ^= in.a;
        v.b ^= in.b;
      }
      *reinterpret_cast<W16 *>(d) = v;
      break;
    }
    case 8: {
      uint64_t v = j.pat[0];
      if (!j.broadcast) v ^= *reinterpret_cast<const uint64_t *>(s);
      *reinterpret_cast<uint64_t *>(d) = v;
      break;
    }
    case 4: {
      uint32_t v = (uint32_t)j.pat[0];
      if (!j.broadcast) v ^= *reinterpret_cast<const uint32_t *>(s);
      *reinterpret_cast<uint32_t *>(d) = v;
      break;
    }
    case 2: {
      uint16_t v = (uint16_t)j.pat[0];
      if (!j.broadcast) v ^= *reinterpret_cast<const uint16_t *>(s);
      *reinterpret_cast<uint16_t *>(d) = v;
      break;
    }
    default: {
      uint8_t v = (uint8_t)j.pat[0];
      if (!j.broadcast) v ^= *reinterpret_cast<const uint8_t *>(s);
      *reinterpret_cast<uint8_t *>(d) = v;
      break;
    }
    }
  }
}

// replicate an `es`-byte element pattern across 16 bytes
void replicate(const char *elem, int64_t es, uint64_t out[2]) {
  char buf[16];
  for (int i = 0; i < 16; ++i) buf[i] = elem[i % es];
  std::memcpy(out, buf, 16);
}

} // namespace

void FillBatch::finalize_upload() {
  std::vector<int64_t> nWords;
  for (const auto &j : jobs) nWords.push_back(j.nWords);
  nBlocks = detail::block_prefix(nWords, prefix); // same cap as CopyBatch
  STENCIL_HIP(hipSetDevice(dev));
  STENCIL_HIP(hipMalloc((void **)&dJobs, jobs.size() * sizeof(FillJob)));
  STENCIL_HIP(hipMalloc((void **)&dPrefix, prefix.size() * sizeof(int64_t)));
  STENCIL_HIP(hipMemcpy(dJobs, jobs.data(), jobs.size() * sizeof(FillJob), hipMemcpyHostToDevice));
  STENCIL_HIP(
      hipMemcpy(dPrefix, prefix.data(), prefix.size() * sizeof(int64_t), hipMemcpyHostToDevice));
}

void FillBatch::launch_plain(hipStream_t stream) {
  if (jobs.empty()) return;
  hipLaunchKernelGGL(boundary_fill_kernel, dim3((uint32_t)nBlocks), dim3(kBlock), 0, stream, dJobs,
                     dPrefix, (int)jobs.size());
  STENCIL_HIP(hipGetLastError());
}

void FillBatch::destroy() {
  if (dJobs) (void)hipFree(dJobs);
  if (dPrefix) (void)hipFree(dPrefix);
  dJobs = nullptr;
  dPrefix = nullptr;
}

int64_t ExchangeEngine::add_boundary_fill(int dom, int64_t qi, const Vec3 &dstPos, const Vec3 &ext,
                                          const std::array<BoundaryAxis, 3> &axes,
                                          const std::string &value, int signWidth, int group) {
  if (finalized_) throw std::runtime_error("add_boundary_fill after finalize");
  if (group < 0 || group >= kMaxExchangeGroups)
    throw std::runtime_error("add_boundary_fill: bad group");
  LocalDomain &d = *domains_.at(dom);
  const int64_t es = d.elem_size(qi);
  const Vec3 raw = d.raw_size();
  if (ext.flatten() <= 0) return 0;
  for (int a = 0; a < 3; ++a)
    if (dstPos[a] < 0 || ext[a] < 0 || dstPos[a] + ext[a] > raw[a])
      throw std::runtime_error("add_boundary_fill: region outside the allocation");

  // resolve the z, y, x walk into per-axis affine maps src = A + B * c
  int64_t A[3] = {0, 0, 0}, B[3] = {1, 1, 1};
  bool mapped = false, negate = false, fixed = false;
  for (int a = 2; a >= 0; --a) {
    const BoundaryAxis &ax = axes[a];
    if (ax.kind == Boundary::PERIODIC) continue;
    const bool below = dstPos[a] + ext[a] <= ax.origin;
    const bool above = dstPos[a] >= ax.origin + ax.extent;
    if (!below && !above)
      throw std::runtime_error("add_boundary_fill: region not outside the global domain");
    bool stop = false;
    switch (ax.kind) {
    case Boundary::OPEN:
      if (!mapped) return 0; // the user owns these cells
      stop = true;           // copy from the source mapped so far
      break;
    case Boundary::FIXED:
      fixed = true;
      stop = true;
      break;
    case Boundary::CLAMP:
      if (ax.extent < 1) throw std::runtime_error("add_boundary_fill: CLAMP on an empty extent");
      A[a] = below ? ax.origin : ax.origin + ax.extent - 1;
      B[a] = 0;
      mapped = true;
      break;
    case Boundary::ANTIMIRROR:
      negate = !negate;
      [[fallthrough]];
    case Boundary::MIRROR:
      A[a] = below ? 2 * ax.origin - 1 : 2 * (ax.origin + ax.extent) - 1;
      B[a] = -1;
      mapped = true;
      break;
    default:
      throw std::runtime_error("add_boundary_fill: bad kind");
    }
    if (stop) break;
  }
  if (negate && !(signWidth == es && (es == 2 || es == 4 || es == 8)))
    throw std::runtime_error("add_boundary_fill: ANTIMIRROR needs a 2/4/8-byte float quantity");

  const Pitched &p = d.curr(qi); // pitch/ysize only; base via slot
  FillJob j{};
  j.slot = (char *const *)(d.dev_curr_slots() + qi);
  j.pitch = p.pitch;
  j.plane = p.plane();
  j.dstOff = dstPos.z * p.plane() + dstPos.y * p.pitch + dstPos.x * es;
  j.extY = (int32_t)ext.y;

  char sign[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (negate) sign[es - 1] = (char)0x80; // little-endian IEEE sign bit

  const int64_t rowBytes = ext.x * es;
  int w;
  if (fixed) {
    if ((int64_t)value.size() != es)
      throw std::runtime_error("add_boundary_fill: FIXED value must be elem_size bytes");
    char elem[8];
    std::memcpy(elem, value.data(), es);
    if (negate) elem[es - 1] ^= (char)0x80;
    // broadcast: the widest word the destination permits, whatever ext.x
    w = detail::pick_word(rowBytes, {j.dstOff, j.pitch});
    j.broadcast = 1;
    replicate(elem, es, j.pat);
  } else {
    // every source cell must lie inside this domain's allocation: first
    // and last mapped coordinate per axis (the map is monotone)
    int64_t s0[3];
    for (int a = 0; a < 3; ++a) {
      s0[a] = A[a] + B[a] * dstPos[a];
      const int64_t s1 = A[a] + B[a] * (dstPos[a] + ext[a] - 1);
      if (std::min(s0[a], s1) < 0 || std::max(s0[a], s1) >= raw[a])
        throw std::runtime_error("add_boundary_fill: mirror source outside the allocation "
                                 "(radius larger than the subdomain extent?)");
    }
    j.srcOff = s0[2] * p.plane() + s0[1] * p.pitch + s0[0] * es;
    j.srcSy = B[1] * p.pitch;
    j.srcSz = B[2] * p.plane();
    if (B[0] == 1) {
      // identity x map (pure y/z faces, y-z edges): whole rows move with
      // the widest word the offsets and pitch permit
      w = detail::pick_word(rowBytes, {j.dstOff, j.srcOff, j.pitch});
    } else {
      w = (int)es; // x is mapped: rows are r elements wide, element-wise
    }
    if (w < es) w = (int)es;
    j.srcSx = B[0] * w;
    j.broadcast = 0;
    replicate(sign, es, j.pat);
  }
  j.wordBytes = w;
  j.extXw = (int32_t)(rowBytes / w);
  j.nWords = (int64_t)j.extXw * ext.y * ext.z;

  auto &batch = fillPending_[{group, d.gpu()}];
  batch.dev = d.gpu();
  batch.jobs.push_back(j);
  return ext.flatten() * es;
}

void ExchangeEngine::launch_boundary(int group) {
  auto &fills = fillBatches_[group];
  if (fills.empty()) return;
  roctxRangePush("stencil::boundary");
  // the fill reads halos the translates deliver (possibly from another
  // device's comm stream): one event per translating device, every fill
  // stream waits on all of them. Unpacks share the fill's pack stream.
  std::vector<hipEvent_t> evs;
  for (auto &t : translateBatches_[group]) {
    if (t.jobs.empty()) continue;
    auto it = boundaryEvents_.find(t.dev);
    STENCIL_HIP(hipSetDevice(t.dev));
    if (it == boundaryEvents_.end()) {
      hipEvent_t e;
      STENCIL_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
      it = boundaryEvents_.emplace(t.dev, e).first;
    }
    STENCIL_HIP(hipEventRecord(it->second, comm_stream_(t.dev)));
    evs.push_back(it->second);
  }
  for (auto &b : fills) {
    STENCIL_HIP(hipSetDevice(b.dev));
    hipStream_t s = pack_stream_(b.dev);
    for (hipEvent_t e : evs) STENCIL_HIP(hipStreamWaitEvent(s, e, 0));
    b.launch_plain(s);
  }
  roctxRangePop();
}

void ExchangeEngine::launch_boundary_plain_on(uintptr_t stream, int group) {
  for (auto &b : fillBatches_[group]) b.launch_plain((hipStream_t)stream);
}

} // namespace stencil_amd
