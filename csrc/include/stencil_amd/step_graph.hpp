// Owning base of the whole-step replay graphs (see ops.hpp for the four
// concrete graphs built on it).
#pragma once

#include <atomic>
#include <vector>

#include "stencil_amd/engine.hpp"
#include "stencil_amd/hip_check.hpp"

namespace stencil_amd {

// One domain's captured step: the capture/replay stream, the side streams
// and events its captures fork through, every hipGraphExec_t instantiated
// from them, and the buffer parity the next replay belongs to. The object
// owns all of it and frees it when destroyed. The captured kernargs point
// into the engine's LocalDomain allocations, so a graph must be destroyed
// BEFORE the engine (and with it the domains) it was captured from.
class ReplayGraph {
public:
  ReplayGraph(const ReplayGraph &) = delete;
  ReplayGraph &operator=(const ReplayGraph &) = delete;

  // block until everything launched on the replay stream is done
  void sync() {
    STENCIL_HIP(hipSetDevice(dev_));
    STENCIL_HIP(hipStreamSynchronize(stream_));
  }
  // the replay stream (hipStream_t), for a stream-ordered RcclWire::barrier
  uintptr_t stream() const { return (uintptr_t)stream_; }

  // number of ReplayGraph objects alive in this process (for tests)
  static int alive() { return alive_.load(); }

protected:
  ReplayGraph(ExchangeEngine &eng, int dom, int nSide = 0, int nEvents = 0)
      : eng_(eng), dom_(dom), dev_(eng.domain(dom).gpu()) {
    try {
      STENCIL_HIP(hipSetDevice(dev_));
      STENCIL_HIP(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
      side_.assign(nSide, nullptr);
      for (hipStream_t &s : side_) STENCIL_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
      events_.assign(nEvents, nullptr);
      for (hipEvent_t &e : events_) STENCIL_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    } catch (...) {
      release();
      throw;
    }
    ++alive_;
  }

  // A graph may still be in flight when its owner drops it: wait for the
  // replay stream first. Never throws and ignores HIP errors (this can run
  // during interpreter shutdown), as ~ExchangeEngine does.
  ~ReplayGraph() {
    (void)hipSetDevice(dev_);
    (void)hipStreamSynchronize(stream_);
    release();
    --alive_;
  }

  // Capture what body() enqueues on stream_ (and on side streams forked from
  // it) into a new instantiated graph, owned by this object. If body()
  // throws, the capture is ended and its graph discarded before the
  // exception propagates: the stream is never left capturing.
  template <class Body> hipGraphExec_t capture(Body &&body) {
    STENCIL_HIP(hipStreamBeginCapture(stream_, hipStreamCaptureModeThreadLocal));
    try {
      body();
    } catch (...) {
      hipGraph_t g = nullptr;
      (void)hipStreamEndCapture(stream_, &g);
      if (g) (void)hipGraphDestroy(g);
      (void)hipGetLastError();
      throw;
    }
    execs_.push_back(nullptr);
    end_capture_instantiate(stream_, execs_.back());
    return execs_.back();
  }

  void launch(hipGraphExec_t exec) {
    STENCIL_HIP(hipSetDevice(dev_));
    STENCIL_HIP(hipGraphLaunch(exec, stream_));
  }

  LocalDomain &domain() { return eng_.domain(dom_); }

  ExchangeEngine &eng_;
  const int dom_;
  const int dev_;
  hipStream_t stream_ = nullptr;
  std::vector<hipStream_t> side_;
  std::vector<hipEvent_t> events_;
  int parity_ = 0;

private:
  void release() noexcept {
    for (hipGraphExec_t x : execs_)
      if (x) (void)hipGraphExecDestroy(x);
    for (hipEvent_t e : events_)
      if (e) (void)hipEventDestroy(e);
    for (hipStream_t s : side_)
      if (s) (void)hipStreamDestroy(s);
    if (stream_) (void)hipStreamDestroy(stream_);
  }

  std::vector<hipGraphExec_t> execs_;
  inline static std::atomic<int> alive_{0};
};

} // namespace stencil_amd
