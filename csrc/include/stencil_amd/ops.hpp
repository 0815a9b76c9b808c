// App compute ops (launched on a domain's compute stream).
#pragma once

#include <array>
#include <memory>

#include "stencil_amd/core.hpp"
#include "stencil_amd/engine.hpp"
#include "stencil_amd/step_graph.hpp"

namespace stencil_amd {

// One Jacobi 7-point step of quantity qi over `region` (global coords):
// next = avg of 6 face neighbors of curr, with the reference's hot/cold
// sphere sources fixed inside `computeRegion` (bin/jacobi3d.cu:40-85).
// extendVec enables the pure-vector + LDS-rows fast path (1 = free
// extension, 2 = strict/no-extension for IPC ranks) by
// extending the row to aligned bounds: ONLY valid when every extended
// cell (x-halo cells, pitch-slack bytes, or exterior-shell cells that a
// LATER kernel on the SAME stream rewrites) is discard-safe and the
// domain has radius >= 1 -- the caller asserts this (the overlap
// interior and full-rect launches qualify).
// A row is only ever extended into cells of its own row (x halo, local
// rect) or pitch-slack bytes; where that room is missing the launch is not
// extended. Throws std::invalid_argument, and launches nothing, for an
// unknown domain or quantity, a non-fp32 quantity, an extendVec outside
// 0..2 and a region whose 1-cell apron leaves full_region() (the graph
// creators below check the same).
void jacobi_step(ExchangeEngine &eng, int dom, int64_t qi, const Rect3 &region,
                 const Rect3 &computeRegion, int streamId = 0, int extendVec = 0);
// The kernel jacobi_step launches for these arguments, after the same checks
// and launching nothing: "scalar", "vec4" (16 B strips with scalar head/tail
// lanes), "vec4-all" (the same kernel, pure-vector over the extended row) or
// "lds" (pure-vector, y rows staged in LDS); "none" for an empty region.
const char *jacobi_step_kernel(ExchangeEngine &eng, int dom, int64_t qi, const Rect3 &region,
                               const Rect3 &computeRegion, int extendVec = 0);

// fill an fp32 region with `value` (curr or next buffer); throws
// std::invalid_argument, launching nothing, unless region is inside
// full_region()
void fill_f32(ExchangeEngine &eng, int dom, int64_t qi, const Rect3 &region, float value,
              bool nextBuf);

// Whole-step hipGraph for the single-process single-domain jacobi path:
// [translate copy_batch -> full-region jacobi -> device-side table swap]
// captured once per buffer parity, replayed per step (~5 us host cost vs
// ~0.25 ms of per-step orchestration). launch() enqueues nSteps replays
// (alternating parities, host mirrors flipped); sync() blocks on them.
// A fully periodic single domain gets the wrap graph instead: the stencil
// kernel alone, reading periodic neighbours from the far side of the
// buffer (no translate, no in-graph swap; STENCIL_JAC_WRAP=0 turns it
// off). Halos are then stale after a step until the next exchange.
// is_wrap() tells which of the two the graph is.
// A wrap graph also captures the fused two-step kernel (STENCIL_JAC_FUSE2=0
// turns that off; is_fused2() tells): launch(n) then replays n/2 fused
// graphs and, for odd n, one single step. Every replay, fused or single, is
// one buffer swap, so after a fused pair the result sits in the buffer that
// was `next` and the new `next` holds time t, not t+1.
// Ownership (all four graph classes below): the creator returns the only
// owner; destroying it waits for its stream and frees its streams, events
// and graph execs. A graph must be destroyed before the engine and domains
// it was captured from.
class JacobiStepGraph final : public ReplayGraph {
public:
  void launch(int64_t nSteps);
  bool is_wrap() const { return wrap_; }
  // whether launch(n >= 2) replays fused two-step graphs (see below)
  bool is_fused2() const { return fused2_; }

private:
  friend std::unique_ptr<JacobiStepGraph> jacobi_graph_create(ExchangeEngine &, int, int64_t,
                                                              const Rect3 &, const Rect3 &);
  JacobiStepGraph(ExchangeEngine &eng, int dom, int64_t qi, const Rect3 &region,
                  const Rect3 &computeRegion);
  hipGraphExec_t exec_[2] = {nullptr, nullptr};
  // wrap graph: the stencil kernel alone; the device tables are flipped
  // by launch(), not by a graph node
  bool wrap_ = false;
  // fused pairs: one more graph per parity, each the two-step kernel alone
  hipGraphExec_t exec2_[2] = {nullptr, nullptr};
  bool fused2_ = false;
};
std::unique_ptr<JacobiStepGraph> jacobi_graph_create(ExchangeEngine &eng, int dom, int64_t qi,
                                                     const Rect3 &region,
                                                     const Rect3 &computeRegion);

// Test hook: out[i] = div6(in[i]) (device_util.hpp), computed on the current
// device from host arrays of n floats; blocks until done.
void div6_f32(const float *in, float *out, int64_t n);

// Multi-rank whole-step graphs (see csrc/src/jacobi.hip): per parity,
// A = [interior + translates + staged packs], B = [staged unpacks +
// exterior + device swap]; the caller runs pre() (A), the cross-rank
// barrier (RcclWire::barrier on stream(), or a host barrier with sync()
// around it), then post() (B).
class JacobiMrStepGraph final : public ReplayGraph {
public:
  void pre();
  void post();

private:
  friend std::unique_ptr<JacobiMrStepGraph>
  jacobi_mr_graph_create(ExchangeEngine &, int, int64_t, const Rect3 &, const Rect3 &,
                         const std::vector<Rect3> &, int);
  JacobiMrStepGraph(ExchangeEngine &eng, int dom, int64_t qi, const Rect3 &interior,
                    const Rect3 &computeRegion, const std::vector<Rect3> &exteriors,
                    int extendVec);
  hipGraphExec_t execA_[2] = {nullptr, nullptr};
  hipGraphExec_t execB_[2] = {nullptr, nullptr};
};
std::unique_ptr<JacobiMrStepGraph>
jacobi_mr_graph_create(ExchangeEngine &eng, int dom, int64_t qi, const Rect3 &interior,
                       const Rect3 &computeRegion, const std::vector<Rect3> &exteriors,
                       int extendVec);

// Generic constant-coefficient linear stencil (csrc/src/stencil_op.hip):
//   next[dstQ](p) = sum_k weights[k] * curr[srcQ](p + offsets[k])
// for every p in `region` (global coords), on compute_stream(dom, streamId).
// srcQ == dstQ is allowed (reads curr, writes next). Accumulation is in the
// quantity's own type; weights are rounded to it once, at launch; the
// summation order is unspecified. Unlike jacobi_step's row extension this
// writes NOTHING outside `region` (no halo cell, no pitch slack, no other
// quantity) and reads no cell outside the rows of region (+) offsets, so
// it is safe next to OPEN boundaries, IPC peers and asymmetric radii.
// Star stencils (every tap on an axis) of radius <= 4 over regions at
// least 8 cells wide run the 16 B-strip z-marching kernel; everything else
// runs the linearised tap-table kernel.
// Throws std::invalid_argument when the quantities' element size does not
// match `type`, when region (+) offsets leaves full_region(), or when
// there are 0 or more than 128 taps. An empty region is a no-op.
struct StencilTaps {
  std::vector<Vec3> offsets;
  std::vector<double> weights;
};
enum class StencilType { F32, F64 };
void stencil_apply(ExchangeEngine &eng, int dom, int64_t srcQ, int64_t dstQ, const Rect3 &region,
                   const StencilTaps &taps, StencilType type, int streamId = 0);

// Variable-coefficient diffusion operator (csrc/src/diffusion_op.hip):
//   next[dstQ](p) = sigma u(p) + sum over a in {x,y,z}, s in {-1,+1} of
//                   h[a] * 0.5 (k(p) + k(p + s e_a)) * (u(p) - u(p + s e_a))
// with u = curr[srcQ], k = curr[kQ] (a cell-centred coefficient of the same
// type and layout) and h[a] = 1 / spacing_a^2, for every p in `region`
// (global coords), on compute_stream(dom, streamId). The face coefficient
// is the arithmetic mean of the two cells, so the operator is symmetric.
// Arithmetic is in the quantity's own type; h and sigma are rounded to it
// once, at launch; association and FMA contraction are unspecified.
// stencil_apply's contract: nothing outside `region` is written in any
// buffer, and only the cells of `region` and their six face neighbours, in
// u and in k, enter the arithmetic (no edge or corner cell; the rest of a
// 16 B line that holds a needed cell may be loaded but is never used).
// Regions at least 8 cells wide whose curr[srcQ], curr[kQ] and next[dstQ]
// rows are equally aligned modulo 16 B run the strip kernel, the rest a
// linearised cell kernel. Throws std::invalid_argument, and launches
// nothing, for an unknown domain or quantity, element sizes that do not
// match `type` (4 / 8) or differ, a region outside full_region() or whose
// 1-cell face apron leaves it, a streamId out of range and layouts that
// differ. An empty region is a no-op.
void diffusion_apply(ExchangeEngine &eng, int dom, int64_t srcQ, int64_t kQ, int64_t dstQ,
                     const Rect3 &region, const double h[3], double sigma, StencilType type,
                     int streamId = 0);
// out(p) = omega / diag(p),  diag(p) = sigma + sum over a, s of
// h[a] * 0.5 (k(p) + k(p + s e_a)), in the quantity's type; out is
// (outQ, outNext). The containment contract and validation of
// diffusion_apply. Runs once per coefficient change: one linearised kernel.
void diffusion_inv_diagonal(ExchangeEngine &eng, int dom, int64_t kQ, int64_t outQ, bool outNext,
                            const Rect3 &region, const double h[3], double sigma, double omega,
                            int streamId = 0);

// Vector operations on pitched quantities (csrc/src/vector_ops.hip): the
// building blocks of Krylov solvers. Every op works on a global-coordinate
// `region` of one local domain, on float32 or float64 quantities (all
// operands of one op of the same type), on compute_stream(dom, streamId).
// An operand is (quantity index, nextBuf). Nothing outside `region` is
// written in any buffer and no cell outside it enters the arithmetic.
// Regions at least 8 cells wide whose operand rows are equally aligned run
// on 16 B strips aligned by address with scalar head/tail lanes; the rest
// runs linearised. All throw std::invalid_argument, and launch nothing,
// for an unknown domain or quantity, an element size other than 4 or 8 or
// one that differs between operands, and a region outside full_region().
// An empty region is a no-op (reductions return 0).
//
// The reductions are deterministic: per-wave shuffles, per-block LDS, one
// partial per block, partials summed in index order on the host; the same
// input on the same launch shape gives the same bits. They use the
// engine's per-domain scratch (no allocation per call) and block the host
// once. With several local domains, call the *_begin form on each, then
// reduction_end on each: one reduction per domain may be in flight.

// sum over region of a(p) * b(p); products and sums in fp64
double field_dot(ExchangeEngine &eng, int dom, int64_t a, bool aNext, int64_t b, bool bNext,
                 const Rect3 &region, int streamId = 0);
void field_dot_begin(ExchangeEngine &eng, int dom, int64_t a, bool aNext, int64_t b, bool bNext,
                     const Rect3 &region, int streamId = 0);
// out = alpha * x + beta * y in the quantity's type (alpha, beta rounded to
// it once at launch; FMA contraction unspecified). out may be the buffer
// of x or of y: the op is element-wise.
void field_axpby(ExchangeEngine &eng, int dom, double alpha, int64_t x, bool xNext, double beta,
                 int64_t y, bool yNext, int64_t out, bool outNext, const Rect3 &region,
                 int streamId = 0);
// out = alpha * x + beta * y + gamma * z, the three-operand form of
// field_axpby (4 passes where two axpby calls take 6): the relaxation
// update e += w (f - A e) of the multigrid smoother. out may be the buffer
// of any input.
void field_axpbypcz(ExchangeEngine &eng, int dom, double alpha, int64_t x, bool xNext,
                    double beta, int64_t y, bool yNext, double gamma, int64_t z, bool zNext,
                    int64_t out, bool outNext, const Rect3 &region, int streamId = 0);
// out = alpha * x + d * (beta * y + gamma * z) with d a quantity (5 passes):
// the diagonally scaled relaxation update e += (omega / diag) (f - A e) of
// the variable-coefficient smoother. With aliased operands also the first
// sweep e = d f (alpha = 0, gamma = 0) and the Jacobi preconditioner
// z = d r. out may be the buffer of any input.
void field_scaled_update(ExchangeEngine &eng, int dom, double alpha, int64_t x, bool xNext,
                         int64_t d, bool dNext, double beta, int64_t y, bool yNext, double gamma,
                         int64_t z, bool zNext, int64_t out, bool outNext, const Rect3 &region,
                         int streamId = 0);
// fused conjugate-gradient update, one pass instead of three:
//   curr[x] += alpha * curr[p];  curr[r] -= alpha * next[p]
// returning sum r_new^2 (fp64 accumulation of the rounded r_new). next[p]
// is where stencil_apply(A, p, p) leaves A p. x, p and r are distinct.
double cg_update(ExchangeEngine &eng, int dom, double alpha, int64_t x, int64_t p, int64_t r,
                 const Rect3 &region, int streamId = 0);
void cg_update_begin(ExchangeEngine &eng, int dom, double alpha, int64_t x, int64_t p, int64_t r,
                     const Rect3 &region, int streamId = 0);
// wait for the reduction begun on `dom` and return its value. For the
// one-valued ops; std::runtime_error (the reduction stays in flight) when
// the one in flight has more values.
double reduction_end(ExchangeEngine &eng, int dom);

// The reductions of singular problems: the projection v - mean(v) onto the
// complement of the constant null space, fused into passes a Krylov
// iteration makes anyway. The contract, the walks, the validation and the
// determinism of the ops above; a reduction with several values writes one
// partial per block AND value (the scratch holds kReduceValues *
// kReducePartials doubles, value-major) and the host sums each value's
// partials in index order. The launch shapes are those of the ops above.
//
// sum over region of a(p), in fp64: one read pass
double field_sum(ExchangeEngine &eng, int dom, int64_t a, bool aNext, const Rect3 &region,
                 int streamId = 0);
void field_sum_begin(ExchangeEngine &eng, int dom, int64_t a, bool aNext, const Rect3 &region,
                     int streamId = 0);
// (sum a * b, sum a, sum b) from ONE pass over a and b, field_dot's traffic;
// products and sums in fp64. a and b may be the same buffer.
std::array<double, 3> field_dot_sums(ExchangeEngine &eng, int dom, int64_t a, bool aNext,
                                     int64_t b, bool bNext, const Rect3 &region,
                                     int streamId = 0);
void field_dot_sums_begin(ExchangeEngine &eng, int dom, int64_t a, bool aNext, int64_t b,
                          bool bNext, const Rect3 &region, int streamId = 0);
// cg_update (the same arithmetic, the same single rounding of alpha; x, p
// and r distinct) returning (sum r_new^2, sum r_new): cg_update's traffic
std::array<double, 2> cg_update_sum(ExchangeEngine &eng, int dom, double alpha, int64_t x,
                                    int64_t p, int64_t r, const Rect3 &region, int streamId = 0);
void cg_update_sum_begin(ExchangeEngine &eng, int dom, double alpha, int64_t x, int64_t p,
                         int64_t r, const Rect3 &region, int streamId = 0);
// out = alpha * x + beta * y + c in the quantity's type (alpha, beta and c
// rounded to it once at launch; FMA contraction and association
// unspecified, as for field_axpby). out may be the buffer of x or of y.
// field_axpby's traffic.
void field_axpbyc(ExchangeEngine &eng, int dom, double alpha, int64_t x, bool xNext, double beta,
                  int64_t y, bool yNext, double c, int64_t out, bool outNext,
                  const Rect3 &region, int streamId = 0);

// The fused passes of BiCGStab (stencil_amd/solvers/bicgstab.py), the
// Krylov method for non-symmetric operators. The contract, the walks, the
// validation and the determinism of the ops above; the launch shapes are
// theirs too, so a value that an op above also computes has the same bits.
//
// out = alpha * x + beta * y as field_axpby writes it, returning sum out^2
// of the stored (rounded) out, squares and sums in fp64: field_axpby's 3
// passes, no fourth for the norm. out may be the buffer of x or of y.
double field_axpby_norm2(ExchangeEngine &eng, int dom, double alpha, int64_t x, bool xNext,
                         double beta, int64_t y, bool yNext, int64_t out, bool outNext,
                         const Rect3 &region, int streamId = 0);
void field_axpby_norm2_begin(ExchangeEngine &eng, int dom, double alpha, int64_t x, bool xNext,
                             double beta, int64_t y, bool yNext, int64_t out, bool outNext,
                             const Rect3 &region, int streamId = 0);
// (sum a * b, sum a * a) from ONE pass over a and b: field_dot's traffic
std::array<double, 2> field_dot_pair(ExchangeEngine &eng, int dom, int64_t a, bool aNext,
                                     int64_t b, bool bNext, const Rect3 &region,
                                     int streamId = 0);
void field_dot_pair_begin(ExchangeEngine &eng, int dom, int64_t a, bool aNext, int64_t b,
                          bool bNext, const Rect3 &region, int streamId = 0);
// the fused BiCGStab update, one pass of 8 (7 when z is the buffer of r)
// instead of 11:
//   curr[x] += alpha * y + omega * z;  curr[r] -= omega * t
// returning (sum r_new^2, sum rhat * r_new), fp64 accumulation of the
// rounded r_new. On entry curr[r] holds s. alpha and omega are rounded to
// the quantity's type once. z may be the buffer of r: every cell is read
// before it is written. curr[x] and curr[r] must be distinct from each
// other and from the buffers of y, t and rhat (std::invalid_argument).
std::array<double, 2> bicgstab_update(ExchangeEngine &eng, int dom, double alpha, int64_t y,
                                      bool yNext, double omega, int64_t z, bool zNext, int64_t x,
                                      int64_t r, int64_t t, bool tNext, int64_t rhat,
                                      bool rhatNext, const Rect3 &region, int streamId = 0);
void bicgstab_update_begin(ExchangeEngine &eng, int dom, double alpha, int64_t y, bool yNext,
                           double omega, int64_t z, bool zNext, int64_t x, int64_t r, int64_t t,
                           bool tNext, int64_t rhat, bool rhatNext, const Rect3 &region,
                           int streamId = 0);

// wait for the n-valued reduction begun on `dom` and write its values to
// out[0..n): n = 1 field_sum (and the one-valued ops above), 2
// cg_update_sum, field_dot_pair and bicgstab_update, 3 field_dot_sums. std::runtime_error, the reduction
// staying in flight, when the one in flight has another value count;
// std::invalid_argument for n outside 1..kReduceValues or a null out.
void reduction_end_n(ExchangeEngine &eng, int dom, double *out, int n);

// Grid transfer between a fine and a coarse local domain on cell-centred
// 2:1 coarsening (csrc/src/grid_transfer.hip): coarse cell c has the 8 fine
// children 2c + {0,1}^3, all coordinates global. The two domains may belong
// to different engines but sit on one device; the kernel is enqueued on
// compute_stream(dom, streamId) of the DESTINATION engine, and the caller
// orders it behind the source engine's work (sync_compute). float32 /
// float64 quantities, all operands of one type; an operand is (quantity,
// nextBuf). The contract of the vector operations holds: nothing outside
// the region is written in any buffer, and no cell outside it (for the
// restriction: outside the children of the region) is loaded, so halos may
// hold NaN. Both throw std::invalid_argument, and launch nothing, for an
// unknown domain or quantity, an element size other than 4 or 8 or mixed
// element sizes, a coarse region outside the coarse full_region() or whose
// doubled box [2 lo, 2 hi) leaves the fine full_region(), and domains on
// different devices. An empty region is a no-op.
//
// out(c) = 0.125 * sum over the children p of c of (alpha a(p) + beta b(p)),
// in the quantity's type (alpha, beta rounded to it once; summation order
// and FMA contraction unspecified). Two operands, so that a residual
// f - A e is restricted without being written out first.
void grid_restrict(ExchangeEngine &fine, int fdom, double alpha, int64_t a, bool aNext,
                   double beta, int64_t b, bool bNext, ExchangeEngine &coarse, int cdom,
                   int64_t out, bool outNext, const Rect3 &coarseRegion, int streamId = 0);
// dst(p) += src(p >> 1) for every fine cell p of [2 lo, 2 hi): piecewise-
// constant injection, 8 x the transpose of the restriction above.
void grid_prolong_add(ExchangeEngine &coarse, int cdom, int64_t src, bool srcNext,
                      ExchangeEngine &fine, int fdom, int64_t dst, bool dstNext,
                      const Rect3 &coarseRegion, int streamId = 0);

// physical coefficients of the MHD solver (see csrc/src/mhd.hip)
struct MhdCoeffs {
  double dsx = 1.0, dsy = 1.0, dsz = 1.0;
  double cs2 = 1.0;
  double cp_inv = 1.0;
  double nu = 5e-3, eta = 5e-3, chi = 5e-4;
};

// one RK3 substep (step in 0..2) of the 8-field 6th-order MHD system over
// `region` (global coords); reads curr, updates next in place (Williamson
// two-buffer form) -- caller swaps after each substep
// Separable-derivative MHD: the domain carries 10 fp64 quantities
// (8 physics fields + div u + div A). Per substep the app runs
//   exchange() -> mhd_div_pass -> exchange() -> mhd_substep
// so grad(div .) reduces to first derivatives of the exchanged div fields.
void mhd_div_pass(ExchangeEngine &eng, int dom, const Rect3 &region, const MhdCoeffs &cf,
                  int streamId = 0);
// Whole-substep hipGraphs for the world=1 single-domain astaroth shape:
// per RK3 substep and buffer parity, [X1 translates -> div -> X2
// translates -> scalar || momentum -> table swap] captured once;
// iter() replays 3*nIters substep graphs (host mirrors flipped).
class MhdStepGraph final : public ReplayGraph {
public:
  void iter(int64_t nIters = 1);

private:
  friend std::unique_ptr<MhdStepGraph> mhd_graph_create(ExchangeEngine &, int, const Rect3 &,
                                                        double, const MhdCoeffs &);
  MhdStepGraph(ExchangeEngine &eng, int dom, const Rect3 &region, double dt,
               const MhdCoeffs &cf);
  hipGraphExec_t exec_[3][2] = {};
};
std::unique_ptr<MhdStepGraph> mhd_graph_create(ExchangeEngine &eng, int dom, const Rect3 &region,
                                               double dt, const MhdCoeffs &cf);

// Multi-rank substep graphs (see csrc/src/mhd.hip): per substep the
// caller runs phase1 / barrier / phase2 / barrier / phase3 (barrier =
// RcclWire::barrier on stream(), or a host barrier with a sync() before
// it).
class MhdMrStepGraph final : public ReplayGraph {
public:
  void phase1();
  void phase2();
  void phase3();

private:
  friend std::unique_ptr<MhdMrStepGraph> mhd_mr_graph_create(ExchangeEngine &, int, const Rect3 &,
                                                            const std::vector<Rect3> &, double,
                                                            const MhdCoeffs &);
  MhdMrStepGraph(ExchangeEngine &eng, int dom, const Rect3 &interior,
                 const std::vector<Rect3> &exteriors, double dt, const MhdCoeffs &cf);
  hipGraphExec_t g1_[2] = {};
  hipGraphExec_t g2_[3][2] = {};
  hipGraphExec_t g3_[3][2] = {};
  int substep_ = 0;
};
std::unique_ptr<MhdMrStepGraph> mhd_mr_graph_create(ExchangeEngine &eng, int dom,
                                                    const Rect3 &interior,
                                                    const std::vector<Rect3> &exteriors,
                                                    double dt, const MhdCoeffs &cf);

void mhd_substep(ExchangeEngine &eng, int dom, const Rect3 &region, int step, double dt,
                 const MhdCoeffs &cf, int streamId = 0);

// fill an fp64 region with base + amp*sin(kx*x + ky*y + kz*z + phase)
// (deterministic smooth initial conditions, reproducible in NumPy)
void init_harmonic_f64(ExchangeEngine &eng, int dom, int64_t qi, const Rect3 &region, double base,
                       double amp, double kx, double ky, double kz, double phase, bool nextBuf);
// radial gaussian bump around (cx,cy,cz) (reference astaroth.cu
// radial_explosion_init_kernel): base + amp*exp(-r^2/(2 sigma^2))
void init_radial_f64(ExchangeEngine &eng, int dom, int64_t qi, const Rect3 &region, double base,
                     double amp, double cx, double cy, double cz, double sigma, bool nextBuf);

// min/max/RMS of a quantity over a region (reference: reductions.cuh)
struct FieldStats {
  double min, max, rms;
};
FieldStats field_stats(ExchangeEngine &eng, int dom, int64_t qi, const Rect3 &region,
                       bool nextBuf = false);

} // namespace stencil_amd
