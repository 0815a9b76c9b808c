"""Conjugate gradients for A x = b with A a symmetric positive definite
stencil operator.

The operator is a `Stencil` applied by `DistributedDomain.apply_stencil`, or
a `DiffusionOperator` (solvers/diffusion.py: sigma I - div(k grad) with a
coefficient field k, whose halos the caller keeps current with refresh());
the halo exchange and the boundary fill of the quantity `p` supply the
neighbour values, so the domain's boundary kinds ARE the discrete boundary
conditions of A. The solver never calls `dd.swap()`: `A p` lives in the
next buffer of `p`, where apply_stencil leaves it, so four quantities
(x, b, r, p) are all the storage there is.

    r = b            (x0_zero)   or   exchange(group_x); next[x] = A x; r = b - next[x]
    p = r; rr = dot(r, r); bb = dot(b, b)
    repeat:  interior(A, p) || exchange(group_p); exterior; sync    -> next[p] = A p
             alpha = rr / dot(p, Next(p))
             rr_new = cg_update(alpha, x, p, r)
             stop if rr_new <= tol^2 * bb
             p = r + (rr_new / rr) * p ;  rr = rr_new

With a preconditioner M (any object with apply(r, z) leaving z = M r, M
symmetric positive definite; solvers/multigrid.py) and a fifth quantity z:

    z = M r; p = z; rz = dot(r, z)
    repeat:  next[p] = A p;  alpha = rz / dot(p, Next(p))
             rr_new = cg_update(alpha, x, p, r);  stop if rr_new <= tol^2 * bb
             z = M r; rz_new = dot(r, z);  p = z + (rz_new / rz) * p

Without one the code path is the loop above, unchanged.

With a `correction` quantity d the solver also verifies what it returns.
The recursive r drifts from b - A x by the roundings of x += alpha p; when
||x|| is large against ||b|| (a nearly singular A: a small sigma on a
periodic or MIRROR box) a float32 solve "converges" with a true residual
several times the tolerance. So after convergence:

    repeat:  exchange(group_x); r = b - A x;  done if ||r|| <= tol ||b||
             d = 0; CG (as above) on A d = r to the same absolute threshold
             x = x + d

which rounds x once per correction instead of once per iteration
(iterative refinement in the working precision; a correction solve takes a
handful of iterations). Without `correction` nothing of this runs.

Boundary conditions. CG needs A symmetric, and linear and homogeneous in
the field: PERIODIC, FIXED(0), MIRROR and ANTIMIRROR qualify (for star
stencils: `u . A v == v . A u` was checked to rounding for the Laplacians
of order 2, 4 and 8 under each of them; for stencils with edge or corner
taps under non-periodic boundaries symmetry is not vouched for). OPEN,
CLAMP and FIXED(c != 0) are refused. Inhomogeneous Dirichlet data is the
caller's job: fold it into b (b -= A applied to the field that holds the
boundary values in its halo and 0 inside).

Singular problems. With every axis PERIODIC or MIRROR and no sigma the
constant is in the null space of A: A x = b has a solution only for
mean(b) = 0, and then a family x + c. `nullspace="constant"` makes the
solver own the projection P v = v - mean(v): it solves A x = P b and
returns the x with mean(x) = 0. A right-hand side with a mean (every
discretised source has one) would otherwise end in a breakdown, and a
smoother that scales per cell (the variable-coefficient multigrid) would
feed a constant into p and x that eats mantissa. The projection adds no
pass to the iteration; it rides on the passes the loop makes anyway:

    r = b - mean(b)                      one sum, one axpbyc; bb = dot(r)
    plain:  (rr, sr) = cg_update_sum(alpha, x, p, r)
            rr_p = rr - sr^2 / N         = (P r) . (P r): stopping test, beta
            p = r + beta p - sr / N      one axpbyc in the place of the axpby
    with M: z = M r; (rz, sr, sz) = dot_sums(r, z)
            rz_p = rz - sr sz / N        = (P r) . (P z): alpha, beta
            p = z + beta p - sz / N      (the stopping test stays on r . r)
    x -= mean(x)                         once, on the way out

with N the global cell count. bb is the norm of P b itself, never
b . b - (sum b)^2 / N, which cancels. The correction loop checks
P (b - A x) and projects x after the last x += d. GeometricMultigrid runs
on such operators as it is (see its module docstring).

Every scalar the iteration branches on comes from `dd.dot` /
`dd.cg_update` and their *_sum(s) forms, which return the bitwise identical value on every rank, so
all ranks stop in the same iteration for the same reason.
"""
from __future__ import annotations

import math
import time
from typing import Optional

import numpy as np

from ..boundary import Boundary
from ..core import DataHandle, DistributedDomain, Next
from ..stencil import Stencil
from ._common import (  # noqa: F401  (CGResult and check_radius are re-exported)
    CGResult,
    check_faces,
    check_quantities,
    check_radius,
    operator_apply,
    overlapped_apply,
)


def check_operator(who: str, dd: DistributedDomain, operator):
    """ValueError unless the operator (a Stencil or a DiffusionOperator) is
    symmetric and dd's radius covers it"""
    if not isinstance(operator, Stencil):
        from .diffusion import DiffusionOperator

        if not isinstance(operator, DiffusionOperator):
            raise ValueError(f"{who}: the operator is a Stencil or a DiffusionOperator")
        if operator.dd is not dd:
            raise ValueError(f"{who}: the DiffusionOperator belongs to another domain")
    if not operator.is_symmetric():
        raise ValueError(f"{who}: the stencil is not symmetric (w(o) != w(-o))")
    check_radius(who, dd, operator)


def check_boundary(who: str, dd: DistributedDomain, handles):
    """ValueError unless every non-periodic face of the given quantities is
    FIXED(0), MIRROR or ANTIMIRROR"""
    check_faces(f"{who}: ", dd, handles, (Boundary.FIXED, Boundary.MIRROR, Boundary.ANTIMIRROR),
                ": the operator must be symmetric, linear and homogeneous (PERIODIC, FIXED(0), "
                "MIRROR or ANTIMIRROR); fold inhomogeneous boundary data into b")


def check_constant_nullspace(who: str, dd: DistributedDomain, operator, handles):
    """ValueError unless the constant is in the null space of A: every face
    of the given quantities PERIODIC or MIRROR, and an operator without a
    zeroth-order term"""
    check_faces(f"{who}: nullspace='constant' but ", dd, handles, (Boundary.MIRROR,),
                " pins the constant: A is not singular (every face must be PERIODIC or MIRROR)")
    if isinstance(operator, Stencil):
        total = math.fsum(operator.weights)
        scale = math.fsum(abs(w) for w in operator.weights)
        if not abs(total) <= 64.0 * float(np.finfo(np.float64).eps) * scale:
            raise ValueError(
                f"{who}: nullspace='constant' but the stencil's weights sum to {total!r}, "
                "not 0: the constant is not in the null space of A")
    elif float(operator.sigma) != 0.0:
        raise ValueError(
            f"{who}: nullspace='constant' but the DiffusionOperator has sigma = "
            f"{operator.sigma!r} != 0: A is not singular")


class ConjugateGradient:
    def __init__(self, dd: DistributedDomain, operator, x: DataHandle, b: DataHandle,
                 r: DataHandle, p: DataHandle, group_p: int = 0,
                 group_x: Optional[int] = None, preconditioner=None,
                 z: Optional[DataHandle] = None, correction: Optional[DataHandle] = None,
                 nullspace: Optional[str] = None):
        """dd is realized and holds x, b, r and p, four distinct quantities
        of one float type. operator is a Stencil or a DiffusionOperator of
        dd (of the same float type). group_p is the exchange group that
        moves p's halos (every iteration); group_x the one that moves x's (needed for
        solve(x0_zero=False) only). Raises ValueError for a non-symmetric
        stencil, a domain radius that does not cover it, mixed dtypes and a
        boundary kind on p or x other than PERIODIC, FIXED(0), MIRROR or
        ANTIMIRROR.

        preconditioner: None (plain CG), or any object with apply(r, z)
        that leaves z = M r in curr[z] for a symmetric positive definite M
        and reads r only (solvers/multigrid.py). It needs z, a fifth
        distinct quantity of the same type.

        correction: None, or one more distinct quantity of the same type.
        solve() then verifies the TRUE residual b - A x once the recursive
        one has converged, and refines until it meets the tolerance too
        (see solve()). Needs group_x.

        nullspace: None, or "constant" for a singular A whose null space is
        the constants: solve() then solves A x = P b, P v = v - mean(v),
        and returns the solution with mean(x) = 0 (module docstring).
        ValueError unless A is such an operator: every face of p and x
        PERIODIC or MIRROR, a DiffusionOperator with sigma == 0, a Stencil
        whose weights sum to zero (to 64 eps of their absolute sum: the
        Laplacian factories round their weights)."""
        if nullspace not in (None, "constant"):
            raise ValueError(
                f"ConjugateGradient: nullspace is None or 'constant', got {nullspace!r}")
        who = "ConjugateGradient"
        if preconditioner is not None and not callable(getattr(preconditioner, "apply", None)):
            raise ValueError(f"{who}: the preconditioner has no apply(r, z)")
        if correction is not None and group_x is None:
            raise ValueError(f"{who}: correction needs group_x, the exchange group of x")
        groups = [(p, group_p, f"p is not in exchange group {group_p}")]
        if group_x is not None:
            groups.append((x, group_x, f"x is not in exchange group {group_x}"))
        check_quantities(
            who, dd, (("x", x), ("b", b), ("r", r), ("p", p)),
            optional=((preconditioner is not None, (z,),
                       "a preconditioner needs z, a fifth distinct quantity",
                       "z is given but no preconditioner"),
                      (correction is not None, (correction,),
                       "correction must be one more distinct quantity", None)),
            groups=groups)
        check_operator(who, dd, operator)
        if not isinstance(operator, Stencil) and operator.k.dtype != x.dtype:
            raise ValueError(f"{who}: the coefficient is {operator.k.dtype}, the unknown {x.dtype}")
        check_boundary(who, dd, (p, x))
        if nullspace is not None:
            check_constant_nullspace(who, dd, operator, (p, x))
        self.nullspace = nullspace
        self._cells = float(dd.size[0]) * float(dd.size[1]) * float(dd.size[2])  # N
        self._bb = 0.0  # ||P b||^2 of the last nullspace solve, for _refine
        self.dd, self.A = dd, operator
        self.x, self.b, self.r, self.p = x, b, r, p
        self.group_p, self.group_x = group_p, group_x
        # host wall time per phase of the last solve (each phase ends in a
        # host sync): operator = apply + exchange, dot = p . A p,
        # update = cg_update + the p update
        self.phase_times = {"operator": 0.0, "dot": 0.0, "update": 0.0}
        self.M, self.z, self.correction = preconditioner, z, correction
        self.corrections = 0  # correction solves of the last solve()
        if preconditioner is not None:
            self.phase_times["precond"] = 0.0  # z = M r and r . z

    def _apply(self, h: DataHandle, group: int, overlap: bool):
        """next[h] = A curr[h] on every local domain, halos refreshed"""
        dd = self.dd
        overlapped_apply(dd, lambda where: operator_apply(dd, self.A, h, where), group, overlap)
        dd.backend.sync_compute()

    def solve(self, tol: float = 1e-6, max_iter: int = 1000, x0_zero: bool = True,
              overlap: bool = True) -> CGResult:
        """iterate until ||r|| <= tol * ||b|| (recursive residual) or
        max_iter. x0_zero=True starts from x = 0 (x's content is
        overwritten); False starts from curr[x] and needs group_x.
        b = 0 gives x = 0 in 0 iterations. A non-positive or non-finite
        p . A p ends the solve with converged=False, reason="breakdown".

        With a `correction` quantity d the recursive residual is not
        trusted: in the quantity's type it drifts from b - A x by the
        roundings of x += alpha p, visibly so when ||x|| is large against
        ||b|| (a nearly singular A in float32). Once it has converged,
        r = b - A x is computed; if ||r|| <= tol ||b|| the solve is done
        (the last entry of `residuals` is then this true residual).
        Otherwise A d = r is solved from d = 0 to the same absolute
        threshold, x += d (one rounding of x instead of one per iteration)
        and the check is repeated. The iterations of the correction solves
        count and are limited by max_iter like the others. A true residual
        that a correction does not bring below 0.9 x the previous one ends
        the solve with converged=False, reason="stagnated": the tolerance
        is then below what the type can resolve.

        With nullspace="constant" everything above holds with P b in the
        place of b and P (b - A x) in the place of the true residual:
        `residuals` and the stopping test are relative to ||P b||, a
        constant b gives "zero_rhs", b is never written, and x is
        projected (x -= mean(x)) on every exit that returns a solution."""
        self.corrections = 0
        res = self._solve(tol, max_iter, x0_zero, overlap)
        if res.reason == "zero_rhs":
            return res
        if self.correction is not None and res.converged:
            res = self._refine(res, tol, max_iter, overlap)
        if self.nullspace is not None:
            self._project(self.x)
        return res

    def _project(self, h: DataHandle):
        """h -= mean(h): one sum and one axpbyc"""
        dd = self.dd
        s = dd.sum(h)
        dd.axpbyc(1.0, h, 0.0, h, -s / self._cells, out=h)
        dd.backend.sync_compute()

    def _refine(self, res: CGResult, tol, max_iter, overlap) -> CGResult:
        dd, x, b, r, p, d = self.dd, self.x, self.b, self.r, self.p, self.correction
        ns = self.nullspace is not None
        bb = self._bb if ns else dd.dot(b)
        limit = tol * tol * bb
        residuals, its, prev = list(res.residuals), res.iterations, None
        while True:
            self._apply(x, self.group_x, overlap)
            dd.axpby(1.0, b, -1.0, Next(x), out=r)
            if ns:  # the true residual is P (b - A x); b carries its mean
                self._project(r)
            rr = dd.dot(r)
            if not math.isfinite(rr):
                return CGResult(False, its, residuals[:-1] + [float("nan")], "breakdown")
            residuals[-1] = math.sqrt(rr / bb)
            if rr <= limit:
                return CGResult(True, its, residuals, "converged")
            if prev is not None and rr > 0.81 * prev:  # squares: 0.9 in norm
                return CGResult(False, its, residuals, "stagnated")
            if its >= max_iter:
                return CGResult(False, its, residuals, "max_iter")
            prev = rr
            self.corrections += 1
            dd.axpby(0.0, r, 0.0, r, out=d)
            dd.axpby(1.0, r, 0.0, r, out=p)
            dd.backend.sync_compute()
            self.x = d  # _iterate updates self.x
            try:
                inner = self._iterate(rr, limit, bb, residuals, max_iter - its, overlap)
            finally:
                self.x = x
            dd.axpby(1.0, x, 1.0, d, out=x)
            dd.backend.sync_compute()
            its, residuals = its + inner.iterations, list(inner.residuals)
            if not inner.converged:
                return CGResult(False, its, residuals, inner.reason)

    def _solve(self, tol, max_iter, x0_zero, overlap) -> CGResult:
        """the set-up, then _iterate. nullspace="constant": for A x = P b,
        with r = P b first and bb = r . r of that r, the norm every
        residual is relative to."""
        dd, x, b, r, p = self.dd, self.x, self.b, self.r, self.p
        ns = self.nullspace is not None
        self.phase_times = {k: 0.0 for k in self.phase_times}
        if not x0_zero and self.group_x is None:
            raise ValueError("solve(x0_zero=False) needs group_x, the exchange group of x")
        rhs = b
        if ns:
            sb = dd.sum(b)
            if not math.isfinite(sb):
                return CGResult(False, 0, [float("nan")], "breakdown")
            dd.axpbyc(1.0, b, 0.0, b, -sb / self._cells, out=r)
            rhs = r
        bb = dd.dot(rhs)
        if not math.isfinite(bb):
            return CGResult(False, 0, [float("nan")], "breakdown")
        self._bb = bb
        if bb == 0.0:
            dd.axpby(0.0, rhs, 0.0, rhs, out=x)  # the right-hand side is all zeros: so is x
            dd.backend.sync_compute()
            return CGResult(True, 0, [0.0], "zero_rhs")
        if x0_zero:
            dd.axpby(0.0, rhs, 0.0, rhs, out=x)
            if ns:
                rr = bb
            else:
                dd.axpby(1.0, b, 0.0, b, out=r)
        else:
            self._apply(x, self.group_x, overlap)
            dd.axpby(1.0, rhs, -1.0, Next(x), out=r)
            if ns:
                self._project(r)
                rr = dd.dot(r)
        dd.axpby(1.0, r, 0.0, r, out=p)
        if not ns:
            rr = dd.dot(r)
        dd.backend.sync_compute()  # the exchange reads p on other streams
        residuals = [math.sqrt(rr / bb)] if math.isfinite(rr) else [float("nan")]
        if not math.isfinite(rr):
            return CGResult(False, 0, residuals, "breakdown")
        limit = tol * tol * bb
        if rr <= limit:
            return CGResult(True, 0, residuals, "converged")
        return self._iterate(rr, limit, bb, residuals, max_iter, overlap)

    def _precondition(self):
        """z = M r; returns (r . z, None), or with nullspace="constant"
        ((P r) . (P z), -sum z / N) from one dot_sums pass"""
        t0 = time.perf_counter()
        self.M.apply(self.r, self.z)
        if self.nullspace is None:
            rz, shift = self.dd.dot(self.r, self.z), None
        else:
            rz, sr, sz = self.dd.dot_sums(self.r, self.z)
            rz, shift = rz - sr * sz / self._cells, -sz / self._cells
        self.phase_times["precond"] += time.perf_counter() - t0
        return rz, shift

    def _set_p(self, v: DataHandle, beta: float, y: DataHandle, shift: Optional[float]):
        """p = v + beta y, plus the constant `shift` unless it is None"""
        if shift is None:
            self.dd.axpby(1.0, v, beta, y, out=self.p)
        else:
            self.dd.axpbyc(1.0, v, beta, y, shift, out=self.p)
        self.dd.backend.sync_compute()  # before the next exchange reads p

    def _iterate(self, rho, limit, bb, residuals, max_iter, overlap) -> CGResult:
        """the loop from p = r and rho = r . r; updates self.x.

        With a preconditioner z = M r stands in the place of r: p = z,
        rho = r . z, alpha = rho / p.Ap, beta = rho' / rho. The stopping
        test and `residuals` stay on r . r, which cg_update still returns.
        A non-finite or non-positive r . z (M not positive definite) is a
        breakdown.

        With nullspace="constant" p starts mean-free and stays so at no
        pass more. Plain: cg_update_sum returns sum r next to r . r;
        (P r) . (P r) drives the stopping test and beta, and
        p = P r + beta p is one axpbyc. Preconditioned: P z stands in the
        place of z, since M r has a constant component even for a
        mean-free r (a smoother that scales per cell) which must reach
        neither p nor x; the stopping test stays on cg_update's r . r and
        the breakdown rules apply to the projected r . z."""
        dd, x, r, p, n = self.dd, self.x, self.r, self.p, self._cells
        pre = self.M is not None
        summed = self.nullspace is not None and not pre  # cg_update_sum in the place of cg_update
        v, shift = r, None  # what p is built from: r or z, and the constant that projects it
        if pre:
            v = self.z
            rho, shift = self._precondition()
            if not (math.isfinite(rho) and rho > 0.0):
                return CGResult(False, 0, residuals, "breakdown")
            self._set_p(v, 0.0, v, shift)
        for it in range(1, max_iter + 1):
            t0 = time.perf_counter()
            self._apply(p, self.group_p, overlap)
            t1 = time.perf_counter()
            pap = dd.dot(p, Next(p))
            t2 = time.perf_counter()
            self.phase_times["operator"] += t1 - t0
            self.phase_times["dot"] += t2 - t1
            if not (math.isfinite(pap) and pap > 0.0):
                return CGResult(False, it - 1, residuals, "breakdown")
            if summed:
                rr_raw, sr = dd.cg_update_sum(rho / pap, x, p, r)
                rr_new, shift = max(rr_raw - sr * sr / n, 0.0), -sr / n
            else:
                rr_new = dd.cg_update(rho / pap, x, p, r)
            self.phase_times["update"] += time.perf_counter() - t2
            if not math.isfinite(rr_new):
                return CGResult(False, it, residuals + [float("nan")], "breakdown")
            residuals.append(math.sqrt(rr_new / bb))
            if rr_new <= limit:
                return CGResult(True, it, residuals, "converged")
            rho_new = rr_new
            if pre:
                rho_new, shift = self._precondition()
                if not (math.isfinite(rho_new) and rho_new > 0.0):
                    return CGResult(False, it, residuals, "breakdown")
            t3 = time.perf_counter()
            self._set_p(v, rho_new / rho, p, shift)
            rho = rho_new
            self.phase_times["update"] += time.perf_counter() - t3
        return CGResult(False, max_iter, residuals, "max_iter")
