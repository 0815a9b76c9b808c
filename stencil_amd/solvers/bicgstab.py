"""BiCGStab for A x = b with A any constant-coefficient stencil operator:
the Krylov method for the non-symmetric problems conjugate gradients
refuses (advection-diffusion, upwinded transport, CLAMP outflow faces).
Short recurrences, fixed storage, no transpose, two operator applications
per iteration.

As in solvers/cg.py the operator is a `Stencil` applied by
`DistributedDomain.apply_stencil`, the halo exchange and the boundary fill
supply the neighbour values, and the solver never calls `dd.swap()`: `A q`
lives in the next buffer of `q`. Five quantities x, b, r, rhat, p are all
the storage of the plain solver.

    r = b (x0_zero) | b - A x;  rhat = r;  bb = dot(b);  rho = dot(rhat, r)
    repeat
      p = r                              first iteration, or after a restart
        | r + beta (p - omega v)         one axpbypcz, v = Next(p^)
      p^ = M p  (or p);  exchange;  v = A p^ -> Next(p^)
      alpha = rho / dot(rhat, v)
      ss = axpby_norm2(1, r, -alpha, v, out=r)        r now holds s
      if ss <= tol^2 bb:  x += alpha p^;  go to verify
      s^ = M r  (or r);  exchange;  t = A s^ -> Next(s^)
      (ts, tt) = dot_pair(t, r);  omega = ts / tt
      (rr, rho_new) = bicgstab_update(alpha, p^, omega, s^, x, r, t, rhat)
      if rr <= tol^2 bb:  go to verify
      beta = (rho_new / rho) (alpha / omega);  rho = rho_new
    verify: exchange(group_x); r = b - A x, freshly computed;
            converged if ||r|| <= tol ||b||, else restart with rhat = r

Composed from axpby, axpbypcz and dot an iteration makes about 22 vector
passes and eight reductions next to its two operator applications; with
the three fused kernels (csrc/src/vector_ops.hip) it makes 4 + 2 + 3 + 2 +
7 = 18 and four.

Right preconditioning. With M (any object with apply(f, e) leaving
e = M f, f read only; M need not be symmetric) and two more quantities y
and z for p^ and s^ the solver iterates on A M u = b, x = M u, so r is
always the residual of the ORIGINAL system and the stopping test is CG's:
||r|| <= tol ||b||.

Verify. The recursive residual of BiCGStab drifts further from b - A x
than CG's. So what is returned is checked: once the recursive residual has
converged, r = b - A x is computed; if it meets the tolerance too, the
solve is done and the last entry of `residuals` is this true residual.
Otherwise the iteration restarts from it (rhat = r, p = r). At most 10
restarts; a restart that does not reduce the true residual ends the solve
with reason="stagnated". The verify step applies A to x, so it needs
group_x; without group_x the recursive residual is what is returned.

Boundary conditions. A must be linear and homogeneous in the field, not
symmetric: PERIODIC, FIXED(0), MIRROR, ANTIMIRROR and CLAMP qualify. OPEN
and FIXED(c != 0) are refused; fold inhomogeneous data into b.

Breakdown. A zero or non-finite rho, rhat . v, t . t, alpha or omega ends
the solve with converged=False, reason="breakdown", on every rank and
without an exception: every scalar the loop branches on comes from the
global reductions of DistributedDomain, bitwise identical on every rank.

Not there: a DiffusionOperator as A, the null-space projection of
ConjugateGradient (this solver is for non-singular A), BiCGStab(l), GMRES.
"""
from __future__ import annotations

import math
import time
from typing import Optional

from ..boundary import Boundary
from ..core import DataHandle, DistributedDomain, Next
from ..stencil import Stencil
from ._common import (  # noqa: F401  (check_radius is re-exported)
    CGResult,
    check_faces,
    check_quantities,
    check_radius,
    operator_apply,
    overlapped_apply,
)

MAX_RESTARTS = 10


def check_homogeneous_boundary(who: str, dd: DistributedDomain, handles):
    """ValueError unless every non-periodic face of the given quantities is
    FIXED(0), MIRROR, ANTIMIRROR or CLAMP"""
    check_faces(f"{who}: ", dd, handles,
                (Boundary.FIXED, Boundary.MIRROR, Boundary.ANTIMIRROR, Boundary.CLAMP),
                ": the operator must be linear and homogeneous (PERIODIC, FIXED(0), MIRROR, "
                "ANTIMIRROR or CLAMP); fold inhomogeneous boundary data into b")


def _usable(v: float) -> bool:
    return math.isfinite(v) and v != 0.0


class BiCGStab:
    def __init__(self, dd: DistributedDomain, operator: Stencil, x: DataHandle, b: DataHandle,
                 r: DataHandle, rhat: DataHandle, p: DataHandle, group_p: int, group_r: int,
                 group_x: Optional[int] = None, preconditioner=None,
                 y: Optional[DataHandle] = None, z: Optional[DataHandle] = None):
        """dd is realized and holds x, b, r, rhat and p, five distinct
        quantities of one float type. operator is any Stencil the domain's
        radius covers. group_p is the exchange group of p^ (p, or y with a
        preconditioner), group_r that of s^ (r, or z with a
        preconditioner): both are exchanged every iteration. group_x is
        x's; the verify step and solve(x0_zero=False) need it.

        preconditioner: None, or any object with apply(f, e) that leaves
        e = M f in curr[e] and reads f only; it is called with (p, y) and
        (r, z), so it needs y and z, two more distinct quantities of the
        same type.

        Raises ValueError for an operator that is not a Stencil (a
        DiffusionOperator is out of scope), a domain radius that does not
        cover it, mixed dtypes, a boundary kind on x, p or an exchanged
        quantity other than PERIODIC, FIXED(0), MIRROR, ANTIMIRROR or
        CLAMP, a preconditioner without apply or without y and z, and y or
        z without a preconditioner."""
        who = "BiCGStab"
        if not isinstance(operator, Stencil):
            raise ValueError(f"{who}: the operator is a Stencil (a DiffusionOperator is not "
                             "supported)")
        if preconditioner is not None and not callable(getattr(preconditioner, "apply", None)):
            raise ValueError(f"{who}: the preconditioner has no apply(r, z)")
        phat, shat = (p, r) if preconditioner is None else (y, z)
        check_quantities(
            who, dd, (("x", x), ("b", b), ("r", r), ("rhat", rhat), ("p", p)),
            optional=((preconditioner is not None, (y, z),
                       "a preconditioner needs y and z, two more distinct quantities",
                       "y or z is given but no preconditioner"),),
            groups=[(h, g, f"{{name}} is not in exchange group {what}={g}")
                    for h, g, what in ((phat, group_p, "group_p"), (shat, group_r, "group_r"),
                                       (x, group_x, "group_x"))
                    if not (g is None and what == "group_x")])
        check_radius(who, dd, operator)
        checked = {h.index: h for h in (x, p, phat, shat)}
        check_homogeneous_boundary(who, dd, checked.values())
        self.dd, self.A = dd, operator
        self.x, self.b, self.r, self.rhat, self.p = x, b, r, rhat, p
        self.phat, self.shat = phat, shat
        self.group_p, self.group_r, self.group_x = group_p, group_r, group_x
        self.M = preconditioner
        self.restarts = 0  # of the last solve()
        # host wall time per phase of the last solve (each phase ends in a
        # host sync): operator = apply + exchange (both applications and the
        # verify step), reduction = rhat . v and (t . s, t . t), update =
        # the p update, axpby_norm2 and bicgstab_update
        self.phase_times = {"operator": 0.0, "reduction": 0.0, "update": 0.0}
        if preconditioner is not None:
            self.phase_times["precond"] = 0.0

    # ---- pieces ----
    def _apply(self, h: DataHandle, group: int, overlap: bool):
        """next[h] = A curr[h] on every local domain, halos refreshed"""
        dd = self.dd
        dd.backend.sync_compute()  # the exchange reads h on other streams
        overlapped_apply(dd, lambda where: operator_apply(dd, self.A, h, where), group, overlap)
        dd.backend.sync_compute()

    def _precondition(self, f: DataHandle, e: DataHandle):
        t0 = time.perf_counter()
        self.M.apply(f, e)
        self.dd.backend.sync_compute()
        self.phase_times["precond"] += time.perf_counter() - t0

    def _true_residual(self, overlap: bool) -> float:
        """r = b - A x; returns r . r"""
        t0 = time.perf_counter()
        self._apply(self.x, self.group_x, overlap)
        self.phase_times["operator"] += time.perf_counter() - t0
        return self.dd.axpby_norm2(1.0, self.b, -1.0, Next(self.x), out=self.r)

    # ---- the solve ----
    def solve(self, tol: float = 1e-6, max_iter: int = 1000, x0_zero: bool = True,
              overlap: bool = True) -> CGResult:
        """iterate until ||r|| <= tol * ||b|| or max_iter iterations (the
        iterations after a restart count too). x0_zero=True starts from
        x = 0 (x's content is overwritten); False starts from curr[x] and
        needs group_x. b = 0 gives x = 0 in 0 iterations, reason
        "zero_rhs". `residuals` holds the relative recursive residual after
        each iteration (the norm of s where the iteration ended on it) and
        entry 0; with group_x the last entry of a converged solve is the
        relative TRUE residual the verify step computed. `restarts` counts
        the restarts of the last solve."""
        dd, x, b, r = self.dd, self.x, self.b, self.r
        self.phase_times = {k: 0.0 for k in self.phase_times}
        self.restarts = 0
        if not x0_zero and self.group_x is None:
            raise ValueError("solve(x0_zero=False) needs group_x, the exchange group of x")
        bb = dd.dot(b)
        if not math.isfinite(bb):
            return CGResult(False, 0, [float("nan")], "breakdown")
        if bb == 0.0:
            dd.axpby(0.0, b, 0.0, b, out=x)  # the right-hand side is all zeros: so is x
            dd.backend.sync_compute()
            return CGResult(True, 0, [0.0], "zero_rhs")
        if x0_zero:
            dd.axpby(0.0, b, 0.0, b, out=x)
            dd.axpby(1.0, b, 0.0, b, out=r)
            rr = bb
        else:
            rr = self._true_residual(overlap)
        if not math.isfinite(rr):
            return CGResult(False, 0, [float("nan")], "breakdown")
        limit = tol * tol * bb
        residuals = [math.sqrt(rr / bb)]
        if rr <= limit:
            return CGResult(True, 0, residuals, "converged")
        its = 0
        while True:
            # one run from a freshly computed residual r with r . r = rr
            its, reason = self._run(rr, limit, bb, residuals, its, max_iter, overlap)
            if reason is not None:
                return CGResult(False, its, residuals, reason)
            if self.group_x is None:  # nothing to verify with
                return CGResult(True, its, residuals, "converged")
            start, rr = rr, self._true_residual(overlap)
            if not math.isfinite(rr):
                return CGResult(False, its, residuals[:-1] + [float("nan")], "breakdown")
            residuals[-1] = math.sqrt(rr / bb)
            if rr <= limit:
                return CGResult(True, its, residuals, "converged")
            if not rr < start or self.restarts >= MAX_RESTARTS:
                return CGResult(False, its, residuals, "stagnated")
            if its >= max_iter:
                return CGResult(False, its, residuals, "max_iter")
            self.restarts += 1

    def _run(self, rho, limit, bb, residuals, its, max_iter, overlap):
        """iterate from curr[r] (rho = r . r) with rhat = r and p = r until
        the recursive residual meets `limit`: returns (iterations so far,
        None), or (iterations, reason) where the solve ends unconverged.
        Appends to `residuals`."""
        dd, x, r, rhat, p = self.dd, self.x, self.r, self.rhat, self.p
        phat, shat, ph = self.phat, self.shat, self.phase_times
        dd.axpby(1.0, r, 0.0, r, out=rhat)
        alpha = omega = beta = 0.0
        first = True
        while its < max_iter:
            t0 = time.perf_counter()
            if first:  # beta = 0 must not read the old p, which may hold NaN
                dd.axpby(1.0, r, 0.0, r, out=p)
                first = False
            else:
                dd.axpbypcz(1.0, r, beta, p, -beta * omega, Next(phat), out=p)
            dd.backend.sync_compute()
            t1 = time.perf_counter()
            ph["update"] += t1 - t0
            if self.M is not None:
                self._precondition(p, phat)
            t1 = time.perf_counter()
            self._apply(phat, self.group_p, overlap)
            t2 = time.perf_counter()
            rv = dd.dot(rhat, Next(phat))
            t3 = time.perf_counter()
            ph["operator"] += t2 - t1
            ph["reduction"] += t3 - t2
            if not _usable(rv):
                return its, "breakdown"
            alpha = rho / rv
            if not _usable(alpha):
                return its, "breakdown"
            ss = dd.axpby_norm2(1.0, r, -alpha, Next(phat), out=r)  # r holds s
            ph["update"] += time.perf_counter() - t3
            if not math.isfinite(ss):
                residuals.append(float("nan"))
                return its + 1, "breakdown"
            if ss <= limit:
                dd.axpby(1.0, x, alpha, phat, out=x)
                dd.backend.sync_compute()
                residuals.append(math.sqrt(ss / bb))
                return its + 1, None
            if self.M is not None:
                self._precondition(r, shat)
            t4 = time.perf_counter()
            self._apply(shat, self.group_r, overlap)
            t5 = time.perf_counter()
            ts, tt = dd.dot_pair(Next(shat), r)
            t6 = time.perf_counter()
            ph["operator"] += t5 - t4
            ph["reduction"] += t6 - t5
            if not _usable(tt) or not math.isfinite(ts):
                return its, "breakdown"
            omega = ts / tt
            if not _usable(omega):
                return its, "breakdown"
            rr, rho_new = dd.bicgstab_update(alpha, phat, omega, shat, x, r, Next(shat), rhat)
            ph["update"] += time.perf_counter() - t6
            its += 1
            if not math.isfinite(rr):
                residuals.append(float("nan"))
                return its, "breakdown"
            residuals.append(math.sqrt(rr / bb))
            if rr <= limit:
                return its, None
            if not _usable(rho_new):
                return its, "breakdown"
            beta = (rho_new / rho) * (alpha / omega)
            if not math.isfinite(beta):
                return its, "breakdown"
            rho = rho_new
        return its, "max_iter"
