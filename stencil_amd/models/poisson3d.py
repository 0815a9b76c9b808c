"""Poisson-3D / Helmholtz-3D: solve (sigma I - laplacian) x = b with the
conjugate-gradient solver (stencil_amd/solvers/cg.py) on the generic
stencil operator. sigma > 0 is an implicit diffusion step or a screened
Poisson problem; sigma = 0 is the Poisson problem proper, which needs a
boundary that pins the constant (FIXED(0) or ANTIMIRROR on some axis) or,
for the singular problem of a periodic box or zero-flux (MIRROR) walls,
nullspace="constant": the solver then solves A x = b - mean(b) and returns
the solution with mean(x) = 0 (solvers/cg.py).

Four quantities x, b, r, p; only p (every iteration) and x (for a nonzero
initial guess) are ever exchanged, each in an exchange group of its own.
The radius is the operator's, so the exchange moves faces only.

preconditioner="multigrid" adds a fifth quantity z in a third exchange
group and a geometric multigrid V-cycle (solvers/multigrid.py) as the
preconditioner of CG: the iteration count then no longer grows with the
grid edge.
"""
from __future__ import annotations

from typing import List, Optional

import numpy as np

from ..boundary import FACES, Boundary, parse_face
from ..core import DistributedDomain
from ..parallel.placement import PlacementStrategy
from ..solvers.cg import CGResult, ConjugateGradient
from ..solvers.diffusion import DiffusionOperator, JacobiPreconditioner
from ..solvers.multigrid import GeometricMultigrid
from ..stencil import Stencil


class Poisson3D:
    def __init__(
        self,
        size,
        order: int = 2,
        dtype=np.float32,
        sigma: float = 0.0,
        spacing=(1.0, 1.0, 1.0),
        backend: str = "native",
        gpus: Optional[List[int]] = None,
        boundary=None,
        placement: PlacementStrategy = PlacementStrategy.NodeAware,
        device: str = "cpu",
        preconditioner: Optional[str] = None,
        mg: Optional[dict] = None,
        coarse_order: int = 2,
        coefficient: bool = False,
        nullspace: Optional[str] = None,
    ):
        """A = sigma I - laplacian(order, spacing); sigma >= 0.

        preconditioner: None (plain CG) or "multigrid": a V-cycle whose
        level l >= 1 uses sigma I - laplacian(coarse_order, spacing * 2^l).
        mg: keyword arguments of GeometricMultigrid (nu, omega,
        coarse_sweeps, max_levels).

        coefficient=True: A = sigma I - div(k grad) with a cell-centred
        coefficient field k (solvers/diffusion.py), initially 1; give it
        with set_coefficient(). Needs order == 2 (ValueError otherwise).
        Three more quantities: k in an exchange group of its own (CLAMP on
        non-periodic faces), dinv, and xc, with which the solver verifies
        the true residual b - A x at convergence and refines x until it
        meets the tolerance (ConjugateGradient.solve; a variable k makes
        nearly singular operators common, where the recursive residual of
        a float32 solve drifts). The multigrid hierarchy is then built
        from k, and preconditioner may also be "jacobi" (diagonal scaling;
        ValueError without a coefficient).

        boundary: {face: kind | (kind, value)} as in Diffusion3D, applied
        to all four quantities; None = fully periodic. The kinds the
        solver accepts are PERIODIC, FIXED(0), MIRROR and ANTIMIRROR; fold
        inhomogeneous Dirichlet data into the right-hand side. Raises
        ValueError when the problem is singular: sigma == 0 with every axis
        periodic or MIRROR (the constant is then in A's null space), unless
        nullspace="constant".

        nullspace: None, or "constant" for exactly that singular problem
        (ValueError for every other configuration: projecting a
        non-singular problem would be wrong), with or without a
        coefficient and with any preconditioner. ConjugateGradient then
        projects off the constants: b may have any mean, the solution
        comes back with mean 0. Always adds the correction quantity xc (a
        singular A is the extreme of the nearly singular case the
        refinement exists for)."""
        sigma = float(sigma)
        if not sigma >= 0.0:
            raise ValueError(f"Poisson3D: sigma must be >= 0, got {sigma}")
        if preconditioner not in (None, "multigrid", "jacobi"):
            raise ValueError(
                "Poisson3D: preconditioner is None, 'multigrid' or 'jacobi', "
                f"got {preconditioner!r}")
        if preconditioner == "jacobi" and not coefficient:
            raise ValueError("Poisson3D: the 'jacobi' preconditioner needs coefficient=True "
                             "(the constant-coefficient diagonal is a multiple of I)")
        if coefficient and order != 2:
            raise ValueError(f"Poisson3D: coefficient=True needs order == 2, got {order}")
        if mg is not None and preconditioner != "multigrid":
            raise ValueError("Poisson3D: mg is given but no multigrid preconditioner")
        self.coefficient = bool(coefficient)
        self.sigma = sigma
        self.order, self.coarse_order = order, coarse_order
        self.spacing = tuple(float(h) for h in spacing)
        self.preconditioner = preconditioner
        self._mg_args = dict(mg or {})
        self.mg: Optional[GeometricMultigrid] = None
        self.stencil = -Stencil.laplacian(order, spacing)
        if sigma != 0.0:
            self.stencil = self.stencil + sigma * Stencil.identity()
        kinds = {}
        if boundary:
            for face, spec in boundary.items():
                kind = spec[0] if isinstance(spec, (tuple, list)) else spec
                for f in parse_face(face):
                    kinds[FACES[f]] = Boundary(kind)
        if nullspace not in (None, "constant"):
            raise ValueError(f"Poisson3D: nullspace is None or 'constant', got {nullspace!r}")
        self.nullspace = nullspace
        singular = sigma == 0.0 and all(
            kinds.get(f, Boundary.PERIODIC) in (Boundary.PERIODIC, Boundary.MIRROR)
            for f in FACES
        )
        if nullspace is not None and not singular:
            raise ValueError(
                "Poisson3D: nullspace='constant' is for the singular problem only: sigma == 0 "
                "with every axis periodic or MIRROR; this one has "
                + (f"sigma = {sigma}" if sigma != 0.0 else "a face that pins the constant"))
        if singular and nullspace is None:
            raise ValueError(
                "Poisson3D: sigma == 0 with every axis periodic or MIRROR is singular "
                "(constants are in the null space); use sigma > 0 or a FIXED(0)/ANTIMIRROR face"
            )
        self.dd = DistributedDomain(*size, backend=backend, device=device)
        self.dd.set_radius(self.stencil.radius())
        self.dd.set_placement(placement)
        if gpus is not None:
            self.dd.set_gpus(gpus)
        dt = np.dtype(dtype)
        if dt not in (np.dtype(np.float32), np.dtype(np.float64)):
            raise ValueError(f"Poisson3D supports float32/float64, got {dt}")
        self.x = self.dd.add_data(dt, "x")
        self.b = self.dd.add_data(dt, "b")
        self.r = self.dd.add_data(dt, "r")
        self.p = self.dd.add_data(dt, "p")
        # quantities in no group are never exchanged: b and r need no halos
        groups = [[self.p.index], [self.x.index]]
        self.z = None
        if preconditioner is not None:
            self.z = self.dd.add_data(dt, "z")
            groups.append([self.z.index])
        self.k = self.dinv = self.xc = None
        self.op: Optional[DiffusionOperator] = None
        self.jacobi: Optional[JacobiPreconditioner] = None
        if self.coefficient:
            self.k = self.dd.add_data(dt, "k")
            self.dinv = self.dd.add_data(dt, "dinv")
            self.xc = self.dd.add_data(dt, "xc")  # CG's correction: true-residual check
            self._group_k = len(groups)
            groups.append([self.k.index])
        elif nullspace is not None:
            self.xc = self.dd.add_data(dt, "xc")
        self.dd.set_exchange_groups(groups)
        if boundary:
            for face, spec in boundary.items():
                kind, value = spec if isinstance(spec, (tuple, list)) else (spec, 0)
                self.dd.set_boundary(face, kind, value)
                if self.coefficient and Boundary(kind) != Boundary.PERIODIC:
                    self.dd.set_boundary(face, Boundary.CLAMP, quantities=[self.k])
        self.cg: Optional[ConjugateGradient] = None

    def operator_at(self, level: int) -> Stencil:
        """the operator at spacing * 2^level: self.stencil on level 0,
        coarse_order below"""
        if level == 0:
            return self.stencil
        st = -Stencil.laplacian(self.coarse_order, [h * 2.0 ** level for h in self.spacing])
        if self.sigma != 0.0:
            st = st + self.sigma * Stencil.identity()
        return st

    def realize(self):
        self.dd.realize()
        operator, operator_at = self.stencil, self.operator_at
        if self.coefficient:
            ones = np.ones((self.dd.size[2], self.dd.size[1], self.dd.size[0]), dtype=self.k.dtype)
            self._scatter(self.k, ones)
            self.op = DiffusionOperator(self.dd, self.k, self._group_k, spacing=self.spacing,
                                        sigma=self.sigma, dinv=self.dinv)
            self.op.refresh()
            operator, operator_at = self.op, (lambda level: self.op)
        M = None
        if self.preconditioner == "multigrid":
            M = self.mg = GeometricMultigrid(self.dd, operator_at, self.z, 2, **self._mg_args)
        elif self.preconditioner == "jacobi":
            M = self.jacobi = JacobiPreconditioner(self.op)
        self.cg = ConjugateGradient(self.dd, operator, self.x, self.b, self.r, self.p,
                                    group_p=0, group_x=1, preconditioner=M, z=self.z,
                                    correction=self.xc, nullspace=self.nullspace)

    def set_coefficient(self, global_array):
        """k = the (z, y, x) global array, every value finite and > 0
        (ValueError otherwise; nothing is written then); refreshes the
        operator's halos, the preconditioner's diagonal and the multigrid
        hierarchy. Realizes the domain first if need be."""
        if not self.coefficient:
            raise ValueError("Poisson3D.set_coefficient: built with coefficient=False")
        g = np.asarray(global_array)
        if not (np.isfinite(g).all() and (g > 0).all()):
            raise ValueError("Poisson3D.set_coefficient: every value must be finite and > 0")
        if self.cg is None:
            self.realize()
        self._scatter(self.k, g)
        if self.mg is not None:
            self.mg.refresh_coefficients()
        else:
            self.op.refresh()
        if self.jacobi is not None:
            self.jacobi.refresh()

    def _scatter(self, handle, g):
        g = np.asarray(g)
        want = (self.dd.size[2], self.dd.size[1], self.dd.size[0])
        if g.shape != want:
            raise ValueError(f"Poisson3D: want a (z, y, x) array of shape {want}, got {g.shape}")
        for li in range(self.dd.num_local()):
            lo, hi = self.dd.local_rect(li)
            block = np.ascontiguousarray(g[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]])
            self.dd.write_global(li, lo, block.astype(handle.dtype), handle)

    def set_rhs(self, global_array):
        """b = the (z, y, x) global array; each rank writes its own cells"""
        self._scatter(self.b, global_array)

    def set_guess(self, global_array):
        """x = the global array, for solve(x0_zero=False)"""
        self._scatter(self.x, global_array)

    def solve(self, tol: float = 1e-6, max_iter: int = 1000, x0_zero: bool = True,
              overlap: bool = True) -> CGResult:
        if self.cg is None:
            self.realize()
        if self.mg is not None:
            self.mg.overlap = overlap
        return self.cg.solve(tol=tol, max_iter=max_iter, x0_zero=x0_zero, overlap=overlap)

    def solution(self) -> np.ndarray:
        """x as a (z, y, x) global array; cells of other ranks' domains are 0"""
        out = np.zeros((self.dd.size[2], self.dd.size[1], self.dd.size[0]), dtype=self.x.dtype)
        for li in range(self.dd.num_local()):
            lo, hi = self.dd.local_rect(li)
            out[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]] = self.dd.read_global(li, lo, hi, self.x)
        return out
