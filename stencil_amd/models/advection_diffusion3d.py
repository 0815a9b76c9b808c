"""Advection-diffusion-3D: solve (sigma I + v . grad - nu laplacian) x = b
with BiCGStab (stencil_amd/solvers/bicgstab.py) on the generic stencil
operator. The velocity makes A non-symmetric, which is what conjugate
gradients (models/poisson3d.py) refuses. One solve with sigma = 1 / dt is a
backward-Euler step of u_t + v . grad u = nu laplacian u; sigma = 0 is the
steady problem, which needs a face that pins the constant.

Five quantities x, b, r, rhat, p; p and r are exchanged every iteration,
x by the solver's verify step, each in an exchange group of its own. The
radius is the operator's: a pure upwind operator (nu = 0) allocates and
exchanges no downwind halo.

preconditioner="multigrid" adds y and z and right-preconditions with the
geometric multigrid V-cycle of the SYMMETRIC PART of A, rediscretised at
every level's spacing (solvers/multigrid.py, unchanged: it wants a
symmetric operator with a positive centre, and (A + A^T) / 2 = sigma I -
nu laplacian - the upwind scheme's numerical diffusion is one). The
exchange groups are then those of y, z and x, and the radius is the
symmetric part's, which covers A.
"""
from __future__ import annotations

import math
from typing import List, Optional

import numpy as np

from ..boundary import FACES, Boundary, parse_face
from ..core import DistributedDomain
from ..parallel.placement import PlacementStrategy
from ..solvers.bicgstab import BiCGStab
from ..solvers.cg import CGResult
from ..solvers.multigrid import GeometricMultigrid
from ..stencil import Stencil


class _CycleInto:
    """M.apply(f, e) for any e: the cycle writes the one quantity it was
    built for, a copy carries the result where BiCGStab wants it"""

    def __init__(self, dd, mg, z):
        self.dd, self.mg, self.z = dd, mg, z

    def apply(self, f, e):
        self.mg.apply(f, self.z)
        if e.index != self.z.index:
            self.dd.axpby(1.0, self.z, 0.0, self.z, out=e)


class AdvectionDiffusion3D:
    def __init__(
        self,
        size,
        velocity=(1.0, 0.0, 0.0),
        nu: float = 0.0,
        sigma: float = 1.0,
        scheme: str = "upwind",
        dtype=np.float32,
        spacing=(1.0, 1.0, 1.0),
        backend: str = "native",
        gpus: Optional[List[int]] = None,
        boundary=None,
        preconditioner: Optional[str] = None,
        mg: Optional[dict] = None,
        placement: PlacementStrategy = PlacementStrategy.NodeAware,
        device: str = "cpu",
    ):
        """A = sigma I + advection(velocity, spacing, scheme) - nu
        laplacian(2, spacing); sigma >= 0, nu >= 0.

        boundary: {face: kind | (kind, value)} as in Poisson3D, applied to
        every quantity; None = fully periodic. The kinds the solver accepts
        are PERIODIC, FIXED(0), MIRROR, ANTIMIRROR and CLAMP (an outflow
        face).

        preconditioner: None or "multigrid" (module docstring); mg: keyword
        arguments of GeometricMultigrid.

        Raises ValueError for sigma < 0, nu < 0, sigma == 0 with no face
        that pins the constant (every face periodic, MIRROR or CLAMP: A is
        then singular), scheme "central" with nu == 0 (the central
        difference alone decouples odd and even cells), and CLAMP faces
        with the multigrid preconditioner (the cycle refuses them)."""
        who = "AdvectionDiffusion3D"
        sigma, nu = float(sigma), float(nu)
        if not (sigma >= 0.0 and math.isfinite(sigma)):
            raise ValueError(f"{who}: sigma must be >= 0, got {sigma}")
        if not (nu >= 0.0 and math.isfinite(nu)):
            raise ValueError(f"{who}: nu must be >= 0, got {nu}")
        if preconditioner not in (None, "multigrid"):
            raise ValueError(f"{who}: preconditioner is None or 'multigrid', "
                             f"got {preconditioner!r}")
        if mg is not None and preconditioner != "multigrid":
            raise ValueError(f"{who}: mg is given but no multigrid preconditioner")
        self.velocity = tuple(float(v) for v in velocity)
        self.spacing = tuple(float(h) for h in spacing)
        self.sigma, self.nu, self.scheme = sigma, nu, scheme
        self.stencil = self.operator(0)  # validates velocity, spacing and scheme
        if scheme == "central" and nu == 0.0:
            raise ValueError(f"{who}: scheme 'central' needs nu > 0")
        kinds = {}
        if boundary:
            for face, spec in boundary.items():
                kind = spec[0] if isinstance(spec, (tuple, list)) else spec
                for f in parse_face(face):
                    kinds[FACES[f]] = Boundary(kind)
        free = (Boundary.PERIODIC, Boundary.MIRROR, Boundary.CLAMP)
        if sigma == 0.0 and all(kinds.get(f, Boundary.PERIODIC) in free for f in FACES):
            raise ValueError(
                f"{who}: sigma == 0 with every face periodic, MIRROR or CLAMP is singular "
                "(constants are in the null space); use sigma > 0 or a FIXED(0)/ANTIMIRROR face")
        if preconditioner is not None and Boundary.CLAMP in kinds.values():
            raise ValueError(f"{who}: the multigrid preconditioner does not take CLAMP faces")
        self.preconditioner = preconditioner
        self._mg_args = dict(mg or {})
        self.mg: Optional[GeometricMultigrid] = None
        self.dd = DistributedDomain(*size, backend=backend, device=device)
        radius = self.stencil.radius() if preconditioner is None else self.operator_at(0).radius()
        self.dd.set_radius(radius)
        self.dd.set_placement(placement)
        if gpus is not None:
            self.dd.set_gpus(gpus)
        dt = np.dtype(dtype)
        if dt not in (np.dtype(np.float32), np.dtype(np.float64)):
            raise ValueError(f"{who} supports float32/float64, got {dt}")
        self.x = self.dd.add_data(dt, "x")
        self.b = self.dd.add_data(dt, "b")
        self.r = self.dd.add_data(dt, "r")
        self.rhat = self.dd.add_data(dt, "rhat")
        self.p = self.dd.add_data(dt, "p")
        self.y = self.z = None
        if preconditioner is None:
            # quantities in no group are never exchanged: b and rhat need no halos
            groups = [[self.p.index], [self.r.index], [self.x.index]]
        else:
            self.y = self.dd.add_data(dt, "y")
            self.z = self.dd.add_data(dt, "z")
            groups = [[self.y.index], [self.z.index], [self.x.index]]
        self.dd.set_exchange_groups(groups)
        if boundary:
            for face, spec in boundary.items():
                kind, value = spec if isinstance(spec, (tuple, list)) else (spec, 0)
                self.dd.set_boundary(face, kind, value)
        self.solver: Optional[BiCGStab] = None

    def operator(self, level: int) -> Stencil:
        """A discretised at spacing * 2^level"""
        h = [s * 2.0 ** level for s in self.spacing]
        st = Stencil.advection(self.velocity, h, self.scheme)
        if self.nu != 0.0:
            st = st - self.nu * Stencil.laplacian(2, h)
        if self.sigma != 0.0:
            st = st + self.sigma * Stencil.identity()
        return st

    def operator_at(self, level: int) -> Stencil:
        """what the multigrid cycle smooths with at spacing * 2^level: the
        symmetric part of operator(level)"""
        return self.operator(level).symmetric_part()

    def realize(self):
        self.dd.realize()
        M = None
        if self.preconditioner == "multigrid":
            self.mg = GeometricMultigrid(self.dd, self.operator_at, self.z, 1, **self._mg_args)
            M = _CycleInto(self.dd, self.mg, self.z)
        self.solver = BiCGStab(self.dd, self.stencil, self.x, self.b, self.r, self.rhat, self.p,
                               group_p=0, group_r=1, group_x=2, preconditioner=M, y=self.y,
                               z=self.z)

    def _scatter(self, handle, g):
        g = np.asarray(g)
        want = (self.dd.size[2], self.dd.size[1], self.dd.size[0])
        if g.shape != want:
            raise ValueError(
                f"AdvectionDiffusion3D: want a (z, y, x) array of shape {want}, got {g.shape}")
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
        if self.solver is None:
            self.realize()
        if self.mg is not None:
            self.mg.overlap = overlap
        return self.solver.solve(tol=tol, max_iter=max_iter, x0_zero=x0_zero, overlap=overlap)

    def solution(self) -> np.ndarray:
        """x as a (z, y, x) global array; cells of other ranks' domains are 0"""
        out = np.zeros((self.dd.size[2], self.dd.size[1], self.dd.size[0]), dtype=self.x.dtype)
        for li in range(self.dd.num_local()):
            lo, hi = self.dd.local_rect(li)
            out[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]] = self.dd.read_global(li, lo, hi, self.x)
        return out
