"""DiffusionOperator: A = sigma I - div(k grad) with a cell-centred
coefficient field k > 0, the variable-coefficient counterpart of the
`Stencil` operator of ConjugateGradient and GeometricMultigrid, and
JacobiPreconditioner, the diagonal preconditioner it makes possible.

With h_a = 1 / spacing_a^2 and e_a the unit vector of axis a:

    (A u)(p) = sigma u(p) + sum over a in {x,y,z}, s in {-1,+1} of
               h_a * 0.5 (k(p) + k(p + s e_a)) * (u(p) - u(p + s e_a))

    diag(p)  = sigma + sum over a, s of  h_a * 0.5 (k(p) + k(p + s e_a))

The face coefficient is the arithmetic mean of the two cells: symmetric in
the pair, so A is symmetric, and positive semi-definite for k > 0 and
sigma >= 0 (positivity of k is the caller's contract; a non-positive
p . A p ends a CG solve as "breakdown"). The halos of u come from the
exchange and the boundary fill as everywhere: u's boundary kinds ARE the
boundary conditions (PERIODIC, FIXED(0), MIRROR, ANTIMIRROR). The halos of
k are read one cell deep on faces only; on non-periodic faces k must be
CLAMP or MIRROR (identical in the first layer). diag is the stencil
diagonal without boundary correction, the convention of the centre weight
the constant-coefficient smoother uses; Gershgorin still gives
rho(D^-1 A) <= 2, so omega in (0, 1) keeps a damped-Jacobi cycle positive
definite. With k = 1 the operator is sigma I - laplacian(2, spacing).

The kernels are csrc/src/diffusion_op.hip on the native backend and tensor
slicing on the torch backend.
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from .. import _C
from ..boundary import FACES, Boundary
from ..core import DataHandle, DistributedDomain


class DiffusionOperator:
    def __init__(self, dd: DistributedDomain, k: DataHandle, group_k: int,
                 spacing=(1.0, 1.0, 1.0), sigma: float = 0.0,
                 dinv: Optional[DataHandle] = None):
        """dd is realized and holds k and, optionally, dinv (the quantity
        inv_diagonal and the preconditioners write omega / diag to), both
        added before realize(). group_k is the exchange group that holds k.
        Raises ValueError for a domain that is not realized or whose face
        radius is below 1, a k that is not float32/float64 or of another
        type than dinv, k not in group_k, sigma < 0 and a boundary kind of k
        other than PERIODIC, CLAMP or MIRROR."""
        who = "DiffusionOperator"
        if not dd._realized:
            raise ValueError(f"{who}: construct after dd.realize()")
        if not isinstance(k, DataHandle):
            raise TypeError(f"{who}: k is a DataHandle")
        if k.dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
            raise ValueError(f"{who} supports float32/float64 quantities, got {k.dtype}")
        if dinv is not None:
            if not isinstance(dinv, DataHandle):
                raise TypeError(f"{who}: dinv is a DataHandle")
            if dinv.dtype != k.dtype or dinv.index == k.index:
                raise ValueError(f"{who}: dinv must be another quantity of k's type {k.dtype}, "
                                 f"got {dinv.dtype}")
        r = dd.radius
        if min(r.x(-1), r.x(1), r.y(-1), r.y(1), r.z(-1), r.z(1)) < 1:
            raise ValueError(f"{who}: the domain's face radius must be at least 1")
        groups = dd.exchange_groups or [list(range(len(dd._data)))]
        if not (0 <= group_k < len(groups) and k.index in groups[group_k]):
            raise ValueError(f"{who}: k is not in exchange group {group_k}")
        sigma = float(sigma)
        if not sigma >= 0.0:
            raise ValueError(f"{who}: sigma must be >= 0, got {sigma}")
        spacing = tuple(float(s) for s in spacing)
        if len(spacing) != 3 or not all(s > 0.0 for s in spacing):
            raise ValueError(f"{who}: spacing is three positive numbers, got {spacing}")
        spec = dd.boundary
        if spec is not None:
            for a in range(3):
                if spec.periodic[a]:
                    continue
                for s in (0, 1):
                    kind = spec.kind(k.index, a, s)
                    if kind not in (Boundary.CLAMP, Boundary.MIRROR):
                        raise ValueError(
                            f"{who}: boundary {kind.name} on face {FACES[2 * a + s]} of the "
                            "coefficient: its non-periodic faces must be CLAMP or MIRROR")
        self.dd, self.k, self.group_k, self.dinv = dd, k, group_k, dinv
        self.spacing, self.sigma = spacing, sigma
        self.h = tuple(1.0 / (s * s) for s in spacing)

    def radius(self) -> "_C.Radius":
        """faces 1, edges and corners 0"""
        r = _C.Radius.constant(0)
        for a in range(3):
            for s in (-1, 1):
                e = [0, 0, 0]
                e[a] = s
                r.set_dir(e[0], e[1], e[2], 1)
        return r

    def is_symmetric(self) -> bool:
        return True

    def refresh(self):
        """exchange k once: its face halos are what apply() and
        inv_diagonal() read. Call after k changed."""
        self.dd.backend.sync_compute()
        self.dd.exchange(self.group_k)

    def apply(self, src: DataHandle, dst: Optional[DataHandle] = None, where="all",
              stream_id: Optional[int] = None):
        """next[dst] = A curr[src]; `where` and `stream_id` as in
        DistributedDomain.apply_stencil"""
        self.dd.apply_diffusion(self.k, src, dst, spacing=self.spacing, sigma=self.sigma,
                                where=where, stream_id=stream_id)

    def inv_diagonal(self, omega: float, out: DataHandle):
        """curr[out] = omega / diag over every local_rect, in the quantity's
        type; k's halos must be current (refresh()). Enqueued on compute
        stream 0."""
        if not isinstance(out, DataHandle) or out.dtype != self.k.dtype:
            raise ValueError("DiffusionOperator.inv_diagonal: out must be a quantity of k's type")
        dd = self.dd
        for li in range(dd.num_local()):
            lo, hi = dd.local_rect(li)
            dd.backend.diffusion_inv_diagonal(li, self.k.index, out.index, False, lo, hi, self.h,
                                              self.sigma, float(omega))


class JacobiPreconditioner:
    def __init__(self, op: DiffusionOperator, omega: float = 1.0):
        """M = omega D^-1 of a DiffusionOperator with a dinv quantity, the
        preconditioner argument of ConjugateGradient. k's halos must be
        current (op.refresh()); call refresh() here after k changed."""
        if not isinstance(op, DiffusionOperator):
            raise TypeError("JacobiPreconditioner: op is a DiffusionOperator")
        if op.dinv is None:
            raise ValueError("JacobiPreconditioner: the operator has no dinv quantity")
        if not float(omega) > 0.0:
            raise ValueError(f"JacobiPreconditioner: omega must be positive, got {omega}")
        self.op, self.omega = op, float(omega)
        self.refresh()

    def refresh(self):
        """recompute dinv = omega / diag from the current k"""
        self.op.inv_diagonal(self.omega, self.op.dinv)
        self.op.dd.backend.sync_compute()

    def apply(self, r: DataHandle, z: DataHandle):
        """curr[z] = omega * curr[r] / diag; r is read only"""
        dd = self.op.dd
        dd.scaled_update(0.0, r, self.op.dinv, 1.0, r, 0.0, r, out=z)
        dd.backend.sync_compute()
