"""GeometricMultigrid: a symmetric V-cycle on cell-centred 2:1 coarsening,
the preconditioner M of ConjugateGradient (solvers/cg.py).

Level 0 is the caller's DistributedDomain; level l >= 1 is a new one of half
the size of level l - 1, partitioned alike (GridTransfer checks that), with
two quantities e (the correction) and f (the restricted residual). At level
l, with A = operator_at(l), w = omega / (centre weight of A) and n =
coarse_sweeps on the last level, nu otherwise:

    e = w f                                           (the first sweep from e = 0)
    n-1 times:  exchange(e); next[e] = A e; e = e + w f - w next[e]
    not last:   exchange(e); next[e] = A e; f_{l+1} = restrict(f - next[e])
                recurse;  e += prolong(e_{l+1})
                n times:  exchange(e); next[e] = A e; e = e + w f - w next[e]

Damped Jacobi before and after, full-weighting-by-mean down and its
transpose (times 8) up: M is symmetric. With omega = 2/3 the damped
iteration matrix of the Laplacians of order 2 to 8 stays below 2 in spectral
radius (rho(D^-1 A) is 2, 2.13 and 2.28 for orders 2, 4 and 8), so M is
positive definite as well.

The cycle never calls swap(): A e lives in the next buffer of e. There are
no reductions, so every rank takes identical branches. Levels >= 1 run
non-overlapped; level 0 honours `overlap`.

Variable coefficients. When operator_at(0) is a DiffusionOperator
(solvers/diffusion.py: sigma I - div(k grad), k a quantity), the hierarchy
is built from it and operator_at is not asked for the levels below. A coarse
level then has four quantities e, f, k, d in the exchange groups [[e], [k]]:
k is the mean of its 8 children (grid_restrict, no new transfer operator;
CLAMP on non-periodic faces, exchanged once), the spacing is doubled, sigma
unchanged, and d = omega / diag per cell (diffusion_inv_diagonal) takes the
place of w: the sweep is e = e + d (f - next[e]), one scaled_update, the
first sweep e = d f. Level 0 uses the operator's dinv quantity for d.
refresh_coefficients() redoes restriction, exchanges and diagonals after k
changed. The constant-coefficient path is the one above, unchanged.

Singular operators. With every face PERIODIC or MIRROR and sigma = 0 every
level's A has the constants in its null space, and the cycle runs on it as
it is: it is a fixed number of damped Jacobi sweeps, nothing is inverted,
and the coarsest level is swept like the others. Restriction by the mean
of 8 keeps a mean-free residual mean-free on every level. What the cycle
does not keep is the mean of its output: z = M r has a constant component
that the operator cannot see, small for a constant coefficient, of the
order of z itself when d = omega / diag varies per cell. Removing it is the
caller's job; ConjugateGradient(nullspace="constant") does it inside the
r . z pass (solvers/cg.py) and needs nothing from this class.

Not there: a whole-cycle hipGraph (each level costs host launches and
syncs, see phase_times), agglomeration of coarse levels onto fewer GPUs,
trilinear transfer, Galerkin coarse operators, harmonic-mean or
user-supplied face coefficients.
"""
from __future__ import annotations

import itertools
import time
from typing import Callable, List, Optional

import numpy as np

from ..boundary import FACES, Boundary
from ..core import DataHandle, DistributedDomain, Next
from ..stencil import Stencil
from ._common import operator_apply, overlapped_apply
from .cg import check_boundary, check_operator
from .diffusion import DiffusionOperator
from .transfer import GridTransfer


class _Level:
    __slots__ = ("dd", "A", "w", "e", "f", "group", "transfer")

    def __init__(self, dd, A, w, e, f, group):
        # A: a Stencil (w = omega / its centre weight) or a DiffusionOperator
        # (w is None: the per-cell omega / diag lives in the quantity A.dinv)
        self.dd, self.A, self.w, self.e, self.f, self.group = dd, A, w, e, f, group
        self.transfer: Optional[GridTransfer] = None  # to the next coarser level

    def apply(self, where):
        operator_apply(self.dd, self.A, self.e, where)


def _centre(who: str, A: Stencil) -> float:
    c = dict(zip(A.offsets, A.weights)).get((0, 0, 0), 0.0)
    if not c > 0.0:
        raise ValueError(f"{who}: the stencil's centre weight {c} is not positive")
    return c


def _face_radius(A: Stencil):
    r = A.radius()
    return (max(r.x(-1), r.x(1)), max(r.y(-1), r.y(1)), max(r.z(-1), r.z(1)))


def _subdomains(dd: DistributedDomain):
    pl = dd.placement
    dim = pl.dim()
    for idx in itertools.product(range(dim[0]), range(dim[1]), range(dim[2])):
        yield idx, tuple(pl.subdomain_origin(idx)), tuple(pl.subdomain_size(idx))


class GeometricMultigrid:
    def __init__(self, dd: DistributedDomain, operator_at: Callable[[int], Stencil],
                 e: DataHandle, group_e: int, nu: int = 2, omega: float = 2.0 / 3.0,
                 coarse_sweeps: int = 8, max_levels: Optional[int] = None):
        """dd is realized. operator_at(level) is the operator at spacing x
        2^level; level 0 must be the operator CG solves with. When
        operator_at(0) is a DiffusionOperator (it needs a dinv quantity:
        ValueError without), the levels below are built from its
        coefficient and operator_at is not called again. e is the
        quantity of dd the cycle writes (CG's z), group_e its exchange
        group. nu sweeps before and after each coarse-grid correction,
        coarse_sweeps on the last level, damping omega.

        Coarsening goes on while every global extent and every subdomain's
        origin and extents are even, every coarse subdomain extent is at
        least max(2, the coarse operator's face radius), the coarse
        domain's placement is the halved fine one and max_levels is not
        reached. Raises ValueError for fewer than 2 levels, a non-symmetric
        stencil, a centre weight that is not positive, a radius of dd that
        does not cover operator_at(0), a boundary kind on e other than
        PERIODIC, FIXED(0), MIRROR or ANTIMIRROR, omega outside (0, 1),
        nu < 1 and coarse_sweeps < 1."""
        who = "GeometricMultigrid"
        if not dd._realized:
            raise ValueError(f"{who}: construct after dd.realize()")
        if not isinstance(e, DataHandle):
            raise TypeError(f"{who}: e is a DataHandle")
        dt = e.dtype
        if dt not in (np.dtype(np.float32), np.dtype(np.float64)):
            raise ValueError(f"{who} supports float32/float64 quantities, got {dt}")
        if not 0.0 < float(omega) < 1.0:
            raise ValueError(f"{who}: omega must lie in (0, 1), got {omega}")
        if int(nu) != nu or nu < 1:
            raise ValueError(f"{who}: nu must be an integer >= 1, got {nu}")
        if int(coarse_sweeps) != coarse_sweeps or coarse_sweeps < 1:
            raise ValueError(f"{who}: coarse_sweeps must be an integer >= 1, got {coarse_sweeps}")
        if max_levels is not None and (int(max_levels) != max_levels or max_levels < 2):
            raise ValueError(f"{who}: fewer than 2 levels (max_levels={max_levels})")
        groups = dd.exchange_groups or [list(range(len(dd._data)))]
        if not (0 <= group_e < len(groups) and e.index in groups[group_e]):
            raise ValueError(f"{who}: e is not in exchange group {group_e}")
        A0 = operator_at(0)
        check_operator(who, dd, A0)
        check_boundary(who, dd, (e,))
        self.omega, self.nu, self.coarse_sweeps = float(omega), int(nu), int(coarse_sweeps)
        self.overlap = True  # of level 0; Poisson3D.solve sets it
        self._variable = isinstance(A0, DiffusionOperator)
        if self._variable:
            if A0.dinv is None:
                raise ValueError(f"{who}: the DiffusionOperator of level 0 has no dinv quantity")
            if A0.k.dtype != dt:
                raise ValueError(f"{who}: the coefficient is {A0.k.dtype}, e is {dt}")
            self._levels: List[_Level] = [_Level(dd, A0, None, e, None, group_e)]
        else:
            self._levels = [_Level(dd, A0, self.omega / _centre(who, A0), e, None, group_e)]
        while max_levels is None or len(self._levels) < max_levels:
            nxt = self._coarsen(who, self._levels[-1], operator_at, len(self._levels), dt)
            if nxt is None:
                break
            self._levels.append(nxt)
        if len(self._levels) < 2:
            raise ValueError(
                f"{who}: a {dd.size} grid in {dd.placement.dim()} subdomains cannot be coarsened "
                "(every extent, origin and subdomain extent must be even, and the halved "
                "subdomains at least max(2, radius) wide)"
            )
        self.levels = [tuple(lv.dd.size) for lv in self._levels]
        if self._variable:
            self.refresh_coefficients()
        # host wall time per level of all cycles since reset_times(): each
        # level's share ends in a host sync
        self.phase_times = {}
        self.reset_times()

    def reset_times(self):
        self.phase_times = {f"level{l}": 0.0 for l in range(len(self._levels))}

    # ---- the hierarchy ----
    def _coarsen(self, who, fine: _Level, operator_at, level: int, dt) -> Optional[_Level]:
        """the level below `fine`, or None where coarsening stops. Decided
        from the global partition only, so every rank decides alike."""
        fdd = fine.dd
        if any(n % 2 for n in fdd.size):
            return None
        subs = list(_subdomains(fdd))
        if any(c % 2 for _, o, s in subs for c in o + s):
            return None
        if self._variable:
            # built from the fine level's operator: operator_at is not asked
            A, w, need, radius = None, None, (2, 2, 2), fine.A.radius()
        else:
            A = operator_at(level)
            if not A.is_symmetric():
                raise ValueError(f"{who}: the stencil of level {level} is not symmetric")
            w = self.omega / _centre(who, A)
            need = tuple(max(2, r) for r in _face_radius(A))
            radius = A.radius()
        if any(s[a] // 2 < need[a] for _, _, s in subs for a in range(3)):
            return None
        cdd = DistributedDomain(*(n // 2 for n in fdd.size), backend=fdd.backend_kind,
                                device=fdd.torch_device)
        cdd.set_radius(radius)
        cdd.set_placement(fdd.strategy)
        cdd.set_methods(fdd.methods)
        cdd.set_gpus(fdd.gpus)
        e = cdd.add_data(dt, "e")
        f = cdd.add_data(dt, "f")
        k = d = None
        if self._variable:
            k = cdd.add_data(dt, "k")
            d = cdd.add_data(dt, "d")
            cdd.set_exchange_groups([[e.index], [k.index]])
        else:
            cdd.set_exchange_groups([[e.index]])
        spec = fdd.boundary
        if spec is not None:
            for a in range(3):
                if spec.periodic[a]:
                    continue
                for s in (0, 1):
                    kind = spec.kind(fine.e.index, a, s)
                    value = spec.value(fine.e.index, a, s)
                    cdd.set_boundary(FACES[2 * a + s], kind, 0 if value is None else value)
                    if k is not None:
                        cdd.set_boundary(FACES[2 * a + s], Boundary.CLAMP, quantities=[k])
        cpl, fpl = cdd.do_placement(), fdd.placement
        if tuple(cpl.dim()) != tuple(fpl.dim()):
            return None
        for idx, o, s in subs:
            if (tuple(cpl.subdomain_origin(idx)) != tuple(c // 2 for c in o)
                    or tuple(cpl.subdomain_size(idx)) != tuple(c // 2 for c in s)
                    or cpl.get_rank(idx) != fpl.get_rank(idx)
                    or cpl.get_subdomain_id(idx) != fpl.get_subdomain_id(idx)
                    or cpl.get_cuda(idx) != fpl.get_cuda(idx)):
                return None
        cdd.realize()
        fine.transfer = GridTransfer(fdd, cdd)
        if self._variable:
            # doubled spacing, the same sigma; k and d are filled by
            # refresh_coefficients()
            A = DiffusionOperator(cdd, k, 1, spacing=tuple(2.0 * s for s in fine.A.spacing),
                                  sigma=fine.A.sigma, dinv=d)
        return _Level(cdd, A, w, e, f, 0)

    def refresh_coefficients(self):
        """after the coefficient k of level 0 changed (DiffusionOperator
        hierarchies only): exchange k, restrict it level by level (the mean
        of the 8 children, then one exchange) and recompute every level's
        d = omega / diag."""
        if not self._variable:
            raise ValueError("GeometricMultigrid.refresh_coefficients: the hierarchy was built "
                             "from constant-coefficient stencils")
        for l, lv in enumerate(self._levels):
            if l > 0:
                fine = self._levels[l - 1]
                fine.transfer.restrict(1.0, fine.A.k, 0.0, fine.A.k, lv.A.k)
            lv.A.refresh()
            lv.A.inv_diagonal(self.omega, lv.A.dinv)
            lv.dd.backend.sync_compute()

    # ---- the cycle ----
    def apply(self, f: DataHandle, e: DataHandle):
        """curr[e] = M curr[f] on level 0; f is read only. e is the quantity
        given to the constructor, f another one of the same type."""
        if not isinstance(e, DataHandle) or e.index != self._levels[0].e.index:
            raise ValueError("GeometricMultigrid.apply: e is not the quantity the cycle was "
                             "built for")
        if not isinstance(f, DataHandle) or f.index == e.index or f.dtype != e.dtype:
            raise ValueError("GeometricMultigrid.apply: f must be another quantity of e's type")
        self._cycle(0, f)

    def _operator(self, lv: _Level, overlap: bool):
        """next[e] = A e, halos refreshed; enqueued, stream 0 may go on"""
        dd = lv.dd
        dd.backend.sync_compute()  # the exchange reads e on other streams
        overlapped_apply(dd, lv.apply, lv.group, overlap)
        if overlap:
            dd.backend.sync_compute()  # the exterior slabs ran on stream 1

    def _sweep(self, lv: _Level, f: DataHandle, overlap: bool):
        self._operator(lv, overlap)
        if lv.w is None:
            lv.dd.scaled_update(1.0, lv.e, lv.A.dinv, 1.0, f, -1.0, Next(lv.e), out=lv.e)
        else:
            lv.dd.axpbypcz(1.0, lv.e, lv.w, f, -lv.w, Next(lv.e), out=lv.e)

    def _cycle(self, l: int, f: DataHandle):
        lv = self._levels[l]
        last = l == len(self._levels) - 1
        overlap = self.overlap and l == 0
        key = f"level{l}"
        t0 = time.perf_counter()
        if lv.w is None:
            lv.dd.scaled_update(0.0, f, lv.A.dinv, 1.0, f, 0.0, f, out=lv.e)
        else:
            lv.dd.axpby(lv.w, f, 0.0, f, out=lv.e)
        for _ in range((self.coarse_sweeps if last else self.nu) - 1):
            self._sweep(lv, f, overlap)
        if not last:
            coarse = self._levels[l + 1]
            self._operator(lv, overlap)
            lv.transfer.restrict(1.0, f, -1.0, Next(lv.e), coarse.f)
            self.phase_times[key] += time.perf_counter() - t0
            self._cycle(l + 1, coarse.f)
            t0 = time.perf_counter()
            lv.transfer.prolong_add(coarse.e, lv.e)
            for _ in range(self.nu):
                self._sweep(lv, f, overlap)
        lv.dd.backend.sync_compute()
        self.phase_times[key] += time.perf_counter() - t0
