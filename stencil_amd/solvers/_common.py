"""What the Krylov solvers and the multigrid cycle share (private; cg.py and
bicgstab.py re-export the public names): the result record, the argument
checks of their constructors and the operator application with its halo
exchange. The host syncs around an application differ per caller on purpose
and stay with the callers."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List

import numpy as np

from ..boundary import FACES, Boundary
from ..core import DataHandle, DistributedDomain
from ..stencil import Stencil


@dataclass
class CGResult:
    converged: bool
    iterations: int
    # relative recursive residual norm sqrt(r.r / b.b) after each iteration;
    # entry 0 is the initial one (1.0 when x0 = 0)
    residuals: List[float] = field(default_factory=list)
    # "converged" | "max_iter" | "breakdown" | "zero_rhs" | "stagnated"
    reason: str = ""


def check_radius(who: str, dd: DistributedDomain, operator):
    """ValueError unless dd's radius covers the operator in every direction"""
    need = operator.radius()
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if (dx, dy, dz) != (0, 0, 0) and dd.radius.dir(dx, dy, dz) < need.dir(dx, dy, dz):
                    raise ValueError(
                        f"{who}: the domain's radius {dd.radius.dir(dx, dy, dz)} in "
                        f"direction {(dx, dy, dz)} does not cover the stencil's "
                        f"{need.dir(dx, dy, dz)}"
                    )


def check_faces(lead: str, dd: DistributedDomain, handles, allowed, tail: str):
    """ValueError unless the kind of every non-periodic face of the given
    quantities is in `allowed`, FIXED standing for FIXED(0). The message is
    lead + "boundary KIND on face F of quantity Q" + tail."""
    spec = dd.boundary
    if spec is None:
        return
    for h in handles:
        for a in range(3):
            if spec.periodic[a]:
                continue
            for s in (0, 1):
                k = spec.kind(h.index, a, s)
                if k not in allowed or (
                        k == Boundary.FIXED and float(spec.value(h.index, a, s)) != 0.0):
                    raise ValueError(f"{lead}boundary {k.name} on face {FACES[2 * a + s]} "
                                     f"of quantity {h.name or h.index}{tail}")


_COUNT = {4: "four", 5: "five"}


def check_quantities(who: str, dd: DistributedDomain, required, optional=(), groups=()):
    """The constructor checks of the quantities of a solver. ValueError
    unless dd is realized; `required`, (name,
    handle) pairs, are distinct DataHandles (TypeError for another type);
    each entry (wanted, handles, needs, stray) of `optional` holds, when
    wanted, further distinct DataHandles (ValueError(needs) otherwise) and
    only Nones when not (ValueError(stray) otherwise); all are of one
    float32/float64 dtype; and for each (handle, group, message) of
    `groups` the handle is in exchange group `group` (ValueError(message)
    otherwise, "{name}" in it standing for the handle's name or index).
    Messages are given without the leading "who: "."""
    if not dd._realized:
        raise ValueError(f"{who}: construct after dd.realize()")
    names = [n for n, _ in required]
    names = ", ".join(names[:-1]) + " and " + names[-1]
    hs = tuple(h for _, h in required)
    if any(not isinstance(h, DataHandle) for h in hs):
        raise TypeError(f"{who}: {names} are DataHandles")
    if len({h.index for h in hs}) != len(hs):
        raise ValueError(f"{who}: {names} must be {_COUNT[len(hs)]} distinct quantities")
    for wanted, more, needs, stray in optional:
        if wanted:
            if (any(not isinstance(h, DataHandle) for h in more)
                    or len({h.index for h in hs + tuple(more)}) != len(hs) + len(more)):
                raise ValueError(f"{who}: {needs}")
            hs = hs + tuple(more)
        elif any(h is not None for h in more):
            raise ValueError(f"{who}: {stray}")
    dt = hs[0].dtype
    if dt not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise ValueError(f"{who} supports float32/float64 quantities, got {dt}")
    if any(h.dtype != dt for h in hs):
        raise ValueError(f"{who}: the quantities must share one dtype, got "
                         + ", ".join(str(h.dtype) for h in hs))
    have = dd.exchange_groups or [list(range(len(dd._data)))]
    for h, g, message in groups:
        if not (isinstance(g, int) and 0 <= g < len(have) and h.index in have[g]):
            raise ValueError(f"{who}: " + message.replace("{name}", str(h.name or h.index)))


def operator_apply(dd: DistributedDomain, A, h: DataHandle, where):
    """next[h] = A curr[h] over `where`, A a Stencil or a DiffusionOperator"""
    if isinstance(A, Stencil):
        dd.apply_stencil(A, h, where=where)
    else:
        A.apply(h, where=where)


def overlapped_apply(dd: DistributedDomain, apply, group: int, overlap: bool):
    """apply(where) over every cell with the halos of `group` refreshed:
    the interior while they move, then the exterior (overlap), or the
    exchange first and then all. The syncs before and after are the
    caller's."""
    if overlap:
        apply("interior")
        dd.exchange(group)
        apply("exterior")
    else:
        dd.exchange(group)
        apply("all")
