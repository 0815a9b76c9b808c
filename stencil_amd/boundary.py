"""Non-periodic boundary conditions: the public Boundary enum, the
per-quantity per-face specification DistributedDomain.set_boundary builds,
and the geometry both backends share (which halo regions point out of the
global domain).

Semantics (every layer and the tests agree on this): the halo cells outside
the global domain hold what padding the global array one axis at a time in
the order x, y, z would produce -- each pass over the full extent the
earlier passes produced -- with numpy pad mode `constant` (FIXED), `edge`
(CLAMP), `symmetric` (MIRROR), negated `symmetric` (ANTIMIRROR) or `wrap`
(a periodic axis). OPEN cells are never written.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _C

Boundary = _C.Boundary

FACES = ("x-", "x+", "y-", "y+", "z-", "z+")

Vec = Tuple[int, int, int]


def parse_face(face: str) -> List[int]:
    """face indices (2 * axis + side) named by "x-", ..., "x", "y", "z", "all\""""
    if face == "all":
        return list(range(6))
    if face in FACES:
        return [FACES.index(face)]
    if face in ("x", "y", "z"):
        a = "xyz".index(face)
        return [2 * a, 2 * a + 1]
    raise ValueError(f"unknown face {face!r} (want one of {FACES}, 'x', 'y', 'z', 'all')")


def face_radius(radius, axis: int, side: int) -> int:
    return (radius.x, radius.y, radius.z)[axis](1 if side else -1)


class BoundarySpec:
    """resolved boundary: `periodic` per axis, and per quantity a list of
    six (kind, value) face entries (value: the FIXED constant as a numpy
    scalar of the quantity's dtype)"""

    def __init__(self, size: Vec, dtypes: Sequence[np.dtype], requests):
        self.size = tuple(size)
        self.dtypes = list(dtypes)
        nq = len(self.dtypes)
        self.faces = [[(Boundary.PERIODIC, None)] * 6 for _ in range(nq)]
        for faces, kind, value, qis in requests:
            for qi in range(nq) if qis is None else qis:
                if not 0 <= qi < nq:
                    raise ValueError(f"set_boundary: no quantity {qi}")
                v = np.array(value, dtype=self.dtypes[qi])[()] if kind == Boundary.FIXED else None
                for f in faces:
                    self.faces[qi][f] = (kind, v)
        per = []
        for a in range(3):
            kinds = [self.faces[qi][2 * a + s][0] for qi in range(nq) for s in (0, 1)]
            n_per = sum(k == Boundary.PERIODIC for k in kinds)
            if 0 < n_per < len(kinds):
                raise ValueError(
                    f"axis {'xyz'[a]} mixes PERIODIC with non-periodic faces: periodicity "
                    "is a property of the whole axis, for all quantities"
                )
            per.append(n_per == len(kinds))
        self.periodic = tuple(per)

    @property
    def any_nonperiodic(self) -> bool:
        return not all(self.periodic)

    def kind(self, qi: int, axis: int, side: int):
        return self.faces[qi][2 * axis + side][0]

    def value(self, qi: int, axis: int, side: int):
        return self.faces[qi][2 * axis + side][1]

    def validate(self, placement, radius):
        """the checks that need the partition (called from realize)"""
        dim = placement.dim()
        for a in range(3):
            if self.periodic[a]:
                continue
            min_ext = self.size[a]
            for i in range(dim[a]):
                idx = [0, 0, 0]
                idx[a] = i
                min_ext = min(min_ext, placement.subdomain_size(tuple(idx))[a])
            for qi, dt in enumerate(self.dtypes):
                for s in (0, 1):
                    k = self.kind(qi, a, s)
                    r = face_radius(radius, a, s)
                    if k in (Boundary.MIRROR, Boundary.ANTIMIRROR) and r > min_ext:
                        raise ValueError(
                            f"{k.name} on face {FACES[2 * a + s]}: radius {r} exceeds the "
                            f"smallest subdomain extent {min_ext} on that axis"
                        )
                    if k == Boundary.CLAMP and min_ext < 1:
                        raise ValueError(f"CLAMP on face {FACES[2 * a + s]}: empty extent")
                    if k == Boundary.ANTIMIRROR and not (
                        dt.kind == "f" and dt.itemsize in (2, 4, 8)
                    ):
                        raise ValueError(
                            f"ANTIMIRROR needs an IEEE float quantity of 2, 4 or 8 bytes; "
                            f"quantity {qi} is {dt}"
                        )

    def out_regions(self, radius, origin: Vec, sz: Vec):
        """the halo regions of a subdomain the fill owns: directions d with
        radius.dir(d) != 0 that point out of the global domain on at least
        one non-periodic axis. Yields (d, out) with out[a] True where d
        leaves the global domain on non-periodic axis a."""
        for dz in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    d = (dx, dy, dz)
                    if d == (0, 0, 0) or radius.dir(dx, dy, dz) == 0:
                        continue
                    out = tuple(
                        (not self.periodic[a])
                        and (
                            (d[a] < 0 and origin[a] == 0)
                            or (d[a] > 0 and origin[a] + sz[a] == self.size[a])
                        )
                        for a in range(3)
                    )
                    if any(out):
                        yield d, out


def make_spec(size, dtypes, requests) -> Optional[BoundarySpec]:
    if not requests:
        return None
    spec = BoundarySpec(size, dtypes, requests)
    return spec if spec.any_nonperiodic else None
