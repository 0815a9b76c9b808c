"""Stencil: a constant-coefficient linear stencil described as data.

A stencil is a set of taps (dx, dy, dz) -> weight. Applying it computes

    next[dst](p) = sum_k  w_k * curr[src](p + o_k)

for every cell p of a region. `Stencil.radius()` derives the minimal
per-direction `Radius` that makes every read legal, so the halo exchange
moves exactly what the stencil reads: a star stencil exchanges no edges or
corners, an upwind stencil allocates no downwind halo.

The taps are applied by `DistributedDomain.apply_stencil` /
`step_stencil` (gfx950 kernels in csrc/src/stencil_op.hip on the native
backend, tensor slicing on the torch backend).
"""
from __future__ import annotations

import itertools
import math
import numbers
from typing import Dict, Iterable, List, Sequence, Tuple

from . import _C

Offset = Tuple[int, int, int]

MAX_TAPS = 128
MAX_OFFSET = 8

# standard central second-derivative coefficients: (centre, [k=1, k=2, ...])
_D2_COEFFS = {
    2: (-2.0, [1.0]),
    4: (-5.0 / 2.0, [4.0 / 3.0, -1.0 / 12.0]),
    6: (-49.0 / 18.0, [3.0 / 2.0, -3.0 / 20.0, 1.0 / 90.0]),
    8: (-205.0 / 72.0, [8.0 / 5.0, -1.0 / 5.0, 8.0 / 315.0, -1.0 / 560.0]),
}


def _sign(v: int) -> int:
    return (v > 0) - (v < 0)


class Stencil:
    """taps (dx, dy, dz) -> weight; weights are Python floats (fp64) and
    are rounded once to the quantity's type at launch"""

    __slots__ = ("_taps",)

    def __init__(self, offsets: Iterable[Sequence[int]], weights: Iterable[float]):
        offsets = list(offsets)
        weights = list(weights)
        if len(offsets) != len(weights):
            raise ValueError(f"{len(offsets)} offsets but {len(weights)} weights")
        taps: Dict[Offset, float] = {}
        for o, w in zip(offsets, weights):
            if len(o) != 3:
                raise ValueError(f"offset {o!r} is not (dx, dy, dz)")
            if any(int(c) != c for c in o):
                raise ValueError(f"offset {o!r} is not integral")
            o = (int(o[0]), int(o[1]), int(o[2]))
            if any(abs(c) > MAX_OFFSET for c in o):
                raise ValueError(f"offset {o} exceeds |component| <= {MAX_OFFSET}")
            w = float(w)
            if not math.isfinite(w):
                raise ValueError(f"non-finite weight {w} at offset {o}")
            taps[o] = taps.get(o, 0.0) + w
        for o, w in taps.items():
            if not math.isfinite(w):
                raise ValueError(f"non-finite merged weight at offset {o}")
        # duplicates are merged above; taps that cancel to exactly 0 vanish
        taps = {o: w for o, w in taps.items() if w != 0.0}
        if not taps:
            raise ValueError("empty stencil (no tap with a nonzero weight)")
        if len(taps) > MAX_TAPS:
            raise ValueError(f"{len(taps)} taps; at most {MAX_TAPS} are supported")
        # deterministic order: z, then y, then x
        self._taps = dict(sorted(taps.items(), key=lambda t: (t[0][2], t[0][1], t[0][0])))

    # ---- factories ----
    @classmethod
    def identity(cls) -> "Stencil":
        return cls([(0, 0, 0)], [1.0])

    @classmethod
    def star(cls, wx: Sequence[float], wy: Sequence[float], wz: Sequence[float]) -> "Stencil":
        """per-axis weight lists, each of odd length 2r+1 and centred: entry
        i of an axis list weighs offset i - r on that axis. The three
        centre entries merge into one centre tap."""
        offsets: List[Offset] = []
        weights: List[float] = []
        for axis, ws in enumerate((wx, wy, wz)):
            ws = list(ws)
            if len(ws) % 2 != 1:
                raise ValueError("star(): each axis list needs an odd length 2r+1")
            r = len(ws) // 2
            for i, w in enumerate(ws):
                o = [0, 0, 0]
                o[axis] = i - r
                offsets.append(tuple(o))
                weights.append(w)
        return cls(offsets, weights)

    @classmethod
    def laplacian(cls, order: int = 2, spacing: Sequence[float] = (1.0, 1.0, 1.0)) -> "Stencil":
        """central-difference Laplacian of the given accuracy order (2, 4, 6
        or 8; radius order/2) on a grid with per-axis `spacing`"""
        if order not in _D2_COEFFS:
            raise ValueError(f"laplacian order must be one of {sorted(_D2_COEFFS)}, got {order}")
        if len(spacing) != 3 or any(not (float(h) > 0 and math.isfinite(float(h))) for h in spacing):
            raise ValueError(f"spacing must be three positive finite numbers, got {spacing!r}")
        c0, side = _D2_COEFFS[order]
        axes = []
        for h in spacing:
            s = 1.0 / (float(h) * float(h))
            axes.append([c * s for c in reversed(side)] + [c0 * s] + [c * s for c in side])
        return cls.star(*axes)

    @classmethod
    def advection(cls, velocity: Sequence[float], spacing: Sequence[float] = (1.0, 1.0, 1.0),
                  scheme: str = "upwind") -> "Stencil":
        """v . grad for a constant velocity on a grid with per-axis
        `spacing`. "upwind" is first order and reads only against the flow:
        per axis v_a (u_i - u_{i-1}) / h_a for v_a > 0, v_a (u_{i+1} - u_i)
        / h_a for v_a < 0, so radius() allocates no downwind halo.
        "central" is v_a (u_{i+1} - u_{i-1}) / (2 h_a). An axis with
        v_a == 0 gets no tap. ValueError for a non-finite velocity, a zero
        velocity on every axis and an unknown scheme."""
        if scheme not in ("upwind", "central"):
            raise ValueError(f"advection scheme is 'upwind' or 'central', got {scheme!r}")
        if len(velocity) != 3 or any(not math.isfinite(float(v)) for v in velocity):
            raise ValueError(f"velocity must be three finite numbers, got {velocity!r}")
        if all(float(v) == 0.0 for v in velocity):
            raise ValueError("advection(): the velocity is zero on every axis")
        if len(spacing) != 3 or any(not (float(h) > 0 and math.isfinite(float(h))) for h in spacing):
            raise ValueError(f"spacing must be three positive finite numbers, got {spacing!r}")
        offsets: List[Offset] = []
        weights: List[float] = []

        def tap(axis, k, w):
            o = [0, 0, 0]
            o[axis] = k
            offsets.append(tuple(o))
            weights.append(w)

        for a, (v, h) in enumerate(zip(velocity, spacing)):
            v, h = float(v), float(h)
            if v == 0.0:
                continue
            if scheme == "central":
                tap(a, 1, v / (2.0 * h))
                tap(a, -1, -v / (2.0 * h))
            elif v > 0.0:
                tap(a, 0, v / h)
                tap(a, -1, -v / h)
            else:
                tap(a, 1, v / h)
                tap(a, 0, -v / h)
        return cls(offsets, weights)

    @classmethod
    def from_array(cls, kernel_zyx, center: Sequence[int]) -> "Stencil":
        """dense box: kernel_zyx[k][j][i] weighs offset (i - cx, j - cy,
        k - cz) with center = (cx, cy, cz)"""
        import numpy as np

        k = np.asarray(kernel_zyx, dtype=np.float64)
        if k.ndim != 3:
            raise ValueError("from_array(): want a 3-D (z, y, x) array")
        if len(center) != 3:
            raise ValueError("from_array(): center is (cx, cy, cz)")
        cx, cy, cz = (int(c) for c in center)
        offsets, weights = [], []
        for (kz, ky, kx), w in np.ndenumerate(k):
            if w != 0.0:
                offsets.append((kx - cx, ky - cy, kz - cz))
                weights.append(float(w))
        return cls(offsets, weights)

    # ---- algebra ----
    def __add__(self, other: "Stencil") -> "Stencil":
        if not isinstance(other, Stencil):
            return NotImplemented
        return Stencil(self.offsets + other.offsets, self.weights + other.weights)

    def __mul__(self, c) -> "Stencil":
        if isinstance(c, Stencil) or not isinstance(c, numbers.Real):
            return NotImplemented
        return Stencil(self.offsets, [w * float(c) for w in self.weights])

    __rmul__ = __mul__

    def __neg__(self) -> "Stencil":
        return self * -1.0

    def __sub__(self, other: "Stencil") -> "Stencil":
        if not isinstance(other, Stencil):
            return NotImplemented
        return self + (-other)

    def __eq__(self, other) -> bool:
        return isinstance(other, Stencil) and self._taps == other._taps

    def __hash__(self):
        return hash(tuple(self._taps.items()))

    def __repr__(self) -> str:
        return f"Stencil(ntaps={self.ntaps}, is_star={self.is_star})"

    # ---- properties ----
    @property
    def offsets(self) -> List[Offset]:
        return list(self._taps.keys())

    @property
    def weights(self) -> List[float]:
        return list(self._taps.values())

    @property
    def ntaps(self) -> int:
        return len(self._taps)

    @property
    def is_star(self) -> bool:
        """every tap has at most one nonzero component"""
        return all(sum(c != 0 for c in o) <= 1 for o in self._taps)

    def is_symmetric(self) -> bool:
        """w(o) == w(-o) for every tap: on a periodic grid the operator is
        then a symmetric matrix (what conjugate gradients needs)"""
        return all(
            self._taps.get((-o[0], -o[1], -o[2])) == w for o, w in self._taps.items()
        )

    def symmetric_part(self) -> "Stencil":
        """the stencil with weights (w(o) + w(-o)) / 2: on a periodic grid
        the symmetric part (A + A^T) / 2 of the operator. For a first-order
        upwind advection it is -(|v_a| h_a / 2) times the second difference
        per axis, the scheme's numerical diffusion. ValueError when nothing
        is left (a skew stencil such as the central advection)."""
        offs = set(self._taps) | {(-o[0], -o[1], -o[2]) for o in self._taps}
        offs = sorted(offs, key=lambda o: (o[2], o[1], o[0]))
        return Stencil(offs, [
            (self._taps.get(o, 0.0) + self._taps.get((-o[0], -o[1], -o[2]), 0.0)) / 2.0
            for o in offs])

    def radius(self) -> "_C.Radius":
        """minimal Radius that makes every read legal. Face radii are the
        extreme offsets per side; an edge/corner direction e is nonzero iff
        some tap has sign(o_i) == e_i on every axis where e_i != 0 (the
        planner uses edge/corner radii only as a flag; extents come from
        the face radii), and then holds the largest face radius among
        those axes."""
        offs = self.offsets
        r = _C.Radius.constant(0)
        face = {}
        for a in range(3):
            face[(a, 1)] = max(max(o[a], 0) for o in offs)
            face[(a, -1)] = max(max(-o[a], 0) for o in offs)
        for e in itertools.product((-1, 0, 1), repeat=3):
            axes = [a for a in range(3) if e[a] != 0]
            if not axes:
                continue
            hit = any(all(_sign(o[a]) == e[a] for a in axes) for o in offs)
            r.set_dir(e[0], e[1], e[2], max(face[(a, e[a])] for a in axes) if hit else 0)
        return r

    def to_native(self) -> "_C.StencilTaps":
        t = _C.StencilTaps()
        t.offsets = [_C.Vec3(*o) for o in self.offsets]
        t.weights = self.weights
        return t
