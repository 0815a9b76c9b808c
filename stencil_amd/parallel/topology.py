"""Stencil neighbor topology (periodic by default, per-axis mask).

Reference: include/stencil/topology.hpp, src/topology.cpp — neighbor lookup
wraps the subdomain index into the partition grid.
"""
from __future__ import annotations

from typing import Optional, Tuple

Vec = Tuple[int, int, int]


class Topology:
    """3D neighbor lookup over the partition grid of extent `dim`: a torus
    on every periodic axis, a bounded line on the others."""

    def __init__(self, dim: Vec, periodic=(True, True, True)):
        self.dim = tuple(int(c) for c in dim)
        self.periodic = tuple(bool(p) for p in periodic)

    def get_neighbor(self, idx: Vec, direction: Vec) -> Optional[Vec]:
        """wrapped neighbor index; None off a non-periodic edge"""
        out = []
        for i in range(3):
            c = idx[i] + direction[i]
            if not self.periodic[i] and not 0 <= c < self.dim[i]:
                return None
            out.append(c % self.dim[i])
        return tuple(out)


DIRECTIONS = [
    (x, y, z)
    for z in (-1, 0, 1)
    for y in (-1, 0, 1)
    for x in (-1, 0, 1)
    if (x, y, z) != (0, 0, 0)
]


def dir_key(d: Vec):
    """deterministic sort key for directions (z, y, x lexicographic)"""
    return (d[2], d[1], d[0])
