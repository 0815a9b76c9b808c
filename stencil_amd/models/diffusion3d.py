"""Diffusion-3D: explicit heat diffusion written with the generic stencil
operator, u <- u + alpha_dt * laplacian(u), as ONE stencil
(identity + alpha_dt * laplacian(order)). The domain's radius is derived
from the stencil, so the exchange moves faces only (a star stencil reads
no edge or corner halo).
"""
from __future__ import annotations

import time
from typing import List, Optional

import numpy as np

from ..core import DistributedDomain
from ..parallel.placement import PlacementStrategy
from ..stencil import Stencil


class Diffusion3D:
    def __init__(
        self,
        size,
        order: int = 2,
        dtype=np.float32,
        alpha_dt: float = 0.1,
        backend: str = "native",
        gpus: Optional[List[int]] = None,
        boundary=None,
        placement: PlacementStrategy = PlacementStrategy.NodeAware,
        device: str = "cpu",
    ):
        """order: accuracy order of the Laplacian (2/4/6/8, radius order/2).
        alpha_dt: diffusivity * time step / spacing^2; explicit stability
        needs roughly alpha_dt <= 1/6 at order 2 (less at higher orders).

        boundary: {face: kind | (kind, value)} forwarded to
        DistributedDomain.set_boundary as Jacobi3D does; None = fully
        periodic. OPEN is allowed: the stencil operator writes nothing
        outside the region it is given, so nothing scribbles on halos."""
        self.stencil = Stencil.identity() + alpha_dt * Stencil.laplacian(order)
        self.dd = DistributedDomain(*size, backend=backend, device=device)
        self.dd.set_radius(self.stencil.radius())
        self.dd.set_placement(placement)
        if gpus is not None:
            self.dd.set_gpus(gpus)
        self.h = self.dd.add_data(np.dtype(dtype), "u")
        if self.h.dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
            raise ValueError(f"Diffusion3D supports float32/float64, got {self.h.dtype}")
        if boundary:
            for face, spec in boundary.items():
                kind, value = spec if isinstance(spec, (tuple, list)) else (spec, 0)
                self.dd.set_boundary(face, kind, value)

    def realize(self):
        self.dd.realize()

    def step(self, overlap: bool = True):
        self.dd.step_stencil(self.stencil, self.h, overlap=overlap)

    def run(self, n: int, overlap: bool = True) -> float:
        """n steps, returning elapsed seconds (each step ends in a sync)"""
        t0 = time.perf_counter()
        for _ in range(n):
            self.step(overlap)
        return time.perf_counter() - t0
