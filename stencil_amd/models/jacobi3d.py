"""Jacobi-3D heat-diffusion app (the flagship benchmark workload).

Reference: bin/jacobi3d.cu — 7-point radius-1 fp32 Jacobi with fixed
hot/cold sphere sources, overlapping interior compute with the halo
exchange and then computing the exterior shells.
"""
from __future__ import annotations

import time
from typing import List, Optional

import numpy as np

from ..core import DistributedDomain
from ..parallel.placement import PlacementStrategy


class Jacobi3D:
    def __init__(
        self,
        size,
        backend: str = "native",
        gpus: Optional[List[int]] = None,
        placement: PlacementStrategy = PlacementStrategy.NodeAware,
        device: str = "cpu",
        radius: int = 1,
        halo_multiplier: int = 1,
        boundary=None,
    ):
        """radius >= 1: halo depth (the 7-point kernel reads 1 cell; deeper
        radii exercise the deeper-halo exchange, reference jacobi3d-strong
        r=2 configuration).

        halo_multiplier m > 1 enables communication-avoiding temporal
        blocking (the reference's v3 wish-list item, README.md:313-315):
        halos are allocated and exchanged m*radius deep every m-th step;
        between exchanges each step computes a region EXPANDED into the
        still-valid halo by (m-1-phase)*radius cells. Results are
        identical to exchanging every step.

        boundary: {face: kind | (kind, value)} forwarded to
        DistributedDomain.set_boundary (faces "x-".."z+", "x", "y", "z",
        "all"); None = fully periodic. OPEN is rejected: the fast
        kernel's free row extension scribbles on next-buffer x halos and
        relies on the exchange refreshing them, which an OPEN face never
        does. halo_multiplier > 1 needs every axis periodic (the expanded
        compute region would leave the global domain). With a
        non-periodic axis the multi-rank step graphs fall back to the
        eager path; the single-domain graph captures the fill."""
        assert halo_multiplier >= 1
        self.m = int(halo_multiplier)
        self.kernel_radius = int(radius)
        self._phase = 0
        self.dd = DistributedDomain(*size, backend=backend, device=device)
        self.dd.set_radius(radius * self.m)
        self.dd.set_placement(placement)
        if gpus is not None:
            self.dd.set_gpus(gpus)
        self.h = self.dd.add_data(np.float32, "temp")
        if boundary:
            from ..boundary import Boundary

            for face, spec in boundary.items():
                kind, value = spec if isinstance(spec, (tuple, list)) else (spec, 0)
                if Boundary(kind) == Boundary.OPEN:
                    raise ValueError(
                        "Jacobi3D does not support OPEN boundaries (the kernel's row "
                        "extension overwrites x halos the exchange must refresh)"
                    )
                self.dd.set_boundary(face, kind, value)
            if self.m > 1 and not all(self.dd.periodic):
                raise ValueError("halo_multiplier > 1 needs every axis periodic")

    def realize(self):
        self.dd.realize()
        self.interiors = self.dd.get_interior()
        self.exteriors = self.dd.get_exterior()
        self.compute_lo, self.compute_hi = (0, 0, 0), self.dd.size
        # initial condition: (HOT+COLD)/2 everywhere, both buffers
        for li in range(self.dd.num_local()):
            lo, hi = self.dd.local_rect(li)
            for next_buf in (False, True):
                self.dd.backend.fill_f32(li, self.h.index, lo, hi, 0.5, next_buf)
        self.dd.backend.sync_compute()
        # whole-step hipGraph fast path: the single-process single-domain
        # periodic self-wrap shape (the N=1 bench) replays a captured
        # [translate -> jacobi -> device table swap] graph per step,
        # removing ~0.25 ms/step of host orchestration at 750^3. The
        # capture is serial: overlap measured no better at this shape
        # (docs/DESIGN.md).
        # When every axis is periodic the graph is the stencil kernel
        # ALONE: it reads the wrapped neighbour from the far side of the
        # buffer, so no translate fills a halo and the table swap moves
        # out of the graph (one swap after an odd run(n); see
        # csrc/src/jacobi.hip jacobi_graph_create; STENCIL_JAC_WRAP=0
        # restores the translate graph; so does a row length without
        # room for the kernel's row extension, (X + 2r) % 64 == 0 unless
        # the rect is aligned as it is). Halos are then STALE after
        # step()/run() until the next dd.exchange(): read_global over a
        # region that includes halo cells shows old values there. With a
        # non-periodic face the graph is [translate -> boundary fill ->
        # jacobi -> swap] as before.
        # The wrap graph also holds a fused two-step kernel: run(n)
        # replays n // 2 of those (one pass over memory per two steps,
        # the intermediate step never reaches memory) and one single
        # step if n is odd; step() is always a single step. Each replay
        # is one buffer swap, so after a fused pair the NEXT buffer holds
        # time t, not t+1. Same bits as single steps;
        # STENCIL_JAC_FUSE2=0 forces single-step replays.
        import os

        self._graph = None
        self._mr_graph = None
        graphs_on = os.environ.get("STENCIL_AMD_STEP_GRAPH", "1") != "0"
        staged_local = any(getattr(self.dd.backend, "_staged_local", []))
        if (
            self.m == 1
            and self.dd.backend_kind == "native"
            and self.dd.comm.world_size == 1
            and self.dd.num_local() == 1
            and graphs_on
            and not staged_local
        ):
            lo, hi = self.dd.local_rect(0)
            self._graph = self.dd.backend.jacobi_graph_create(
                0, self.h.index, lo, hi, self.compute_lo, self.compute_hi
            )
        elif (
            self.m == 1
            and self.dd.backend_kind == "native"
            and self.dd.comm.world_size > 1
            and self.dd.num_local() == 1
            and graphs_on
            and getattr(self.dd.backend, "_ipc_active", False)
            and not any(getattr(self.dd.backend, "_has_wire", [True]))
            and not staged_local
            and self.dd.boundary is None  # non-periodic: eager path (fill not captured)
        ):
            # multi-rank whole-step graphs (single-node 1-rank/GPU shape:
            # every cross-rank halo is an IPC direct write or staged thin
            # pack, so the step is two graphs around the colo barrier;
            # see csrc/src/jacobi.hip jacobi_mr_graph_create)
            from .. import _C

            b = self.dd.backend
            ilo, ihi = self.interiors[0]
            self._mr_graph = _C.jacobi_mr_graph_create(
                b.engine, 0, self.h.index,
                _C.Rect3(_C.Vec3(*ilo), _C.Vec3(*ihi)),
                _C.Rect3(_C.Vec3(*self.compute_lo), _C.Vec3(*self.compute_hi)),
                [_C.Rect3(_C.Vec3(*blo), _C.Vec3(*bhi)) for blo, bhi in self.exteriors[0]],
                extend_vec=2,
            )

    def _mr_step(self, sync: bool = True):
        """one queued multi-rank graph step: A, barrier, B (see realize)"""
        from .. import _C

        b = self.dd.backend
        _C.jacobi_mr_graph_pre(self._mr_graph)
        if b._colo_wire is not None:
            # all-reduce posted on the graph stream: fully stream-ordered
            b._colo_wire.barrier(_C.jacobi_mr_graph_stream(self._mr_graph))
        else:
            # host barrier (shared-device/test configs): A must be done
            # before signalling, B only after every rank signalled
            import torch.distributed as dist

            _C.jacobi_mr_graph_sync(self._mr_graph)
            dist.barrier(group=b._colo_group)
        _C.jacobi_mr_graph_post(self._mr_graph)
        b._colo_parity[0] ^= 1  # keep the eager path's mirror in sync
        if sync or b._colo_wire is None:
            _C.jacobi_mr_graph_sync(self._mr_graph)

    def step(self, overlap: bool = True):
        dd = self.dd
        if self.m > 1:
            self._step_multiplied()
            return
        if self._graph is not None:
            dd.backend.jacobi_graph_step(self._graph, 1)
            return
        if self._mr_graph is not None:
            if overlap:
                self._mr_step()
                return
            # the graph's parity cannot be resynced once an eager step
            # interleaves; degrade one-way to the eager path (dropping the
            # last reference frees the graph's streams and graph execs)
            self._mr_graph = None
        self._eager_step(overlap)

    def run(self, n: int) -> float:
        """n steps with one host sync at the end, returning elapsed
        seconds: in graph mode the n replays queue back-to-back, hiding
        the ~0.1 ms/step of hipGraphLaunch + stream-sync wake latency
        (measured gpu23: 1.132 ms GPU-busy vs 1.263 ms walled per step
        at 750^3)"""
        t0 = time.perf_counter()
        if self._graph is not None and self.m == 1:
            from .. import _C

            _C.jacobi_graph_launch(self._graph, n)
            _C.jacobi_graph_sync(self._graph)
        elif self._mr_graph is not None and self.m == 1:
            from .. import _C

            # with the device barrier the n steps queue back-to-back and
            # only the final sync touches the host
            for _ in range(n):
                self._mr_step(sync=False)
            _C.jacobi_mr_graph_sync(self._mr_graph)
        else:
            for _ in range(n):
                self.step()
        return time.perf_counter() - t0

    def _eager_step(self, overlap: bool = True):
        dd = self.dd
        # pure-vector + LDS-rows fast path (see csrc/src/jacobi.hip
        # plan_jacobi). Mode 1 (free row extension) is valid when the
        # extended cells are discard-safe LOCALLY: single process, or
        # multi-rank without direct IPC writes (an IPC peer running one
        # exchange ahead writes our next-buffer halos during our compute,
        # which the extension would race). IPC ranks use mode 2: the fast
        # kernel engages only when the region is already aligned -- which
        # the allocation pad arranges for the overlap interior. m>1 is
        # excluded: temporal blocking keeps halo data live across phases.
        ext_mode = 0
        if dd.backend_kind == "native" and self.m == 1:
            ext_mode = 2 if getattr(dd.backend, "_ipc_active", False) else 1
        if overlap:
            # interior compute (on compute streams) overlaps the exchange
            for li in range(dd.num_local()):
                ilo, ihi = self.interiors[li]
                dd.backend.jacobi_step(li, self.h.index, ilo, ihi, self.compute_lo,
                                       self.compute_hi, extend_vec=ext_mode)
            dd.exchange()
            # exterior shells: in mode 1 the +-x slabs intersect the
            # interior's row extension, so they go on stream 0 ORDERED
            # AFTER the interior kernel (their correct values must land
            # last); y/z slabs only touch rows the interior never writes
            # and stay concurrent on the second compute stream. An x slab
            # is one whose x range lies outside the interior's (slabs are
            # `radius` wide: a width threshold would miss radius >= 3)
            for li in range(dd.num_local()):
                ilo, ihi = self.interiors[li]
                for blo, bhi in self.exteriors[li]:
                    x_slab = ext_mode == 1 and (bhi[0] <= ilo[0] or blo[0] >= ihi[0])
                    dd.backend.jacobi_step(
                        li, self.h.index, blo, bhi, self.compute_lo, self.compute_hi,
                        stream_id=0 if x_slab else 1,
                    )
        else:
            dd.exchange()
            for li in range(dd.num_local()):
                lo, hi = dd.local_rect(li)
                dd.backend.jacobi_step(li, self.h.index, lo, hi, self.compute_lo,
                                       self.compute_hi, extend_vec=ext_mode)
        dd.backend.sync_compute()
        dd.swap()

    def _step_multiplied(self):
        """temporal-blocking step: exchange every m-th call, compute an
        expanded region in between (expansion shrinks by kernel_radius per
        phase, reaching the exact compute region just before the next
        exchange)"""
        dd = self.dd
        if self._phase == 0:
            dd.exchange()
        e = (self.m - 1 - self._phase) * self.kernel_radius
        for li in range(dd.num_local()):
            lo, hi = dd.local_rect(li)
            glo = tuple(c - e for c in lo)
            ghi = tuple(c + e for c in hi)
            dd.backend.jacobi_step(li, self.h.index, glo, ghi, self.compute_lo, self.compute_hi)
        dd.backend.sync_compute()
        dd.swap()
        self._phase = (self._phase + 1) % self.m
