"""DistributedDomain: the top-level orchestrator.

MI355X-native re-design of the reference's DistributedDomain
(reference: include/stencil/stencil.hpp:33-225, src/stencil.cu). One object
per process; a process may own several GPUs (single-process multi-GPU is the
primary mode on an 8x MI355X node: all halos then move by direct-write
kernels over xGMI with no process boundary at all), or one GPU per rank with
torch.distributed (RCCL) carrying cross-rank halos.
"""
from __future__ import annotations

import enum
import os
import time
from typing import Dict, List, Optional, Tuple

import numpy as np

from . import _C
from .boundary import Boundary, make_spec, parse_face
from .parallel.comm import Comm
from .parallel.placement import PlacementStrategy, gather_slots, make_placement
from .parallel.planning import plan_exchange

Vec = Tuple[int, int, int]

_NP_DTYPES = {1: np.uint8, 2: np.int16, 4: np.float32, 8: np.float64}


class Method(enum.Flag):
    """transport methods (reference: include/stencil/method.hpp). The MI355X
    mapping collapses the reference's 8 CUDA transports into the ones that
    make sense on xGMI-connected GPUs + RCCL."""

    NONE = 0
    DIRECT_KERNEL = 1  # same-process direct-write translate kernels (xGMI peer stores)
    RCCL = 2  # cross-process packed RCCL point-to-point
    IPC_KERNEL = 4  # colocated cross-process direct writes via HIP IPC over xGMI
    DEFAULT = DIRECT_KERNEL | RCCL | IPC_KERNEL


class DataHandle:
    __slots__ = ("index", "elem_size", "name", "dtype")

    def __init__(self, index: int, elem_size: int, name: str, dtype=None):
        self.index = index
        self.elem_size = elem_size
        self.name = name
        # the numpy view dtype for host-side access (read_global /
        # write_paraview); defaults to the size-canonical dtype
        self.dtype = np.dtype(dtype) if dtype is not None else np.dtype(_NP_DTYPES[elem_size])


class Next:
    """marks "the next buffer of this quantity" wherever a vector operation
    (dot, axpby) expects an operand; a bare DataHandle means curr"""

    __slots__ = ("handle",)

    def __init__(self, handle: DataHandle):
        if not isinstance(handle, DataHandle):
            raise TypeError("Next() wraps a DataHandle")
        self.handle = handle


def _np_dtype_of(dtype_or_size) -> np.dtype:
    """resolve an add_data() spec (torch dtype / numpy dtype / element
    size) to the numpy dtype used for host views. Kept alongside the
    element size so read_global/write_paraview never reinterpret e.g.
    int32 data as float32 (round-1 advisor finding)."""
    try:
        import torch

        if isinstance(dtype_or_size, torch.dtype):
            t = torch.tensor([], dtype=dtype_or_size)
            try:
                return t.numpy().dtype
            except Exception:  # no numpy equivalent (bf16...): raw view
                return np.dtype(_NP_DTYPES[t.element_size()])
    except ImportError:
        pass
    if isinstance(dtype_or_size, np.dtype):
        return dtype_or_size
    if isinstance(dtype_or_size, type) and issubclass(dtype_or_size, np.generic):
        return np.dtype(dtype_or_size)
    size = int(dtype_or_size)
    if size not in _NP_DTYPES:
        raise ValueError(f"unsupported element size {size} (want 1/2/4/8)")
    return np.dtype(_NP_DTYPES[size])


class DistributedDomain:
    def __init__(self, x: int, y: int, z: int, backend: str = "native", device: str = "cpu"):
        """backend: 'native' (C++/HIP, production) or 'torch' (reference
        implementation; `device` selects its tensor device)."""
        self.size: Vec = (int(x), int(y), int(z))
        self.backend_kind = backend
        self.torch_device = device
        self.radius = _C.Radius.constant(0)
        self._data: List[Tuple[int, str]] = []
        self._dtypes: List[np.dtype] = []
        self.methods = Method.DEFAULT
        self.strategy = PlacementStrategy.NodeAware
        self.gpus: Optional[List[int]] = None
        self.exchange_groups: Optional[List[List[int]]] = None
        self.output_prefix = os.environ.get("STENCIL_OUTPUT_PREFIX", "")
        self.comm = None
        self.placement = None
        self.backend = None
        self._realized = False
        # per-method exchanged bytes (one full exchange)
        self.bytes_by_method: Dict[str, int] = {"direct_kernel": 0, "rccl": 0, "ipc_kernel": 0}
        # physical boundaries (set_boundary): requests resolve at realize()
        self._bc_requests: List[tuple] = []
        self.boundary = None  # BoundarySpec when some axis is non-periodic
        self.boundary_bytes = 0  # bytes written by one full boundary fill
        self._boundary_lines: List[str] = []
        self.time_exchange = 0.0
        self.time_swap = 0.0
        # setup-phase timers (reference STENCIL_SETUP_STATS,
        # stencil.hpp:103-112)
        self.setup_times: Dict[str, float] = {}

    # ---- configuration (before realize) ----
    def set_radius(self, r):
        if isinstance(r, int):
            self.radius = _C.Radius.constant(r)
        else:
            self.radius = r

    def add_data(self, dtype_or_size, name: str = "") -> DataHandle:
        dt = _np_dtype_of(dtype_or_size)
        es = dt.itemsize
        self._data.append((es, name))
        self._dtypes.append(dt)
        return DataHandle(len(self._data) - 1, es, name, dt)

    def data_handle(self, index: int) -> DataHandle:
        """handle for an already-added quantity (dtype-preserving)"""
        es, name = self._data[index]
        return DataHandle(index, es, name, self._dtypes[index])

    def set_methods(self, m: Method):
        self.methods = m

    def set_placement(self, s: PlacementStrategy):
        self.strategy = s

    def set_gpus(self, gpus: List[int]):
        self.gpus = list(gpus)

    def set_exchange_groups(self, groups: List[List[int]]):
        """partition quantities into independently exchangeable groups;
        exchange(group=i) then moves only groups[i]'s quantities (e.g. the
        MHD solver exchanges its 8 physics fields and its 2 div fields at
        different points of a substep). Call before realize().

        At most 4 groups: each group needs 3 engine launch slots (wire
        packs + two staged-IPC parities) and the engine encodes 12
        (engine.hpp kGroups) — raise kGroups there to lift this."""
        seen = [q for g in groups for q in g]
        if sorted(seen) != sorted(set(seen)):
            raise ValueError("exchange groups must be disjoint")
        if len(groups) > 4:
            raise ValueError(
                "at most 4 exchange groups (engine launch-group encoding: "
                "3 slots per group x kGroups=12; see csrc engine.hpp)"
            )
        self.exchange_groups = [sorted(g) for g in groups]

    def set_boundary(self, face: str, kind: Boundary, value=0, quantities=None):
        """boundary kind of global face(s): `face` is "x-", "x+", "y-",
        "y+", "z-", "z+", an axis "x"/"y"/"z" (both faces) or "all".

        Kinds: PERIODIC (default; a property of a whole AXIS and of all
        quantities -- both faces of an axis are periodic or neither is),
        and on a non-periodic axis, per face and per quantity: OPEN (the
        library never touches those halo cells), FIXED(value), CLAMP
        (nearest interior cell), MIRROR (halo[-1-k] = interior[k]) and
        ANTIMIRROR (halo[-1-k] = -interior[k]; IEEE float quantities of
        2/4/8 bytes only). Edges and corners hold what padding the global
        array one axis at a time in the order x, y, z would give.

        `quantities`: handles or indices (None = all). The halos are
        re-imposed on the current buffer by every exchange of the
        quantity's group. Call before realize(); later calls override
        earlier ones. OPEN x faces do not mix with the jacobi kernel's
        free row extension (extend_vec=1), which scribbles on next-buffer
        x halos and relies on the exchange refreshing them."""
        if self._realized:
            raise ValueError("set_boundary() must be called before realize()")
        kind = Boundary(kind)
        faces = parse_face(face)
        qis = None
        if quantities is not None:
            qis = [q.index if isinstance(q, DataHandle) else int(q) for q in quantities]
            if kind == Boundary.PERIODIC:
                raise ValueError("PERIODIC applies to an axis for all quantities")
        self._bc_requests.append((faces, kind, value, qis))

    @property
    def periodic(self) -> Tuple[bool, bool, bool]:
        """per-axis periodicity as currently configured"""
        spec = make_spec(self.size, self._dtypes, self._bc_requests)
        return spec.periodic if spec is not None else (True, True, True)

    def set_output_prefix(self, p: str):
        self.output_prefix = p

    # ---- realize ----
    def _default_gpus(self) -> List[int]:
        n = _C.device_count()
        if self.backend_kind == "torch":
            return [0]  # torch backend does not need real devices on CPU
        if n == 0:
            raise RuntimeError("no HIP devices visible; use backend='torch' for CPU runs")
        comm = self.comm
        if comm.world_size == 1:
            return [0]
        # one GPU per colocated rank, round-robin (reference src/stencil.cu:74-85)
        colo = comm.colocated_ranks()
        local_rank = int(os.environ.get("LOCAL_RANK", colo.index(comm.rank)))
        return [local_rank % n]

    def do_placement(self):
        """compute partition + placement only (no allocation)"""
        t0 = time.perf_counter()
        self.comm = Comm()
        if self.gpus is None:
            self.gpus = self._default_gpus()
        slots = gather_slots(self.comm, self.gpus)
        self.setup_times["topo"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        self.placement = make_placement(self.strategy, self.size, self.radius, slots)
        self.setup_times["placement"] = time.perf_counter() - t0
        return self.placement

    def realize(self):
        if self._realized:
            raise RuntimeError("realize() called twice")
        if self.placement is None:
            self.do_placement()
        rank = self.comm.rank
        self.boundary = make_spec(self.size, self._dtypes, self._bc_requests)
        if self.boundary is not None:
            self.boundary.validate(self.placement, self.radius)
        periodic = self.boundary.periodic if self.boundary is not None else (True, True, True)
        n_local = self.placement.num_local(rank)
        specs = []
        for li in range(n_local):
            idx = self.placement.get_idx(rank, li)
            specs.append(
                (
                    self.placement.subdomain_size(idx),
                    self.placement.subdomain_origin(idx),
                    self.placement.get_cuda(idx),
                )
            )
        t0 = time.perf_counter()
        if self.backend_kind == "native":
            from .native_backend import NativeBackend

            self.backend = NativeBackend(specs, self._data, self.radius, self.exchange_groups)
        else:
            from .torch_backend import TorchBackend

            self.backend = TorchBackend(
                specs, self._data, self.radius, self.torch_device, self.exchange_groups
            )
        self.setup_times["realize"] = time.perf_counter() - t0

        t0 = time.perf_counter()
        plan = plan_exchange(self.placement, self.radius, rank, periodic)
        self.setup_times["plan"] = time.perf_counter() - t0
        if not (self.methods & Method.DIRECT_KERNEL) and plan.translates:
            raise RuntimeError("same-rank halos require Method.DIRECT_KERNEL")
        if not (self.methods & Method.RCCL) and (plan.sends or plan.recvs):
            raise RuntimeError("cross-rank halos require Method.RCCL")
        ctx = {
            "comm": self.comm,
            "placement": self.placement,
            "ipc": bool(self.methods & Method.IPC_KERNEL),
            "boundary": self.boundary,
        }
        t0 = time.perf_counter()
        self.backend.register_plan(plan, ctx)
        self.setup_times["create"] = time.perf_counter() - t0
        self.plan = plan
        self._boundary_lines = list(getattr(self.backend, "boundary_lines", []))
        self.boundary_bytes = int(getattr(self.backend, "boundary_bytes", 0))
        self._count_bytes(plan)
        if self.output_prefix:
            self._write_plan_files(plan)
        self._realized = True

    def _count_bytes(self, plan):
        es_total = sum(es for es, _ in self._data)
        self.bytes_by_method["direct_kernel"] = sum(
            t.ext[0] * t.ext[1] * t.ext[2] * es_total for t in plan.translates
        )
        colo = (
            set(self.comm.colocated_ranks()) - {self.comm.rank}
            if getattr(self.backend, "_ipc_active", False)
            else set()
        )
        self.bytes_by_method["ipc_kernel"] = sum(
            m.volume() * es_total for s in plan.sends if s.peer_rank in colo for m in s.messages
        )
        self.bytes_by_method["rccl"] = sum(
            m.volume() * es_total
            for s in plan.sends
            if s.peer_rank not in colo
            for m in s.messages
        )

    def exchange_bytes_for_method(self, method: Method) -> int:
        total = 0
        if method & Method.DIRECT_KERNEL:
            total += self.bytes_by_method["direct_kernel"]
        if method & Method.RCCL:
            total += self.bytes_by_method["rccl"]
        if method & Method.IPC_KERNEL:
            total += self.bytes_by_method["ipc_kernel"]
        return total

    # ---- iteration ----
    def exchange(self, group: int = 0):
        t0 = time.perf_counter()
        self.backend.exchange(group)
        self.time_exchange += time.perf_counter() - t0

    def exchange_begin(self, group: int = 0):
        """asynchronous exchange start (native backend): all device work is
        enqueued; call exchange_end() before reading halos"""
        if hasattr(self.backend, "exchange_begin"):
            self.backend.exchange_begin(group)
        # torch backend has no async path; everything happens in end()

    def exchange_end(self, group: int = 0):
        t0 = time.perf_counter()
        if hasattr(self.backend, "exchange_end"):
            self.backend.exchange_end(group)
        else:
            self.backend.exchange(group)
        self.time_exchange += time.perf_counter() - t0

    def swap(self):
        t0 = time.perf_counter()
        self.backend.swap()
        self.time_swap += time.perf_counter() - t0

    # ---- generic stencil operator ----
    def _stencil_dtype(self, src: DataHandle, dst: DataHandle) -> np.dtype:
        if src.dtype != dst.dtype:
            raise ValueError(f"apply_stencil: src is {src.dtype} but dst is {dst.dtype}")
        if src.dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
            raise ValueError(f"apply_stencil supports float32/float64 quantities, got {src.dtype}")
        return src.dtype

    def apply_stencil(self, stencil, src: DataHandle, dst: Optional[DataHandle] = None,
                      where="all", stream_id: Optional[int] = None):
        """next[dst] = stencil(curr[src]) on every local domain (dst=None:
        the same quantity; the kernel reads curr and writes next, so that
        is safe). `where` selects the cells: "all" (local_rect),
        "interior" (get_interior: cells whose taps read no halo),
        "exterior" (get_exterior slabs) or an explicit global box (lo, hi),
        which is applied as given on every local domain: it must lie inside
        each one's allocation together with the taps. Work is enqueued on compute
        stream `stream_id` (default: 1 for exterior slabs, 0 otherwise);
        call backend.sync_compute() before reading. The halos the stencil
        reads must be current (exchange()) except for where="interior".
        float32/float64 quantities only (ValueError otherwise, also for
        taps that reach outside the allocated halo)."""
        dst = src if dst is None else dst
        dt = self._stencil_dtype(src, dst)
        boxes, sid = self._operator_boxes("apply_stencil", where, stream_id)
        for li, bs in enumerate(boxes):
            for lo, hi in bs:
                self.backend.stencil_apply(li, src.index, dst.index, lo, hi, stencil, dt, sid)

    def _operator_boxes(self, op: str, where, stream_id: Optional[int]):
        """(per local domain: the boxes of `where`, the compute stream id)"""
        if isinstance(where, str):
            if where not in ("all", "interior", "exterior"):
                raise ValueError(f"{op}: where={where!r}")
            if where == "all":
                boxes = [[self.local_rect(li)] for li in range(self.num_local())]
            elif where == "interior":
                boxes = [[b] for b in self.get_interior()]
            else:
                boxes = self.get_exterior()
            sid = (1 if where == "exterior" else 0) if stream_id is None else stream_id
        else:
            lo, hi = where
            boxes = [[(tuple(lo), tuple(hi))] for _ in range(self.num_local())]
            sid = 0 if stream_id is None else stream_id
        return boxes, sid

    def apply_diffusion(self, k: DataHandle, src: DataHandle, dst: Optional[DataHandle] = None,
                        spacing=(1.0, 1.0, 1.0), sigma: float = 0.0, where="all",
                        stream_id: Optional[int] = None):
        """next[dst] = (sigma I - div(k grad)) curr[src] on every local
        domain (dst=None: the same quantity), k a cell-centred coefficient
        quantity of the same type:

            (A u)(p) = sigma u(p) + sum over a in {x,y,z}, s in {-1,+1} of
                       h_a * 0.5 (k(p) + k(p + s e_a)) * (u(p) - u(p + s e_a))

        with h_a = 1 / spacing_a^2. `where` and `stream_id` are those of
        apply_stencil. The face halos of src AND of k must be current
        (exchange() of their groups) except for where="interior"; edge and
        corner halos are never read. float32/float64 quantities only
        (ValueError otherwise, also for a box whose 1-cell face apron
        leaves the allocation). solvers/diffusion.py wraps this as an
        operator for ConjugateGradient and GeometricMultigrid."""
        dst = src if dst is None else dst
        dt = self._stencil_dtype(src, dst)
        if k.dtype != dt:
            raise ValueError(f"apply_diffusion: k is {k.dtype} but src is {dt}")
        h = [1.0 / (float(s) * float(s)) for s in spacing]
        boxes, sid = self._operator_boxes("apply_diffusion", where, stream_id)
        for li, bs in enumerate(boxes):
            for lo, hi in bs:
                self.backend.diffusion_apply(li, src.index, k.index, dst.index, lo, hi, h,
                                             float(sigma), dt, sid)

    def step_stencil(self, stencil, src: DataHandle, dst: Optional[DataHandle] = None,
                     overlap: bool = True):
        """one time step of a stencil update: overlap=True computes the
        interior while the halos move, then the exterior slabs (interior,
        exchange(), exterior, sync_compute, swap()); overlap=False is
        exchange, all, sync, swap. The domain's radius must cover the
        stencil (set_radius(stencil.radius()) is the minimal choice).
        Always eager: whole-step hipGraphs for this operator are out of
        scope (Jacobi3D has them for its fixed 7-point kernel)."""
        if overlap:
            self.apply_stencil(stencil, src, dst, where="interior")
            self.exchange()
            self.apply_stencil(stencil, src, dst, where="exterior")
        else:
            self.exchange()
            self.apply_stencil(stencil, src, dst, where="all")
        self.backend.sync_compute()
        self.swap()

    # ---- vector operations (the building blocks of solvers/) ----
    def _vector_operands(self, op: str, operands):
        """[(quantity index, next_buf)] of handles / Next(handle)s, all of
        one float type"""
        out, dt = [], None
        for o in operands:
            nxt = isinstance(o, Next)
            h = o.handle if nxt else o
            if not isinstance(h, DataHandle):
                raise TypeError(f"{op}: operands are DataHandles or Next(DataHandle)")
            if h.dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
                raise ValueError(f"{op} supports float32/float64 quantities, got {h.dtype}")
            if dt is not None and h.dtype != dt:
                raise ValueError(f"{op}: operands mix {dt} and {h.dtype}")
            dt = h.dtype
            out.append((h.index, nxt))
        return out

    def _vector_boxes(self, op: str, where):
        if isinstance(where, str):
            if where != "all":
                raise ValueError(f"{op}: where={where!r}")
            return [self.local_rect(li) for li in range(self.num_local())]
        lo, hi = where
        return [(tuple(lo), tuple(hi)) for _ in range(self.num_local())]

    def _global_sum(self, per_domain) -> float:
        """local domains in li order, then ranks in rank order: every rank
        computes the bitwise identical value (all ranks of a solver must
        take the same convergence branch). World 1 does no collective."""
        local = 0.0
        for v in per_domain:
            local += float(v)
        if self.comm.world_size == 1:
            return local
        total = 0.0
        for v in self.comm.allgather_object(local):
            total += v
        return total

    def dot(self, a, b=None, where="all") -> float:
        """GLOBAL inner product sum a(p) * b(p) (b=None: a . a) over every
        rank's cells: `where` is "all" (each local_rect) or a global box
        (lo, hi) applied as given on every local domain, as in
        apply_stencil. Operands are handles (curr) or Next(handle).
        Products and sums are in fp64 whatever the quantity type; the
        value is deterministic and bitwise identical on every rank. Blocks
        until the value is there (the native backend syncs the compute
        stream of each local domain once)."""
        (qa, na), (qb, nb) = self._vector_operands("dot", [a, a if b is None else b])
        boxes = self._vector_boxes("dot", where)
        return self._global_sum(self.backend.field_dot(boxes, qa, na, qb, nb))

    def axpby(self, alpha: float, x, beta: float, y, out, where="all"):
        """out = alpha * x + beta * y, element-wise in the quantity's type
        (alpha and beta are rounded to it once). out may be the buffer of x
        or of y. Enqueued on compute stream 0; backend.sync_compute()
        before another stream or the exchange reads the result."""
        (qx, nx), (qy, ny), (qo, no) = self._vector_operands("axpby", [x, y, out])
        boxes = self._vector_boxes("axpby", where)
        self.backend.field_axpby(boxes, float(alpha), qx, nx, float(beta), qy, ny, qo, no)

    def axpbypcz(self, alpha: float, x, beta: float, y, gamma: float, z, out, where="all"):
        """out = alpha * x + beta * y + gamma * z, the three-operand axpby
        (one 4-pass kernel): the relaxation update e += w (f - A e) of the
        multigrid smoother. out may be the buffer of any input. Enqueued on
        compute stream 0 like axpby."""
        (qx, nx), (qy, ny), (qz, nz), (qo, no) = self._vector_operands("axpbypcz", [x, y, z, out])
        boxes = self._vector_boxes("axpbypcz", where)
        self.backend.field_axpbypcz(boxes, float(alpha), qx, nx, float(beta), qy, ny,
                                    float(gamma), qz, nz, qo, no)

    def scaled_update(self, alpha: float, x, d, beta: float, y, gamma: float, z, out,
                      where="all"):
        """out = alpha * x + d * (beta * y + gamma * z), element-wise, with
        d a quantity (one 5-pass kernel): the diagonally scaled relaxation
        update e += (omega / diag) (f - A e) of the variable-coefficient
        smoother; with aliased operands also e = d f and the Jacobi
        preconditioner z = d r. out may be the buffer of any input.
        Enqueued on compute stream 0 like axpby."""
        (qx, nx), (qd, nd), (qy, ny), (qz, nz), (qo, no) = self._vector_operands(
            "scaled_update", [x, d, y, z, out])
        boxes = self._vector_boxes("scaled_update", where)
        self.backend.field_scaled_update(boxes, float(alpha), qx, nx, qd, nd, float(beta), qy, ny,
                                         float(gamma), qz, nz, qo, no)

    def cg_update(self, alpha: float, x, p, r) -> float:
        """the fused conjugate-gradient update over every local_rect:
        curr[x] += alpha * curr[p]; curr[r] -= alpha * next[p] (where
        apply_stencil(A, p) left A p); returns the GLOBAL sum of r_new^2,
        bitwise identical on every rank like dot()."""
        for h in (x, p, r):
            if not isinstance(h, DataHandle):
                raise TypeError("cg_update: x, p and r are DataHandles")
        (qx, _), (qp, _), (qr, _) = self._vector_operands("cg_update", [x, p, r])
        boxes = self._vector_boxes("cg_update", "all")
        return self._global_sum(self.backend.cg_update(boxes, float(alpha), qx, qp, qr))

    # The sums that the projection v - mean(v) off the constant null space
    # needs (solvers/cg.py, nullspace="constant"), each fused into a pass a
    # CG iteration makes anyway. Every returned scalar goes through
    # _global_sum on its own: bitwise identical on every rank.
    def _global_sums(self, per_domain, n: int):
        return tuple(self._global_sum([v[k] for v in per_domain]) for k in range(n))

    def sum(self, a, where="all") -> float:
        """GLOBAL sum of a(p), in fp64, deterministic like dot(); `where`
        and the operand (a handle or Next(handle)) as in dot(). Blocks
        until the value is there."""
        ((qa, na),) = self._vector_operands("sum", [a])
        boxes = self._vector_boxes("sum", where)
        return self._global_sum(self.backend.field_sum(boxes, qa, na))

    def dot_sums(self, a, b=None, where="all"):
        """(sum a * b, sum a, sum b), GLOBAL, from ONE pass over a and b
        (b=None: a with itself): dot()'s traffic, dot()'s determinism."""
        (qa, na), (qb, nb) = self._vector_operands("dot_sums", [a, a if b is None else b])
        boxes = self._vector_boxes("dot_sums", where)
        return self._global_sums(self.backend.field_dot_sums(boxes, qa, na, qb, nb), 3)

    def cg_update_sum(self, alpha: float, x, p, r):
        """cg_update (the same arithmetic on x and r, the same sum of
        r_new^2) returning (sum r_new^2, sum r_new), GLOBAL: the second
        value is what projecting r off the constants needs."""
        for h in (x, p, r):
            if not isinstance(h, DataHandle):
                raise TypeError("cg_update_sum: x, p and r are DataHandles")
        (qx, _), (qp, _), (qr, _) = self._vector_operands("cg_update_sum", [x, p, r])
        boxes = self._vector_boxes("cg_update_sum", "all")
        return self._global_sums(
            self.backend.cg_update_sum(boxes, float(alpha), qx, qp, qr), 2)

    def axpbyc(self, alpha: float, x, beta: float, y, c: float, out, where="all"):
        """out = alpha * x + beta * y + c, element-wise in the quantity's
        type (alpha, beta and c are rounded to it once): axpby plus a
        constant shift, at axpby's traffic. out may be the buffer of x or
        of y. Enqueued on compute stream 0 like axpby."""
        (qx, nx), (qy, ny), (qo, no) = self._vector_operands("axpbyc", [x, y, out])
        boxes = self._vector_boxes("axpbyc", where)
        self.backend.field_axpbyc(boxes, float(alpha), qx, nx, float(beta), qy, ny, float(c),
                                  qo, no)

    # The fused passes of BiCGStab (solvers/bicgstab.py). GLOBAL values like
    # dot(): bitwise identical on every rank.
    def axpby_norm2(self, alpha: float, x, beta: float, y, out, where="all") -> float:
        """out = alpha * x + beta * y exactly as axpby() writes it, and the
        GLOBAL sum of out^2 (the stored out, squares and sums in fp64) from
        the same pass: 3 passes where axpby + dot take 4. out may be the
        buffer of x or of y. Blocks until the value is there."""
        (qx, nx), (qy, ny), (qo, no) = self._vector_operands("axpby_norm2", [x, y, out])
        boxes = self._vector_boxes("axpby_norm2", where)
        return self._global_sum(self.backend.field_axpby_norm2(
            boxes, float(alpha), qx, nx, float(beta), qy, ny, qo, no))

    def dot_pair(self, a, b, where="all"):
        """(sum a * b, sum a * a), GLOBAL, from ONE pass over a and b:
        dot()'s traffic, and its first value has dot(a, b)'s bits."""
        (qa, na), (qb, nb) = self._vector_operands("dot_pair", [a, b])
        boxes = self._vector_boxes("dot_pair", where)
        return self._global_sums(self.backend.field_dot_pair(boxes, qa, na, qb, nb), 2)

    def bicgstab_update(self, alpha: float, y, omega: float, z, x, r, t, rhat):
        """the fused BiCGStab update over every local_rect:
        curr[x] += alpha * y + omega * z; curr[r] -= omega * t (curr[r]
        holds s on entry); returns the GLOBAL (sum r_new^2, sum rhat *
        r_new). x and r are handles; y, z, t and rhat handles or
        Next(handle). z may be the buffer of r (the unpreconditioned
        solver: 7 passes, otherwise 8). ValueError when x and r are not
        distinct from each other and from the buffers of y, t and rhat."""
        for h in (x, r):
            if not isinstance(h, DataHandle):
                raise TypeError("bicgstab_update: x and r are DataHandles")
        (qy, ny), (qz, nz), (qx, _), (qr, _), (qt, nt), (qh, nh) = self._vector_operands(
            "bicgstab_update", [y, z, x, r, t, rhat])
        boxes = self._vector_boxes("bicgstab_update", "all")
        return self._global_sums(
            self.backend.bicgstab_update(boxes, float(alpha), qy, ny, float(omega), qz, nz, qx, qr,
                                         qt, nt, qh, nh), 2)

    # ---- geometry queries ----
    def any_methods(self, m: Method) -> bool:
        """True if any of the given transport methods are enabled
        (reference stencil.hpp:150)"""
        return bool(self.methods & m)

    def get_origin(self, li: int) -> Vec:
        """global coordinate of local subdomain li's interior origin
        (reference stencil.hpp:162)"""
        return self.local_rect(li)[0]

    def get_topology(self):
        """neighbor topology over the partition grid
        (reference stencil.hpp:203)"""
        from .parallel.topology import Topology

        return Topology(self.placement.dim(), self.periodic)

    def get_placement(self):
        return self.placement

    def num_local(self) -> int:
        return self.placement.num_local(self.comm.rank)

    def get_compute_region(self):
        return ((0, 0, 0), self.size)

    def local_rect(self, li: int):
        idx = self.placement.get_idx(self.comm.rank, li)
        o = self.placement.subdomain_origin(idx)
        s = self.placement.subdomain_size(idx)
        return o, tuple(o[i] + s[i] for i in range(3))

    def get_interior(self) -> List[Tuple[Vec, Vec]]:
        """per local domain: the sub-box whose stencil never reads halo
        (reference src/stencil.cu:878-923)"""
        out = []
        r = self.radius
        shrink_lo = (
            max(r.dir(-1, y, z) for y in (-1, 0, 1) for z in (-1, 0, 1)),
            max(r.dir(x, -1, z) for x in (-1, 0, 1) for z in (-1, 0, 1)),
            max(r.dir(x, y, -1) for x in (-1, 0, 1) for y in (-1, 0, 1)),
        )
        shrink_hi = (
            max(r.dir(1, y, z) for y in (-1, 0, 1) for z in (-1, 0, 1)),
            max(r.dir(x, 1, z) for x in (-1, 0, 1) for z in (-1, 0, 1)),
            max(r.dir(x, y, 1) for x in (-1, 0, 1) for y in (-1, 0, 1)),
        )
        for li in range(self.num_local()):
            lo, hi = self.local_rect(li)
            ilo = tuple(min(lo[i] + shrink_lo[i], hi[i]) for i in range(3))
            ihi = tuple(max(hi[i] - shrink_hi[i], ilo[i]) for i in range(3))
            out.append((ilo, ihi))
        return out

    def get_exterior(self) -> List[List[Tuple[Vec, Vec]]]:
        """per local domain: non-overlapping slabs covering compute-region
        minus interior (reference's slide-faces-in decomposition,
        src/stencil.cu:927-977)"""
        out = []
        interiors = self.get_interior()
        for li in range(self.num_local()):
            lo, hi = self.local_rect(li)
            ilo, ihi = interiors[li]
            boxes = []
            clo, chi = list(lo), list(hi)
            for axis in range(3):  # +x,+y,+z
                if ihi[axis] != chi[axis]:
                    blo = list(clo)
                    blo[axis] = ihi[axis]
                    boxes.append((tuple(blo), tuple(chi)))
                    chi[axis] = ihi[axis]
            for axis in range(3):  # -x,-y,-z
                if ilo[axis] != clo[axis]:
                    bhi = list(chi)
                    bhi[axis] = ilo[axis]
                    boxes.append((tuple(clo), tuple(bhi)))
                    clo[axis] = ilo[axis]
            out.append(boxes)
        return out

    # ---- data access helpers (global-coordinate region of a quantity) ----
    def read_global(self, li: int, lo: Vec, hi: Vec, handle: DataHandle, from_next=False,
                    out: Optional[np.ndarray] = None) -> np.ndarray:
        """read a global-coordinate region of local domain li as numpy
        (z,y,x). Pass `out` (a contiguous array of the right shape/dtype)
        to reuse a buffer -- repeated checkpoint reads then skip the
        fresh-page faults of a new allocation (native backend only)."""
        idx = self.placement.get_idx(self.comm.rank, li)
        o = self.placement.subdomain_origin(idx)
        r = self.radius
        flo = (o[0] - r.x(-1), o[1] - r.y(-1), o[2] - r.z(-1))
        pos = tuple(lo[i] - flo[i] for i in range(3))
        ext = tuple(hi[i] - lo[i] for i in range(3))
        shape = (ext[2], ext[1], ext[0])
        if out is not None and self.backend_kind == "native":
            assert out.shape == shape and out.dtype == handle.dtype and out.flags["C_CONTIGUOUS"]
            self.backend.read_region(li, pos, ext, handle.index, from_next, out=out)
            return out
        raw = self.backend.read_region(li, pos, ext, handle.index, from_next)
        arr = np.frombuffer(raw, dtype=handle.dtype)
        return arr.reshape(*shape)

    def write_global(self, li: int, lo: Vec, arr: np.ndarray, handle: DataHandle, to_next=False):
        idx = self.placement.get_idx(self.comm.rank, li)
        o = self.placement.subdomain_origin(idx)
        r = self.radius
        flo = (o[0] - r.x(-1), o[1] - r.y(-1), o[2] - r.z(-1))
        pos = tuple(lo[i] - flo[i] for i in range(3))
        ext = (arr.shape[2], arr.shape[1], arr.shape[0])
        # native backend takes any contiguous buffer zero-copy; torch
        # backend wants bytes
        if self.backend_kind == "native":
            data = np.ascontiguousarray(arr)
        else:
            data = arr.tobytes()
        self.backend.write_region(li, data, pos, ext, handle.index, to_next)

    # ---- checkpoint/restore ----
    def save_checkpoint(self, path: str, compress: bool = False):
        """save every quantity's interior of every local domain (npz; one
        file per rank). Beyond the reference's capabilities (it only had
        ParaView text dumps). compress=False by default: zlib measured
        ~40 MB/s single-threaded (a 4.3 GB checkpoint took 115 s of pure
        compression, profiles/r2/r2_gpu14_io.log) while the device->host
        path runs at 5-55 GB/s."""
        rank = self.comm.rank
        arrays = {}
        for li in range(self.num_local()):
            lo, hi = self.local_rect(li)
            gid = self.placement.linearize(self.placement.get_idx(rank, li))
            for i in range(len(self._data)):
                h = self.data_handle(i)
                arrays[f"d{gid}_q{i}"] = self.read_global(li, lo, hi, h)
        save = np.savez_compressed if compress else np.savez
        save(f"{path}.rank{rank}.npz", **arrays)

    def load_checkpoint(self, path: str):
        """restore interiors saved by save_checkpoint (same partition and
        placement required)"""
        rank = self.comm.rank
        with np.load(f"{path}.rank{rank}.npz") as data:
            for li in range(self.num_local()):
                lo, hi = self.local_rect(li)
                gid = self.placement.linearize(self.placement.get_idx(rank, li))
                for i in range(len(self._data)):
                    h = self.data_handle(i)
                    self.write_global(li, lo, data[f"d{gid}_q{i}"], h)

    # ---- observability ----
    def _write_plan_files(self, plan):
        """plan_<rank>.txt + rank x rank byte matrix (reference
        src/stencil.cu:482-637 format preserved in spirit)"""
        rank = self.comm.rank
        es_total = sum(es for es, _ in self._data)
        with open(f"{self.output_prefix}plan_{rank}.txt", "w") as f:
            f.write(f"rank {rank} world {self.comm.world_size} dim {self.placement.dim()}\n")
            for t in plan.translates:
                b = t.ext[0] * t.ext[1] * t.ext[2] * es_total
                f.write(f"direct_kernel dir={t.dir} src_local={t.src_local} dst_local={t.dst_local} bytes={b}\n")
            for s in plan.sends:
                for m in s.messages:
                    f.write(
                        f"rccl_send dir={m.dir} dst_rank={s.peer_rank} src_gid={m.src_gid} dst_gid={m.dst_gid} bytes={m.volume() * es_total}\n"
                    )
            for rcv in plan.recvs:
                for m in rcv.messages:
                    f.write(
                        f"rccl_recv dir={m.dir} src_rank={rcv.peer_rank} src_gid={m.src_gid} dst_gid={m.dst_gid} bytes={m.volume() * es_total}\n"
                    )
            for line in self._boundary_lines:  # only with a non-periodic axis
                f.write(line + "\n")
        # rank-rank comm matrix (numpy loadtxt-able; rank 0 writes)
        row = [0] * self.comm.world_size
        for s in plan.sends:
            row[s.peer_rank] += sum(m.volume() * es_total for m in s.messages)
        rows = self.comm.allgather_object(row)
        if rank == 0:
            with open(f"{self.output_prefix}mat_npy_loadtxt.txt", "w") as f:
                for rrow in rows:
                    f.write(" ".join(str(v) for v in rrow) + "\n")

    def write_paraview(self, prefix: str, zero_nans: bool = False):
        """dump each local subdomain interior as CSV 'Z,Y,X,q0,q1,...'
        (reference src/stencil.cu:1188-1264)"""
        rank = self.comm.rank
        handles = [self.data_handle(i) for i in range(len(self._data))]
        for li in range(self.num_local()):
            lo, hi = self.local_rect(li)
            arrays = [self.read_global(li, lo, hi, h).astype(np.float64) for h in handles]
            if zero_nans:
                arrays = [np.nan_to_num(a, nan=0.0) for a in arrays]
            gid = self.placement.linearize(self.placement.get_idx(rank, li))
            # vectorized dump (the round-1 Python triple loop took minutes
            # on large domains): one savetxt over a coordinate+value table
            Z, Y, X = np.mgrid[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]]
            table = np.column_stack(
                [Z.ravel(), Y.ravel(), X.ravel()] + [a.ravel() for a in arrays]
            )
            with open(f"{prefix}{gid}.txt", "w") as f:
                f.write("Z,Y,X," + ",".join(h.name or f"q{h.index}" for h in handles) + "\n")
                np.savetxt(
                    f, table, delimiter=",",
                    fmt=["%d", "%d", "%d"] + ["%.17g"] * len(arrays),
                )
