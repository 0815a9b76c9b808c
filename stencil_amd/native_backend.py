"""Native (C++/HIP) backend: wraps stencil_amd._C LocalDomain/ExchangeEngine.

This is the production path on MI355X. Same-rank halos move by direct-write
translate kernels over xGMI; cross-rank halos are packed into contiguous
buffers exported via DLPack and sent with torch.distributed (RCCL) P2P.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

from . import _C
from .parallel.planning import (
    ExchangePlan,
    Message,
    pair_seq_tags,
    wire_layout,
    wire_layout_pairs,
)

Vec = Tuple[int, int, int]


def _vec3(t) -> "_C.Vec3":
    return _C.Vec3(int(t[0]), int(t[1]), int(t[2]))


def _rect3(lo, hi) -> "_C.Rect3":
    return _C.Rect3(_vec3(lo), _vec3(hi))


class NativeBackend:
    def __init__(self, domain_specs: List[Tuple[Vec, Vec, int]], data_defs: List[Tuple[int, str]],
                 radius: "_C.Radius", groups: Optional[List[List[int]]] = None):
        """domain_specs: (size, origin, cuda) per local domain.
        groups: quantity-index lists defining independent exchange groups
        (None = one group with every quantity); exchange(g) then moves
        only that group's quantities."""
        self.radius = radius
        self.data_defs = list(data_defs)
        self.groups = groups if groups is not None else [list(range(len(data_defs)))]
        if len(self.groups) > 4:
            raise ValueError("at most 4 exchange groups (engine launch-group encoding)")
        self.domains = []
        for size, origin, cuda in domain_specs:
            d = _C.LocalDomain(_vec3(size), _vec3(origin), int(cuda))
            d.set_radius(radius)
            for es, name in data_defs:
                d.add_data(int(es), name)
            d.realize()
            self.domains.append(d)
        self.engine = _C.ExchangeEngine(self.domains)
        if len({c for _, _, c in domain_specs}) > 1:
            self.engine.enable_peer_all()
        ng = len(self.groups)
        self._send_items = [[] for _ in range(ng)]  # per group: (buf_id, peer, tag)
        self._recv_items = [[] for _ in range(ng)]
        self._send_ops = [[] for _ in range(ng)]  # torch/cpu modes: (tensor, peer, tag)
        self._recv_ops = [[] for _ in range(ng)]
        self._has_wire = [False] * ng
        self._wire_mode = "none"  # none | nccl | torch | cpu
        self._wire = None  # _C.RcclWire (nccl mode)
        self._wire_dev = -1
        self._cpu_mirror = {}
        self._ipc_active = False
        self._colo_group = None
        self._colo_wire = None  # _C.RcclWire over colocated ranks (device barrier)
        self._ipc_error = None
        self._colo_parity = [0] * ng
        self._staged_local = [False] * ng
        self._staging_recv = {}
        self._has_boundary = [False] * ng
        self.boundary_bytes = 0  # bytes one full boundary fill writes
        self.boundary_lines: List[str] = []  # plan-file lines
        self._stencil_taps = {}  # id(Stencil) -> (Stencil, _C.StencilTaps): built once

    # ---- plan registration ----
    def register_plan(self, plan: ExchangePlan, ctx: Optional[dict] = None):
        """ctx (multi-rank): {'comm': Comm, 'placement': Placement,
        'ipc': bool} -- colocated cross-rank halos then move by direct-write
        IPC translate kernels over xGMI instead of packed RCCL transfers."""
        import os

        self._ipc_active = False
        self._colo_group = None
        self._colo_wire = None
        self._ipc_error = None
        self._colo_parity = [0] * len(self.groups)
        self._staging_recv = {}
        if ctx and ctx.get("ipc", True) and os.environ.get("STENCIL_AMD_IPC", "1") != "0":
            comm = ctx["comm"]
            colo = set(comm.colocated_ranks()) - {comm.rank}
            if colo:
                ipc_sends = [s for s in plan.sends if s.peer_rank in colo]
                ipc_recvs = [r for r in plan.recvs if r.peer_rank in colo]
                try:
                    self._setup_ipc(plan, ctx, ipc_sends, ipc_recvs)
                    plan = ExchangePlan(
                        translates=plan.translates,
                        sends=[s for s in plan.sends if s.peer_rank not in colo],
                        recvs=[r for r in plan.recvs if r.peer_rank not in colo],
                    )
                    self._ipc_active = True
                except Exception as e:  # pragma: no cover - fallback path
                    import traceback
                    import warnings

                    self._ipc_error = traceback.format_exc()
                    warnings.warn(f"HIP IPC transport unavailable ({e}); falling back to RCCL")
                    ipc_sends = []
        self._make_colo_groups(ctx)
        elem_sizes = [es for es, _ in self.data_defs]
        # STENCIL_AMD_STAGE_LOCAL: auto (default) stages thin-row
        # cross-DEVICE translates through a coalesced pack into a buffer
        # on the destination GPU + local unpack (a direct xGMI scatter of
        # 4-24 B rows is what the IPC staged path already avoids across
        # processes); all = stage every local translate (test hook,
        # exercises the path on one GPU); 0 = off.
        stage_mode = os.environ.get("STENCIL_AMD_STAGE_LOCAL", "auto")
        self._staged_local = [False] * len(self.groups)
        for g, qis in enumerate(self.groups):
            for t in plan.translates:
                src = self.domains[t.src_local]
                dst = self.domains[t.dst_local]
                d = _vec3(t.dir)
                nd = _vec3(tuple(-c for c in t.dir))
                src_pos = src.halo_pos(d, False)
                dst_pos = dst.halo_pos(nd, True)
                cross = src.gpu() != dst.gpu()
                if stage_mode == "all":
                    staged_qis = sorted(qis)
                elif stage_mode == "0" or not cross:
                    staged_qis = []
                else:
                    staged_qis = [
                        qi for qi in sorted(qis) if self._is_thin(t, elem_sizes[qi])
                    ]
                fat_qis = [qi for qi in sorted(qis) if qi not in staged_qis]
                if fat_qis:
                    self.engine.add_translate(
                        t.src_local, t.dst_local, src_pos, dst_pos, _vec3(t.ext), g, fat_qis
                    )
                if staged_qis:
                    m = Message(t.dir, 0, 0, t.ext)
                    total, chunks = wire_layout_pairs(
                        [(m, qi) for qi in staged_qis], elem_sizes
                    )
                    buf = self.engine.create_buffer(t.dst_local, total)
                    for _m, qi, off, nb in chunks:
                        self.engine.add_pack(
                            t.src_local, buf, off, src_pos, _vec3(t.ext), qi, group=3 * g
                        )
                        self.engine.add_unpack(
                            t.dst_local, buf, off, dst_pos, _vec3(t.ext), qi, group=3 * g
                        )
                    self._staged_local[g] = True

        seq = pair_seq_tags(plan)
        ng = len(self.groups)
        for g, qis in enumerate(self.groups):
            for item, is_send in [(s, True) for s in plan.sends] + [(r, False) for r in plan.recvs]:
                total, chunks = wire_layout(item.messages, elem_sizes, qis)
                buf = self.engine.create_buffer(item.local_id, total)
                dom = self.domains[item.local_id]
                for mi, qi, off, nbytes in chunks:
                    m = item.messages[mi]
                    if is_send:
                        pos = dom.halo_pos(_vec3(m.dir), False)
                        self.engine.add_pack(item.local_id, buf, off, pos, _vec3(m.ext), qi,
                                             group=3 * g)
                    else:
                        nd = _vec3(tuple(-c for c in m.dir))
                        pos = dom.halo_pos(nd, True)
                        self.engine.add_unpack(item.local_id, buf, off, pos, _vec3(m.ext), qi,
                                               group=3 * g)
                # per-rank-pair sequence index, group-disambiguated: both
                # sides compute the identical (small) tag for this buffer
                tag = seq[(item.peer_rank, item.src_gid, item.dst_gid)] * ng + g
                if is_send:
                    self._send_items[g].append((buf, item.peer_rank, tag))
                else:
                    self._recv_items[g].append((buf, item.peer_rank, tag))
            self._has_wire[g] = bool(self._send_items[g] or self._recv_items[g])
        self._register_boundary(ctx.get("boundary") if ctx else None)
        self.engine.finalize()
        if ctx is not None:
            self._setup_wire(ctx)
        elif any(self._has_wire):
            raise RuntimeError("cross-rank wire transfers need a comm context")

    def _register_boundary(self, spec):
        """physical boundaries: per exchange group, one fill job per
        (local domain, out-pointing halo region, quantity of the group),
        all executed by ONE boundary_fill launch per GPU per exchange
        (csrc/src/boundary.hip). Positions are allocation coordinates."""
        from .boundary import Boundary

        self._has_boundary = [False] * len(self.groups)
        self.boundary_bytes = 0
        self.boundary_lines = []
        if spec is None:
            return
        elem_sizes = [es for es, _ in self.data_defs]
        for g, qis in enumerate(self.groups):
            for li, dom in enumerate(self.domains):
                origin = dom.origin().tuple()
                full_lo = dom.full_region().lo.tuple()
                for d, out in spec.out_regions(self.radius, origin, dom.size().tuple()):
                    ext = dom.halo_extent(_vec3(d))
                    if ext.flatten() == 0:
                        continue
                    pos = dom.halo_pos(_vec3(d), True)
                    nbytes = 0
                    for qi in sorted(qis):
                        axes = []
                        value = b""
                        sign_width = 0
                        for a in range(3):
                            if not out[a]:
                                axes.append((Boundary.PERIODIC, 0, 0))
                                continue
                            side = 1 if d[a] > 0 else 0
                            # allocation coordinate of global cell 0, global extent
                            axes.append((spec.kind(qi, a, side), -full_lo[a], spec.size[a]))
                        for a in (2, 1, 0):  # the z, y, x walk stops at its first FIXED face
                            if not out[a]:
                                continue
                            side = 1 if d[a] > 0 else 0
                            k = spec.kind(qi, a, side)
                            if k == Boundary.FIXED and not value:
                                value = spec.value(qi, a, side).tobytes()
                            if k == Boundary.ANTIMIRROR:
                                sign_width = elem_sizes[qi]
                        nbytes += self.engine.add_boundary_fill(
                            li, qi, pos, ext, axes, value, sign_width, g
                        )
                    if nbytes:
                        self._has_boundary[g] = True
                    self.boundary_bytes += nbytes
                    self.boundary_lines.append(
                        f"boundary_fill dir={d} local={li} group={g} bytes={nbytes}"
                    )

    def _setup_wire(self, ctx):
        """choose the cross-rank wire transport, identically on every rank
        (the vote is allgathered; a mixed choice would deadlock):

        - 'nccl' (production default on GPUs): native RcclWire
          (csrc/src/wire.hip) -- grouped ncclSend/ncclRecv posted on the
          engine's per-device pack stream, so pack -> wire -> unpack is
          entirely stream-ordered with ONE host sync per exchange (the
          round-1 path host-blocked between each phase)
          and libtorch is out of the hot path.
        - 'torch': torch.distributed batch_isend_irecv on the same device
          buffers (the round-1 implementation; retained as the test
          oracle, forced with STENCIL_AMD_WIRE=torch).
        - 'cpu': pinned host mirrors over gloo (CPU-only boxes/tests;
          forced with STENCIL_AMD_WIRE=cpu)."""
        import os

        comm = ctx["comm"]
        if comm.world_size == 1:
            self._wire_mode = "none"  # no cross-rank traffic possible
            return
        env = os.environ.get("STENCIL_AMD_WIRE", "")
        want = "cpu" if (env == "cpu" or self._detect_cpu_wire()) else (
            "torch" if env == "torch" else "nccl"
        )
        # the native wire drives ONE device; multi-device ranks fall back
        devs = {
            self.engine.buffer_device(b)
            for g in range(len(self.groups))
            for b, _, _ in self._send_items[g] + self._recv_items[g]
        }
        if want == "nccl" and len(devs) > 1:
            want = "torch"
        my_dev = next(iter(devs)) if devs else (
            self.domains[0].gpu() if self.domains else -1
        )
        votes = comm.allgather_object(
            (want, any(self._has_wire), comm.hostname, my_dev)
        )
        if not any(w for _, w, _, _ in votes):
            self._wire_mode = "none"
            return
        modes = {m for m, _, _, _ in votes}
        mode = "cpu" if "cpu" in modes else ("torch" if "torch" in modes else "nccl")
        # NCCL (native or torch) refuses two ranks on one GPU: demote to
        # the host-staged wire when colocated ranks share a device (the
        # time-shared simulation shape; real nodes give each rank its own
        # GPU and keep the fast path)
        if mode in ("nccl", "torch"):
            seen = set()
            for _, _, host, dev in votes:
                if (host, dev) in seen:
                    mode = "cpu"
                    break
                seen.add((host, dev))
        self._wire_mode = mode
        if mode == "nccl":
            self._wire_dev = next(iter(devs)) if devs else (
                self.domains[0].gpu() if self.domains else 0
            )
            # the unique id travels over the gloo control plane, setup only
            uid = _C.RcclWire.unique_id() if comm.rank == 0 else None
            uid = comm.allgather_object(uid)[0]
            self._wire = _C.RcclWire(self._wire_dev, comm.rank, comm.world_size, uid)
            for g in range(len(self.groups)):
                for b, peer, tag in self._send_items[g]:
                    self._wire.add_send(g, self.engine.buffer_ptr(b),
                                        self.engine.buffer_bytes(b), peer, tag)
                for b, peer, tag in self._recv_items[g]:
                    self._wire.add_recv(g, self.engine.buffer_ptr(b),
                                        self.engine.buffer_bytes(b), peer, tag)
            self._wire.finalize()
            return
        import torch

        for g in range(len(self.groups)):
            for items, ops in ((self._send_items[g], self._send_ops[g]),
                               (self._recv_items[g], self._recv_ops[g])):
                for b, peer, tag in items:
                    t = torch.from_dlpack(self.engine.buffer_dlpack(b))
                    ops.append((t, peer, tag))
                    if mode == "cpu":
                        self._cpu_mirror[id(t)] = torch.empty(
                            t.shape, dtype=torch.uint8, device="cpu",
                            pin_memory=torch.cuda.is_available(),
                        )

    @staticmethod
    def _is_thin(m, elem_size: int) -> bool:
        """thin-row (message, quantity) chunks (x-faces/edges) written
        directly into remote memory scatter <64 B rows over xGMI; they go
        through the staged path instead (coalesced pack into the
        receiver's staging buffer + local unpack). Per-quantity: an
        8-cell fp64 row (64 B) is fat while the same row at fp32 (32 B)
        is thin."""
        return m.ext[0] * elem_size < 64

    def _thin_pairs(self, messages, qis):
        """deterministic (message, qi) enumeration of a transfer's thin
        chunks -- identical on sender and receiver, so it defines the
        staged buffer's wire layout"""
        es = [e for e, _ in self.data_defs]
        return [(m, qi) for m in messages for qi in sorted(qis) if self._is_thin(m, es[qi])]

    def _setup_ipc(self, plan: ExchangePlan, ctx: dict, ipc_sends, ipc_recvs):
        """exchange hipIpc handles among colocated ranks and register
        direct-write translate jobs into the peer processes' buffers
        (the reference's ColoHaloSender direct-access idea,
        src/tx_colocated.cu, re-done with xGMI stores + a gloo barrier
        instead of IPC events). Thin messages are double-buffered staged
        (see _is_thin)."""
        comm, placement = ctx["comm"], ctx["placement"]
        radius = self.radius
        elem_sizes = [es for es, _ in self.data_defs]
        # phase 1: export handles. A failing rank must still reach the
        # allgather (its peers would otherwise hang), so errors are
        # exported as data and re-raised on EVERY rank afterwards.
        try:
            export = []
            for d in self.domains:
                nq = d.num_data()
                export.append(
                    {
                        "gpu": d.gpu(),
                        "pitch": [d.curr_pitch(qi) for qi in range(nq)],
                        "ysize": [d.curr_ysize(qi) for qi in range(nq)],
                        "es": [d.elem_size(qi) for qi in range(nq)],
                        "pad": [d.pad_bytes(qi) for qi in range(nq)],
                        "curr": [d.ipc_handle(qi, False) for qi in range(nq)],
                        "next": [d.ipc_handle(qi, True) for qi in range(nq)],
                    }
                )
            # receiver side of the staged path: per exchange group, a
            # double-buffered staging buffer per incoming (src,dst) pair's
            # thin messages, with parity unpack jobs in groups 3g+1/3g+2
            staging = {}
            for g, qis in enumerate(self.groups):
                for r in ipc_recvs:
                    pairs = self._thin_pairs(r.messages, qis)
                    if not pairs:
                        continue
                    total, chunks = wire_layout_pairs(pairs, elem_sizes)
                    buf = self.engine.create_buffer(r.local_id, 2 * total)
                    dom = self.domains[r.local_id]
                    for m, qi, off, nbytes in chunks:
                        nd = _vec3(tuple(-c for c in m.dir))
                        pos = dom.halo_pos(nd, True)
                        for parity in (0, 1):
                            self.engine.add_unpack(
                                r.local_id, buf, off + parity * total, pos, _vec3(m.ext), qi,
                                group=3 * g + 1 + parity,
                            )
                    staging[(r.src_gid, r.dst_gid, g)] = (
                        self.engine.buffer_ipc_handle(buf),
                        total,
                    )
                    self._staging_recv[(r.src_gid, r.dst_gid, g)] = (buf, total)
            export = {"domains": export, "staging": staging}
        except Exception as e:
            export = {"error": str(e)}
        infos = comm.allgather_object(export)
        errs = [i["error"] for i in infos if "error" in i]
        if errs:
            raise RuntimeError(f"IPC export failed on some rank: {errs[0]}")

        # phase 2: open every view first (a failure here leaves no
        # translate specs registered, keeping the RCCL fallback clean),
        # then register the direct-write jobs.
        views = {}
        remote_staging = {}
        open_err = None
        all_q = sorted({q for qs in self.groups for q in qs})
        try:
            for s in ipc_sends:
                dst_idx = placement.dimensionize(s.dst_gid)
                dst_li = placement.get_subdomain_id(dst_idx)
                src_gpu = self.domains[s.local_id].gpu()
                key = (s.peer_rank, dst_li, src_gpu)
                any_fat = any(
                    not self._is_thin(m, elem_sizes[qi]) for m in s.messages for qi in all_q
                )
                if key not in views and any_fat:
                    info = infos[s.peer_rank]["domains"][dst_li]
                    views[key] = self.engine.create_remote_view(
                        src_gpu, info["curr"], info["next"], info["pitch"], info["ysize"],
                        info["es"], info["pad"]
                    )
                for g in range(len(self.groups)):
                    skey = (s.src_gid, s.dst_gid, g)
                    stg = infos[s.peer_rank]["staging"].get(skey)
                    if stg is not None and skey not in remote_staging:
                        handle, total = stg
                        rb = self.engine.open_remote_buffer(src_gpu, handle, 2 * total)
                        remote_staging[skey] = (rb, total)
        except Exception as e:
            open_err = str(e)
        # consensus: either EVERY rank uses IPC or none does (a mixed state
        # would deadlock: IPC ranks at the barrier, RCCL ranks at a recv)
        votes = comm.allgather_object(open_err)
        bad = [v for v in votes if v is not None]
        if bad:
            raise RuntimeError(f"IPC open failed on some rank: {bad[0]}")
        for g, qis in enumerate(self.groups):
            for s in ipc_sends:
                dst_idx = placement.dimensionize(s.dst_gid)
                dst_li = placement.get_subdomain_id(dst_idx)
                dst_size = placement.subdomain_size(dst_idx)
                src_gpu = self.domains[s.local_id].gpu()
                key = (s.peer_rank, dst_li, src_gpu)
                dom = self.domains[s.local_id]
                for m in s.messages:
                    fat_qis = [
                        qi for qi in sorted(qis) if not self._is_thin(m, elem_sizes[qi])
                    ]
                    if not fat_qis:
                        continue
                    nd = _vec3(tuple(-c for c in m.dir))
                    src_pos = dom.halo_pos(_vec3(m.dir), False)
                    dst_pos = _C.halo_pos(nd, _vec3(dst_size), radius, True)
                    self.engine.add_translate_view(
                        s.local_id, views[key], src_pos, dst_pos, _vec3(m.ext), g, fat_qis
                    )
                thin = self._thin_pairs(s.messages, qis)
                if thin:
                    rb, total = remote_staging[(s.src_gid, s.dst_gid, g)]
                    _t2, chunks = wire_layout_pairs(thin, elem_sizes)
                    assert _t2 == total, "staged wire layout mismatch"
                    for m, qi, off, nbytes in chunks:
                        pos = dom.halo_pos(_vec3(m.dir), False)
                        for parity in (0, 1):
                            self.engine.add_pack(
                                s.local_id, rb, off + parity * total, pos, _vec3(m.ext), qi,
                                group=3 * g + 1 + parity,
                            )

    def _make_colo_groups(self, ctx):
        """per-node barrier machinery for the post-translate IPC path.
        new_group is collective: every rank creates every node's group.

        Two barrier flavors: a gloo host barrier (always created; the
        fallback and the only option when ranks share a device — RCCL
        refuses communicators with two ranks on one GPU), and a native
        device barrier: a 1-float all-reduce on a colocated-ranks
        RcclWire communicator (csrc/src/wire.hip), posted on the engine's
        pack stream so the staged unpacks can be stream-ordered behind it
        with no extra host block. A host gloo barrier costs O(100us..ms)
        per exchange at world 8, which is material against a ~1.3 ms
        jacobi step; the RCCL barrier tracks stream completion at
        collective cost (~20-30us). STENCIL_AMD_BARRIER=gloo forces the
        host barrier; the decision is allgathered so it is identical on
        every rank (a mixed choice would deadlock)."""
        if not self._ipc_active or ctx is None:
            return
        import os

        import torch.distributed as dist

        comm = ctx["comm"]
        nodes = comm.node_of_rank()
        by_node = {}
        for r, node in enumerate(nodes):
            by_node.setdefault(node, []).append(r)
        my_dev = self.domains[0].gpu() if self.domains else -1
        want_dev = (
            os.environ.get("STENCIL_AMD_BARRIER", "auto") != "gloo"
            and _C.device_count() > 0
            and my_dev >= 0
        )
        infos = comm.allgather_object((nodes[comm.rank], my_dev, bool(want_dev)))
        use_dev = all(i[2] for i in infos)
        if use_dev:
            for node, ranks in by_node.items():
                devs = [infos[r][1] for r in ranks]
                if len(set(devs)) != len(devs):
                    use_dev = False  # shared device somewhere -> gloo everywhere
        for node in sorted(by_node):
            g = dist.new_group(ranks=by_node[node], backend="gloo")
            if comm.rank in by_node[node]:
                self._colo_group = g
        self._colo_wire = None
        if use_dev:
            # one sub-communicator per node; each node leader mints the
            # unique id, exchanged over the gloo control plane (setup only)
            my_ranks = by_node[nodes[comm.rank]]
            uid = _C.RcclWire.unique_id() if comm.rank == my_ranks[0] else None
            uids = comm.allgather_object(uid)
            self._colo_wire = _C.RcclWire(
                my_dev, my_ranks.index(comm.rank), len(my_ranks), uids[my_ranks[0]]
            )

    def _colo_barrier(self):
        """ensure every colocated rank has passed its translate sync
        (their xGMI writes into our buffers are complete). Native flavor:
        the all-reduce is ENQUEUED on the pack stream — callers that only
        enqueue more pack-stream work after it need no host block here."""
        if self._colo_wire is not None:
            self._colo_wire.barrier(self.engine.pack_stream_handle(self._colo_wire.device()))
        else:
            import torch.distributed as dist

            dist.barrier(group=self._colo_group)

    @staticmethod
    def _detect_cpu_wire() -> bool:
        """True when the process group cannot carry CUDA tensors (plain gloo):
        pack buffers are then staged through pinned host mirrors. RCCL (nccl)
        carries the device buffers directly over xGMI."""
        import os

        if os.environ.get("STENCIL_AMD_WIRE", "") == "cpu":
            return True
        import torch.distributed as dist

        backend = str(dist.get_backend())
        return "nccl" not in backend

    # ---- per-iteration ----
    def exchange_begin(self, group: int = 0):
        """stream-ordered first half for one exchange group: launch all
        local/IPC translates and (if cross-rank) the pack kernels. Returns
        immediately; GPU work overlaps the app's compute streams."""
        g = group
        self.engine.launch_translates(g)
        if self._ipc_active:
            # staged thin messages: coalesced pack straight into the
            # receiver's staging buffer (parity-selected half)
            self.engine.launch_packs(3 * g + 1 + self._colo_parity[g])
        if self._has_wire[g] or self._staged_local[g]:
            self.engine.launch_packs(3 * g)

    def exchange_end(self, group: int = 0):
        """second half: move wire buffers, unpack, and block until the
        group's halos are in place."""
        g = group
        if self._has_wire[g]:
            if self._wire_mode == "nccl":
                # fully stream-ordered: the packs already sit on the pack
                # stream (exchange_begin), the grouped send/recv is posted
                # behind them, and the unpacks are enqueued behind the
                # recvs -- the only host block is sync_all below. Staged-
                # local cross-device unpacks need the event fence (their
                # packs ran on another device's stream).
                self._wire.post(g, self.engine.pack_stream_handle(self._wire_dev))
                if self._staged_local[g]:
                    self.engine.fence_packs_unpacks(3 * g)
                self.engine.launch_unpacks(3 * g)
            else:
                import torch.distributed as dist

                self.engine.sync_packs()
                if self._wire_mode == "cpu":
                    ops = []
                    for t, peer, tag in self._send_ops[g]:
                        m = self._cpu_mirror[id(t)]
                        m.copy_(t)
                        ops.append(dist.P2POp(dist.isend, m, peer, tag=tag))
                    for t, peer, tag in self._recv_ops[g]:
                        ops.append(dist.P2POp(dist.irecv, self._cpu_mirror[id(t)], peer, tag=tag))
                    for w in dist.batch_isend_irecv(ops):
                        w.wait()
                    for t, _, _ in self._recv_ops[g]:
                        t.copy_(self._cpu_mirror[id(t)])
                else:
                    ops = [
                        dist.P2POp(dist.isend, t, peer, tag=tag)
                        for t, peer, tag in self._send_ops[g]
                    ]
                    ops += [
                        dist.P2POp(dist.irecv, t, peer, tag=tag)
                        for t, peer, tag in self._recv_ops[g]
                    ]
                    for w in dist.batch_isend_irecv(ops):
                        w.wait()
                self.engine.launch_unpacks(3 * g)
        elif self._staged_local[g]:
            # pack (src device) -> buffer on dst device -> unpack (dst
            # device): cross-device ordering via the event fence, one
            # host sync below
            self.engine.fence_packs_unpacks(3 * g)
            self.engine.launch_unpacks(3 * g)
        if self._has_boundary[g] and not self._ipc_active:
            # physical boundaries: the fill reads halos this exchange
            # delivers, so it is event-ordered behind every translate of
            # the group and stream-ordered behind the unpacks just
            # enqueued on the pack stream; sync_all below covers it
            self.engine.launch_boundary(g)
        self.engine.sync_all()
        if self._ipc_active:
            # all colocated ranks' direct writes and staged packs are
            # complete after the barrier (each rank synced its own streams
            # above); then unpack this exchange's staging parity locally.
            # The barrier also keeps senders at most one exchange (of this
            # group) ahead, which makes two staging parities sufficient.
            # With the native device barrier the staged unpacks are stream-
            # ordered behind the barrier all-reduce on the pack stream, so
            # the host blocks once (sync_packs), not twice.
            self._colo_barrier()
            self.engine.launch_unpacks(3 * g + 1 + self._colo_parity[g])
            if self._has_boundary[g]:
                # IPC peers write our halos too: fill only behind the
                # colocated barrier and the staged unpacks (pack stream)
                self.engine.launch_boundary(g)
            self.engine.sync_packs()
            self._colo_parity[g] ^= 1

    def exchange(self, group: int = 0):
        self.exchange_begin(group)
        self.exchange_end(group)

    def swap(self):
        for d in self.domains:
            d.swap()
        if self._ipc_active:
            self.engine.flip_views()

    def sync(self):
        self.engine.sync_all()
        self.engine.sync_compute()

    # ---- app/test helpers (positions in allocation coords) ----
    def read_region(self, li: int, pos: Vec, ext: Vec, qi: int, from_next=False, out=None):
        if out is not None:  # reuse caller's buffer: no fresh-page faults
            self.domains[li].region_to_host_into(out, _vec3(pos), _vec3(ext), qi, from_next)
            return out
        return self.domains[li].region_to_host(_vec3(pos), _vec3(ext), qi, from_next)

    def write_region(self, li: int, data: bytes, pos: Vec, ext: Vec, qi: int, to_next=False):
        self.domains[li].region_from_host(data, _vec3(pos), _vec3(ext), qi, to_next)

    def fill_f32(self, li: int, qi: int, region_lo: Vec, region_hi: Vec, value: float, next_buf: bool):
        """ValueError (nothing launched) for a region outside the allocation"""
        _C.fill_f32(self.engine, li, qi, _rect3(region_lo, region_hi), value, next_buf)

    def jacobi_step(self, li: int, qi: int, region_lo: Vec, region_hi: Vec,
                    c_lo: Vec, c_hi: Vec, stream_id: int = 0, extend_vec: int = 0):
        """one Jacobi step over the global box; extend_vec 0/1/2 as in
        ops.hpp. ValueError (nothing launched) when the box plus its 1-cell
        apron leaves the allocation."""
        _C.jacobi_step(self.engine, li, qi, _rect3(region_lo, region_hi), _rect3(c_lo, c_hi),
                       stream_id, extend_vec)

    def stencil_apply(self, li: int, src_qi: int, dst_qi: int, lo: Vec, hi: Vec, stencil,
                      dtype, stream_id: int = 0):
        """next[dst_qi] = stencil(curr[src_qi]) over the global box [lo, hi)
        (csrc/src/stencil_op.hip); dtype is float32 or float64. Raises
        ValueError on a dtype/element-size mismatch or a tap that reads
        outside the allocation; nothing is launched then."""
        import numpy as np

        dt = np.dtype(dtype)
        if dt == np.float32:
            ty = _C.StencilType.F32
        elif dt == np.float64:
            ty = _C.StencilType.F64
        else:
            raise ValueError(f"stencil_apply supports float32/float64, got {dt}")
        taps = self._stencil_taps.get(id(stencil))
        if taps is None or taps[0] is not stencil:
            taps = (stencil, stencil.to_native())
            self._stencil_taps[id(stencil)] = taps
        _C.stencil_apply(self.engine, li, src_qi, dst_qi, _rect3(lo, hi), taps[1], ty, stream_id)

    # ---- vector operations (csrc/src/vector_ops.hip) ----
    # `boxes` holds one global box (lo, hi) per local domain; an operand is
    # (quantity index, next_buf). The reductions return one fp64 sum (or one
    # tuple of sums) per local domain: every domain's kernel is launched
    # before the first wait, so a reduction costs one host sync per domain.
    def _each_box(self, boxes, stream_id: int, op, *args):
        """op(engine, li, *args, rect, stream_id), the shape of every _C
        vector op, on every local domain's box in li order"""
        for li, (lo, hi) in enumerate(boxes):
            op(self.engine, li, *args, _rect3(lo, hi), stream_id)

    def _reduce_n(self, boxes, stream_id: int, n_values: int, begin, *args) -> List[tuple]:
        """begin(engine, li, *args, rect, stream_id), a *_begin op, on every
        local domain, then reduction_end_n on each begun one (also when a
        begin raised): one tuple of n_values fp64 sums per local domain"""
        n = 0
        try:
            for li, (lo, hi) in enumerate(boxes):
                begin(self.engine, li, *args, _rect3(lo, hi), stream_id)
                n += 1
        finally:
            out = [_C.reduction_end_n(self.engine, li, n_values) for li in range(n)]
        return out

    def _reduce_1(self, boxes, stream_id: int, begin, *args) -> List[float]:
        return [v[0] for v in self._reduce_n(boxes, stream_id, 1, begin, *args)]

    def field_dot(self, boxes, a: int, a_next: bool, b: int, b_next: bool,
                  stream_id: int = 0) -> List[float]:
        """per local domain: sum of a * b over its box, products and sums
        in fp64, deterministic. ValueError (nothing launched) on an unknown
        quantity, a non-float32/float64 or mixed element size, or a box
        outside the allocation."""
        return self._reduce_1(boxes, stream_id, _C.field_dot_begin, a, a_next, b, b_next)

    def field_axpby(self, boxes, alpha: float, x: int, x_next: bool, beta: float, y: int,
                    y_next: bool, out: int, out_next: bool, stream_id: int = 0):
        """out = alpha * x + beta * y over each local domain's box, in the
        quantity's type; out may alias x or y. Enqueued, not awaited."""
        self._each_box(boxes, stream_id, _C.field_axpby, alpha, x, x_next, beta, y, y_next, out,
                       out_next)

    def field_axpbypcz(self, boxes, alpha: float, x: int, x_next: bool, beta: float, y: int,
                       y_next: bool, gamma: float, z: int, z_next: bool, out: int,
                       out_next: bool, stream_id: int = 0):
        """out = alpha * x + beta * y + gamma * z over each local domain's
        box; out may alias any input. Enqueued, not awaited."""
        self._each_box(boxes, stream_id, _C.field_axpbypcz, alpha, x, x_next, beta, y, y_next,
                       gamma, z, z_next, out, out_next)

    def field_scaled_update(self, boxes, alpha: float, x: int, x_next: bool, d: int, d_next: bool,
                            beta: float, y: int, y_next: bool, gamma: float, z: int,
                            z_next: bool, out: int, out_next: bool, stream_id: int = 0):
        """out = alpha * x + d * (beta * y + gamma * z) over each local
        domain's box, d a quantity; out may alias any input. Enqueued, not
        awaited."""
        self._each_box(boxes, stream_id, _C.field_scaled_update, alpha, x, x_next, d, d_next, beta,
                       y, y_next, gamma, z, z_next, out, out_next)

    # ---- variable-coefficient diffusion (csrc/src/diffusion_op.hip) ----
    @staticmethod
    def _stencil_type(op: str, dtype):
        import numpy as np

        dt = np.dtype(dtype)
        if dt == np.float32:
            return _C.StencilType.F32
        if dt == np.float64:
            return _C.StencilType.F64
        raise ValueError(f"{op} supports float32/float64, got {dt}")

    def diffusion_apply(self, li: int, src_qi: int, k_qi: int, dst_qi: int, lo: Vec, hi: Vec,
                        h, sigma: float, dtype, stream_id: int = 0):
        """next[dst_qi] = (sigma I - div(k grad)) curr[src_qi] over the
        global box [lo, hi), k = curr[k_qi], h[a] = 1 / spacing_a^2. Raises
        ValueError, launching nothing, as diffusion_apply in ops.hpp."""
        _C.diffusion_apply(self.engine, li, src_qi, k_qi, dst_qi, _rect3(lo, hi),
                           [float(v) for v in h], float(sigma),
                           self._stencil_type("diffusion_apply", dtype), stream_id)

    def diffusion_inv_diagonal(self, li: int, k_qi: int, out_qi: int, out_next: bool, lo: Vec,
                               hi: Vec, h, sigma: float, omega: float, stream_id: int = 0):
        """out = omega / diag of the diffusion operator over the global box"""
        _C.diffusion_inv_diagonal(self.engine, li, k_qi, out_qi, out_next, _rect3(lo, hi),
                                  [float(v) for v in h], float(sigma), float(omega), stream_id)

    # ---- grid transfer (csrc/src/grid_transfer.hip) ----
    # self is the DESTINATION backend: its compute stream carries the kernel.
    # Boxes are coarse global boxes; the caller has synced the source side.
    def grid_restrict(self, fine: "NativeBackend", fli: int, alpha: float, a: int, a_next: bool,
                      beta: float, b: int, b_next: bool, cli: int, out: int, out_next: bool,
                      lo: Vec, hi: Vec, stream_id: int = 0):
        """coarse out(c) = mean over the 8 children of alpha a + beta b, for
        the coarse cells c of [lo, hi) of this backend's local domain cli;
        a and b live in local domain fli of `fine`"""
        _C.grid_restrict(fine.engine, fli, alpha, a, a_next, beta, b, b_next, self.engine, cli,
                         out, out_next, _rect3(lo, hi), stream_id)

    def grid_prolong_add(self, coarse: "NativeBackend", cli: int, src: int, src_next: bool,
                         fli: int, dst: int, dst_next: bool, lo: Vec, hi: Vec,
                         stream_id: int = 0):
        """fine dst(p) += src(p >> 1) for the fine cells of [2 lo, 2 hi) of
        this backend's local domain fli; src lives in local domain cli of
        `coarse`"""
        _C.grid_prolong_add(coarse.engine, cli, src, src_next, self.engine, fli, dst, dst_next,
                            _rect3(lo, hi), stream_id)

    def device_of(self, li: int) -> int:
        return self.domains[li].gpu()

    def cg_update(self, boxes, alpha: float, x: int, p: int, r: int,
                  stream_id: int = 0) -> List[float]:
        """fused CG update per local domain: curr[x] += alpha * curr[p];
        curr[r] -= alpha * next[p]; returns each domain's sum of r_new^2"""
        return self._reduce_1(boxes, stream_id, _C.cg_update_begin, alpha, x, p, r)

    # ---- the reductions of singular problems: several values per pass ----
    def field_sum(self, boxes, a: int, a_next: bool, stream_id: int = 0) -> List[float]:
        """per local domain: sum of a over its box in fp64, deterministic;
        the ValueErrors of field_dot"""
        return self._reduce_1(boxes, stream_id, _C.field_sum_begin, a, a_next)

    def field_dot_sums(self, boxes, a: int, a_next: bool, b: int, b_next: bool,
                       stream_id: int = 0) -> List[tuple]:
        """per local domain: (sum a * b, sum a, sum b) over its box from one
        pass, in fp64, deterministic; a and b may be the same buffer"""
        return self._reduce_n(boxes, stream_id, 3, _C.field_dot_sums_begin, a, a_next, b, b_next)

    def cg_update_sum(self, boxes, alpha: float, x: int, p: int, r: int,
                      stream_id: int = 0) -> List[tuple]:
        """cg_update per local domain, returning (sum r_new^2, sum r_new)"""
        return self._reduce_n(boxes, stream_id, 2, _C.cg_update_sum_begin, alpha, x, p, r)

    def field_axpbyc(self, boxes, alpha: float, x: int, x_next: bool, beta: float, y: int,
                     y_next: bool, c: float, out: int, out_next: bool, stream_id: int = 0):
        """out = alpha * x + beta * y + c over each local domain's box, in
        the quantity's type; out may alias x or y. Enqueued, not awaited."""
        self._each_box(boxes, stream_id, _C.field_axpbyc, alpha, x, x_next, beta, y, y_next, c,
                       out, out_next)

    # ---- the fused passes of BiCGStab ----
    def field_axpby_norm2(self, boxes, alpha: float, x: int, x_next: bool, beta: float, y: int,
                          y_next: bool, out: int, out_next: bool,
                          stream_id: int = 0) -> List[float]:
        """field_axpby per local domain, returning each domain's sum of
        out^2 from the same pass"""
        return self._reduce_1(boxes, stream_id, _C.field_axpby_norm2_begin, alpha, x, x_next,
                              beta, y, y_next, out, out_next)

    def field_dot_pair(self, boxes, a: int, a_next: bool, b: int, b_next: bool,
                       stream_id: int = 0) -> List[tuple]:
        """per local domain: (sum a * b, sum a * a) over its box from one pass"""
        return self._reduce_n(boxes, stream_id, 2, _C.field_dot_pair_begin, a, a_next, b, b_next)

    def bicgstab_update(self, boxes, alpha: float, y: int, y_next: bool, omega: float, z: int,
                        z_next: bool, x: int, r: int, t: int, t_next: bool, rhat: int,
                        rhat_next: bool, stream_id: int = 0) -> List[tuple]:
        """fused BiCGStab update per local domain: curr[x] += alpha * y +
        omega * z; curr[r] -= omega * t; returns each domain's
        (sum r_new^2, sum rhat * r_new)"""
        return self._reduce_n(boxes, stream_id, 2, _C.bicgstab_update_begin, alpha, y, y_next,
                              omega, z, z_next, x, r, t, t_next, rhat, rhat_next)

    def jacobi_graph_create(self, li: int, qi: int, region_lo: Vec, region_hi: Vec,
                            c_lo: Vec, c_hi: Vec) -> "_C.JacobiStepGraph":
        """whole-step replay graph (single-process single-domain path);
        see csrc/src/jacobi.hip jacobi_graph_create. The returned object
        owns the graph and keeps the engine alive; dropping it frees it."""
        return _C.jacobi_graph_create(self.engine, li, qi, _rect3(region_lo, region_hi),
                                      _rect3(c_lo, c_hi))

    def jacobi_graph_step(self, graph: "_C.JacobiStepGraph", n: int = 1):
        _C.jacobi_graph_launch(graph, n)
        _C.jacobi_graph_sync(graph)

    def sync_compute(self):
        self.engine.sync_compute()
