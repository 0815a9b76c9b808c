"""Torch reference backend.

A plain-PyTorch implementation of the same exchange plan, used as
1) the fp32/fp64 numerics reference that every HIP kernel is tested
   against, and 2) the CPU path for multi-process (gloo) tests of the
   distributed planning/transport logic on machines without GPUs.
Not a performance path.
"""
from __future__ import annotations

from typing import Tuple

import torch

from . import _C
from .parallel.planning import ExchangePlan, pair_seq_tags, wire_layout

Vec = Tuple[int, int, int]

_DTYPES = {1: torch.uint8, 2: torch.int16, 4: torch.float32, 8: torch.float64}


def _vec3(t):
    return _C.Vec3(int(t[0]), int(t[1]), int(t[2]))


class _TorchDomain:
    """tensor-backed LocalDomain mirror (geometry via the native statics)"""

    def __init__(self, size: Vec, origin: Vec, device: str, data_defs, radius):
        self.size = tuple(size)
        self.origin = tuple(origin)
        self.device = device
        self.radius = radius
        self.elem_sizes = [es for es, _ in data_defs]
        raw = self.raw_size()
        self.curr = []
        self.next = []
        for es, _name in data_defs:
            if es not in _DTYPES:
                raise ValueError(f"torch backend supports elem sizes {list(_DTYPES)}, got {es}")
            shape = (raw[2], raw[1], raw[0])  # (z, y, x)
            self.curr.append(torch.zeros(shape, dtype=_DTYPES[es], device=device))
            self.next.append(torch.zeros(shape, dtype=_DTYPES[es], device=device))

    def raw_size(self) -> Vec:
        r = self.radius
        return (
            self.size[0] + r.x(-1) + r.x(1),
            self.size[1] + r.y(-1) + r.y(1),
            self.size[2] + r.z(-1) + r.z(1),
        )

    def halo_pos(self, d: Vec, halo: bool) -> Vec:
        return _C.halo_pos(_vec3(d), _vec3(self.size), self.radius, halo).tuple()

    def halo_extent(self, d: Vec) -> Vec:
        return _C.halo_extent(_vec3(d), _vec3(self.size), self.radius).tuple()

    def full_lo(self) -> Vec:
        r = self.radius
        return (self.origin[0] - r.x(-1), self.origin[1] - r.y(-1), self.origin[2] - r.z(-1))

    @staticmethod
    def _sl(pos: Vec, ext: Vec):
        return (
            slice(pos[2], pos[2] + ext[2]),
            slice(pos[1], pos[1] + ext[1]),
            slice(pos[0], pos[0] + ext[0]),
        )

    def region(self, qi: int, pos: Vec, ext: Vec, from_next=False) -> torch.Tensor:
        t = (self.next if from_next else self.curr)[qi]
        return t[self._sl(pos, ext)]


class TorchBackend:
    def __init__(self, domain_specs, data_defs, radius, device: str = "cpu", groups=None):
        self.radius = radius
        self.data_defs = list(data_defs)
        self.groups = groups if groups is not None else [list(range(len(data_defs)))]
        if device.startswith("cuda") and len({c for _, _, c in domain_specs}) > 1:
            # one tensor device per local domain
            self.domains = [
                _TorchDomain(s, o, f"cuda:{c}", data_defs, radius) for s, o, c in domain_specs
            ]
        else:
            self.domains = [
                _TorchDomain(s, o, device, data_defs, radius) for s, o, c in domain_specs
            ]
        ng = len(self.groups)
        self._translates = [[] for _ in range(ng)]
        self._send_bufs = [[] for _ in range(ng)]  # per group
        self._recv_bufs = [[] for _ in range(ng)]
        self._boundary = None
        self.boundary_bytes = 0
        self.boundary_lines = []

    def register_plan(self, plan: ExchangePlan, ctx=None):
        self._boundary = ctx.get("boundary") if ctx else None
        self._plan_boundary()
        elem_sizes = [es for es, _ in self.data_defs]
        seq = pair_seq_tags(plan)
        ng = len(self.groups)
        for g, qis in enumerate(self.groups):
            for t in plan.translates:
                src = self.domains[t.src_local]
                dst = self.domains[t.dst_local]
                nd = tuple(-c for c in t.dir)
                self._translates[g].append(
                    (t.src_local, t.dst_local, src.halo_pos(t.dir, False),
                     dst.halo_pos(nd, True), t.ext, sorted(qis))
                )
            for item, is_send in [(s, True) for s in plan.sends] + [(r, False) for r in plan.recvs]:
                total, chunks = wire_layout(item.messages, elem_sizes, qis)
                dom = self.domains[item.local_id]
                buf = torch.zeros(total, dtype=torch.uint8, device=dom.device)
                entries = []
                for mi, qi, off, nbytes in chunks:
                    m = item.messages[mi]
                    nd = tuple(-c for c in m.dir)
                    pos = dom.halo_pos(m.dir, False) if is_send else dom.halo_pos(nd, True)
                    entries.append((off, nbytes, item.local_id, pos, m.ext, qi))
                tag = seq[(item.peer_rank, item.src_gid, item.dst_gid)] * ng + g
                rec = (buf, item.peer_rank, tag, entries)
                (self._send_bufs[g] if is_send else self._recv_bufs[g]).append(rec)

    def _pack(self, g):
        for buf, _peer, _tag, entries in self._send_bufs[g]:
            for off, nbytes, li, pos, ext, qi in entries:
                reg = self.domains[li].region(qi, pos, ext).contiguous()
                buf[off : off + nbytes] = reg.view(-1).view(torch.uint8)

    def _unpack(self, g):
        for buf, _peer, _tag, entries in self._recv_bufs[g]:
            for off, nbytes, li, pos, ext, qi in entries:
                dom = self.domains[li]
                dtype = dom.curr[qi].dtype
                reg = buf[off : off + nbytes].view(dtype).reshape(ext[2], ext[1], ext[0])
                dom.region(qi, pos, ext).copy_(reg)

    def exchange(self, group: int = 0):
        g = group
        for sl, dl, spos, dpos, ext, qis in self._translates[g]:
            src = self.domains[sl]
            dst = self.domains[dl]
            for qi in qis:
                dst.region(qi, dpos, ext).copy_(src.region(qi, spos, ext))
        if self._send_bufs[g] or self._recv_bufs[g]:
            import torch.distributed as dist

            self._pack(g)
            ops = [
                dist.P2POp(dist.isend, buf, peer, tag=tag)
                for buf, peer, tag, _ in self._send_bufs[g]
            ]
            ops += [
                dist.P2POp(dist.irecv, buf, peer, tag=tag)
                for buf, peer, tag, _ in self._recv_bufs[g]
            ]
            for w in dist.batch_isend_irecv(ops):
                w.wait()
            self._unpack(g)
        if self._boundary is not None:
            self._fill_boundary(g)

    # ---- physical boundaries ----
    def _plan_boundary(self):
        """the fill as a list of tensor-slicing passes, in the DEFINING
        order: axis x, then y, then z, each pass over everything the
        earlier passes produced. A region that also points out of the
        domain on a LATER non-periodic axis is left to that axis's pass."""
        from .boundary import Boundary

        spec = self._boundary
        ng = len(self.groups)
        self._fills = [[] for _ in range(ng)]
        self.boundary_bytes = 0
        self.boundary_lines = []
        if spec is None:
            return
        for g, qis in enumerate(self.groups):
            for li, dom in enumerate(self.domains):
                regions = list(spec.out_regions(self.radius, dom.origin, dom.size))
                written = {d: 0 for d, _ in regions}
                for a in range(3):  # pass order x, y, z
                    for d, out in regions:
                        if not out[a] or any(out[b] for b in range(a + 1, 3)):
                            continue
                        ext = dom.halo_extent(d)
                        if ext[0] * ext[1] * ext[2] == 0:
                            continue
                        pos = dom.halo_pos(d, True)
                        side = 1 if d[a] > 0 else 0
                        # allocation coordinate of the first/last global cell on axis a
                        g0 = -dom.full_lo()[a]
                        edge = g0 + spec.size[a] - 1 if side else g0
                        for qi in sorted(qis):
                            k = spec.kind(qi, a, side)
                            if k == Boundary.OPEN:
                                continue
                            self._fills[g].append(
                                (li, qi, a, side, k, spec.value(qi, a, side), pos, ext, edge)
                            )
                            written[d] += ext[0] * ext[1] * ext[2] * dom.elem_sizes[qi]
                for d, nbytes in written.items():
                    self.boundary_bytes += nbytes
                    self.boundary_lines.append(
                        f"boundary_fill dir={d} local={li} group={g} bytes={nbytes}"
                    )

    _SIGN_VIEW = {2: torch.int16, 4: torch.int32, 8: torch.int64}

    def _fill_boundary(self, g):
        from .boundary import Boundary

        for li, qi, a, side, k, value, pos, ext, edge in self._fills[g]:
            dom = self.domains[li]
            dst = dom.region(qi, pos, ext)
            tdim = 2 - a  # tensors are (z, y, x)
            if k == Boundary.FIXED:
                # bit pattern, not a numeric cast: a 2-byte float quantity
                # lives in an int16 tensor here
                pat = torch.frombuffer(bytearray(value.tobytes()), dtype=dst.dtype)
                dst.copy_(pat.to(dst.device).expand(dst.shape))
                continue
            # source slab: same range as dst on the other axes
            spos, sext = list(pos), list(ext)
            if k == Boundary.CLAMP:
                spos[a], sext[a] = edge, 1
                src = dom.region(qi, spos, sext).expand(ext[2], ext[1], ext[0])
                dst.copy_(src.clone())
                continue
            # MIRROR / ANTIMIRROR: the r interior cells next to the face, reversed
            spos[a] = edge - ext[a] + 1 if side else edge
            src = dom.region(qi, spos, sext).flip(tdim)
            if k == Boundary.ANTIMIRROR:
                # IEEE negation is a sign-bit flip: do it on the integer view
                # so the result is bitwise-defined for every float width
                iv = self._SIGN_VIEW[dom.elem_sizes[qi]]
                src = src.contiguous().view(iv)
                src = (src ^ torch.iinfo(iv).min).view(dst.dtype)
            dst.copy_(src)

    def swap(self):
        for d in self.domains:
            d.curr, d.next = d.next, d.curr

    def sync(self):
        pass

    # ---- helpers mirroring NativeBackend ----
    def read_region(self, li, pos, ext, qi, from_next=False) -> bytes:
        reg = self.domains[li].region(qi, pos, ext, from_next).contiguous().cpu()
        return reg.view(-1).view(torch.uint8).numpy().tobytes()

    def write_region(self, li, data: bytes, pos, ext, qi, to_next=False):
        dom = self.domains[li]
        dtype = dom.curr[qi].dtype
        t = torch.frombuffer(bytearray(data), dtype=torch.uint8).view(dtype)
        t = t.reshape(ext[2], ext[1], ext[0]).to(dom.device)
        dom.region(qi, pos, ext, to_next).copy_(t)

    def fill_f32(self, li, qi, region_lo, region_hi, value, next_buf):
        dom = self.domains[li]
        flo = dom.full_lo()
        pos = tuple(region_lo[i] - flo[i] for i in range(3))
        ext = tuple(region_hi[i] - region_lo[i] for i in range(3))
        dom.region(qi, pos, ext, next_buf).fill_(value)

    def jacobi_step(self, li, qi, region_lo, region_hi, c_lo, c_hi, stream_id=0,
                    extend_vec=0):  # extend_vec: native-only fast-path hint, ignored here
        """reference 7-point Jacobi with hot/cold spheres (fp32)"""
        dom = self.domains[li]
        flo = dom.full_lo()
        pos = tuple(region_lo[i] - flo[i] for i in range(3))
        ext = tuple(region_hi[i] - region_lo[i] for i in range(3))
        src = dom.curr[qi]
        sl = dom._sl(pos, ext)

        def sh(dx, dy, dz):
            p = (pos[0] + dx, pos[1] + dy, pos[2] + dz)
            return src[dom._sl(p, ext)]

        avg = (sh(1, 0, 0) + sh(-1, 0, 0) + sh(0, 1, 0) + sh(0, -1, 0) + sh(0, 0, 1) + sh(0, 0, -1)) / 6.0

        # hot/cold spheres (truncated-int sqrt distance like the reference)
        device = src.device
        zz = torch.arange(region_lo[2], region_hi[2], device=device).view(-1, 1, 1)
        yy = torch.arange(region_lo[1], region_hi[1], device=device).view(1, -1, 1)
        xx = torch.arange(region_lo[0], region_hi[0], device=device).view(1, 1, -1)
        cw = c_hi[0] - c_lo[0]
        hot = (c_lo[0] + cw // 3, (c_lo[1] + c_hi[1]) // 2, (c_lo[2] + c_hi[2]) // 2)
        cold = (c_lo[0] + cw * 2 // 3, hot[1], hot[2])
        r = cw // 10

        def mask(center):
            d2 = (xx - center[0]) ** 2 + (yy - center[1]) ** 2 + (zz - center[2]) ** 2
            return torch.sqrt(d2.float()).long() <= r

        out = torch.where(mask(hot), torch.ones_like(avg), avg)
        out = torch.where(mask(cold), torch.zeros_like(avg), out)
        dom.next[qi][sl] = out

    def stencil_apply(self, li, src_qi, dst_qi, lo, hi, stencil, dtype, stream_id=0):
        """slicing reference of the native stencil_apply: next[dst_qi] =
        sum_k w_k * curr[src_qi] shifted by o_k over the global box [lo, hi),
        accumulated in the quantity's type with weights rounded to it once.
        Same validation as the native op (ValueError)."""
        import numpy as np

        dt = np.dtype(dtype)
        if dt not in (np.dtype(np.float32), np.dtype(np.float64)):
            raise ValueError(f"stencil_apply supports float32/float64, got {dt}")
        dom = self.domains[li]
        for qi in (src_qi, dst_qi):
            if not 0 <= qi < len(dom.elem_sizes):
                raise ValueError("stencil_apply: no such quantity")
            if dom.elem_sizes[qi] != dt.itemsize:
                raise ValueError(
                    "stencil_apply: element size of the quantities does not match the stencil type"
                )
        offsets, weights = stencil.offsets, stencil.weights
        if not 1 <= len(offsets) <= 128:
            raise ValueError(f"stencil_apply: want 1..128 taps, got {len(offsets)}")
        ext = tuple(hi[i] - lo[i] for i in range(3))
        if min(ext) <= 0:
            return
        flo = dom.full_lo()
        raw = dom.raw_size()
        pos = tuple(lo[i] - flo[i] for i in range(3))
        for o in [(0, 0, 0)] + offsets:
            for i in range(3):
                if pos[i] + o[i] < 0 or pos[i] + o[i] + ext[i] > raw[i]:
                    raise ValueError(
                        f"stencil_apply: tap {o} over region {lo}..{hi} reads outside the allocation"
                    )
        src = dom.curr[src_qi]
        tdt = src.dtype
        acc = torch.zeros((ext[2], ext[1], ext[0]), dtype=tdt, device=src.device)
        for o, w in zip(offsets, weights):
            p = (pos[0] + o[0], pos[1] + o[1], pos[2] + o[2])
            acc += torch.tensor(w, dtype=tdt, device=src.device) * src[dom._sl(p, ext)]
        dom.next[dst_qi][dom._sl(pos, ext)] = acc

    # ---- vector operations: slicing references of csrc/src/vector_ops.hip ----
    def _vector_views(self, op, li, lo, hi, operands):
        """validated tensor views of the operands over the global box
        [lo, hi) of local domain li (None for an empty box); the native
        ops' checks, as ValueErrors"""
        dom = self.domains[li]
        es = None
        for qi, _nxt in operands:
            if not 0 <= qi < len(dom.elem_sizes):
                raise ValueError(f"{op}: no such quantity")
            if dom.elem_sizes[qi] not in (4, 8):
                raise ValueError(
                    f"{op}: float32/float64 quantities only (element size {dom.elem_sizes[qi]})"
                )
            if es is not None and dom.elem_sizes[qi] != es:
                raise ValueError(f"{op}: operands differ in element size")
            es = dom.elem_sizes[qi]
        ext = tuple(hi[i] - lo[i] for i in range(3))
        if min(ext) <= 0:
            return None
        flo, raw = dom.full_lo(), dom.raw_size()
        pos = tuple(lo[i] - flo[i] for i in range(3))
        if any(pos[i] < 0 or pos[i] + ext[i] > raw[i] for i in range(3)):
            raise ValueError(f"{op}: region {lo}..{hi} is outside the allocation")
        return [dom.region(qi, pos, ext, nxt) for qi, nxt in operands]

    def _box_views(self, op, boxes, operands, scalars=()):
        """for every non-empty box in turn: the operands' views, then the
        scalars rounded to the views' dtype (0-d tensors on their device)"""
        for li, (lo, hi) in enumerate(boxes):
            v = self._vector_views(op, li, lo, hi, operands)
            if v is not None:
                yield (*v, *(torch.tensor(s, dtype=v[0].dtype, device=v[0].device)
                             for s in scalars))

    def field_dot(self, boxes, a, a_next, b, b_next, stream_id=0):
        """per local domain: sum of a * b over its box, products and sums in fp64"""
        out = []
        for li, (lo, hi) in enumerate(boxes):
            v = self._vector_views("field_dot", li, lo, hi, [(a, a_next), (b, b_next)])
            out.append(0.0 if v is None else float((v[0].double() * v[1].double()).sum()))
        return out

    def field_axpby(self, boxes, alpha, x, x_next, beta, y, y_next, out, out_next, stream_id=0):
        """out = alpha * x + beta * y in the quantity's type, alpha and beta
        rounded to it once; two products and one sum, no FMA"""
        for tx, ty, tout, al, be in self._box_views(
                "field_axpby", boxes, [(x, x_next), (y, y_next), (out, out_next)], (alpha, beta)):
            tout.copy_(al * tx + be * ty)

    def field_axpbypcz(self, boxes, alpha, x, x_next, beta, y, y_next, gamma, z, z_next, out,
                       out_next, stream_id=0):
        """out = alpha * x + beta * y + gamma * z in the quantity's type, the
        coefficients rounded to it once; summed left to right, no FMA"""
        for tx, ty, tz, tout, al, be, ga in self._box_views(
                "field_axpbypcz", boxes, [(x, x_next), (y, y_next), (z, z_next), (out, out_next)],
                (alpha, beta, gamma)):
            tout.copy_(al * tx + be * ty + ga * tz)

    def field_scaled_update(self, boxes, alpha, x, x_next, d, d_next, beta, y, y_next, gamma, z,
                            z_next, out, out_next, stream_id=0):
        """out = alpha * x + d * (beta * y + gamma * z) in the quantity's
        type, the coefficients rounded to it once; no FMA"""
        for tx, td, ty, tz, tout, al, be, ga in self._box_views(
                "field_scaled_update", boxes,
                [(x, x_next), (d, d_next), (y, y_next), (z, z_next), (out, out_next)],
                (alpha, beta, gamma)):
            tout.copy_(al * tx + td * (be * ty + ga * tz))

    # ---- variable-coefficient diffusion: slicing references of
    # csrc/src/diffusion_op.hip, written from the operator's definition ----
    def _diffusion_views(self, op, li, qis, lo, hi, stream_id):
        """(dom, pos, ext) of the validated global box, None when empty; the
        native ops' checks, as ValueErrors"""
        if not 0 <= li < len(self.domains):
            raise ValueError(f"{op}: no such domain {li}")
        dom = self.domains[li]
        for qi in qis:
            if not 0 <= qi < len(dom.elem_sizes):
                raise ValueError(f"{op}: no such quantity")
        sizes = {dom.elem_sizes[qi] for qi in qis}
        if not sizes <= {4, 8}:
            raise ValueError(f"{op}: float32/float64 quantities only")
        if len(sizes) != 1:
            raise ValueError(f"{op}: quantities differ in element size")
        if stream_id not in (0, 1):
            raise ValueError(f"{op}: stream id must be 0 or 1")
        ext = tuple(hi[i] - lo[i] for i in range(3))
        if min(ext) <= 0:
            return None
        flo, raw = dom.full_lo(), dom.raw_size()
        pos = tuple(lo[i] - flo[i] for i in range(3))
        if any(pos[i] < 0 or pos[i] + ext[i] > raw[i] for i in range(3)):
            raise ValueError(f"{op}: region {lo}..{hi} is outside the allocation")
        if any(pos[i] < 1 or pos[i] + ext[i] + 1 > raw[i] for i in range(3)):
            raise ValueError(f"{op}: the 1-cell face apron of region {lo}..{hi} leaves the "
                             "allocation")
        return dom, pos, ext

    @staticmethod
    def _face_neighbours(dom, t, pos, ext):
        """[(axis, view of t shifted by -1, by +1)] for axis x, y, z"""
        out = []
        for a in range(3):
            lo_p, hi_p = list(pos), list(pos)
            lo_p[a] -= 1
            hi_p[a] += 1
            out.append((a, t[dom._sl(lo_p, ext)], t[dom._sl(hi_p, ext)]))
        return out

    def diffusion_apply(self, li, src_qi, k_qi, dst_qi, lo, hi, h, sigma, dtype, stream_id=0):
        """next[dst_qi] = sigma u + sum over the six faces of
        h_a * 0.5 (k + k') * (u - u'), u = curr[src_qi], k = curr[k_qi], in
        the quantity's type (h and sigma rounded to it once)"""
        import numpy as np

        dt = np.dtype(dtype)
        if dt not in (np.dtype(np.float32), np.dtype(np.float64)):
            raise ValueError(f"diffusion_apply supports float32/float64, got {dt}")
        v = self._diffusion_views("diffusion_apply", li, (src_qi, k_qi, dst_qi), lo, hi, stream_id)
        if self.domains[li].elem_sizes[k_qi] != dt.itemsize:
            raise ValueError("diffusion_apply: element size of the quantities does not match "
                             "the type")
        if v is None:
            return
        dom, pos, ext = v
        u, k = dom.curr[src_qi], dom.curr[k_qi]
        tdt = u.dtype
        uc, kc = u[dom._sl(pos, ext)], k[dom._sl(pos, ext)]
        half = torch.tensor(0.5, dtype=tdt)
        acc = torch.tensor(sigma, dtype=tdt) * uc
        for (a, um, up), (_, km, kp) in zip(self._face_neighbours(dom, u, pos, ext),
                                            self._face_neighbours(dom, k, pos, ext)):
            ha = torch.tensor(h[a], dtype=tdt)
            acc = acc + ha * (half * (kc + km)) * (uc - um)
            acc = acc + ha * (half * (kc + kp)) * (uc - up)
        dom.next[dst_qi][dom._sl(pos, ext)] = acc

    def diffusion_inv_diagonal(self, li, k_qi, out_qi, out_next, lo, hi, h, sigma, omega,
                               stream_id=0):
        """out = omega / (sigma + sum over the six faces of h_a * 0.5 (k + k'))"""
        v = self._diffusion_views("diffusion_inv_diagonal", li, (k_qi, out_qi), lo, hi, stream_id)
        if v is None:
            return
        dom, pos, ext = v
        k = dom.curr[k_qi]
        tdt = k.dtype
        kc = k[dom._sl(pos, ext)]
        half = torch.tensor(0.5, dtype=tdt)
        diag = torch.full_like(kc, sigma)
        for a, km, kp in self._face_neighbours(dom, k, pos, ext):
            ha = torch.tensor(h[a], dtype=tdt)
            diag = diag + ha * (half * (kc + km)) + ha * (half * (kc + kp))
        dom.region(out_qi, pos, ext, out_next).copy_(torch.tensor(omega, dtype=tdt) / diag)

    # ---- grid transfer: slicing references of csrc/src/grid_transfer.hip ----
    def device_of(self, li):
        return self.domains[li].device

    def _transfer_views(self, op, fine, fli, fops, cli, cops, lo, hi):
        """(fine views over [2 lo, 2 hi), coarse views over [lo, hi)), or
        None for an empty box; the native ops' checks, as ValueErrors"""
        if not 0 <= fli < len(fine.domains) or not 0 <= cli < len(self.domains):
            raise ValueError(f"{op}: no such domain")
        fd, cd = fine.domains[fli], self.domains[cli]
        sizes = []
        for dom, ops in ((fd, fops), (cd, cops)):
            for qi, _nxt in ops:
                if not 0 <= qi < len(dom.elem_sizes):
                    raise ValueError(f"{op}: no such quantity")
                sizes.append(dom.elem_sizes[qi])
        if any(es not in (4, 8) for es in sizes):
            raise ValueError(f"{op}: float32/float64 quantities only")
        if len(set(sizes)) != 1:
            raise ValueError(f"{op}: operands differ in element size")
        if fd.device != cd.device:
            raise ValueError(f"{op}: fine and coarse domains are on different devices")
        flo, fhi = tuple(2 * c for c in lo), tuple(2 * c for c in hi)
        fv = fine._vector_views(op, fli, flo, fhi, fops)
        cv = self._vector_views(op, cli, lo, hi, cops)
        if fv is None or cv is None:
            return None
        return fv, cv

    def grid_restrict(self, fine, fli, alpha, a, a_next, beta, b, b_next, cli, out, out_next,
                      lo, hi, stream_id=0):
        """self is the coarse backend: out(c) = 0.125 * the sum over the 8
        children of alpha a + beta b, in the quantity's type"""
        v = self._transfer_views("grid_restrict", fine, fli, [(a, a_next), (b, b_next)], cli,
                                 [(out, out_next)], lo, hi)
        if v is None:
            return
        (ta, tb), (tout,) = v
        al = torch.tensor(alpha, dtype=ta.dtype, device=ta.device)
        be = torch.tensor(beta, dtype=ta.dtype, device=ta.device)
        val = al * ta + be * tb
        ez, ey, ex = tout.shape
        s = val.reshape(ez, 2, ey, 2, ex, 2)
        acc = torch.zeros_like(tout)
        for dz in (0, 1):
            for dy in (0, 1):
                for dx in (0, 1):
                    acc += s[:, dz, :, dy, :, dx]
        tout.copy_(acc * 0.125)

    def grid_prolong_add(self, coarse, cli, src, src_next, fli, dst, dst_next, lo, hi,
                         stream_id=0):
        """self is the fine backend: dst(p) += src(p >> 1) over [2 lo, 2 hi)"""
        v = coarse._transfer_views("grid_prolong_add", self, fli, [(dst, dst_next)], cli,
                                   [(src, src_next)], lo, hi)
        if v is None:
            return
        (tdst,), (tsrc,) = v
        ez, ey, ex = tsrc.shape
        tdst += tsrc[:, None, :, None, :, None].expand(ez, 2, ey, 2, ex, 2).reshape(
            2 * ez, 2 * ey, 2 * ex)

    def _check_cg_update(self, op, boxes, x, p, r):
        """ValueError unless x, p and r are distinct and every operand is
        valid on every box: nothing has been written then"""
        if x == p or x == r or p == r:
            raise ValueError(f"{op}: x, p and r must be distinct quantities")
        for li, (lo, hi) in enumerate(boxes):
            self._vector_views(op, li, lo, hi, [(x, False), (p, False), (p, True), (r, False)])

    def cg_update(self, boxes, alpha, x, p, r, stream_id=0):
        """the unfused composition: x = 1 x + alpha p; r = 1 r + (-alpha) A p
        (A p in next[p]); returns each domain's dot(r, r)"""
        self._check_cg_update("cg_update", boxes, x, p, r)
        self.field_axpby(boxes, 1.0, x, False, alpha, p, False, x, False)
        self.field_axpby(boxes, 1.0, r, False, -alpha, p, True, r, False)
        return self.field_dot(boxes, r, False, r, False)

    # ---- the reductions of singular problems (vector_ops.hip's second family) ----
    def field_sum(self, boxes, a, a_next, stream_id=0):
        """per local domain: sum of a over its box, in fp64"""
        out = []
        for li, (lo, hi) in enumerate(boxes):
            v = self._vector_views("field_sum", li, lo, hi, [(a, a_next)])
            out.append(0.0 if v is None else float(v[0].double().sum()))
        return out

    def field_dot_sums(self, boxes, a, a_next, b, b_next, stream_id=0):
        """per local domain: (sum a * b, sum a, sum b) over its box, products
        and sums in fp64"""
        out = []
        for li, (lo, hi) in enumerate(boxes):
            v = self._vector_views("field_dot_sums", li, lo, hi, [(a, a_next), (b, b_next)])
            if v is None:
                out.append((0.0, 0.0, 0.0))
                continue
            ta, tb = v[0].double(), v[1].double()
            out.append((float((ta * tb).sum()), float(ta.sum()), float(tb.sum())))
        return out

    def cg_update_sum(self, boxes, alpha, x, p, r, stream_id=0):
        """cg_update, returning (dot(r, r), sum r) per domain"""
        self._check_cg_update("cg_update_sum", boxes, x, p, r)
        self.field_axpby(boxes, 1.0, x, False, alpha, p, False, x, False)
        self.field_axpby(boxes, 1.0, r, False, -alpha, p, True, r, False)
        return [(rr, sr) for rr, sr, _ in self.field_dot_sums(boxes, r, False, r, False)]

    def field_axpbyc(self, boxes, alpha, x, x_next, beta, y, y_next, c, out, out_next,
                     stream_id=0):
        """out = alpha * x + beta * y + c in the quantity's type, alpha, beta
        and c rounded to it once; summed left to right, no FMA"""
        for tx, ty, tout, al, be, cc in self._box_views(
                "field_axpbyc", boxes, [(x, x_next), (y, y_next), (out, out_next)],
                (alpha, beta, c)):
            tout.copy_(al * tx + be * ty + cc)

    # ---- the fused passes of BiCGStab (vector_ops.hip's third family) ----
    def field_axpby_norm2(self, boxes, alpha, x, x_next, beta, y, y_next, out, out_next,
                          stream_id=0):
        """field_axpby, returning each domain's sum of out^2 (the stored
        out, squares and sums in fp64)"""
        self.field_axpby(boxes, alpha, x, x_next, beta, y, y_next, out, out_next)
        return self.field_dot(boxes, out, out_next, out, out_next)

    def field_dot_pair(self, boxes, a, a_next, b, b_next, stream_id=0):
        """per local domain: (sum a * b, sum a * a) over its box, in fp64"""
        res = []
        for li, (lo, hi) in enumerate(boxes):
            v = self._vector_views("field_dot_pair", li, lo, hi, [(a, a_next), (b, b_next)])
            if v is None:
                res.append((0.0, 0.0))
                continue
            ta, tb = v[0].double(), v[1].double()
            res.append((float((ta * tb).sum()), float((ta * ta).sum())))
        return res

    def bicgstab_update(self, boxes, alpha, y, y_next, omega, z, z_next, x, r, t, t_next, rhat,
                        rhat_next, stream_id=0):
        """x = x + alpha y + omega z; r = r - omega t, in the quantity's
        type with alpha and omega rounded to it once, every operand read
        before x and r are written (z may be the buffer of r); returns each
        domain's (dot(r, r), dot(rhat, r))"""
        op = "bicgstab_update"
        reads = [(y, y_next), (t, t_next), (rhat, rhat_next)]
        if x == r or any(not nxt and q in (x, r) for q, nxt in reads):
            raise ValueError(f"{op}: x and r must be distinct from each other and from y, t "
                             "and rhat")
        operands = [(y, y_next), (z, z_next), (x, False), (r, False), (t, t_next),
                    (rhat, rhat_next)]
        views = [self._vector_views(op, li, lo, hi, operands)
                 for li, (lo, hi) in enumerate(boxes)]  # validate before any write
        res = []
        for v in views:
            if v is None:
                res.append((0.0, 0.0))
                continue
            ty, tz, tx, tr, tt, th = v
            al = torch.tensor(alpha, dtype=tx.dtype, device=tx.device)
            om = torch.tensor(omega, dtype=tx.dtype, device=tx.device)
            xn = tx + al * ty + om * tz
            rn = tr - om * tt
            tx.copy_(xn)
            tr.copy_(rn)
            rd = rn.double()
            res.append((float((rd * rd).sum()), float((th.double() * rd).sum())))
        return res

    def sync_compute(self):
        pass
