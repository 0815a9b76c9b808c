"""GridTransfer: restriction and prolongation between two
DistributedDomains on cell-centred 2:1 coarsening (coarse cell c has the 8
fine children 2c + {0,1}^3). The kernels are csrc/src/grid_transfer.hip on
the native backend and tensor reshapes on the torch backend.

    restrict:     coarse out(c)  = mean over the children of alpha a + beta b
    prolong_add:  fine   dst(p) += src(p >> 1)

The prolongation is piecewise-constant injection, 8 x the transpose of the
restriction: a V-cycle built from the pair is symmetric.

Both domains live in one process and are partitioned alike: local domain li
of the coarse one is exactly the halved rectangle of local domain li of the
fine one, on the same device, so a transfer never leaves a GPU. Each call
first waits for the source domain's compute streams on the host
(sync_compute) and then enqueues on the destination's compute stream 0.
"""
from __future__ import annotations

import numpy as np

from ..core import DataHandle, DistributedDomain, Next


def _operand(op: str, o, dtype=None):
    nxt = isinstance(o, Next)
    h = o.handle if nxt else o
    if not isinstance(h, DataHandle):
        raise TypeError(f"{op}: operands are DataHandles or Next(DataHandle)")
    if h.dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise ValueError(f"{op} supports float32/float64 quantities, got {h.dtype}")
    if dtype is not None and h.dtype != dtype:
        raise ValueError(f"{op}: operands mix {dtype} and {h.dtype}")
    return h.index, nxt, h.dtype


class GridTransfer:
    def __init__(self, fine: DistributedDomain, coarse: DistributedDomain):
        """both domains are realized. Raises ValueError unless they have the
        same backend kind and number of local domains and local domain li of
        `coarse` is the halved rectangle of local domain li of `fine` on
        the same device."""
        if not (fine._realized and coarse._realized):
            raise ValueError("GridTransfer: construct after both domains are realized")
        if fine.backend_kind != coarse.backend_kind:
            raise ValueError("GridTransfer: the domains use different backends")
        if fine.num_local() != coarse.num_local():
            raise ValueError(
                f"GridTransfer: {fine.num_local()} fine local domains but "
                f"{coarse.num_local()} coarse ones"
            )
        self.boxes = []
        for li in range(fine.num_local()):
            flo, fhi = fine.local_rect(li)
            clo, chi = coarse.local_rect(li)
            if tuple(2 * c for c in clo) != tuple(flo) or tuple(2 * c for c in chi) != tuple(fhi):
                raise ValueError(
                    f"GridTransfer: coarse local domain {li} is {clo}..{chi}, not the half of the "
                    f"fine one {flo}..{fhi}"
                )
            if fine.backend.device_of(li) != coarse.backend.device_of(li):
                raise ValueError(
                    f"GridTransfer: local domain {li} is on device {fine.backend.device_of(li)} "
                    f"in the fine domain and on {coarse.backend.device_of(li)} in the coarse one"
                )
            self.boxes.append((tuple(clo), tuple(chi)))
        self.fine, self.coarse = fine, coarse

    def restrict(self, alpha: float, a, beta: float, b, out):
        """out (a quantity of the coarse domain) = the mean over the 8
        children of alpha a + beta b (quantities of the fine domain), over
        every local rectangle, in the quantity's type"""
        qa, na, dt = _operand("restrict", a)
        qb, nb, _ = _operand("restrict", b, dt)
        qo, no, _ = _operand("restrict", out, dt)
        self.fine.backend.sync_compute()
        for li, (lo, hi) in enumerate(self.boxes):
            self.coarse.backend.grid_restrict(self.fine.backend, li, float(alpha), qa, na,
                                              float(beta), qb, nb, li, qo, no, lo, hi)

    def prolong_add(self, src, dst):
        """dst (fine) += src (coarse) of the parent cell, over every local
        rectangle"""
        qs, ns, dt = _operand("prolong_add", src)
        qd, nd, _ = _operand("prolong_add", dst, dt)
        self.coarse.backend.sync_compute()
        for li, (lo, hi) in enumerate(self.boxes):
            self.fine.backend.grid_prolong_add(self.coarse.backend, li, qs, ns, li, qd, nd, lo, hi)
