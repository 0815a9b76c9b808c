#!/usr/bin/env python3
"""BiCGStab benchmark: (sigma I + v . grad - nu laplacian) x = b on a size^3
grid with AdvectionDiffusion3D. --iters N runs exactly N iterations (the
tolerance is then 0); without it the problem is solved to --tol with at
most --max-iter iterations. --precond mg right-preconditions with the multigrid
V-cycle of the operator's symmetric part.

Prints one JSON line: ms_per_iter, iterations, reason, restarts, solve_ms
and the host wall time per iteration of the phases (each ends in a host
sync):
  operator_ms   the two apply_stencil + exchange of an iteration (and the
                verify step)
  reduction_ms  rhat . v and (t . s, t . t)
  update_ms     the p update, axpby_norm2 and bicgstab_update
  precond_ms    the two cycles (--precond mg)
With --tol also true_residual: ||b - A x|| / ||b|| as the solver's own
kernels compute it after the solve.

--kernels N adds a kernel-only window per new vector kernel (N calls, each
waiting for its value as the solver does) with its effective bandwidth,
one element read or written counting as one pass: axpby_norm2 3, dot_pair
2, bicgstab_update 8, or 7 with z the buffer of r (the unpreconditioned
solver's call, bicgstab_update_z_is_r). And the 8-pass update against its
composition from the ops there were before, x += alpha y + omega z
(axpbypcz, 4), r -= omega t (axpby, 3), r . r and rhat . r (two dots,
2 + 2): 11 passes, alternated old, new, old, new in one process so that
drift hits both alike (bicgstab_update_pair_ms, bicgstab_update_ratio =
new / old of the means; the passes predict 8/11).
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

import numpy as np

import stencil_amd as sa
from stencil_amd import Boundary
from stencil_amd.models.advection_diffusion3d import AdvectionDiffusion3D

_BOUNDARIES = {
    "periodic": None,
    "fixed": {"all": (Boundary.FIXED, 0)},
    "mirror": {"all": (Boundary.MIRROR, 0)},
    "antimirror": {"all": (Boundary.ANTIMIRROR, 0)},
    "clamp": {"all": (Boundary.CLAMP, 0)},
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256, help="edge of the global cube")
    ap.add_argument("--velocity", type=float, nargs=3, default=[1.0, 0.5, -0.25])
    ap.add_argument("--nu", type=float, default=1.0)
    ap.add_argument("--sigma", type=float, default=1.0)
    ap.add_argument("--scheme", default="upwind", choices=["upwind", "central"])
    ap.add_argument("--dtype", default="f32", choices=["f32", "f64"])
    ap.add_argument("--boundary", default="periodic", choices=sorted(_BOUNDARIES))
    ap.add_argument("--precond", default="none", choices=["none", "mg"])
    ap.add_argument("--iters", type=int, default=None,
                    help="run exactly this many iterations (tolerance 0)")
    ap.add_argument("--tol", type=float, default=1e-6)
    ap.add_argument("--max-iter", type=int, default=5000, help="the cap of a solve to --tol")
    ap.add_argument("--warmup", type=int, default=2, help="iterations of an untimed first solve")
    ap.add_argument("--backend", default="native", choices=["native", "torch"])
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--no-overlap", action="store_true")
    ap.add_argument("--kernels", type=int, default=0, metavar="N",
                    help="also time N calls of each new vector kernel and of the unfused update")
    args = ap.parse_args()

    dtype = np.float32 if args.dtype == "f32" else np.float64
    gpus = list(range(args.gpus)) if args.backend == "native" else [0] * args.gpus
    size = (args.size,) * 3
    app = AdvectionDiffusion3D(size, velocity=args.velocity, nu=args.nu, sigma=args.sigma,
                               scheme=args.scheme, dtype=dtype, backend=args.backend, gpus=gpus,
                               boundary=_BOUNDARIES[args.boundary],
                               preconditioner="multigrid" if args.precond == "mg" else None)
    app.realize()
    dd = app.dd
    rng = np.random.default_rng(0)
    for li in range(dd.num_local()):
        lo, hi = dd.local_rect(li)
        shape = (hi[2] - lo[2], hi[1] - lo[1], hi[0] - lo[0])
        dd.write_global(li, lo, rng.standard_normal(shape, dtype=np.float32).astype(dtype), app.b)

    overlap = not args.no_overlap
    exact = args.iters is not None
    tol, max_iter = (0.0, args.iters) if exact else (args.tol, args.max_iter)
    if args.warmup:
        app.solve(tol=0.0, max_iter=args.warmup, overlap=overlap)
    dd.backend.sync()
    t0 = time.perf_counter()
    res = app.solve(tol=tol, max_iter=max_iter, overlap=overlap)
    dd.backend.sync()
    dt = time.perf_counter() - t0
    n = max(res.iterations, 1)
    cells = size[0] * size[1] * size[2]
    ph = app.solver.phase_times
    out = {
        "benchmark": "advection_diffusion",
        "size": args.size,
        "velocity": list(args.velocity),
        "nu": args.nu,
        "sigma": args.sigma,
        "scheme": args.scheme,
        "dtype": args.dtype,
        "boundary": args.boundary,
        "precond": args.precond,
        "gpus": args.gpus,
        "backend": args.backend,
        "overlap": overlap,
        "tol": tol,
        "iterations": res.iterations,
        "converged": res.converged,
        "reason": res.reason,
        "restarts": app.solver.restarts,
        "final_residual": res.residuals[-1],
        "solve_ms": dt * 1e3,
        "ms_per_iter": dt / n * 1e3,
        "gcells_per_s": cells / (dt / n * 1e3) / 1e6,
        "operator_ms": ph["operator"] / n * 1e3,
        "reduction_ms": ph["reduction"] / n * 1e3,
        "update_ms": ph["update"] / n * 1e3,
    }
    if app.mg is not None:
        out["precond_ms"] = ph["precond"] / n * 1e3
        out["levels"] = [list(lv) for lv in app.mg.levels]
    if not exact:
        # r is free after the solve: b - A x with the solver's own kernels
        rr = app.solver._true_residual(overlap)
        out["true_residual"] = float(np.sqrt(rr / dd.dot(app.b)))

    if args.kernels:
        k = args.kernels
        es = np.dtype(dtype).itemsize
        x, r, rhat, p = app.x, app.r, app.rhat, app.p
        nxt = sa.Next

        def window(fn):
            fn()
            dd.backend.sync()
            t = time.perf_counter()
            for _ in range(k):
                fn()
            dd.backend.sync()
            return (time.perf_counter() - t) / k * 1e3

        def report(name, passes, t_ms):
            out[f"{name}_kernel_ms"] = t_ms
            out[f"{name}_gb_per_s"] = passes * cells * es / t_ms / 1e6

        # scalars that leave the fields where they are: the windows measure
        # traffic, and the data must stay finite over 4 k calls. z = b is
        # the call with a separate z (8 passes), z = r the plain solver's (7)
        b = app.b

        def fused():
            return dd.bicgstab_update(1e-30, p, 1e-30, b, x, r, nxt(r), rhat)

        def unfused():
            dd.axpbypcz(1.0, x, 1e-30, p, 1e-30, b, out=x)
            dd.axpby(1.0, r, -1e-30, nxt(r), out=r)
            return dd.dot(r), dd.dot(rhat, r)

        report("axpby_norm2", 3,
               window(lambda: dd.axpby_norm2(1.0, r, -1e-30, nxt(p), out=r)))
        report("dot_pair", 2, window(lambda: dd.dot_pair(nxt(r), r)))
        report("bicgstab_update_z_is_r", 7,
               window(lambda: dd.bicgstab_update(1e-30, p, 1e-30, r, x, r, nxt(r), rhat)))
        ts = [window(unfused), window(fused), window(unfused), window(fused)]
        report("bicgstab_update", 8, (ts[1] + ts[3]) / 2)
        report("unfused_update", 11, (ts[0] + ts[2]) / 2)
        out["bicgstab_update_pair_ms"] = ts
        out["bicgstab_update_ratio"] = (ts[1] + ts[3]) / (ts[0] + ts[2])
        t = time.perf_counter()
        for _ in range(k):
            dd.backend.sync_compute()
        out["empty_sync_ms"] = (time.perf_counter() - t) / k * 1e3
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
