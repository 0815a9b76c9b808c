#!/usr/bin/env python3
"""Conjugate-gradient benchmark: (sigma I - laplacian) x = b on a size^3
grid with Poisson3D, exactly --iters iterations (--tol 0, the default), or
solved to --tol T > 0 with at most --iters iterations: the record then
holds iterations, converged, solve_ms and levels as well. --precond mg
preconditions with the geometric multigrid V-cycle and adds precond_ms, the
host wall time per level of one cycle (mg_level_ms) and coarse_share, the
part of a cycle spent on levels >= 1.

Prints one JSON line: ms_per_iter, gcells_per_s and the host wall time per
iteration of the three phases (each ends in a host sync):
  operator_ms  apply_stencil(A, p) + exchange of p
  dot_ms       p . A p
  update_ms    cg_update (x, r, r . r) + the p update
--kernels N adds a kernel-only window per vector kernel (N launches
enqueued, one sync) with its effective bandwidth, one element read or
written counting as one pass: dot 2, cg_update 6, the p update 3; and the
cost of one empty host sync of the compute stream. With --precond mg also
axpbypcz 4, grid_restrict 2 + 1/8 and grid_prolong_add 2 + 1/8 passes over
the fine grid.

--coefficient one|smooth|jump solves (sigma I - div(k grad)) x = b instead,
with k = 1, a smooth field of contrast 55 or a jump 1 : --contrast (see
coefficient_field); --precond jacobi is the diagonal preconditioner it makes
possible. The record then holds coefficient (and contrast), and --kernels
adds diffusion_apply (3 passes: u, k, out) and scaled_update (5 passes, in
place). Without --coefficient the output is what it was.

--nullspace constant solves the singular problem (--sigma 0 with --boundary
periodic or mirror) with the solver's projection off the constants; the
record then holds nullspace, and corrections, the number of correction
solves the true-residual check asked for. --kernels also times each kernel
of the projection against the existing kernel of equal traffic, alternated
old, new, old, new in one process: dot_sums : dot, cg_update_sum :
cg_update, axpbyc : axpby (the *_pair_ms lists, and *_ratio = new / old of
the means).
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
from stencil_amd.models.poisson3d import Poisson3D

_BOUNDARIES = {
    "periodic": None,
    "fixed": {"all": (Boundary.FIXED, 0)},
    "mirror": {"all": (Boundary.MIRROR, 0)},
    "antimirror": {"all": (Boundary.ANTIMIRROR, 0)},
}


def coefficient_field(kind, size, contrast=16.0):
    """the (z, y, x) fp64 k field: 'smooth' = exp(1.5 sin(2 pi x/nx)
    cos(2 pi y/ny) + 0.5 sin(2 pi z/nz)) (contrast 55), 'jump' = contrast
    where x >= nx/2 and y < ny/2, else 1"""
    nx, ny, nz = size
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    if kind == "smooth":
        return np.exp(1.5 * np.sin(2 * np.pi * x / nx) * np.cos(2 * np.pi * y / ny)
                      + 0.5 * np.sin(2 * np.pi * z / nz))
    if kind == "jump":
        return np.where((x >= nx / 2) & (y < ny / 2), float(contrast), 1.0)
    raise ValueError(kind)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256, help="edge of the global cube")
    ap.add_argument("--order", type=int, default=2, choices=[2, 4, 6, 8])
    ap.add_argument("--dtype", default="f32", choices=["f32", "f64"])
    ap.add_argument("--sigma", type=float, default=1.0)
    ap.add_argument("--boundary", default="periodic", choices=sorted(_BOUNDARIES))
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3, help="iterations of an untimed first solve")
    ap.add_argument("--backend", default="native", choices=["native", "torch"])
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--no-overlap", action="store_true")
    ap.add_argument("--kernels", type=int, default=0, metavar="N",
                    help="also time N back-to-back launches of each vector kernel")
    ap.add_argument("--precond", default="none", choices=["none", "mg", "jacobi"])
    ap.add_argument("--coefficient", default="none", choices=["none", "one", "smooth", "jump"],
                    help="variable-coefficient operator with this k field")
    ap.add_argument("--contrast", type=float, default=16.0, help="the high value of 'jump'")
    ap.add_argument("--tol", type=float, default=0.0,
                    help="0: exactly --iters iterations; > 0: solve to this tolerance")
    ap.add_argument("--nullspace", default="none", choices=["none", "constant"],
                    help="constant: the singular problem, --sigma 0 --boundary periodic|mirror")
    args = ap.parse_args()
    if args.nullspace == "constant" and not (
            args.sigma == 0.0 and args.boundary in ("periodic", "mirror")):
        ap.error("--nullspace constant needs --sigma 0 and --boundary periodic or mirror")

    dtype = np.float32 if args.dtype == "f32" else np.float64
    gpus = list(range(args.gpus)) if args.backend == "native" else [0] * args.gpus
    size = (args.size,) * 3
    app = Poisson3D(size, order=args.order, dtype=dtype, sigma=args.sigma, backend=args.backend,
                    gpus=gpus, boundary=_BOUNDARIES[args.boundary],
                    preconditioner={"none": None, "mg": "multigrid", "jacobi": "jacobi"}[args.precond],
                    coefficient=args.coefficient != "none",
                    nullspace=None if args.nullspace == "none" else args.nullspace)
    app.realize()
    dd = app.dd
    if args.coefficient in ("smooth", "jump"):
        app.set_coefficient(coefficient_field(args.coefficient, size, args.contrast))
    rng = np.random.default_rng(0)
    for li in range(dd.num_local()):
        lo, hi = dd.local_rect(li)
        shape = (hi[2] - lo[2], hi[1] - lo[1], hi[0] - lo[0])
        dd.write_global(li, lo, rng.standard_normal(shape, dtype=np.float32).astype(dtype), app.b)

    overlap = not args.no_overlap
    if args.warmup:
        app.solve(tol=0.0, max_iter=args.warmup, overlap=overlap)
    dd.backend.sync()
    if app.mg is not None:
        app.mg.reset_times()
    t0 = time.perf_counter()
    res = app.solve(tol=args.tol, max_iter=args.iters, overlap=overlap)
    dd.backend.sync()
    dt = time.perf_counter() - t0
    n = max(res.iterations, 1)
    cells = size[0] * size[1] * size[2]
    ms = dt / n * 1e3
    ph = app.cg.phase_times
    out = {
        "benchmark": "poisson_cg",
        "size": args.size,
        "order": args.order,
        "dtype": args.dtype,
        "sigma": args.sigma,
        "boundary": args.boundary,
        "gpus": args.gpus,
        "backend": args.backend,
        "overlap": overlap,
        "iters": res.iterations,
        "reason": res.reason,
        "final_residual": res.residuals[-1],
        "ms_per_iter": ms,
        "gcells_per_s": cells / ms / 1e6,
        "operator_ms": ph["operator"] / n * 1e3,
        "dot_ms": ph["dot"] / n * 1e3,
        "update_ms": ph["update"] / n * 1e3,
        "precond": args.precond,
        "tol": args.tol,
    }
    if args.coefficient != "none":
        out["coefficient"] = args.coefficient
        if args.coefficient == "jump":
            out["contrast"] = args.contrast
        if app.jacobi is not None:
            out["precond_ms"] = ph["precond"] / n * 1e3
    if args.nullspace != "none":
        out["nullspace"] = args.nullspace
        out["corrections"] = app.cg.corrections
    if args.tol > 0:
        out["iterations"] = res.iterations
        out["converged"] = res.converged
        out["solve_ms"] = dt * 1e3
        out["levels"] = [list(lv) for lv in app.mg.levels] if app.mg is not None else None
    if app.mg is not None:
        cycles = res.iterations + 1  # one per iteration and the first z = M r
        level_ms = [t / cycles * 1e3 for t in app.mg.phase_times.values()]
        out["precond_ms"] = ph["precond"] / n * 1e3
        out["mg_level_ms"] = level_ms
        out["coarse_share"] = sum(level_ms[1:]) / sum(level_ms)

    if args.kernels:
        k = args.kernels
        es = np.dtype(dtype).itemsize
        x, r, p = app.x, app.r, app.p

        def window(fn, sync=dd.backend.sync):
            fn()
            sync()
            t = time.perf_counter()
            for _ in range(k):
                fn()
            sync()
            return (time.perf_counter() - t) / k * 1e3

        def report(name, passes, t_ms):
            out[f"{name}_kernel_ms"] = t_ms
            out[f"{name}_gb_per_s"] = passes * cells * es / t_ms / 1e6

        report("axpby", 3, window(lambda: dd.axpby(1.0, r, 0.5, p, out=p)))
        report("stencil", 2, window(lambda: dd.apply_stencil(app.stencil, p, where="all")))
        # the reductions wait for their value: a window of k synchronous calls
        report("dot", 2, window(lambda: dd.dot(p, sa.Next(p))))
        report("cg_update", 6, window(lambda: dd.cg_update(1e-30, x, p, r)))
        if app.op is not None:
            # 3 passes: read u, read k, write; 5 passes in place: x, d, y, z, out
            report("diffusion_apply", 3, window(lambda: app.op.apply(p, where="all")))
            report("scaled_update", 5,
                   window(lambda: dd.scaled_update(1.0, x, app.dinv, 1e-30, r, -1e-30, sa.Next(p),
                                                   out=x)))
        if app.mg is not None:
            z, top = app.z, app.mg._levels[0]
            coarse = app.mg._levels[1]
            report("axpbypcz", 4,
                   window(lambda: dd.axpbypcz(1.0, z, 1e-30, r, -1e-30, sa.Next(z), out=z)))

            # each transfer call syncs its source side first, an idle stream
            # here; the restriction runs on the coarse domain's stream
            report("grid_restrict", 2.125,
                   window(lambda: top.transfer.restrict(1.0, r, -1.0, sa.Next(z), coarse.f),
                          sync=coarse.dd.backend.sync))
            report("grid_prolong_add", 2.125,
                   window(lambda: top.transfer.prolong_add(coarse.f, z)))

        # the projection's kernels against the kernels of equal traffic,
        # alternated old, new, old, new so that drift hits both alike
        def pair(name, old, new):
            ts = [window(old), window(new), window(old), window(new)]
            out[f"{name}_pair_ms"] = ts
            out[f"{name}_ratio"] = (ts[1] + ts[3]) / (ts[0] + ts[2])

        pair("dot_sums", lambda: dd.dot(p, sa.Next(p)), lambda: dd.dot_sums(p, sa.Next(p)))
        pair("cg_update_sum", lambda: dd.cg_update(1e-30, x, p, r),
             lambda: dd.cg_update_sum(1e-30, x, p, r))
        pair("axpbyc", lambda: dd.axpby(1.0, r, 0.5, p, out=p),
             lambda: dd.axpbyc(1.0, r, 0.5, p, 1e-30, out=p))
        t = time.perf_counter()
        for _ in range(k):
            dd.backend.sync_compute()
        out["empty_sync_ms"] = (time.perf_counter() - t) / k * 1e3
        # the control-plane sum of the per-rank values (world 1: no collective)
        t = time.perf_counter()
        for _ in range(k):
            dd._global_sum([1.0] * dd.num_local())
        out["global_sum_ms"] = (time.perf_counter() - t) / k * 1e3
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
