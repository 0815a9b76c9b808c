#!/usr/bin/env python3
"""Generic stencil operator benchmark: explicit diffusion
u <- u + alpha_dt * laplacian(u) (star path, --order 2/4/6/8) or a 27-point
box smoother (--box, general tap-table path) on a size^3 periodic grid.

Prints one JSON line with ms_per_step and gcells_per_s.

Default: whole eager steps (DistributedDomain.step_stencil: interior,
exchange, exterior, sync, swap). --kernel-only times the operator alone
over the whole local rect: all steps enqueued, one device sync.
--compare-jacobi N (native, fp32, one GPU) alternates N rounds of the
kernel-only window with the same window of jacobi_step(extend_vec=0) and
reports both medians, their spreads and the ratio.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

import numpy as np

import stencil_amd as sa
from stencil_amd.models.diffusion3d import Diffusion3D


def box27():
    """27-point smoother: weights 1/27 (not a star: general path)"""
    return sa.Stencil.from_array(np.full((3, 3, 3), 1.0 / 27.0), (1, 1, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256, help="edge of the global cube")
    ap.add_argument("--order", type=int, default=2, choices=[2, 4, 6, 8])
    ap.add_argument("--dtype", default="f32", choices=["f32", "f64"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--backend", default="native", choices=["native", "torch"])
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--box", action="store_true", help="27-point box stencil (general path)")
    ap.add_argument("--no-overlap", action="store_true")
    ap.add_argument("--kernel-only", action="store_true",
                    help="time the operator alone over the whole local rect, one sync")
    ap.add_argument("--compare-jacobi", type=int, default=0, metavar="N",
                    help="N alternating rounds against jacobi_step(extend_vec=0)")
    args = ap.parse_args()

    dtype = np.float32 if args.dtype == "f32" else np.float64
    gpus = list(range(args.gpus)) if args.backend == "native" else [0] * args.gpus
    size = (args.size,) * 3
    app = Diffusion3D(size, order=args.order, dtype=dtype, alpha_dt=0.05,
                      backend=args.backend, gpus=gpus)
    if args.box:
        app.stencil = box27()
        app.dd.set_radius(app.stencil.radius())
    app.realize()
    dd, h, st = app.dd, app.h, app.stencil

    # seeded smooth-ish initial field in both buffers
    rng = np.random.default_rng(0)
    for li in range(dd.num_local()):
        lo, hi = dd.local_rect(li)
        shape = (hi[2] - lo[2], hi[1] - lo[1], hi[0] - lo[0])
        block = rng.random(shape, dtype=np.float32).astype(dtype)
        dd.write_global(li, lo, block, h)
        dd.write_global(li, lo, block, h, to_next=True)
    dd.exchange()

    def sync():
        dd.backend.sync()

    def stencil_window(n):
        for _ in range(n):
            dd.apply_stencil(st, h, where="all")
        sync()

    def jacobi_window(n):
        for li in range(dd.num_local()):
            lo, hi = dd.local_rect(li)
            for _ in range(n):
                dd.backend.jacobi_step(li, h.index, lo, hi, (0, 0, 0), dd.size, extend_vec=0)
        sync()

    def timed(fn, n):
        sync()
        t0 = time.perf_counter()
        fn(n)
        return (time.perf_counter() - t0) / n * 1e3

    cells = size[0] * size[1] * size[2]
    out = {
        "benchmark": "stencil_apply",
        "stencil": "box27" if args.box else f"diffusion_order{args.order}",
        "ntaps": st.ntaps,
        "path": "star" if st.is_star else "general",
        "dtype": args.dtype,
        "size": args.size,
        "gpus": args.gpus,
        "backend": args.backend,
        "steps": args.steps,
        "warmup": args.warmup,
    }
    if args.compare_jacobi:
        if args.backend != "native" or args.dtype != "f32" or args.gpus != 1:
            ap.error("--compare-jacobi needs --backend native --dtype f32 --gpus 1")
        stencil_window(args.warmup)
        jacobi_window(args.warmup)
        ts, tj = [], []
        for _ in range(args.compare_jacobi):
            ts.append(timed(stencil_window, args.steps))
            tj.append(timed(jacobi_window, args.steps))
        ms, mj = statistics.median(ts), statistics.median(tj)
        out.update({
            "mode": "kernel-only-vs-jacobi",
            "ms_per_step": ms,
            "gcells_per_s": cells / ms / 1e6,
            "stencil_ms_runs": ts,
            "stencil_spread_ms": max(ts) - min(ts),
            "jacobi_ms_per_step": mj,
            "jacobi_gcells_per_s": cells / mj / 1e6,
            "jacobi_ms_runs": tj,
            "jacobi_spread_ms": max(tj) - min(tj),
            "stencil_over_jacobi_time": ms / mj,
        })
    elif args.kernel_only:
        stencil_window(args.warmup)
        ms = timed(stencil_window, args.steps)
        out.update({"mode": "kernel-only", "ms_per_step": ms, "gcells_per_s": cells / ms / 1e6})
    else:
        for _ in range(args.warmup):
            app.step(overlap=not args.no_overlap)
        ms = timed(lambda n: app.run(n, overlap=not args.no_overlap), args.steps)
        out.update({
            "mode": "step",
            "overlap": not args.no_overlap,
            "ms_per_step": ms,
            "gcells_per_s": cells / ms / 1e6,
            "exchange_bytes_per_step": dd.exchange_bytes_for_method(dd.methods),
        })
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
