"""Singular Poisson problems on the torch backend (CPU tier): the four
vector operations of the projection P v = v - mean(v) against exact numpy,
the argument checks of ConjugateGradient / Poisson3D(nullspace=...), the
singular solves against the truth operator, grid independence of the
multigrid iteration count, nullspace=None as the old solver, rank agreement
over gloo and the benchmark CLI."""
import json
import multiprocessing as mp
import os
import subprocess
import sys

import numpy as np
import pytest

from stencil_amd import Boundary, Stencil
from stencil_amd.models.poisson3d import Poisson3D
from stencil_amd.solvers import ConjugateGradient
from stencil_amd.solvers.diffusion import DiffusionOperator

import boundary_util
import cg_util as cu
import nullspace_util as nu
import stencil_util as su

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE = (19, 10, 9)
BOX = ((3, 1, 1), (16, 8, 8))

_DOMAINS = [([0], None), ([0, 0], None), ([0], BOX)]
_DOMAIN_IDS = ["1dom-all", "2dom-all", "1dom-box"]


# ------------------------------------------------------------ vector operations
@pytest.mark.parametrize("dtype", nu.DTYPES, ids=nu.DT_IDS)
@pytest.mark.parametrize("gpus,box", _DOMAINS, ids=_DOMAIN_IDS)
def test_sum_and_dot_sums_match_numpy(gpus, box, dtype):
    nu.check_reductions_exact("torch", SIZE, gpus, dtype, *(box or ()))


@pytest.mark.parametrize("dtype", nu.DTYPES, ids=nu.DT_IDS)
@pytest.mark.parametrize("gpus,box", _DOMAINS, ids=_DOMAIN_IDS)
def test_axpbyc_matches_numpy(gpus, box, dtype):
    nu.check_axpbyc_exact("torch", SIZE, gpus, dtype, *(box or ()))


@pytest.mark.parametrize("dtype", nu.DTYPES, ids=nu.DT_IDS)
@pytest.mark.parametrize("gpus", [[0], [0, 0]], ids=["1dom", "2dom"])
def test_cg_update_sum_matches_numpy_and_cg_update(gpus, dtype):
    nu.check_cg_update_sum_exact("torch", SIZE, gpus, dtype)


@pytest.mark.parametrize("dtype", nu.DTYPES, ids=nu.DT_IDS)
def test_global_box_on_two_domains(dtype):
    """a global box is applied as given on EVERY local domain, so it has to
    lie inside both allocations: the two cell layers either side of the
    split, one of them a halo layer on each domain (current after an
    exchange). Each domain then sums the same cells: twice numpy's value."""
    dd, (a, b, c) = cu.vector_domain(SIZE, [dtype] * 3, "torch", [0, 0])
    ga, gb = su.ripple_global(SIZE, dtype), nu.second(SIZE, dtype)
    su.scatter(dd, a, ga)
    su.scatter(dd, b, gb)
    su.scatter(dd, c, np.zeros_like(ga))
    dd.exchange()
    (lo0, hi0), (lo1, _) = dd.local_rect(0), dd.local_rect(1)
    (ax,) = [i for i in range(3) if hi0[i] == lo1[i]]
    lo, hi = list(lo0), list(hi0)
    lo[ax], hi[ax] = hi0[ax] - 1, hi0[ax] + 1
    where, bx = (tuple(lo), tuple(hi)), nu.box_of(lo, hi)
    sa_, sb_ = float(nu.f64(ga[bx]).sum()), float(nu.f64(gb[bx]).sum())
    assert dd.sum(a, where=where) == 2 * sa_
    assert dd.dot_sums(a, b, where=where) == (
        2 * float((nu.f64(ga[bx]) * nu.f64(gb[bx])).sum()), 2 * sa_, 2 * sb_)
    dd.axpbyc(nu.ALPHA, a, nu.BETA, b, nu.C, out=c, where=where)
    want = np.zeros_like(ga)
    want[bx] = (nu.ALPHA * ga + nu.BETA * gb + nu.C).astype(dtype)[bx]
    nu.same_bits(su.gather(dd, c), want)


# ---------------------------------------------------------------- argument checks
def _cg_domain(st, boundary=None, n=4):
    dd, hs = su.make_domain(SIZE, st.radius(), [np.float32] * n, "torch", [0], boundary=boundary)
    return dd, hs


def test_solver_nullspace_value_errors():
    lap = -Stencil.laplacian(2)
    dd, (x, b, r, p) = _cg_domain(lap)
    cg = ConjugateGradient(dd, lap, x, b, r, p, nullspace="constant")  # the valid baseline
    assert cg.nullspace == "constant"
    assert ConjugateGradient(dd, lap, x, b, r, p).nullspace is None
    with pytest.raises(ValueError, match="nullspace"):
        ConjugateGradient(dd, lap, x, b, r, p, nullspace="linear")
    # a face that pins the constant: A is not singular
    for kind in (Boundary.FIXED, Boundary.ANTIMIRROR):
        ddb, (xb, bb, rb, pb) = _cg_domain(lap, boundary={"y-": (kind, 0),
                                                         "y+": (Boundary.MIRROR, 0)})
        ConjugateGradient(ddb, lap, xb, bb, rb, pb)
        with pytest.raises(ValueError, match="nullspace"):
            ConjugateGradient(ddb, lap, xb, bb, rb, pb, nullspace="constant")
    ddm, (xm, bm, rm, pm) = _cg_domain(lap, boundary=boundary_util.all_faces(Boundary.MIRROR, 0))
    ConjugateGradient(ddm, lap, xm, bm, rm, pm, nullspace="constant")
    # a zeroth-order term
    with pytest.raises(ValueError, match="nullspace"):
        ConjugateGradient(dd, 0.5 * Stencil.identity() + lap, x, b, r, p, nullspace="constant")
    # every Laplacian factory passes although its weights are rounded
    for order in (2, 4, 6, 8):
        st = -Stencil.laplacian(order, (0.1, 0.3, 0.7))
        ddo, (xo, bo, ro, po) = _cg_domain(st)
        ConjugateGradient(ddo, st, xo, bo, ro, po, nullspace="constant")
    ddk, (xk, bk, rk, pk, k) = _cg_domain(lap, n=5)
    ConjugateGradient(ddk, DiffusionOperator(ddk, k, 0, sigma=0.0), xk, bk, rk, pk,
                      nullspace="constant")
    with pytest.raises(ValueError, match="sigma"):
        ConjugateGradient(ddk, DiffusionOperator(ddk, k, 0, sigma=0.25), xk, bk, rk, pk,
                          nullspace="constant")


def test_poisson3d_nullspace_value_errors():
    mirror = boundary_util.all_faces(Boundary.MIRROR, 0)
    for kw in (dict(), dict(boundary=mirror), dict(boundary=nu.KINDS["mixed"]),
               dict(boundary=mirror, coefficient=True, preconditioner="jacobi"),
               dict(preconditioner="multigrid")):
        app = Poisson3D((16, 16, 16), sigma=0.0, backend="torch", gpus=[0], nullspace="constant",
                        **kw)
        assert app.xc is not None  # always the true-residual check
    with pytest.raises(ValueError, match="nullspace"):
        Poisson3D(SIZE, sigma=0.0, backend="torch", gpus=[0], nullspace="linear")
    with pytest.raises(ValueError, match="nullspace"):
        Poisson3D(SIZE, sigma=1.0, backend="torch", gpus=[0], nullspace="constant")
    with pytest.raises(ValueError, match="nullspace"):
        Poisson3D(SIZE, sigma=0.0, backend="torch", gpus=[0], nullspace="constant",
                  boundary={"z-": (Boundary.FIXED, 0), "z+": Boundary.MIRROR})
    with pytest.raises(ValueError, match="nullspace"):
        Poisson3D(SIZE, sigma=0.0, backend="torch", gpus=[0], nullspace="constant",
                  boundary=boundary_util.all_faces(Boundary.ANTIMIRROR, 0))
    # the default still refuses the singular problem
    with pytest.raises(ValueError):
        Poisson3D(SIZE, sigma=0.0, backend="torch", gpus=[0])
    assert Poisson3D(SIZE, sigma=1.0, backend="torch", gpus=[0]).xc is None


def test_vector_operation_errors():
    dd, (f, g, i32, d) = cu.vector_domain(
        SIZE, [np.float32, np.float32, np.int32, np.float64], "torch", [0])
    with pytest.raises(ValueError):
        dd.sum(i32)
    with pytest.raises(ValueError):
        dd.dot_sums(f, d)
    with pytest.raises(ValueError):
        dd.axpbyc(1.0, f, 1.0, f, 1.0, out=d)
    with pytest.raises(ValueError):
        dd.axpbyc(1.0, f, 1.0, d, 1.0, out=f)
    with pytest.raises(ValueError):
        dd.cg_update_sum(1.0, f, g, d)
    with pytest.raises(ValueError):
        dd.cg_update_sum(1.0, f, f, g)
    with pytest.raises(ValueError):
        dd.sum(f, where=((-2, 0, 0), (5, 5, 5)))  # outside the radius-1 allocation
    with pytest.raises(ValueError):
        dd.dot_sums(f, where=((0, 0, 0), (SIZE[0] + 2, 5, 5)))
    empty = ((2, 2, 2), (2, 5, 5))
    assert dd.sum(f, where=empty) == 0.0
    assert dd.dot_sums(f, g, where=empty) == (0.0, 0.0, 0.0)


# ------------------------------------------------------------------------ solves
@pytest.mark.parametrize("dtype", nu.DTYPES, ids=nu.DT_IDS)
@pytest.mark.parametrize("case", nu.SOLVE_CASES, ids=nu.solve_id)
def test_singular_solves(case, dtype):
    nu.check_solve("torch", case, dtype)


@pytest.mark.parametrize("case", nu.COEFF_CASES, ids=nu.coeff_id)
def test_singular_solves_with_a_coefficient_jump(case):
    nu.check_coefficient_solve("torch", case)


@pytest.mark.parametrize("dtype", nu.DTYPES, ids=nu.DT_IDS)
def test_constant_rhs_is_a_zero_rhs(dtype):
    nu.check_constant_rhs("torch", dtype, [0, 0])


@pytest.mark.parametrize("n", [16, 32, 64])
@pytest.mark.parametrize("bc", ["periodic", "mirror"])
def test_iterations_do_not_grow_with_the_grid(bc, n):
    want = nu.GRID_ITERATIONS[bc][n]
    res, x, b, app = nu.solve_constant("torch", ((n, n, n), 2, bc, [0], "multigrid"), np.float64)
    print(f"{bc} {n}^3: {res.iterations} iterations, the unprojected arithmetic {want}")
    assert res.converged, res.reason
    assert res.iterations <= want + 2


@pytest.mark.parametrize("dtype", nu.DTYPES, ids=nu.DT_IDS)
def test_nullspace_none_is_the_old_solver(dtype):
    case = cu.SOLVER_CASES[4]
    size, order, sigma, bc, gpus = case
    res0, x0, b, _ = cu.solve_case("torch", case, dtype)
    app = Poisson3D(size, order=order, dtype=dtype, sigma=sigma, backend="torch", gpus=gpus,
                    boundary=cu.kinds_of(bc), nullspace=None)
    app.realize()
    app.set_rhs(b)
    res1 = app.solve(tol=cu.TOL[dtype], max_iter=cu.MAX_ITER)
    assert res0.converged and res1.reason == res0.reason
    assert res1.residuals == res0.residuals
    nu.same_bits(app.solution(), x0)


# ------------------------------------------------------------------ two ranks
def _rank_worker(rank, world, port, q):
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        import torch.distributed as dist

        dist.init_process_group("gloo", rank=rank, world_size=world)
        sys.path.insert(0, os.path.dirname(__file__))
        import nullspace_util

        size = (19, 10, 9)
        app = Poisson3D(size, order=4, dtype=np.float32, sigma=0.0, backend="torch", gpus=[0],
                        boundary=nullspace_util.KINDS["mirror"], nullspace="constant")
        app.realize()
        assert app.dd.comm.world_size == world
        app.set_rhs(nullspace_util.rhs(size, np.float32))
        res = app.solve(tol=1e-5, max_iter=nullspace_util.MAX_ITER)
        sums = (app.dd.sum(app.x), app.dd.sum(app.b), app.dd.dot_sums(app.x, app.r),
                app.dd.dot_sums(app.b))
        dist.destroy_process_group()
        q.put((rank, "ok", res.converged, res.iterations, res.residuals, sums))
    except Exception:  # pragma: no cover
        import traceback

        q.put((rank, traceback.format_exc(), None, None, None, None))


def test_two_ranks_agree_bitwise():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_rank_worker, args=(r, 2, 29643, q)) for r in range(2)]
    for p in procs:
        p.start()
    results = sorted(q.get(timeout=300) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        if p.is_alive():
            p.terminate()
    for rank, status, *_ in results:
        assert status == "ok", f"rank {rank}: {status}"
    (_, _, conv0, it0, res0, sums0), (_, _, conv1, it1, res1, sums1) = results
    assert conv0 and conv1
    assert it0 == it1
    assert res0 == res1  # every entry the identical double
    assert sums0 == sums1
    assert res0[-1] <= 1e-5
    # the sums are global: b = normal + 3 over every rank's cells
    assert abs(sums0[1] / (19 * 10 * 9) - 3.0) < 0.2


# ------------------------------------------------------------------------ CLI
def test_poisson_cg_cli_nullspace():
    out = subprocess.run(
        [sys.executable, os.path.join(REPO, "benchmarks", "poisson_cg.py"), "--backend", "torch",
         "--nullspace", "constant", "--sigma", "0", "--boundary", "mirror", "--size", "16",
         "--iters", "5", "--precond", "mg"],
        capture_output=True, text=True, timeout=300, cwd=REPO,
    )
    assert out.returncode == 0, out.stderr
    rec = json.loads(out.stdout.strip().splitlines()[-1])
    assert rec["benchmark"] == "poisson_cg" and rec["nullspace"] == "constant"
    assert rec["iters"] == 5 and rec["final_residual"] < 1.0
