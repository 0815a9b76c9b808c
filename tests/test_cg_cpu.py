"""Conjugate-gradient solver on the torch backend (CPU tier): the vector
operations of DistributedDomain against numpy, the solver's argument
checks and edge cases, Poisson3D against the boundary-aware truth operator,
rank agreement over gloo and the benchmark CLI."""
import json
import multiprocessing as mp
import os
import subprocess
import sys

import numpy as np
import pytest

import stencil_amd as sa
from stencil_amd import Boundary, Next, Stencil
from stencil_amd.models.poisson3d import Poisson3D
from stencil_amd.solvers import ConjugateGradient

import boundary_util
import cg_util as cu
import stencil_util as su

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE = (19, 10, 9)


def test_is_symmetric():
    for order in (2, 4, 6, 8):
        assert Stencil.laplacian(order, spacing=(1.0, 0.7, 1.3)).is_symmetric()
    assert (Stencil.identity() - 0.1 * Stencil.laplacian(4)).is_symmetric()
    assert not su.upwind().is_symmetric()
    assert not su.exact_star(1).is_symmetric()


# ------------------------------------------------------------ vector operations
@pytest.mark.parametrize("dtype", cu.DTYPES, ids=cu.DT_IDS)
def test_dot_and_axpby_match_numpy_two_domains(dtype):
    dd, (a, b, c) = cu.vector_domain(SIZE, [dtype] * 3, "torch", [0, 0])
    assert dd.num_local() == 2
    ga = su.ripple_global(SIZE, dtype)
    gb = (su.ripple_global(SIZE, dtype)[::-1, ::-1, ::-1] % 97).copy()
    su.scatter(dd, a, ga)
    su.scatter(dd, b, gb)
    su.scatter(dd, b, ga, to_next=True)
    wide = ga.astype(np.float64)
    # integers: every product < 2^20 and the sums < 2^53, exact in fp64
    assert dd.dot(a) == float((wide * wide).sum())
    assert dd.dot(a, b) == float((wide * gb.astype(np.float64)).sum())
    assert dd.dot(a, Next(b)) == float((wide * wide).sum())
    # dyadic coefficients: exact in either type
    dd.axpby(0.5, a, -0.25, b, out=c)
    np.testing.assert_array_equal(su.gather(dd, c), (0.5 * ga - 0.25 * gb).astype(dtype))
    dd.axpby(0.5, a, -0.25, b, out=a)  # out aliases x
    np.testing.assert_array_equal(su.gather(dd, a), (0.5 * ga - 0.25 * gb).astype(dtype))
    dd.axpby(2.0, c, 1.0, Next(b), out=Next(c))  # operands and out in next buffers
    np.testing.assert_array_equal(su.gather(dd, c, from_next=True),
                                  (2.0 * (0.5 * ga - 0.25 * gb) + ga).astype(dtype))


@pytest.mark.parametrize("dtype", cu.DTYPES, ids=cu.DT_IDS)
def test_sub_box(dtype):
    dd, (a, b) = cu.vector_domain(SIZE, [dtype] * 2, "torch", [0])
    ga = su.ripple_global(SIZE, dtype)
    su.scatter(dd, a, ga)
    lo, hi = (3, 1, 1), (9, 8, 8)
    box = (slice(lo[2], hi[2]), slice(lo[1], hi[1]), slice(lo[0], hi[0]))
    sub = ga[box].astype(np.float64)
    assert dd.dot(a, where=(lo, hi)) == float((sub * sub).sum())
    dd.axpby(0.5, a, 0.25, a, out=b, where=(lo, hi))
    want = np.zeros_like(ga)
    want[box] = 0.75 * ga[box]
    np.testing.assert_array_equal(su.gather(dd, b), want)


@pytest.mark.parametrize("dtype", cu.DTYPES, ids=cu.DT_IDS)
def test_axpby_rounds_in_the_quantity_type(dtype):
    dd, (a, b, c) = cu.vector_domain(SIZE, [dtype] * 3, "torch", [0])
    ga, gb = su.normal_global(SIZE, dtype, seed=1), su.normal_global(SIZE, dtype, seed=2)
    su.scatter(dd, a, ga)
    su.scatter(dd, b, gb)
    dd.axpby(1.0 / 3.0, a, -0.7, b, out=c)
    want = dtype(1.0 / 3.0) * ga + dtype(-0.7) * gb
    assert want.dtype == dtype
    np.testing.assert_array_equal(su.gather(dd, c), want)


@pytest.mark.parametrize("dtype", cu.DTYPES, ids=cu.DT_IDS)
def test_cg_update_equals_the_unfused_composition(dtype):
    alpha = 0.37
    gx, gp, gr, gap = (su.normal_global(SIZE, dtype, seed=s) for s in (1, 2, 3, 4))
    outs = []
    for fused in (True, False):
        dd, (x, p, r) = cu.vector_domain(SIZE, [dtype] * 3, "torch", [0, 0])
        su.scatter(dd, x, gx)
        su.scatter(dd, p, gp)
        su.scatter(dd, r, gr)
        su.scatter(dd, p, gap, to_next=True)
        if fused:
            rr = dd.cg_update(alpha, x, p, r)
        else:
            dd.axpby(1.0, x, alpha, p, out=x)
            dd.axpby(1.0, r, -alpha, Next(p), out=r)
            rr = dd.dot(r)
        outs.append((rr, su.gather(dd, x), su.gather(dd, r), su.gather(dd, p),
                     su.gather(dd, p, from_next=True)))
    assert outs[0][0] == outs[1][0]
    for got, want in zip(outs[0][1:], outs[1][1:]):
        np.testing.assert_array_equal(got.view(np.uint8), want.view(np.uint8))
    np.testing.assert_array_equal(outs[0][3], gp)  # p and A p are read only
    np.testing.assert_array_equal(outs[0][4], gap)
    np.testing.assert_array_equal(outs[0][1], gx + dtype(alpha) * gp)


def test_vector_operation_errors():
    dd, (f, i32, d) = cu.vector_domain(SIZE, [np.float32, np.int32, np.float64], "torch", [0])
    with pytest.raises(ValueError):
        dd.dot(i32)
    with pytest.raises(ValueError):
        dd.dot(f, d)
    with pytest.raises(ValueError):
        dd.axpby(1.0, f, 1.0, f, out=d)
    with pytest.raises(ValueError):
        dd.dot(f, where=((-2, 0, 0), (5, 5, 5)))  # outside the radius-1 allocation
    with pytest.raises(ValueError):
        dd.axpby(1.0, f, 1.0, f, out=f, where=((0, 0, 0), (SIZE[0] + 2, 5, 5)))
    with pytest.raises(ValueError):
        dd.cg_update(1.0, f, f, f)
    assert dd.dot(f, where=((2, 2, 2), (2, 5, 5))) == 0.0  # an empty box


# ------------------------------------------------------------ solver arguments
def _cg_domain(dtypes=(np.float32,) * 4, radius=None, boundary=None, st=None):
    st = st if st is not None else Stencil.identity() - Stencil.laplacian(2)
    dd, hs = su.make_domain(SIZE, radius if radius is not None else st.radius(), list(dtypes),
                            "torch", [0], boundary=boundary)
    return dd, hs, st


def test_solver_value_errors():
    dd, (x, b, r, p), st = _cg_domain()
    ConjugateGradient(dd, st, x, b, r, p)  # the valid baseline
    with pytest.raises(ValueError):
        ConjugateGradient(dd, su.upwind(), x, b, r, p)  # not symmetric
    with pytest.raises(ValueError):
        ConjugateGradient(dd, Stencil.identity() - Stencil.laplacian(4), x, b, r, p)  # radius
    dd2, (x2, b2, r2, p2), _ = _cg_domain(
        dtypes=(np.float32, np.float32, np.float64, np.float32))
    with pytest.raises(ValueError):
        ConjugateGradient(dd2, st, x2, b2, r2, p2)  # mixed dtypes
    for kind, value in ((Boundary.OPEN, 0), (Boundary.CLAMP, 0), (Boundary.FIXED, 0.5)):
        ddb, (xb, bb, rb, pb), _ = _cg_domain(boundary={"y-": (kind, value),
                                                        "y+": (Boundary.MIRROR, 0)})
        with pytest.raises(ValueError):
            ConjugateGradient(ddb, st, xb, bb, rb, pb)
    for kind in (Boundary.MIRROR, Boundary.ANTIMIRROR, Boundary.FIXED):
        ddb, (xb, bb, rb, pb), _ = _cg_domain(boundary=boundary_util.all_faces(kind, 0))
        ConjugateGradient(ddb, st, xb, bb, rb, pb)


def test_poisson3d_refuses_singular_problems():
    with pytest.raises(ValueError):
        Poisson3D(SIZE, sigma=0.0, backend="torch", gpus=[0])
    with pytest.raises(ValueError):
        Poisson3D(SIZE, sigma=0.0, backend="torch", gpus=[0],
                  boundary={"z": Boundary.MIRROR})
    Poisson3D(SIZE, sigma=0.0, backend="torch", gpus=[0], boundary={"z-": (Boundary.FIXED, 0),
                                                                   "z+": Boundary.MIRROR})
    app = Poisson3D(SIZE, sigma=1.0, backend="torch", gpus=[0])
    assert app.dd.exchange_groups == [[app.p.index], [app.x.index]]
    assert app.dd.radius.x(1) == 1 and app.dd.radius.dir(1, 1, 0) == 0


@pytest.mark.parametrize("dtype", cu.DTYPES, ids=cu.DT_IDS)
def test_zero_rhs(dtype):
    app = Poisson3D(SIZE, sigma=1.0, dtype=dtype, backend="torch", gpus=[0, 0])
    app.realize()
    app.set_guess(su.ripple_global(SIZE, dtype))  # x's content must not survive
    res = app.solve()
    assert res.converged and res.iterations == 0
    assert (app.solution() == 0).all()


def test_breakdown_is_reported_not_raised():
    """an indefinite operator (-I - laplacian has negative eigenvalues):
    p . A p <= 0 ends the solve without an exception"""
    st = Stencil.laplacian(2) - 0.5 * Stencil.identity()
    dd, (x, b, r, p), _ = _cg_domain(st=st)
    su.scatter(dd, b, np.ones((SIZE[2], SIZE[1], SIZE[0]), dtype=np.float32))
    res = ConjugateGradient(dd, st, x, b, r, p).solve(tol=1e-6, max_iter=20)
    assert not res.converged and res.reason == "breakdown"


# ------------------------------------------------------------------ the solves
@pytest.mark.parametrize("dtype", cu.DTYPES, ids=cu.DT_IDS)
@pytest.mark.parametrize("case", cu.SOLVER_CASES, ids=cu.case_id)
def test_poisson3d_solves(case, dtype):
    res, x, b, app = cu.solve_case("torch", case, dtype)
    cu.check_solution(res, x, b, app, case, dtype, "torch")


def test_nonzero_initial_guess_and_no_overlap():
    case = cu.SOLVER_CASES[2]
    size, order, sigma, bc, gpus = case
    app = Poisson3D(size, order=order, dtype=np.float64, sigma=sigma, backend="torch", gpus=gpus,
                    boundary=cu.kinds_of(bc))
    app.realize()
    b = su.normal_global(size, np.float64)
    app.set_rhs(b)
    app.set_guess(su.normal_global(size, np.float64, seed=7))
    res = app.solve(tol=1e-10, max_iter=cu.MAX_ITER, x0_zero=False, overlap=False)
    assert res.converged and res.residuals[0] > 1.0
    assert cu.true_rel_residual(app.solution(), b, app.stencil, cu.kinds_of(bc)) <= 2e-10


# ------------------------------------------------------------------ two ranks
def _rank_worker(rank, world, port, q):
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        import torch.distributed as dist

        dist.init_process_group("gloo", rank=rank, world_size=world)
        sys.path.insert(0, os.path.dirname(__file__))
        import cg_util
        import stencil_util

        size = (19, 10, 9)
        app = Poisson3D(size, order=4, dtype=np.float32, sigma=0.25, backend="torch", gpus=[0],
                        boundary=cg_util.kinds_of("mirror"))
        app.realize()
        assert app.dd.comm.world_size == world
        app.set_rhs(stencil_util.normal_global(size, np.float32))
        res = app.solve(tol=1e-5, max_iter=cg_util.MAX_ITER)
        dist.destroy_process_group()
        q.put((rank, "ok", res.converged, res.iterations, res.residuals))
    except Exception:  # pragma: no cover
        import traceback

        q.put((rank, traceback.format_exc(), None, None, None))


def test_two_ranks_agree_bitwise():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_rank_worker, args=(r, 2, 29641, q)) for r in range(2)]
    for p in procs:
        p.start()
    results = sorted(q.get(timeout=300) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        if p.is_alive():
            p.terminate()
    for rank, status, *_ in results:
        assert status == "ok", f"rank {rank}: {status}"
    (_, _, conv0, it0, res0), (_, _, conv1, it1, res1) = results
    assert conv0 and conv1
    assert it0 == it1
    assert res0 == res1  # every entry the identical double
    assert res0[-1] <= 1e-5


# ------------------------------------------------------------------------ CLI
def test_poisson_cg_cli():
    out = subprocess.run(
        [sys.executable, os.path.join(REPO, "benchmarks", "poisson_cg.py"), "--backend", "torch",
         "--size", "12", "--iters", "4", "--warmup", "1", "--gpus", "2", "--order", "4",
         "--boundary", "antimirror", "--sigma", "0", "--no-overlap", "--kernels", "1"],
        capture_output=True, text=True, timeout=300, cwd=REPO,
    )
    assert out.returncode == 0, out.stderr
    rec = json.loads(out.stdout.strip().splitlines()[-1])
    assert rec["benchmark"] == "poisson_cg" and rec["iters"] == 4
    for key in ("ms_per_iter", "gcells_per_s", "operator_ms", "dot_ms", "update_ms"):
        assert rec[key] > 0
    assert rec["final_residual"] < 1.0
