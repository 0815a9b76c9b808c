"""Geometric multigrid on the torch backend (CPU tier): axpbypcz and the
grid transfer against numpy, the hierarchy rules and argument checks of
GeometricMultigrid, the V-cycle against the numpy oracle of mg_util.py, its
symmetry, the preconditioned solves, rank agreement over gloo and the
benchmark CLI."""
import json
import math
import multiprocessing as mp
import os
import subprocess
import sys

import numpy as np
import pytest

import stencil_amd as sa
from stencil_amd import Boundary, Next, Stencil
from stencil_amd.models.poisson3d import Poisson3D
from stencil_amd.solvers import ConjugateGradient, GeometricMultigrid, GridTransfer

import boundary_util
import cg_util as cu
import mg_util as mu
import stencil_util as su

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE = (19, 10, 9)


# ------------------------------------------------------------------- axpbypcz
@pytest.mark.parametrize("dtype", cu.DTYPES, ids=cu.DT_IDS)
def test_axpbypcz_matches_numpy_two_domains(dtype):
    dd, (a, b, c, d) = cu.vector_domain(SIZE, [dtype] * 4, "torch", [0, 0])
    ga = su.ripple_global(SIZE, dtype)
    gb = (ga[::-1, ::-1, ::-1] % 97).copy()
    gc = ((ga + 3 * gb) % 211).astype(dtype)
    su.scatter(dd, a, ga)
    su.scatter(dd, b, gb)
    su.scatter(dd, c, gc, to_next=True)
    want = (0.5 * ga - 0.25 * gb + 2.0 * gc).astype(dtype)  # dyadic: exact
    dd.axpbypcz(0.5, a, -0.25, b, 2.0, Next(c), out=d)
    np.testing.assert_array_equal(su.gather(dd, d), want)
    dd.axpbypcz(0.5, a, -0.25, b, 2.0, Next(c), out=a)  # out aliases x
    np.testing.assert_array_equal(su.gather(dd, a), want)
    # a sub-box, on one domain (a box is applied as given on every local domain)
    dd, (d,) = cu.vector_domain(SIZE, [dtype], "torch", [0])
    su.scatter(dd, d, want)
    lo, hi = (3, 1, 1), (9, 8, 8)
    dd.axpbypcz(1.0, d, 1.0, d, 1.0, d, out=Next(d), where=(lo, hi))
    sub = np.zeros_like(want)
    box = (slice(lo[2], hi[2]), slice(lo[1], hi[1]), slice(lo[0], hi[0]))
    sub[box] = 3 * want[box]
    np.testing.assert_array_equal(su.gather(dd, d, from_next=True), sub)


@pytest.mark.parametrize("dtype", cu.DTYPES, ids=cu.DT_IDS)
def test_axpbypcz_rounds_in_the_quantity_type(dtype):
    dd, (a, b, c) = cu.vector_domain(SIZE, [dtype] * 3, "torch", [0])
    ga, gb, gc = (su.normal_global(SIZE, dtype, seed=s) for s in (1, 2, 3))
    for h, g in ((a, ga), (b, gb), (c, gc)):
        su.scatter(dd, h, g)
    dd.axpbypcz(1.0, a, 1.0 / 3.0, b, -0.7, c, out=c)
    want = dtype(1.0) * ga + dtype(1.0 / 3.0) * gb + dtype(-0.7) * gc
    assert want.dtype == dtype
    np.testing.assert_array_equal(su.gather(dd, c), want)


def test_axpbypcz_errors():
    dd, (f, i32, d) = cu.vector_domain(SIZE, [np.float32, np.int32, np.float64], "torch", [0])
    with pytest.raises(ValueError):
        dd.axpbypcz(1.0, f, 1.0, f, 1.0, i32, out=f)
    with pytest.raises(ValueError):
        dd.axpbypcz(1.0, f, 1.0, f, 1.0, f, out=d)
    with pytest.raises(ValueError):
        dd.axpbypcz(1.0, f, 1.0, f, 1.0, f, out=f, where=((-2, 0, 0), (5, 5, 5)))
    dd.axpbypcz(1.0, f, 1.0, f, 1.0, f, out=f, where=((2, 2, 2), (2, 5, 5)))  # empty: a no-op


# -------------------------------------------------------------- grid transfer
def _pair(fsize, dtype, gpus, rf=1, rc=1, nf=3, nc=2):
    fine, fh = cu.vector_domain(fsize, [dtype] * nf, "torch", gpus, radius=rf)
    coarse, ch = cu.vector_domain(tuple(n // 2 for n in fsize), [dtype] * nc, "torch", gpus,
                                  radius=rc)
    return fine, fh, coarse, ch


@pytest.mark.parametrize("dtype", cu.DTYPES, ids=cu.DT_IDS)
@pytest.mark.parametrize("radii", [(1, 1), (2, 1), (1, 2)], ids=str)
def test_transfer_matches_numpy_two_domains(radii, dtype):
    fsize = (32, 12, 10)
    fine, (a, b, d), coarse, (c, s) = _pair(fsize, dtype, [0, 0], *radii)
    assert fine.num_local() == 2
    tr = GridTransfer(fine, coarse)
    shape = (fsize[2], fsize[1], fsize[0])
    ga, gb = mu.int_field(shape, dtype, 1), mu.int_field(shape, dtype, 2)
    su.scatter(fine, a, ga)
    su.scatter(fine, b, gb, to_next=True)
    tr.restrict(2.0, a, -0.5, Next(b), c)
    np.testing.assert_array_equal(su.gather(coarse, c), mu.restrict_mean(2.0 * ga - 0.5 * gb))
    gs = mu.int_field(tuple(n // 2 for n in shape), dtype, 3)
    su.scatter(coarse, s, gs, to_next=True)
    tr.prolong_add(Next(s), a)
    np.testing.assert_array_equal(su.gather(fine, a), ga + mu.prolong(gs))
    np.testing.assert_array_equal(su.gather(fine, b, from_next=True), gb)
    # P = 8 R^T, exactly on integers: <P s, a> = 8 <s, R a>
    lhs = float((mu.prolong(gs).astype(np.float64) * ga).sum())
    rhs = 8.0 * float((gs.astype(np.float64) * mu.restrict_mean(ga.astype(np.float64))).sum())
    assert lhs == rhs


def test_transfer_value_errors():
    f32, f64 = np.float32, np.float64
    fine, (a, b, d), coarse, (c, s) = _pair((32, 12, 10), f32, [0, 0])
    other, _ = cu.vector_domain((16, 6, 6), [f32], "torch", [0, 0])  # not the half
    with pytest.raises(ValueError):
        GridTransfer(fine, other)
    one, _ = cu.vector_domain((16, 6, 5), [f32], "torch", [0])  # another partition
    with pytest.raises(ValueError):
        GridTransfer(fine, one)
    odd_f, _ = cu.vector_domain((36, 12, 10), [f32], "torch", [0, 0])  # subdomains 18 = 2 x 9,
    odd_c, _ = cu.vector_domain((18, 6, 5), [f32], "torch", [0, 0])  # halves at 9, fine
    GridTransfer(odd_f, odd_c)
    mixed, (m,) = cu.vector_domain((16, 6, 5), [f64], "torch", [0, 0])
    tr = GridTransfer(fine, mixed)
    with pytest.raises(ValueError):
        tr.restrict(1.0, a, 1.0, b, m)
    with pytest.raises(ValueError):
        tr.prolong_add(m, a)
    # below GridTransfer: the backend's own checks
    be_f, be_c = fine.backend, coarse.backend
    lo, hi = coarse.local_rect(0)
    with pytest.raises(ValueError):  # the doubled box leaves the fine allocation
        be_c.grid_restrict(be_f, 0, 1.0, 0, False, 1.0, 1, False, 0, 0, False,
                           lo, (hi[0] + 1, hi[1], hi[2]))
    with pytest.raises(ValueError):  # outside the coarse allocation
        be_c.grid_restrict(be_f, 0, 1.0, 0, False, 1.0, 1, False, 0, 0, False,
                           (lo[0] - 2, lo[1], lo[2]), hi)
    with pytest.raises(ValueError):
        be_c.grid_restrict(be_f, 0, 1.0, 0, False, 1.0, 7, False, 0, 0, False, lo, hi)
    with pytest.raises(ValueError):
        be_f.grid_prolong_add(be_c, 5, 0, False, 0, 0, False, lo, hi)
    be_f.grid_prolong_add(be_c, 0, 0, False, 0, 0, False, lo, lo)  # empty: a no-op


# ------------------------------------------------------------ hierarchy rules
def _mg_domain(size, gpus, dtype=np.float32, boundary=None, st=None, radius=None, nq=2):
    st = st if st is not None else Stencil.identity() - Stencil.laplacian(2)
    dd, hs = su.make_domain(size, radius if radius is not None else st.radius(), [dtype] * nq,
                            "torch", gpus, boundary=boundary)
    return dd, hs, st


def _helmholtz(level):
    return Stencil.identity() - Stencil.laplacian(2, (2.0 ** level,) * 3)


def test_hierarchy_rules():
    dd, (e, f), _ = _mg_domain((32, 16, 16), [0, 0])
    mg = GeometricMultigrid(dd, _helmholtz, e, 0)
    assert mg.levels == [(32, 16, 16), (16, 8, 8), (8, 4, 4), (4, 2, 2)]
    assert [lv.dd.local_rect(1)[0][0] for lv in mg._levels] == [16, 8, 4, 2]
    dd, (e, f), _ = _mg_domain((24, 16, 16), [0])
    mg = GeometricMultigrid(dd, _helmholtz, e, 0)
    assert mg.levels[-1] == (3, 2, 2) and len(mg.levels) == 4
    dd, (e, f), _ = _mg_domain((20, 12, 12), [0, 0])
    assert GeometricMultigrid(dd, _helmholtz, e, 0).levels == [(20, 12, 12), (10, 6, 6)]
    dd, (e, f), _ = _mg_domain((18, 8, 8), [0, 0])  # subdomains of 9 cells
    with pytest.raises(ValueError):
        GeometricMultigrid(dd, _helmholtz, e, 0)
    dd, (e, f), _ = _mg_domain((32, 16, 16), [0])
    assert len(GeometricMultigrid(dd, _helmholtz, e, 0, max_levels=3).levels) == 3
    assert len(GeometricMultigrid(dd, _helmholtz, e, 0, max_levels=2).levels) == 2
    with pytest.raises(ValueError):
        GeometricMultigrid(dd, _helmholtz, e, 0, max_levels=1)


def test_coarse_levels_mirror_the_fine_domain():
    bc = {"x-": (Boundary.FIXED, 0), "x+": (Boundary.MIRROR, 0),
          "y-": (Boundary.ANTIMIRROR, 0), "y+": (Boundary.ANTIMIRROR, 0)}
    dd, (e, f), _ = _mg_domain((16, 16, 8), [0, 0], dtype=np.float64, boundary=bc)
    mg = GeometricMultigrid(dd, _helmholtz, e, 0)
    for lv in mg._levels[1:]:
        c = lv.dd
        assert c.backend_kind == "torch" and c.gpus == [0, 0] and c.strategy == dd.strategy
        assert [h.dtype for h in (lv.e, lv.f)] == [np.dtype(np.float64)] * 2
        assert c.exchange_groups == [[lv.e.index]]
        assert c.radius.x(1) == 1 and c.radius.dir(1, 1, 0) == 0
        assert c.boundary.periodic == (False, False, True)
        for q in (lv.e.index, lv.f.index):
            assert c.boundary.kind(q, 0, 0) == Boundary.FIXED
            assert c.boundary.kind(q, 0, 1) == Boundary.MIRROR
            assert c.boundary.kind(q, 1, 1) == Boundary.ANTIMIRROR


def test_multigrid_value_errors():
    dd, (e, f), st = _mg_domain((16, 16, 16), [0])
    GeometricMultigrid(dd, _helmholtz, e, 0)  # the valid baseline
    for kw in ({"omega": 0.0}, {"omega": 1.0}, {"omega": -0.5}, {"nu": 0}, {"coarse_sweeps": 0},
               {"nu": 1.5}):
        with pytest.raises(ValueError):
            GeometricMultigrid(dd, _helmholtz, e, 0, **kw)
    with pytest.raises(ValueError):
        GeometricMultigrid(dd, lambda l: su.upwind(), e, 0)  # not symmetric
    with pytest.raises(ValueError):  # not symmetric below level 0
        GeometricMultigrid(dd, lambda l: _helmholtz(0) if l == 0 else su.upwind_x(), e, 0)
    with pytest.raises(ValueError):  # the radius does not cover order 4
        GeometricMultigrid(dd, lambda l: Stencil.identity() - Stencil.laplacian(4), e, 0)
    with pytest.raises(ValueError):  # a centre weight that is not positive
        GeometricMultigrid(dd, lambda l: Stencil.laplacian(2), e, 0)
    dd3 = sa.DistributedDomain(16, 16, 16, backend="torch")
    dd3.set_radius(st.radius())
    dd3.set_gpus([0])
    e3, f3 = dd3.add_data(np.float32, "e"), dd3.add_data(np.float32, "f")
    dd3.set_exchange_groups([[f3.index]])
    with pytest.raises(ValueError):
        GeometricMultigrid(dd3, _helmholtz, e3, 0)  # not realized
    dd3.realize()
    with pytest.raises(ValueError):
        GeometricMultigrid(dd3, _helmholtz, e3, 0)  # e is not in group 0
    ddi, (ei, fi), _ = _mg_domain((16, 16, 16), [0], dtype=np.int32)
    with pytest.raises(ValueError):
        GeometricMultigrid(ddi, _helmholtz, ei, 0)
    for kind, value in ((Boundary.OPEN, 0), (Boundary.CLAMP, 0), (Boundary.FIXED, 0.5)):
        ddb, (eb, fb), _ = _mg_domain((16, 16, 16), [0], boundary={
            "y-": (kind, value), "y+": (Boundary.MIRROR, 0)})
        with pytest.raises(ValueError):
            GeometricMultigrid(ddb, _helmholtz, eb, 0)
    mg = GeometricMultigrid(dd, _helmholtz, e, 0)
    with pytest.raises(ValueError):
        mg.apply(e, f)  # the cycle writes e, not f
    with pytest.raises(ValueError):
        mg.apply(e, e)


def test_solver_preconditioner_value_errors():
    dd, (x, b, r, p, z), st = _mg_domain((16, 16, 16), [0], nq=5)
    mg = GeometricMultigrid(dd, _helmholtz, z, 0)
    ConjugateGradient(dd, st, x, b, r, p, preconditioner=mg, z=z)
    with pytest.raises(ValueError):
        ConjugateGradient(dd, st, x, b, r, p, preconditioner=mg)  # no z
    with pytest.raises(ValueError):
        ConjugateGradient(dd, st, x, b, r, p, preconditioner=mg, z=r)  # not distinct
    with pytest.raises(ValueError):
        ConjugateGradient(dd, st, x, b, r, p, preconditioner=object(), z=z)  # no apply
    with pytest.raises(ValueError):
        ConjugateGradient(dd, st, x, b, r, p, z=z)  # z without a preconditioner
    with pytest.raises(ValueError):
        Poisson3D((16, 16, 16), sigma=1.0, backend="torch", gpus=[0], preconditioner="ilu")
    app = Poisson3D((16, 16, 16), sigma=1.0, backend="torch", gpus=[0],
                    preconditioner="multigrid", mg={"nu": 1, "max_levels": 2})
    assert app.dd.exchange_groups == [[app.p.index], [app.x.index], [app.z.index]]
    app.realize()
    assert app.mg.nu == 1 and len(app.mg.levels) == 2


# ------------------------------------------------------------------ the cycle
@pytest.mark.parametrize("dtype", cu.DTYPES, ids=cu.DT_IDS)
@pytest.mark.parametrize("case", mu.MG_CASES, ids=cu.case_id)
def test_cycle_against_the_oracle(case, dtype):
    app = mu.check_cycle("torch", case, dtype)
    assert all(t > 0 for t in app.mg.phase_times.values())
    assert sorted(app.mg.phase_times) == [f"level{l}" for l in range(len(app.mg.levels))]


@pytest.mark.parametrize("case", [mu.MG_CASES[1], mu.MG_CASES[2]], ids=cu.case_id)
def test_cycle_is_symmetric_positive_definite(case):
    size, order, sigma, bc, gpus = case
    app = Poisson3D(size, order=order, dtype=np.float64, sigma=sigma, backend="torch", gpus=gpus,
                    boundary=cu.kinds_of(bc), preconditioner="multigrid")
    app.realize()
    u, v = su.normal_global(size, np.float64, seed=5), su.normal_global(size, np.float64, seed=6)
    out = []
    for g in (u, v):
        su.scatter(app.dd, app.r, g)
        app.mg.apply(app.r, app.z)
        out.append(su.gather(app.dd, app.z).astype(np.longdouble))
    mu_, mv = out
    asym = abs(float((u * mv).sum() - (v * mu_).sum()))
    bound = 1e-10 * float(cu.norm2(u)) * float(cu.norm2(mv))
    print(f"|u.Mv - v.Mu| = {asym:.3e} (bound {bound:.3e}), u.Mu = {float((u * mu_).sum()):.3e}")
    assert asym <= bound
    assert float((u * mu_).sum()) > 0 and float((v * mv).sum()) > 0


# ----------------------------------------------------------------- the solves
@pytest.mark.parametrize("dtype", cu.DTYPES, ids=cu.DT_IDS)
@pytest.mark.parametrize("case", mu.MG_CASES, ids=cu.case_id)
def test_preconditioned_solves(case, dtype):
    mu.check_mg_solve("torch", case, dtype)


def _parent_solve(app, tol, max_iter):
    """the unpreconditioned loop of solve(x0_zero=True, overlap=True),
    spelled out on the public vector operations"""
    dd, x, b, r, p = app.dd, app.x, app.b, app.r, app.p
    bb = dd.dot(b)
    dd.axpby(0.0, b, 0.0, b, out=x)
    dd.axpby(1.0, b, 0.0, b, out=r)
    dd.axpby(1.0, r, 0.0, r, out=p)
    rr = dd.dot(r)
    residuals = [math.sqrt(rr / bb)]
    for _ in range(max_iter):
        dd.apply_stencil(app.stencil, p, where="interior")
        dd.exchange(0)
        dd.apply_stencil(app.stencil, p, where="exterior")
        alpha = rr / dd.dot(p, Next(p))
        rr_new = dd.cg_update(alpha, x, p, r)
        residuals.append(math.sqrt(rr_new / bb))
        if rr_new <= tol * tol * bb:
            break
        dd.axpby(1.0, r, rr_new / rr, p, out=p)
        rr = rr_new
    return residuals


def test_no_preconditioner_is_the_unchanged_solver():
    case = cu.SOLVER_CASES[4]
    size, order, sigma, bc, gpus = case
    runs = []
    for kwargs in ({}, {"preconditioner": None}):
        app = Poisson3D(size, order=order, dtype=np.float32, sigma=sigma, backend="torch",
                        gpus=gpus, boundary=cu.kinds_of(bc), **kwargs)
        app.realize()
        app.set_rhs(su.normal_global(size, np.float32))
        runs.append(app)
    res = runs[0].solve(tol=1e-5, max_iter=cu.MAX_ITER)
    assert res.converged and sorted(runs[0].cg.phase_times) == ["dot", "operator", "update"]
    assert runs[0].z is None and len(runs[0].dd._data) == 4
    assert res.residuals == _parent_solve(runs[1], 1e-5, cu.MAX_ITER)  # the identical doubles
    cg = runs[1].cg
    explicit = ConjugateGradient(runs[1].dd, runs[1].stencil, cg.x, cg.b, cg.r, cg.p, group_p=0,
                                 group_x=1, preconditioner=None, z=None)
    assert explicit.solve(tol=1e-5, max_iter=cu.MAX_ITER).residuals == res.residuals


class _Negated:
    """z = -r: a preconditioner that is not positive definite"""

    def __init__(self, dd):
        self.dd = dd

    def apply(self, r, z):
        self.dd.axpby(-1.0, r, 0.0, r, out=z)


class _NotANumber(_Negated):
    def apply(self, r, z):
        self.dd.axpby(float("nan"), r, 0.0, r, out=z)


@pytest.mark.parametrize("bad", [_Negated, _NotANumber], ids=["negative", "nan"])
def test_preconditioner_breakdown_is_reported_not_raised(bad):
    dd, (x, b, r, p, z), st = _mg_domain(SIZE, [0], nq=5)
    su.scatter(dd, b, su.normal_global(SIZE, np.float32))
    cg = ConjugateGradient(dd, st, x, b, r, p, preconditioner=bad(dd), z=z)
    res = cg.solve(tol=1e-6, max_iter=20)
    assert not res.converged and res.reason == "breakdown" and res.iterations == 0
    assert "precond" in cg.phase_times


def test_nonzero_initial_guess_and_no_overlap():
    case = mu.MG_CASES[2]
    size, order, sigma, bc, gpus = case
    app = Poisson3D(size, order=order, dtype=np.float64, sigma=sigma, backend="torch", gpus=gpus,
                    boundary=cu.kinds_of(bc), preconditioner="multigrid")
    app.realize()
    b = su.normal_global(size, np.float64)
    app.set_rhs(b)
    app.set_guess(su.normal_global(size, np.float64, seed=7))
    res = app.solve(tol=1e-10, max_iter=cu.MAX_ITER, x0_zero=False, overlap=False)
    assert res.converged and res.residuals[0] > 1.0
    assert res.iterations <= mu.oracle_iterations(case, np.float64) + 4  # a rougher start
    assert app.cg.phase_times["precond"] > 0
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

        size = (32, 16, 16)
        app = Poisson3D(size, order=2, dtype=np.float32, sigma=0.01, backend="torch", gpus=[0],
                        boundary=cg_util.kinds_of("mirror"), preconditioner="multigrid")
        app.realize()
        assert app.dd.comm.world_size == world
        app.set_rhs(stencil_util.normal_global(size, np.float32))
        res = app.solve(tol=1e-5, max_iter=cg_util.MAX_ITER)
        levels = app.mg.levels
        dist.destroy_process_group()
        q.put((rank, "ok", res.converged, res.iterations, res.residuals, levels))
    except Exception:  # pragma: no cover
        import traceback

        q.put((rank, traceback.format_exc(), None, None, None, None))


def test_two_ranks_agree_bitwise():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_rank_worker, args=(r, 2, 29653, q)) for r in range(2)]
    for p in procs:
        p.start()
    results = sorted(q.get(timeout=300) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        if p.is_alive():
            p.terminate()
    for rank, status, *_ in results:
        assert status == "ok", f"rank {rank}: {status}"
    (_, _, conv0, it0, res0, lv0), (_, _, conv1, it1, res1, lv1) = results
    assert conv0 and conv1
    assert it0 == it1 and lv0 == lv1 and len(lv0) == 4
    assert res0 == res1  # every entry the identical double
    assert res0[-1] <= 1e-5 and it0 <= 20


# ------------------------------------------------------------------------ CLI
def _cli(*extra):
    out = subprocess.run(
        [sys.executable, os.path.join(REPO, "benchmarks", "poisson_cg.py"), "--backend", "torch",
         "--size", "16", "--warmup", "1", "--gpus", "2", "--boundary", "antimirror",
         "--sigma", "0", *extra],
        capture_output=True, text=True, timeout=300, cwd=REPO,
    )
    assert out.returncode == 0, out.stderr
    return json.loads(out.stdout.strip().splitlines()[-1])


def test_poisson_cg_cli_multigrid():
    fixed = _cli("--precond", "mg", "--iters", "3", "--kernels", "1")
    assert fixed["precond"] == "mg" and fixed["iters"] == 3 and fixed["precond_ms"] > 0
    assert "converged" not in fixed
    for name in ("axpbypcz", "grid_restrict", "grid_prolong_add"):
        assert fixed[f"{name}_kernel_ms"] > 0 and fixed[f"{name}_gb_per_s"] > 0
    mg = _cli("--precond", "mg", "--tol", "1e-5", "--iters", "200")
    plain = _cli("--precond", "none", "--tol", "1e-5", "--iters", "200")
    for rec in (mg, plain):
        assert rec["converged"] and rec["iterations"] == rec["iters"] and rec["solve_ms"] > 0
        assert rec["final_residual"] <= 1e-5
    assert mg["levels"] == [[16, 16, 16], [8, 8, 8], [4, 4, 4]] and plain["levels"] is None
    assert 0 < mg["coarse_share"] < 1
    assert 2 * mg["iterations"] <= plain["iterations"]
