"""BiCGStab on the torch backend (CPU tier): Stencil.advection and
symmetric_part, the three fused vector operations of DistributedDomain
against numpy on exact data, the solver's argument checks and edge cases,
AdvectionDiffusion3D against the boundary-aware truth operator, the
multigrid preconditioner, rank agreement over gloo and the benchmark CLI."""
import json
import multiprocessing as mp
import os
import subprocess
import sys

import numpy as np
import pytest

import stencil_amd as sa
from stencil_amd import Boundary, Next, Stencil
from stencil_amd.models.advection_diffusion3d import AdvectionDiffusion3D
from stencil_amd.solvers import BiCGStab, CGResult, DiffusionOperator

import bicgstab_util as bu
import boundary_util
import cg_util as cu
import stencil_util as su

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE = (19, 10, 9)


def _taps(st):
    return dict(zip(st.offsets, st.weights))


def _unit(axis, k):
    o = [0, 0, 0]
    o[axis] = k
    return tuple(o)


# ------------------------------------------------------------ Stencil.advection
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_advection_taps(axis):
    h = (0.5, 2.0, 0.25)
    for v in (1.5, -0.75):
        vel = [0.0, 0.0, 0.0]
        vel[axis] = v
        up = _taps(Stencil.advection(vel, spacing=h))
        w = v / h[axis]
        if v > 0:
            assert up == {_unit(axis, 0): w, _unit(axis, -1): -w}
        else:
            assert up == {_unit(axis, 1): w, _unit(axis, 0): -w}
        ce = _taps(Stencil.advection(vel, spacing=h, scheme="central"))
        assert ce == {_unit(axis, 1): w / 2, _unit(axis, -1): -w / 2}
    # all three axes at once: the centre taps merge
    st = _taps(Stencil.advection((1.0, -2.0, 0.5)))
    assert st == {(0, 0, 0): 1.0 + 2.0 + 0.5, (-1, 0, 0): -1.0, (0, 1, 0): -2.0, (0, 0, -1): -0.5}


def test_advection_radius_and_symmetry():
    st = Stencil.advection((1, 0, 0))
    r = st.radius()
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if (dx, dy, dz) != (0, 0, 0):
                    assert r.dir(dx, dy, dz) == (1 if (dx, dy, dz) == (-1, 0, 0) else 0)
    assert not st.is_symmetric()
    assert not Stencil.advection((1, 0.5, -0.25), scheme="central").is_symmetric()


def test_advection_value_errors():
    for vel in ((0, 0, 0), (float("nan"), 1, 0), (1, float("inf"), 0), (1, 2)):
        with pytest.raises(ValueError):
            Stencil.advection(vel)
    with pytest.raises(ValueError):
        Stencil.advection((1, 0, 0), scheme="quick")
    with pytest.raises(ValueError):
        Stencil.advection((1, 0, 0), spacing=(1, 0, 1))


@pytest.mark.parametrize("scheme", ["upwind", "central"])
def test_advection_of_a_linear_field_is_v_dot_grad(scheme):
    """u = g . p with integer g on integer cells, dyadic v and h: every tap
    product and sum is exact, so away from the periodic seam the result is
    v . g / h per axis, bitwise"""
    vel, h, g = (1.5, -0.5, 0.25), (0.5, 2.0, 1.0), (3.0, -2.0, 5.0)
    st = Stencil.advection(vel, spacing=h, scheme=scheme)
    z, y, x = np.meshgrid(np.arange(9.0), np.arange(10.0), np.arange(19.0), indexing="ij")
    u = g[0] * x + g[1] * y + g[2] * z
    got, _ = su.roll_sum(u, st)
    want = sum(vel[a] * g[a] / h[a] for a in range(3))
    inner = got[1:-1, 1:-1, 1:-1]
    assert (inner == want).all()


def test_symmetric_part_of_upwind_is_its_numerical_diffusion():
    vel, h = (1.5, -0.5, 0.25), (0.5, 2.0, 1.0)
    sym = Stencil.advection(vel, spacing=h).symmetric_part()
    assert sym.is_symmetric()
    # -(|v_a| h_a / 2) * (u_{i-1} - 2 u_i + u_{i+1}) / h_a^2 per axis
    want = Stencil.star(*[[-abs(v) / (2 * ha), abs(v) / ha, -abs(v) / (2 * ha)]
                          for v, ha in zip(vel, h)])
    assert _taps(sym) == _taps(want)
    lap = Stencil.identity() - 0.5 * Stencil.laplacian(4)
    assert lap.symmetric_part() == lap
    with pytest.raises(ValueError):  # a skew stencil has no symmetric part
        Stencil.advection(vel, scheme="central").symmetric_part()


# ------------------------------------------------------------ the three ops
@pytest.mark.parametrize("dtype", bu.DTYPES, ids=bu.DT_IDS)
@pytest.mark.parametrize("box,gpus", [("all", [0, 0]), ("box", [0])], ids=["all-2dom", "box-1dom"])
def test_ops_match_numpy_bitwise(box, gpus, dtype):
    lo, hi = ((0, 0, 0), SIZE) if box == "all" else ((3, 1, 1), (12, 8, 8))
    bu.run_ops_exact("torch", SIZE, lo, hi, dtype, gpus)


@pytest.mark.parametrize("dtype", bu.DTYPES, ids=bu.DT_IDS)
def test_ops_round_in_the_quantity_type(dtype):
    """non-dyadic scalars on normal data: the torch backend rounds alpha,
    beta and omega once and computes in the quantity's type"""
    dd, (a, b, c, d) = cu.vector_domain(SIZE, [dtype] * 4, "torch", [0, 0])
    ga, gb, gc, gd = (su.normal_global(SIZE, dtype, seed=s) for s in (1, 2, 3, 4))
    for h, g in zip((a, b, c, d), (ga, gb, gc, gd)):
        su.scatter(dd, h, g)
    su.scatter(dd, d, ga, to_next=True)
    al, om = dtype(1.0 / 3.0), dtype(-0.7)
    nn = dd.axpby_norm2(1.0 / 3.0, a, -0.7, b, out=Next(c))
    want = al * ga + om * gb
    np.testing.assert_array_equal(su.gather(dd, c, from_next=True), want)
    assert nn == pytest.approx(float((want.astype(np.float64) ** 2).sum()), rel=1e-12)
    rr, rho = dd.bicgstab_update(1.0 / 3.0, a, -0.7, d, c, d, Next(d), b)  # z is r
    rn = gd - om * ga
    np.testing.assert_array_equal(su.gather(dd, d), rn)
    np.testing.assert_array_equal(su.gather(dd, c), gc + al * ga + om * gd)
    assert rr == pytest.approx(float((rn.astype(np.float64) ** 2).sum()), rel=1e-12)
    assert rho == pytest.approx(float((gb.astype(np.float64) * rn).sum()), rel=1e-9, abs=1e-9)


def test_ops_refuse():
    dd, (f, g, e, h, i32, d) = cu.vector_domain(
        SIZE, [np.float32] * 4 + [np.int32, np.float64], "torch", [0])
    with pytest.raises(ValueError):
        dd.axpby_norm2(1.0, f, 1.0, d, out=g)  # mixed types
    with pytest.raises(ValueError):
        dd.axpby_norm2(1.0, f, 1.0, g, out=i32)
    with pytest.raises(ValueError):
        dd.dot_pair(f, d)
    with pytest.raises(ValueError):
        dd.dot_pair(i32, i32)
    with pytest.raises(TypeError):
        dd.dot_pair(f, 3.0)
    with pytest.raises(ValueError):
        dd.dot_pair(f, g, where=((-2, 0, 0), (5, 5, 5)))  # outside the radius-1 allocation
    with pytest.raises(ValueError):
        dd.axpby_norm2(1.0, f, 1.0, g, out=e, where=((0, 0, 0), (SIZE[0] + 2, 5, 5)))
    # bicgstab_update(alpha, y, omega, z, x, r, t, rhat)
    with pytest.raises(TypeError):
        dd.bicgstab_update(1.0, f, 1.0, g, Next(e), h, Next(g), f)  # x is a handle
    with pytest.raises(TypeError):
        dd.bicgstab_update(1.0, f, 1.0, g, e, Next(h), Next(g), f)  # r is a handle
    with pytest.raises(ValueError):
        dd.bicgstab_update(1.0, f, 1.0, g, e, e, Next(g), f)  # x is r
    with pytest.raises(ValueError):
        dd.bicgstab_update(1.0, e, 1.0, g, e, h, Next(g), f)  # y is x
    with pytest.raises(ValueError):
        dd.bicgstab_update(1.0, f, 1.0, g, e, h, h, f)  # t is r
    with pytest.raises(ValueError):
        dd.bicgstab_update(1.0, f, 1.0, g, e, h, Next(g), e)  # rhat is x
    with pytest.raises(ValueError):
        dd.bicgstab_update(1.0, f, 1.0, g, e, h, Next(g), d)  # mixed types
    # the next buffers of x and r are other buffers: accepted
    dd.bicgstab_update(1.0, Next(e), 1.0, h, e, h, Next(h), Next(e))
    assert dd.dot_pair(f, g, where=((2, 2, 2), (2, 5, 5))) == (0.0, 0.0)  # an empty box
    assert dd.axpby_norm2(1.0, f, 1.0, g, out=e, where=((2, 2, 2), (2, 5, 5))) == 0.0


# ------------------------------------------------------------ solver arguments
def _domain(dtypes=(np.float32,) * 5, radius=None, boundary=None, st=None, groups=None):
    st = st if st is not None else Stencil.identity() + Stencil.advection((1, 0.5, -0.25)) \
        - 0.5 * Stencil.laplacian(2)
    dd = sa.DistributedDomain(*SIZE, backend="torch")
    dd.set_radius(radius if radius is not None else st.radius())
    dd.set_gpus([0])
    hs = [dd.add_data(dt, f"q{i}") for i, dt in enumerate(dtypes)]
    # x, b, r, rhat, p (, y, z): p, r and x in a group each, or y, z and x
    if groups is None:
        groups = [[hs[4].index], [hs[2].index], [hs[0].index]] if len(hs) == 5 else \
            [[hs[5].index], [hs[6].index], [hs[0].index]]
    dd.set_exchange_groups(groups)
    if boundary:
        for face, (kind, value) in boundary.items():
            dd.set_boundary(face, kind, value)
    dd.realize()
    return dd, hs, st


class _Identity:
    def __init__(self, dd):
        self.dd = dd

    def apply(self, f, e):
        self.dd.axpby(1.0, f, 0.0, f, out=e)


def test_solver_value_errors():
    dd, (x, b, r, rhat, p), st = _domain()
    BiCGStab(dd, st, x, b, r, rhat, p, 0, 1, 2)  # the valid baseline
    BiCGStab(dd, st, x, b, r, rhat, p, 0, 1)  # no group_x: no verify step
    with pytest.raises(ValueError):
        BiCGStab(dd, st - 0.1 * Stencil.laplacian(4), x, b, r, rhat, p, 0, 1, 2)  # radius
    with pytest.raises(ValueError):
        BiCGStab(dd, st, x, b, r, r, p, 0, 1, 2)  # not distinct
    with pytest.raises(ValueError):
        BiCGStab(dd, st, x, b, r, rhat, p, 1, 1, 2)  # p is not in group 1
    with pytest.raises(ValueError):
        BiCGStab(dd, st, x, b, r, rhat, p, 0, 1, 2, preconditioner=_Identity(dd))  # no y, z
    with pytest.raises(ValueError):
        BiCGStab(dd, st, x, b, r, rhat, p, 0, 1, 2, y=rhat)  # y without a preconditioner
    dd2, hs2, _ = _domain(dtypes=(np.float32, np.float32, np.float64, np.float32, np.float32))
    with pytest.raises(ValueError):
        BiCGStab(dd2, st, *hs2, 0, 1, 2)  # mixed dtypes
    for kind, value in ((Boundary.OPEN, 0), (Boundary.FIXED, 0.5)):
        ddb, hsb, _ = _domain(boundary={"y-": (kind, value), "y+": (Boundary.MIRROR, 0)})
        with pytest.raises(ValueError):
            BiCGStab(ddb, st, *hsb, 0, 1, 2)
    for kind in (Boundary.MIRROR, Boundary.ANTIMIRROR, Boundary.FIXED, Boundary.CLAMP):
        ddb, hsb, _ = _domain(boundary=boundary_util.all_faces(kind, 0))
        BiCGStab(ddb, st, *hsb, 0, 1, 2)
    # a DiffusionOperator is out of scope
    dd3, hs3, _ = _domain(dtypes=(np.float32,) * 6, radius=sa.Radius.constant(1),
                          groups=[[4], [2], [0], [5]])
    op = DiffusionOperator(dd3, hs3[5], 3)
    with pytest.raises(ValueError):
        BiCGStab(dd3, op, *hs3[:5], 0, 1, 2)
    # preconditioners: one without apply, and the complete call
    dd4, hs4, _ = _domain(dtypes=(np.float32,) * 7)
    with pytest.raises(ValueError):
        BiCGStab(dd4, st, *hs4[:5], 0, 1, 2, preconditioner=object(), y=hs4[5], z=hs4[6])
    with pytest.raises(ValueError):
        BiCGStab(dd4, st, *hs4[:5], 0, 1, 2, preconditioner=_Identity(dd4), y=hs4[5], z=hs4[5])
    BiCGStab(dd4, st, *hs4[:5], 0, 1, 2, preconditioner=_Identity(dd4), y=hs4[5], z=hs4[6])


def test_model_value_errors():
    kw = dict(backend="torch", gpus=[0])
    with pytest.raises(ValueError):
        AdvectionDiffusion3D(SIZE, (1, 0, 0), nu=1.0, sigma=-1.0, **kw)
    with pytest.raises(ValueError):
        AdvectionDiffusion3D(SIZE, (1, 0, 0), nu=-1.0, sigma=1.0, **kw)
    with pytest.raises(ValueError):
        AdvectionDiffusion3D(SIZE, (1, 0, 0), nu=1.0, sigma=0.0, **kw)  # periodic: singular
    with pytest.raises(ValueError):
        AdvectionDiffusion3D(SIZE, (1, 0, 0), nu=1.0, sigma=0.0,
                             boundary={"x": Boundary.CLAMP, "z": Boundary.MIRROR}, **kw)
    with pytest.raises(ValueError):
        AdvectionDiffusion3D(SIZE, (1, 0, 0), nu=0.0, sigma=1.0, scheme="central", **kw)
    with pytest.raises(ValueError):
        AdvectionDiffusion3D((16, 16, 16), (1, 0, 0), nu=1.0, sigma=1.0,
                             boundary={"x": Boundary.CLAMP}, preconditioner="multigrid", **kw)
    AdvectionDiffusion3D(SIZE, (1, 0, 0), nu=1.0, sigma=0.0,
                         boundary={"z-": (Boundary.FIXED, 0), "z+": Boundary.CLAMP}, **kw)
    app = AdvectionDiffusion3D(SIZE, (1, 0.5, -0.25), nu=0.0, sigma=1.0, **kw)
    assert app.dd.exchange_groups == [[app.p.index], [app.r.index], [app.x.index]]
    r = app.dd.radius  # pure upwind: no downwind halo
    assert (r.x(-1), r.x(1), r.y(-1), r.y(1), r.z(-1), r.z(1)) == (1, 0, 1, 0, 0, 1)


@pytest.mark.parametrize("dtype", bu.DTYPES, ids=bu.DT_IDS)
def test_zero_rhs(dtype):
    app = AdvectionDiffusion3D(SIZE, (1, 0.5, -0.25), nu=0.5, sigma=1.0, dtype=dtype,
                               backend="torch", gpus=[0, 0])
    app.realize()
    app.set_guess(su.ripple_global(SIZE, dtype))  # x's content must not survive
    res = app.solve()
    assert isinstance(res, CGResult)
    assert res.converged and res.iterations == 0 and res.reason == "zero_rhs"
    assert (app.solution() == 0).all()


def test_breakdown_is_reported_not_raised():
    """A = the periodic shift, b a single 1: v = A rhat is b shifted, so
    rhat . v == 0 exactly"""
    st = Stencil([(1, 0, 0)], [1.0])
    dd, (x, b, r, rhat, p), _ = _domain(st=st)
    gb = np.zeros((SIZE[2], SIZE[1], SIZE[0]), dtype=np.float32)
    gb[4, 5, 6] = 1.0
    su.scatter(dd, b, gb)
    su.scatter(dd, p, np.full_like(gb, np.nan))  # the old p must not be read
    res = BiCGStab(dd, st, x, b, r, rhat, p, 0, 1, 2).solve(tol=1e-6, max_iter=20)
    assert not res.converged and res.reason == "breakdown"
    assert res.iterations <= 1 and len(res.residuals) == res.iterations + 1


# ------------------------------------------------------------------ the solves
@pytest.mark.parametrize("dtype", bu.DTYPES, ids=bu.DT_IDS)
@pytest.mark.parametrize("case", bu.SOLVER_CASES, ids=bu.case_id)
def test_advection_diffusion_solves(case, dtype):
    res, x, b, app = bu.solve_case("torch", case, dtype)
    bu.check_solution(res, x, b, app, case, dtype, "torch")


@pytest.mark.parametrize("case", bu.SOLVER_CASES, ids=bu.case_id)
def test_numpy_bicgstab_solves_the_cases(case):
    """the independent solver and the truth operator agree that the cases
    are solvable within the cap: what the library is held to is not an
    artefact of the library"""
    size, vel, nu, sigma, bc, _ = case
    app = AdvectionDiffusion3D(size, velocity=vel, nu=nu, sigma=sigma, backend="torch", gpus=[0],
                               boundary=bu.kinds_of(bc))
    b = su.normal_global(size, np.float32)
    tol = bu.TOL[np.float32]
    x, its, ok = bu.numpy_bicgstab(b, app.stencil, bu.kinds_of(bc), tol, bu.MAX_ITER)
    print(f"numpy {bu.case_id(case)}: {its} iterations")
    assert ok
    assert bu.true_rel_residual(x, b, app.stencil, bu.kinds_of(bc)) <= 2 * tol


def test_nonzero_initial_guess_and_no_overlap():
    case = bu.SOLVER_CASES[4]
    app = bu.make_app("torch", case, np.float64)
    b = su.normal_global(case[0], np.float64)
    app.set_rhs(b)
    app.set_guess(su.normal_global(case[0], np.float64, seed=7))
    res = app.solve(tol=1e-10, max_iter=bu.MAX_ITER, x0_zero=False, overlap=False)
    assert res.converged and res.residuals[0] > 1.0
    assert bu.true_rel_residual(app.solution(), b, app.stencil, bu.kinds_of(case[4])) <= 2e-10


@pytest.mark.parametrize("dtype", bu.DTYPES, ids=bu.DT_IDS)
@pytest.mark.parametrize("gpus", [[0], [0, 0]], ids=["1dom", "2dom"])
def test_multigrid_preconditioner(gpus, dtype):
    case = bu.MG_CASE + (gpus,)
    plain = bu.solve_case("torch", case, dtype)
    pre = bu.solve_case("torch", case, dtype, preconditioner="multigrid")
    bu.check_solution(*plain, case, dtype, "torch plain")
    bu.check_solution(*pre, case, dtype, "torch multigrid")
    print(f"iterations: plain {plain[0].iterations}, multigrid {pre[0].iterations}")
    assert pre[0].iterations < plain[0].iterations


# ------------------------------------------------------------------ two ranks
def _rank_worker(rank, world, port, q):
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        import torch.distributed as dist

        dist.init_process_group("gloo", rank=rank, world_size=world)
        sys.path.insert(0, os.path.dirname(__file__))
        import bicgstab_util
        import stencil_util

        case = bicgstab_util.SOLVER_CASES[4][:5] + ([0],)
        app = bicgstab_util.make_app("torch", case, np.float32)
        assert app.dd.comm.world_size == world
        app.set_rhs(stencil_util.normal_global(case[0], np.float32))
        res = app.solve(tol=1e-5, max_iter=bicgstab_util.MAX_ITER)
        dist.destroy_process_group()
        q.put((rank, "ok", res.converged, res.iterations, res.reason, res.residuals))
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
    (_, _, conv0, it0, why0, res0), (_, _, conv1, it1, why1, res1) = results
    assert conv0 and conv1
    assert it0 == it1 and why0 == why1
    assert res0 == res1  # every entry the identical double
    assert res0[-1] <= 1e-5


# ------------------------------------------------------------------------ CLI
def test_advection_diffusion_cli():
    out = subprocess.run(
        [sys.executable, os.path.join(REPO, "benchmarks", "advection_diffusion.py"), "--backend",
         "torch", "--size", "16", "--iters", "3"],
        capture_output=True, text=True, timeout=300, cwd=REPO,
    )
    assert out.returncode == 0, out.stderr
    lines = out.stdout.strip().splitlines()
    assert len(lines) == 1
    rec = json.loads(lines[0])
    assert rec["benchmark"] == "advection_diffusion" and rec["iterations"] == 3
    assert rec["reason"] == "max_iter"
    for key in ("ms_per_iter", "operator_ms", "reduction_ms", "update_ms"):
        assert rec[key] > 0
