"""Variable-coefficient diffusion on the torch backend (CPU tier): the
slicing references of diffusion_apply, diffusion_inv_diagonal and
scaled_update against the numpy oracle of diffusion_util.py, the argument
checks of DiffusionOperator, JacobiPreconditioner, GeometricMultigrid and
Poisson3D, the V-cycle against the oracle and the plain, Jacobi- and
multigrid-preconditioned solves of the eight cases.

The own-type numpy oracle was run on every row for both dtypes before the
iteration conditions were committed (plain / Jacobi / multigrid, fp32 then
fp64): the oracle alone meets 2 jacobi <= plain and 4 mg <= jacobi on all
eight rows, so no row was dropped or replaced (the counts are printed by
test_oracle_meets_the_iteration_conditions).

Not here: a rank-agreement case over gloo. The launcher of test_mp_gloo.py
starts a worker function fixed inside that file, so it cannot be reused
from a new file without editing it.
"""
import numpy as np
import pytest

import stencil_amd as sa
from stencil_amd import Boundary, Next, Stencil
from stencil_amd.models.poisson3d import Poisson3D

import cg_util as cu
import diffusion_util as du
import mg_util as mu
import stencil_util as su

SIZE = (19, 10, 9)
_ZYX = (SIZE[2], SIZE[1], SIZE[0])


def _domain(dtype, gpus, kinds=None, n=4, size=SIZE, k_kind=Boundary.CLAMP, radius=1):
    """a realized torch domain with quantities u, k, d, o: u's boundary is
    `kinds`, k's non-periodic faces are k_kind; groups [[u], [k]]"""
    dd = sa.DistributedDomain(*size, backend="torch")
    dd.set_radius(radius)
    dd.set_gpus(gpus)
    hs = [dd.add_data(dtype, name) for name in ("u", "k", "d", "o")[:n]]
    dd.set_exchange_groups([[hs[0].index], [hs[1].index]])
    for face, (kind, value) in (kinds or {}).items():
        dd.set_boundary(face, kind, value)
        dd.set_boundary(face, k_kind, quantities=[hs[1]])
    dd.realize()
    return dd, hs


# ------------------------------------------------------------------ the operator
@pytest.mark.parametrize("dtype", cu.DTYPES, ids=cu.DT_IDS)
@pytest.mark.parametrize("bc", ["periodic", "fixed0", "mirror", "antimirror"])
def test_apply_and_diagonal_match_the_oracle_exactly(bc, dtype):
    """exact data (see test_gpu_diffusion.py): bit for bit, two domains"""
    from stencil_amd.solvers import DiffusionOperator

    kinds = cu.kinds_of(bc)
    dd, (u, k, d, o) = _domain(dtype, [0, 0], kinds)
    gu, gk = mu.int_field(_ZYX, dtype, 1), du.int_k(_ZYX, dtype, 2)
    spacing, sigma = (2.0, 1.0, 0.5), 3.0  # h = 0.25, 1, 4
    op = DiffusionOperator(dd, k, 1, spacing=spacing, sigma=sigma, dinv=d)
    su.scatter(dd, u, gu)
    su.scatter(dd, k, gk)
    op.refresh()
    dd.exchange(0)
    for where in ("all", "interior", "exterior"):
        op.apply(u, o, where=where)
    want = du.apply_op(gu, gk, kinds, spacing, sigma, np.dtype(dtype).type)
    np.testing.assert_array_equal(su.gather(dd, o, from_next=True), want)
    op.inv_diagonal(0.5, d)
    diag = du.diagonal(gk, kinds, spacing, sigma, np.dtype(dtype).type)
    np.testing.assert_array_equal(su.gather(dd, d), dtype(0.5) / diag)


@pytest.mark.parametrize("dtype", cu.DTYPES, ids=cu.DT_IDS)
def test_unit_coefficient_is_the_laplacian(dtype):
    kinds = cu.kinds_of("antimirror")
    dd, (u, k, d, o) = _domain(dtype, [0, 0], kinds)
    spacing, sigma = (1.0, 2.0, 0.5), 0.5
    st = -Stencil.laplacian(2, spacing) + sigma * Stencil.identity()
    su.scatter(dd, u, mu.int_field(_ZYX, dtype, 3))
    su.scatter(dd, k, np.ones(_ZYX, dtype=dtype))
    dd.exchange(0)
    dd.exchange(1)
    dd.apply_diffusion(k, u, o, spacing=spacing, sigma=sigma)
    dd.apply_stencil(st, u, d)
    np.testing.assert_array_equal(su.gather(dd, o, from_next=True),
                                  su.gather(dd, d, from_next=True))


@pytest.mark.parametrize("dtype", cu.DTYPES, ids=cu.DT_IDS)
def test_scaled_update_matches_numpy(dtype):
    dd, (x, d, y, z) = cu.vector_domain(SIZE, [dtype] * 4, "torch", [0, 0])
    gx, gd, gy, gz = (su.normal_global(SIZE, dtype, seed=s) for s in (1, 2, 3, 4))
    for h, g in ((x, gx), (d, gd), (y, gy)):
        su.scatter(dd, h, g)
    su.scatter(dd, z, gz, to_next=True)
    al, be, ga = dtype(1.0 / 3.0), dtype(-0.7), dtype(1.1)
    want = al * gx + gd * (be * gy + ga * gz)
    assert want.dtype == dtype
    dd.scaled_update(1.0 / 3.0, x, d, -0.7, y, 1.1, Next(z), out=z)
    np.testing.assert_array_equal(su.gather(dd, z), want)
    dd.scaled_update(1.0 / 3.0, x, d, -0.7, y, 1.1, Next(z), out=x)  # out aliases x
    np.testing.assert_array_equal(su.gather(dd, x), want)
    i32 = cu.vector_domain(SIZE, [np.float32, np.int32], "torch", [0])
    with pytest.raises(ValueError):
        i32[0].scaled_update(1.0, i32[1][0], i32[1][1], 1.0, i32[1][0], 1.0, i32[1][0],
                             out=i32[1][0])
    with pytest.raises(ValueError):
        dd.scaled_update(1.0, x, d, 1.0, y, 1.0, z, out=x, where=((-2, 0, 0), (5, 5, 5)))


def test_operator_argument_errors():
    from stencil_amd.solvers import (ConjugateGradient, DiffusionOperator, GeometricMultigrid,
                                     JacobiPreconditioner)

    f32, f64 = np.float32, np.float64
    fixed = cu.kinds_of("fixed0")
    dd, (u, k, d, o) = _domain(f32, [0], fixed)
    DiffusionOperator(dd, k, 1, dinv=d)  # fine
    raw = sa.DistributedDomain(8, 8, 8, backend="torch")
    raw.set_radius(1)
    rk = raw.add_data(f32, "k")
    with pytest.raises(ValueError):  # not realized
        DiffusionOperator(raw, rk, 0)
    with pytest.raises(ValueError):  # k is not in group 0
        DiffusionOperator(dd, k, 0)
    with pytest.raises(ValueError):
        DiffusionOperator(dd, k, 1, sigma=-1.0)
    r0, (_, k0, _, _) = _domain(f32, [0], radius=sa.Radius.constant(0))
    with pytest.raises(ValueError):  # face radius below 1
        DiffusionOperator(r0, k0, 1)
    mixed = sa.DistributedDomain(8, 8, 8, backend="torch")
    mixed.set_radius(1)
    mixed.set_gpus([0])
    mk, md = mixed.add_data(f32, "k"), mixed.add_data(f64, "d")
    mixed.realize()
    with pytest.raises(ValueError):  # k and dinv of different float types
        DiffusionOperator(mixed, mk, 0, dinv=md)
    for kind in (Boundary.FIXED, Boundary.ANTIMIRROR, Boundary.OPEN):
        bad, (_, bk, _, _) = _domain(f32, [0], fixed, k_kind=kind)
        with pytest.raises(ValueError):
            DiffusionOperator(bad, bk, 1)
    ok, (_, mk2, _, _) = _domain(f32, [0], fixed, k_kind=Boundary.MIRROR)
    DiffusionOperator(ok, mk2, 1)
    # a preconditioner needs the operator's dinv
    bare = DiffusionOperator(dd, k, 1)
    with pytest.raises(ValueError):
        JacobiPreconditioner(bare)
    big, (e, bk2, bd, bo) = _domain(f32, [0], fixed, size=(16, 16, 16))
    with pytest.raises(ValueError):
        GeometricMultigrid(big, lambda level: DiffusionOperator(big, bk2, 1), e, 0)
    asked = []

    def operator_at(level):
        asked.append(level)
        return DiffusionOperator(big, bk2, 1, dinv=bd)

    su.scatter(big, bk2, np.ones((16, 16, 16), dtype=f32))
    mg = GeometricMultigrid(big, operator_at, e, 0)
    assert asked == [0]  # the levels below are built from level 0
    assert mg.levels == [(16, 16, 16), (8, 8, 8), (4, 4, 4), (2, 2, 2)]
    assert [lv.A.spacing for lv in mg._levels] == [(s,) * 3 for s in (1.0, 2.0, 4.0, 8.0)]
    const = Poisson3D((16, 16, 16), backend="torch", gpus=[0], boundary=fixed,
                      preconditioner="multigrid")
    const.realize()
    with pytest.raises(ValueError):
        const.mg.refresh_coefficients()
    with pytest.raises(ValueError):  # the operator of another domain
        ConjugateGradient(big, DiffusionOperator(dd, k, 1), e, bk2, bd, bo, group_p=0)


def test_poisson3d_argument_errors():
    fixed = cu.kinds_of("fixed0")
    with pytest.raises(ValueError):
        Poisson3D((16, 16, 16), order=4, backend="torch", boundary=fixed, coefficient=True)
    with pytest.raises(ValueError):
        Poisson3D((16, 16, 16), backend="torch", boundary=fixed, preconditioner="jacobi")
    with pytest.raises(ValueError):  # the singularity check stays
        Poisson3D((16, 16, 16), backend="torch", coefficient=True)
    app = Poisson3D((16, 16, 16), backend="torch", gpus=[0], boundary=fixed, coefficient=True,
                    preconditioner="jacobi")
    k = np.ones((16, 16, 16))
    for bad in (0.0, -1.0, np.nan, np.inf):
        k[3, 4, 5] = bad
        with pytest.raises(ValueError):
            app.set_coefficient(k)
    with pytest.raises(ValueError):
        app.set_coefficient(np.ones((16, 16, 8)))
    plain = Poisson3D((16, 16, 16), backend="torch", gpus=[0], boundary=fixed)
    with pytest.raises(ValueError):
        plain.set_coefficient(np.ones((16, 16, 16)))


def test_correction_argument_errors_and_result():
    """ConjugateGradient(correction=): one more distinct quantity and
    group_x; the result's last residual is then the true one"""
    from stencil_amd.solvers import ConjugateGradient

    dd, (x, b, r, p, d) = su.make_domain((12, 8, 8), sa.Radius.constant(1), [np.float64] * 5,
                                         "torch", [0])
    st = -Stencil.laplacian(2) + 0.5 * Stencil.identity()
    with pytest.raises(ValueError):
        ConjugateGradient(dd, st, x, b, r, p, correction=d)  # no group_x
    with pytest.raises(ValueError):
        ConjugateGradient(dd, st, x, b, r, p, group_x=0, correction=p)
    cg = ConjugateGradient(dd, st, x, b, r, p, group_x=0, correction=d)
    gb = su.normal_global((12, 8, 8), np.float64)
    su.scatter(dd, b, gb)
    res = cg.solve(tol=1e-10, max_iter=200)
    assert res.converged and len(res.residuals) == res.iterations + 1
    true = cu.true_rel_residual(su.gather(dd, x), gb, st, None)
    assert true <= 1e-10 and abs(res.residuals[-1] - true) <= 1e-3 * true


# ------------------------------------------------------ the cycle and the solves
@pytest.mark.parametrize("dtype", cu.DTYPES, ids=cu.DT_IDS)
@pytest.mark.parametrize("case", du.DIFF_CASES, ids=du.case_id)
def test_oracle_meets_the_iteration_conditions(case, dtype):
    """the own-type numpy oracle alone: the conditions asked of the
    library hold for the scheme itself on this row"""
    its = {w: du.oracle_iterations(case, dtype, w) for w in ("plain", "jacobi", "mg")}
    print(f"oracle {du.case_id(case)} {np.dtype(dtype).name}: {its}")
    assert its["plain"] < du.MAX_ITER
    assert 2 * its["jacobi"] <= its["plain"]
    assert 4 * its["mg"] <= its["jacobi"]


@pytest.mark.parametrize("dtype", cu.DTYPES, ids=cu.DT_IDS)
@pytest.mark.parametrize("case", du.DIFF_CASES, ids=du.case_id)
def test_cycle_torch_against_the_oracle(case, dtype):
    du.check_cycle("torch", case, dtype)


@pytest.mark.parametrize("dtype", cu.DTYPES, ids=cu.DT_IDS)
@pytest.mark.parametrize("case", du.DIFF_CASES, ids=du.case_id)
def test_iteration_conditions_torch(case, dtype):
    du.check_iterations("torch", case, dtype)


@pytest.mark.parametrize("dtype", cu.DTYPES, ids=cu.DT_IDS)
@pytest.mark.parametrize("solver", list(du.SOLVERS))
@pytest.mark.parametrize("case", du.DIFF_CASES, ids=du.case_id)
def test_solve_true_residual_torch(case, solver, dtype):
    """Converged, and the true residual in the wide type within 2 tol.

    Without the solver's true-residual check (ConjugateGradient's
    `correction`) float32 misses this on the two periodic sigma = 1e-3
    rows: the recursive residual converges while b - A x stays at 2.2e-05
    (smooth, plain), 8.8e-05 (jump, plain), 5.3e-05 (jump, Jacobi) and
    2.3e-05 (jump, multigrid), as in a float32 numpy oracle of the same
    iterations: lambda_min = sigma = 1e-3, ||x|| / ||b|| = 5.4, and every
    x += alpha p rounds x. With it the same solves need 0 to 6 iterations
    more and end below 1e-05."""
    du.check_solve("torch", case, dtype, solver)


@pytest.mark.parametrize("pre", ["jacobi", "multigrid"])
def test_refresh_coefficients_torch(pre):
    """solve, set_coefficient(new k), solve: as many iterations as an app
    built with the new k from the start"""
    case, dtype = du.DIFF_CASES[1], np.float64
    new_k = du.k_smooth(case[0])
    b = su.normal_global(case[0], dtype)
    app = du.make_app("torch", case, dtype, pre)
    app.set_rhs(b)
    first = app.solve(tol=cu.TOL[dtype], max_iter=du.MAX_ITER)
    app.set_coefficient(new_k)
    again = app.solve(tol=cu.TOL[dtype], max_iter=du.MAX_ITER)
    fresh = du.make_app("torch", case, dtype, pre, k=new_k)
    fresh.set_rhs(b)
    want = fresh.solve(tol=cu.TOL[dtype], max_iter=du.MAX_ITER)
    assert first.converged and again.converged and want.converged
    assert again.iterations == want.iterations
    np.testing.assert_array_equal(app.solution(), fresh.solution())


@pytest.mark.parametrize("dtype", cu.DTYPES, ids=cu.DT_IDS)
def test_unit_coefficient_solves_like_the_constant_path(dtype):
    """k = 1 (the initial coefficient): the iteration counts of the
    constant-coefficient solver within 1, plain and multigrid"""
    case = mu.MG_CASES[0]
    size, order, sigma, bc, gpus = case
    for pre in (None, "multigrid"):
        app = Poisson3D(size, dtype=dtype, sigma=sigma, backend="torch", gpus=gpus,
                        boundary=cu.kinds_of(bc), preconditioner=pre, coefficient=True)
        app.realize()
        app.set_rhs(su.normal_global(size, dtype))
        res = app.solve(tol=cu.TOL[dtype], max_iter=cu.MAX_ITER)
        want = mu.solve_case("torch", case, dtype, pre)[0]
        assert res.converged and abs(res.iterations - want.iterations) <= 1


@pytest.mark.parametrize("dtype", cu.DTYPES, ids=cu.DT_IDS)
def test_constant_coefficient_path_is_unchanged(dtype):
    """regression guard (passes before this feature too): Poisson3D without
    a coefficient solves MG_CASES[0] in the iteration counts of mg_util's
    own solves, and within the numpy oracle's count + 2"""
    case = mu.MG_CASES[0]
    size, order, sigma, bc, gpus = case
    for pre in (None, "multigrid"):
        app = Poisson3D(size, order=order, dtype=dtype, sigma=sigma, backend="torch", gpus=gpus,
                        boundary=cu.kinds_of(bc), preconditioner=pre)
        app.realize()
        app.set_rhs(su.normal_global(size, dtype))
        res = app.solve(tol=cu.TOL[dtype], max_iter=cu.MAX_ITER)
        assert res.converged
        if pre is None:
            assert res.iterations == mu.plain_iterations("torch", case, dtype)
        else:
            assert res.iterations == mu.solve_case("torch", case, dtype, pre)[0].iterations
            assert res.iterations <= mu.oracle_iterations(case, dtype) + 2
