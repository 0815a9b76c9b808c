"""Shared helpers of the null-space tests (test_nullspace_cpu.py,
test_gpu_nullspace.py): the four vector operations of the projection
P v = v - mean(v) against exact numpy, and the singular solves
(Poisson3D(nullspace="constant")) against the truth operator in numpy's
wide type.

Exact data: integer-valued fields below 753 and dyadic coefficients, so
every product, every sum and every association is exact in either type and
each result equals numpy's bit for bit.

The solves use b = normal + 3, grossly inconsistent (mean(b) ~ 3 against a
standard deviation of 1): without the projection CG breaks down on it.
"""
import numpy as np

from stencil_amd import Boundary, Next
from stencil_amd.models.poisson3d import Poisson3D

import boundary_util
import cg_util as cu
import diffusion_util as du
import stencil_util as su

DTYPES, DT_IDS = cu.DTYPES, cu.DT_IDS
MAX_ITER = 300

KINDS = {
    "periodic": None,
    "mirror": boundary_util.all_faces(Boundary.MIRROR, 0),
    # x periodic, y and z MIRROR
    "mixed": {f: (Boundary.MIRROR, 0) for f in ("y-", "y+", "z-", "z+")},
}

# (size, order, boundary, gpus, preconditioner): the six probed cases and
# one with mixed boundary kinds
SOLVE_CASES = [
    ((19, 10, 9), 2, "periodic", [0], None),
    ((19, 10, 9), 4, "mirror", [0, 0], None),
    ((17, 9, 33), 8, "mirror", [0], None),
    ((32, 16, 24), 2, "periodic", [0, 0], "multigrid"),
    ((16, 16, 16), 2, "mirror", [0], "multigrid"),
    ((32, 32, 32), 4, "mirror", [0, 0], "multigrid"),
    ((19, 10, 9), 2, "mixed", [0], None),
]

# (size, boundary, dtype, gpus, iterations of the unprojected arithmetic on
# a right-hand side made consistent by hand)
COEFF_CASES = [
    ((32, 32, 32), "mirror", np.float64, [0], 29),
    ((16, 16, 16), "mixed", np.float32, [0, 0], 13),
]

# multigrid-CG iterations of the unprojected arithmetic in fp64 at tol 1e-10
GRID_ITERATIONS = {
    "periodic": {16: 16, 32: 18, 64: 20},
    "mirror": {16: 17, 32: 19, 64: 21},
}


def solve_id(c):
    size, order, bc, gpus, pre = c
    return f"{'x'.join(map(str, size))}-o{order}-{bc}-{len(gpus)}dom-{pre or 'plain'}"


def coeff_id(c):
    size, bc, dtype, gpus, _ = c
    return f"{'x'.join(map(str, size))}-{bc}-{np.dtype(dtype).name}-{len(gpus)}dom"


# ---- exact data ----
def second(size, dtype):
    """another integer field below 753"""
    return (su.ripple_global(size, dtype)[::-1, ::-1, ::-1] % 97 + 1).astype(dtype)


def cg_fields(size, dtype):
    """(x, p, r, A p): integer fields"""
    gx, gp = su.ripple_global(size, dtype), second(size, dtype)
    gr = ((gx + 2 * gp) % 211).astype(dtype)
    gap = ((3 * gx + gp) % 89).astype(dtype)
    return gx, gp, gr, gap


def box_of(lo, hi):
    return (slice(lo[2], hi[2]), slice(lo[1], hi[1]), slice(lo[0], hi[0]))


def f64(a):
    return a.astype(np.float64)


def same_bits(got, want, what=""):
    assert got.dtype == want.dtype, (what, got.dtype, want.dtype)
    np.testing.assert_array_equal(got.view(np.uint8), want.view(np.uint8), err_msg=what)


ALPHA, BETA, C = 0.5, -0.25, 1.5  # dyadic


def check_reductions_exact(backend, size, gpus, dtype, lo=None, hi=None):
    """sum and dot_sums over the box [lo, hi) (None: where="all") of
    integer fields, curr and next operands: bitwise numpy's"""
    dd, (a, b) = cu.vector_domain(size, [dtype] * 2, backend, gpus)
    ga, gb = su.ripple_global(size, dtype), second(size, dtype)
    gn = ((ga + gb) % 101).astype(dtype)
    su.scatter(dd, a, ga)
    su.scatter(dd, b, gb)
    su.scatter(dd, b, gn, to_next=True)
    where = "all" if lo is None else (lo, hi)
    bx = box_of((0, 0, 0), size) if lo is None else box_of(lo, hi)
    sa_, sb_, sn_ = (float(f64(g[bx]).sum()) for g in (ga, gb, gn))
    assert dd.sum(a, where=where) == sa_
    assert dd.sum(Next(b), where=where) == sn_
    assert dd.dot_sums(a, b, where=where) == (float((f64(ga[bx]) * f64(gb[bx])).sum()), sa_, sb_)
    assert dd.dot_sums(a, Next(b), where=where) == (
        float((f64(ga[bx]) * f64(gn[bx])).sum()), sa_, sn_)
    # a == b is allowed: (a . a, sum a, sum a)
    assert dd.dot_sums(a, where=where) == (float((f64(ga[bx]) ** 2).sum()), sa_, sa_)
    # read only
    same_bits(su.gather(dd, a), ga)
    same_bits(su.gather(dd, b), gb)
    same_bits(su.gather(dd, b, from_next=True), gn)


def check_axpbyc_exact(backend, size, gpus, dtype, lo=None, hi=None):
    """out = alpha x + beta y + c with dyadic coefficients on integer data,
    out in a third quantity, in a next buffer and aliasing x and y"""
    dd, (a, b, c) = cu.vector_domain(size, [dtype] * 3, backend, gpus)
    ga, gb = su.ripple_global(size, dtype), second(size, dtype)
    su.scatter(dd, a, ga)
    su.scatter(dd, b, gb)
    where = "all" if lo is None else (lo, hi)
    bx = box_of((0, 0, 0), size) if lo is None else box_of(lo, hi)

    def expect(base, g):
        want = base.copy()
        want[bx] = g[bx]
        return want.astype(dtype)

    zero = np.zeros_like(ga)
    su.scatter(dd, c, zero)
    su.scatter(dd, c, zero, to_next=True)
    first =(ALPHA * ga + BETA * gb + C).astype(dtype)
    dd.axpbyc(ALPHA, a, BETA, b, C, out=c, where=where)
    dd.axpbyc(ALPHA, a, BETA, b, C, out=Next(c), where=where)
    dd.axpbyc(ALPHA, a, BETA, b, C, out=a, where=where)  # out aliases x
    dd.backend.sync_compute()
    same_bits(su.gather(dd, c), expect(zero, first), "out")
    same_bits(su.gather(dd, c, from_next=True), expect(zero, first), "out in next")
    ga2 = expect(ga, first)
    same_bits(su.gather(dd, a), ga2, "out aliases x")
    dd.axpbyc(2.0, a, 0.5, b, -C, out=b, where=where)  # out aliases y
    dd.backend.sync_compute()
    same_bits(su.gather(dd, b), expect(gb, (2.0 * ga2 + 0.5 * gb - C).astype(dtype)),
              "out aliases y")
    same_bits(su.gather(dd, a), ga2, "x is read only")


def check_cg_update_sum_exact(backend, size, gpus, dtype):
    """cg_update_sum against numpy, and against cg_update on a copy: the
    same bits in x and r, the same r . r"""
    gx, gp, gr, gap = cg_fields(size, dtype)
    alpha = 0.25
    outs = []
    for fused_sum in (True, False):
        dd, (x, p, r) = cu.vector_domain(size, [dtype] * 3, backend, gpus)
        su.scatter(dd, x, gx)
        su.scatter(dd, p, gp)
        su.scatter(dd, p, gap, to_next=True)
        su.scatter(dd, r, gr)
        if fused_sum:
            rr, sr = dd.cg_update_sum(alpha, x, p, r)
        else:
            rr, sr = dd.cg_update(alpha, x, p, r), None
        outs.append((rr, sr, su.gather(dd, x), su.gather(dd, r), su.gather(dd, p),
                     su.gather(dd, p, from_next=True)))
    rn = (gr - alpha * gap).astype(dtype)
    (rr, sr, ox, orr, op, oap), (rr0, _, ox0, or0, _, _) = outs
    # r_new is a multiple of 1/4 below 2^10: squares and sums exact in fp64
    assert rr == float((f64(rn) ** 2).sum())
    assert sr == float(f64(rn).sum())
    assert rr == rr0
    same_bits(ox, (gx + alpha * gp).astype(dtype), "x")
    same_bits(orr, rn, "r")
    same_bits(ox, ox0, "x against cg_update")
    same_bits(orr, or0, "r against cg_update")
    same_bits(op, gp, "p is read only")
    same_bits(oap, gap, "A p is read only")


# ---- the singular solves ----
def rhs(size, dtype):
    return (su.normal_global(size, dtype) + 3).astype(dtype)


def check_projected_solution(res, x, b, ax, dtype, what, max_iterations=None):
    """the assertions of a singular solve. ax = A x in the wide type.
    - the true residual ||P b - A x|| / ||P b|| within 2 tol, check_solution's
      bound;
    - |mean(x)| <= 2 eps max|x|: x -= c rounds x_i - c once and c once,
      each at most eps / 2 relative, and |c| <= max|x|."""
    tol, wide = cu.TOL[dtype], su._wide(dtype)
    pb = b.astype(wide) - b.astype(wide).mean()
    true = float(cu.norm2(pb - ax) / cu.norm2(pb))
    mean = abs(float(x.astype(wide).mean()))
    bound = 2 * float(np.finfo(dtype).eps) * float(np.abs(x).max())
    print(f"{what} {np.dtype(dtype).name}: {res.reason}, {res.iterations} iterations, "
          f"recursive {res.residuals[-1]:.3e} true {true:.3e} (tol {tol:.0e}), "
          f"|mean x| {mean:.3e} (bound {bound:.3e})")
    assert res.converged, res.reason
    assert res.residuals[0] == 1.0
    assert res.residuals[-1] <= tol
    assert true <= 2 * tol
    assert mean <= bound
    if max_iterations is not None:
        assert res.iterations <= max_iterations


def solve_constant(backend, case, dtype):
    """(CGResult, x, b, app) of one SOLVE_CASES entry"""
    size, order, bc, gpus, pre = case
    app = Poisson3D(size, order=order, dtype=dtype, sigma=0.0, backend=backend, gpus=gpus,
                    boundary=KINDS[bc], preconditioner=pre, nullspace="constant")
    app.realize()
    b = rhs(size, dtype)
    app.set_rhs(b)
    res = app.solve(tol=cu.TOL[dtype], max_iter=MAX_ITER)
    return res, app.solution(), b, app


def check_solve(backend, case, dtype, max_iterations=None):
    res, x, b, app = solve_constant(backend, case, dtype)
    wide = su._wide(dtype)
    ax = cu.apply_true(x.astype(wide), app.stencil, KINDS[case[2]])
    check_projected_solution(res, x, b, ax, dtype, f"{backend} {solve_id(case)}", max_iterations)
    same_bits(su.gather(app.dd, app.b), b, "b is never written")
    assert app.xc is not None  # the true residual was checked


def jump_k(size, dtype):
    """k = 100 where y < ny/2 and x >= nx/2, 1 elsewhere"""
    return du.k_jump(size, contrast=100.0).astype(dtype)


def check_coefficient_solve(backend, case):
    size, bc, dtype, gpus, parent_iterations = case
    app = Poisson3D(size, dtype=dtype, sigma=0.0, backend=backend, gpus=gpus, boundary=KINDS[bc],
                    preconditioner="multigrid", coefficient=True, nullspace="constant")
    app.realize()
    k = jump_k(size, dtype)
    app.set_coefficient(k)
    b = rhs(size, dtype)
    app.set_rhs(b)
    res = app.solve(tol=cu.TOL[dtype], max_iter=MAX_ITER)
    x = app.solution()
    ax = du.apply_op(x, k, KINDS[bc], (1.0, 1.0, 1.0), 0.0, su._wide(dtype))
    print(f"iterations {res.iterations}, the unprojected arithmetic on a consistent b "
          f"{parent_iterations}")
    # + 3: one V-cycle's worth of slack for the different b
    check_projected_solution(res, x, b, ax, dtype, f"{backend} jump {coeff_id(case)}",
                             parent_iterations + 3)


def check_constant_rhs(backend, dtype, gpus):
    """b = 0.5 everywhere: P b = 0"""
    size = (19, 10, 9)
    app = Poisson3D(size, order=2, dtype=dtype, sigma=0.0, backend=backend, gpus=gpus,
                    boundary=KINDS["mirror"], nullspace="constant")
    app.realize()
    b = np.full((size[2], size[1], size[0]), 0.5, dtype=dtype)
    app.set_rhs(b)
    app.set_guess(su.ripple_global(size, dtype))  # x's content must not survive
    res = app.solve(tol=cu.TOL[dtype], max_iter=MAX_ITER)
    assert res.reason == "zero_rhs" and res.converged and res.iterations == 0
    assert (app.solution() == 0).all()
    same_bits(su.gather(app.dd, app.b), b, "b is unchanged")
