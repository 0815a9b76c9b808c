"""Shared helpers of the BiCGStab tests (test_bicgstab_cpu.py,
test_gpu_bicgstab.py): the solver cases, an independent numpy BiCGStab in
the wide type, the boundary-aware truth operator with CLAMP, and the exact
data and numpy oracles of the three fused vector operations."""
import numpy as np

import stencil_amd as sa
from stencil_amd import Boundary, Next
from stencil_amd.models.advection_diffusion3d import AdvectionDiffusion3D

import boundary_util
import cg_util as cu
import stencil_util as su

DTYPES, DT_IDS, TOL, MAX_ITER = cu.DTYPES, cu.DT_IDS, cu.TOL, cu.MAX_ITER

_KINDS = {
    "periodic": None,
    "fixed0": boundary_util.all_faces(Boundary.FIXED, 0),
    "mirror": boundary_util.all_faces(Boundary.MIRROR, 0),
    "clamp": boundary_util.all_faces(Boundary.CLAMP, 0),
}

# (size, velocity, nu, sigma, boundary, gpus)
SOLVER_CASES = [
    ((19, 10, 9), (1.0, 0.5, -0.25), 0.5, 1.0, "periodic", [0]),
    # pure upwind: an asymmetric radius, no downwind halo
    ((19, 10, 9), (1.0, 0.5, -0.25), 0.0, 1.0, "periodic", [0, 0]),
    ((17, 9, 33), (0.75, -0.5, 0.25), 1.0, 0.0, "fixed0", [0, 0]),
    ((19, 10, 9), (1.0, 0.5, -0.25), 0.5, 0.25, "mirror", [0]),
    ((19, 10, 9), (4.0, 2.0, -1.0), 0.125, 0.5, "clamp", [0, 0]),
]
# the multigrid case: (size, velocity, nu, sigma, boundary), 1 and 2 local domains
MG_CASE = ((32, 32, 32), (1.0, 0.5, -0.25), 1.0, 0.0, "fixed0")


def case_id(c):
    size, vel, nu, sigma, bc, gpus = c
    return (f"{'x'.join(map(str, size))}-v{','.join(f'{v:g}' for v in vel)}-nu{nu:g}-s{sigma:g}"
            f"-{bc}-{len(gpus)}dom")


def kinds_of(bc):
    return _KINDS[bc]


# ---- the truth operator, CLAMP included ----
def pad_array(g, radius, kinds):
    """cg_util.pad_array with CLAMP: the global array padded by the face
    radii, one axis at a time in the order x, y, z, with the numpy pad modes
    of boundary_util.padded_global"""
    kinds = kinds or {}
    faces = (radius.x, radius.y, radius.z)
    for a in range(3):
        ax = 2 - a  # arrays are (z, y, x)
        rlo, rhi = faces[a](-1), faces[a](1)
        name = "xyz"[a]
        if name + "-" not in kinds and name + "+" not in kinds:
            pw = [(0, 0)] * 3
            pw[ax] = (rlo, rhi)
            g = np.pad(g, pw, mode="wrap")
            continue
        for side, r in ((0, rlo), (1, rhi)):
            kind, value = kinds[name + "-+"[side]]
            pw = [(0, 0)] * 3
            pw[ax] = (r, 0) if side == 0 else (0, r)
            n = g.shape[ax]
            if kind == Boundary.FIXED:
                g = np.pad(g, pw, mode="constant", constant_values=np.array(value, dtype=g.dtype))
            elif kind == Boundary.CLAMP:
                g = np.pad(g, pw, mode="edge")
            elif kind in (Boundary.MIRROR, Boundary.ANTIMIRROR):
                g = np.pad(g, pw, mode="symmetric")
                if kind == Boundary.ANTIMIRROR:
                    sl = [slice(None)] * 3
                    sl[ax] = slice(0, r) if side == 0 else slice(n, n + r)
                    g[tuple(sl)] = -g[tuple(sl)]
            else:
                raise AssertionError(kind)
    return g


def apply_true(g, stencil, kinds):
    """A g in the wide type of g's dtype, boundary included"""
    radius = stencil.radius()
    size = (g.shape[2], g.shape[1], g.shape[0])
    return su.correlate_padded(pad_array(g, radius, kinds), radius, size, stencil)


def true_rel_residual(x, b, stencil, kinds):
    """||b - A x|| / ||b|| from the gathered x, in the wide type"""
    wide = su._wide(b.dtype)
    res = b.astype(wide) - apply_true(x, stencil, kinds)
    return float(cu.norm2(res) / cu.norm2(b.astype(wide)))


def numpy_bicgstab(b, stencil, kinds, tol, max_iter):
    """textbook unpreconditioned BiCGStab from x = 0, every array and
    scalar in the wide type of b's dtype; returns (x, iterations,
    converged). Independent of the library: numpy and apply_true only."""
    dtype = b.dtype
    wide = su._wide(dtype)

    def A(v):
        return apply_true(v.astype(wide), stencil, kinds)

    bw = b.astype(wide)
    x = np.zeros_like(bw)
    r = bw.copy()
    rhat = r.copy()
    bb = (bw * bw).sum()
    rho = (rhat * r).sum()
    p = r.copy()
    for it in range(1, max_iter + 1):
        v = A(p)
        alpha = rho / (rhat * v).sum()
        s = r - alpha * v
        if (s * s).sum() <= tol * tol * bb:
            return x + alpha * p, it, True
        t = A(s)
        omega = (t * s).sum() / (t * t).sum()
        x = x + alpha * p + omega * s
        r = s - omega * t
        if (r * r).sum() <= tol * tol * bb:
            return x, it, True
        rho_new = (rhat * r).sum()
        beta = (rho_new / rho) * (alpha / omega)
        p = r + beta * (p - omega * v)
        rho = rho_new
    return x, max_iter, False


# ---- the solves ----
def make_app(backend, case, dtype, preconditioner=None):
    size, vel, nu, sigma, bc, gpus = case
    app = AdvectionDiffusion3D(size, velocity=vel, nu=nu, sigma=sigma, dtype=dtype,
                               backend=backend, gpus=gpus, boundary=kinds_of(bc),
                               preconditioner=preconditioner)
    app.realize()
    return app


def solve_case(backend, case, dtype, preconditioner=None):
    """(CGResult, x, b, app) of one case"""
    app = make_app(backend, case, dtype, preconditioner)
    b = su.normal_global(case[0], dtype)
    app.set_rhs(b)
    res = app.solve(tol=TOL[dtype], max_iter=MAX_ITER)
    return res, app.solution(), b, app


def check_solution(res, x, b, app, case, dtype, what):
    """the issue's assertions: converged, residuals[0] == 1, one entry per
    iteration, and the true residual in the wide type within 2 tol (the
    bound of cg_util.check_solution for a solver that verifies its residual
    in the working precision)"""
    tol = TOL[dtype]
    true = true_rel_residual(x, b, app.stencil, kinds_of(case[4]))
    print(f"{what} {case_id(case)} {np.dtype(dtype).name}: {res.iterations} iterations, "
          f"{app.solver.restarts} restarts, last residual {res.residuals[-1]:.3e} "
          f"true {true:.3e} (tol {tol:.0e})")
    assert res.converged, res.reason
    assert res.residuals[0] == 1.0
    assert len(res.residuals) == res.iterations + 1
    assert true <= 2 * tol
    return true


# ---- exact data for the three ops ----
# Integers of magnitude <= 8 and dyadic scalars: every product, sum and
# square below is a multiple of 1/64 far below 2^24 / 64, exact in fp32 and
# fp64 in any order, with or without FMA; the fp64 sums of at most 43k such
# terms are exact too. Compared bitwise.
ALPHA, BETA, OMEGA = 0.5, -0.25, 0.125


def small_ints(size, dtype, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(-8, 9, size=(size[2], size[1], size[0])).astype(dtype)


def box_slices(lo, hi):
    return (slice(lo[2], hi[2]), slice(lo[1], hi[1]), slice(lo[0], hi[0]))


def fsum(a, b):
    return float((a.astype(np.float64) * b.astype(np.float64)).sum())


def oracle_axpby_norm2(gx, gy, bx):
    out = (ALPHA * gx[bx] + BETA * gy[bx]).astype(gx.dtype)
    return out, fsum(out, out)


def oracle_dot_pair(ga, gb, bx):
    return fsum(ga[bx], gb[bx]), fsum(ga[bx], ga[bx])


def oracle_bicgstab_update(gy, gz, gx, gr, gt, gh, bx):
    """(x_new, r_new, (rr, rho)) over the box"""
    xn = (gx[bx] + ALPHA * gy[bx] + OMEGA * gz[bx]).astype(gx.dtype)
    rn = (gr[bx] - OMEGA * gt[bx]).astype(gx.dtype)
    return xn, rn, (fsum(rn, rn), fsum(gh[bx], rn))


def embed(base, bx, part):
    out = base.copy()
    out[bx] = part
    return out


def run_ops_exact(backend, size, lo, hi, dtype, gpus):
    """the three ops on exact data over the box [lo, hi) ("all" when it is
    the whole domain; a box is applied as given on every local domain, so a
    proper box wants one local domain), every variant of operand placement and aliasing the
    issue names, each compared bitwise with the numpy oracle"""
    dd, (a, b, c, d, e, f) = cu.vector_domain(size, [dtype] * 6, backend, gpus)
    where = "all" if (tuple(lo), tuple(hi)) == ((0, 0, 0), tuple(size)) else (lo, hi)
    bx = box_slices(lo, hi)
    g = [small_ints(size, dtype, seed) for seed in range(1, 9)]
    zero = np.zeros_like(g[0])

    def eq(got, want):
        np.testing.assert_array_equal(got.view(np.uint8), want.view(np.uint8))

    def fill():
        for h, arr in zip((a, b, c, d, e, f), g):
            su.scatter(dd, h, arr)
        su.scatter(dd, a, g[6], to_next=True)
        su.scatter(dd, b, g[7], to_next=True)
        su.scatter(dd, c, zero, to_next=True)

    # axpby_norm2: out a third buffer, a next buffer, x's, y's
    fill()
    out, nn = oracle_axpby_norm2(g[0], g[7], bx)
    assert dd.axpby_norm2(ALPHA, a, BETA, Next(b), out=c, where=where) == nn
    eq(su.gather(dd, c), embed(g[2], bx, out))
    assert dd.axpby_norm2(ALPHA, a, BETA, Next(b), out=Next(c), where=where) == nn
    eq(su.gather(dd, c, from_next=True), embed(zero, bx, out))
    assert dd.axpby_norm2(ALPHA, a, BETA, Next(b), out=a, where=where) == nn  # out is x
    eq(su.gather(dd, a), embed(g[0], bx, out))
    fill()
    assert dd.axpby_norm2(ALPHA, a, BETA, Next(b), out=Next(b), where=where) == nn  # out is y
    eq(su.gather(dd, b, from_next=True), embed(g[7], bx, out))
    eq(su.gather(dd, a), g[0])

    # dot_pair
    fill()
    assert dd.dot_pair(a, b, where=where) == oracle_dot_pair(g[0], g[1], bx)
    assert dd.dot_pair(Next(a), b, where=where) == oracle_dot_pair(g[6], g[1], bx)
    assert dd.dot_pair(a, a, where=where) == oracle_dot_pair(g[0], g[0], bx)

    # bicgstab_update goes over the local_rects at the DistributedDomain
    # level: a box goes through the backend, one (lo, hi) per local domain
    def update(y, z, x, r, t, h):
        ops = dd._vector_operands("bicgstab_update", [y, z, x, r, t, h])
        (qy, ny), (qz, nz), (qx, _), (qr, _), (qt, nt), (qh, nh) = ops
        if where == "all":
            return dd.bicgstab_update(ALPHA, y, OMEGA, z, x, r, t, h)
        per = dd.backend.bicgstab_update([(lo, hi)] * dd.num_local(), ALPHA, qy, ny, OMEGA, qz,
                                         nz, qx, qr, qt, nt, qh, nh)
        return dd._global_sums(per, 2)

    # y = a, z = b, x = c, r = d, t = Next(a), rhat = Next(b): distinct buffers
    fill()
    xn, rn, vals = oracle_bicgstab_update(g[0], g[1], g[2], g[3], g[6], g[7], bx)
    assert update(a, b, c, d, Next(a), Next(b)) == vals
    eq(su.gather(dd, c), embed(g[2], bx, xn))
    eq(su.gather(dd, d), embed(g[3], bx, rn))
    for h, nxt, want in ((a, False, g[0]), (b, False, g[1]), (a, True, g[6]), (b, True, g[7])):
        eq(su.gather(dd, h, from_next=nxt), want)
    # z is r (the unpreconditioned solver), t = Next(r), y = Next(a), rhat = e
    fill()
    su.scatter(dd, d, g[5], to_next=True)
    xn, rn, vals = oracle_bicgstab_update(g[6], g[3], g[2], g[3], g[5], g[4], bx)
    assert update(Next(a), d, c, d, Next(d), e) == vals
    eq(su.gather(dd, c), embed(g[2], bx, xn))
    eq(su.gather(dd, d), embed(g[3], bx, rn))
    eq(su.gather(dd, d, from_next=True), g[5])
    eq(su.gather(dd, e), g[4])
