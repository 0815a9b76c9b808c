"""Shared helpers of the multigrid tests (test_mg_cpu.py, test_gpu_mg.py):
an independent numpy oracle of the V-cycle and of preconditioned CG, written
from the definition in stencil_amd/solvers/multigrid.py, the solver cases
and the exact oracles of the grid-transfer kernels.

The oracle works on global (z, y, x) arrays. It runs in one `work` type:
the quantity's own type (coefficients and stencil weights rounded to it, as
the library does) or numpy's wide type of it (float64 for float32,
longdouble for float64; nothing rounded), which stands for exact
arithmetic. A is applied through cg_util.pad_array, so the boundary kinds
are the operator's boundary conditions on every level.
"""
import math

import numpy as np

from stencil_amd import Stencil
from stencil_amd.models.poisson3d import Poisson3D

import cg_util as cu
import stencil_util as su

# (size, order, sigma, boundary, gpus)
MG_CASES = [
    ((32, 32, 32), 2, 0.0, "fixed0", [0]),
    ((32, 16, 16), 2, 1e-3, "periodic", [0, 0]),
    ((32, 32, 16), 4, 0.0, "antimirror", [0, 0]),
    ((24, 16, 16), 2, 0.01, "mirror", [0]),
    ((32, 32, 32), 8, 0.5, "periodic", [0]),
]
NU, OMEGA, COARSE_SWEEPS = 2, 2.0 / 3.0, 8


def operator_at(order, sigma, level, coarse_order=2):
    st = -Stencil.laplacian(order if level == 0 else coarse_order, (2.0 ** level,) * 3)
    return st + sigma * Stencil.identity() if sigma != 0.0 else st


def apply_op(g, stencil, kinds, work):
    """A g in the type `work`, boundary included"""
    radius = stencil.radius()
    padded = cu.pad_array(g.astype(work), radius, kinds)
    off = (radius.x(-1), radius.y(-1), radius.z(-1))
    nz, ny, nx = g.shape
    out = np.zeros(g.shape, dtype=work)
    for (dx, dy, dz), w in zip(stencil.offsets, stencil.weights):
        out += work(w) * padded[off[2] + dz:off[2] + dz + nz, off[1] + dy:off[1] + dy + ny,
                                off[0] + dx:off[0] + dx + nx]
    return out


def restrict_mean(v):
    """the mean over the 8 children, in v's type"""
    nz, ny, nx = (n // 2 for n in v.shape)
    s = v.reshape(nz, 2, ny, 2, nx, 2)
    acc = np.zeros((nz, ny, nx), dtype=v.dtype)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                acc += s[:, dz, :, dy, :, dx]
    return acc * v.dtype.type(0.125)


def prolong(c):
    """every coarse cell copied to its 8 children"""
    return np.repeat(np.repeat(np.repeat(c, 2, axis=0), 2, axis=1), 2, axis=2)


def num_levels(size, gpus_x=1, max_levels=None):
    """the library's coarsening rule for subdomains split in x only and
    operators of radius <= 2 on the coarse levels"""
    n, size = 1, tuple(size)
    while max_levels is None or n < max_levels:
        sub = (size[0] // gpus_x, size[1], size[2])
        if any(c % 2 for c in size + sub) or any(c // 2 < 2 for c in sub):
            break
        size = tuple(c // 2 for c in size)
        n += 1
    return n


class CycleOracle:
    def __init__(self, size, order, sigma, kinds, work, levels, nu=NU, omega=OMEGA,
                 coarse_sweeps=COARSE_SWEEPS, coarse_order=2):
        self.work, self.kinds, self.nu, self.coarse_sweeps = work, kinds, nu, coarse_sweeps
        self.ops = [operator_at(order, sigma, l, coarse_order) for l in range(levels)]
        self.w = []
        for A in self.ops:
            centre = dict(zip(A.offsets, A.weights))[(0, 0, 0)]
            self.w.append(work(omega / centre))

    def A(self, l, e):
        return apply_op(e, self.ops[l], self.kinds, self.work)

    def cycle(self, f, l=0):
        """M f"""
        f = f.astype(self.work)
        w, last = self.w[l], l == len(self.ops) - 1
        e = w * f
        for _ in range((self.coarse_sweeps if last else self.nu) - 1):
            e = e + w * f - w * self.A(l, e)
        if not last:
            e = e + prolong(self.cycle(restrict_mean(f - self.A(l, e)), l + 1))
            for _ in range(self.nu):
                e = e + w * f - w * self.A(l, e)
        assert e.dtype == self.work
        return e


def _dot(a, b):
    return float((a.astype(np.float64) * b.astype(np.float64)).sum())


def pcg_oracle(oracle, b, tol, max_iter=300):
    """preconditioned CG in oracle.work with fp64 inner products, as the
    library: the iteration count and the relative recursive residuals"""
    work = oracle.work
    b = b.astype(work)
    x = np.zeros_like(b)
    r = b.copy()
    bb = rr = _dot(b, b)
    limit = tol * tol * bb
    z = oracle.cycle(r)
    p = z.copy()
    rz = _dot(r, z)
    residuals = [1.0]
    for it in range(1, max_iter + 1):
        ap = oracle.A(0, p)
        alpha = work(rz / _dot(p, ap))
        x = x + alpha * p
        r = r - alpha * ap
        rr = _dot(r, r)
        residuals.append(math.sqrt(rr / bb))
        if rr <= limit:
            return it, residuals
        z = oracle.cycle(r)
        rz_new = _dot(r, z)
        p = z + work(rz_new / rz) * p
        rz = rz_new
    return max_iter, residuals


# ---- references computed once per (case, dtype) and shared ----
_CACHE = {}


def _cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def case_oracle(case, work):
    size, order, sigma, bc, gpus = case
    return CycleOracle(size, order, sigma, cu.kinds_of(bc), work,
                       num_levels(size, gpus_x=len(gpus)))


def cycle_reference(case, dtype):
    """(r, M r in the wide type, relative L2 error of the oracle run in the
    quantity's own type against it) for the seeded normal r"""
    def make():
        r = su.normal_global(case[0], dtype, seed=11)
        wide = su._wide(dtype)
        ref = case_oracle(case, wide).cycle(r)
        own = case_oracle(case, np.dtype(dtype).type).cycle(r)
        assert own.dtype == np.dtype(dtype)
        err = float(cu.norm2(own.astype(wide) - ref) / cu.norm2(ref))
        return r, ref, err

    return _cached(("cycle", cu.case_id(case), np.dtype(dtype).name), make)


def oracle_iterations(case, dtype):
    def make():
        b = su.normal_global(case[0], dtype)
        return pcg_oracle(case_oracle(case, np.dtype(dtype).type), b, cu.TOL[dtype])[0]

    return _cached(("pcg", cu.case_id(case), np.dtype(dtype).name), make)


def solve_case(backend, case, dtype, preconditioner):
    """(CGResult, x, b, app) of one MG_CASES entry, plain or preconditioned"""
    size, order, sigma, bc, gpus = case
    app = Poisson3D(size, order=order, dtype=dtype, sigma=sigma, backend=backend, gpus=gpus,
                    boundary=cu.kinds_of(bc), preconditioner=preconditioner)
    app.realize()
    b = su.normal_global(size, dtype)
    app.set_rhs(b)
    res = app.solve(tol=cu.TOL[dtype], max_iter=cu.MAX_ITER)
    return res, app.solution(), b, app


def plain_iterations(backend, case, dtype):
    return _cached(("plain", backend, cu.case_id(case), np.dtype(dtype).name),
                   lambda: solve_case(backend, case, dtype, None)[0].iterations)


def check_mg_solve(backend, case, dtype):
    res, x, b, app = solve_case(backend, case, dtype, "multigrid")
    cu.check_solution(res, x, b, app, case, dtype, f"{backend} mg")
    plain = plain_iterations(backend, case, dtype)
    want = oracle_iterations(case, dtype)
    print(f"levels {app.mg.levels}: {res.iterations} iterations, plain CG {plain}, "
          f"numpy oracle {want}")
    assert len(app.mg.levels) == num_levels(case[0], gpus_x=len(case[4]))
    assert 3 * res.iterations <= plain
    assert res.iterations <= want + 2


def check_cycle(backend, case, dtype):
    """z = M r of the library against the wide oracle: at most 8 x the
    error of the oracle run in the quantity's own type (the factor covers
    summation order and FMA contraction)"""
    size, order, sigma, bc, gpus = case
    r, ref, own_err = cycle_reference(case, dtype)
    app = Poisson3D(size, order=order, dtype=dtype, sigma=sigma, backend=backend, gpus=gpus,
                    boundary=cu.kinds_of(bc), preconditioner="multigrid")
    app.realize()
    su.scatter(app.dd, app.r, r)
    app.mg.apply(app.r, app.z)
    app.dd.backend.sync_compute()
    z = su.gather(app.dd, app.z)
    err = float(cu.norm2(z.astype(ref.dtype) - ref) / cu.norm2(ref))
    print(f"{backend} cycle {cu.case_id(case)} {np.dtype(dtype).name}: relative L2 error "
          f"{err:.3e}, the own-type oracle's {own_err:.3e} (bound {8 * own_err:.3e})")
    np.testing.assert_array_equal(su.gather(app.dd, app.r), r)  # f is read only
    assert np.isfinite(z).all()
    assert err <= 8 * own_err
    return app


# ---- exact data of the kernel tests: integers below 753 ----
def int_field(shape_zyx, dtype, seed):
    """integers in [0, 753), as the ripple fields of test_gpu_cg.py"""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 753, size=shape_zyx).astype(dtype)
