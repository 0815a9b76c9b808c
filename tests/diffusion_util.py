"""Shared helpers of the variable-coefficient diffusion tests
(test_diffusion_cpu.py, test_gpu_diffusion.py): an independent numpy oracle
of the operator, written from its definition

    (A u)(p) = sigma u(p) + sum over a in {x,y,z}, s in {-1,+1} of
               h_a * 0.5 (k(p) + k(p + s e_a)) * (u(p) - u(p + s e_a))
    diag(p)  = sigma + sum over a, s of  h_a * 0.5 (k(p) + k(p + s e_a))

(h_a = 1 / spacing_a^2), of the V-cycle built on it (per-cell
w = omega / diag, k restricted by the mean of the 8 children, spacing
doubled per level) and of plain / preconditioned CG; the solver cases.

The oracle works on global (z, y, x) arrays: u is padded with
cg_util.pad_array (its boundary kinds are the boundary conditions), k with
np.pad mode "edge" (CLAMP) or "wrap" (a periodic axis). As in mg_util it
runs in one `work` type: the quantity's own or numpy's wide type of it.
"""

import numpy as np

from stencil_amd import Stencil
from stencil_amd.models.poisson3d import Poisson3D

import cg_util as cu
import mg_util as mu
import stencil_util as su

MAX_ITER = 800
RADIUS1 = Stencil.laplacian(2).radius()  # faces 1


# ---- coefficient fields, (z, y, x), fp64 ----
def k_smooth(size):
    nx, ny, nz = size
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return np.exp(1.5 * np.sin(2 * np.pi * x / nx) * np.cos(2 * np.pi * y / ny)
                  + 0.5 * np.sin(2 * np.pi * z / nz))


def k_jump(size, contrast=16.0):
    nx, ny, nz = size
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return np.where((x >= nx / 2) & (y < ny / 2), contrast, 1.0)


K_FIELDS = {"smooth": k_smooth, "jump": k_jump}

# (size (x, y, z), sigma, boundary, k field, gpus): the eight rows of the
# prototype's table
DIFF_CASES = [
    ((32, 16, 16), 0.0, "fixed0", "smooth", [0]),
    ((32, 16, 16), 0.0, "fixed0", "jump", [0, 0]),
    ((32, 16, 16), 1e-3, "periodic", "smooth", [0, 0]),
    ((32, 16, 16), 1e-3, "periodic", "jump", [0]),
    ((32, 32, 16), 0.0, "antimirror", "smooth", [0, 0]),
    ((32, 32, 16), 0.0, "antimirror", "jump", [0]),
    ((24, 16, 16), 0.01, "mirror", "smooth", [0]),
    ((24, 16, 16), 0.01, "mirror", "jump", [0, 0]),
]


def case_id(c):
    size, sigma, bc, kf, gpus = c
    return f"{'x'.join(map(str, size))}-s{sigma}-{bc}-{kf}-{len(gpus)}dom"


def case_k(case, dtype):
    """the case's coefficient, rounded to the quantity's type"""
    return K_FIELDS[case[3]](case[0]).astype(dtype)


# ---- the operator ----
def pad_k(k, kinds):
    """k padded one cell per face: wrap on a periodic axis, edge otherwise"""
    kinds = kinds or {}
    for a in range(3):
        pw = [(0, 0)] * 3
        pw[2 - a] = (1, 1)
        name = "xyz"[a]
        periodic = name + "-" not in kinds and name + "+" not in kinds
        k = np.pad(k, pw, mode="wrap" if periodic else "edge")
    return k


def _shifted(padded, shape):
    """[(axis, padded shifted by -1, by +1)] over the interior, axis 0 = x"""
    nz, ny, nx = shape
    out = []
    for a in range(3):
        lo, hi = [1, 1, 1], [1, 1, 1]
        lo[a] -= 1
        hi[a] += 1
        out.append((a, padded[lo[2]:lo[2] + nz, lo[1]:lo[1] + ny, lo[0]:lo[0] + nx],
                    padded[hi[2]:hi[2] + nz, hi[1]:hi[1] + ny, hi[0]:hi[0] + nx]))
    return out


def apply_op(u, k, kinds, spacing, sigma, work):
    """A u in the type `work`, boundary included"""
    u, k = u.astype(work), k.astype(work)
    pu, pk = cu.pad_array(u, RADIUS1, kinds), pad_k(k, kinds)
    out = work(sigma) * u
    for (a, um, up), (_, km, kp) in zip(_shifted(pu, u.shape), _shifted(pk, u.shape)):
        h = work(1.0 / (spacing[a] * spacing[a]))
        out = out + h * (work(0.5) * (k + km)) * (u - um)
        out = out + h * (work(0.5) * (k + kp)) * (u - up)
    assert out.dtype == np.dtype(work)
    return out


def diagonal(k, kinds, spacing, sigma, work):
    k = k.astype(work)
    out = np.full(k.shape, sigma, dtype=work)
    for a, km, kp in _shifted(pad_k(k, kinds), k.shape):
        h = work(1.0 / (spacing[a] * spacing[a]))
        out = out + h * (work(0.5) * (k + km)) + h * (work(0.5) * (k + kp))
    return out


# ---- the cycle and the solvers ----
class DiffCycleOracle:
    def __init__(self, k, sigma, kinds, work, levels, nu=mu.NU, omega=mu.OMEGA,
                 coarse_sweeps=mu.COARSE_SWEEPS, spacing=(1.0, 1.0, 1.0)):
        self.work, self.kinds, self.nu, self.coarse_sweeps = work, kinds, nu, coarse_sweeps
        self.sigma = sigma
        self.k, self.spacing, self.w = [k.astype(work)], [tuple(spacing)], []
        for _ in range(levels - 1):
            self.k.append(mu.restrict_mean(self.k[-1]))
            self.spacing.append(tuple(2.0 * s for s in self.spacing[-1]))
        for kl, sp in zip(self.k, self.spacing):
            self.w.append(work(omega) / diagonal(kl, kinds, sp, sigma, work))

    def A(self, l, e):
        return apply_op(e, self.k[l], self.kinds, self.spacing[l], self.sigma, self.work)

    def cycle(self, f, l=0):
        """M f"""
        f = f.astype(self.work)
        w, last = self.w[l], l == len(self.k) - 1
        e = w * f
        for _ in range((self.coarse_sweeps if last else self.nu) - 1):
            e = e + w * (f - self.A(l, e))
        if not last:
            e = e + mu.prolong(self.cycle(mu.restrict_mean(f - self.A(l, e)), l + 1))
            for _ in range(self.nu):
                e = e + w * (f - self.A(l, e))
        assert e.dtype == np.dtype(self.work)
        return e


class JacobiOracle(DiffCycleOracle):
    """M = D^-1: one level, omega 1, no sweep beyond the first"""

    def __init__(self, k, sigma, kinds, work):
        super().__init__(k, sigma, kinds, work, 1, omega=1.0, coarse_sweeps=1)


def cg_oracle(oracle, b, tol, max_iter=MAX_ITER):
    """plain CG in oracle.work with fp64 inner products: the iteration count"""
    work = oracle.work
    b = b.astype(work)
    x, r = np.zeros_like(b), b.copy()
    p = r.copy()
    bb = rr = mu._dot(b, b)
    for it in range(1, max_iter + 1):
        ap = oracle.A(0, p)
        alpha = work(rr / mu._dot(p, ap))
        x, r = x + alpha * p, r - alpha * ap
        rr_new = mu._dot(r, r)
        if rr_new <= tol * tol * bb:
            return it
        p = r + work(rr_new / rr) * p
        rr = rr_new
    return max_iter


_CACHE = {}


def _cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def levels_of(case):
    return mu.num_levels(case[0], gpus_x=len(case[4]))


def case_oracle(case, dtype, work, jacobi=False):
    size, sigma, bc, kf, gpus = case
    k = case_k(case, dtype)
    if jacobi:
        return JacobiOracle(k, sigma, cu.kinds_of(bc), work)
    return DiffCycleOracle(k, sigma, cu.kinds_of(bc), work, levels_of(case))


def oracle_iterations(case, dtype, what):
    """iteration count of the own-type numpy oracle: what = plain | jacobi | mg"""
    def make():
        b = su.normal_global(case[0], dtype)
        own = np.dtype(dtype).type
        tol = cu.TOL[dtype]
        if what == "plain":
            return cg_oracle(case_oracle(case, dtype, own), b, tol)
        return mu.pcg_oracle(case_oracle(case, dtype, own, jacobi=what == "jacobi"), b, tol,
                             max_iter=MAX_ITER)[0]

    return _cached(("it", what, case_id(case), np.dtype(dtype).name), make)


def cycle_reference(case, dtype):
    """(r, M r in the wide type, relative L2 error of the own-type oracle)"""
    def make():
        r = su.normal_global(case[0], dtype, seed=11)
        wide = su._wide(dtype)
        ref = case_oracle(case, dtype, wide).cycle(r)
        own = case_oracle(case, dtype, np.dtype(dtype).type).cycle(r)
        assert own.dtype == np.dtype(dtype)
        return r, ref, float(cu.norm2(own.astype(wide) - ref) / cu.norm2(ref))

    return _cached(("cycle", case_id(case), np.dtype(dtype).name), make)


def make_app(backend, case, dtype, preconditioner, k=None):
    size, sigma, bc, kf, gpus = case
    app = Poisson3D(size, dtype=dtype, sigma=sigma, backend=backend, gpus=gpus,
                    boundary=cu.kinds_of(bc), preconditioner=preconditioner, coefficient=True)
    app.realize()
    app.set_coefficient(case_k(case, dtype) if k is None else k)
    return app


def solve_case(backend, case, dtype, preconditioner):
    """(CGResult, x, b, app)"""
    def make():
        app = make_app(backend, case, dtype, preconditioner)
        b = su.normal_global(case[0], dtype)
        app.set_rhs(b)
        res = app.solve(tol=cu.TOL[dtype], max_iter=MAX_ITER)
        return res, app.solution(), b, app

    return _cached(("solve", backend, preconditioner, case_id(case), np.dtype(dtype).name), make)


def check_solution(res, x, b, case, dtype, what):
    """cg_util.check_solution with the oracle operator as the truth"""
    size, sigma, bc, kf, gpus = case
    tol, wide = cu.TOL[dtype], su._wide(dtype)
    ax = apply_op(x, case_k(case, dtype), cu.kinds_of(bc), (1.0, 1.0, 1.0), sigma, wide)
    true = float(cu.norm2(b.astype(wide) - ax) / cu.norm2(b.astype(wide)))
    print(f"{what} {case_id(case)} {np.dtype(dtype).name}: {res.iterations} iterations, "
          f"recursive {res.residuals[-1]:.3e} true {true:.3e} (tol {tol:.0e})")
    assert res.converged, res.reason
    assert res.residuals[0] == 1.0
    assert res.residuals[-1] <= tol
    assert len(res.residuals) == res.iterations + 1
    assert true <= 2 * tol


SOLVERS = {"plain": None, "jacobi": "jacobi", "mg": "multigrid"}


def check_solve(backend, case, dtype, solver):
    """one solve (plain | jacobi | mg): converged on the recursive residual,
    and the true residual in the wide type within 2 tol"""
    res, x, b, _ = solve_case(backend, case, dtype, SOLVERS[solver])
    check_solution(res, x, b, case, dtype, f"{backend} {solver}")


def check_iterations(backend, case, dtype):
    """the iteration conditions of one case: 2 jacobi <= plain,
    4 mg <= jacobi, mg <= oracle + 2, and the number of levels"""
    its = {}
    for name, pre in SOLVERS.items():
        res, _, _, app = solve_case(backend, case, dtype, pre)
        assert res.converged, (name, res.reason)
        its[name] = res.iterations
        if pre == "multigrid":
            assert len(app.mg.levels) == levels_of(case)
    want = oracle_iterations(case, dtype, "mg")
    print(f"iterations {its}, numpy oracle mg {want}")
    assert 2 * its["jacobi"] <= its["plain"]
    assert 4 * its["mg"] <= its["jacobi"]
    assert its["mg"] <= want + 2


def check_cycle(backend, case, dtype):
    """z = M r against the wide oracle: at most 8 x the own-type oracle's
    error, as mg_util.check_cycle"""
    r, ref, own_err = cycle_reference(case, dtype)
    app = make_app(backend, case, dtype, "multigrid")
    su.scatter(app.dd, app.r, r)
    app.mg.apply(app.r, app.z)
    app.dd.backend.sync_compute()
    z = su.gather(app.dd, app.z)
    err = float(cu.norm2(z.astype(ref.dtype) - ref) / cu.norm2(ref))
    print(f"{backend} cycle {case_id(case)} {np.dtype(dtype).name}: relative L2 error "
          f"{err:.3e}, the own-type oracle's {own_err:.3e} (bound {8 * own_err:.3e})")
    np.testing.assert_array_equal(su.gather(app.dd, app.r), r)  # f is read only
    assert np.isfinite(z).all()
    assert err <= 8 * own_err


# ---- the operator on one allocation (kernel tests) ----
def _block_neighbours(whole, lo, hi):
    """[(axis, the box [lo, hi) of `whole` shifted by -1, by +1)], axis 0 = x;
    lo / hi are (x, y, z) allocation coordinates"""
    out = []
    for a in range(3):
        views = []
        for s in (-1, 1):
            l, h = list(lo), list(hi)
            l[a] += s
            h[a] += s
            views.append(whole[l[2]:h[2], l[1]:h[1], l[0]:h[0]])
        out.append((a, views[0], views[1]))
    return out


def apply_block(wu, wk, lo, hi, h, sigma, work):
    """(A u, sum of the magnitudes of its seven terms) over the box of two
    whole-allocation arrays, in the type `work`; reads the box and its six
    face neighbours only"""
    wu, wk = wu.astype(work), wk.astype(work)
    u, k = (w[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]] for w in (wu, wk))
    out = work(sigma) * u
    mag = np.abs(out)
    for (a, um, up), (_, km, kp) in zip(_block_neighbours(wu, lo, hi),
                                        _block_neighbours(wk, lo, hi)):
        for un, kn in ((um, km), (up, kp)):
            term = work(h[a]) * (work(0.5) * (k + kn)) * (u - un)
            out = out + term
            mag = mag + np.abs(term)
    return out, mag


def diagonal_block(wk, lo, hi, h, sigma, work):
    wk = wk.astype(work)
    k = wk[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]]
    out = np.full(k.shape, sigma, dtype=work)
    for a, km, kp in _block_neighbours(wk, lo, hi):
        out = out + work(h[a]) * (work(0.5) * (k + km)) + work(h[a]) * (work(0.5) * (k + kp))
    return out


def cross_mask(shape_zyx, lo, hi):
    """True on the box and its six face neighbours, False elsewhere (edge
    and corner neighbours included)"""
    m = np.zeros(shape_zyx, dtype=bool)
    for a in range(3):
        l, h = list(lo), list(hi)
        l[a] -= 1
        h[a] += 1
        m[l[2]:h[2], l[1]:h[1], l[0]:h[0]] = True
    return m


# ---- exact data of the kernel tests ----
def int_k(shape_zyx, dtype, seed):
    """integers in [1, 16]"""
    return np.random.default_rng(seed).integers(1, 17, size=shape_zyx).astype(dtype)


H_VALUES = [0.25, 0.5, 1.0, 2.0]
