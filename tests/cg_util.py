"""Shared helpers of the conjugate-gradient tests (test_cg_cpu.py,
test_gpu_cg.py): the solver cases, the boundary-aware truth operator in
numpy's wide type, and domain set-up for the vector operations."""
import numpy as np

import stencil_amd as sa
from stencil_amd import Boundary
from stencil_amd.models.poisson3d import Poisson3D

import boundary_util
import stencil_util as su

DTYPES = [np.float32, np.float64]
DT_IDS = ["f32", "f64"]
TOL = {np.float32: 1e-5, np.float64: 1e-10}
MAX_ITER = 300

_KINDS = {
    "periodic": None,
    "fixed0": boundary_util.all_faces(Boundary.FIXED, 0),
    "antimirror": boundary_util.all_faces(Boundary.ANTIMIRROR, 0),
    "mirror": boundary_util.all_faces(Boundary.MIRROR, 0),
}

# (size, order, sigma, boundary, gpus)
SOLVER_CASES = [
    ((19, 10, 9), 2, 1.0, "periodic", [0]),
    ((19, 10, 9), 8, 0.5, "periodic", [0, 0]),
    ((17, 9, 33), 2, 0.0, "fixed0", [0, 0]),
    ((17, 9, 33), 4, 0.0, "antimirror", [0]),
    ((19, 10, 9), 4, 0.25, "mirror", [0, 0]),
]


def case_id(c):
    size, order, sigma, bc, gpus = c
    return f"{'x'.join(map(str, size))}-o{order}-s{sigma}-{bc}-{len(gpus)}dom"


def kinds_of(bc):
    return _KINDS[bc]


def pad_array(g, radius, kinds):
    """the global array g padded by the face radii, one axis at a time in
    the order x, y, z, with the numpy pad modes of boundary_util
    (padded_global does the same for its ripple field only)"""
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


def norm2(a):
    return np.sqrt((a * a).sum())


def true_rel_residual(x, b, stencil, kinds):
    """||b - A x|| / ||b|| from the gathered x, in the wide type"""
    wide = su._wide(b.dtype)
    res = b.astype(wide) - apply_true(x, stencil, kinds)
    return float(norm2(res) / norm2(b.astype(wide)))


def solve_case(backend, case, dtype):
    """(CGResult, x, b, app) of one SOLVER_CASES entry"""
    size, order, sigma, bc, gpus = case
    app = Poisson3D(size, order=order, dtype=dtype, sigma=sigma, backend=backend, gpus=gpus,
                    boundary=kinds_of(bc))
    app.realize()
    b = su.normal_global(size, dtype)
    app.set_rhs(b)
    res = app.solve(tol=TOL[dtype], max_iter=MAX_ITER)
    return res, app.solution(), b, app


def check_solution(res, x, b, app, case, dtype, what):
    tol = TOL[dtype]
    true = true_rel_residual(x, b, app.stencil, kinds_of(case[3]))
    print(f"{what} {case_id(case)} {np.dtype(dtype).name}: {res.iterations} iterations, "
          f"recursive {res.residuals[-1]:.3e} true {true:.3e} (tol {tol:.0e})")
    assert res.converged, res.reason
    assert res.residuals[0] == 1.0
    assert res.residuals[-1] <= tol
    assert len(res.residuals) == res.iterations + 1
    assert true <= 2 * tol


def vector_domain(size, dtypes, backend, gpus, radius=1):
    """a periodic domain with one quantity per entry of dtypes"""
    return su.make_domain(size, sa.Radius.constant(radius), dtypes, backend, gpus)
