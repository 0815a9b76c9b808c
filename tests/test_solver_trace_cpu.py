"""The backend calls of the solvers pinned across changes of their
scaffolding (stencil_amd/solvers/): same operations, same syncs, same
exchanges, in the same order.

A recording proxy stands in the place of `dd.backend` (torch backend, CPU)
and logs the name of every backend method the solver calls, in order;
`exchange` with its group, `stencil_apply` / `diffusion_apply` with their
compute stream id. tests/golden/solver_call_traces.json holds the traces of
the commit named in its "commit" entry. Equality.

No trace depends on rounding. The loops run with tol=0.0, max_iter=3 on
sigma I - laplacian(2) at 12 x 10 x 8 in two local domains and end in
"max_iter". The verify / correction exits run on the centre-only stencil
A = 2 I with small-integer b: alpha = 0.5, x = b / 2 and the residual 0 are
exact, so the solve converges in one iteration and the true residual is 0.

To record the file again (only where a change of the calls is intended):
    python tests/test_solver_trace_cpu.py <commit> <out.json>
"""
import inspect
import json
import sys
from pathlib import Path

import numpy as np
import pytest

GOLDEN = Path(__file__).resolve().parent / "golden" / "solver_call_traces.json"
SIZE = (12, 10, 8)
_ARG_LOGGED = {"exchange": "group", "stencil_apply": "stream_id", "diffusion_apply": "stream_id"}


class Recorder:
    """forwards everything to `backend`; logs the public methods called"""

    def __init__(self, backend, log):
        self._backend, self._log = backend, log

    def __getattr__(self, name):
        attr = getattr(self._backend, name)
        if name.startswith("_") or not callable(attr):
            return attr

        def call(*args, **kwargs):
            entry = name
            if name in _ARG_LOGGED:
                bound = inspect.signature(attr).bind(*args, **kwargs)
                bound.apply_defaults()
                entry += f"({_ARG_LOGGED[name]}={bound.arguments[_ARG_LOGGED[name]]})"
            self._log.append(entry)
            return attr(*args, **kwargs)

        return call


def _record(dd, run):
    log = []
    real = dd.backend
    dd.backend = Recorder(real, log)
    try:
        out = run()
    finally:
        dd.backend = real
    return log, out


def _poisson(**kw):
    from stencil_amd.models.poisson3d import Poisson3D

    import stencil_util as su

    app = Poisson3D(SIZE, order=2, dtype=np.float64, backend="torch", gpus=[0, 0], **kw)
    app.realize()
    app.set_rhs(su.normal_global(SIZE, np.float64))
    return app


def _loop(app, reason="max_iter", **solve_kw):
    log, res = _record(app.dd, lambda: app.solve(tol=0.0, max_iter=3, **solve_kw))
    assert (res.reason, res.iterations) == (reason, 3), res
    return log


def _domain(n, groups):
    """a periodic radius-1 domain of n float64 quantities in two local
    domains and the small-integer right-hand side of the exact cases"""
    import stencil_amd as sa

    dd = sa.DistributedDomain(*SIZE, backend="torch")
    dd.set_radius(sa.Radius.constant(1))
    dd.set_gpus([0, 0])
    hs = [dd.add_data(np.float64, f"q{i}") for i in range(n)]
    dd.set_exchange_groups(groups)
    dd.realize()
    b = np.random.default_rng(5).integers(1, 9, size=(SIZE[2], SIZE[1], SIZE[0])).astype(np.float64)
    return dd, hs, b


def _helmholtz():
    from stencil_amd import Stencil

    return Stencil.identity() - Stencil.laplacian(2)


def _two_identity():
    from stencil_amd import Stencil

    return 2.0 * Stencil.identity()


class _Copy:
    """the identity as a preconditioner: e = f"""

    def __init__(self, dd):
        self.dd = dd

    def apply(self, f, e):
        self.dd.axpby(1.0, f, 0.0, f, out=e)


def _cg_plain():
    return _loop(_poisson(sigma=1.0))


def _cg_no_overlap():
    return _loop(_poisson(sigma=1.0), overlap=False)


def _cg_jacobi():
    return _loop(_poisson(sigma=1.0, coefficient=True, preconditioner="jacobi"))


def _cg_nullspace():
    return _loop(_poisson(sigma=0.0, nullspace="constant"))


def _cg_correction_exact():
    from stencil_amd.solvers import ConjugateGradient

    import stencil_util as su

    dd, (x, b, r, p, d), gb = _domain(5, [[3], [0]])
    su.scatter(dd, b, gb)
    cg = ConjugateGradient(dd, _two_identity(), x, b, r, p, group_p=0, group_x=1, correction=d)
    log, res = _record(dd, lambda: cg.solve(tol=0.0, max_iter=3))
    assert (res.reason, res.iterations, res.residuals) == ("converged", 1, [1.0, 0.0]), res
    assert cg.corrections == 0
    np.testing.assert_array_equal(su.gather(dd, x), 0.5 * gb)
    return log


def _cg_zero_rhs():
    app = _poisson(sigma=1.0)
    app.set_rhs(np.zeros((SIZE[2], SIZE[1], SIZE[0])))
    log, res = _record(app.dd, lambda: app.solve(tol=0.0, max_iter=3))
    assert res.reason == "zero_rhs"
    return log


def _bicgstab(A, n=5, pre=False, group_x=2, b=None):
    from stencil_amd.solvers import BiCGStab

    import stencil_util as su

    # x, b, r, rhat, p (, y, z): p^, s^ and x in a group each
    dd, hs, gb = _domain(n, [[5], [6], [0]] if pre else [[4], [2], [0]])
    su.scatter(dd, hs[1], gb if b is None else b)
    kw = dict(preconditioner=_Copy(dd), y=hs[5], z=hs[6]) if pre else {}
    solver = BiCGStab(dd, A, *hs[:5], 0, 1, group_x, **kw)
    log, res = _record(dd, lambda: solver.solve(tol=0.0, max_iter=3))
    return log, res, solver, su.gather(dd, hs[0]), gb


def _bicgstab_plain():
    import stencil_util as su

    log, res, *_ = _bicgstab(_helmholtz(), b=su.normal_global(SIZE, np.float64))
    assert (res.reason, res.iterations) == ("max_iter", 3), res
    return log


def _bicgstab_preconditioned():
    import stencil_util as su

    log, res, *_ = _bicgstab(_helmholtz(), n=7, pre=True, b=su.normal_global(SIZE, np.float64))
    assert (res.reason, res.iterations) == ("max_iter", 3), res
    return log


def _bicgstab_verify_exact():
    log, res, solver, x, gb = _bicgstab(_two_identity())
    assert (res.reason, res.iterations, res.residuals) == ("converged", 1, [1.0, 0.0]), res
    assert solver.restarts == 0
    np.testing.assert_array_equal(x, 0.5 * gb)
    return log


def _bicgstab_zero_rhs():
    log, res, *_ = _bicgstab(_helmholtz(), b=np.zeros((SIZE[2], SIZE[1], SIZE[0])))
    assert res.reason == "zero_rhs"
    return log


def _multigrid_apply():
    import stencil_util as su

    app = _poisson(sigma=1.0, preconditioner="multigrid")
    assert app.mg.levels == [SIZE, (6, 5, 4)]
    su.scatter(app.dd, app.r, su.normal_global(SIZE, np.float64, seed=11))
    log, _ = _record(app.dd, lambda: app.mg.apply(app.r, app.z))
    return log


CASES = {
    "cg-plain": _cg_plain,
    "cg-no-overlap": _cg_no_overlap,
    "cg-jacobi-z": _cg_jacobi,
    "cg-nullspace-constant": _cg_nullspace,
    "cg-correction-2I": _cg_correction_exact,
    "cg-zero-rhs": _cg_zero_rhs,
    "bicgstab-plain": _bicgstab_plain,
    "bicgstab-preconditioned": _bicgstab_preconditioned,
    "bicgstab-verify-2I": _bicgstab_verify_exact,
    "bicgstab-zero-rhs": _bicgstab_zero_rhs,
    "multigrid-apply-fine-level": _multigrid_apply,
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_solver_issues_the_recorded_backend_calls(case):
    want = json.loads(GOLDEN.read_text())["traces"][case]
    got = CASES[case]()
    assert got == want


if __name__ == "__main__":
    here = Path(__file__).resolve().parent
    sys.path[:0] = [str(here.parent), str(here)]
    commit, path = sys.argv[1:]
    traces = {c: CASES[c]() for c in sorted(CASES)}
    Path(path).write_text(json.dumps({"commit": commit, "traces": traces}, indent=1,
                                     sort_keys=True) + "\n")
