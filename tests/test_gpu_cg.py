"""Vector operations and the conjugate-gradient solver on the GPU
(csrc/src/vector_ops.hip): dot / axpby / cg_update against exact numpy
oracles, their containment contract, determinism and validation, and the
native solver against the boundary-aware truth operator."""
import numpy as np
import pytest

from stencil_amd import Next, _C
from stencil_amd.models.poisson3d import Poisson3D

import cg_util as cu
import stencil_util as su
from util import full_region_of

pytestmark = pytest.mark.gpu

DTYPES, DT_IDS = cu.DTYPES, cu.DT_IDS

# the R1_SHAPES of test_gpu_stencil.py: x 8..19 gives tail 0..3 (and head
# 0..3 once the box start moves, see X0S), y 4..7 rows cut off at the block
# edge, z 3 / 33 / 65 several z chunks (a thread marches at least 4 planes).
# 261 x 5 x 3: 65 strips + 1 tail lane in fp32, 130 strips in fp64: a row
# spans more than one 64-lane block in x.
ZC = 32
R1_SHAPES = [
    (8, 4, 3),
    (9, 5, ZC + 1),
    (10, 6, 2 * ZC + 1),
    (11, 7, 3),
    (13, 4, ZC + 1),
    (19, 5, 2 * ZC + 1),
    (8, 7, ZC + 1),
    (19, 6, 3),
    (261, 5, 3),
]
X0S = [0, 1, 2, 3]  # box start in x: head = 0, 3, 2, 1 cells in fp32 (0, 1, 0, 1 in fp64)


def _sid(s):
    return "x".join(map(str, s))


def _second(size, dtype):
    """another integer field below 753"""
    return (su.ripple_global(size, dtype)[::-1, ::-1, ::-1] % 97 + 1).astype(dtype)


def _box(lo, hi):
    return (slice(lo[2], hi[2]), slice(lo[1], hi[1]), slice(lo[0], hi[0]))


def _isum(*arrays):
    """exact integer-valued sum of the product of the arrays, as a float"""
    prod = np.ones(arrays[0].shape, dtype=np.float64)
    for a in arrays:
        prod = prod * a.astype(np.float64)
    return float(prod.sum())


# ------------------------------------------------------------------ exact dot
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("x0", X0S)
@pytest.mark.parametrize("size", R1_SHAPES, ids=_sid)
def test_dot_exact(size, x0, dtype):
    """integers below 753: every product < 2^20, every sum < 2^53, so the
    fp64 result equals the integer sum in any summation order"""
    dd, (a, b) = cu.vector_domain(size, [dtype] * 2, "native", [0])
    ga, gb = su.ripple_global(size, dtype), _second(size, dtype)
    gn = ((ga + gb) % 101).astype(dtype)
    su.scatter(dd, a, ga)
    su.scatter(dd, b, gb)
    su.scatter(dd, b, gn, to_next=True)
    lo, hi = (x0, 0, 0), size
    bx = _box(lo, hi)
    where = "all" if x0 == 0 else (lo, hi)
    assert dd.dot(a, where=where) == _isum(ga[bx], ga[bx])
    assert dd.dot(a, b, where=where) == _isum(ga[bx], gb[bx])
    assert dd.dot(a, Next(b), where=where) == _isum(ga[bx], gn[bx])
    assert dd.dot(Next(b), where=where) == _isum(gn[bx], gn[bx])


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_dot_two_domains(dtype):
    size = (19, 10, 9)
    dd, (a, b) = cu.vector_domain(size, [dtype] * 2, "native", [0, 0])
    assert dd.num_local() == 2
    ga, gb = su.ripple_global(size, dtype), _second(size, dtype)
    su.scatter(dd, a, ga)
    su.scatter(dd, b, gb)
    assert dd.dot(a, b) == _isum(ga, gb)
    assert dd.dot(b) == _isum(gb, gb)


# ---------------------------------------------------------------- exact axpby
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("size", R1_SHAPES, ids=_sid)
def test_axpby_exact(size, dtype):
    """dyadic coefficients on integer data: exact with or without FMA"""
    dd, (a, b, c) = cu.vector_domain(size, [dtype] * 3, "native", [0])
    ga, gb = su.ripple_global(size, dtype), _second(size, dtype)
    want = (0.5 * ga - 0.25 * gb).astype(dtype)
    su.scatter(dd, a, ga)
    su.scatter(dd, b, gb)
    dd.axpby(0.5, a, -0.25, b, out=c)
    dd.axpby(0.5, a, -0.25, b, out=Next(c))  # out in the next buffer
    dd.axpby(0.5, a, -0.25, b, out=Next(a))
    dd.axpby(0.5, a, -0.25, b, out=a)  # out aliases x
    dd.axpby(0.5, Next(a), 0.25, b, out=b)  # out aliases y; x from a next buffer
    dd.backend.sync_compute()
    for h, nxt in ((c, False), (c, True), (a, True), (a, False)):
        np.testing.assert_array_equal(su.gather(dd, h, from_next=nxt).view(np.uint8),
                                      want.view(np.uint8))
    np.testing.assert_array_equal(su.gather(dd, b), (0.5 * want + 0.25 * gb).astype(dtype))


# -------------------------------------------------------------- bounded axpby
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("size", [(19, 10, 9), (261, 5, 3)], ids=_sid)
def test_axpby_bounded(size, dtype):
    """non-dyadic coefficients on normal data: two roundings per cell,
    |err| <= 2 eps (|alpha x| + |beta y|)"""
    alpha, beta = 1.0 / 3.0, -0.7
    dd, (a, b, c) = cu.vector_domain(size, [dtype] * 3, "native", [0])
    ga, gb = su.normal_global(size, dtype, seed=1), su.normal_global(size, dtype, seed=2)
    su.scatter(dd, a, ga)
    su.scatter(dd, b, gb)
    dd.axpby(alpha, a, beta, b, out=c)
    dd.backend.sync_compute()
    wide = su._wide(dtype)
    tx, ty = wide(alpha) * ga.astype(wide), wide(beta) * gb.astype(wide)
    bound = 2 * np.finfo(dtype).eps * (np.abs(tx) + np.abs(ty))
    su.assert_within_bound(su.gather(dd, c), tx + ty, bound, "axpby")


# ---------------------------------------------------------------- containment
CONTRACT_SIZE = (24, 10, 9)
_BOXES = {
    # x start odd; the thin box is narrower than 8 cells (linearised path)
    "wide": ((3, 1, 1), (20, 8, 8)),
    "thin": ((5, 2, 1), (12, 9, 7)),
}
_SENTINELS = {"sentinel": -99.0, "nan": np.nan}


def _sentinel_domain(dtype, nq, sentinel, gpus=(0,)):
    dd, hs = su.make_domain(CONTRACT_SIZE, _C.Radius.constant(2), [dtype] * nq, "native",
                            list(gpus))
    flo, fhi = full_region_of(dd, 0)
    sent = np.full((fhi[2] - flo[2], fhi[1] - flo[1], fhi[0] - flo[0]), sentinel, dtype=dtype)
    for h in hs:
        for to_next in (False, True):
            dd.write_global(0, flo, sent, h, to_next=to_next)
    return dd, hs, flo, fhi, sent


def _put(dd, h, g, lo, hi, to_next=False):
    dd.write_global(0, lo, np.ascontiguousarray(g[_box(lo, hi)]), h, to_next=to_next)


def _expect(sent, flo, lo, hi, g):
    want = sent.copy()
    o = tuple(lo[i] - flo[i] for i in range(3))
    e = tuple(hi[i] - lo[i] for i in range(3))
    want[o[2]:o[2] + e[2], o[1]:o[1] + e[1], o[0]:o[0] + e[0]] = g[_box(lo, hi)]
    return want


def _assert_buffer(dd, flo, fhi, h, nxt, want):
    got = dd.read_global(0, flo, fhi, h, from_next=nxt)
    np.testing.assert_array_equal(got.view(np.uint8), want.view(np.uint8))


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("sentinel", sorted(_SENTINELS))
@pytest.mark.parametrize("box", sorted(_BOXES))
def test_axpby_and_dot_containment(box, sentinel, dtype):
    lo, hi = _BOXES[box]
    dd, (a, b, c), flo, fhi, sent = _sentinel_domain(dtype, 3, _SENTINELS[sentinel])
    ga, gb = su.ripple_global(CONTRACT_SIZE, dtype), _second(CONTRACT_SIZE, dtype)
    _put(dd, a, ga, lo, hi)
    _put(dd, b, gb, lo, hi, to_next=True)
    # no cell outside the box enters the arithmetic: finite and exact
    assert dd.dot(a, Next(b), where=(lo, hi)) == _isum(ga[_box(lo, hi)], gb[_box(lo, hi)])
    dd.axpby(0.5, a, -0.25, Next(b), out=c, where=(lo, hi))
    dd.axpby(2.0, a, 0.5, Next(b), out=a, where=(lo, hi))  # in place
    dd.backend.sync_compute()
    _assert_buffer(dd, flo, fhi, c, False, _expect(sent, flo, lo, hi, 0.5 * ga - 0.25 * gb))
    _assert_buffer(dd, flo, fhi, a, False, _expect(sent, flo, lo, hi, 2.0 * ga + 0.5 * gb))
    _assert_buffer(dd, flo, fhi, b, True, _expect(sent, flo, lo, hi, gb))
    for h, nxt in ((a, True), (b, False), (c, True)):
        _assert_buffer(dd, flo, fhi, h, nxt, sent)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("sentinel", sorted(_SENTINELS))
@pytest.mark.parametrize("box", sorted(_BOXES))
def test_cg_update_containment(box, sentinel, dtype):
    lo, hi = _BOXES[box]
    dd, (x, p, r), flo, fhi, sent = _sentinel_domain(dtype, 3, _SENTINELS[sentinel])
    size = CONTRACT_SIZE
    gx, gp = su.ripple_global(size, dtype), _second(size, dtype)
    gr = ((gx + 2 * gp) % 211).astype(dtype)
    gap = ((3 * gx + gp) % 89).astype(dtype)
    _put(dd, x, gx, lo, hi)
    _put(dd, p, gp, lo, hi)
    _put(dd, p, gap, lo, hi, to_next=True)
    _put(dd, r, gr, lo, hi)
    alpha = 0.25
    # the op takes local_rect at the DistributedDomain level: the box goes
    # through the backend, one (lo, hi) per local domain
    (rr,) = dd.backend.cg_update([(lo, hi)], alpha, x.index, p.index, r.index)
    rn = gr - alpha * gap
    assert rr == float((rn[_box(lo, hi)].astype(np.float64) ** 2).sum())
    _assert_buffer(dd, flo, fhi, x, False, _expect(sent, flo, lo, hi, gx + alpha * gp))
    _assert_buffer(dd, flo, fhi, r, False, _expect(sent, flo, lo, hi, rn))
    _assert_buffer(dd, flo, fhi, p, False, _expect(sent, flo, lo, hi, gp))
    _assert_buffer(dd, flo, fhi, p, True, _expect(sent, flo, lo, hi, gap))
    for h in (x, r):
        _assert_buffer(dd, flo, fhi, h, True, sent)


# ------------------------------------------------- cg_update, the composition
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("gpus", [[0], [0, 0]], ids=["1dom", "2dom"])
@pytest.mark.parametrize("size", [(9, 5, ZC + 1), (19, 5, 2 * ZC + 1), (19, 10, 9), (261, 5, 3)],
                         ids=_sid)
def test_cg_update_exact(size, gpus, dtype):
    """dyadic alpha on integer data: x and r are exact, r_new^2 is a
    multiple of 1/16 and the sum stays far below 2^53 / 16"""
    dd, (x, p, r) = cu.vector_domain(size, [dtype] * 3, "native", gpus)
    gx, gp = su.ripple_global(size, dtype), _second(size, dtype)
    gr = ((gx + 2 * gp) % 211).astype(dtype)
    gap = ((3 * gx + gp) % 89).astype(dtype)
    su.scatter(dd, x, gx)
    su.scatter(dd, p, gp)
    su.scatter(dd, p, gap, to_next=True)
    su.scatter(dd, r, gr)
    alpha = 0.25
    rr = dd.cg_update(alpha, x, p, r)
    rn = (gr - alpha * gap).astype(dtype)
    assert rr == float((rn.astype(np.float64) ** 2).sum())
    np.testing.assert_array_equal(su.gather(dd, x), (gx + alpha * gp).astype(dtype))
    np.testing.assert_array_equal(su.gather(dd, r), rn)
    np.testing.assert_array_equal(su.gather(dd, p), gp)
    np.testing.assert_array_equal(su.gather(dd, p, from_next=True), gap)
    assert rr == dd.dot(r)


# ---------------------------------------------------------------- determinism
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_dot_is_deterministic(dtype):
    size = (61, 19, 37)
    dd, (a, b) = cu.vector_domain(size, [dtype] * 2, "native", [0])
    ga, gb = su.normal_global(size, dtype, seed=1), su.normal_global(size, dtype, seed=2)
    su.scatter(dd, a, ga)
    su.scatter(dd, b, gb)
    vals = [dd.dot(a, b) for _ in range(3)]
    assert vals[0] == vals[1] == vals[2]
    wide = su._wide(np.float64)
    ref = float((ga.astype(wide) * gb.astype(wide)).sum())
    mag = float((np.abs(ga).astype(wide) * np.abs(gb).astype(wide)).sum())
    # one rounding per fp64 product (none for fp32 data) and n - 1 fp64 additions
    assert abs(vals[0] - ref) <= (ga.size + 1) * np.finfo(np.float64).eps * mag


# ----------------------------------------------------------------- validation
def test_validation_launches_nothing():
    size = (19, 10, 9)
    dd, (f, g, e, i32, d) = su.make_domain(
        size, _C.Radius.constant(1),
        [np.float32, np.float32, np.float32, np.int32, np.float64], "native", [0])
    flo, fhi = full_region_of(dd, 0)
    sent = np.full((fhi[2] - flo[2], fhi[1] - flo[1], fhi[0] - flo[0]), -99.0, dtype=np.float32)
    for h in (f, g, e):
        dd.write_global(0, flo, sent, h)
    outside = ((flo[0] - 1, 0, 0), (5, 5, 5))
    beyond = ((0, 0, 0), (fhi[0] + 1, 5, 5))
    with pytest.raises(ValueError):
        dd.dot(i32)
    with pytest.raises(ValueError):
        dd.dot(f, d)
    with pytest.raises(ValueError):
        dd.axpby(1.0, f, 1.0, d, out=g)
    with pytest.raises(ValueError):
        dd.axpby(1.0, f, 1.0, f, out=i32)
    with pytest.raises(ValueError):
        dd.cg_update(1.0, f, g, d)
    for where in (outside, beyond):
        with pytest.raises(ValueError):
            dd.dot(f, where=where)
        with pytest.raises(ValueError):
            dd.axpby(2.0, f, 2.0, f, out=g, where=where)
        with pytest.raises(ValueError):
            dd.backend.cg_update([where], 1.0, f.index, g.index, e.index)
    # below the dtype checks of DistributedDomain: element sizes and indices
    eng = dd.backend.engine
    rect = _C.Rect3(_C.Vec3(0, 0, 0), _C.Vec3(5, 5, 5))
    with pytest.raises(ValueError):
        _C.field_dot(eng, 0, f.index, False, d.index, False, rect)
    with pytest.raises(ValueError):
        _C.field_axpby(eng, 0, 1.0, f.index, False, 1.0, f.index, False, d.index, False, rect)
    with pytest.raises(ValueError):
        _C.field_axpby(eng, 0, 1.0, f.index, False, 1.0, f.index, False, 17, False, rect)
    with pytest.raises(ValueError):
        _C.field_dot(eng, 3, f.index, False, f.index, False, rect)
    with pytest.raises(ValueError):
        _C.cg_update(eng, 0, 1.0, f.index, f.index, g.index, rect)
    # an empty region is a no-op returning 0
    empty = ((2, 2, 2), (2, 5, 5))
    assert dd.dot(f, where=empty) == 0.0
    dd.axpby(2.0, f, 2.0, f, out=g, where=empty)
    assert dd.backend.cg_update([empty], 1.0, f.index, g.index, e.index) == [0.0]
    assert _C.field_dot(eng, 0, f.index, False, g.index, False,
                        _C.Rect3(_C.Vec3(2, 2, 2), _C.Vec3(2, 5, 5))) == 0.0
    dd.backend.sync_compute()
    for h in (f, g, e):
        got = dd.read_global(0, flo, fhi, h)
        np.testing.assert_array_equal(got.view(np.uint8), sent.view(np.uint8))


# ----------------------------------------------------- solver against the truth
_TORCH_RUNS = {}


def _torch_iterations(case, dtype):
    """the torch backend's iteration count of a case, computed once"""
    key = (cu.case_id(case), np.dtype(dtype).name)
    if key not in _TORCH_RUNS:
        _TORCH_RUNS[key] = cu.solve_case("torch", case, dtype)[0].iterations
    return _TORCH_RUNS[key]


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", cu.SOLVER_CASES, ids=cu.case_id)
def test_solver_native_against_the_truth(case, dtype):
    res, x, b, app = cu.solve_case("native", case, dtype)
    cu.check_solution(res, x, b, app, case, dtype, "native")
    want = _torch_iterations(case, dtype)
    print(f"torch backend: {want} iterations")
    assert abs(res.iterations - want) <= 2


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_solver_no_overlap_and_initial_guess(dtype):
    case = cu.SOLVER_CASES[4]
    size, order, sigma, bc, gpus = case
    app = Poisson3D(size, order=order, dtype=dtype, sigma=sigma, backend="native", gpus=gpus,
                    boundary=cu.kinds_of(bc))
    app.realize()
    b = su.normal_global(size, dtype)
    app.set_rhs(b)
    app.set_guess(su.normal_global(size, dtype, seed=7))
    tol = cu.TOL[dtype]
    res = app.solve(tol=tol, max_iter=cu.MAX_ITER, x0_zero=False, overlap=False)
    assert res.converged and res.residuals[-1] <= tol
    assert cu.true_rel_residual(app.solution(), b, app.stencil, cu.kinds_of(bc)) <= 2 * tol


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_poisson3d_round_trip(dtype):
    """b = A x* for a smooth x*, solved back: periodic sigma = 1 order 2
    has eigenvalues in [1, 13], so ||x - x*|| <= kappa * tol * ||x*||-type
    bounds hold with 10 as slack"""
    size = (19, 10, 9)
    tol = cu.TOL[dtype]
    app = Poisson3D(size, order=2, dtype=dtype, sigma=1.0, backend="native", gpus=[0])
    app.realize()
    z, y, x = np.meshgrid(*(np.arange(n) * (2 * np.pi / n) for n in size[::-1]), indexing="ij")
    wide = su._wide(dtype)
    xs = (np.sin(x) * np.cos(2 * y) + 0.5 * np.cos(z) + 0.25).astype(dtype)
    b = cu.apply_true(xs, app.stencil, None).astype(dtype)
    app.set_rhs(b)
    res = app.solve(tol=tol, max_iter=cu.MAX_ITER)
    assert res.converged
    err = float(np.abs(app.solution().astype(wide) - xs.astype(wide)).max() / np.abs(xs).max())
    print(f"round trip {np.dtype(dtype).name}: {res.iterations} iterations, "
          f"max error / max |x*| = {err:.3e} (bound {10 * tol:.0e})")
    assert err <= 10 * tol
