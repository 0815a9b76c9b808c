"""Variable-coefficient diffusion on the GPU: diffusion_apply and
diffusion_inv_diagonal (csrc/src/diffusion_op.hip) and scaled_update
(csrc/src/vector_ops.hip) bitwise against numpy on exact data, their
containment contract, determinism, symmetry and validation; the native
V-cycle against the numpy oracle of diffusion_util.py and the plain,
Jacobi- and multigrid-preconditioned solves.

Exact data: u integers in [0, 753), k integers in [1, 16], h_a and sigma
from {0.25, 0.5, 1, 2} (also sigma = 0 and 3). k + k' <= 32, 0.5 h (k + k')
is a multiple of 1/8 up to 32, |u - u'| < 753: every product is a multiple
of 1/8 below 2^15 and every partial sum of the seven terms, in flux form or
as diag * u - sum kf * u', a multiple of 1/16 below 2^19: exact in fp32 and
fp64 in any association, with or without FMA contraction. The diagonal is a
multiple of 1/8 below 2^8, so omega / diag is one correctly rounded
division of exact operands. For scaled_update: d from {0.25, 0.5, 1, 2},
integer operands below 753 and the COEFFS of test_gpu_mg.py."""
import numpy as np
import pytest

from stencil_amd import Boundary, DistributedDomain, Next, Stencil, _C
from stencil_amd.models.poisson3d import Poisson3D

import cg_util as cu
import diffusion_util as du
import mg_util as mu
import stencil_util as su
from util import full_region_of

pytestmark = pytest.mark.gpu

DTYPES, DT_IDS = cu.DTYPES, cu.DT_IDS

# head / tail lanes, a short last z chunk (a thread marches 4 planes; 33 and
# 65 leave a chunk of one), one / several / many z chunks, a row wider than a
# 64-lane block, and (narrower than 8 cells) the linearised path
SHAPES = [(8, 4, 3), (9, 5, 33), (19, 6, 65), (261, 5, 3), (5, 3, 2), (1, 1, 1)]
X0S = [0, 1, 2, 3]  # box start in x: every 16 B alignment of the rows
COEFFS = [(1.0, -1.0), (2.0, 0.5), (-1.0, 2.0), (0.5, 1.0)]
# per box start: (h_x, h_y, h_z), sigma
PARAMS = [((0.25, 0.5, 1.0), 0.0), ((2.0, 0.25, 0.5), 3.0), ((1.0, 2.0, 0.25), 0.5),
          ((0.5, 1.0, 2.0), 2.0)]
SENTINEL = -99.0


def _sid(s):
    return "x".join(map(str, s))


def _zyx(ext):
    return (ext[2], ext[1], ext[0])


def _box(lo, hi):
    return (slice(lo[2], hi[2]), slice(lo[1], hi[1]), slice(lo[0], hi[0]))


def _same_bits(got, want):
    np.testing.assert_array_equal(got.view(np.uint8), want.view(np.uint8))


class _Alloc:
    """one native domain, 3 cells longer in x than the shape so that the box
    can start at 0..3; whole-allocation reads and writes"""

    def __init__(self, shape, radius, dtype, n):
        self.shape, self.dtype = shape, dtype
        size = (shape[0] + 3, shape[1], shape[2])
        self.dd, self.h = su.make_domain(size, _C.Radius.constant(radius), [dtype] * n, "native",
                                         [0])
        self.flo, self.fhi = full_region_of(self.dd, 0)
        self.ext = _zyx(tuple(self.fhi[i] - self.flo[i] for i in range(3)))

    def whole(self, value):
        return np.full(self.ext, value, dtype=self.dtype)

    def rel(self, p):
        return tuple(p[i] - self.flo[i] for i in range(3))

    def put(self, h, whole, nxt=False):
        self.dd.write_global(0, self.flo, whole, h, to_next=nxt)

    def get(self, h, nxt=False):
        return self.dd.read_global(0, self.flo, self.fhi, h, from_next=nxt)

    def inset(self, whole, lo, hi, block):
        out = whole.copy()
        out[_box(self.rel(lo), self.rel(hi))] = block
        return out

    def cross(self, data, lo, hi):
        """`data` (a whole allocation) on the box and its six face
        neighbours, NaN everywhere else: edge and corner halos included"""
        return np.where(du.cross_mask(self.ext, self.rel(lo), self.rel(hi)), data,
                        self.dtype(np.nan))


# ------------------------------------------------- the kernels, bit for bit
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("radius", [1, 2], ids=["r1", "r2"])
@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_apply_and_diagonal_exact_and_contained(shape, radius, dtype):
    """per box start: u and k hold NaN everywhere outside the region and
    its face neighbours (read containment: no NaN may come out), the
    destination allocation is compared whole against sentinel + numpy
    (write containment) and the sources whole against what was written"""
    al = _Alloc(shape, radius, dtype, 4)
    u, k, o, d = al.h
    sent = al.whole(SENTINEL)
    work = np.dtype(dtype).type
    for x0, (h, sigma) in zip(X0S, PARAMS):
        lo, hi = (x0, 0, 0), (x0 + shape[0], shape[1], shape[2])
        rlo, rhi = al.rel(lo), al.rel(hi)
        wu = al.cross(mu.int_field(al.ext, dtype, 50 + x0), lo, hi)
        wk = al.cross(du.int_k(al.ext, dtype, 60 + x0), lo, hi)
        want, _ = du.apply_block(wu, wk, rlo, rhi, h, sigma, work)
        exact, _ = du.apply_block(wu, wk, rlo, rhi, h, sigma, su._wide(dtype))
        assert np.array_equal(want.astype(exact.dtype), exact)  # the data really is exact
        al.put(u, wu)
        al.put(k, wk)
        al.put(o, sent, nxt=True)
        al.put(d, sent)
        al.dd.backend.diffusion_apply(0, u.index, k.index, o.index, lo, hi, h, sigma, dtype)
        al.dd.backend.diffusion_inv_diagonal(0, k.index, d.index, False, lo, hi, h, sigma,
                                             mu.OMEGA)
        al.dd.backend.sync_compute()
        _same_bits(al.get(o, nxt=True), al.inset(sent, lo, hi, want))
        diag = du.diagonal_block(wk, rlo, rhi, h, sigma, work)
        assert np.array_equal(diag.astype(np.float64),
                              du.diagonal_block(wk, rlo, rhi, h, sigma, np.float64))
        _same_bits(al.get(d), al.inset(sent, lo, hi, work(mu.OMEGA) / diag))
        _same_bits(al.get(u), wu)  # the sources are read only
        _same_bits(al.get(k), wk)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_scaled_update_exact_and_contained(shape, dtype):
    al = _Alloc(shape, 2, dtype, 5)
    x, d, y, z, o = al.h
    nan, sent = al.whole(np.nan), al.whole(SENTINEL)
    dd = al.dd
    for x0, (alpha, beta) in zip(X0S, COEFFS):
        lo, hi = (x0, 0, 0), (x0 + shape[0], shape[1], shape[2])
        gx, gy, gz = (mu.int_field(_zyx(shape), dtype, 70 + 3 * x0 + i) for i in range(3))
        gd = np.random.default_rng(80 + x0).choice([0.25, 0.5, 1.0, 2.0],
                                                   size=_zyx(shape)).astype(dtype)
        gamma = -beta
        want = (alpha * gx + gd * (beta * gy + gamma * gz)).astype(dtype)
        al.put(x, al.inset(nan, lo, hi, gx))
        al.put(d, al.inset(nan, lo, hi, gd))
        al.put(y, al.inset(nan, lo, hi, gy), nxt=True)
        al.put(z, al.inset(nan, lo, hi, gz))
        al.put(o, sent)
        dd.scaled_update(alpha, x, d, beta, Next(y), gamma, z, out=o, where=(lo, hi))
        dd.scaled_update(alpha, x, d, beta, Next(y), gamma, z, out=z, where=(lo, hi))  # in place
        dd.backend.sync_compute()
        _same_bits(al.get(o), al.inset(sent, lo, hi, want))
        _same_bits(al.get(z), al.inset(nan, lo, hi, want))
        _same_bits(al.get(x), al.inset(nan, lo, hi, gx))
        _same_bits(al.get(d), al.inset(nan, lo, hi, gd))
        _same_bits(al.get(y, nxt=True), al.inset(nan, lo, hi, gy))
        # the first sweep e = d f and the Jacobi preconditioner z = d r
        al.put(o, sent, nxt=True)
        dd.scaled_update(0.0, x, d, 1.0, x, 0.0, x, out=Next(o), where=(lo, hi))
        dd.backend.sync_compute()
        _same_bits(al.get(o, nxt=True), al.inset(sent, lo, hi, gd * gx))


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_unit_coefficient_is_the_laplacian(dtype):
    """k = 1: bit for bit apply_stencil(sigma I - laplacian(2, spacing)) on
    the exact data, for every `where`, on two domains of one GPU"""
    size = (38, 7, 6)
    dd, (u, k, a, b) = su.make_domain(size, _C.Radius.constant(1), [dtype] * 4, "native", [0, 0])
    assert dd.num_local() == 2
    spacing, sigma = (2.0, 1.0, 0.5), 0.5  # h = 0.25, 1, 4
    st = -Stencil.laplacian(2, spacing) + sigma * Stencil.identity()
    su.scatter(dd, u, mu.int_field(_zyx(size), dtype, 4))
    su.scatter(dd, k, np.ones(_zyx(size), dtype=dtype))
    dd.exchange()
    sent = np.full(_zyx(size), SENTINEL, dtype=dtype)
    for where in ("all", "interior", "exterior"):
        su.scatter(dd, a, sent, to_next=True)
        su.scatter(dd, b, sent, to_next=True)
        dd.apply_diffusion(k, u, a, spacing=spacing, sigma=sigma, where=where)
        dd.apply_stencil(st, u, b, where=where)
        dd.backend.sync_compute()
        got, want = su.gather(dd, a, from_next=True), su.gather(dd, b, from_next=True)
        assert (want != SENTINEL).any()
        _same_bits(got, want)
    full = su.exact_oracle(su.gather(dd, u), st)
    su.scatter(dd, a, sent, to_next=True)
    dd.apply_diffusion(k, u, a, spacing=spacing, sigma=sigma)
    dd.backend.sync_compute()
    _same_bits(su.gather(dd, a, from_next=True), full)


# A cell's value is the sum of seven terms. The sigma term takes two
# roundings (sigma, the product), a face term five (0.5 h_a, k + k', their
# product, u - u', the product with it), and the terms are joined by six
# additions, each rounding at most half an eps of a partial sum that the sum
# S of the seven magnitudes bounds: |err| <= (5 + 6) (eps / 2) S to first
# order, FMA contraction only removing roundings. 6 eps S holds with the
# second-order terms.
ROUNDINGS = 6


def _normal_case(dtype, kinds, gpus, size=(37, 10, 9)):
    """(dd, handles u v k au av, global u v k) with exchanged halos"""
    dd = DistributedDomain(*size, backend="native")
    dd.set_radius(1)
    dd.set_gpus(gpus)
    hs = [dd.add_data(dtype, n) for n in ("u", "v", "k", "au", "av")]
    for face, (kind, value) in (kinds or {}).items():
        dd.set_boundary(face, kind, value)
        dd.set_boundary(face, Boundary.CLAMP, quantities=[hs[2]])
    dd.realize()
    gu, gv = su.normal_global(size, dtype, seed=1), su.normal_global(size, dtype, seed=2)
    gk = np.exp(su.normal_global(size, np.float64, seed=3)).astype(dtype)
    for h, g in zip(hs, (gu, gv, gk)):
        su.scatter(dd, h, g)
    dd.exchange()
    return dd, hs, (gu, gv, gk)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_normal_data_bounded_and_deterministic(dtype):
    """seeded normal u and k = exp(normal), periodic, two domains: within
    ROUNDINGS eps S of the wide oracle (derivation above), and the same
    bits twice"""
    dd, (u, v, k, au, av), (gu, gv, gk) = _normal_case(dtype, None, [0, 0])
    spacing, sigma = (1.0, 0.7, 1.3), 0.37
    outs = []
    for _ in range(2):
        su.scatter(dd, au, np.full(gu.shape, SENTINEL, dtype=dtype), to_next=True)
        dd.apply_diffusion(k, u, au, spacing=spacing, sigma=sigma)
        dd.backend.sync_compute()
        outs.append(su.gather(dd, au, from_next=True))
    _same_bits(outs[0], outs[1])
    wide = su._wide(dtype)
    h = [1.0 / (s * s) for s in spacing]
    pu, pk = np.pad(gu, 1, mode="wrap"), np.pad(gk, 1, mode="wrap")
    lo, hi = (1, 1, 1), tuple(n + 1 for n in (gu.shape[2], gu.shape[1], gu.shape[0]))
    ref, mag = du.apply_block(pu, pk, lo, hi, h, sigma, wide)
    su.assert_within_bound(outs[0], ref, ROUNDINGS * np.finfo(dtype).eps * mag, "diffusion_apply")


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("bc", ["fixed0", "mirror", "antimirror", "periodic"])
def test_operator_is_symmetric(bc, dtype):
    """|u . A v - v . A u| within the rounding bound, two domains. A is
    exactly symmetric, so the difference is rounding alone: A v is off by at
    most ROUNDINGS eps S_v per cell, and each fp64 inner product of N cells
    by at most (N + 2) eps64 sum |u| |A v| <= (N + 2) eps64 sum |u| S_v."""
    kinds = cu.kinds_of(bc)
    dd, (u, v, k, au, av), (gu, gv, gk) = _normal_case(dtype, kinds, [0, 0])
    spacing, sigma = (1.0, 0.7, 1.3), 0.37
    dd.apply_diffusion(k, u, au, spacing=spacing, sigma=sigma)
    dd.apply_diffusion(k, v, av, spacing=spacing, sigma=sigma)
    dd.backend.sync_compute()
    diff = abs(dd.dot(u, Next(av)) - dd.dot(v, Next(au)))
    wide = su._wide(dtype)
    h = [1.0 / (s * s) for s in spacing]
    pk = du.pad_k(gk, kinds)
    n = gu.shape
    lo, hi = (1, 1, 1), (n[2] + 1, n[1] + 1, n[0] + 1)
    _, su_mag = du.apply_block(cu.pad_array(gu, du.RADIUS1, kinds), pk, lo, hi, h, sigma, wide)
    _, sv_mag = du.apply_block(cu.pad_array(gv, du.RADIUS1, kinds), pk, lo, hi, h, sigma, wide)
    cross = float((np.abs(gu) * sv_mag).sum() + (np.abs(gv) * su_mag).sum())
    bound = (ROUNDINGS * np.finfo(dtype).eps + (gu.size + 2) * np.finfo(np.float64).eps) * cross
    print(f"{bc} {np.dtype(dtype).name}: |u.Av - v.Au| = {diff:.3e}, bound {bound:.3e}")
    assert np.isfinite(diff) and diff <= bound


# ----------------------------------------------------------------- validation
def test_validation_launches_nothing():
    """every ValueError of the three ops, and an empty region, leave every
    allocation as it was. Not covered: layouts that differ (the quantities
    of one domain share one layout, so the check cannot be reached from
    Python)."""
    f32, f64, i16 = np.float32, np.float64, np.int16
    dd, (a, b, c, fd, i1, i2, i3) = su.make_domain(
        (16, 8, 8), _C.Radius.constant(1), [f32, f32, f32, f64, i16, i16, i16], "native", [0])
    fl, fu = full_region_of(dd, 0)
    sent = np.full(_zyx(tuple(fu[i] - fl[i] for i in range(3))), SENTINEL, dtype=f32)
    for h in (a, b, c):
        dd.write_global(0, fl, sent, h)
        dd.write_global(0, fl, sent, h, to_next=True)
    eng = dd.backend.engine

    def rect(lo, hi):
        return _C.Rect3(_C.Vec3(*lo), _C.Vec3(*hi))

    ok = rect((0, 0, 0), (16, 8, 8))
    bad_regions = [
        rect((0, 0, 0), (16, 8, 10)),  # outside the allocation
        rect((-2, 0, 0), (16, 8, 8)),
        rect((-1, 0, 0), (16, 8, 8)),  # allocated, but its face apron is not
        rect((0, 0, 0), (16, 9, 8)),
        rect(fl, fu),
    ]
    h = [1.0, 1.0, 1.0]

    def apply(dom=0, src=a.index, k=b.index, dst=c.index, region=ok, ty=_C.StencilType.F32,
              sid=0):
        _C.diffusion_apply(eng, dom, src, k, dst, region, h, 0.5, ty, sid)

    def inv_diag(dom=0, k=b.index, out=c.index, region=ok, sid=0):
        _C.diffusion_inv_diagonal(eng, dom, k, out, False, region, h, 0.5, 1.0, sid)

    def scaled(dom=0, x=a.index, d=b.index, y=a.index, z=c.index, out=c.index, region=ok, sid=0):
        _C.field_scaled_update(eng, dom, 1.0, x, False, d, False, 1.0, y, False, 1.0, z, True,
                               out, False, region, sid)

    for kw in ({"dom": 1}, {"dom": -1}, {"src": 9}, {"src": -1}, {"k": 7}, {"k": -1}, {"dst": 11},
               {"dst": -2}, {"dst": fd.index}, {"k": fd.index}, {"src": fd.index},
               {"src": i1.index, "k": i2.index, "dst": i3.index}, {"ty": _C.StencilType.F64},
               {"sid": 2}, {"sid": -1}):
        with pytest.raises(ValueError):
            apply(**kw)
    for kw in ({"dom": 1}, {"dom": -1}, {"k": 7}, {"k": -1}, {"out": 9}, {"out": fd.index},
               {"k": fd.index}, {"k": i1.index, "out": i2.index}, {"sid": 2}):
        with pytest.raises(ValueError):
            inv_diag(**kw)
    for kw in ({"dom": 1}, {"x": 9}, {"d": -1}, {"d": fd.index}, {"out": fd.index},
               {"x": i1.index, "d": i1.index, "y": i1.index, "z": i2.index, "out": i2.index},
               {"sid": 2}):
        with pytest.raises(ValueError):
            scaled(**kw)
    for region in bad_regions:
        with pytest.raises(ValueError):
            apply(region=region)
        with pytest.raises(ValueError):
            inv_diag(region=region)
    for region in bad_regions[:2]:
        with pytest.raises(ValueError):
            scaled(region=region)
    with pytest.raises(ValueError):
        dd.scaled_update(1.0, a, b, 1.0, a, 1.0, fd, out=a)
    with pytest.raises(ValueError):
        dd.apply_diffusion(fd, a, c)
    with pytest.raises(ValueError):
        dd.apply_diffusion(b, a, c, where="some")
    # an empty region is a no-op
    empty = rect((2, 2, 2), (2, 4, 4))
    apply(region=empty)
    inv_diag(region=empty)
    scaled(region=empty)
    dd.backend.sync_compute()
    for hd in (a, b, c):
        _same_bits(dd.read_global(0, fl, fu, hd), sent)
        _same_bits(dd.read_global(0, fl, fu, hd, from_next=True), sent)


# ------------------------------------------------------ the cycle and the solves
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", du.DIFF_CASES, ids=du.case_id)
def test_cycle_native_against_the_oracle(case, dtype):
    du.check_cycle("native", case, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", du.DIFF_CASES, ids=du.case_id)
def test_iteration_conditions_native(case, dtype):
    du.check_iterations("native", case, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("solver", list(du.SOLVERS))
@pytest.mark.parametrize("case", du.DIFF_CASES, ids=du.case_id)
def test_solve_true_residual_native(case, solver, dtype):
    """Converged, and the true residual in the wide type within 2 tol (see
    test_diffusion_cpu.py::test_solve_true_residual_torch: float32 meets it
    on the periodic sigma = 1e-3 rows through the solver's true-residual
    check only)."""
    du.check_solve("native", case, dtype, solver)


@pytest.mark.parametrize("pre", ["jacobi", "multigrid"])
def test_refresh_coefficients_native(pre):
    """solve, set_coefficient(new k), solve: as many iterations as an app
    built with the new k from the start, and the same bits"""
    case, dtype = du.DIFF_CASES[1], np.float64
    new_k = du.k_smooth(case[0])
    b = su.normal_global(case[0], dtype)
    app = du.make_app("native", case, dtype, pre)
    app.set_rhs(b)
    first = app.solve(tol=cu.TOL[dtype], max_iter=du.MAX_ITER)
    app.set_coefficient(new_k)
    again = app.solve(tol=cu.TOL[dtype], max_iter=du.MAX_ITER)
    fresh = du.make_app("native", case, dtype, pre, k=new_k)
    fresh.set_rhs(b)
    want = fresh.solve(tol=cu.TOL[dtype], max_iter=du.MAX_ITER)
    assert first.converged and again.converged and want.converged
    assert again.iterations == want.iterations
    _same_bits(app.solution(), fresh.solution())


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_constant_coefficient_path_is_unchanged(dtype):
    """regression guard (passes before this feature too): Poisson3D without
    a coefficient solves MG_CASES[0] in the iteration counts of mg_util's
    own solves, and within the numpy oracle's count + 2"""
    case = mu.MG_CASES[0]
    size, order, sigma, bc, gpus = case
    for pre in (None, "multigrid"):
        app = Poisson3D(size, order=order, dtype=dtype, sigma=sigma, backend="native", gpus=gpus,
                        boundary=cu.kinds_of(bc), preconditioner=pre)
        app.realize()
        app.set_rhs(su.normal_global(size, dtype))
        res = app.solve(tol=cu.TOL[dtype], max_iter=cu.MAX_ITER)
        assert res.converged
        if pre is None:
            assert res.iterations == mu.plain_iterations("native", case, dtype)
        else:
            assert res.iterations == mu.solve_case("native", case, dtype, pre)[0].iterations
            assert res.iterations <= mu.oracle_iterations(case, dtype) + 2
