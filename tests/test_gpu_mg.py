"""Geometric multigrid on the GPU: the axpbypcz kernel (csrc/src/
vector_ops.hip) and the grid-transfer kernels (csrc/src/grid_transfer.hip)
bitwise against numpy on exact data, their containment contract,
determinism and validation; the native V-cycle against the numpy oracle of
mg_util.py and the preconditioned solves.

Exact data: integer fields below 753 and coefficients in {1, -1, 2, 0.5}.
alpha a + beta b is then a multiple of 1/2 below 2^11, the sum over 8
children a multiple of 1/2 below 2^14 and its eighth a multiple of 1/16
below 2^11: exact in fp32 and fp64 in any summation order, with or without
FMA contraction."""
import numpy as np
import pytest

from stencil_amd import Next, _C
from stencil_amd.models.poisson3d import Poisson3D
from stencil_amd.solvers import GridTransfer

import cg_util as cu
import mg_util as mu
import stencil_util as su
from util import full_region_of

pytestmark = pytest.mark.gpu

DTYPES, DT_IDS = cu.DTYPES, cu.DT_IDS

# COARSE regions; the fine region is twice each. A strip is 8 B of the
# coarse row (fp32: 2 cells, one tail lane when x is odd; fp64: 1 cell), a
# block 64 strips x 4 rows, a thread marches 4 coarse planes: y 2..5 cuts
# rows at the block edge, z 17 / 33 gives several z chunks with a short last
# one, 131 a row wider than one 64-lane block in either type. Narrower than
# 4 cells: the linearised cell path.
STRIP_SHAPES = [(4, 2, 1), (5, 3, 2), (6, 4, 17), (7, 5, 33), (9, 2, 17), (10, 3, 1),
                (131, 3, 2)]
CELL_SHAPES = [(1, 1, 1), (2, 3, 2), (3, 2, 5)]
X0S = [0, 1, 2, 3]  # box start in x: every 16 B alignment of both rows
# (fine radius, coarse radius): the first child sits at an odd / even index
RADII = [(1, 1), (2, 1), (1, 2), (2, 2)]
COEFFS = [(1.0, -1.0), (2.0, 0.5), (-1.0, 2.0), (0.5, 1.0)]
SENTINEL = -99.0


def _sid(s):
    return "x".join(map(str, s))


def _rid(r):
    return f"rf{r[0]}rc{r[1]}"


def _zyx(ext):
    return (ext[2], ext[1], ext[0])


def _box(lo, hi):
    return (slice(lo[2], hi[2]), slice(lo[1], hi[1]), slice(lo[0], hi[0]))


class _Pair:
    """a fine and a coarse single-domain DistributedDomain, the coarse one
    3 cells longer in x than the shape so that the box can start at 0..3"""

    def __init__(self, shape, radii, dtype, nf=3, nc=2):
        self.csize = (shape[0] + 3, shape[1], shape[2])
        self.fsize = tuple(2 * n for n in self.csize)
        self.dtype = dtype
        self.fine, self.fh = cu.vector_domain(self.fsize, [dtype] * nf, "native", [0], radii[0])
        self.coarse, self.ch = cu.vector_domain(self.csize, [dtype] * nc, "native", [0], radii[1])
        self.fl, self.fu = full_region_of(self.fine, 0)
        self.cl, self.cu_ = full_region_of(self.coarse, 0)

    def whole(self, fine, value):
        lo, hi = (self.fl, self.fu) if fine else (self.cl, self.cu_)
        return np.full(_zyx(tuple(hi[i] - lo[i] for i in range(3))), value, dtype=self.dtype)

    def put(self, fine, h, whole, nxt=False):
        dd, lo = (self.fine, self.fl) if fine else (self.coarse, self.cl)
        dd.write_global(0, lo, whole, h, to_next=nxt)

    def get(self, fine, h, nxt=False):
        dd, lo, hi = (self.fine, self.fl, self.fu) if fine else (self.coarse, self.cl, self.cu_)
        return dd.read_global(0, lo, hi, h, from_next=nxt)

    def inset(self, fine, whole, lo, hi, block):
        """`whole` (a full allocation) with the global box [lo, hi) replaced"""
        flo = self.fl if fine else self.cl
        out = whole.copy()
        out[_box(tuple(lo[i] - flo[i] for i in range(3)),
                 tuple(hi[i] - flo[i] for i in range(3)))] = block
        return out

    def restrict(self, alpha, a, a_next, beta, b, b_next, out, out_next, lo, hi):
        self.fine.backend.sync_compute()
        self.coarse.backend.grid_restrict(self.fine.backend, 0, alpha, a.index, a_next, beta,
                                          b.index, b_next, 0, out.index, out_next, lo, hi)
        self.coarse.backend.sync_compute()

    def prolong_add(self, src, src_next, dst, dst_next, lo, hi):
        self.coarse.backend.sync_compute()
        self.fine.backend.grid_prolong_add(self.coarse.backend, 0, src.index, src_next, 0,
                                           dst.index, dst_next, lo, hi)
        self.fine.backend.sync_compute()


def _same_bits(got, want):
    np.testing.assert_array_equal(got.view(np.uint8), want.view(np.uint8))


# -------------------------------------------- the transfer kernels, bit for bit
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("radii", RADII, ids=_rid)
@pytest.mark.parametrize("shape", STRIP_SHAPES + CELL_SHAPES, ids=_sid)
def test_transfer_exact_and_contained(shape, radii, dtype):
    """per box start: the sources hold NaN everywhere outside the region
    (read containment: no NaN may come out), every destination allocation
    is compared whole against sentinel + numpy (write containment)"""
    pr = _Pair(shape, radii, dtype)
    a, b, d = pr.fh
    c, s = pr.ch
    nan_f, nan_c = pr.whole(True, np.nan), pr.whole(False, np.nan)
    sent_f, sent_c = pr.whole(True, SENTINEL), pr.whole(False, SENTINEL)
    for x0, (alpha, beta) in zip(X0S, COEFFS):
        lo, hi = (x0, 0, 0), (x0 + shape[0], shape[1], shape[2])
        flo, fhi = tuple(2 * v for v in lo), tuple(2 * v for v in hi)
        ga = mu.int_field(_zyx(tuple(2 * n for n in shape)), dtype, 10 + x0)
        gb = mu.int_field(ga.shape, dtype, 20 + x0)
        gs = mu.int_field(_zyx(shape), dtype, 30 + x0)
        # restriction: a in curr, b in next, out in next
        src_a, src_b = pr.inset(True, nan_f, flo, fhi, ga), pr.inset(True, nan_f, flo, fhi, gb)
        pr.put(True, a, src_a)
        pr.put(True, b, src_b, nxt=True)
        pr.put(False, c, sent_c, nxt=True)
        pr.restrict(alpha, a, False, beta, b, True, c, True, lo, hi)
        want = mu.restrict_mean((alpha * ga + beta * gb).astype(dtype))
        _same_bits(pr.get(False, c, nxt=True), pr.inset(False, sent_c, lo, hi, want))
        _same_bits(pr.get(True, a), src_a)  # the sources are read only
        _same_bits(pr.get(True, b, nxt=True), src_b)
        # prolongation: src in curr, dst in curr
        pr.put(False, s, pr.inset(False, nan_c, lo, hi, gs))
        pr.put(True, d, pr.inset(True, sent_f, flo, fhi, ga))
        pr.prolong_add(s, False, d, False, lo, hi)
        _same_bits(pr.get(True, d), pr.inset(True, sent_f, flo, fhi, ga + mu.prolong(gs)))
        _same_bits(pr.get(False, s), pr.inset(False, nan_c, lo, hi, gs))


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_transfer_two_domains_on_one_gpu(dtype):
    fsize, csize = (32, 16, 16), (16, 8, 8)
    fine, (a, b) = cu.vector_domain(fsize, [dtype] * 2, "native", [0, 0])
    coarse, (c, s) = cu.vector_domain(csize, [dtype] * 2, "native", [0, 0])
    assert fine.num_local() == 2
    tr = GridTransfer(fine, coarse)
    ga, gb = mu.int_field(_zyx(fsize), dtype, 1), mu.int_field(_zyx(fsize), dtype, 2)
    gs = mu.int_field(_zyx(csize), dtype, 3)
    su.scatter(fine, a, ga)
    su.scatter(fine, b, gb, to_next=True)
    su.scatter(coarse, s, gs)
    tr.restrict(1.0, a, -1.0, Next(b), c)
    tr.prolong_add(s, a)
    fine.backend.sync_compute()
    coarse.backend.sync_compute()
    _same_bits(su.gather(coarse, c), mu.restrict_mean(ga - gb))
    _same_bits(su.gather(fine, a), ga + mu.prolong(gs))
    other, _ = cu.vector_domain((16, 8, 6), [dtype], "native", [0, 0])
    with pytest.raises(ValueError):
        GridTransfer(fine, other)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_transfer_is_deterministic(dtype):
    """normal data, non-dyadic coefficients: the same bits twice. The value
    is within a rounding bound: a cell's path through the arithmetic has a
    coefficient, a product and at most 15 additions, each rounding at most
    half an eps of the running sum of magnitudes, and an exact scaling:
    17 eps * mean(|alpha a| + |beta b|) holds with room to spare"""
    shape = (37, 6, 9)
    pr = _Pair(shape, (1, 1), dtype)
    a, b, d = pr.fh
    c, s = pr.ch
    lo, hi = (1, 0, 0), (1 + shape[0], shape[1], shape[2])
    flo, fhi = tuple(2 * v for v in lo), tuple(2 * v for v in hi)
    fshape = _zyx(tuple(2 * n for n in shape))
    rng = np.random.default_rng(5)
    ga, gb = (rng.standard_normal(fshape).astype(dtype) for _ in range(2))
    alpha, beta = 1.0 / 3.0, -0.7
    pr.put(True, a, pr.inset(True, pr.whole(True, 0.0), flo, fhi, ga))
    pr.put(True, b, pr.inset(True, pr.whole(True, 0.0), flo, fhi, gb))
    outs = []
    for _ in range(2):
        pr.put(False, c, pr.whole(False, SENTINEL))
        pr.restrict(alpha, a, False, beta, b, False, c, False, lo, hi)
        outs.append(pr.get(False, c).copy())
    _same_bits(outs[0], outs[1])
    wide = su._wide(dtype)
    ta, tb = wide(alpha) * ga.astype(wide), wide(beta) * gb.astype(wide)
    ref = mu.restrict_mean(ta + tb)
    bound = 17 * np.finfo(dtype).eps * mu.restrict_mean(np.abs(ta) + np.abs(tb))
    got = outs[0][_box(tuple(lo[i] - pr.cl[i] for i in range(3)),
                       tuple(hi[i] - pr.cl[i] for i in range(3)))]
    su.assert_within_bound(got, ref, bound, "restrict")


# ------------------------------------------------------------------- axpbypcz
# the shapes of test_gpu_cg.py that take another path each: head/tail lanes,
# several z chunks, a row wider than a block, and the linearised thin box
AXPBYPCZ_SHAPES = [(8, 4, 3), (9, 5, 33), (19, 6, 65), (261, 5, 3), (5, 3, 2)]


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape", AXPBYPCZ_SHAPES, ids=_sid)
def test_axpbypcz_exact_and_contained(shape, dtype):
    size = (shape[0] + 3, shape[1], shape[2])
    dd, (x, y, z, o) = su.make_domain(size, _C.Radius.constant(2), [dtype] * 4, "native", [0])
    flo, fhi = full_region_of(dd, 0)
    ext = _zyx(tuple(fhi[i] - flo[i] for i in range(3)))
    nan, sent = np.full(ext, np.nan, dtype=dtype), np.full(ext, SENTINEL, dtype=dtype)

    def inset(whole, lo, hi, block):
        out = whole.copy()
        out[_box(tuple(lo[i] - flo[i] for i in range(3)),
                 tuple(hi[i] - flo[i] for i in range(3)))] = block
        return out

    for x0, (alpha, beta) in zip(X0S, COEFFS):
        lo, hi = (x0, 0, 0), (x0 + shape[0], shape[1], shape[2])
        gx, gy, gz = (mu.int_field(_zyx(shape), dtype, 40 + 3 * x0 + k) for k in range(3))
        gamma = -beta
        want = (alpha * gx + beta * gy + gamma * gz).astype(dtype)
        dd.write_global(0, flo, inset(nan, lo, hi, gx), x)
        dd.write_global(0, flo, inset(nan, lo, hi, gy), y, to_next=True)
        dd.write_global(0, flo, inset(nan, lo, hi, gz), z)
        dd.write_global(0, flo, sent, o)
        dd.axpbypcz(alpha, x, beta, Next(y), gamma, z, out=o, where=(lo, hi))
        dd.axpbypcz(alpha, x, beta, Next(y), gamma, z, out=z, where=(lo, hi))  # in place
        dd.backend.sync_compute()
        _same_bits(dd.read_global(0, flo, fhi, o), inset(sent, lo, hi, want))
        _same_bits(dd.read_global(0, flo, fhi, z), inset(nan, lo, hi, want))
        _same_bits(dd.read_global(0, flo, fhi, x), inset(nan, lo, hi, gx))
        _same_bits(dd.read_global(0, flo, fhi, y, from_next=True), inset(nan, lo, hi, gy))


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_axpbypcz_two_domains_bounded(dtype):
    """the relaxation update e + w f - w A e on normal data: three products
    and two additions, |err| <= 3 eps sum of the |terms|"""
    size = (37, 10, 9)
    dd, (e, f) = cu.vector_domain(size, [dtype] * 2, "native", [0, 0])
    ge, gf, gae = (su.normal_global(size, dtype, seed=s) for s in (1, 2, 3))
    su.scatter(dd, e, ge)
    su.scatter(dd, f, gf)
    su.scatter(dd, e, gae, to_next=True)
    w = 1.0 / 9.0
    dd.axpbypcz(1.0, e, w, f, -w, Next(e), out=e)
    dd.backend.sync_compute()
    wide = su._wide(dtype)
    wt = wide(dtype(w))
    terms = [ge.astype(wide), wt * gf.astype(wide), -wt * gae.astype(wide)]
    bound = 3 * np.finfo(dtype).eps * sum(np.abs(t) for t in terms)
    su.assert_within_bound(su.gather(dd, e), sum(terms), bound, "axpbypcz")


# ----------------------------------------------------------------- validation
def test_validation_launches_nothing():
    f32, f64 = np.float32, np.float64
    fine, (a, b, fd, fi) = su.make_domain((16, 8, 8), _C.Radius.constant(1),
                                          [f32, f32, f64, np.int16], "native", [0])
    coarse, (c, cd) = su.make_domain((8, 4, 4), _C.Radius.constant(1), [f32, f64], "native", [0])
    fl, fu = full_region_of(fine, 0)
    cl, cu_ = full_region_of(coarse, 0)
    sent_f = np.full(_zyx(tuple(fu[i] - fl[i] for i in range(3))), SENTINEL, dtype=f32)
    sent_c = np.full(_zyx(tuple(cu_[i] - cl[i] for i in range(3))), SENTINEL, dtype=f32)
    for h in (a, b):
        fine.write_global(0, fl, sent_f, h)
    coarse.write_global(0, cl, sent_c, c)
    fe, ce = fine.backend.engine, coarse.backend.engine

    def rect(lo, hi):
        return _C.Rect3(_C.Vec3(*lo), _C.Vec3(*hi))

    ok = rect((0, 0, 0), (8, 4, 4))
    bad_regions = [
        rect((0, 0, 0), (9, 4, 4)),  # the coarse halo is allocated, its children are not
        rect((-1, 0, 0), (8, 4, 4)),
        rect((0, 0, 0), (8, 4, 6)),  # outside the coarse allocation
    ]

    def restrict(fdom=0, qa=a.index, qb=b.index, cdom=0, out=c.index, region=ok, sid=0):
        _C.grid_restrict(fe, fdom, 2.0, qa, False, 2.0, qb, False, ce, cdom, out, False, region,
                         sid)

    def prolong(cdom=0, src=c.index, fdom=0, dst=a.index, region=ok, sid=0):
        _C.grid_prolong_add(ce, cdom, src, False, fe, fdom, dst, False, region, sid)

    for kw in ({"fdom": 1}, {"cdom": -1}, {"qa": 9}, {"out": 2}, {"qb": fd.index},
               {"qa": fi.index},
               {"out": cd.index}, {"sid": 5}):
        with pytest.raises(ValueError):
            restrict(**kw)
    for kw in ({"fdom": 3}, {"cdom": 1}, {"src": -1}, {"dst": 4}, {"dst": fd.index},
               {"dst": fi.index},
               {"src": cd.index}, {"sid": 2}):
        with pytest.raises(ValueError):
            prolong(**kw)
    for region in bad_regions:
        with pytest.raises(ValueError):
            restrict(region=region)
        with pytest.raises(ValueError):
            prolong(region=region)
    with pytest.raises(ValueError):
        fine.axpbypcz(1.0, a, 1.0, b, 1.0, fd, out=a)
    with pytest.raises(ValueError):
        fine.axpbypcz(2.0, a, 2.0, b, 2.0, a, out=b, where=((0, 0, 0), (fu[0] + 1, 4, 4)))
    rect5 = rect((0, 0, 0), (5, 5, 5))
    with pytest.raises(ValueError):
        _C.field_axpbypcz(fe, 0, 1.0, a.index, False, 1.0, b.index, False, 1.0, fd.index, False,
                          a.index, False, rect5)
    with pytest.raises(ValueError):
        _C.field_axpbypcz(fe, 0, 1.0, a.index, False, 1.0, b.index, False, 1.0, 17, False,
                          a.index, False, rect5)
    with pytest.raises(ValueError):
        _C.field_axpbypcz(fe, 2, 1.0, a.index, False, 1.0, b.index, False, 1.0, a.index, False,
                          a.index, False, rect5)
    # an empty region is a no-op
    empty = rect((2, 2, 2), (2, 4, 4))
    restrict(region=empty)
    prolong(region=empty)
    fine.axpbypcz(2.0, a, 2.0, b, 2.0, a, out=b, where=((2, 2, 2), (2, 5, 5)))
    fine.backend.sync_compute()
    coarse.backend.sync_compute()
    for h in (a, b):
        _same_bits(fine.read_global(0, fl, fu, h), sent_f)
    _same_bits(coarse.read_global(0, cl, cu_, c), sent_c)


# ------------------------------------------------------ the cycle and the solves
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", mu.MG_CASES, ids=cu.case_id)
def test_cycle_native_against_the_oracle(case, dtype):
    mu.check_cycle("native", case, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", mu.MG_CASES, ids=cu.case_id)
def test_preconditioned_solves_native(case, dtype):
    mu.check_mg_solve("native", case, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_native_no_overlap_matches_overlap(dtype):
    """level 0 with and without the interior/exterior split: both converge,
    in the same number of iterations up to the threshold crossing"""
    case = mu.MG_CASES[2]
    runs = []
    for overlap in (True, False):
        size, order, sigma, bc, gpus = case
        app = Poisson3D(size, order=order, dtype=dtype, sigma=sigma, backend="native", gpus=gpus,
                        boundary=cu.kinds_of(bc), preconditioner="multigrid")
        app.realize()
        app.set_rhs(su.normal_global(size, dtype))
        res = app.solve(tol=cu.TOL[dtype], max_iter=cu.MAX_ITER, overlap=overlap)
        assert res.converged
        runs.append(res)
    assert abs(runs[0].iterations - runs[1].iterations) <= 1
