"""The kernels of the null-space projection on the GPU
(csrc/src/vector_ops.hip: field_sum, field_dot_sums, cg_update_sum,
field_axpbyc) against exact numpy oracles, their containment contract,
determinism and validation, the existing reductions' bits next to them, and
the singular solves on the native backend."""
import numpy as np
import pytest

from stencil_amd import Next, _C

import cg_util as cu
import nullspace_util as nu
import stencil_util as su
from util import full_region_of

pytestmark = pytest.mark.gpu

DTYPES, DT_IDS = nu.DTYPES, nu.DT_IDS

# the shapes of test_gpu_cg.py: x 8..19 gives tail 0..3 (and head 0..3 once
# the box start moves, see X0S), y 4..7 rows cut off at the block edge,
# z 3 / 33 / 65 several z chunks. 261 x 5 x 3: a row spans more than one
# 64-lane block in x.
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
THIN = ((19, 10, 9), (5, 2, 1), (12, 9, 7))  # narrower than 8 cells: the linearised walk


def _sid(s):
    return "x".join(map(str, s))


def _cg_update_sum_box(size, lo, hi, dtype):
    """cg_update_sum over a box through the backend (DistributedDomain takes
    local_rect), against numpy and against cg_update on a copy"""
    gx, gp, gr, gap = nu.cg_fields(size, dtype)
    alpha, bx = 0.25, nu.box_of(lo, hi)
    outs = []
    for with_sum in (True, False):
        dd, (x, p, r) = cu.vector_domain(size, [dtype] * 3, "native", [0])
        su.scatter(dd, x, gx)
        su.scatter(dd, p, gp)
        su.scatter(dd, p, gap, to_next=True)
        su.scatter(dd, r, gr)
        op = dd.backend.cg_update_sum if with_sum else dd.backend.cg_update
        (v,) = op([(lo, hi)], alpha, x.index, p.index, r.index)
        outs.append((v, su.gather(dd, x), su.gather(dd, r)))
    rn = (gr - alpha * gap).astype(dtype)
    wx, wr = gx.copy(), gr.copy()
    wx[bx] = (gx + alpha * gp).astype(dtype)[bx]
    wr[bx] = rn[bx]
    (v, ox, orr), (rr0, ox0, or0) = outs
    assert v == (float((nu.f64(rn[bx]) ** 2).sum()), float(nu.f64(rn[bx]).sum()))
    assert v[0] == rr0
    nu.same_bits(ox, wx, "x")
    nu.same_bits(orr, wr, "r")
    nu.same_bits(ox, ox0, "x against cg_update")
    nu.same_bits(orr, or0, "r against cg_update")


# ----------------------------------------------------------------- exactness
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("x0", X0S)
@pytest.mark.parametrize("size", R1_SHAPES, ids=_sid)
def test_kernels_exact(size, x0, dtype):
    """integers below 753 and dyadic coefficients: every product < 2^20,
    every sum < 2^53, so each value equals numpy's in any order"""
    box = () if x0 == 0 else ((x0, 0, 0), size)
    nu.check_reductions_exact("native", size, [0], dtype, *box)
    nu.check_axpbyc_exact("native", size, [0], dtype, *box)
    _cg_update_sum_box(size, (x0, 0, 0), size, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_kernels_exact_thin_box(dtype):
    size, lo, hi = THIN
    nu.check_reductions_exact("native", size, [0], dtype, lo, hi)
    nu.check_axpbyc_exact("native", size, [0], dtype, lo, hi)
    _cg_update_sum_box(size, lo, hi, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("gpus", [[0], [0, 0]], ids=["1dom", "2dom"])
@pytest.mark.parametrize("size", [(9, 5, ZC + 1), (19, 10, 9), (261, 5, 3)], ids=_sid)
def test_domains_exact(size, gpus, dtype):
    nu.check_cg_update_sum_exact("native", size, gpus, dtype)
    if len(gpus) == 2:
        nu.check_reductions_exact("native", size, gpus, dtype)
        nu.check_axpbyc_exact("native", size, gpus, dtype)


# ---------------------------------------------------------------- containment
CONTRACT_SIZE = (24, 10, 9)
_BOXES = {
    # x start odd; the thin box is narrower than 8 cells (linearised path)
    "wide": ((3, 1, 1), (20, 8, 8)),
    "thin": ((5, 2, 1), (12, 9, 7)),
}
_SENTINELS = {"sentinel": -99.0, "nan": np.nan}


def _sentinel_domain(dtype, nq, sentinel):
    dd, hs = su.make_domain(CONTRACT_SIZE, _C.Radius.constant(2), [dtype] * nq, "native", [0])
    flo, fhi = full_region_of(dd, 0)
    sent = np.full((fhi[2] - flo[2], fhi[1] - flo[1], fhi[0] - flo[0]), sentinel, dtype=dtype)
    for h in hs:
        for to_next in (False, True):
            dd.write_global(0, flo, sent, h, to_next=to_next)
    return dd, hs, flo, fhi, sent


def _put(dd, h, g, lo, hi, to_next=False):
    dd.write_global(0, lo, np.ascontiguousarray(g[nu.box_of(lo, hi)]), h, to_next=to_next)


def _expect(sent, flo, lo, hi, g):
    want = sent.copy()
    o = tuple(lo[i] - flo[i] for i in range(3))
    e = tuple(hi[i] - lo[i] for i in range(3))
    want[o[2]:o[2] + e[2], o[1]:o[1] + e[1], o[0]:o[0] + e[0]] = g[nu.box_of(lo, hi)]
    return want


def _assert_buffer(dd, flo, fhi, h, nxt, want):
    got = dd.read_global(0, flo, fhi, h, from_next=nxt)
    np.testing.assert_array_equal(got.view(np.uint8), want.view(np.uint8))


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("sentinel", sorted(_SENTINELS))
@pytest.mark.parametrize("box", sorted(_BOXES))
def test_reductions_and_axpbyc_containment(box, sentinel, dtype):
    """the sentinel (NaN in one variant) fills everything outside the box in
    every operand, both buffers, and a bystander quantity"""
    lo, hi = _BOXES[box]
    dd, (a, b, c, by), flo, fhi, sent = _sentinel_domain(dtype, 4, _SENTINELS[sentinel])
    ga, gb = su.ripple_global(CONTRACT_SIZE, dtype), nu.second(CONTRACT_SIZE, dtype)
    bx = nu.box_of(lo, hi)
    _put(dd, a, ga, lo, hi)
    _put(dd, b, gb, lo, hi, to_next=True)
    sa_, sb_ = float(nu.f64(ga[bx]).sum()), float(nu.f64(gb[bx]).sum())
    # no cell outside the box enters the arithmetic: finite and exact
    assert dd.sum(a, where=(lo, hi)) == sa_
    assert dd.dot_sums(a, Next(b), where=(lo, hi)) == (
        float((nu.f64(ga[bx]) * nu.f64(gb[bx])).sum()), sa_, sb_)
    dd.axpbyc(0.5, a, -0.25, Next(b), 1.5, out=c, where=(lo, hi))
    dd.axpbyc(2.0, a, 0.5, Next(b), -0.5, out=a, where=(lo, hi))  # in place
    dd.backend.sync_compute()
    _assert_buffer(dd, flo, fhi, c, False, _expect(sent, flo, lo, hi, 0.5 * ga - 0.25 * gb + 1.5))
    _assert_buffer(dd, flo, fhi, a, False, _expect(sent, flo, lo, hi, 2.0 * ga + 0.5 * gb - 0.5))
    _assert_buffer(dd, flo, fhi, b, True, _expect(sent, flo, lo, hi, gb))
    for h, nxt in ((a, True), (b, False), (c, True), (by, False), (by, True)):
        _assert_buffer(dd, flo, fhi, h, nxt, sent)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("sentinel", sorted(_SENTINELS))
@pytest.mark.parametrize("box", sorted(_BOXES))
def test_cg_update_sum_containment(box, sentinel, dtype):
    lo, hi = _BOXES[box]
    dd, (x, p, r, by), flo, fhi, sent = _sentinel_domain(dtype, 4, _SENTINELS[sentinel])
    gx, gp, gr, gap = nu.cg_fields(CONTRACT_SIZE, dtype)
    _put(dd, x, gx, lo, hi)
    _put(dd, p, gp, lo, hi)
    _put(dd, p, gap, lo, hi, to_next=True)
    _put(dd, r, gr, lo, hi)
    alpha = 0.25
    (v,) = dd.backend.cg_update_sum([(lo, hi)], alpha, x.index, p.index, r.index)
    rn = gr - alpha * gap
    sub = nu.f64(rn[nu.box_of(lo, hi)])
    assert v == (float((sub ** 2).sum()), float(sub.sum()))
    _assert_buffer(dd, flo, fhi, x, False, _expect(sent, flo, lo, hi, gx + alpha * gp))
    _assert_buffer(dd, flo, fhi, r, False, _expect(sent, flo, lo, hi, rn))
    _assert_buffer(dd, flo, fhi, p, False, _expect(sent, flo, lo, hi, gp))
    _assert_buffer(dd, flo, fhi, p, True, _expect(sent, flo, lo, hi, gap))
    for h, nxt in ((x, True), (r, True), (by, False), (by, True)):
        _assert_buffer(dd, flo, fhi, h, nxt, sent)


# ---------------------------------------------------------------- determinism
def _normal_cg_domain(size, dtype):
    dd, (x, p, r) = cu.vector_domain(size, [dtype] * 3, "native", [0])
    for h, seed in ((x, 1), (p, 2), (r, 3)):
        su.scatter(dd, h, su.normal_global(size, dtype, seed=seed))
    su.scatter(dd, p, su.normal_global(size, dtype, seed=4), to_next=True)
    return dd, x, p, r


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_reductions_are_deterministic(dtype):
    size = (61, 19, 37)
    runs = []
    for _ in range(2):
        dd, x, p, r = _normal_cg_domain(size, dtype)
        runs.append((dd.dot_sums(x, Next(p)), dd.dot_sums(r), dd.sum(p),
                     dd.cg_update_sum(0.37, x, p, r)))
        again = (dd.dot_sums(p, Next(p)), dd.dot_sums(p, Next(p)))
        assert again[0] == again[1]
    assert runs[0] == runs[1]
    # and the values are the sums: fp64 accumulation of n terms
    ga, gn = su.normal_global(size, dtype, seed=1), su.normal_global(size, dtype, seed=4)
    wide = su._wide(np.float64)
    eps = (ga.size + 1) * np.finfo(np.float64).eps
    ab, s_a, s_n = runs[0][0]
    assert abs(ab - float((ga.astype(wide) * gn.astype(wide)).sum())) <= eps * float(
        (np.abs(ga).astype(wide) * np.abs(gn).astype(wide)).sum())
    assert abs(s_a - float(ga.astype(wide).sum())) <= eps * float(np.abs(ga).astype(wide).sum())
    assert abs(s_n - float(gn.astype(wide).sum())) <= eps * float(np.abs(gn).astype(wide).sum())


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
        dd.sum(i32)
    with pytest.raises(ValueError):
        dd.dot_sums(f, d)
    with pytest.raises(ValueError):
        dd.axpbyc(1.0, f, 1.0, d, 1.0, out=g)
    with pytest.raises(ValueError):
        dd.axpbyc(1.0, f, 1.0, f, 1.0, out=i32)
    with pytest.raises(ValueError):
        dd.cg_update_sum(1.0, f, g, d)
    for where in (outside, beyond):
        with pytest.raises(ValueError):
            dd.sum(f, where=where)
        with pytest.raises(ValueError):
            dd.dot_sums(f, g, where=where)
        with pytest.raises(ValueError):
            dd.axpbyc(2.0, f, 2.0, f, 1.0, out=g, where=where)
        with pytest.raises(ValueError):
            dd.backend.cg_update_sum([where], 1.0, f.index, g.index, e.index)
    # below the dtype checks of DistributedDomain: element sizes and indices
    eng = dd.backend.engine
    rect = _C.Rect3(_C.Vec3(0, 0, 0), _C.Vec3(5, 5, 5))
    with pytest.raises(ValueError):
        _C.field_sum(eng, 0, 17, False, rect)
    with pytest.raises(ValueError):
        _C.field_sum(eng, 3, f.index, False, rect)
    with pytest.raises(ValueError):
        _C.field_dot_sums(eng, 0, f.index, False, d.index, False, rect)
    with pytest.raises(ValueError):
        _C.field_axpbyc(eng, 0, 1.0, f.index, False, 1.0, f.index, False, 1.0, d.index, False,
                        rect)
    with pytest.raises(ValueError):
        _C.field_axpbyc(eng, 0, 1.0, f.index, False, 1.0, f.index, False, 1.0, 17, False, rect)
    with pytest.raises(ValueError):
        _C.cg_update_sum(eng, 0, 1.0, f.index, f.index, g.index, rect)  # x == p
    with pytest.raises(ValueError):
        _C.cg_update_sum(eng, 0, 1.0, f.index, g.index, d.index, rect)
    # none of the refused calls left a reduction in flight
    with pytest.raises(RuntimeError):
        _C.reduction_end_n(eng, 0, 3)
    # one reduction per domain: a second begin is refused, the first survives
    _C.field_dot_sums_begin(eng, 0, f.index, False, g.index, False, rect)
    for begin in (lambda: _C.field_sum_begin(eng, 0, f.index, False, rect),
                  lambda: _C.field_dot_sums_begin(eng, 0, f.index, False, f.index, False, rect),
                  lambda: _C.cg_update_sum_begin(eng, 0, 1.0, f.index, g.index, e.index, rect),
                  lambda: _C.field_dot_begin(eng, 0, f.index, False, g.index, False, rect)):
        with pytest.raises(RuntimeError):
            begin()
    # the value count must match: reduction_end is for one value
    with pytest.raises(RuntimeError):
        _C.reduction_end(eng, 0)
    with pytest.raises(RuntimeError):
        _C.reduction_end_n(eng, 0, 2)
    with pytest.raises(ValueError):
        _C.reduction_end_n(eng, 0, 4)
    n = 5 * 5 * 5
    assert _C.reduction_end_n(eng, 0, 3) == (99.0 * 99.0 * n, -99.0 * n, -99.0 * n)
    _C.field_dot_begin(eng, 0, f.index, False, g.index, False, rect)
    with pytest.raises(RuntimeError):
        _C.reduction_end_n(eng, 0, 3)
    assert _C.reduction_end(eng, 0) == 99.0 * 99.0 * n
    _C.field_sum_begin(eng, 0, f.index, False, rect)
    assert _C.reduction_end(eng, 0) == -99.0 * n  # one value: either end call
    # an empty region is a no-op returning zeros
    empty = ((2, 2, 2), (2, 5, 5))
    assert dd.sum(f, where=empty) == 0.0
    assert dd.dot_sums(f, g, where=empty) == (0.0, 0.0, 0.0)
    dd.axpbyc(2.0, f, 2.0, f, 1.0, out=g, where=empty)
    assert dd.backend.cg_update_sum([empty], 1.0, f.index, g.index, e.index) == [(0.0, 0.0)]
    dd.backend.sync_compute()
    for h in (f, g, e):
        got = dd.read_global(0, flo, fhi, h)
        np.testing.assert_array_equal(got.view(np.uint8), sent.view(np.uint8))


# ------------------------------------------------------- existing ops unchanged
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_existing_reductions_keep_their_bits(dtype):
    """dot and cg_update before and after a three-valued reduction on the
    same domain: the enlarged scratch changes neither their launch shape
    nor where their partials land"""
    size = (19, 5, 2 * ZC + 1)

    def run(with_sums):
        dd, x, p, r = _normal_cg_domain(size, dtype)
        if with_sums:
            dd.dot_sums(x, Next(p))
            dd.sum(r)
        vals = [dd.dot(x, Next(p)), dd.dot(r)]
        if with_sums:
            dd.dot_sums(p, r)
        vals.append(dd.cg_update(0.37, x, p, r))
        if with_sums:
            dd.cg_update_sum(0.0, x, p, r)  # alpha = 0: x and r keep their bits
        vals.append(dd.dot(r))
        return vals, su.gather(dd, x), su.gather(dd, r)

    (v0, x0, r0), (v1, x1, r1) = run(False), run(True)
    assert v0 == v1
    nu.same_bits(x0, x1)
    nu.same_bits(r0, r1)


# ------------------------------------------------------------------------ solves
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", nu.SOLVE_CASES, ids=nu.solve_id)
def test_singular_solves_native(case, dtype):
    nu.check_solve("native", case, dtype)


@pytest.mark.parametrize("case", nu.COEFF_CASES, ids=nu.coeff_id)
def test_singular_solves_with_a_coefficient_jump_native(case):
    nu.check_coefficient_solve("native", case)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_constant_rhs_is_a_zero_rhs_native(dtype):
    nu.check_constant_rhs("native", dtype, [0, 0])
