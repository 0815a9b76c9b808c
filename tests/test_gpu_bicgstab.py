"""The fused vector operations of BiCGStab and the solver on the GPU
(csrc/src/vector_ops.hip): axpby_norm2 / dot_pair / bicgstab_update against
exact numpy oracles, what they share with the existing ops bit for bit,
their containment contract, determinism and validation, and the native
solver against the boundary-aware truth operator."""
import numpy as np
import pytest

from stencil_amd import Next, _C

import bicgstab_util as bu
import cg_util as cu
import stencil_util as su
from util import full_region_of

pytestmark = pytest.mark.gpu

DTYPES, DT_IDS = bu.DTYPES, bu.DT_IDS

# The shapes of test_gpu_vector_bits.py, the smallest that reach every path
# of the walks. name: (size, box lo, box hi). The strips walk with head 3
# (fp32) / 1 (fp64), tail 3 and three z chunks; a row wider than one 64-lane
# block; several blocks in x, y and z with head 0; the linearised walk
# (narrower than 8).
CASES = {
    "19x5x65-x1": ((19, 5, 65), (1, 0, 0), (19, 5, 65)),
    "261x5x3": ((261, 5, 3), (0, 0, 0), (261, 5, 3)),
    "61x19x37": ((61, 19, 37), (0, 0, 0), (61, 19, 37)),
    "thin-5,2,1": ((19, 10, 9), (5, 2, 1), (12, 9, 7)),
}
ALPHA, BETA, OMEGA = 0.37, -1.25, 0.3  # 0.37 and 0.3 are rounded to fp32 once


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


# ------------------------------------------------------------------ exact ops
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", sorted(CASES))
def test_ops_exact(case, dtype):
    size, lo, hi = CASES[case]
    bu.run_ops_exact("native", size, lo, hi, dtype, [0])


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_ops_exact_two_domains(dtype):
    size = (19, 10, 9)
    bu.run_ops_exact("native", size, (0, 0, 0), size, dtype, [0, 0])


# ------------------------------------------------- shared with the existing ops
def _normal_domain(size, dtype, nq=6):
    dd, hs = cu.vector_domain(size, [dtype] * nq, "native", [0])
    gs = [su.normal_global(size, dtype, seed=s + 1) for s in range(nq)]

    def fill():
        for h, g in zip(hs, gs):
            su.scatter(dd, h, g)
        su.scatter(dd, hs[0], su.normal_global(size, dtype, seed=11), to_next=True)

    fill()
    return dd, hs, gs, fill


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", sorted(CASES))
def test_ops_share_bits_with_the_existing_ops(case, dtype):
    """seeded normal data, arbitrary scalars: the new ops run the launch
    shape and the arithmetic of axpby, dot and cg_update, so what both
    compute has the same bits"""
    size, lo, hi = CASES[case]
    box = (lo, hi)
    dd, (a, b, c, d, e, f), gs, fill = _normal_domain(size, dtype)

    # axpby_norm2 writes what axpby writes, and returns dot(out)
    dd.axpby(ALPHA, a, BETA, Next(a), out=c, where=box)
    dd.backend.sync_compute()
    want = su.gather(dd, c)
    nn = dd.axpby_norm2(ALPHA, a, BETA, Next(a), out=d, where=box)
    got = su.gather(dd, d)
    bx = bu.box_slices(lo, hi)
    np.testing.assert_array_equal(_bits(got[bx]), _bits(want[bx]))
    assert nn == dd.dot(d, where=box)

    # dot_pair is (dot(a, b), dot(a, a))
    fill()
    ab, aa = dd.dot_pair(Next(a), b, where=box)
    assert ab == dd.dot(Next(a), b, where=box)
    assert aa == dd.dot(Next(a), where=box)

    # bicgstab_update: omega = 0 leaves r alone; its first value is dot(r),
    # its second dot(rhat, r)
    def update(alpha, omega):
        per = dd.backend.bicgstab_update([box], alpha, a.index, False, omega, b.index, False,
                                         c.index, d.index, a.index, True, e.index, False)
        return per[0]

    fill()
    before = su.gather(dd, d)
    rr, rho = update(ALPHA, 0.0)
    np.testing.assert_array_equal(_bits(su.gather(dd, d)), _bits(before))
    assert rr == dd.dot(d, where=box)
    assert rho == dd.dot(e, d, where=box)
    rr, rho = update(ALPHA, OMEGA)
    assert not np.array_equal(su.gather(dd, d)[bx], before[bx])
    assert rr == dd.dot(d, where=box)
    assert rho == dd.dot(e, d, where=box)


# ---------------------------------------------------------------- containment
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", sorted(CASES))
def test_ops_containment(case, dtype):
    """NaN in every cell outside the box of every buffer, halos included:
    the values are finite and those of the clean run, every cell outside
    the box of a written buffer keeps its bits, unwritten operands keep
    theirs everywhere"""
    size, lo, hi = CASES[case]
    box, bx = (lo, hi), bu.box_slices(lo, hi)
    gs = [bu.small_ints(size, dtype, seed) for seed in range(1, 9)]

    def run(poison):
        dd, hs = su.make_domain(size, _C.Radius.constant(2), [dtype] * 6, "native", [0])
        flo, fhi = full_region_of(dd, 0)
        shape = (fhi[2] - flo[2], fhi[1] - flo[1], fhi[0] - flo[0])
        base = np.full(shape, np.nan if poison else 0.0, dtype=dtype)
        o = tuple(lo[i] - flo[i] for i in range(3))
        inner = tuple(slice(o[a], o[a] + hi[a] - lo[a]) for a in (2, 1, 0))

        def full(g):
            w = base.copy()
            w[inner] = g[bx]
            return w

        def put(h, g, nxt=False):
            dd.write_global(0, flo, full(g), h, to_next=nxt)

        def get(h, nxt=False):
            dd.backend.sync_compute()
            return dd.read_global(0, flo, fhi, h, from_next=nxt)

        a, b, c, d, e, f = hs
        for h, g in zip(hs, gs):
            put(h, g)
            put(h, gs[6] if h is a else gs[7], nxt=True)
        vals = [dd.axpby_norm2(bu.ALPHA, a, bu.BETA, Next(b), out=f, where=box),
                dd.dot_pair(Next(a), b, where=box)]
        out_f = get(f)
        per = dd.backend.bicgstab_update([box], bu.ALPHA, a.index, False, bu.OMEGA, d.index, False,
                                         c.index, d.index, d.index, True, e.index, False)
        vals.append(per[0])
        bufs = {"f": out_f, "x": get(c), "r": get(d)}
        # unwritten: every operand that was only read, and every next buffer
        for name, h, nxt, g in (("a", a, False, gs[0]), ("b", b, False, gs[1]),
                                ("e", e, False, gs[4]), ("a'", a, True, gs[6]),
                                ("b'", b, True, gs[7]), ("d'", d, True, gs[7]),
                                ("c'", c, True, gs[7])):
            np.testing.assert_array_equal(_bits(get(h, nxt)), _bits(full(g)), err_msg=name)
        return vals, bufs, inner, base

    clean, cbufs, inner, _ = run(False)
    dirty, dbufs, _, base = run(True)
    assert dirty == clean
    assert all(np.isfinite(v).all() for v in np.asarray(dirty[0:1] + list(dirty[1]) + list(dirty[2])))
    out, nn = bu.oracle_axpby_norm2(gs[0], gs[7], bx)
    xn, rn, pair = bu.oracle_bicgstab_update(gs[0], gs[3], gs[2], gs[3], gs[7], gs[4], bx)
    assert clean == [nn, bu.oracle_dot_pair(gs[6], gs[1], bx), pair]
    for name, part in (("f", out), ("x", xn), ("r", rn)):
        want = base.copy()
        want[inner] = part
        np.testing.assert_array_equal(_bits(dbufs[name]), _bits(want), err_msg=name)
        np.testing.assert_array_equal(_bits(cbufs[name][inner]), _bits(part), err_msg=name)


# ---------------------------------------------------------------- determinism
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_ops_are_deterministic(dtype):
    size = (61, 19, 37)
    dd, (a, b, c, d, e, f), gs, fill = _normal_domain(size, dtype)
    runs = []
    for _ in range(2):
        fill()
        runs.append((dd.axpby_norm2(ALPHA, a, BETA, b, out=f),
                     dd.dot_pair(Next(a), b),
                     dd.bicgstab_update(ALPHA, a, OMEGA, d, c, d, Next(a), e),
                     su.gather(dd, c).tobytes(), su.gather(dd, d).tobytes()))
    assert runs[0] == runs[1]


# ----------------------------------------------------------------- validation
def test_validation_launches_nothing():
    size = (19, 10, 9)
    dd, (f, g, e, h, i32, d) = su.make_domain(
        size, _C.Radius.constant(1), [np.float32] * 4 + [np.int32, np.float64], "native", [0])
    flo, fhi = full_region_of(dd, 0)
    sent = np.full((fhi[2] - flo[2], fhi[1] - flo[1], fhi[0] - flo[0]), -99.0, dtype=np.float32)
    for q in (f, g, e, h):
        dd.write_global(0, flo, sent, q)
    outside = ((flo[0] - 1, 0, 0), (5, 5, 5))
    beyond = ((0, 0, 0), (fhi[0] + 1, 5, 5))
    with pytest.raises(ValueError):
        dd.axpby_norm2(1.0, f, 1.0, d, out=g)
    with pytest.raises(ValueError):
        dd.axpby_norm2(1.0, f, 1.0, g, out=i32)
    with pytest.raises(ValueError):
        dd.dot_pair(f, d)
    with pytest.raises(ValueError):
        dd.bicgstab_update(1.0, f, 1.0, g, e, h, Next(g), d)
    for args in ((f, g, e, e, Next(g), f),  # x is r
                 (e, g, e, h, Next(g), f),  # y is x
                 (f, g, e, h, h, f),        # t is r
                 (f, g, e, h, Next(g), e)):  # rhat is x
        y, z, x, r, t, rh = args
        with pytest.raises(ValueError):
            dd.bicgstab_update(1.0, y, 1.0, z, x, r, t, rh)
    for where in (outside, beyond):
        with pytest.raises(ValueError):
            dd.axpby_norm2(2.0, f, 2.0, f, out=g, where=where)
        with pytest.raises(ValueError):
            dd.dot_pair(f, g, where=where)
        with pytest.raises(ValueError):
            dd.backend.bicgstab_update([where], 1.0, f.index, False, 1.0, g.index, False, e.index,
                                       h.index, g.index, True, f.index, False)
    # below the dtype checks of DistributedDomain: element sizes and indices
    eng = dd.backend.engine
    rect = _C.Rect3(_C.Vec3(0, 0, 0), _C.Vec3(5, 5, 5))
    with pytest.raises(ValueError):
        _C.field_dot_pair(eng, 0, f.index, False, d.index, False, rect)
    with pytest.raises(ValueError):
        _C.field_axpby_norm2(eng, 0, 1.0, f.index, False, 1.0, f.index, False, 17, False, rect)
    with pytest.raises(ValueError):
        _C.field_dot_pair(eng, 3, f.index, False, f.index, False, rect)
    with pytest.raises(ValueError):
        _C.bicgstab_update(eng, 0, 1.0, f.index, False, 1.0, g.index, False, e.index, e.index,
                           g.index, True, f.index, False, rect)
    with pytest.raises(ValueError):
        _C.bicgstab_update(eng, 0, 1.0, f.index, False, 1.0, g.index, False, e.index, h.index,
                           g.index, True, d.index, False, rect)
    # nothing stayed in flight, and an empty region is a no-op returning 0
    empty = ((2, 2, 2), (2, 5, 5))
    assert dd.dot_pair(f, g, where=empty) == (0.0, 0.0)
    assert dd.axpby_norm2(2.0, f, 2.0, f, out=g, where=empty) == 0.0
    assert dd.backend.bicgstab_update([empty], 1.0, f.index, False, 1.0, g.index, False, e.index,
                                      h.index, g.index, True, f.index, False) == [(0.0, 0.0)]
    dd.backend.sync_compute()
    for q in (f, g, e, h):
        got = dd.read_global(0, flo, fhi, q)
        np.testing.assert_array_equal(got.view(np.uint8), sent.view(np.uint8))


# ----------------------------------------------------- solver against the truth
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", bu.SOLVER_CASES, ids=bu.case_id)
def test_solver_native_against_the_truth(case, dtype):
    res, x, b, app = bu.solve_case("native", case, dtype)
    bu.check_solution(res, x, b, app, case, dtype, "native")


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("gpus", [[0], [0, 0]], ids=["1dom", "2dom"])
def test_multigrid_preconditioner_native(gpus, dtype):
    case = bu.MG_CASE + (gpus,)
    plain = bu.solve_case("native", case, dtype)
    pre = bu.solve_case("native", case, dtype, preconditioner="multigrid")
    bu.check_solution(*plain, case, dtype, "native plain")
    bu.check_solution(*pre, case, dtype, "native multigrid")
    print(f"iterations: plain {plain[0].iterations}, multigrid {pre[0].iterations}")
    assert pre[0].iterations < plain[0].iterations


def test_breakdown_native():
    """the periodic shift and a single 1: rhat . v == 0 exactly"""
    import stencil_amd as sa
    from stencil_amd.solvers import BiCGStab

    size = (19, 10, 9)
    st = sa.Stencil([(1, 0, 0)], [1.0])
    dd = sa.DistributedDomain(*size, backend="native")
    dd.set_radius(st.radius())
    dd.set_gpus([0])
    x, b, r, rhat, p = (dd.add_data(np.float32, n) for n in ("x", "b", "r", "rhat", "p"))
    dd.set_exchange_groups([[p.index], [r.index], [x.index]])
    dd.realize()
    gb = np.zeros((size[2], size[1], size[0]), dtype=np.float32)
    gb[4, 5, 6] = 1.0
    su.scatter(dd, b, gb)
    su.scatter(dd, p, np.full_like(gb, np.nan))
    res = BiCGStab(dd, st, x, b, r, rhat, p, 0, 1, 2).solve(tol=1e-6, max_iter=20)
    assert not res.converged and res.reason == "breakdown" and res.iterations <= 1
