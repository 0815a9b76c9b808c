"""Generic stencil operator on the GPU (csrc/src/stencil_op.hip):
stencil_star_kernel<T, R> (16 B strips, z march) and stencil_taps_kernel<T>
(tap table), against the two oracles of stencil_util, plus the operator's
hard contract: nothing written outside the region, nothing read outside
region (+) offsets."""
import numpy as np
import pytest

import stencil_amd as sa
from stencil_amd import Boundary, Stencil, _C

import boundary_util
import stencil_util as su
from util import full_region_of, ripple_block

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
DT_IDS = ["f32", "f64"]

# ZC = 32 is the star kernel's default z chunk (kDefaultZc, STENCIL_OP_ZC).
# x 8..19: head = 0..3 cells before the first 16 B-aligned address (the
# allocation pad puts the interior start on one for radius 1, the sub-box
# tests below move it), tail 0..3, and 19 has more than one strip per
# side; y 4..7: every extY % 4 with rows cut off at the block edge;
# z 3 / ZC+1 / 2*ZC+1: chunks that do not start at plane 0.
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
]
# every extent > 2R up to R = 4
RN_SHAPES = [(19, 10, 9), (17, 9, ZC + 1)]


def _sid(s):
    return "x".join(map(str, s))


def _apply_periodic(size, st, dtype, g, gpus=(0,), radius=None, where="all"):
    dd, (h,) = su.make_domain(size, radius if radius is not None else st.radius(), [dtype],
                              "native", list(gpus))
    su.scatter(dd, h, g)
    su.apply_once(dd, st, h, where=where)
    return su.gather(dd, h, from_next=True)


# ------------------------------------------------------------- star, exact
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("size", R1_SHAPES, ids=_sid)
def test_star_r1_exact(size, dtype):
    st = su.exact_star(1)
    g = su.ripple_global(size, dtype)
    np.testing.assert_array_equal(_apply_periodic(size, st, dtype, g), su.exact_oracle(g, st))


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("size", RN_SHAPES, ids=_sid)
@pytest.mark.parametrize("r", [2, 3, 4])
def test_star_rn_exact(r, size, dtype):
    st = su.exact_star(r)
    g = su.ripple_global(size, dtype)
    np.testing.assert_array_equal(_apply_periodic(size, st, dtype, g), su.exact_oracle(g, st))


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("r", [1, 2, 3, 4])
def test_star_under_a_wider_halo(r, dtype):
    """radius constant(4) moves the interior start: other head/tail splits
    than the derived radius gives"""
    st = su.exact_star(r)
    size = RN_SHAPES[0]
    g = su.ripple_global(size, dtype)
    got = _apply_periodic(size, st, dtype, g, radius=_C.Radius.constant(4))
    np.testing.assert_array_equal(got, su.exact_oracle(g, st))


# ---------------------------------------------------- laplacian, bounded
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("size", RN_SHAPES, ids=_sid)
@pytest.mark.parametrize("order", [2, 4, 6, 8])
def test_laplacian_bounded(order, size, dtype):
    st = Stencil.laplacian(order, spacing=(1.0, 0.7, 1.3))
    g = su.normal_global(size, dtype)
    ref, mag = su.roll_sum(g, st)
    got = _apply_periodic(size, st, dtype, g)
    su.assert_within_bound(got, ref, su.bound_of(st, mag, dtype), f"laplacian{order}")


# ------------------------------------------------------------ general path
_BOXES = {"box3": su.exact_box3(), "asymbox": su.exact_asym_box()}


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("name", sorted(_BOXES))
def test_box_exact(name, dtype):
    st = _BOXES[name]
    size = RN_SHAPES[0]
    g = su.ripple_global(size, dtype)
    np.testing.assert_array_equal(_apply_periodic(size, st, dtype, g), su.exact_oracle(g, st))


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("name", sorted(_BOXES))
def test_box_bounded(name, dtype):
    base = _BOXES[name]
    # the same taps with non-dyadic weights
    st = Stencil(base.offsets, [w / 3.0 + 0.1 for w in base.weights])
    size = RN_SHAPES[1]
    g = su.normal_global(size, dtype)
    ref, mag = su.roll_sum(g, st)
    got = _apply_periodic(size, st, dtype, g)
    su.assert_within_bound(got, ref, su.bound_of(st, mag, dtype), name)


# --------------------------------------------------------- the hard contract
SENTINEL = -99.0
CONTRACT_SIZE = (24, 10, 9)


def _full_block(dd, value, dtype):
    flo, fhi = full_region_of(dd, 0)
    shape = (fhi[2] - flo[2], fhi[1] - flo[1], fhi[0] - flo[0])
    return flo, fhi, np.full(shape, value, dtype=dtype)


_CONTAIN = {
    # name: (stencil, sub-box): x start odd; the thin box is < 8 cells wide
    "star": (su.exact_star(2), ((3, 1, 1), (20, 8, 8))),
    "star-thin": (su.exact_star(2), ((5, 2, 1), (12, 9, 7))),
    "general": (su.exact_box3(), ((3, 1, 1), (20, 8, 8))),
}


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("name", sorted(_CONTAIN))
def test_write_containment(name, dtype):
    st, (lo, hi) = _CONTAIN[name]
    size = CONTRACT_SIZE
    dd, (a, b) = su.make_domain(size, _C.Radius.constant(2), [dtype, dtype], "native", [0])
    flo, fhi, sent = _full_block(dd, SENTINEL, dtype)
    for h in (a, b):
        for to_next in (False, True):
            dd.write_global(0, flo, sent, h, to_next=to_next)
    g = su.ripple_global(size, dtype)
    su.scatter(dd, a, g)
    dd.exchange()
    dd.apply_stencil(st, a, where=(lo, hi))
    dd.backend.sync_compute()
    want = sent.copy()
    o = tuple(lo[i] - flo[i] for i in range(3))
    e = tuple(hi[i] - lo[i] for i in range(3))
    box = (slice(o[2], o[2] + e[2]), slice(o[1], o[1] + e[1]), slice(o[0], o[0] + e[0]))
    want[box] = su.exact_oracle(g, st)[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]]
    got = dd.read_global(0, flo, fhi, a, from_next=True)
    np.testing.assert_array_equal(got.view(np.uint8), want.view(np.uint8))
    # the second quantity's next buffer and both current buffers are untouched
    other = dd.read_global(0, flo, fhi, b, from_next=True)
    np.testing.assert_array_equal(other.view(np.uint8), sent.view(np.uint8))
    np.testing.assert_array_equal(dd.read_global(0, flo, fhi, b).view(np.uint8),
                                  sent.view(np.uint8))


def test_write_to_second_quantity():
    st = su.exact_star(1)
    size = CONTRACT_SIZE
    dd, (a, b) = su.make_domain(size, st.radius(), [np.float32, np.float32], "native", [0])
    g = su.ripple_global(size, np.float32)
    su.scatter(dd, a, g)
    su.scatter(dd, a, np.full_like(g, SENTINEL), to_next=True)
    su.apply_once(dd, st, a, b)
    np.testing.assert_array_equal(su.gather(dd, b, from_next=True), su.exact_oracle(g, st))
    assert (su.gather(dd, a, from_next=True) == SENTINEL).all()


_READ = {
    "upwind-x-star": su.upwind_x(),
    "asymbox": su.exact_asym_box(),
}


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("box", ["all", "sub"])
@pytest.mark.parametrize("name", sorted(_READ))
def test_read_containment(name, box, dtype):
    """every allocated cell outside region (+) offsets is NaN: a read of
    one that reaches the arithmetic makes the output non-finite"""
    st = _READ[name]
    size = RN_SHAPES[0]
    dd, (h,) = su.make_domain(size, _C.Radius.constant(4), [dtype], "native", [0])
    lo, hi = ((0, 0, 0), size) if box == "all" else ((3, 1, 1), (18, 9, 8))
    flo, fhi, cur = _full_block(dd, np.nan, dtype)
    offs = st.offsets
    rlo = tuple(lo[i] + min(o[i] for o in offs) for i in range(3))
    rhi = tuple(hi[i] + max(o[i] for o in offs) for i in range(3))
    p = tuple(rlo[i] - flo[i] for i in range(3))
    e = tuple(rhi[i] - rlo[i] for i in range(3))
    # dense boxes and one-axis stars: region (+) offsets is the box rlo..rhi
    cur[p[2]:p[2] + e[2], p[1]:p[1] + e[1], p[0]:p[0] + e[0]] = ripple_block(
        rlo, rhi, size).astype(dtype)
    dd.write_global(0, flo, cur, h)
    dd.apply_stencil(st, h, where=(lo, hi))  # no exchange: it would refill the halos
    dd.backend.sync_compute()
    got = dd.read_global(0, lo, hi, h, from_next=True)
    assert np.isfinite(got).all()
    g = su.ripple_global(size, dtype)
    np.testing.assert_array_equal(got, su.exact_oracle(g, st)[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]])


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("path", ["star", "general"])
@pytest.mark.parametrize("gpus", [[0], [0, 0]], ids=["1dom", "2dom"])
def test_asymmetric_allocation(gpus, path, dtype):
    """set_radius(stencil.radius()) of the upwind stencil allocates no +x,
    -y or z halo; the general path is reached through x slabs narrower
    than 8 cells"""
    st = su.upwind()
    size = RN_SHAPES[0]
    dd, (h,) = su.make_domain(size, st.radius(), [dtype], "native", gpus)
    assert dd.backend.domains[0].raw_size().tuple()[0] == dd.local_rect(0)[1][0] - dd.local_rect(0)[0][0] + 2
    g = su.ripple_global(size, dtype)
    su.scatter(dd, h, g)
    dd.exchange()
    if path == "star":
        dd.apply_stencil(st, h)
    else:
        for li in range(dd.num_local()):
            lo, hi = dd.local_rect(li)
            for x0 in range(lo[0], hi[0], 7):
                dd.backend.stencil_apply(li, h.index, h.index, (x0, lo[1], lo[2]),
                                         (min(x0 + 7, hi[0]), hi[1], hi[2]), st, dtype)
    dd.backend.sync_compute()
    np.testing.assert_array_equal(su.gather(dd, h, from_next=True), su.exact_oracle(g, st))


@pytest.mark.parametrize("name", ["star1", "star3", "star4", "box3"])
def test_region_split_equals_all(name):
    """interior + exterior slabs (extent 1..R: the general path) == all"""
    st = {"star1": su.exact_star(1), "star3": su.exact_star(3), "star4": su.exact_star(4),
          "box3": su.exact_box3()}[name]
    size = RN_SHAPES[1]
    g = su.ripple_global(size, np.float32)
    outs = []
    for wheres in (("all",), ("interior", "exterior")):
        dd, (h,) = su.make_domain(size, st.radius(), [np.float32], "native", [0])
        su.scatter(dd, h, g)
        dd.exchange()
        for w in wheres:
            dd.apply_stencil(st, h, where=w)
        dd.backend.sync_compute()
        outs.append(su.gather(dd, h, from_next=True))
    np.testing.assert_array_equal(outs[0], outs[1])
    np.testing.assert_array_equal(outs[0], su.exact_oracle(g, st))


# ------------------------------------------------------- native against torch
STEPS = 3


def _gentle_star():
    """star of radius 2, weights +-1/4 and a 1/2 centre: sum |w| = 3.5, so
    after 3 steps of ripple data every partial sum is a multiple of 1/64
    below 753 * 3.5^3 * 64 < 2^24 -- still exact in fp32"""
    ws = [0.25, -0.25, 0.0, 0.25, -0.25]
    return Stencil.star([0.25, -0.25, 0.5, 0.25, -0.25], ws, ws)


def _run_steps(backend, size, st, dtype, g, boundary=None):
    dd, (h,) = su.make_domain(size, st.radius(), [dtype], backend, [0, 0], boundary=boundary)
    su.scatter(dd, h, g)
    for _ in range(STEPS):
        dd.step_stencil(st, h, overlap=True)
    return su.gather(dd, h)


@pytest.mark.parametrize("boundary", [None, "fixed"], ids=["periodic", "fixed"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_steps_match_torch_exact(dtype, boundary):
    st = _gentle_star()
    size = RN_SHAPES[1]
    bc = None if boundary is None else boundary_util.all_faces(Boundary.FIXED, 0.25)
    g = su.ripple_global(size, dtype)
    want = _run_steps("torch", size, st, dtype, g, bc)
    got = _run_steps("native", size, st, dtype, g, bc)
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("order", [2, 8])
def test_steps_match_torch_bounded(order, dtype):
    st = Stencil.identity() + 0.02 * Stencil.laplacian(order)
    size = RN_SHAPES[0]
    g = su.normal_global(size, dtype)
    want = _run_steps("torch", size, st, dtype, g)
    got = _run_steps("native", size, st, dtype, g)
    # 3x the one-step bound, on the torch result's magnitudes
    _, mag = su.roll_sum(want, st)
    su.assert_within_bound(got, want.astype(mag.dtype), 3 * su.bound_of(st, mag, dtype),
                           f"diffusion{order} x{STEPS}")


def test_diffusion3d_native_matches_torch():
    from stencil_amd.models.diffusion3d import Diffusion3D

    outs = []
    g = su.ripple_global(RN_SHAPES[0], np.float32)
    for backend in ("torch", "native"):
        # alpha_dt = 1/4 and order 2: dyadic weights, exact for one step
        app = Diffusion3D(RN_SHAPES[0], order=2, alpha_dt=0.25, backend=backend, gpus=[0, 0])
        app.realize()
        su.scatter(app.dd, app.h, g)
        app.step()
        outs.append(su.gather(app.dd, app.h))
    np.testing.assert_array_equal(outs[0], outs[1])
    np.testing.assert_array_equal(outs[1], su.exact_oracle(g, app.stencil))


# ---------------------------------------------------------------- validation
def test_validation_launches_nothing():
    size = RN_SHAPES[0]
    dd, (f, i32, d) = su.make_domain(size, _C.Radius.constant(1),
                                     [np.float32, np.int32, np.float64], "native", [0])
    flo, fhi, sent = _full_block(dd, SENTINEL, np.float32)
    dd.write_global(0, flo, sent, f, to_next=True)
    st = su.exact_star(1)
    with pytest.raises(ValueError):
        dd.apply_stencil(su.exact_star(2), f)  # a tap outside the allocated halo
    with pytest.raises(ValueError):
        dd.apply_stencil(st, i32)
    with pytest.raises(ValueError):
        dd.apply_stencil(st, f, d)
    lo, hi = dd.local_rect(0)
    rect = _C.Rect3(_C.Vec3(*lo), _C.Vec3(*hi))
    taps = _C.StencilTaps()
    taps.offsets = [_C.Vec3(0, 0, 0)] * 129
    taps.weights = [1.0] * 129
    with pytest.raises(ValueError):
        _C.stencil_apply(dd.backend.engine, 0, f.index, f.index, rect, taps, _C.StencilType.F32)
    taps.offsets, taps.weights = [], []
    with pytest.raises(ValueError):
        _C.stencil_apply(dd.backend.engine, 0, f.index, f.index, rect, taps, _C.StencilType.F32)
    # element size against the type, below the dtype check of apply_stencil
    one = st.to_native()
    with pytest.raises(ValueError):
        _C.stencil_apply(dd.backend.engine, 0, f.index, f.index, rect, one, _C.StencilType.F64)
    with pytest.raises(ValueError):
        _C.stencil_apply(dd.backend.engine, 0, f.index, d.index, rect, one, _C.StencilType.F32)
    # an empty region is a no-op
    empty = _C.Rect3(_C.Vec3(2, 2, 2), _C.Vec3(2, 5, 5))
    _C.stencil_apply(dd.backend.engine, 0, f.index, f.index, empty, one, _C.StencilType.F32)
    dd.backend.sync_compute()
    got = dd.read_global(0, flo, fhi, f, from_next=True)
    np.testing.assert_array_equal(got.view(np.uint8), sent.view(np.uint8))
