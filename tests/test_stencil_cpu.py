"""Generic stencil operator, CPU tier: the Stencil class (coefficients,
algebra, validation, derived radius) and the torch backend's
apply_stencil / step_stencil against the two oracles of stencil_util."""
import json
import math
import multiprocessing as mp
import os
import subprocess
import sys

import numpy as np
import pytest

import stencil_amd as sa
from stencil_amd import Boundary, Stencil, _C

import boundary_util
import stencil_util as su
from util import ripple_block

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE = (16, 12, 10)


# ---------------------------------------------------------------- Stencil
@pytest.mark.parametrize("order", [2, 4, 6, 8])
def test_laplacian_coefficients(order):
    h = (0.5, 1.25, 2.0)
    st = Stencil.laplacian(order, spacing=h)
    assert st.is_star and st.ntaps == 3 * order + 1
    taps = dict(zip(st.offsets, st.weights))
    centre = taps[(0, 0, 0)]
    for a in range(3):
        axis = {o[a]: w for o, w in taps.items() if o[a] != 0}
        assert sorted(axis) == [k for k in range(-order // 2, order // 2 + 1) if k]
        want = 2.0 / h[a] ** 2
        # this axis's share of the merged centre tap: -(sum of its side taps)
        s0 = math.fsum(axis.values())
        s1 = math.fsum(w * k for k, w in axis.items())
        s2 = math.fsum(w * k * k for k, w in axis.items())
        assert abs(s1) <= 1e-13 * want
        assert abs(s2 - want) <= 1e-13 * want
        centre += s0
    # sum of all weights is 0: what is left of the centre after every axis's share
    scale = sum(2.0 / x ** 2 for x in h)
    assert abs(centre) <= 1e-13 * scale
    assert abs(math.fsum(st.weights)) <= 1e-13 * scale


def test_laplacian_unit_spacing_order2():
    st = Stencil.laplacian(2)
    taps = dict(zip(st.offsets, st.weights))
    assert taps[(0, 0, 0)] == -6.0
    assert all(w == 1.0 for o, w in taps.items() if o != (0, 0, 0))
    assert st.ntaps == 7


def test_duplicates_merge_and_zeros_drop():
    st = Stencil([(1, 0, 0), (1, 0, 0), (0, 1, 0), (0, 1, 0), (0, 0, 0)], [0.5, 0.25, 1.0, -1.0, 2.0])
    assert dict(zip(st.offsets, st.weights)) == {(1, 0, 0): 0.75, (0, 0, 0): 2.0}
    assert st.ntaps == 2
    assert all(isinstance(w, float) for w in st.weights)


def test_algebra():
    lap = Stencil.laplacian(2)
    st = Stencil.identity() + 0.125 * lap
    taps = dict(zip(st.offsets, st.weights))
    assert taps[(0, 0, 0)] == 1.0 - 0.75
    assert taps[(-1, 0, 0)] == 0.125 and taps[(0, 0, 1)] == 0.125
    assert st.ntaps == 7 and st.is_star
    assert (lap * 2.0) == (2 * lap) == (lap + lap)
    # a centre that cancels disappears
    assert (Stencil.identity() + (1.0 / 6.0) * lap).ntaps == 6
    assert not su.exact_box3().is_star
    assert Stencil.star([1, 0, 2], [0], [3, 0, 0]).offsets == [(0, 0, -1), (-1, 0, 0), (1, 0, 0)]


def test_from_array_center():
    k = np.zeros((1, 2, 3))
    k[0, 1, 2] = 4.0
    k[0, 0, 0] = -1.0
    st = Stencil.from_array(k, (1, 0, 0))
    assert dict(zip(st.offsets, st.weights)) == {(1, 1, 0): 4.0, (-1, 0, 0): -1.0}


def test_constructor_errors():
    with pytest.raises(ValueError):
        Stencil([], [])
    with pytest.raises(ValueError):
        Stencil([(1, 0, 0), (1, 0, 0)], [1.0, -1.0])  # cancels to empty
    with pytest.raises(ValueError):
        Stencil([(0, 0, 0)], [float("nan")])
    with pytest.raises(ValueError):
        Stencil([(0, 0, 0)], [float("inf")])
    with pytest.raises(ValueError):
        Stencil([(9, 0, 0)], [1.0])
    with pytest.raises(ValueError):
        Stencil([(0, -9, 0)], [1.0])
    offs = [(x, y, 0) for x in range(-8, 9) for y in range(-4, 4)][:129]
    assert len(offs) == 129
    with pytest.raises(ValueError):
        Stencil(offs, [1.0] * 129)
    assert Stencil(offs[:128], [1.0] * 128).ntaps == 128
    assert Stencil([(8, -8, 8)], [1.0]).ntaps == 1
    with pytest.raises(ValueError):
        Stencil.laplacian(3)


def _dirs():
    import itertools

    return [d for d in itertools.product((-1, 0, 1), repeat=3) if d != (0, 0, 0)]


def test_radius_star():
    r = su.exact_star(3).radius()
    for d in _dirs():
        nz = sum(c != 0 for c in d)
        assert r.dir(*d) == (3 if nz == 1 else 0), d


def test_radius_box():
    assert su.exact_box3().radius() == _C.Radius.constant(1)


def test_radius_upwind():
    r = su.upwind().radius()
    assert (r.x(-1), r.x(1), r.y(-1), r.y(1), r.z(-1), r.z(1)) == (2, 0, 0, 1, 0, 0)
    assert r.dir(-1, 1, 0) == 0
    for d in _dirs():
        if sum(c != 0 for c in d) > 1:
            assert r.dir(*d) == 0, d


def test_radius_single_diagonal_tap():
    r = Stencil([(2, 1, 0)], [1.0]).radius()
    assert r.dir(1, 1, 0) == 2
    assert (r.x(1), r.y(1), r.x(-1), r.y(-1), r.z(1), r.z(-1)) == (2, 1, 0, 0, 0, 0)
    assert r.dir(-1, 1, 0) == 0 and r.dir(1, -1, 0) == 0 and r.dir(1, 1, 1) == 0


def test_star_radius_moves_fewer_bytes():
    totals = []
    for radius in (su.exact_star(2).radius(), _C.Radius.constant(2)):
        dd, _ = su.make_domain(SIZE, radius, [np.float32], "torch", [0, 0])
        totals.append(sum(dd.bytes_by_method.values()))
    assert 0 < totals[0] < totals[1]


# ------------------------------------------------- torch backend, oracle 1
_CASES = {
    "star1": su.exact_star(1),
    "star3": su.exact_star(3),
    "box3": su.exact_box3(),
    "asymbox": su.exact_asym_box(),
    "upwind": su.upwind(),
}


@pytest.mark.parametrize("gpus", [[0], [0, 0]], ids=["1dom", "2dom"])
@pytest.mark.parametrize("name", sorted(_CASES))
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_torch_apply_exact(name, dtype, gpus):
    """derived radius (for upwind: no +x, -y or z halo at all) is sufficient"""
    st = _CASES[name]
    dd, (h,) = su.make_domain(SIZE, st.radius(), [dtype], "torch", gpus)
    g = su.ripple_global(SIZE, dtype)
    su.scatter(dd, h, g)
    su.apply_once(dd, st, h)
    np.testing.assert_array_equal(su.gather(dd, h, from_next=True), su.exact_oracle(g, st))


@pytest.mark.parametrize("overlap", [True, False], ids=["overlap", "serial"])
@pytest.mark.parametrize("gpus", [[0], [0, 0]], ids=["1dom", "2dom"])
def test_torch_step_stencil_exact(gpus, overlap):
    st = su.exact_star(2)
    dd, (h,) = su.make_domain(SIZE, st.radius(), [np.float32], "torch", gpus)
    g = su.ripple_global(SIZE, np.float32)
    su.scatter(dd, h, g)
    dd.step_stencil(st, h, overlap=overlap)
    np.testing.assert_array_equal(su.gather(dd, h), su.exact_oracle(g, st))


def test_torch_region_split_equals_all():
    st = su.exact_box3()
    g = su.ripple_global(SIZE, np.float32)
    outs = []
    for wheres in (("all",), ("interior", "exterior")):
        dd, (h,) = su.make_domain(SIZE, st.radius(), [np.float32], "torch", [0, 0])
        su.scatter(dd, h, g)
        dd.exchange()
        for w in wheres:
            dd.apply_stencil(st, h, where=w)
        outs.append(su.gather(dd, h, from_next=True))
    np.testing.assert_array_equal(outs[0], outs[1])
    np.testing.assert_array_equal(outs[0], su.exact_oracle(g, st))


def test_torch_src_to_other_quantity():
    st = su.exact_star(1)
    dd, (a, b) = su.make_domain(SIZE, st.radius(), [np.float64, np.float64], "torch", [0, 0])
    g = su.ripple_global(SIZE, np.float64)
    su.scatter(dd, a, g)
    su.scatter(dd, b, np.full_like(g, -5.0), to_next=True)
    su.scatter(dd, a, np.full_like(g, -3.0), to_next=True)
    su.apply_once(dd, st, a, b)
    np.testing.assert_array_equal(su.gather(dd, b, from_next=True), su.exact_oracle(g, st))
    # the source quantity's next buffer is untouched
    assert (su.gather(dd, a, from_next=True) == -3.0).all()


def test_torch_explicit_box():
    st = su.upwind()
    dd, (h,) = su.make_domain(SIZE, _C.Radius.constant(2), [np.float32], "torch", [0])
    g = su.ripple_global(SIZE, np.float32)
    su.scatter(dd, h, g)
    su.scatter(dd, h, np.full_like(g, -9.0), to_next=True)
    dd.exchange()
    lo, hi = (3, 2, 1), (12, 9, 7)
    dd.apply_stencil(st, h, where=(lo, hi))
    got = su.gather(dd, h, from_next=True)
    want = np.full_like(g, -9.0)
    sl = (slice(lo[2], hi[2]), slice(lo[1], hi[1]), slice(lo[0], hi[0]))
    want[sl] = su.exact_oracle(g, st)[sl]
    np.testing.assert_array_equal(got, want)


# ------------------------------------------------- torch backend, oracle 2
@pytest.mark.parametrize("order", [4, 6, 8])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_torch_laplacian_bounded(order, dtype):
    st = Stencil.laplacian(order, spacing=(1.0, 0.7, 1.3))
    dd, (h,) = su.make_domain(SIZE, st.radius(), [dtype], "torch", [0, 0])
    g = su.normal_global(SIZE, dtype)
    su.scatter(dd, h, g)
    su.apply_once(dd, st, h)
    ref, mag = su.roll_sum(g, st)
    su.assert_within_bound(su.gather(dd, h, from_next=True), ref, su.bound_of(st, mag, dtype),
                           f"laplacian{order}")


# ------------------------------------------------------------- boundaries
@pytest.mark.parametrize(
    "kind,name",
    [(Boundary.FIXED, "star2"), (Boundary.MIRROR, "box3")],
    ids=["fixed-star", "mirror-box"],
)
def test_torch_boundary(kind, name):
    st = {"star2": su.exact_star(2), "box3": su.exact_box3()}[name]
    # FIXED value a multiple of 1/4 keeps the data exact
    kinds = boundary_util.all_faces(kind, boundary_util.FIXED_VALUE)
    radius = st.radius()
    dd, (h,) = su.make_domain(SIZE, radius, [np.float32], "torch", [0, 0], boundary=kinds)
    boundary_util.fill(dd, h)
    su.apply_once(dd, st, h)
    padded = boundary_util.padded_global(SIZE, radius, kinds, 1.0, np.float32)
    ref = su.correlate_padded(padded, radius, SIZE, st)
    want = ref.astype(np.float32)
    assert np.array_equal(want.astype(ref.dtype), ref)
    np.testing.assert_array_equal(su.gather(dd, h, from_next=True), want)


# -------------------------------------------------------------- validation
def test_torch_validation():
    dd, (f, i32, d) = su.make_domain(
        SIZE, _C.Radius.constant(1), [np.float32, np.int32, np.float64], "torch", [0]
    )
    st = su.exact_star(1)
    dd.apply_stencil(st, f)  # fine
    with pytest.raises(ValueError):
        dd.apply_stencil(st, i32)
    with pytest.raises(ValueError):
        dd.apply_stencil(st, f, d)
    with pytest.raises(ValueError):
        dd.apply_stencil(su.exact_star(2), f)  # reads beyond the radius-1 halo
    with pytest.raises(ValueError):
        dd.apply_stencil(st, f, where="nowhere")
    # an empty region is a no-op
    dd.apply_stencil(st, f, where=((2, 2, 2), (2, 5, 5)))


# ---------------------------------------------------------- two-rank gloo
def _gloo_worker(rank, world, port, q):
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        import torch.distributed as dist

        dist.init_process_group("gloo", rank=rank, world_size=world)
        sys.path.insert(0, os.path.dirname(__file__))
        import stencil_util as su2

        for st, overlap in ((su2.exact_star(2), True), (su2.exact_box3(), True),
                            (su2.upwind(), False)):
            dd = sa.DistributedDomain(*SIZE, backend="torch")
            dd.set_radius(st.radius())
            dd.set_gpus([0])
            h = dd.add_data(np.float32, "q")
            dd.realize()
            g = su2.ripple_global(SIZE, np.float32)
            su2.scatter(dd, h, g)
            dd.step_stencil(st, h, overlap=overlap)
            want = su2.exact_oracle(g, st)
            for li in range(dd.num_local()):
                lo, hi = dd.local_rect(li)
                got = dd.read_global(li, lo, hi, h)
                np.testing.assert_array_equal(
                    got, want[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]]
                )
        dist.destroy_process_group()
        q.put((rank, "ok"))
    except Exception:  # pragma: no cover
        import traceback

        q.put((rank, traceback.format_exc()))


def test_two_ranks_gloo_step_stencil():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_gloo_worker, args=(r, 2, 29641, q)) for r in range(2)]
    for p in procs:
        p.start()
    results = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=30)
        if p.is_alive():
            p.terminate()
    for rank, status in results:
        assert status == "ok", f"rank {rank}: {status}"


# ------------------------------------------------------------ app and CLI
def test_diffusion3d_torch_conserves_mean():
    from stencil_amd.models.diffusion3d import Diffusion3D

    app = Diffusion3D((12, 10, 8), order=4, dtype=np.float64, alpha_dt=0.05,
                      backend="torch", gpus=[0, 0])
    app.realize()
    g = su.normal_global((12, 10, 8), np.float64)
    su.scatter(app.dd, app.h, g)
    for _ in range(3):
        app.step()
    out = su.gather(app.dd, app.h)
    # the weights sum to 1 and the domain is periodic: the mean is kept
    assert abs(out.mean() - g.mean()) < 1e-13
    assert out.std() < g.std()  # and it diffuses


def test_stencil_apply_cli():
    out = subprocess.run(
        [sys.executable, os.path.join(REPO, "benchmarks", "stencil_apply.py"),
         "--backend", "torch", "--size", "12", "--steps", "2"],
        capture_output=True, text=True, timeout=300, cwd=REPO,
    )
    assert out.returncode == 0, out.stderr
    rec = json.loads(out.stdout.strip().splitlines()[-1])
    assert rec["ms_per_step"] > 0 and rec["gcells_per_s"] > 0
    assert rec["path"] == "star" and rec["ntaps"] == 7
