"""Wrap-reading whole-step graph of the single-domain fully periodic Jacobi
run (csrc/src/jacobi.hip, jacobi_kernel_v4_lds<ZC, true>): the stencil
kernel reads periodic neighbours from the far side of the same buffer, no
translate fills a halo and the table swap is hoisted out of the graph.

Every comparison is bitwise against the eager path
(STENCIL_AMD_STEP_GRAPH=0): the same expression runs on the same values,
so no tolerance applies."""
import numpy as np
import pytest

from stencil_amd import Boundary, _C

from util import fill_interiors, full_region_of

pytestmark = pytest.mark.gpu

STEPS = 3

# x 8..11 covers over = 0..3 of the row extension (radius 1: under = 3, so
# extX + 3 + over is a multiple of 4); y 4..7 covers every extY % 4, with
# blocks whose last rows are clamped lanes; z 33 / 65 put the z wrap in a
# block with lz0 != 0 (ZC = 32). x = 24 has cw / 10 = 2: sphere cells that
# must still be overridden on wrapped rows.
SHAPES = [
    (8, 4, 3),
    (9, 5, 33),
    (10, 6, 65),
    (11, 7, 3),
    (8, 7, 33),
    (11, 4, 65),
    (9, 6, 3),
    (24, 5, 33),
]
RADIUS_SHAPE = (19, 10, 9)  # x >= 16; every extent > 2 * radius up to radius 4


def _make(monkeypatch, size, graph, radius=1, boundary=None, wrap=None):
    from stencil_amd.models.jacobi3d import Jacobi3D

    monkeypatch.setenv("STENCIL_AMD_STEP_GRAPH", "1" if graph else "0")
    if wrap is None:
        monkeypatch.delenv("STENCIL_JAC_WRAP", raising=False)
    else:
        monkeypatch.setenv("STENCIL_JAC_WRAP", "1" if wrap else "0")
    app = Jacobi3D(size, backend="native", gpus=[0], radius=radius, boundary=boundary)
    app.realize()
    fill_interiors(app.dd, app.h)
    assert (app._graph is not None) == graph
    return app


def _interior(app):
    lo, hi = app.dd.local_rect(0)
    return app.dd.read_global(0, lo, hi, app.h).copy()


_EAGER = {}


def _eager(monkeypatch, size, radius=1, boundary_key=None, boundary=None):
    """interior after STEPS eager steps from a clean domain, computed once
    per configuration and shared (never modified)"""
    key = (size, radius, boundary_key)
    if key not in _EAGER:
        app = _make(monkeypatch, size, graph=False, radius=radius, boundary=boundary)
        for _ in range(STEPS):
            app.step()
        out = _interior(app)
        assert np.isfinite(out).all()
        out.setflags(write=False)
        _EAGER[key] = out
    return _EAGER[key]


def _poison_halos(app):
    """NaN into every halo cell of both buffers, interiors kept"""
    dd, h = app.dd, app.h
    lo, hi = dd.local_rect(0)
    flo, fhi = full_region_of(dd, 0)
    shape = (fhi[2] - flo[2], fhi[1] - flo[1], fhi[0] - flo[0])
    for to_next in (False, True):
        inner = dd.read_global(0, lo, hi, h, from_next=to_next).copy()
        dd.write_global(0, flo, np.full(shape, np.nan, dtype=np.float32), h, to_next=to_next)
        dd.write_global(0, lo, inner, h, to_next=to_next)


@pytest.mark.parametrize("size", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_wrap_graph_never_reads_a_halo(size, monkeypatch):
    """3 steps with every halo cell NaN match eager steps on a clean
    domain: any halo read would surface as NaN"""
    want = _eager(monkeypatch, size)
    app = _make(monkeypatch, size, graph=True)
    assert _C.jacobi_graph_is_wrap(app._graph), "wrap graph did not activate"
    _poison_halos(app)
    for _ in range(STEPS):
        app.step()
    np.testing.assert_array_equal(_interior(app), want)


@pytest.mark.parametrize("radius", [1, 2, 3, 4])
def test_wrap_graph_every_row_alignment(radius, monkeypatch):
    """radius 1..4 gives under = 3, 2, 1, 0: both the `left`-scalar case
    (under == 0) and the cc-component cases of the x wrap"""
    size = RADIUS_SHAPE
    want = _eager(monkeypatch, size, radius=radius)
    app = _make(monkeypatch, size, graph=True, radius=radius)
    assert _C.jacobi_graph_is_wrap(app._graph)
    # under = (address of the first interior cell of a row) % 16 / 4.
    # Buffers start pad_bytes past a hipMalloc base (256 B aligned) and the
    # first interior cell sits `radius` cells into the row.
    pad = app.dd.backend.domains[0].pad_bytes(app.h.index)
    assert ((pad + 4 * radius) % 16) // 4 == {1: 3, 2: 2, 3: 1, 4: 0}[radius]
    _poison_halos(app)
    for _ in range(STEPS):
        app.step()
    np.testing.assert_array_equal(_interior(app), want)


@pytest.mark.parametrize("size", [(10, 6, 33), (24, 5, 33)], ids=lambda s: "x".join(map(str, s)))
def test_odd_run_then_exchange(size, monkeypatch):
    """run(3) leaves one hoisted table swap behind the replays: the
    exchange that follows goes through the device tables and must fill the
    halos of the buffer the host calls current"""
    want = _eager(monkeypatch, size)
    app = _make(monkeypatch, size, graph=True)
    assert _C.jacobi_graph_is_wrap(app._graph)
    app.run(STEPS)
    app.dd.exchange()
    np.testing.assert_array_equal(_interior(app), want)
    flo, fhi = full_region_of(app.dd, 0)
    full = app.dd.read_global(0, flo, fhi, app.h)
    r = app.dd.radius
    pads = ((r.z(-1), r.z(1)), (r.y(-1), r.y(1)), (r.x(-1), r.x(1)))
    np.testing.assert_array_equal(full, np.pad(want, pads, mode="wrap"))


def test_even_run_then_single_step(monkeypatch):
    size = (11, 7, 33)
    want = _eager(monkeypatch, size)
    app = _make(monkeypatch, size, graph=True)
    assert _C.jacobi_graph_is_wrap(app._graph)
    app.run(2)
    app.step()
    np.testing.assert_array_equal(_interior(app), want)


def test_wrap_switch_off_gives_the_same_bits(monkeypatch):
    size = (10, 6, 33)
    want = _eager(monkeypatch, size)
    app = _make(monkeypatch, size, graph=True, wrap=False)
    assert not _C.jacobi_graph_is_wrap(app._graph)
    app.run(STEPS)
    np.testing.assert_array_equal(_interior(app), want)


def test_fixed_wall_keeps_the_translate_graph(monkeypatch):
    """a FIXED wall on z (x, y periodic) still runs the whole-step graph,
    but the one with translates and boundary fill, and matches eager"""
    size = (10, 6, 33)
    bc = {"z": (Boundary.FIXED, 0.25)}
    want = _eager(monkeypatch, size, boundary_key="z-fixed", boundary=bc)
    app = _make(monkeypatch, size, graph=True, boundary=bc)
    assert not _C.jacobi_graph_is_wrap(app._graph)
    for _ in range(STEPS):
        app.step()
    np.testing.assert_array_equal(_interior(app), want)
