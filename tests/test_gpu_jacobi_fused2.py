"""Fused two-step replays of the wrap graph (csrc/src/jacobi.hip,
jacobi_kernel_fuse2): run(n >= 2) on a single fully periodic domain replays
n // 2 graphs that each hold the two-step kernel alone, then one single
step if n is odd.

Everything is bitwise against the NumPy oracle of jacobi_util.py: both
stages evaluate the same float32 expression as a single step, and the
division helper is correctly rounded for every input (test_gpu_div6.py).

The kernel's tile is 64 float4 vectors (256 cells) by 6 useful rows,
marching chunks of 64 planes (TILE_Y, ZC below); the shapes put an
extent just below, at and just above each of those edges.

The kernel takes its x neighbours from the neighbouring lanes of the wave and
everything from outside its tile from one gathered load per wave and plane.
The last four tests pin what that code can get wrong and the shapes above do
not: all kinds of tile edge in ONE launch, a row of exactly one full block
column, and hot / cold sphere cells at the row ends for the alignments that
need the x selects. STENCIL_JAC_FUSE2=0 in the environment runs those four on
single-step replays, which must give the same bits."""
import os

import numpy as np
import pytest

from stencil_amd import _C

import jacobi_util as ju
from util import full_region_of

pytestmark = pytest.mark.gpu

TILE_Y = 6   # useful rows of a block (8 rows, one redundant on each side)
ZC = 64      # planes per block (STENCIL_JAC_F2ZC default)

WRAP_SHAPES = [(8, 4, 3), (9, 5, 33), (10, 6, 65), (11, 7, 3), (8, 7, 33), (11, 4, 65), (24, 5, 33)]
# x: with radius 1 a row's first vector starts 3 cells before the first true
# cell, so a row of N cells is ceil((N + 3) / 4) vectors. 249 -> 63 vectors,
# 252 -> 64 (one full block column), 255 / 256 / 257 -> 65 (a second column
# of ONE lane, which is both a tile's first and the row's last lane).
X_EDGE = [(249, 4, 3), (252, 4, 3), (255, 4, 3), (256, 5, 3), (257, 4, 3)]
Y_EDGE = [(9, TILE_Y - 1, 3), (9, TILE_Y, 3), (10, TILE_Y + 1, 3), (11, 2 * TILE_Y + 1, 3)]
Z_EDGE = [(9, 5, ZC - 1), (10, 5, ZC), (11, 4, ZC + 1), (9, 4, 2 * ZC + 1)]
# sphere radius 4 (x = 40): hot/cold cells on every row and plane, across the
# y tile edges at rows 6, 12, 18 and on the rows and planes that wrap
SPHERE = [(40, 7, 9), (40, 25, 9)]
SHAPES = WRAP_SHAPES + X_EDGE + Y_EDGE + Z_EDGE + SPHERE
RADIUS_SHAPE = (19, 10, 9)

_G0, _WANT = {}, {}


def _g0(size):
    if size not in _G0:
        g = ju.random_field((size[2], size[1], size[0]),
                            seed=size[0] * 10007 + size[1] * 101 + size[2])
        g.setflags(write=False)
        _G0[size] = g
    return _G0[size]


def _want(size, steps):
    """the oracle after `steps` steps; computed once per size, incrementally"""
    have = max((s for (sz, s) in _WANT if sz == size and s <= steps), default=0)
    g = _WANT[(size, have)] if have else _g0(size)
    for s in range(have + 1, steps + 1):
        g = ju.jacobi_global(g, 1)
        g.setflags(write=False)
        _WANT[(size, s)] = g
    return _WANT[(size, steps)] if steps else g


def _app(monkeypatch, size, radius=1, fuse=None):
    from stencil_amd.models.jacobi3d import Jacobi3D

    monkeypatch.setenv("STENCIL_AMD_STEP_GRAPH", "1")
    monkeypatch.delenv("STENCIL_JAC_WRAP", raising=False)
    monkeypatch.delenv("STENCIL_JAC_F2ZC", raising=False)
    if fuse is None:
        monkeypatch.delenv("STENCIL_JAC_FUSE2", raising=False)
    else:
        monkeypatch.setenv("STENCIL_JAC_FUSE2", "1" if fuse else "0")
    app = Jacobi3D(size, backend="native", gpus=[0], radius=radius)
    app.realize()
    ju.scatter(app.dd, app.h, _g0(size))
    ju.scatter(app.dd, app.h, _g0(size), to_next=True)
    assert app._graph is not None
    return app


def _fill_halos(app, value):
    """`value` into every halo cell of both buffers, interiors kept"""
    dd, h = app.dd, app.h
    lo, hi = dd.local_rect(0)
    flo, fhi = full_region_of(dd, 0)
    shape = (fhi[2] - flo[2], fhi[1] - flo[1], fhi[0] - flo[0])
    for to_next in (False, True):
        inner = dd.read_global(0, lo, hi, h, from_next=to_next).copy()
        dd.write_global(0, flo, np.full(shape, value, dtype=np.float32), h, to_next=to_next)
        dd.write_global(0, lo, inner, h, to_next=to_next)


def _ids(v):
    return "x".join(map(str, v))


@pytest.mark.parametrize("size", SHAPES, ids=_ids)
def test_run_n_equals_the_oracle(size, monkeypatch):
    """run(n), n = 2..5: one and two fused replays, each with and without a
    trailing single step"""
    for n in (2, 3, 4, 5):
        app = _app(monkeypatch, size)
        fused = _C.jacobi_graph_is_fused2(app._graph)
        if size[0] >= 9:
            assert fused, f"{size}: declined"
        app.run(n)
        ju.assert_rects_equal(app.dd, app.h, _want(size, n),
                              f"{size} run({n}) {'fused' if fused else 'DECLINED'}")


@pytest.mark.parametrize("radius", [1, 2, 3, 4])
def test_every_row_alignment(radius, monkeypatch):
    """radius 1..4 gives under = 3, 2, 1, 0: every component that can take
    the wrapped x neighbour, at both stages"""
    size = RADIUS_SHAPE
    app = _app(monkeypatch, size, radius=radius)
    assert _C.jacobi_graph_is_fused2(app._graph)
    pad = app.dd.backend.domains[0].pad_bytes(app.h.index)
    assert ((pad + 4 * radius) % 16) // 4 == {1: 3, 2: 2, 3: 1, 4: 0}[radius]
    _fill_halos(app, np.nan)
    app.run(5)
    ju.assert_rects_equal(app.dd, app.h, _want(size, 5), f"radius {radius}")


@pytest.mark.parametrize("size", [(8, 4, 3), (24, 5, 33), (255, 4, 3), (11, 25, 3), (11, 4, 65)],
                         ids=_ids)
def test_never_reads_a_halo(size, monkeypatch):
    """NaN in every halo cell of both buffers: any halo read would surface"""
    app = _app(monkeypatch, size)
    assert _C.jacobi_graph_is_fused2(app._graph) or size[0] < 9
    _fill_halos(app, np.nan)
    app.run(4)
    ju.assert_rects_equal(app.dd, app.h, _want(size, 4), f"{size} NaN halos")


@pytest.mark.parametrize("size,radius", [((9, 5, 33), 1), ((10, 6, 3), 1), ((11, 13, 3), 1),
                                         ((255, 4, 3), 1), (RADIUS_SHAPE, 2), (RADIUS_SHAPE, 3)],
                         ids=lambda v: _ids(v) if isinstance(v, tuple) else f"r{v}")
def test_write_containment(size, radius, monkeypatch):
    """after run(4) (two fused replays, one into each buffer) every halo
    cell still holds the sentinel, except the same-row x-overshoot cells the
    row extension permits: `under` cells left and `over` cells right of the
    true row, in interior (y, z) rows only"""
    app = _app(monkeypatch, size, radius=radius)
    assert _C.jacobi_graph_is_fused2(app._graph)
    _fill_halos(app, ju.SENTINEL)
    app.run(4)
    dd, h = app.dd, app.h
    lo, hi = dd.local_rect(0)
    flo, fhi = full_region_of(dd, 0)
    pad = dd.backend.domains[0].pad_bytes(h.index)
    under = ((pad + 4 * radius) % 16) // 4
    over = (4 - ((size[0] + under) & 3)) & 3
    shape = (fhi[2] - flo[2], fhi[1] - flo[1], fhi[0] - flo[0])
    halo = np.ones(shape, dtype=bool)
    halo[lo[2] - flo[2]:hi[2] - flo[2], lo[1] - flo[1]:hi[1] - flo[1],
         lo[0] - flo[0]:hi[0] - flo[0]] = False
    allowed = np.zeros(shape, dtype=bool)
    zs, ys = slice(lo[2] - flo[2], hi[2] - flo[2]), slice(lo[1] - flo[1], hi[1] - flo[1])
    allowed[zs, ys, max(lo[0] - under - flo[0], 0):lo[0] - flo[0]] = True
    allowed[zs, ys, hi[0] - flo[0]:min(hi[0] + over, fhi[0]) - flo[0]] = True
    for from_next in (False, True):
        full = dd.read_global(0, flo, fhi, h, from_next=from_next)
        touched = halo & ~allowed & (ju.bits(full) != ju.bits(np.full(shape, ju.SENTINEL)))
        assert not touched.any(), (
            f"{size} r{radius} next={from_next}: {touched.sum()} halo cells written, first at "
            f"(z,y,x)={tuple(np.argwhere(touched)[0])}")
    ju.assert_rects_equal(dd, h, _want(size, 4), f"{size} r{radius}")


@pytest.mark.parametrize("size", [(10, 6, 33), (24, 5, 33)], ids=_ids)
def test_parity_bookkeeping(size, monkeypatch):
    """fused, single, fused + single: three, then four buffer flips; the
    exchange that follows goes through the device tables"""
    app = _app(monkeypatch, size)
    assert _C.jacobi_graph_is_fused2(app._graph)
    app.run(2)
    app.step()
    app.run(3)
    app.dd.exchange()
    want = _want(size, 6)
    ju.assert_rects_equal(app.dd, app.h, want, f"{size} 2+1+3")
    flo, fhi = full_region_of(app.dd, 0)
    full = app.dd.read_global(0, flo, fhi, app.h)
    r = app.dd.radius
    pads = ((r.z(-1), r.z(1)), (r.y(-1), r.y(1)), (r.x(-1), r.x(1)))
    ju.assert_bitwise(full, np.pad(want, pads, mode="wrap"), f"{size} halos after exchange")


def test_switch_off_gives_the_same_bits(monkeypatch):
    size = (10, 6, 33)
    app = _app(monkeypatch, size, fuse=False)
    assert _C.jacobi_graph_is_wrap(app._graph)
    assert not _C.jacobi_graph_is_fused2(app._graph)
    app.run(5)
    ju.assert_rects_equal(app.dd, app.h, _want(size, 5), "STENCIL_JAC_FUSE2=0")


# --------------------------------------------------------------------------
# lane shifts and the gathered load: tile edges
# --------------------------------------------------------------------------
FUSE = os.environ.get("STENCIL_JAC_FUSE2", "1")[:1] != "0"

# two block columns, the second one lane wide (65 vectors); three y tiles,
# the last one partial (13 = 6 + 6 + 1); two z chunks (66 = 64 + 2)
ALL_EDGES = (257, 13, 66)
# 252 cells at radius 1: 64 vectors, one full column. Lane 63 is the row's
# last lane and the edge cell right of the tile wraps to the row's first cell
ONE_COLUMN = (252, 7, 3)


def _edge_app(monkeypatch, size, radius=1):
    app = _app(monkeypatch, size, radius=radius, fuse=FUSE)
    assert _C.jacobi_graph_is_fused2(app._graph) == FUSE
    return app


@pytest.mark.parametrize("halo", ["clean", "nan"])
def test_every_kind_of_tile_edge_in_one_launch(halo, monkeypatch):
    app = _edge_app(monkeypatch, ALL_EDGES)
    if halo == "nan":
        _fill_halos(app, np.nan)
    app.run(4)
    ju.assert_rects_equal(app.dd, app.h, _want(ALL_EDGES, 4), f"{ALL_EDGES} halos {halo}")


def test_row_of_one_full_block_column(monkeypatch):
    app = _edge_app(monkeypatch, ONE_COLUMN)
    _fill_halos(app, np.nan)
    app.run(4)
    ju.assert_rects_equal(app.dd, app.h, _want(ONE_COLUMN, 4), f"{ONE_COLUMN}")


@pytest.mark.parametrize("radius", [2, 3])
@pytest.mark.parametrize("size", SPHERE, ids=_ids)
def test_sphere_cells_at_selected_row_ends(size, radius, monkeypatch):
    """radius 2 / 3: the first true cell is component 2 / 1 of the row's first
    vector. Sphere radius 4: the edge cells the gathered load serves lie inside
    the hot and cold spheres on some rows and planes."""
    app = _edge_app(monkeypatch, size, radius=radius)
    pad = app.dd.backend.domains[0].pad_bytes(app.h.index)
    assert ((pad + 4 * radius) % 16) // 4 == {2: 2, 3: 1}[radius]
    _fill_halos(app, np.nan)
    app.run(5)
    ju.assert_rects_equal(app.dd, app.h, _want(size, 5), f"{size} radius {radius}")


@pytest.mark.parametrize("size,radius", [(ALL_EDGES, 1), (ALL_EDGES, 2), (RADIUS_SHAPE, 2)],
                         ids=lambda v: _ids(v) if isinstance(v, tuple) else f"r{v}")
def test_write_containment_with_every_kind_of_tile_edge(size, radius, monkeypatch):
    """after run(4) every halo cell still holds the sentinel, except the
    same-row x-overshoot cells the row extension permits"""
    app = _edge_app(monkeypatch, size, radius=radius)
    _fill_halos(app, ju.SENTINEL)
    app.run(4)
    dd, h = app.dd, app.h
    lo, hi = dd.local_rect(0)
    flo, fhi = full_region_of(dd, 0)
    pad = dd.backend.domains[0].pad_bytes(h.index)
    under = ((pad + 4 * radius) % 16) // 4
    over = (4 - ((size[0] + under) & 3)) & 3
    shape = (fhi[2] - flo[2], fhi[1] - flo[1], fhi[0] - flo[0])
    zs, ys = slice(lo[2] - flo[2], hi[2] - flo[2]), slice(lo[1] - flo[1], hi[1] - flo[1])
    halo = np.ones(shape, dtype=bool)
    halo[zs, ys, lo[0] - flo[0]:hi[0] - flo[0]] = False
    allowed = np.zeros(shape, dtype=bool)
    allowed[zs, ys, max(lo[0] - under - flo[0], 0):lo[0] - flo[0]] = True
    allowed[zs, ys, hi[0] - flo[0]:min(hi[0] + over, fhi[0]) - flo[0]] = True
    sentinel = ju.bits(np.full(shape, ju.SENTINEL))
    for from_next in (False, True):
        full = dd.read_global(0, flo, fhi, h, from_next=from_next)
        touched = halo & ~allowed & (ju.bits(full) != sentinel)
        assert not touched.any(), (
            f"{size} r{radius} next={from_next}: {touched.sum()} halo cells written, first at "
            f"(z,y,x)={tuple(np.argwhere(touched)[0])}")
    ju.assert_rects_equal(dd, h, _want(size, 4), f"{size} r{radius}")
