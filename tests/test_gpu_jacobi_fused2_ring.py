"""jacobi_kernel_fuse2 (csrc/src/jacobi.hip) takes its x neighbours from the
neighbouring lanes of the wave and everything from outside its tile from one
gathered load per wave and plane. These shapes pin what that code can get
wrong and test_gpu_jacobi_fused2.py does not: all kinds of tile edge in ONE
launch, a row of exactly one full block column, and hot / cold sphere cells
at the row ends for the alignments that need the x selects.

Bitwise against the NumPy oracle, with the helpers of the existing file (the
oracle cache is shared). STENCIL_JAC_FUSE2=0 in the environment runs the same
cases on single-step replays, which must give the same bits.

The t planes are staged through registers, not through an LDS ring (measured,
see profiles/README.md), so there are no ring wrap-around cases."""
import os

import numpy as np
import pytest

from stencil_amd import _C

import jacobi_util as ju
import test_gpu_jacobi_fused2 as f2
from util import full_region_of

pytestmark = pytest.mark.gpu

FUSE = os.environ.get("STENCIL_JAC_FUSE2", "1")[:1] != "0"

# two block columns, the second one lane wide (65 vectors); three y tiles,
# the last one partial (13 = 6 + 6 + 1); two z chunks (66 = 64 + 2)
ALL_EDGES = (257, 13, 66)
# 252 cells at radius 1: 64 vectors, one full column. Lane 63 is the row's
# last lane and the edge cell right of the tile wraps to the row's first cell
ONE_COLUMN = (252, 7, 3)
SPHERE = [(40, 7, 9), (40, 25, 9)]


def _app(monkeypatch, size, radius=1):
    app = f2._app(monkeypatch, size, radius=radius, fuse=FUSE)
    assert _C.jacobi_graph_is_fused2(app._graph) == FUSE
    return app


@pytest.mark.parametrize("halo", ["clean", "nan"])
def test_every_kind_of_edge_in_one_launch(halo, monkeypatch):
    app = _app(monkeypatch, ALL_EDGES)
    if halo == "nan":
        f2._fill_halos(app, np.nan)
    app.run(4)
    ju.assert_rects_equal(app.dd, app.h, f2._want(ALL_EDGES, 4), f"{ALL_EDGES} halos {halo}")


def test_one_full_block_column(monkeypatch):
    app = _app(monkeypatch, ONE_COLUMN)
    f2._fill_halos(app, np.nan)
    app.run(4)
    ju.assert_rects_equal(app.dd, app.h, f2._want(ONE_COLUMN, 4), f"{ONE_COLUMN}")


@pytest.mark.parametrize("radius", [2, 3])
@pytest.mark.parametrize("size", SPHERE, ids=f2._ids)
def test_sphere_cells_at_selected_row_ends(size, radius, monkeypatch):
    """radius 2 / 3: the first true cell is component 2 / 1 of the row's first
    vector. Sphere radius 4: the edge cells the gathered load serves lie inside
    the hot and cold spheres on some rows and planes."""
    app = _app(monkeypatch, size, radius=radius)
    pad = app.dd.backend.domains[0].pad_bytes(app.h.index)
    assert ((pad + 4 * radius) % 16) // 4 == {2: 2, 3: 1}[radius]
    f2._fill_halos(app, np.nan)
    app.run(5)
    ju.assert_rects_equal(app.dd, app.h, f2._want(size, 5), f"{size} radius {radius}")


@pytest.mark.parametrize("size,radius", [(ALL_EDGES, 1), (ALL_EDGES, 2), (f2.RADIUS_SHAPE, 2)],
                         ids=lambda v: f2._ids(v) if isinstance(v, tuple) else f"r{v}")
def test_write_containment(size, radius, monkeypatch):
    """after run(4) every halo cell still holds the sentinel, except the
    same-row x-overshoot cells the row extension permits"""
    app = _app(monkeypatch, size, radius=radius)
    f2._fill_halos(app, ju.SENTINEL)
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
    ju.assert_rects_equal(dd, h, f2._want(size, 4), f"{size} r{radius}")
