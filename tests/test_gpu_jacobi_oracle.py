"""The Jacobi kernels (csrc/src/jacobi.hip: jacobi_kernel, jacobi_kernel_v4,
jacobi_kernel_v4_lds<ZC, WRAP>) against the NumPy oracle of jacobi_util.py,
bitwise, and where each launch path is allowed to write.

Kernel level: one launch through backend.jacobi_step per case. CURR holds
a seeded field over the whole full region (halos included: no exchange is
involved, the oracle's apron is simply what was written), NEXT a sentinel.
After the launch
- NEXT inside the region equals jacobi_cells bitwise,
- CURR is unchanged,
- extend_vec 0 and 2: every cell outside the region still holds the
  sentinel (mode 2 is what lets IPC peers write our halos during compute);
  extend_vec 1: cells outside the region differ from the sentinel only in
  the region's own (y, z) rows. Those rows consist of x-halo cells and
  cells of the local rect, which is all the free row extension may touch.

Application level: Jacobi3D over 3 steps (4 where buffer parity matters)
against jacobi_global, bitwise per local rect, one axis of variation at a
time against a base configuration plus the combinations the code singles
out.

jacobi_util.py explains why equality of bits is the right comparison;
test_jacobi_oracle_cpu.py checks the oracle itself without a GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

import stencil_amd as sa
from stencil_amd import Boundary, _C

import jacobi_util as ju
from util import full_region_of

pytestmark = pytest.mark.gpu

MODES = (0, 1, 2)


# --------------------------------------------------------------------------
# kernel level
# --------------------------------------------------------------------------
class _Dom:
    """one realized domain set, reused across regions; per local domain a
    seeded full-region field (never modified)"""

    def __init__(self, size, radius, n_domains):
        self.size = size
        dd = sa.DistributedDomain(*size, backend="native")
        dd.set_radius(radius)
        dd.set_gpus([0] * n_domains)
        self.h = dd.add_data(np.float32, "temp")
        dd.realize()
        assert dd.num_local() == n_domains
        self.dd = dd
        self.full, self.field, self.sent = [], [], []
        for li in range(n_domains):
            flo, fhi = full_region_of(dd, li)
            shape = (fhi[2] - flo[2], fhi[1] - flo[1], fhi[0] - flo[0])
            f = ju.random_field(shape, seed=100 + li)
            f.setflags(write=False)
            s = np.full(shape, ju.SENTINEL, dtype=np.float32)
            s.setflags(write=False)
            self.full.append((flo, fhi))
            self.field.append(f)
            self.sent.append(s)


_DOMS = {}


def _dom(size, radius=1, n_domains=1):
    key = (size, radius, n_domains)
    if key not in _DOMS:
        _DOMS[key] = _Dom(size, radius, n_domains)
    return _DOMS[key]


def _sl(lo, hi, flo):
    return tuple(slice(lo[a] - flo[a], hi[a] - flo[a]) for a in (2, 1, 0))


def _rect(lo, hi):
    return _C.Rect3(_C.Vec3(*lo), _C.Vec3(*hi))


def _kind(dom, li, lo, hi, mode):
    """the kernel jacobi_step picks for this launch (plans, launches nothing)"""
    return _C.jacobi_step_kernel(dom.dd.backend.engine, li, dom.h.index, _rect(lo, hi),
                                 _rect((0, 0, 0), dom.size), extend_vec=mode)


KINDS = set()  # the kernels of the launches _check_launch has checked in this process


def _check_launch(dom, li, lo, hi, mode):
    dd, h = dom.dd, dom.h
    KINDS.add(_kind(dom, li, lo, hi, mode))
    flo, fhi = dom.full[li]
    field, sent = dom.field[li], dom.sent[li]
    what = f"size {dom.size} r {dd.radius.x(1)} domain {li} region {lo}..{hi} extend_vec={mode}"
    dd.write_global(li, flo, field, h)
    dd.write_global(li, flo, sent, h, to_next=True)
    dd.backend.jacobi_step(li, h.index, lo, hi, (0, 0, 0), dom.size, extend_vec=mode)
    dd.backend.sync_compute()
    curr = dd.read_global(li, flo, fhi, h).copy()
    nxt = dd.read_global(li, flo, fhi, h, from_next=True).copy()

    box = _sl(lo, hi, flo)
    apron = _sl(tuple(c - 1 for c in lo), tuple(c + 1 for c in hi), flo)
    want = ju.jacobi_cells(np.ascontiguousarray(field[apron]), lo, hi, (0, 0, 0), dom.size)
    ju.assert_bitwise(nxt[box], want, what + ": NEXT inside the region")
    ju.assert_bitwise(curr, field, what + ": CURR changed")

    touched = ju.bits(nxt) != ju.bits(sent)
    touched[box] = False
    if mode == 1:
        rows = np.zeros(touched.shape, dtype=bool)
        rows[box[0], box[1], :] = True  # the region's own (y, z) rows, every x
        touched &= ~rows
    if touched.any():
        bad = np.argwhere(touched)
        z, y, x = bad[0]
        raise AssertionError(
            f"{what}: {len(bad)} cells outside the region were written; first at global "
            f"(x,y,z)=({x + flo[0]},{y + flo[1]},{z + flo[2]}) holding {nxt[z, y, x]!r}"
        )


def _regions(dom, li, family):
    dd = dom.dd
    lo, hi = dd.local_rect(li)
    if family == "whole":
        return [(lo, hi)]
    if family == "interior":
        return [dd.get_interior()[li]]
    if family == "exterior":
        return list(dd.get_exterior()[li])
    if family == "ysub":  # leaves rows on both sides
        return [((lo[0], lo[1] + 1, lo[2]), (hi[0], hi[1] - 1, hi[2]))]
    if family == "xsub":
        # extent 7: scalar kernel; 8+: jacobi_kernel_v4, every head/tail
        # combination (start address mod 16 B x extent mod 4)
        return [
            ((lo[0] + s, lo[1] + 1, lo[2] + 1), (lo[0] + s + e, lo[1] + 4, lo[2] + 3))
            for s in range(4)
            for e in (7, 8, 9, 10, 11, 13)
        ]
    if family == "xend":
        # boxes at and next to the row's +x end: where a row has no pitch
        # slack the right overshoot would land in the next row's cells
        return [
            ((hi[0] - k - e, lo[1] + 1, lo[2]), (hi[0] - k, hi[1] - 1, hi[2]))
            for k in (0, 1)
            for e in (8, 9, 10, 11)
        ]
    if family == "zchunks":  # chunks of 16 (v4) and 32 (LDS) planes
        return [
            ((lo[0], lo[1], lo[2] + a), (hi[0], hi[1], lo[2] + b))
            for a, b in ((0, 16), (0, 17), (0, 33), (15, 18))
        ]
    if family == "grown":  # the region of a halo_multiplier step
        return [(tuple(c - 1 for c in lo), tuple(c + 1 for c in hi))]
    if family == "spheres":
        # boxes that cut through the hot and the cold sphere, starting on
        # every x mod 4, with the scalar (7) and the vector (9) kernel
        cw = dom.size[0]
        cy, cz = dom.size[1] // 2, dom.size[2] // 2
        out = []
        for cx in (cw // 3, 2 * cw // 3):
            for s in range(4):
                for e in (7, 9):
                    out.append(((cx - s, cy - 1, lo[2]), (cx - s + e, cy + 2, hi[2])))
        return out
    raise AssertionError(family)


BASE = ("whole", "interior", "exterior", "ysub")

KERNEL_CASES = [
    ((19, 10, 9), 1, 1, BASE + ("xsub",)),
    ((19, 10, 9), 2, 1, BASE + ("xsub", "grown")),
    ((11, 7, 33), 1, 1, BASE + ("zchunks",)),
    ((261, 5, 3), 1, 1, BASE),  # more than 64 vector lanes per row
    ((62, 5, 3), 1, 1, BASE + ("xend",)),  # rows without pitch slack
    ((60, 5, 3), 2, 1, BASE + ("xend", "grown")),  # the same at radius 2
    ((30, 9, 7), 1, 1, BASE + ("spheres",)),  # sphere radius 3
    ((8, 4, 3), 1, 1, BASE),  # sphere radius 0: the centre cells alone
    ((19, 10, 9), 1, 2, BASE),
]


def _kernel_params():
    for size, radius, n, families in KERNEL_CASES:
        for fam in families:
            name = "x".join(map(str, size)) + f"-r{radius}-{n}dom-{fam}"
            yield pytest.param(size, radius, n, fam, id=name)


@pytest.mark.parametrize("size,radius,n_domains,family", list(_kernel_params()))
def test_kernel_bits_and_containment(size, radius, n_domains, family):
    dom = _dom(size, radius, n_domains)
    n = 0
    for li in range(n_domains):
        for lo, hi in _regions(dom, li, family):
            for mode in MODES:
                _check_launch(dom, li, lo, hi, mode)
                n += 1
    assert n >= 3 * n_domains


def test_kernel_cases_reach_every_kernel():
    """the launches of KERNEL_CASES, planned again without launching: every
    kernel a default process can pick is among them, and nothing
    _check_launch has met so far is missing from the plan. (Planned again
    rather than read from KINDS alone, so that the answer does not depend on
    which tests ran before this one; the planner is the one jacobi_step
    launches from.)"""
    kinds = set()
    for size, radius, n_domains, families in KERNEL_CASES:
        dom = _dom(size, radius, n_domains)
        for li in range(n_domains):
            for fam in families:
                for lo, hi in _regions(dom, li, fam):
                    kinds.update(_kind(dom, li, lo, hi, mode) for mode in MODES)
    assert kinds >= {"scalar", "vec4", "lds"}
    assert KINDS <= kinds


def test_zero_slack_rows_really_have_none():
    """(62,5,3) at radius 1 and (60,5,3) at radius 2 are 64 cells per row:
    exactly one 256 B pitch"""
    for size, radius in (((62, 5, 3), 1), ((60, 5, 3), 2)):
        dom = _dom(size, radius, 1)
        d = dom.dd.backend.domains[0]
        assert d.curr_pitch(dom.h.index) == (size[0] + 2 * radius) * 4 == 256


_CHILD = """
import sys
import test_gpu_jacobi_oracle as t
n = 0
for size, radius in (((19, 10, 9), 1), ((62, 5, 3), 1)):
    dom = t._dom(size, radius, 1)
    for fam in ("whole", "interior"):
        for lo, hi in t._regions(dom, 0, fam):
            for mode in t.MODES:
                t._check_launch(dom, 0, lo, hi, mode)
                n += 1
print("lds-off cases ok:", n)
print("lds-off kinds:", sorted(t.KINDS))
"""


def test_kernel_bits_with_the_lds_kernel_off():
    """STENCIL_JAC_LDS=0 (read once per process, hence a fresh child):
    pure-vector launches go to jacobi_kernel_v4's vecAll branch"""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ)
    env["STENCIL_JAC_LDS"] = "0"
    env["PYTHONPATH"] = os.pathsep.join(
        [os.path.dirname(here), here] + [p for p in env.get("PYTHONPATH", "").split(os.pathsep) if p]
    )
    res = subprocess.run([sys.executable, "-c", _CHILD], env=env, cwd=here, capture_output=True,
                         text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "lds-off cases ok: 12" in res.stdout, res.stdout + res.stderr
    kinds = res.stdout.split("lds-off kinds:")[1].splitlines()[0]
    assert "'vec4-all'" in kinds and "'lds'" not in kinds, res.stdout


def test_validation_launches_nothing():
    dom = _dom((19, 10, 9), 1, 1)
    dd, h = dom.dd, dom.h
    flo, fhi = dom.full[0]
    lo, hi = dd.local_rect(0)
    sent = dom.sent[0]
    for to_next in (False, True):
        dd.write_global(0, flo, sent, h, to_next=to_next)
    b = dd.backend
    size = dom.size
    bad_regions = [
        (flo, fhi),  # the full region: its apron is outside
        ((lo[0] - 1, lo[1], lo[2]), hi),  # apron one cell past -x
        (lo, (hi[0] + 1, hi[1], hi[2])),
        ((lo[0], lo[1] - 1, lo[2]), hi),
        (lo, (hi[0], hi[1] + 1, hi[2])),
        ((lo[0], lo[1], lo[2] - 1), hi),
        (lo, (hi[0], hi[1], hi[2] + 1)),
        ((lo[0] + 100, lo[1], lo[2]), (hi[0] + 100, hi[1], hi[2])),
    ]
    graphs_before = _C.step_graphs_alive()
    for rlo, rhi in bad_regions:
        for mode in MODES:
            with pytest.raises(ValueError):
                b.jacobi_step(0, h.index, rlo, rhi, (0, 0, 0), size, extend_vec=mode)
        with pytest.raises(ValueError):
            b.jacobi_graph_create(0, h.index, rlo, rhi, (0, 0, 0), size)
    with pytest.raises(ValueError):
        b.jacobi_step(0, h.index, lo, hi, (0, 0, 0), size, extend_vec=3)
    with pytest.raises(ValueError):
        b.jacobi_step(0, 5, lo, hi, (0, 0, 0), size)
    with pytest.raises(ValueError):
        b.jacobi_step(1, h.index, lo, hi, (0, 0, 0), size)
    rect = lambda a, c: _C.Rect3(_C.Vec3(*a), _C.Vec3(*c))  # noqa: E731
    with pytest.raises(ValueError):
        _C.jacobi_mr_graph_create(b.engine, 0, h.index, rect(lo, hi), rect((0, 0, 0), size),
                                  [rect(flo, fhi)], extend_vec=2)
    with pytest.raises(ValueError):
        _C.jacobi_mr_graph_create(b.engine, 0, h.index, rect(flo, fhi), rect((0, 0, 0), size),
                                  [], extend_vec=2)
    # a refused creation leaves no graph object behind
    assert _C.step_graphs_alive() == graphs_before
    # fill_f32: the region itself must be inside the full region
    for next_buf in (False, True):
        for rlo, rhi in (
            ((flo[0] - 1, flo[1], flo[2]), fhi),
            (flo, (fhi[0], fhi[1] + 1, fhi[2])),
            (flo, (fhi[0], fhi[1], fhi[2] + 1)),
        ):
            with pytest.raises(ValueError):
                b.fill_f32(0, h.index, rlo, rhi, 3.0, next_buf)
        with pytest.raises(ValueError):
            b.fill_f32(0, 5, lo, hi, 3.0, next_buf)
    # an empty region is a no-op
    b.jacobi_step(0, h.index, (2, 2, 2), (2, 5, 5), (0, 0, 0), size)
    b.fill_f32(0, h.index, (2, 2, 2), (2, 5, 5), 3.0, True)
    b.sync_compute()
    for from_next in (False, True):
        got = dd.read_global(0, flo, fhi, h, from_next=from_next)
        np.testing.assert_array_equal(got.view(np.uint8), sent.view(np.uint8))
    # what is valid still works: the full region may be filled
    b.fill_f32(0, h.index, flo, fhi, 3.0, True)
    b.sync_compute()
    assert (dd.read_global(0, flo, fhi, h, from_next=True) == 3.0).all()


# --------------------------------------------------------------------------
# application level
# --------------------------------------------------------------------------
# SHAPES / RADIUS_SHAPE of test_gpu_jacobi_wrap.py (over = 0..3, extY % 4,
# z wraps in a second chunk, a sphere on wrapped rows; radius 1..4 gives
# under = 3..0)
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
RADIUS_SHAPE = (19, 10, 9)
EXTRA_SHAPES = [(62, 5, 3), (30, 9, 7), (261, 5, 3)]

FIXED = {f: (Boundary.FIXED, 0.25) for f in ("x-", "x+", "y-", "y+", "z-", "z+")}
MIRROR = {f: (Boundary.MIRROR, 0) for f in ("x-", "x+", "y-", "y+", "z-", "z+")}
WALLS = {"fixed": FIXED, "mirror": MIRROR}

_G0, _WANT = {}, {}


def _g0(size):
    if size not in _G0:
        g = ju.random_field((size[2], size[1], size[0]), seed=size[0] * 10007 + size[1] * 101 + size[2])
        g.setflags(write=False)
        _G0[size] = g
    return _G0[size]


def _want(size, steps, walls=None):
    """the oracle's global array, computed once per configuration"""
    key = (size, steps, walls)
    if key not in _WANT:
        pad = ju.wrap_pad if walls is None else ju.walls_pad(WALLS[walls])
        w = ju.jacobi_global(_g0(size), steps, pad)
        w.setflags(write=False)
        _WANT[key] = w
    return _WANT[key]


def _app(monkeypatch, size, graph, n_domains=1, radius=1, wrap=None, walls=None, m=1):
    from stencil_amd.models.jacobi3d import Jacobi3D

    monkeypatch.setenv("STENCIL_AMD_STEP_GRAPH", "1" if graph else "0")
    if wrap is None:
        monkeypatch.delenv("STENCIL_JAC_WRAP", raising=False)
    else:
        monkeypatch.setenv("STENCIL_JAC_WRAP", "1" if wrap else "0")
    app = Jacobi3D(size, backend="native", gpus=[0] * n_domains, radius=radius,
                   halo_multiplier=m, boundary=None if walls is None else WALLS[walls])
    app.realize()
    assert app.dd.num_local() == n_domains
    ju.scatter(app.dd, app.h, _g0(size))  # realize() filled 0.5: the field goes in afterwards
    assert (app._graph is not None) == (graph and n_domains == 1 and m == 1)
    return app


def _steps(app, n, overlap=True):
    for _ in range(n):
        app.step(overlap=overlap)


def _ids(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else None


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("size", SHAPES + EXTRA_SHAPES, ids=_ids)
def test_app_single_domain(size, graph, monkeypatch):
    app = _app(monkeypatch, size, graph)
    _steps(app, 3)
    ju.assert_rects_equal(app.dd, app.h, _want(size, 3), f"{size} graph={graph}")


def test_wrap_graph_needs_rows_it_may_extend(monkeypatch):
    """(19,10,9): 21 cells of a 64-cell pitch, the extension lands in halo
    cells and slack: wrap graph. (62,5,3): no slack, the extension would
    land in the neighbouring rows' cells: translate graph."""
    app = _app(monkeypatch, RADIUS_SHAPE, graph=True)
    assert _C.jacobi_graph_is_wrap(app._graph)
    app = _app(monkeypatch, (62, 5, 3), graph=True)
    assert not _C.jacobi_graph_is_wrap(app._graph)


@pytest.mark.parametrize("path", ["wrap", "translate", "overlap", "serial"])
@pytest.mark.parametrize("radius", [1, 2, 3, 4])
def test_app_radius(radius, path, monkeypatch):
    """radius 1..4: under = 3..0 of the wrap kernel's x select; 4 steps so
    that both buffer parities are replayed twice"""
    size = RADIUS_SHAPE
    graph = path in ("wrap", "translate")
    app = _app(monkeypatch, size, graph, radius=radius, wrap=(path == "wrap") if graph else None)
    if graph:
        assert _C.jacobi_graph_is_wrap(app._graph) == (path == "wrap")
    _steps(app, 4, overlap=path != "serial")
    ju.assert_rects_equal(app.dd, app.h, _want(size, 4), f"radius {radius} {path}")


@pytest.mark.parametrize("overlap", [True, False], ids=["overlap", "serial"])
@pytest.mark.parametrize("n_domains", [1, 2, 8])
def test_app_domains(n_domains, overlap, monkeypatch):
    size = RADIUS_SHAPE
    app = _app(monkeypatch, size, graph=False, n_domains=n_domains)
    _steps(app, 3, overlap=overlap)
    ju.assert_rects_equal(app.dd, app.h, _want(size, 3), f"{n_domains} domains")


@pytest.mark.parametrize("size", [RADIUS_SHAPE, (30, 9, 7)], ids=_ids)
@pytest.mark.parametrize("radius", [3, 4])
def test_app_wide_x_slabs_two_domains_overlap(radius, size, monkeypatch):
    """radius >= 3 with overlap: the +-x exterior slabs are `radius` wide
    and must still run behind the interior kernel, whose row extension
    reaches into them. (The ordering itself cannot be shown to matter at
    this size: the interior kernel finishes first either way.)"""
    app = _app(monkeypatch, size, graph=False, n_domains=2, radius=radius)
    _steps(app, 4, overlap=True)
    ju.assert_rects_equal(app.dd, app.h, _want(size, 4), f"radius {radius} 2 domains")


@pytest.mark.parametrize("n_domains,graph", [(1, True), (1, False), (2, False)],
                         ids=["1dom-graph", "1dom-eager", "2dom-eager"])
@pytest.mark.parametrize("walls", ["fixed", "mirror"])
def test_app_walls(walls, n_domains, graph, monkeypatch):
    size = RADIUS_SHAPE
    app = _app(monkeypatch, size, graph, n_domains=n_domains, walls=walls)
    if graph:
        assert not _C.jacobi_graph_is_wrap(app._graph)
    _steps(app, 3)
    ju.assert_rects_equal(app.dd, app.h, _want(size, 3, walls), f"walls {walls}")


@pytest.mark.parametrize("radius", [1, 2])
def test_app_halo_multiplier(radius, monkeypatch):
    size = RADIUS_SHAPE
    app = _app(monkeypatch, size, graph=False, n_domains=2, radius=radius, m=2)
    _steps(app, 4)  # two whole exchange periods
    ju.assert_rects_equal(app.dd, app.h, _want(size, 4), f"halo_multiplier 2 radius {radius}")


@pytest.mark.parametrize("size", [RADIUS_SHAPE, (62, 5, 3)], ids=_ids)
def test_app_run_then_exchange(size, monkeypatch):
    """run(3), then exchange(): the full region, halos included, is the
    oracle's array wrapped"""
    app = _app(monkeypatch, size, graph=True)
    app.run(3)
    app.dd.exchange()
    want = _want(size, 3)
    ju.assert_rects_equal(app.dd, app.h, want, "run(3)")
    flo, fhi = full_region_of(app.dd, 0)
    full = app.dd.read_global(0, flo, fhi, app.h)
    ju.assert_bitwise(full, np.pad(want, 1, mode="wrap"), "full region after exchange")
