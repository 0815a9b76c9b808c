"""Ownership of the whole-step replay graphs (ReplayGraph in
csrc/include/stencil_amd/step_graph.hpp): the object a *_graph_create
returns owns its streams, events and graph execs, keeps its engine alive,
and frees everything when the last reference goes.
_C.step_graphs_alive() counts the live objects.

Shapes are the smallest at which the other tests get each graph kind to
activate: (8, 4, 3) for the Jacobi wrap graph (test_gpu_jacobi_wrap.py),
(19, 10, 9) with STENCIL_JAC_WRAP=0 for the translate graph
(test_gpu_jacobi_oracle.py) and 16^3 for MHD (test_gpu_mhd.py)."""
import gc
import weakref

import numpy as np
import pytest

from stencil_amd import _C
from stencil_amd.models import mhd_ref as M
from stencil_amd.models.astaroth import FIELDS, Astaroth
from stencil_amd.models.jacobi3d import Jacobi3D

import jacobi_util as ju
from test_gpu_mhd import global_init

pytestmark = pytest.mark.gpu

STEPS = 3
KINDS = ["wrap", "translate", "mhd"]
SIZES = {"wrap": (8, 4, 3), "translate": (19, 10, 9), "mhd": (16, 16, 16)}

_G0 = {}


def _g0(size):
    if size not in _G0:
        g = ju.random_field((size[2], size[1], size[0]), seed=sum(size))
        g.setflags(write=False)
        _G0[size] = g
    return _G0[size]


def _build(kind, monkeypatch):
    """a realized, initialised app of `kind` whose graph activated"""
    size = SIZES[kind]
    monkeypatch.setenv("STENCIL_AMD_STEP_GRAPH", "1")
    if kind == "mhd":
        app = Astaroth(size, backend="native", gpus=[0])
        app.realize()
        app.init_fields()
        assert app._graph is not None, "mhd graph did not activate"
        return app
    if kind == "wrap":
        monkeypatch.delenv("STENCIL_JAC_WRAP", raising=False)
    else:
        monkeypatch.setenv("STENCIL_JAC_WRAP", "0")
    app = Jacobi3D(size, backend="native", gpus=[0])
    app.realize()
    ju.scatter(app.dd, app.h, _g0(size))
    assert app._graph is not None, "jacobi graph did not activate"
    assert _C.jacobi_graph_is_wrap(app._graph) == (kind == "wrap")
    return app


def _steps(kind, app):
    for _ in range(STEPS):
        if kind == "mhd":
            app.step(overlap=False)  # conf dt, no overlap: the graph path
        else:
            app.step()


def _field(kind, app):
    if kind == "mhd":
        return np.stack([app.read_field(0, n) for n in FIELDS])
    lo, hi = app.dd.local_rect(0)
    return app.dd.read_global(0, lo, hi, app.h).copy()


_WANT = {}


def _want(kind, app):
    """what the oracle of that shape gives after STEPS steps, computed once"""
    if kind not in _WANT:
        size = SIZES[kind]
        if kind == "mhd":
            cf = {k: float(app.conf[k])
                  for k in ("dsx", "dsy", "dsz", "cs2", "cp_inv", "nu", "eta", "chi")}
            curr = global_init(size)
            nxt = [np.zeros(curr[0].shape) for _ in range(8)]
            for _ in range(STEPS):
                for s in range(3):
                    curr, nxt = M.substep(curr, nxt, s, float(app.conf["dt"]), cf)
            w = np.stack(curr)
        else:
            w = ju.jacobi_global(_g0(size), STEPS)
        w.setflags(write=False)
        _WANT[kind] = w
    return _WANT[kind]


@pytest.mark.parametrize("kind", KINDS)
def test_counter_returns(kind, monkeypatch):
    gc.collect()
    base = _C.step_graphs_alive()
    app = _build(kind, monkeypatch)
    assert _C.step_graphs_alive() == base + 1
    _steps(kind, app)
    del app
    gc.collect()
    assert _C.step_graphs_alive() == base


@pytest.mark.parametrize("kind", KINDS)
def test_rebuild_in_one_process(kind, monkeypatch):
    """a second app built after the first was collected computes the same
    bits: nothing of the first one's graph is left to interfere"""
    gc.collect()
    base = _C.step_graphs_alive()
    fields = []
    for _ in range(2):
        app = _build(kind, monkeypatch)
        _steps(kind, app)
        fields.append(_field(kind, app))
        want = _want(kind, app)
        del app
        gc.collect()
        assert _C.step_graphs_alive() == base
    np.testing.assert_array_equal(fields[0], fields[1])
    if kind == "mhd":  # tolerances of test_gpu_mhd.py
        np.testing.assert_allclose(fields[0], want, rtol=1e-9, atol=1e-12)
    else:
        ju.assert_bitwise(fields[0], want, f"{kind} graph after {STEPS} steps")


@pytest.mark.parametrize("kind", KINDS)
def test_live_graph_keeps_its_engine_alive(kind, monkeypatch):
    """ownership only: nothing is launched after the app is gone"""
    gc.collect()
    base = _C.step_graphs_alive()
    app = _build(kind, monkeypatch)
    engine = weakref.ref(app.dd.backend.engine)
    g = app._graph
    del app
    gc.collect()
    assert engine() is not None, "the engine died under a live graph"
    assert _C.step_graphs_alive() == base + 1
    del g
    gc.collect()
    assert engine() is None
    assert _C.step_graphs_alive() == base
