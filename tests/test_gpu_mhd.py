"""MHD solver numerics on GPU: the HIP kernel + distributed exchange must
match the NumPy global-periodic reference over full RK3 iterations."""
import numpy as np
import pytest

from stencil_amd.models import mhd_ref as M
from stencil_amd.models.astaroth import Astaroth, FIELDS, harmonic_np, init_modes

pytestmark = pytest.mark.gpu


def global_init(size):
    out = []
    for base, amp, m, phase in init_modes(size):
        out.append(harmonic_np((0, 0, 0), (size[0], size[1], size[2]), size, base, amp, m, phase))
    return out


@pytest.mark.parametrize("n_domains", [1, 2])
def test_mhd_matches_numpy_reference(n_domains):
    size = (24, 24, 24)
    app = Astaroth(size, backend="native", gpus=[0] * n_domains)
    app.realize()
    app.init_fields()

    # numpy reference on the full periodic grid
    cf = {k: float(app.conf[k]) for k in ("dsx", "dsy", "dsz", "cs2", "cp_inv", "nu", "eta", "chi")}
    curr = global_init(size)
    nxt = [np.zeros(curr[0].shape) for _ in range(8)]
    dt = 1e-4

    # device init must match the numpy init
    got0 = app.read_field(0, "lnrho")
    lo, hi = app.dd.local_rect(0)
    np.testing.assert_allclose(
        got0, curr[0][lo[2] : hi[2], lo[1] : hi[1], lo[0] : hi[0]], rtol=0, atol=1e-13
    )

    for _ in range(2):  # two full iterations = 6 substeps
        app.step(dt=dt)
        for s in range(3):
            curr, nxt = M.substep(curr, nxt, s, dt, cf)

    for li in range(app.dd.num_local()):
        lo, hi = app.dd.local_rect(li)
        for qi, name in enumerate(FIELDS):
            got = app.read_field(li, name)
            want = curr[qi][lo[2] : hi[2], lo[1] : hi[1], lo[0] : hi[0]]
            np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-12, err_msg=f"{name} li={li}")


@pytest.mark.parametrize("mode", ["graph", "eager"])
def test_mhd_ychunk_dispatch_matches_numpy_reference(mode, monkeypatch):
    """y-chunked block dispatch (the default at every benchmark size): with
    the default 64x2x2 block, (16, 68, 12) gives a 1x34x6 block grid, for
    which the default chunk request of 32 picks C = 17, so the in-kernel
    remap really runs. x does not fill a block and the three extents differ,
    so an axis mix-up in the block decode cannot cancel."""
    monkeypatch.setenv("STENCIL_AMD_STEP_GRAPH", "1" if mode == "graph" else "0")
    size = (16, 68, 12)
    app = Astaroth(size, backend="native", gpus=[0])
    app.realize()
    if mode == "graph":
        assert app._graph is not None, "mhd graph did not activate"
    else:
        assert app._graph is None
    app.init_fields()

    cf = {k: float(app.conf[k]) for k in ("dsx", "dsy", "dsz", "cs2", "cp_inv", "nu", "eta", "chi")}
    curr = global_init(size)
    nxt = [np.zeros(curr[0].shape) for _ in range(8)]
    dt = 1e-4
    for _ in range(2):  # two full iterations = 6 substeps
        app.step(dt=dt)
        for s in range(3):
            curr, nxt = M.substep(curr, nxt, s, dt, cf)

    lo, hi = app.dd.local_rect(0)
    for qi, name in enumerate(FIELDS):
        got = app.read_field(0, name)
        want = curr[qi][lo[2] : hi[2], lo[1] : hi[1], lo[0] : hi[0]]
        np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-12, err_msg=name)


def test_mhd_no_compute_mode():
    app = Astaroth((16, 16, 16), backend="native", gpus=[0])
    app.realize()
    app.init_fields()
    app.step(compute=False)  # pure exchange path must run
    arr = app.read_field(0, "uux")
    assert np.isfinite(arr).all()


@pytest.mark.parametrize("stream_id", [-1, 2])
def test_mhd_rejects_stream_id_other_than_0_or_1(stream_id):
    """an engine has compute streams 0 and 1 per domain; any other id is an
    error, not an alias of one of them"""
    from stencil_amd import _C

    app = Astaroth((16, 16, 16), backend="native", gpus=[0])
    app.realize()
    lo, hi = app.dd.local_rect(0)
    rect = _C.Rect3(_C.Vec3(*lo), _C.Vec3(*hi))
    with pytest.raises(ValueError):
        _C.mhd_div_pass(app.dd.backend.engine, 0, rect, app.cf, stream_id)


def test_mhd_overlap_equals_no_overlap():
    """interior/exterior overlap (with per-stream scratch) must be
    bitwise-identical to the sequential full-region sweep"""
    outs = []
    for overlap in (True, False):
        app = Astaroth((20, 20, 20), backend="native", gpus=[0, 0])
        app.realize()
        app.init_fields()
        app.step(dt=1e-4, overlap=overlap)
        outs.append(
            [app.read_field(li, n) for li in range(app.dd.num_local()) for n in FIELDS]
        )
    for a, b in zip(outs[0], outs[1]):
        np.testing.assert_array_equal(a, b)


def test_mhd_substep_graph_matches_eager(monkeypatch):
    """whole-substep hipGraph path (auto at world=1, conf dt) must be
    bitwise-identical to the eager path over full iterations"""
    size = (20, 20, 20)
    outs = {}
    for mode in ("graph", "eager"):
        monkeypatch.setenv("STENCIL_AMD_STEP_GRAPH", "1" if mode == "graph" else "0")
        app = Astaroth(size, backend="native", gpus=[0])
        app.realize()
        if mode == "graph":
            assert app._graph is not None, "mhd graph did not activate"
        else:
            assert app._graph is None
        app.init_fields()
        for _ in range(2):
            app.step(overlap=False)  # conf dt -> graph path when active
        outs[mode] = np.stack([app.read_field(0, n) for n in FIELDS])
    assert np.isfinite(outs["graph"]).all()
    np.testing.assert_array_equal(outs["graph"], outs["eager"])


def test_radial_init_matches_numpy():
    """init_radial_f64 (reference radial_explosion_init_kernel analog)
    vs the NumPy gaussian, and a few stable steps from the explosion IC"""
    from stencil_amd.models.astaroth import Astaroth

    size = (24, 20, 16)
    app = Astaroth(size, backend="native")
    app.realize()
    app.init_fields(kind="explosion")
    cx, cy, cz = (s / 2.0 for s in size)
    sigma = min(size) / 8.0
    lo, hi = app.dd.local_rect(0)
    got = app.read_field(0, "uux")
    zz, yy, xx = np.meshgrid(
        np.arange(lo[2], hi[2], dtype=np.float64),
        np.arange(lo[1], hi[1], dtype=np.float64),
        np.arange(lo[0], hi[0], dtype=np.float64),
        indexing="ij",
    )
    want = 0.1 * np.exp(
        -((xx - cx) ** 2 + (yy - cy) ** 2 + (zz - cz) ** 2) / (2 * sigma * sigma)
    )
    np.testing.assert_allclose(got, want, rtol=1e-13, atol=1e-15)
    assert np.allclose(app.read_field(0, "lnrho"), 0.0)
    app.step()
    app.step()
    for name in ("lnrho", "uux", "ss"):
        assert np.isfinite(app.read_field(0, name)).all()
