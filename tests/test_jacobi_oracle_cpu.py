"""The NumPy Jacobi oracle (jacobi_util.py) against the torch backend, on
the CPU: bitwise over 3 steps. No kernel is involved; this validates the
oracle that test_gpu_jacobi_oracle.py holds the HIP kernels to, and it runs
on any machine."""
import numpy as np
import pytest

from stencil_amd import Boundary

import jacobi_util as ju

STEPS = 3

ALL_FACES = ("x-", "x+", "y-", "y+", "z-", "z+")


def _run_torch(size, n_domains, g0, steps=STEPS, **kw):
    from stencil_amd.models.jacobi3d import Jacobi3D

    app = Jacobi3D(size, backend="torch", gpus=[0] * n_domains, **kw)
    app.realize()
    ju.scatter(app.dd, app.h, g0)  # realize() filled 0.5: the field goes in afterwards
    for _ in range(steps):
        app.step()
    return app


def _field(size, seed=7):
    return ju.random_field((size[2], size[1], size[0]), seed)


@pytest.mark.parametrize(
    "size,n_domains",
    [((30, 9, 7), 2), ((62, 5, 3), 1), ((19, 10, 9), 4), ((8, 4, 3), 1)],
    ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"{v}dom",
)
def test_oracle_equals_torch_backend_periodic(size, n_domains):
    g0 = _field(size)
    app = _run_torch(size, n_domains, g0)
    assert app.dd.num_local() == n_domains
    ju.assert_rects_equal(app.dd, app.h, ju.jacobi_global(g0, STEPS), "periodic")


@pytest.mark.parametrize(
    "kinds",
    [
        {f: (Boundary.FIXED, 0.25) for f in ALL_FACES},
        {f: (Boundary.MIRROR, 0) for f in ALL_FACES},
    ],
    ids=["fixed", "mirror"],
)
def test_oracle_equals_torch_backend_walls(kinds):
    size = (19, 10, 9)
    g0 = _field(size, seed=11)
    app = _run_torch(size, 2, g0, boundary=kinds)
    want = ju.jacobi_global(g0, STEPS, ju.walls_pad(kinds))
    ju.assert_rects_equal(app.dd, app.h, want, "walls")


def test_oracle_equals_torch_backend_halo_multiplier():
    size = (19, 10, 9)
    g0 = _field(size, seed=13)
    # 4 steps: two whole exchange periods of the temporal blocking
    app = _run_torch(size, 2, g0, steps=4, halo_multiplier=2)
    ju.assert_rects_equal(app.dd, app.h, ju.jacobi_global(g0, 4), "halo_multiplier=2")


def test_oracle_is_not_vacuous():
    """the field is not separable: swapping two neighbours of one axis pair
    keeps the sum's value set but the rounding differs somewhere, and the
    spheres override cells"""
    size = (30, 9, 7)
    g0 = _field(size)
    one = ju.jacobi_global(g0, 1)
    hot, cold = ju.sphere_masks((0, 0, 0), size, (0, 0, 0), size)
    assert hot.sum() > 1 and cold.sum() > 1  # radius 3
    assert (one[hot] == 1.0).all() and (one[cold] == 0.0).all()
    # a shifted neighbour is seen
    shifted = ju.jacobi_cells(np.roll(ju.wrap_pad(g0), 1, axis=2), (0, 0, 0), size, (0, 0, 0), size)
    free = ~(hot | cold)
    assert (ju.bits(one)[free] != ju.bits(shifted)[free]).mean() > 0.9
    hot0, cold0 = ju.sphere_masks((0, 0, 0), (8, 4, 3), (0, 0, 0), (8, 4, 3))
    assert hot0.sum() == 1 and cold0.sum() == 1  # radius 0: the centre cells alone
