"""Non-periodic boundary conditions, CPU tier: planner masks (Python and
C++), the torch backend's fill against the numpy.pad oracle, validation,
and one world-2 gloo run."""
import multiprocessing as mp
import os

import numpy as np
import pytest

import stencil_amd as sa
from stencil_amd import Boundary, _C
from stencil_amd.parallel.placement import NodeAwarePlacement, Slot, TrivialPlacement
from stencil_amd.parallel.planning import pair_seq_tags, plan_exchange
from stencil_amd.parallel.topology import Topology

from boundary_util import (
    FIXED_VALUE,
    MIXED,
    SENTINEL,
    all_faces,
    apply_boundary,
    check_boundary_regions,
    fill,
    write_sentinel,
)

ALL_TRUE = (True, True, True)


def _plan_tuple(plan):
    return (
        [(t.src_local, t.dst_local, t.dir, t.ext) for t in plan.translates],
        [
            (i.peer_rank, i.src_gid, i.dst_gid, i.local_id,
             [(m.dir, m.src_gid, m.dst_gid, m.ext) for m in i.messages])
            for i in plan.sends
        ],
        [
            (i.peer_rank, i.src_gid, i.dst_gid, i.local_id,
             [(m.dir, m.src_gid, m.dst_gid, m.ext) for m in i.messages])
            for i in plan.recvs
        ],
    )


# the shapes tests/test_planning.py plans
PLANNING_SHAPES = [
    ((32, 32, 32), 1, 1, 8),
    ((16, 16, 16), 1, 1, 1),
    ((20, 20, 20), 1, 2, 1),
    ((24, 8, 8), 1, 2, 1),
    ((16, 16, 16), 2, 2, 1),
]


@pytest.mark.parametrize("size,r,n_ranks,gpr", PLANNING_SHAPES)
def test_all_periodic_mask_changes_nothing(size, r, n_ranks, gpr):
    radius = _C.Radius.constant(r)
    slots = [Slot(rk, li, li, 0) for rk in range(n_ranks) for li in range(gpr)]
    p = TrivialPlacement(size, radius, slots)
    for rank in range(n_ranks):
        default = plan_exchange(p, radius, rank)
        explicit = plan_exchange(p, radius, rank, ALL_TRUE)
        assert _plan_tuple(default) == _plan_tuple(explicit)
        # a torus: every subdomain sends in all 26 directions
        n_msgs = len(default.translates) + sum(len(s.messages) for s in default.sends)
        assert n_msgs == 26 * p.num_local(rank)


MASKS = [(False, False, False), (True, False, True), (False, True, True)]


@pytest.mark.parametrize("periodic", MASKS)
@pytest.mark.parametrize("n_slots", [1, 2, 3, 4, 8])
def test_cpp_python_plan_parity_nonperiodic(periodic, n_slots):
    size, radius = (24, 20, 16), _C.Radius.constant(2)
    slots = [Slot(rk, 0, rk, 0) for rk in range(n_slots)]
    tuples = [(s.rank, s.local_id, s.cuda, s.node) for s in slots]
    pp = NodeAwarePlacement(size, radius, slots)
    dim = pp.dim()
    for rank in range(n_slots):
        cpp = _C.cpp_plan(_C.Vec3(*size), radius, rank, tuples, "node_aware", periodic=periodic)
        plan = plan_exchange(pp, radius, rank, periodic)
        tags = pair_seq_tags(plan)
        got = (
            [(sl, dl, tuple(d), tuple(e)) for sl, dl, d, e in cpp["translates"]],
            [
                (peer, sg, dg, li, [(tuple(d), a, b, tuple(e)) for d, a, b, e in msgs])
                for peer, sg, dg, li, msgs, _tag in cpp["sends"]
            ],
            [
                (peer, sg, dg, li, [(tuple(d), a, b, tuple(e)) for d, a, b, e in msgs])
                for peer, sg, dg, li, msgs, _tag in cpp["recvs"]
            ],
        )
        assert got == _plan_tuple(plan)
        for key, items in (("sends", plan.sends), ("recvs", plan.recvs)):
            for (peer, sg, dg, _li, _m, tag), it in zip(cpp[key], items):
                assert tag == tags[(it.peer_rank, it.src_gid, it.dst_gid)]

        # no plan item crosses a non-periodic edge
        def crossing(gid, d, sign):
            idx = pp.dimensionize(gid)
            return any(
                not periodic[a] and not 0 <= idx[a] + sign * d[a] < dim[a] for a in range(3)
            )

        for t in plan.translates:
            src_gid = pp.linearize(pp.get_idx(rank, t.src_local))
            assert not crossing(src_gid, t.dir, 1)
        for item in plan.sends + plan.recvs:
            for m in item.messages:
                assert not crossing(m.src_gid, m.dir, 1)
                assert not crossing(m.dst_gid, m.dir, -1)


def test_single_domain_nonperiodic_has_no_self_wrap():
    radius = _C.Radius.constant(1)
    p = TrivialPlacement((16, 16, 16), radius, [Slot(0, 0, 0, 0)])
    plan = plan_exchange(p, radius, 0, (False, False, False))
    assert not plan.translates and not plan.sends and not plan.recvs
    plan = plan_exchange(p, radius, 0, (True, False, False))
    assert sorted(t.dir for t in plan.translates) == [(-1, 0, 0), (1, 0, 0)]


def test_topology_mask():
    t = Topology((2, 3, 1), (False, True, False))
    assert t.get_neighbor((0, 0, 0), (-1, 0, 0)) is None
    assert t.get_neighbor((1, 0, 0), (1, 0, 0)) is None
    assert t.get_neighbor((0, 0, 0), (1, -1, 0)) == (1, 2, 0)
    assert t.get_neighbor((0, 0, 0), (0, 0, 1)) is None
    assert Topology((2, 3, 1)).get_neighbor((0, 0, 0), (-1, -1, -1)) == (1, 2, 0)


def make_dd(size, radius, n_domains, backend="torch"):
    dd = sa.DistributedDomain(*size, backend=backend)
    dd.set_radius(radius)
    dd.set_gpus([0] * n_domains)
    return dd


KINDS = {
    "fixed": all_faces(Boundary.FIXED, FIXED_VALUE),
    "clamp": all_faces(Boundary.CLAMP),
    "mirror": all_faces(Boundary.MIRROR),
    "antimirror": all_faces(Boundary.ANTIMIRROR),
    "mixed": MIXED,
}


@pytest.mark.parametrize("kinds", list(KINDS))
@pytest.mark.parametrize("n_domains", [1, 2, 3, 8])
@pytest.mark.parametrize("r", [1, 3])
@pytest.mark.parametrize("size", [(12, 10, 8), (13, 10, 8)])
def test_torch_fill_matches_oracle(size, r, n_domains, kinds):
    dd = make_dd(size, r, n_domains)
    h = dd.add_data(np.float32, "q")
    apply_boundary(dd, KINDS[kinds])
    dd.realize()
    fill(dd, h)
    dd.exchange()
    check_boundary_regions(dd, h, KINDS[kinds])
    assert dd.boundary_bytes > 0
    assert "boundary" not in dd.bytes_by_method


OPEN_MIXES = {
    "all_open": all_faces(Boundary.OPEN),
    "open_mix": {
        "x-": (Boundary.OPEN, 0), "x+": (Boundary.FIXED, 3.0),
        "y-": (Boundary.ANTIMIRROR, 0), "y+": (Boundary.OPEN, 0),
        "z-": (Boundary.CLAMP, 0), "z+": (Boundary.ANTIMIRROR, 0),
    },
}


@pytest.mark.parametrize("kinds", list(OPEN_MIXES))
@pytest.mark.parametrize("n_domains", [1, 2])
def test_torch_open_cells_keep_the_sentinel(n_domains, kinds):
    dd = make_dd((12, 10, 8), 2, n_domains)
    h = dd.add_data(np.float32, "q")
    apply_boundary(dd, OPEN_MIXES[kinds])
    dd.realize()
    write_sentinel(dd, h)
    fill(dd, h)
    dd.exchange()
    check_boundary_regions(dd, h, OPEN_MIXES[kinds], open_value=SENTINEL)


def test_torch_mixed_element_sizes():
    dd = make_dd((13, 10, 8), 2, 2)
    hs = [dd.add_data(np.uint8, "a"), dd.add_data(np.int16, "b"),
          dd.add_data(np.float16, "h"), dd.add_data(np.float64, "d")]
    int_kinds = {
        "x-": (Boundary.FIXED, 7), "x+": (Boundary.FIXED, 9),
        "y-": (Boundary.MIRROR, 0), "y+": (Boundary.MIRROR, 0),
        "z-": (Boundary.MIRROR, 0), "z+": (Boundary.FIXED, 3),
    }
    flt_kinds = dict(all_faces(Boundary.ANTIMIRROR), **{"x+": (Boundary.FIXED, FIXED_VALUE)})
    apply_boundary(dd, int_kinds, hs[:2])
    apply_boundary(dd, flt_kinds, hs[2:])
    dd.realize()
    for i, h in enumerate(hs):
        fill(dd, h, scale=1.0 + i)
    dd.exchange()
    for i, h in enumerate(hs):
        check_boundary_regions(dd, h, int_kinds if i < 2 else flt_kinds, scale=1.0 + i)


def test_plan_file_lines(tmp_path):
    for kinds, expect in ((None, False), (KINDS["clamp"], True)):
        dd = make_dd((12, 10, 8), 1, 2)
        dd.add_data(np.float32, "q")
        dd.set_output_prefix(str(tmp_path) + "/")
        if kinds:
            apply_boundary(dd, kinds)
        dd.realize()
        text = (tmp_path / "plan_0.txt").read_text()
        assert ("boundary_fill dir=" in text) == expect
        assert (dd.boundary_bytes > 0) == expect


# ---- validation ----


def test_mixed_periodic_axis_rejected():
    dd = make_dd((12, 10, 8), 1, 1)
    dd.add_data(np.float32, "q")
    dd.set_boundary("x-", Boundary.CLAMP)
    with pytest.raises(ValueError):
        dd.realize()


def test_mixed_periodic_axis_across_quantities_rejected():
    dd = make_dd((12, 10, 8), 1, 1)
    a = dd.add_data(np.float32, "a")
    dd.add_data(np.float32, "b")
    dd.set_boundary("x", Boundary.CLAMP, quantities=[a])
    with pytest.raises(ValueError):
        dd.realize()


def test_set_boundary_after_realize_rejected():
    dd = make_dd((12, 10, 8), 1, 1)
    dd.add_data(np.float32, "q")
    dd.realize()
    with pytest.raises(ValueError):
        dd.set_boundary("all", Boundary.CLAMP)


@pytest.mark.parametrize("kind", [Boundary.MIRROR, Boundary.ANTIMIRROR])
def test_mirror_radius_larger_than_subdomain_rejected(kind):
    dd = make_dd((12, 10, 4), 3, 2)  # z extent 4 splits... x splits: 6 >= 3; z = 4 >= 3
    dd.add_data(np.float32, "q")
    dd.set_boundary("all", kind)
    dd.realize()  # fits
    dd = make_dd((12, 10, 2), 3, 1)  # z extent 2 < radius 3
    dd.add_data(np.float32, "q")
    dd.set_boundary("all", kind)
    with pytest.raises(ValueError):
        dd.realize()


def test_clamp_on_empty_extent_rejected():
    dd = make_dd((12, 10, 0), 1, 1)
    dd.add_data(np.float32, "q")
    dd.set_boundary("z", Boundary.CLAMP)
    with pytest.raises(ValueError):
        dd.realize()


@pytest.mark.parametrize("dtype", [np.int16, np.uint8, np.int32])
def test_antimirror_on_non_float_rejected(dtype):
    dd = make_dd((12, 10, 8), 1, 1)
    dd.add_data(dtype, "q")
    dd.set_boundary("z", Boundary.ANTIMIRROR)
    with pytest.raises(ValueError):
        dd.realize()


def test_unknown_face_rejected():
    dd = make_dd((12, 10, 8), 1, 1)
    dd.add_data(np.float32, "q")
    with pytest.raises(ValueError):
        dd.set_boundary("w+", Boundary.CLAMP)


def test_jacobi_rejects_open_and_halo_multiplier():
    from stencil_amd.models.jacobi3d import Jacobi3D

    with pytest.raises(ValueError):
        Jacobi3D((16, 16, 16), backend="torch", boundary={"all": Boundary.OPEN})
    with pytest.raises(ValueError):
        Jacobi3D((16, 16, 16), backend="torch", halo_multiplier=2,
                 boundary={"z": (Boundary.FIXED, 1.0)})


def test_jacobi_torch_fixed_walls_hold():
    """a box with all faces FIXED at 0.25: after a step every halo cell
    outside the domain still reads 0.25 and the interior stays in range"""
    from stencil_amd.models.jacobi3d import Jacobi3D

    app = Jacobi3D((16, 12, 10), backend="torch", gpus=[0, 0],
                   boundary={"all": (Boundary.FIXED, 0.25)})
    app.realize()
    for _ in range(2):
        app.step()
    app.dd.exchange()
    from util import full_region_of

    for li in range(app.dd.num_local()):
        flo, fhi = full_region_of(app.dd, li)
        arr = app.dd.read_global(li, flo, fhi, app.h)
        zz, yy, xx = np.meshgrid(
            np.arange(flo[2], fhi[2]), np.arange(flo[1], fhi[1]), np.arange(flo[0], fhi[0]),
            indexing="ij",
        )
        outside = (
            (xx < 0) | (xx >= 16) | (yy < 0) | (yy >= 12) | (zz < 0) | (zz >= 10)
        )
        assert np.all(arr[outside] == np.float32(0.25))
        assert arr.min() >= 0.0 and arr.max() <= 1.0


def test_jacobi3d_cli_boundary():
    import subprocess
    import sys

    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run(
        [sys.executable, os.path.join(repo, "benchmarks", "jacobi3d.py"), "--backend", "torch",
         "--size", "16", "--iters", "2", "--gpus", "2", "--boundary", "mirror", "--queued"],
        capture_output=True, text=True, timeout=300, cwd=repo,
    )
    assert out.returncode == 0, out.stderr
    assert "boundary=mirror,bytes_boundary=" in out.stdout
    assert "ms_per_step_queued=" in out.stdout


# ---- world-2 gloo (harness as tests/test_mp_gloo.py) ----


def _worker(rank, world, port, q):
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        import torch.distributed as dist

        dist.init_process_group("gloo", rank=rank, world_size=world)
        import sys

        sys.path.insert(0, os.path.dirname(__file__))
        import stencil_amd as sa
        from boundary_util import MIXED, apply_boundary, check_boundary_regions, fill

        dd = sa.DistributedDomain(12, 10, 8, backend="torch")
        dd.set_radius(2)
        dd.set_gpus([0, 0])
        h = dd.add_data(np.float32, "q")
        apply_boundary(dd, MIXED)
        dd.realize()
        assert dd.plan.sends and dd.plan.recvs
        fill(dd, h)
        dd.exchange()
        check_boundary_regions(dd, h, MIXED)
        dd.swap()
        fill(dd, h, scale=2.0)
        dd.exchange()
        check_boundary_regions(dd, h, MIXED, scale=2.0)
        dist.destroy_process_group()
        q.put((rank, "ok"))
    except Exception as e:  # pragma: no cover
        import traceback

        q.put((rank, f"FAIL: {e}\n{traceback.format_exc()}"))


def test_two_ranks_gloo_mixed_boundary():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 2, 29641, q)) for r in range(2)]
    for p in procs:
        p.start()
    results = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=30)
        if p.is_alive():
            p.terminate()
    for rank, status in results:
        assert status == "ok", f"rank {rank}: {status}"
