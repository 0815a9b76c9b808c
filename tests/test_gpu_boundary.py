"""Non-periodic boundary conditions on a real MI355X: the batched
boundary_fill kernel (csrc/src/boundary.hip) against the numpy.pad oracle,
bitwise, through the Python and C++ orchestrators, exchange groups, buffer
swaps, the staged-local path, the jacobi step graph and 2-rank IPC."""
import multiprocessing as mp
import os

import numpy as np
import pytest

import stencil_amd as sa
from stencil_amd import Boundary, _C

from boundary_util import (
    FIXED_VALUE,
    MIXED,
    SENTINEL,
    all_faces,
    apply_boundary,
    check_boundary_regions,
    fill,
    padded_global,
    write_sentinel,
)
from util import full_region_of

pytestmark = pytest.mark.gpu

KINDS = {
    "fixed": all_faces(Boundary.FIXED, FIXED_VALUE),
    "clamp": all_faces(Boundary.CLAMP),
    "mirror": all_faces(Boundary.MIRROR),
    "antimirror": all_faces(Boundary.ANTIMIRROR),
    "mixed": MIXED,
}


def make_radius(r):
    if r == "asym":
        rad = _C.Radius.constant(1)
        rad.set_dir(1, 0, 0, 2)
        return rad
    return _C.Radius.constant(r)


def make_dd(size, r, n_domains=1):
    dd = sa.DistributedDomain(*size, backend="native")
    dd.set_radius(make_radius(r))
    dd.set_gpus([0] * n_domains)  # same-GPU fake-multi-GPU
    return dd


_ORACLE = {}


def oracle(size, r, kinds, scale=1.0):
    """the padded global array, computed once per (shape, radius, kinds)"""
    key = (size, r, kinds, scale)
    if key not in _ORACLE:
        want = padded_global(size, make_radius(r), KINDS[kinds], scale)
        want.setflags(write=False)
        _ORACLE[key] = want
    return _ORACLE[key]


@pytest.mark.parametrize("kinds", list(KINDS))
@pytest.mark.parametrize("n_domains", [1, 2, 8])
@pytest.mark.parametrize("r", [1, 3, "asym"])
@pytest.mark.parametrize("size", [(12, 10, 8), (13, 10, 8)])
def test_native_fill_matches_oracle(size, r, n_domains, kinds):
    dd = make_dd(size, r, n_domains)
    h = dd.add_data(np.float32, "q")
    apply_boundary(dd, KINDS[kinds])
    dd.realize()
    fill(dd, h)
    dd.exchange()
    check_boundary_regions(dd, h, KINDS[kinds], want=oracle(size, r, kinds))
    assert dd.boundary_bytes > 0
    assert set(dd.bytes_by_method) == {"direct_kernel", "rccl", "ipc_kernel"}


@pytest.mark.parametrize("kinds", list(KINDS))
@pytest.mark.parametrize("r", [1, 3])
def test_three_domains_middle_has_no_boundary_face(r, kinds):
    """(18,4,4) on 3 domains splits x: the middle subdomain has no
    boundary face on the split axis"""
    size = (18, 4, 4)
    dd = make_dd(size, r, 3)
    h = dd.add_data(np.float32, "q")
    apply_boundary(dd, KINDS[kinds])
    dd.realize()
    assert dd.placement.dim() == (3, 1, 1)
    fill(dd, h)
    dd.exchange()
    check_boundary_regions(dd, h, KINDS[kinds], want=oracle(size, r, kinds))


def test_mixed_element_sizes():
    """1/2/4/8-byte quantities in one domain: ANTIMIRROR on the floats,
    FIXED and MIRROR on the integers"""
    dd = make_dd((13, 10, 8), 2, 2)
    hs = [dd.add_data(np.uint8, "a"), dd.add_data(np.int16, "b"),
          dd.add_data(np.float32, "c"), dd.add_data(np.float64, "d")]
    int_kinds = {
        "x-": (Boundary.FIXED, 7), "x+": (Boundary.FIXED, 9),
        "y-": (Boundary.MIRROR, 0), "y+": (Boundary.MIRROR, 0),
        "z-": (Boundary.MIRROR, 0), "z+": (Boundary.FIXED, 3),
    }
    flt_kinds = all_faces(Boundary.ANTIMIRROR)
    apply_boundary(dd, int_kinds, hs[:2])
    apply_boundary(dd, flt_kinds, hs[2:])
    dd.realize()
    for i, h in enumerate(hs):
        fill(dd, h, scale=1.0 + i)
    dd.exchange()
    for i, h in enumerate(hs):
        check_boundary_regions(dd, h, int_kinds if i < 2 else flt_kinds, scale=1.0 + i)


def test_exchange_groups_fill_only_their_quantities():
    dd = make_dd((12, 10, 8), 2, 2)
    a = dd.add_data(np.float32, "a")
    b = dd.add_data(np.float32, "b")
    dd.set_exchange_groups([[a.index], [b.index]])
    ka, kb = all_faces(Boundary.CLAMP), all_faces(Boundary.MIRROR)
    apply_boundary(dd, ka, [a])
    apply_boundary(dd, kb, [b])
    dd.realize()
    for h in (a, b):
        write_sentinel(dd, h)
        fill(dd, h)
    dd.exchange(group=1)
    check_boundary_regions(dd, b, kb)
    # group 0 was not exchanged: every halo cell of `a` still holds the sentinel
    for li in range(dd.num_local()):
        flo, fhi = full_region_of(dd, li)
        lo, hi = dd.local_rect(li)
        got = dd.read_global(li, flo, fhi, a).copy()
        inner = tuple(slice(lo[i] - flo[i], hi[i] - flo[i]) for i in (2, 1, 0))
        got[inner] = SENTINEL
        assert np.all(got == np.float32(SENTINEL))
    dd.exchange(group=0)
    check_boundary_regions(dd, a, ka)
    check_boundary_regions(dd, b, kb)


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
def test_open_cells_keep_the_sentinel(n_domains, kinds):
    dd = make_dd((12, 10, 8), 2, n_domains)
    h = dd.add_data(np.float32, "q")
    apply_boundary(dd, OPEN_MIXES[kinds])
    dd.realize()
    write_sentinel(dd, h)
    fill(dd, h)
    dd.exchange()
    # OPEN cells outside stay at the sentinel; cells inside are exchanged
    check_boundary_regions(dd, h, OPEN_MIXES[kinds], open_value=SENTINEL)


def test_fill_follows_buffer_parity():
    dd = make_dd((12, 10, 8), 2, 2)
    h = dd.add_data(np.float32, "q")
    apply_boundary(dd, KINDS["mixed"])
    dd.realize()
    fill(dd, h)
    dd.exchange()
    check_boundary_regions(dd, h, KINDS["mixed"])
    dd.swap()
    fill(dd, h, scale=2.0)
    dd.exchange()
    check_boundary_regions(dd, h, KINDS["mixed"], scale=2.0)
    dd.swap()  # the first buffer still holds the scale-1 fill
    check_boundary_regions(dd, h, KINDS["mixed"])


@pytest.mark.parametrize("r", [1, 2])
def test_fill_after_staged_local_unpacks(r, monkeypatch):
    monkeypatch.setenv("STENCIL_AMD_STAGE_LOCAL", "all")
    dd = make_dd((12, 10, 8), r, 2)
    h = dd.add_data(np.float32, "q")
    apply_boundary(dd, KINDS["mixed"])
    dd.realize()
    assert any(dd.backend._staged_local), "staged-local path did not engage"
    fill(dd, h)
    dd.exchange()
    check_boundary_regions(dd, h, KINDS["mixed"])
    dd.swap()
    fill(dd, h, scale=3.0)
    dd.exchange()
    check_boundary_regions(dd, h, KINDS["mixed"], scale=3.0)


JACOBI_BC = {
    "fixed": {"all": (Boundary.FIXED, 0.25)},
    "mirror": {"all": Boundary.MIRROR},
}


def _run_jacobi(backend, size, steps, n_domains, boundary):
    from stencil_amd.models.jacobi3d import Jacobi3D
    from util import fill_interiors

    app = Jacobi3D(size, backend=backend, gpus=[0] * n_domains, boundary=boundary)
    app.realize()
    fill_interiors(app.dd, app.h)
    for _ in range(steps):
        app.step()
    out = []
    for li in range(app.dd.num_local()):
        lo, hi = app.dd.local_rect(li)
        out.append((lo, app.dd.read_global(li, lo, hi, app.h)))
    return app, out


_JACOBI_REF = {}


@pytest.mark.parametrize("n_domains", [1, 2])
@pytest.mark.parametrize("bc", list(JACOBI_BC))
def test_jacobi_matches_torch_with_walls(bc, n_domains):
    size = (20, 16, 12)
    _app, native = _run_jacobi("native", size, 3, n_domains, JACOBI_BC[bc])
    key = (bc, n_domains)
    if key not in _JACOBI_REF:
        _JACOBI_REF[key] = _run_jacobi("torch", size, 3, n_domains, JACOBI_BC[bc])[1]
    ref = _JACOBI_REF[key]
    assert len(native) == len(ref)
    for (lo_n, a), (lo_t, b) in zip(native, ref):
        assert lo_n == lo_t
        np.testing.assert_array_equal(a, b)


def test_jacobi_step_graph_matches_eager_with_fixed_walls(monkeypatch):
    size = (24, 18, 14)
    outs = {}
    for mode in ("graph", "eager"):
        monkeypatch.setenv("STENCIL_AMD_STEP_GRAPH", "1" if mode == "graph" else "0")
        app, out = _run_jacobi("native", size, 4, 1, JACOBI_BC["fixed"])
        assert (app._graph is not None) == (mode == "graph")
        assert not app.dd.plan.translates  # fully non-periodic: [fill -> jacobi -> swap]
        outs[mode] = out[0][1]
    np.testing.assert_array_equal(outs["graph"], outs["eager"])


def test_cpp_domain_matches_python_native():
    size, r = (12, 10, 8), 2
    kinds = KINDS["mixed"]
    py = make_dd(size, r, 2)
    h = py.add_data(np.float32, "q")
    apply_boundary(py, kinds)
    py.realize()
    fill(py, h)
    py.exchange()
    check_boundary_regions(py, h, kinds)

    dd = _C.CppDistributedDomain(*size)
    dd.set_radius(_C.Radius.constant(r))
    qi = dd.add_data(4, "q")
    dd.set_gpus([0, 0])
    for face, (kind, value) in kinds.items():
        dd.set_boundary(face, kind, value)
    dd.realize()
    assert dd.boundary_bytes() == py.boundary_bytes
    rects = {}
    for li in range(dd.num_local()):
        rect = dd.local_rect(li)
        lo, hi = rect.lo.tuple(), rect.hi.tuple()
        ext = tuple(hi[i] - lo[i] for i in range(3))
        from boundary_util import field

        dd.domain(li).region_from_host(
            field(lo, hi, size, 1.0, np.float32).tobytes(), _C.Vec3(r, r, r), _C.Vec3(*ext), qi
        )
        rects[lo] = li
    dd.exchange()
    for pli in range(py.num_local()):
        lo, hi = py.local_rect(pli)
        flo, fhi = full_region_of(py, pli)
        want = py.read_global(pli, flo, fhi, h)
        fext = tuple(fhi[i] - flo[i] for i in range(3))
        raw = dd.domain(rects[lo]).region_to_host(_C.Vec3(0, 0, 0), _C.Vec3(*fext), qi)
        got = np.frombuffer(raw, dtype=np.float32).reshape(fext[2], fext[1], fext[0])
        assert np.array_equal(got, want)


def test_cpp_domain_validation():
    dd = _C.CppDistributedDomain(12, 10, 8)
    dd.set_radius(_C.Radius.constant(1))
    dd.add_data(4, "q")
    dd.set_gpus([0])
    dd.set_boundary("x-", Boundary.CLAMP)
    with pytest.raises(ValueError):
        dd.realize()
    dd = _C.CppDistributedDomain(12, 10, 8)
    dd.set_radius(_C.Radius.constant(1))
    dd.add_data(2, "q")  # size-canonical int16
    dd.set_gpus([0])
    dd.set_boundary("z", Boundary.ANTIMIRROR)
    with pytest.raises(ValueError):
        dd.realize()


# ---- 2 ranks on one GPU (harness as tests/test_gpu_mp.py) ----


def _ipc_worker(rank, world, port, q, use_ipc):
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        os.environ["STENCIL_AMD_WIRE"] = "cpu"  # single GPU: stage over gloo
        os.environ["STENCIL_AMD_IPC"] = "1" if use_ipc else "0"
        import torch.distributed as dist

        dist.init_process_group("gloo", rank=rank, world_size=world)
        import sys

        sys.path.insert(0, os.path.dirname(__file__))
        import stencil_amd as sa
        from stencil_amd import Boundary
        from boundary_util import all_faces, apply_boundary, check_boundary_regions, fill

        kinds = all_faces(Boundary.CLAMP)
        dd = sa.DistributedDomain(12, 10, 8, backend="native")
        dd.set_radius(2)
        dd.set_gpus([0])
        h = dd.add_data(np.float32, "q")
        apply_boundary(dd, kinds)
        dd.realize()
        if use_ipc:
            assert dd.backend._ipc_active, f"IPC did not activate: {dd.backend._ipc_error}"
            assert dd.bytes_by_method["ipc_kernel"] > 0
        else:  # packed wire: the fill is ordered behind the wire unpacks
            assert dd.bytes_by_method["rccl"] > 0
        assert dd.boundary_bytes > 0
        fill(dd, h)
        dd.exchange()
        check_boundary_regions(dd, h, kinds)
        dd.swap()
        fill(dd, h, scale=2.0)
        dd.exchange()
        check_boundary_regions(dd, h, kinds, scale=2.0)
        dist.destroy_process_group()
        q.put((rank, "ok"))
    except Exception as e:  # pragma: no cover
        import traceback

        q.put((rank, f"FAIL: {e}\n{traceback.format_exc()}"))


@pytest.mark.parametrize("use_ipc,port", [(True, 29745), (False, 29749)])
def test_two_rank_clamp_one_gpu(use_ipc, port):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_ipc_worker, args=(r, 2, port, q, use_ipc)) for r in range(2)]
    for p in procs:
        p.start()
    results = [q.get(timeout=300) for _ in procs]
    for p in procs:
        p.join(timeout=30)
        if p.is_alive():
            p.terminate()
    for rank, status in results:
        assert status == "ok", f"rank {rank}: {status}"
