"""Cross-process exchange with the NATIVE backend on one GPU (2 ranks,
gloo control plane). Two transports:
- wire: packed buffers staged over gloo (exercises DLPack export and the
  HIP pack/unpack kernels; on multi-GPU nodes the same path runs over
  RCCL with device buffers)
- ipc: direct-write translate kernels into the peer process's buffers via
  hipIpcMemHandle (the xGMI colocated path)
"""
import multiprocessing as mp
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _worker(rank, world, port, q, use_ipc):
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
        from util import check_full_regions, fill_interiors

        dd = sa.DistributedDomain(12, 10, 8, backend="native")
        dd.set_radius(2)
        dd.set_gpus([0])
        h = dd.add_data(np.float32, "q")
        dd.realize()
        if use_ipc:
            assert dd.backend._ipc_active, (
                f"IPC transport did not activate: {dd.backend._ipc_error}"
            )
            assert dd.bytes_by_method["ipc_kernel"] > 0
            assert dd.bytes_by_method["rccl"] == 0
        fill_interiors(dd, h)
        dd.exchange()
        check_full_regions(dd, h)
        dd.swap()
        fill_interiors(dd, h, scale=2.0)
        dd.exchange()
        check_full_regions(dd, h, scale=2.0)
        dist.destroy_process_group()
        q.put((rank, "ok"))
    except Exception as e:  # pragma: no cover
        import traceback

        q.put((rank, f"FAIL: {e}\n{traceback.format_exc()}"))


@pytest.mark.parametrize(
    "world,use_ipc,port", [(2, False, 29717), (2, True, 29721), (4, True, 29725)]
)
def test_native_multi_rank_one_gpu(world, use_ipc, port):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q, use_ipc)) for r in range(world)]
    for p in procs:
        p.start()
    results = [q.get(timeout=300) for _ in procs]
    for p in procs:
        p.join(timeout=30)
        if p.is_alive():
            p.terminate()
    for rank, status in results:
        assert status == "ok", f"rank {rank}: {status}"


def _jacobi_worker(rank, world, port, q, use_ipc, step_graph=True):
    """3 jacobi steps across 2 ranks, every rank returns its interior for
    comparison against the single-process torch reference (validates the
    mode-1/mode-2 fast-kernel paths AND the multi-rank whole-step graphs
    under the real multi-rank transports)"""
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        os.environ["STENCIL_AMD_WIRE"] = "cpu"
        os.environ["STENCIL_AMD_IPC"] = "1" if use_ipc else "0"
        os.environ["STENCIL_AMD_STEP_GRAPH"] = "1" if step_graph else "0"
        import torch.distributed as dist

        dist.init_process_group("gloo", rank=rank, world_size=world)
        import sys

        sys.path.insert(0, os.path.dirname(__file__))
        from stencil_amd.models.jacobi3d import Jacobi3D
        from util import fill_interiors

        size = (24, 18, 14)
        app = Jacobi3D(size, backend="native")
        app.dd.set_gpus([0])
        app.realize()
        if use_ipc:
            assert app.dd.backend._ipc_active, app.dd.backend._ipc_error
            # the multi-rank whole-step graph path must actually engage
            # when graphs are on (every cross-rank halo is IPC here)
            if step_graph:
                assert app._mr_graph is not None
            else:
                assert app._mr_graph is None
        fill_interiors(app.dd, app.h)
        for _ in range(3):
            app.step()
        out = []
        for li in range(app.dd.num_local()):
            lo, hi = app.dd.local_rect(li)
            out.append((lo, hi, app.dd.read_global(li, lo, hi, app.h)))
        # the app owns its step graph: nothing of it survives the app
        import gc

        from stencil_amd import _C

        del app
        gc.collect()
        assert _C.step_graphs_alive() == 0
        dist.destroy_process_group()
        q.put((rank, "ok", out))
    except Exception as e:  # pragma: no cover
        import traceback

        q.put((rank, f"FAIL: {e}\n{traceback.format_exc()}", None))


@pytest.mark.parametrize(
    "use_ipc,port,step_graph",
    [(True, 29731, True), (True, 29739, False), (False, 29735, True)],
)
def test_multi_rank_jacobi_matches_torch(use_ipc, port, step_graph):
    # torch single-process global reference
    import sys

    sys.path.insert(0, os.path.dirname(__file__))
    from stencil_amd.models.jacobi3d import Jacobi3D
    from util import fill_interiors

    size = (24, 18, 14)
    ref = Jacobi3D(size, backend="torch", gpus=[0, 0])
    ref.realize()
    fill_interiors(ref.dd, ref.h)
    for _ in range(3):
        ref.step()

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [
        ctx.Process(target=_jacobi_worker, args=(r, 2, port, q, use_ipc, step_graph))
        for r in range(2)
    ]
    for p in procs:
        p.start()
    results = [q.get(timeout=300) for _ in procs]
    for p in procs:
        p.join(timeout=30)
        if p.is_alive():
            p.terminate()
    for rank, status, out in results:
        assert status == "ok", f"rank {rank}: {status}"
        for lo, hi, arr in out:
            # read the same global box from the torch reference
            got_ref = None
            for li in range(ref.dd.num_local()):
                rlo, rhi = ref.dd.local_rect(li)
                if rlo == lo and rhi == hi:
                    got_ref = ref.dd.read_global(li, rlo, rhi, ref.h)
            assert got_ref is not None, f"no matching ref subdomain for {lo}"
            np.testing.assert_allclose(arr, got_ref, rtol=1e-6, atol=1e-6)
