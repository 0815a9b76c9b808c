"""The driver depends on bench.py's CLI + JSON output contract; verify it
end-to-end on the torch backend (CPU, tiny grid)."""
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_json_contract():
    out = subprocess.run(
        [
            sys.executable,
            os.path.join(REPO, "bench.py"),
            "--backend",
            "torch",
            "--gpus",
            "1",
            "--per-gpu",
            "32",
            "--steps",
            "2",
            "--warmup",
            "1",
        ],
        capture_output=True,
        text=True,
        timeout=300,
        cwd=REPO,
    )
    assert out.returncode == 0, out.stderr
    lines = [l for l in out.stdout.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    d = json.loads(lines[0])
    for key in (
        "metric",
        "value",
        "unit",
        "n_gpus",
        "steps",
        "warmup",
        "ms_per_step",
        "higher_is_better",
        "scaling",
        "vs_baseline",
        "dtype",
        "data",
        "config",
    ):
        assert key in d, key
    assert d["metric"] == "jacobi3d_cell_updates_per_s"
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1
    assert d["higher_is_better"] is True
    assert d["scaling"] == "weak"
    assert d["data"] == "synthetic"
    assert d["value"] > 0 and d["ms_per_step"] > 0
    assert d["config"]["model"] == "jacobi3d"


def _dump(tmp_path, name, *extra):
    d = tmp_path / name
    out = subprocess.run(
        [sys.executable, os.path.join(REPO, "bench.py"), "--backend", "torch",
         "--gpus", "1", "--per-gpu", "16", "--steps", "2", "--warmup", "1",
         "--dump-outputs", str(d), *extra],
        capture_output=True,
        text=True,
        timeout=300,
        cwd=REPO,
    )
    assert out.returncode == 0, out.stderr
    assert len([l for l in out.stdout.splitlines() if l.startswith("{")]) == 1
    return d


def test_dump_outputs_is_the_field_after_the_last_step(tmp_path):
    """--dump-outputs writes what a caller reads back after warmup+steps
    steps, as float32, identically from run to run; --full changes neither"""
    import numpy as np

    sys.path.insert(0, REPO)
    from stencil_amd.models.jacobi3d import Jacobi3D

    a = _dump(tmp_path, "a")
    b = _dump(tmp_path, "b", "--full")
    assert sorted(p.name for p in a.iterdir()) == ["temp_r0_d0.npy"]
    got = np.load(a / "temp_r0_d0.npy")
    assert got.dtype == np.float32 and got.shape == (16, 16, 16)
    np.testing.assert_array_equal(got, np.load(b / "temp_r0_d0.npy"))

    app = Jacobi3D((16, 16, 16), backend="torch", gpus=[0])
    app.realize()
    for _ in range(3):
        app.step()
    lo, hi = app.dd.local_rect(0)
    np.testing.assert_array_equal(got, app.dd.read_global(0, lo, hi, app.h))


def test_dump_outputs_samples_large_fields(monkeypatch, tmp_path):
    """a field over the budget is reduced to the same seeded cells each time"""
    import importlib

    import numpy as np

    sys.path.insert(0, REPO)
    bench = importlib.import_module("bench")
    from stencil_amd.models.jacobi3d import Jacobi3D

    app = Jacobi3D((16, 12, 10), backend="torch", gpus=[0])
    app.realize()
    app.step()
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4 * 500)
    bench.dump_outputs(app, str(tmp_path / "a"), 0, 1)
    bench.dump_outputs(app, str(tmp_path / "b"), 0, 1)
    got = np.load(tmp_path / "a" / "temp_r0_d0.npy")
    assert got.dtype == np.float32 and got.shape == (500,)
    np.testing.assert_array_equal(got, np.load(tmp_path / "b" / "temp_r0_d0.npy"))
    lo, hi = app.dd.local_rect(0)
    full = app.dd.read_global(0, lo, hi, app.h).reshape(-1)
    assert np.isin(got, full).all()


def test_weak_dims():
    sys.path.insert(0, REPO)
    import importlib

    bench = importlib.import_module("bench")
    for n, want in [(1, [1, 1, 1]), (2, [2, 1, 1]), (4, [2, 2, 1]), (8, [2, 2, 2]), (6, [3, 2, 1])]:
        assert bench.weak_dims(n) == want, n
