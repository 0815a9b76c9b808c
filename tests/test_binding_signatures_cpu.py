"""The Python surface of the native ops pinned across changes of the
bindings (csrc/src/bindings.cpp).

pybind11 writes every overload's signature -- keyword names, defaults,
argument and return types -- into the function's __doc__.
tests/golden/binding_signatures.json holds {name: _C.<name>.__doc__} as the
commit named in its "commit" entry built it, for every function
stencil_amd.ops exports plus jacobi_step_kernel and the grid transfer.
Equality: a binding that loses a keyword, a default or its tuple return
type differs here.

The error contract (std::invalid_argument -> ValueError with the C++
message, through pybind11's built-in translator) is asserted by the GPU
suites for every vector op; the one std::invalid_argument a machine without
a GPU can reach, the C++ DistributedDomain's set_boundary, is checked here.

To record the file again (only where a change of the surface is intended):
    python tests/test_binding_signatures_cpu.py <commit> <out.json>
"""
import json
import sys
from pathlib import Path

import pytest

GOLDEN = Path(__file__).resolve().parent / "golden" / "binding_signatures.json"
EXTRA = ("jacobi_step_kernel", "grid_restrict", "grid_prolong_add")


def signatures():
    from stencil_amd import _C, ops

    names = [n for n in ops.__all__ if not isinstance(getattr(_C, n), type)]
    return {n: getattr(_C, n).__doc__ for n in sorted(names + list(EXTRA))}


def test_signatures_are_the_recorded_ones():
    want = json.loads(GOLDEN.read_text())["signatures"]
    got = signatures()
    assert sorted(got) == sorted(want)
    differ = {n: (got[n], want[n]) for n in got if got[n] != want[n]}
    assert not differ, differ


def test_ops_reexports_the_native_objects():
    from stencil_amd import _C, ops

    assert sorted(ops.__all__) == json.loads(GOLDEN.read_text())["exports"]
    for n in ops.__all__:
        assert getattr(ops, n) is getattr(_C, n)


def test_invalid_argument_is_a_value_error_with_the_cpp_message(monkeypatch):
    from stencil_amd import _C

    for var in ("STENCIL_RANK", "RANK", "STENCIL_WORLD", "WORLD_SIZE"):
        monkeypatch.delenv(var, raising=False)
    d = _C.CppDistributedDomain(8, 8, 8)
    d.add_data(4, "q")
    with pytest.raises(ValueError, match=r"^set_boundary: unknown face 'w-'$"):
        d.set_boundary("w-", _C.Boundary.MIRROR)
    with pytest.raises(ValueError, match=r"^set_boundary: PERIODIC applies to all quantities$"):
        d.set_boundary("x", _C.Boundary.PERIODIC, quantities=[0])
    d.set_boundary("x", _C.Boundary.MIRROR, 0.0, [0])  # the valid call still binds


if __name__ == "__main__":
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
    commit, path = sys.argv[1:]
    from stencil_amd import ops

    rec = {"commit": commit, "exports": sorted(ops.__all__), "signatures": signatures()}
    Path(path).write_text(json.dumps(rec, indent=1, sort_keys=True) + "\n")
