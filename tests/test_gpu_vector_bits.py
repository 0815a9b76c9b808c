"""The bits of the vector operations (csrc/src/vector_ops.hip) pinned across
changes of their kernels and of the reduction path.

The other suites compare the reductions on random data against a bound, or
against themselves; tests/golden/vector_ops_bits.json holds what the commit
named in its "commit" entry computed on an MI355X for seeded normal fields:
every reduction value as float.hex(), every written field as the SHA-256 of
its bytes. Equality, no tolerance. The launch shape is part of what is
pinned: the partials are summed per block, so another grid gives other bits.

To record the file again (only where a change of the bits is intended):
    python tests/test_gpu_vector_bits.py <commit> <out.json>
"""
import hashlib
import json
import sys
from pathlib import Path

import numpy as np
import pytest

GOLDEN = Path(__file__).resolve().parent / "golden" / "vector_ops_bits.json"

ALPHA, BETA, GAMMA, SHIFT = 0.37, -1.25, 0.3, 0.1  # 0.37, 0.3, 0.1: rounded to fp32 once

# name: (size, box lo, box hi). The strips walk with head 3 (fp32) / 1 (fp64),
# tail 3 and three z chunks; a row wider than one 64-lane block; several
# blocks in x, y and z with head 0; the linearised walk (narrower than 8).
CASES = {
    "19x5x65-x1": ((19, 5, 65), (1, 0, 0), (19, 5, 65)),
    "261x5x3": ((261, 5, 3), (0, 0, 0), (261, 5, 3)),
    "61x19x37": ((61, 19, 37), (0, 0, 0), (61, 19, 37)),
    "thin-5,2,1": ((19, 10, 9), (5, 2, 1), (12, 9, 7)),
}
DTYPES = {"f32": np.float32, "f64": np.float64}


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def values(case, dt, backend="native"):
    """{name: float.hex() strings or a SHA-256} of one case and dtype"""
    from stencil_amd import Next

    import cg_util as cu
    import stencil_util as su

    size, lo, hi = CASES[case]
    dtype, box = DTYPES[dt], (lo, hi)
    dd, (x, p, r, d, o) = cu.vector_domain(size, [dtype] * 5, backend, [0])
    seeds = ((x, 1), (p, 2), (r, 3), (d, 5), (o, 6))
    fields = {h: su.normal_global(size, dtype, seed=s) for h, s in seeds}

    def fill():
        for h, g in fields.items():
            su.scatter(dd, h, g)
        su.scatter(dd, p, su.normal_global(size, dtype, seed=4), to_next=True)

    def written(h):
        dd.backend.sync_compute()
        return _sha(su.gather(dd, h))

    fill()
    out = {
        "dot": [dd.dot(x, Next(p), where=box).hex()],
        "dot_sums": [v.hex() for v in dd.dot_sums(x, Next(p), where=box)],
        "sum": [dd.sum(r, where=box).hex()],
    }
    dd.axpby(ALPHA, x, BETA, r, out=o, where=box)
    out["axpby"] = written(o)
    dd.axpbyc(ALPHA, x, BETA, r, SHIFT, out=o, where=box)
    out["axpbyc"] = written(o)
    dd.axpbypcz(ALPHA, x, BETA, r, GAMMA, Next(p), out=o, where=box)
    out["axpbypcz"] = written(o)
    dd.scaled_update(ALPHA, x, d, BETA, r, GAMMA, Next(p), out=o, where=box)
    out["scaled_update"] = written(o)
    (rr,) = dd.backend.cg_update([box], ALPHA, x.index, p.index, r.index)
    out["cg_update"] = [rr.hex()]
    out["cg_update_x"], out["cg_update_r"] = written(x), written(r)
    fill()
    (rs,) = dd.backend.cg_update_sum([box], ALPHA, x.index, p.index, r.index)
    out["cg_update_sum"] = [v.hex() for v in rs]
    out["cg_update_sum_x"], out["cg_update_sum_r"] = written(x), written(r)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("case", sorted(CASES))
def test_vector_ops_keep_their_bits(case, dt):
    want = json.loads(GOLDEN.read_text())["values"][f"{case}-{dt}"]
    got = values(case, dt)
    assert sorted(got) == sorted(want)
    differ = {k: (got[k], want[k]) for k in got if got[k] != want[k]}
    assert not differ, differ


if __name__ == "__main__":
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
    commit, path = sys.argv[1:]
    vals = {f"{c}-{t}": values(c, t) for c in sorted(CASES) for t in sorted(DTYPES)}
    Path(path).write_text(json.dumps({"commit": commit, "values": vals}, indent=1, sort_keys=True) + "\n")
