"""Shared helpers of the generic stencil operator tests
(test_stencil_cpu.py, test_gpu_stencil.py): the stencils under test, the
two oracles and the scatter/gather of global arrays.

Oracle 1 (exact): the field is util.ripple (integers <= 753), the weights
are multiples of 1/4 with |w| <= 4 and there are at most 125 taps, so every
partial sum is an integer multiple of 1/4 below 2^24 * (1/4): exact in fp32
and fp64 in any summation order, with or without FMA. Compared bitwise.

Oracle 2 (bounded): seeded normal fields and arbitrary weights, reference
summed in float64 (longdouble for fp64 runs); pointwise
    |got - ref| <= (ntaps + 2) * eps_T * sum_k |w_k| * |v_k|,
the dot-product rounding bound (one rounding per weight, one per product,
ntaps - 1 adds). Derived, not measured.
"""
import numpy as np

import stencil_amd as sa

from util import ripple_block


# ---- stencils ----
def exact_star(r):
    """star of radius r on every axis: distinct dyadic weights, centre tap"""
    axes = []
    for a in range(3):
        ws = []
        for j in range(-r, r + 1):
            if j == 0:
                ws.append(-0.75 if a == 0 else 0.0)
            else:
                mag = (1 + (a * 9 + j + 4) % 15) / 4.0  # 0.25 .. 3.75
                ws.append(mag if (j + a) % 2 else -mag)
        axes.append(ws)
    return sa.Stencil.star(*axes)


def exact_box3():
    """27-point box, dyadic weights, none zero"""
    k = np.empty((3, 3, 3))
    for i in range(27):
        w = ((i * 7) % 17 - 8) / 4.0
        k.flat[i] = w if w != 0 else 0.25
    return sa.Stencil.from_array(k, (1, 1, 1))


def exact_asym_box():
    """5 x 3 x 1 box reaching x in [-1, 3], y in [-2, 0], z = 0"""
    k = np.empty((1, 3, 5))
    for i in range(15):
        w = ((i * 5) % 13 - 6) / 4.0
        k.flat[i] = w if w != 0 else -0.5
    return sa.Stencil.from_array(k, (1, 2, 0))


UPWIND_OFFSETS = [(0, 0, 0), (-1, 0, 0), (-2, 0, 0), (0, 1, 0)]


def upwind():
    """second-order upwind in x plus one +y tap: a star with no +x, -y or z reach"""
    return sa.Stencil(UPWIND_OFFSETS, [1.5, -2.0, 0.5, 0.25])


def upwind_x():
    """upwind in x only"""
    return sa.Stencil(UPWIND_OFFSETS[:3], [1.5, -2.0, 0.5])


# ---- fields ----
def ripple_global(size, dtype):
    return ripple_block((0, 0, 0), size, size).astype(dtype)


def normal_global(size, dtype, seed=1234):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((size[2], size[1], size[0])).astype(dtype)


# ---- oracles (periodic global arrays, (z, y, x)) ----
def _wide(dtype):
    return np.longdouble if np.dtype(dtype) == np.float64 else np.float64


def roll_sum(g, stencil):
    """(sum_k w_k g(p + o_k), sum_k |w_k| |g(p + o_k)|) over the periodic
    global array, in the wide type of g's dtype"""
    wide = _wide(g.dtype)
    gw = g.astype(wide)
    ref = np.zeros(g.shape, dtype=wide)
    mag = np.zeros(g.shape, dtype=wide)
    for (dx, dy, dz), w in zip(stencil.offsets, stencil.weights):
        v = np.roll(gw, shift=(-dz, -dy, -dx), axis=(0, 1, 2))
        ref += wide(w) * v
        mag += abs(wide(w)) * np.abs(v)
    return ref, mag


def exact_oracle(g, stencil):
    ref, _ = roll_sum(g, stencil)
    out = ref.astype(g.dtype)
    assert np.array_equal(out.astype(ref.dtype), ref)  # the data really is exact
    return out


def bound_of(stencil, mag, dtype):
    return (stencil.ntaps + 2) * np.finfo(dtype).eps * mag


def assert_within_bound(got, ref, bound, what=""):
    err = np.abs(got.astype(ref.dtype) - ref)
    worst = float(np.max(err - bound))
    print(f"{what} max err {float(err.max()):.3e} max bound {float(bound.max()):.3e}")
    assert np.isfinite(got).all(), f"{what}: non-finite output"
    assert worst <= 0, f"{what}: error exceeds the bound by {worst:.3e}"


def correlate_padded(padded, radius, size, stencil):
    """stencil applied to the interior of a padded global array (pad widths
    = the face radii), in the wide type"""
    wide = _wide(padded.dtype)
    pw = padded.astype(wide)
    off = (radius.x(-1), radius.y(-1), radius.z(-1))
    ref = np.zeros((size[2], size[1], size[0]), dtype=wide)
    for (dx, dy, dz), w in zip(stencil.offsets, stencil.weights):
        ref += wide(w) * pw[
            off[2] + dz : off[2] + dz + size[2],
            off[1] + dy : off[1] + dy + size[1],
            off[0] + dx : off[0] + dx + size[0],
        ]
    return ref


# ---- domains ----
def make_domain(size, radius, dtypes, backend, gpus, boundary=None):
    dd = sa.DistributedDomain(*size, backend=backend)
    dd.set_radius(radius)
    dd.set_gpus(gpus)
    hs = [dd.add_data(dt, f"q{i}") for i, dt in enumerate(dtypes)]
    if boundary:
        for face, (kind, value) in boundary.items():
            dd.set_boundary(face, kind, value)
    dd.realize()
    return dd, hs


def scatter(dd, h, g, to_next=False):
    """write each local domain's part of the global array g"""
    for li in range(dd.num_local()):
        lo, hi = dd.local_rect(li)
        block = np.ascontiguousarray(g[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]]).astype(h.dtype)
        dd.write_global(li, lo, block, h, to_next=to_next)


def gather(dd, h, from_next=False):
    """global array assembled from the local domains' interiors (one
    process holds every domain)"""
    out = np.empty((dd.size[2], dd.size[1], dd.size[0]), dtype=h.dtype)
    for li in range(dd.num_local()):
        lo, hi = dd.local_rect(li)
        out[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]] = dd.read_global(li, lo, hi, h, from_next)
    return out


def apply_once(dd, stencil, src, dst=None, where="all"):
    """exchange, apply, sync; the result is gather(..., from_next=True)"""
    dd.exchange()
    dd.apply_stencil(stencil, src, dst, where=where)
    dd.backend.sync_compute()
