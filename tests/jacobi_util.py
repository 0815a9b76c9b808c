"""NumPy oracle of the Jacobi kernels (csrc/src/jacobi.hip), bit for bit.

The kernels compute, per cell and entirely in float32,
    (((((+x + -x) + +y) + -y) + +z) + -z) / 6
and then override the cells of the hot and the cold sphere. Every step of
that has exactly one correctly rounded result:
- the sum holds no multiply, so no FMA contraction can change it, and the
  extension is built without fast-math;
- the division is IEEE (correctly rounded), denormals are kept;
- the sphere test truncates the float32 square root of an integer below
  2^24, which is exact or correctly rounded.
So the comparison is `view(np.uint32)` equality and no tolerance applies.

Nothing here imports the torch backend: test_jacobi_oracle_cpu.py checks
that backend against this file, not the other way round.

The field is seeded and made of multiples of 2^-20 in [0.25, 1): distinct
looking values, no denormals, unlike util.ripple not separable and not
periodic, so a swapped or shifted neighbour changes the result.
"""
import numpy as np

from stencil_amd import Boundary

SENTINEL = np.float32(-99.0)  # outside [0, 1]: no Jacobi output equals it


def random_field(shape, seed):
    """(z, y, x) float32 array of k / 2^20, k in [2^18, 2^20)"""
    rng = np.random.default_rng(seed)
    return (rng.integers(2**18, 2**20, size=shape) / 2**20).astype(np.float32)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_bitwise(got, want, what=""):
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, f"{what}: shape {g.shape} != {w.shape}"
    if not np.array_equal(g, w):
        bad = np.argwhere(g != w)
        i = tuple(bad[0])
        raise AssertionError(
            f"{what}: {len(bad)} of {g.size} cells differ; first at (z,y,x)={i} "
            f"got {np.asarray(got)[i]!r} want {np.asarray(want)[i]!r}"
        )


def sphere_masks(lo, hi, c_lo, c_hi):
    """(hot, cold) boolean (z, y, x) masks over the box [lo, hi) of the
    compute region [c_lo, c_hi)"""
    cw = c_hi[0] - c_lo[0]
    hot_x, cold_x = c_lo[0] + cw // 3, c_lo[0] + 2 * cw // 3
    cy, cz = (c_lo[1] + c_hi[1]) // 2, (c_lo[2] + c_hi[2]) // 2
    r = cw // 10
    zz = np.arange(lo[2], hi[2], dtype=np.int64).reshape(-1, 1, 1)
    yy = np.arange(lo[1], hi[1], dtype=np.int64).reshape(1, -1, 1)
    xx = np.arange(lo[0], hi[0], dtype=np.int64).reshape(1, 1, -1)

    def inside(cx):
        d2 = (xx - cx) ** 2 + (yy - cy) ** 2 + (zz - cz) ** 2
        assert d2.size == 0 or d2.max() < 2**24  # the float32 conversion below is exact
        return np.sqrt(d2.astype(np.float32)).astype(np.int64) <= r

    hot, cold = inside(hot_x), inside(cold_x)
    assert not (hot & cold).any(), "hot and cold spheres overlap"
    return hot, cold


def jacobi_cells(padded, lo, hi, c_lo, c_hi):
    """one Jacobi step over the box [lo, hi) (global coords). `padded` is a
    (z, y, x) float32 array holding the box plus a 1-cell apron."""
    ez, ey, ex = hi[2] - lo[2], hi[1] - lo[1], hi[0] - lo[0]
    assert padded.dtype == np.float32 and padded.shape == (ez + 2, ey + 2, ex + 2)

    def sh(dx, dy, dz):
        return padded[1 + dz : 1 + dz + ez, 1 + dy : 1 + dy + ey, 1 + dx : 1 + dx + ex]

    s = sh(1, 0, 0) + sh(-1, 0, 0)
    for d in ((0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)):
        s = s + sh(*d)
        assert s.dtype == np.float32
    out = s / np.float32(6)
    assert out.dtype == np.float32
    hot, cold = sphere_masks(lo, hi, c_lo, c_hi)
    out[hot] = np.float32(1.0)
    out[cold] = np.float32(0.0)
    return out


def wrap_pad(g):
    return np.pad(g, 1, mode="wrap")


def walls_pad(kinds):
    """pad function for `jacobi_global` with walls: `kinds` maps faces
    ("x-" .. "z+") to (Boundary, value); axes without an entry are
    periodic. Axis by axis in the order x, y, z, each pass over the extent
    the earlier passes produced (as boundary_util.padded_global)."""

    def pad(g):
        for a, name in enumerate("xyz"):
            ax = 2 - a
            if name + "-" not in kinds and name + "+" not in kinds:
                pw = [(0, 0)] * 3
                pw[ax] = (1, 1)
                g = np.pad(g, pw, mode="wrap")
                continue
            for side in (0, 1):
                kind, value = kinds[name + "-+"[side]]
                pw = [(0, 0)] * 3
                pw[ax] = (1, 0) if side == 0 else (0, 1)
                if kind == Boundary.FIXED:
                    g = np.pad(g, pw, mode="constant", constant_values=np.float32(value))
                elif kind == Boundary.MIRROR:
                    g = np.pad(g, pw, mode="symmetric")
                else:
                    raise AssertionError(kind)
        return g

    return pad


def jacobi_global(g, steps, pad=wrap_pad):
    """`steps` whole-grid Jacobi steps on the global (z, y, x) array g"""
    size = (g.shape[2], g.shape[1], g.shape[0])
    g = np.ascontiguousarray(g, dtype=np.float32)
    for _ in range(steps):
        g = jacobi_cells(pad(g), (0, 0, 0), size, (0, 0, 0), size)
    return g


def scatter(dd, h, g, to_next=False):
    """write every local domain's part of the global array"""
    for li in range(dd.num_local()):
        lo, hi = dd.local_rect(li)
        dd.write_global(li, lo, np.ascontiguousarray(g[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]]),
                        h, to_next=to_next)


def assert_rects_equal(dd, h, want, what=""):
    """every local rect equals its part of the global array, bitwise"""
    for li in range(dd.num_local()):
        lo, hi = dd.local_rect(li)
        got = dd.read_global(li, lo, hi, h)
        assert_bitwise(got, want[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]],
                       f"{what} domain {li} rect {lo}..{hi}")
