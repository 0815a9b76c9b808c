"""Oracle for the non-periodic boundary tests: the global ripple array
padded one axis at a time in the order x, y, z with numpy.pad, compared
bitwise against every local domain's full region (halos included)."""
import numpy as np

from stencil_amd import Boundary

from util import full_region_of, ripple_block

FIXED_VALUE = -7.25  # outside the ripple range (111..753 times the scale)
SENTINEL = -99.0  # OPEN cells must keep it

ALL_FACES = ("x-", "x+", "y-", "y+", "z-", "z+")


def all_faces(kind, value=0):
    return {f: (kind, value) for f in ALL_FACES}


MIXED = {  # x periodic, y- FIXED, y+ CLAMP, z ANTIMIRROR
    "y-": (Boundary.FIXED, FIXED_VALUE),
    "y+": (Boundary.CLAMP, 0),
    "z-": (Boundary.ANTIMIRROR, 0),
    "z+": (Boundary.ANTIMIRROR, 0),
}


def apply_boundary(dd, kinds, quantities=None):
    for face, (kind, value) in kinds.items():
        dd.set_boundary(face, kind, value, quantities)


def field(lo, hi, size, scale, dtype):
    """the test field over [lo, hi): ripple for floats (all positive and
    non-zero, so ANTIMIRROR is distinguishable); folded into 1..200 for
    integer quantities so a 1-byte element holds it"""
    base = ripple_block(lo, hi, size, scale)
    dtype = np.dtype(dtype)
    if dtype.kind == "f":
        return base.astype(dtype)
    return (base.astype(np.int64) % 200 + 1).astype(dtype)


def fill(dd, handle, scale=1.0):
    for li in range(dd.num_local()):
        lo, hi = dd.local_rect(li)
        dd.write_global(li, lo, field(lo, hi, dd.size, scale, handle.dtype), handle)


def write_sentinel(dd, handle, value=SENTINEL):
    for li in range(dd.num_local()):
        flo, fhi = full_region_of(dd, li)
        shape = (fhi[2] - flo[2], fhi[1] - flo[1], fhi[0] - flo[0])
        dd.write_global(li, flo, np.full(shape, value, dtype=handle.dtype), handle)


def padded_global(size, radius, kinds, scale=1.0, dtype=np.float32, open_value=SENTINEL):
    """global array padded axis by axis (x, y, z), each pass over the full
    extent the earlier passes produced. An axis without an entry in `kinds`
    is periodic (`wrap`, both sides in one call: a second wrap call would
    wrap the first call's padding). Non-periodic lo and hi sides are padded
    in separate calls. OPEN cells hold `open_value`."""
    g = field((0, 0, 0), size, size, scale, dtype)
    faces = (radius.x, radius.y, radius.z)
    for a in range(3):
        ax = 2 - a  # arrays are (z, y, x)
        rlo, rhi = faces[a](-1), faces[a](1)
        name = "xyz"[a]
        if name + "-" not in kinds and name + "+" not in kinds:
            pw = [(0, 0)] * 3
            pw[ax] = (rlo, rhi)
            g = np.pad(g, pw, mode="wrap")
            continue
        for side, r in ((0, rlo), (1, rhi)):
            kind, value = kinds[name + "-+"[side]]
            pw = [(0, 0)] * 3
            pw[ax] = (r, 0) if side == 0 else (0, r)
            n = g.shape[ax]
            if kind == Boundary.FIXED:
                g = np.pad(g, pw, mode="constant", constant_values=np.array(value, dtype=dtype))
            elif kind == Boundary.OPEN:
                g = np.pad(g, pw, mode="constant", constant_values=np.array(open_value, dtype=dtype))
            elif kind == Boundary.CLAMP:
                g = np.pad(g, pw, mode="edge")
            elif kind in (Boundary.MIRROR, Boundary.ANTIMIRROR):
                g = np.pad(g, pw, mode="symmetric")
                if kind == Boundary.ANTIMIRROR:
                    sl = [slice(None)] * 3
                    sl[ax] = slice(0, r) if side == 0 else slice(n, n + r)
                    g[tuple(sl)] = -g[tuple(sl)]
            else:
                raise AssertionError(kind)
    return g


def check_boundary_regions(dd, handle, kinds, scale=1.0, open_value=SENTINEL, want=None):
    """every cell of every local domain's full region equals the padded
    global array, bitwise"""
    r = dd.radius
    if want is None:
        want = padded_global(dd.size, r, kinds, scale, handle.dtype, open_value)
    off = (r.x(-1), r.y(-1), r.z(-1))
    for li in range(dd.num_local()):
        flo, fhi = full_region_of(dd, li)
        got = dd.read_global(li, flo, fhi, handle)
        w = want[
            flo[2] + off[2] : fhi[2] + off[2],
            flo[1] + off[1] : fhi[1] + off[1],
            flo[0] + off[0] : fhi[0] + off[0],
        ]
        if not np.array_equal(got, w):
            bad = np.argwhere(got != w)
            i = tuple(bad[0])
            raise AssertionError(
                f"domain {li}: {len(bad)} mismatches; first at (z,y,x)={i} "
                f"got {got[i]} want {w[i]} (full region {flo}..{fhi})"
            )
    return want
