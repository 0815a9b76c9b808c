"""The device division helper div6 (csrc/include/stencil_amd/device_util.hpp)
against NumPy's correctly rounded float32 division, bit for bit.

The fast form (multiply by 1/6, one fma correction) is exact for
2^-125 <= |x| <= FLT_MAX and guarded outside that, where the helper takes
the true division for the whole wave. The inputs are laid out by exponent,
so most waves are uniformly on one side of the guard and both paths run;
the special values sit together with ordinary ones in the last waves, where
the guard fails for the wave. tools/div6_exhaustive.cpp checks all 2^32
inputs of the same source on the host."""
import numpy as np
import pytest

from stencil_amd import _C

pytestmark = pytest.mark.gpu


def _inputs():
    rng = np.random.default_rng(6)
    per = 2**15  # mantissas per (sign, exponent): 2 * 256 * 2^15 = 2^24 patterns
    mant = rng.integers(0, 2**23, size=per, dtype=np.uint32)
    mant[:4] = (0, 1, 2**23 - 1, 2**22)
    exp = np.arange(256, dtype=np.uint32).reshape(-1, 1) << 23
    pos = (exp | mant.reshape(1, -1)).reshape(-1)
    special = np.array(
        [0.0, -0.0, np.inf, -np.inf, 2.0**-125, -(2.0**-125), 2.0**-149, -(2.0**-149),
         2.0**-126, np.finfo(np.float32).max, -np.finfo(np.float32).max, 0.5, 6.0, 1.0],
        dtype=np.float32).view(np.uint32)
    below = np.float32(2.0**-125).view(np.uint32) - np.uint32(1)  # largest value under the guard
    special = np.concatenate([special, [below, below | np.uint32(1 << 31)]]).astype(np.uint32)
    return np.concatenate([pos, pos | np.uint32(1 << 31), special]).view(np.float32)


def test_div6_matches_ieee_division():
    x = _inputs()
    assert x.size >= 2**24
    got = np.asarray(_C.div6_f32(x), dtype=np.float32)
    with np.errstate(all="ignore"):
        want = x / np.float32(6)
    assert want.dtype == np.float32 and got.shape == want.shape
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    g, w = got.view(np.uint32), want.view(np.uint32)
    bad = np.flatnonzero((g != w) & ~nan)
    assert bad.size == 0, (
        f"{bad.size} of {x.size} differ; first x={x[bad[0]]!r} "
        f"(0x{x.view(np.uint32)[bad[0]]:08x}) got 0x{g[bad[0]]:08x} want 0x{w[bad[0]]:08x}")
