"""The address table of the gathered load of jacobi_kernel_fuse2
(csrc/include/stencil_amd/jacobi_fuse2_map.hpp) is integer logic shared by
host and device, so it is checked here without a GPU, over every wave of the
grid: each of the 64 lanes holds the offset of a TRUE cell of the plane (so no
lane, the repeating ones included, can address outside the allocation), and
lane 2 j + side holds quantity j (+x, -x, +y, -y, self) of the periodic
neighbourhood of the cell left (side 0) or right (side 1) of the wave's tile."""
import pytest

from stencil_amd import _C

NY = 8          # rows of a block, NY - 2 of them stored
TILE = 64       # vectors of a block

# (x, y, z) of the GPU tests of the fused kernel, and the benchmark's 750^3
SHAPES = [(8, 4, 3), (9, 5, 33), (11, 7, 3), (24, 5, 33), (19, 10, 9), (40, 7, 9), (40, 25, 9),
          (249, 4, 3), (252, 7, 3), (255, 4, 3), (256, 5, 3), (257, 13, 66), (750, 750, 750)]


def _rows(size, under):
    X, Y, _ = size
    over = (4 - ((X + under) & 3)) & 3
    body4 = (X + under + over) // 4
    last = under + X - 1
    return body4, last


@pytest.mark.parametrize("under", [0, 1, 2, 3])
@pytest.mark.parametrize("size", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gather_table(size, under):
    X, Y, _ = size
    body4, last = _rows(size, under)
    pitch = (body4 * 16 + 255) // 256 * 256
    for ub in range(0, body4, TILE):
        # true x of the cells just outside the tile, periodic
        x_first = max(ub * 4 - under, 0)
        x_end = min((ub + TILE) * 4 - under, X)
        edges = ((x_first - 1) % X, x_end % X)
        for by in range((Y + NY - 3) // (NY - 2)):
            for ry in range(NY):
                yb = by * (NY - 2) - 1 + ry
                off = _C.jacobi_fuse2_gather_offsets(ub, body4, under, last, yb, Y, pitch)
                assert len(off) == 64
                yo = yb % Y
                want = []
                for j in range(5):
                    for side in (0, 1):
                        xe = edges[side]
                        x, y = [((xe + 1) % X, yo), ((xe - 1) % X, yo), (xe, (yo + 1) % Y),
                                (xe, (yo - 1) % Y), (xe, yo)][j]
                        want.append(y * pitch + (x + under) * 4)
                want += [want[-1]] * (64 - len(want))
                assert list(off) == want, f"{size} under={under} ub={ub} yb={yb}"
                for o in off:
                    y, xb = divmod(o, pitch)
                    assert o % 4 == 0 and 0 <= y < Y and under * 4 <= xb <= last * 4
                    assert o < Y * pitch  # below one plane stride
