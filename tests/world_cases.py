"""Raw grids and edits for the map-update tests on the CPU and on the GPU."""
import numpy as np

# (inflation_dist, potential_dist, potential_pow) at 0.3 m voxels: the shipped setting (radii 1, 1, 5), no potential field (rn2 = 0),
# the widest one the byte-sized distance field takes (rn2 = 9), a wider inflation (2, 2, 4), no inflation (0, 0, 3)
SETTINGS = [(0.3, 1.5, 4), (0.3, 0.0, 1), (0.3, 2.6, 4), (0.6, 1.2, 2), (0.0, 0.9, 1)]


def random_raw(rng, shape, p_occ=0.01, p_unk=0.02):
    """A raw grid (-1, 0, 100) with pillars, scattered occupied and unknown voxels and an unexplored corner that reaches the border."""
    nz, ny, nx = shape
    g = np.zeros(shape, np.int8)
    for _ in range(int(rng.integers(3, 12))):
        g[: int(rng.integers(1, nz + 1)), int(rng.integers(0, ny)), int(rng.integers(0, nx))] = 100
    g[rng.random(shape) < p_occ] = 100
    g[(rng.random(shape) < p_unk) & (g == 0)] = -1
    corner = g[:, : ny // 4, : nx // 5]
    corner[corner == 0] = -1
    return g


def random_edit(rng, raw, lo, bdim):
    """raw with the box redrawn: occupied, free and unknown voxels in random proportions (so edits add and remove all three)."""
    out = raw.copy()
    p = rng.dirichlet([1.0, 1.0, 1.0])
    out[lo[2]:lo[2] + bdim[2], lo[1]:lo[1] + bdim[1], lo[0]:lo[0] + bdim[0]] = rng.choice(np.array([100, 0, -1], np.int8), size=bdim[::-1], p=p)
    return out
