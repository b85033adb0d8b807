"""The scenes the AMR tests share (tests/test_volume_amr_host.py, tests/test_gpu_volume_amr.py): the smallest volume that crosses every
table boundary, and exactly refined fields."""
import numpy as np

from gravit_amd import scenes
from gravit_amd.layouts import RAY_DTYPE

F = np.float32
COUNTS = (21, 19, 18)  # vertices: 20 x 18 x 17 cells = 3 x 3 x 3 macro cells, the last of every axis partial
S0 = dict(lo=(3, 2, 1), cells=(6, 5, 9), ratio=2)      # crosses the macro-cell plane at 8 on x and z
S1 = dict(lo=(2, 1, 3), cells=(3, 3, 4), ratio=4)      # child of S0 (12 x 10 x 18 cells)
S2 = dict(lo=(9, 2, 1), cells=(1, 5, 6), ratio=2)      # level 1, shares the face x = 9 with S0
S3 = dict(lo=(19, 17, 16), cells=(1, 1, 1), ratio=8)   # the brick's last cell
CUTS = ([0, 10, 20], [0, 9, 18], [0, 11, 17])          # a 2 x 2 x 2 bricking whose cuts keep clear of S0, S2 and S3


def level0(data=None):
    """21 x 19 x 18 vertices of value noise with tests.test_gpu_volume.grid's anisotropic geometry."""
    nx, ny, nz = COUNTS
    if data is None:
        data = np.ascontiguousarray(scenes.noise_volume(nx, seed=3).data[:nz, :ny, :nx])
    n = nx
    return scenes.VolumeData(data, np.array([-0.25, 0.1, -0.4], F), np.array([1.0 / (n - 1), 1.1 / (n - 1), 0.9 / (n - 1)], F))


def scene(data=None, fn=None):
    """Level 0 with S0, its child S1, S2 and S3 (indices 0..3).  fn: the subgrids' field (scenes.refine); default: prolongation + detail."""
    vol = level0(data)
    s0 = scenes.refine(vol, S0["lo"], S0["cells"], S0["ratio"], fn=fn, seed=1)
    scenes.refine(vol, S1["lo"], S1["cells"], S1["ratio"], parent=s0, fn=fn, seed=2)
    scenes.refine(vol, S2["lo"], S2["cells"], S2["ratio"], fn=fn, seed=3)
    scenes.refine(vol, S3["lo"], S3["cells"], S3["ratio"], fn=fn, seed=4)
    return vol


def exact_scene(axis, which):
    """Level 0 holds v = the vertex index along `axis` (integers) and the subgrids the exactly refined field v = i + j / R: the AMR volume
    and the plain one are the same piecewise-linear function, and every lerp of the descent's cell rounds as the level-0 cell's does.
    which: "r2" (S0 alone), "r8" (one ratio-8 subgrid), "nested" (S0 with its ratio-4 child)."""
    nx, ny, nz = COUNTS
    idx = np.arange((nx, ny, nz)[axis], dtype=F)
    shape = [1, 1, 1]
    shape[2 - axis] = len(idx)
    vol = level0(np.ascontiguousarray(np.broadcast_to(idx.reshape(shape), (nz, ny, nx)), F))
    org, sp = float(vol.origin[axis]), float(vol.spacing[axis])

    def fn(x, y, z):
        return ((x, y, z)[axis] - org) / sp  # the index coordinate: i + j / R, exact in float32 after rounding (a multiple of 1 / 64)

    def exact(i):  # (the positions carry float64 rounding of a few 1e-16: snap to the lattice of the finest level)
        s = vol.subgrids[i]
        s.data = (np.rint(s.data.astype(np.float64) * 64) / 64).astype(F)

    if which == "r8":
        exact(scenes.refine(vol, (5, 4, 3), (3, 2, 4), 8, fn=fn))
    else:
        s0 = scenes.refine(vol, S0["lo"], S0["cells"], S0["ratio"], fn=fn)
        exact(s0)
        if which == "nested":
            exact(scenes.refine(vol, S1["lo"], S1["cells"], S1["ratio"], parent=s0, fn=fn))
    return vol


def plane_rays(vol, m, n=400, seed=5):
    """Rays that run exactly IN a vertex plane of S0 (d[a] == 0 in object space, the origin on the plane): planes of level-0 vertices
    and of S0's own (half indices), through S0's box, for axis a = 0, 1, 2 in turn.  m: the instance's matrix (world = m * object)."""
    rng = np.random.default_rng(seed)
    org, sp = np.asarray(vol.origin, F), np.asarray(vol.spacing, F)
    lo = (org + np.array(S0["lo"], F) * sp).astype(F)
    ext = (np.array(S0["cells"], F) * sp).astype(F)
    o = (lo + ext * rng.random((n, 3)) + np.array([0.3, 0.4, 0.5]) * np.sign(rng.random((n, 3)) - 0.5)).astype(F)
    tgt = (lo + ext * rng.random((n, 3))).astype(F)
    a = np.arange(n) % 3
    half = rng.integers(0, 2 * np.array(S0["cells"])[a] + 1)  # S0's vertex planes along a: level-0 index lo + half / 2
    o[np.arange(n), a] = (org[a] + (np.array(S0["lo"], F)[a] + half.astype(F) / F(2)) * sp[a]).astype(F)
    d = (tgt - o).astype(F)
    d[np.arange(n), a] = 0
    M = np.asarray(m, F).reshape(4, 4).T
    r = np.zeros(n, RAY_DTYPE)
    r["origin"] = (o @ M[:3, :3].T + M[:3, 3]).astype(F)
    r["direction"] = (d @ M[:3, :3].T).astype(F)
    r["t_min"] = F(1e-6)
    r["t_max"] = np.finfo(F).max
    r["id"] = np.arange(n)
    return r
