"""The inputs the smooth-gradient tests share (no GPU here): tests/test_volume_smooth_host.py proves on the CPU that they are not vacuous
-- something is shaded, something is crossed, CENTRAL shows -- and tests/test_gpu_volume_smooth.py runs them on the device."""
import functools
import os

import numpy as np

from gravit_amd import scenes
from gravit_amd.adapter import TransferFunction
from tests import volume_smooth_checker as sm
from tests import volume_surface_checker as sc
from tests.conftest import GOLDEN

F = np.float32
CMAPS = os.path.join(GOLDEN, "colormaps")
IDENT = scenes.mat_translate_scale((0, 0, 0), (1, 1, 1))
COUNTS = (19, 14, 11)  # x y z vertices: 3 x 2 x 2 macro cells, the last one partial on every axis
RATE = 1.3
LIGHTS = [((3.0, 4.0, 5.0), (1.0, 0.9, 0.8)), ((-2.0, 1.0, 0.5), (0.2, 0.3, 0.4))]
ISO = [0.42, 0.58]
PLANE = [[0.5, 0.7, -0.4, 0.3]]
SPLITS = ((1, 1, 1), (2, 2, 2), (3, 1, 2))
THIN_X = (9, 1, 1)  # applied to a grid of 10 vertices along x: every brick is one cell thick there, both x-neighbours of a vertex are ghosts


def volume(counts=COUNTS, seed=3):
    nx, ny, nz = counts
    data = np.ascontiguousarray(scenes.noise_volume(max(counts), seed=seed).data[:nz, :ny, :nx])
    return scenes.VolumeData(data, np.array([-0.25, 0.1, -0.4], F), np.array([1.0 / 18, 1.1 / 13, 0.9 / 10], F))


def camera(w=64, h=48):
    return scenes.Camera((1.55, 1.5, 1.75), (0.25, 0.65, 0.05), (0.0, 1.0, 0.0), float(F(40.0 * np.pi / 180.0)), w, h)


def read(name, width):
    return TransferFunction.read_map(os.path.join(CMAPS, name), width)


def table(kind, hi=None):
    """dense: opacity everywhere.  spikes: fivespikes.omap, sparse (opacity at 0.9 of the table only: macro cells are skipped); its range ends
    at 0.6, which puts the spike at 0.54, near the grid's median.  hi: the value the table's top maps to."""
    if kind == "dense":
        return TransferFunction(read("CoolWarm.cmap", 4), np.array([[0, 0.02], [1, 0.3]], F), (0.0, 1.0 if hi is None else hi))
    return TransferFunction(read("Grayramp.cmap", 4), read("fivespikes.omap", 2), (0.0, 0.6 if hi is None else hi))


def lit():
    return sc.Surfaces(lights=LIGHTS)


def surfaces(lights=LIGHTS):
    return sc.Surfaces(ISO, PLANE, 0.5, lights)


SETUPS = {"lit": (lit, sm.SHADE_GRADIENT), "surfaces": (surfaces, sm.SHADE_NONE), "both": (surfaces, sm.SHADE_GRADIENT)}


def bricks_of(vol, split):
    """The bricks of a split with their ghosts; 1 x 1 x 1: the whole grid (every face on the global boundary: no layer exists)."""
    return [vol] if tuple(split) == (1, 1, 1) else scenes.split_volume(vol, *split, ghosts=True)


def box(vol):
    lo = np.asarray(vol.origin, F)
    return lo, (lo + (vol.counts - 1).astype(F) * np.asarray(vol.spacing, F)).astype(F)


def brick_rays(brick, n=600, seed=5):
    """Rays aimed through a brick from every side, a third of them starting inside it; identity instance."""
    from gravit_amd.layouts import RAY_DTYPE

    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(brick.lo, F), np.asarray(brick.hi, F)
    ext = hi - lo
    tgt = lo + ext * rng.random((n, 3))
    org = (lo + hi) / 2 + (rng.random((n, 3)) - 0.5) * (ext * 2 + 1.5)
    org[::3] = lo + ext * rng.random((len(org[::3]), 3))
    r = np.zeros(n, RAY_DTYPE)
    r["origin"] = org.astype(F)
    r["direction"] = (tgt - org).astype(F)
    r["t_min"] = F(1e-6)
    r["t_max"] = np.finfo(F).max
    r["id"] = np.arange(n)
    r["t"] = 77.0
    return r


@functools.lru_cache(maxsize=None)
def frame_want(setup, kind, table_kind="dense"):
    """The checker's frame of the whole grid as one brick: (image, shaded, crossings)."""
    vol, (S, mode) = volume(), SETUPS[setup]
    B = sm.Brick(vol, table(table_kind), RATE)
    img, _ = sm.frame([B], B.lo[None], B.hi[None], IDENT, camera(), S(), mode, kind=kind)
    img.setflags(write=False)
    return img, sm.frame.shaded, sm.frame.crossings


def nonfinite_volume():
    """tests/volume_edge_cases.py's inputs on one grid: its `mixed` non-finite vertices (NaN, +Inf, -Inf) and its `huge` pairs, whose
    differences overflow; a ramp instead of the constant 0.5, so that the finite part has a gradient."""
    from tests import volume_edge_cases as ec

    vol = ec.nonfinite("mixed")
    nx = ec.COUNTS[0]
    vol.data += (np.arange(nx, dtype=F) * F(0.02))[None, None, :]
    for (x, y, z), v in ec.HUGE_VERTS:
        vol.data[z, y, x] = v
    return vol
