"""What the time-varying AMR tests share (tests/test_volume_amr_update_host.py, tests/test_gpu_volume_amr_update.py): two time steps of
tests/volume_amr_cases.py's tree, and fields designed so that only the merged ranges of the NEW step keep skipping exact."""
import functools

import numpy as np

from gravit_amd import scenes
from gravit_amd.adapter import TransferFunction
from gravit_amd.layouts import RAY_DTYPE
from tests import volume_amr_cases as cases
from tests.test_gpu_volume import read

F = np.float32
RATE = 1.3
LOW, HIGH = F(0.2), F(0.9)
# the designed fields: which subgrid holds the lone HIGH vertex in step B (its index z, y, x), and the macro cells (z, y, x) it must open
DESIGNED = {
    "s3_opens": dict(subgrid=3, vertex=(4, 4, 4), cells=[(2, 2, 2)]),               # strictly inside S3 and inside macro cell (2, 2, 2)
    "boundary": dict(subgrid=0, vertex=(3, 3, 10), cells=[(0, 0, 0), (0, 0, 1)]),   # S0's x index 10 is level-0 x = 3 + 10 / 2 = 8
}
NONFINITE = ("nan", "inf", "mix")


@functools.lru_cache(maxsize=None)
def step(k):
    """Time step A (k = 0: cases.scene()) or B (k = 1: another level-0 noise, the subgrids refined from it) of the one tree.  Read-only."""
    if k == 0:
        return cases.scene()
    nx, ny, nz = cases.COUNTS
    return cases.scene(np.ascontiguousarray(scenes.noise_volume(nx, seed=9).data[:nz, :ny, :nx]))


def with_subgrid(vol, index, data):
    """vol with subgrid `index` holding `data`: a new VolumeData on the same level-0 array and the same tree."""
    subs = list(vol.subgrids)
    s = subs[index]
    subs[index] = scenes.Subgrid(s.parent, s.ratio, s.lo, s.cells, np.ascontiguousarray(data, F))
    return scenes.VolumeData(vol.data, vol.origin, vol.spacing, subs)


def half():
    """Zero opacity below mid-range: LOW is transparent, HIGH is not."""
    return TransferFunction(read("CoolWarm.cmap", 4), np.array([[0.0, 0.0], [0.5, 0.0], [1.0, 0.8]], F), (0.0, 1.0))


def designed(which):
    """(A, B): every vertex of every level is LOW in A; B is A with ONE vertex of one subgrid at HIGH (DESIGNED[which])."""
    flat = lambda x, y, z: LOW + 0 * (x + y + z)  # noqa: E731
    a = cases.scene(np.full(cases.COUNTS[::-1], LOW, F), fn=flat)
    d = DESIGNED[which]
    data = a.subgrids[d["subgrid"]].data.copy()
    data[d["vertex"]] = HIGH
    return a, with_subgrid(a, d["subgrid"], data)


def vertex_position(vol, index, vertex):
    """Object-space position of vertex (z, y, x) of subgrid `index` (float64)."""
    org, sp = scenes.subgrid_geometry(vol, index)
    return org + np.asarray(vertex[::-1], np.float64) * sp


def aimed_rays(vol, target, n=256, seed=21):
    """Rays from around the brick through a small neighbourhood of `target` (object space, identity instance)."""
    rng = np.random.default_rng(seed)
    sp = np.asarray(vol.spacing, np.float64)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    tgt = np.asarray(target, np.float64) + (rng.random((n, 3)) - 0.5) * 0.05 * sp
    r = np.zeros(n, RAY_DTYPE)
    r["origin"] = (tgt - (2.5 + rng.random((n, 1))) * d).astype(F)  # (a random distance: the lattice t = k * dt meets the target at every phase)
    r["direction"] = d.astype(F)
    r["t_min"] = F(1e-6)
    r["t_max"] = np.finfo(F).max
    r["id"] = np.arange(n)
    return r


def nonfinite(kind):
    """Step B with not-finite vertices in S0's new samples: a NaN, a +Inf, or both and a -Inf, inside S0 and on its x = 8 plane."""
    data = step(1).subgrids[0].data.copy()
    if kind in ("nan", "mix"):
        data[5, 4, 6] = np.nan
    if kind in ("inf", "mix"):
        data[7, 6, 10] = np.inf
    if kind == "mix":
        data[12, 3, 2] = -np.inf
        data[12, 3, 3] = np.nan
    return with_subgrid(step(1), 0, data)


def changed_trees(vol):
    """{what: subgrids} -- the subgrids of vol (a VolumeData or a Brick that holds S0, S1 and S2 as entries 0..2) with one field of the
    tree changed (the data arrays are vol's own, whatever their shape)."""
    def change(i, **kw):
        subs = list(vol.subgrids)
        s = subs[i]
        f = dict(parent=s.parent, ratio=s.ratio, lo=s.lo, cells=s.cells)
        f.update(kw)
        subs[i] = scenes.Subgrid(f["parent"], f["ratio"], f["lo"], f["cells"], s.data)
        return subs

    s2, s1 = vol.subgrids[2], vol.subgrids[1]
    return {
        "lo": change(2, lo=(int(s2.lo[0]) + 1, int(s2.lo[1]), int(s2.lo[2]))),
        "cells": change(2, cells=(int(s2.cells[0]), int(s2.cells[1]) - 1, int(s2.cells[2]))),
        "ratio": change(2, ratio=4),
        "parent": change(1, parent=-1),
        "count": list(vol.subgrids[:-1]),
        "lo of a child": change(1, lo=(int(s1.lo[0]), int(s1.lo[1]), int(s1.lo[2]) + 1)),
    }
