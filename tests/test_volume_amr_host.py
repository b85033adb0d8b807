"""AMR volumes without a device: the numpy checker (tests/volume_amr_checker.py) against the plain checker on exactly refined fields, its
merged macro-cell ranges against a brute-force loop over every vertex, and the scene helpers (scenes.refine, subgrid_from_geometry,
split_amr_volume)."""
import os

import numpy as np
import pytest

from gravit_amd import scenes
from gravit_amd.adapter import TransferFunction
from gravit_amd.layouts import RAY_DTYPE
from tests import volume_amr_cases as cases
from tests import volume_amr_checker as ac
from tests import volume_checker as vc
from tests.conftest import GOLDEN

F = np.float32
CMAPS = os.path.join(GOLDEN, "colormaps")
IDENT = scenes.mat_translate_scale((0, 0, 0), (1, 1, 1))


def read(name, width):
    return TransferFunction.read_map(os.path.join(CMAPS, name), width)


def rays_through(vol, n=500, seed=9):
    rng = np.random.default_rng(seed)
    lo = np.asarray(vol.origin, F)
    ext = ((vol.counts - 1).astype(F) * np.asarray(vol.spacing, F)).astype(F)
    r = np.zeros(n, RAY_DTYPE)
    o = lo + ext * (rng.random((n, 3)) * 1.6 - 0.3)
    o[: n // 2, 2] = lo[2] + ext[2] + 0.4
    r["origin"] = o.astype(F)
    r["direction"] = (lo + ext * rng.random((n, 3)) - o).astype(F)
    r["t_min"] = F(1e-6)
    r["t_max"] = np.finfo(F).max
    r["id"] = np.arange(n)
    return r


def same_bits(a, b, fields=("color", "w", "t_min", "depth")):
    for f in fields:
        assert (np.ascontiguousarray(a[f]).view(np.uint32) == np.ascontiguousarray(b[f]).view(np.uint32)).all(), f


@pytest.mark.parametrize("which", ["r2", "r8", "nested"])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_exact_refinement_gives_the_plain_bits(axis, which):
    """v = the vertex index along one axis, refined exactly (v = i + j / R): every lerp of the fine cell rounds as the coarse cell's."""
    vol = cases.exact_scene(axis, which)
    t = TransferFunction(read("CoolWarm.cmap", 4), read("ramp.omap", 2), (0.0, 20.0))
    rays = rays_through(vol)
    counts = {}
    got = ac.march(ac.AmrBrick(vol, t, 1.3), rays, IDENT, counts)
    plain = scenes.VolumeData(vol.data, vol.origin, vol.spacing)
    same_bits(got, vc.march(vc.Brick(plain, t, 1.3), rays, IDENT))
    assert 0 < counts["refined"] < counts["marched"] and (got["w"] > 0).any()


def test_without_subgrids_the_checker_is_the_plain_one():
    vol = cases.level0()
    t = TransferFunction(read("CoolWarm.cmap", 4), read("CoolWarm.omap", 2), (0.0, 1.0))
    rays = rays_through(vol)
    same_bits(ac.march(ac.AmrBrick(vol, t, 2.6), rays, IDENT), vc.march(vc.Brick(vol, t, 2.6), rays, IDENT))


def brute_ranges(vol):
    """Every vertex of every grid, one at a time: its position in level-0 cells (an exact fraction) and the macro cells whose closed box
    holds it."""
    nx, ny, nz = (int(c) for c in vol.counts)
    nb = [(c - 1 + 7) // 8 for c in (nx, ny, nz)]
    mn = np.full((nb[2], nb[1], nb[0]), np.inf, F)
    mx = np.full((nb[2], nb[1], nb[0]), -np.inf, F)
    wild = np.zeros((nb[2], nb[1], nb[0]), bool)
    geo = []  # per subgrid: (total ratio, vertex 0 in 1 / ratio of a level-0 cell)
    for s in vol.subgrids:
        r, p = (1, np.zeros(3, np.int64)) if s.parent < 0 else geo[s.parent]
        geo.append((r * s.ratio, (p + np.asarray(s.lo, np.int64)) * s.ratio))
    for r, p, data in [(1, np.zeros(3, np.int64), vol.data)] + [(g[0], g[1], s.data) for g, s in zip(geo, vol.subgrids)]:
        for (k, j, i), v in np.ndenumerate(data):
            pos = (p + np.array([i, j, k])) / r  # level-0 cells, exact in double
            cells = []
            for a, n in enumerate((nx, ny, nz)):
                cells.append([m for m in range(nb[a]) if 8 * m <= pos[a] <= min(8 * m + 8, n - 1)])
            for bz in cells[2]:
                for by in cells[1]:
                    for bx in cells[0]:
                        if np.isnan(v):
                            wild[bz, by, bx] = True
                            continue
                        mn[bz, by, bx] = min(mn[bz, by, bx], v)
                        mx[bz, by, bx] = max(mx[bz, by, bx], v)
                        wild[bz, by, bx] |= bool(np.isinf(v))
    return mn, mx, wild


def test_merged_ranges_equal_a_loop_over_every_vertex():
    vol = cases.scene()
    vol.subgrids[0].data[3, 4, 5] = np.nan      # S0, macro cell (0, 0, 0)
    vol.subgrids[1].data[-1, -1, -1] = np.inf   # S1, inside S0
    vol.subgrids[3].data[8, 8, 8] = 7.5         # S3: the maximum, in the last macro cell
    vol.subgrids[0].data[14, 0, 10] = -3.0      # S0's vertex ON the macro-cell planes x = 8 and z = 8: counts on both sides
    t = TransferFunction(read("CoolWarm.cmap", 4), read("fivespikes.omap", 2), (0.0, 1.0))
    B = ac.AmrBrick(vol, t, 1.0)
    mn, mx, wild = ac.ranges(B)
    bmn, bmx, bwild = brute_ranges(vol)
    assert (mn == bmn).all() and (mx == bmx).all() and (wild == bwild).all()
    assert mn.shape == (3, 3, 3) and wild[0, 0, 0] and mx[2, 2, 2] == F(7.5)
    assert (mn[0:2, 0, 0:2] == F(-3.0)).all() and mn[0, 1, 0] > F(-3.0)
    # the subgrids change ranges: without them the level-0 ranges differ in the cells S0 touches
    pm = ac.ranges(ac.AmrBrick(cases.level0(), t, 1.0))
    assert (pm[0][0, 0, 0] != mn[0, 0, 0]) and (pm[0][2, 2, 0] == mn[2, 2, 0])
    info = ac.info(B)
    assert info["value_min"] == F(-3.0) and info["value_max"] == np.inf and info["n_blocks"] == 27


def test_subgrid_from_geometry():
    po, ps = np.array([-0.25, 0.1, -0.4]), np.array([0.05, 0.055, 0.045])
    for ratio in (2, 4, 8):
        lo, cells = np.array([3, 0, 7]), np.array([6, 5, 1])
        r, glo, gcells = scenes.subgrid_from_geometry(po, ps, po + lo * ps, ps / ratio, cells * ratio + 1)
        assert r == ratio and (glo == lo).all() and (gcells == cells).all()
    ok = (po + 3 * ps, ps / 2, [13, 11, 3])
    assert scenes.subgrid_from_geometry(po, ps, *ok)[0] == 2
    for bad in ((po + 3 * ps, ps / 3, [13, 13, 4]),                      # ratio 3
                (po + 3 * ps, ps / 16, [17, 17, 17]),                    # ratio 16
                (po + 3 * ps, ps / np.array([2, 4, 2]), [13, 13, 3]),    # not the same on every axis
                (po + 3.5 * ps, ps / 2, [13, 11, 3]),                    # vertex 0 off the parent's vertices
                (po - 1 * ps, ps / 2, [13, 11, 3]),                      # in front of the parent
                (po + 3 * ps, ps / 2, [12, 11, 3]),                      # half a parent cell
                (po + 3 * ps, ps / 2, [13, 11, 1])):                     # no cell
        with pytest.raises(ValueError):
            scenes.subgrid_from_geometry(po, ps, *bad)


def test_refine_makes_what_the_library_accepts():
    vol = cases.scene()
    assert [s.parent for s in vol.subgrids] == [-1, 0, -1, -1]
    assert vol.subgrids[0].data.shape == (19, 11, 13) and vol.subgrids[1].data.shape == (17, 13, 13) and vol.subgrids[3].data.shape == (9, 9, 9)
    assert all(s.data.dtype == F for s in vol.subgrids)
    # the prolongation: on the parent's vertices the subgrid holds the parent's values (detail 0)
    flat = cases.level0()
    i = scenes.refine(flat, (3, 2, 1), (6, 5, 9), 2, detail=0.0)
    assert np.allclose(flat.subgrids[i].data[::2, ::2, ::2], flat.data[1:11, 2:8, 3:10], atol=1e-6)
    org, sp = scenes.subgrid_geometry(flat, i)
    assert np.allclose(org, flat.origin + np.array([3, 2, 1]) * flat.spacing) and np.allclose(sp, flat.spacing / 2)
    for bad in (dict(lo=(3, 2, 1), cells=(6, 5, 9), ratio=3), dict(lo=(3, 2, 1), cells=(6, 5, 9), ratio=2),  # ratio | overlaps subgrid i
                dict(lo=(15, 2, 1), cells=(6, 5, 9), ratio=2), dict(lo=(0, 0, 0), cells=(1, 0, 1), ratio=2),  # leaves the grid | no cell
                dict(lo=(0, 0, 0), cells=(1, 1, 1), ratio=2, parent=5)):
        with pytest.raises(ValueError):
            scenes.refine(flat, **bad)
    assert len(flat.subgrids) == 1


def test_split_amr_volume_hands_every_subgrid_to_its_brick():
    vol = cases.scene()
    bricks = scenes.split_amr_volume(vol, 2, 2, 2, cuts=cases.CUTS)
    assert len(bricks) == 8
    assert [len(b.subgrids) for b in bricks] == [3, 0, 0, 0, 0, 0, 0, 1]
    b0 = bricks[0]
    assert [s.parent for s in b0.subgrids] == [-1, 0, -1]  # S0, S1 (its child, re-indexed), S2
    assert b0.subgrids[1].data is vol.subgrids[1].data and (b0.subgrids[2].lo == vol.subgrids[2].lo).all()
    assert (bricks[7].subgrids[0].lo == np.array(cases.S3["lo"])).all() and bricks[7].subgrids[0].parent == -1
    assert (bricks[7].offset == np.array([10, 9, 11])).all() and (bricks[0].counts == np.array([11, 10, 12])).all()
    # re-indexing when a brick's first subgrid is not the volume's first: S3's child in the last brick
    scenes.refine(vol, (1, 1, 1), (2, 2, 2), 2, parent=3)
    last = scenes.split_amr_volume(vol, 2, 2, 2, cuts=cases.CUTS)[7]
    assert [s.parent for s in last.subgrids] == [-1, 0] and last.subgrids[1].ratio == 2
    # the even cuts put z = 8 through S0
    with pytest.raises(ValueError, match="straddles"):
        scenes.split_amr_volume(vol, 2, 2, 2)
    with pytest.raises(ValueError):
        scenes.split_amr_volume(vol, 2, 2, 2, cuts=([0, 10, 20], [0, 9, 18], [0, 17]))
    # without cuts and without a straddling subgrid it is split_volume
    one = scenes.split_amr_volume(vol, 1, 1, 1)
    assert len(one) == 1 and len(one[0].subgrids) == 5 and [s.parent for s in one[0].subgrids] == [-1, 0, -1, -1, 3]
    plain = scenes.split_volume(vol, 2, 1, 1)
    assert all(not b.subgrids for b in plain)


def test_bricked_checker_equals_the_one_brick_checker():
    """The bricking rule on the checker alone: one lattice, one owner, the same bits however the data is cut."""
    vol = cases.scene()
    t = TransferFunction(read("CoolWarm.cmap", 4), read("CoolWarm.omap", 2), (0.0, 1.0))
    cam = scenes.Camera((0.9, 1.3, 1.6), (0.25, 0.6, 0.0), (0.0, 1.0, 0.0), float(F(35.0 * np.pi / 180.0)), 24, 18)
    whole = ac.AmrBrick(vol, t, 1.3)
    want, calls = ac.frame([whole], whole.lo[None], whole.hi[None], IDENT, cam)
    parts = scenes.split_amr_volume(vol, 2, 2, 2, cuts=cases.CUTS)
    bricks = [ac.AmrBrick(b, t, 1.3) for b in parts]
    got, calls8 = ac.frame(bricks, [b.lo for b in parts], [b.hi for b in parts], IDENT, cam)
    assert calls == 1 and calls8 > 1 and (want[..., 3] > 0).sum() > 50
    assert (got.view(np.uint32) == want.view(np.uint32)).all()
