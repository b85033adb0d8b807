"""Smooth gradients on the host (no GPU): the new entry points in the header and the binding, the numpy checker
(tests/volume_smooth_checker.py) against its parent where the kind cannot show, on fields whose gradients are known exactly, across
brickings, scenes.split_volume's ghosts, and the proof that the inputs of tests/test_gpu_volume_smooth.py are not vacuous."""
import os
import re

import numpy as np
import pytest

from gravit_amd import capi, scenes
from tests import volume_checker as vc
from tests import volume_clip_checker as cc
from tests import volume_shade_checker as lc
from tests import volume_smooth_cases as cases
from tests import volume_smooth_checker as sm
from tests.conftest import ROOT

F = np.float32
NEW = ["gvt_hip_volume_set_ghosts", "gvt_hip_volume_set_gradient", "gvt_hip_volume_get_gradient"]
ALL = ("color", "w", "t_min", "depth", "t")
IDENT = cases.IDENT


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b, fields=ALL):
    assert len(a) == len(b)
    for f in fields:
        assert (bits(a[f]) == bits(b[f])).all(), f


def test_header_declares_and_binding_lists_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "gvt_hip.h")).read()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in capi.SYMBOLS
    assert int(re.search(r"#define\s+GVT_HIP_VOLUME_GRADIENT_CELL\s+(\d+)", hdr).group(1)) == 0 == capi.VOLUME_GRADIENT_CELL == sm.CELL
    assert int(re.search(r"#define\s+GVT_HIP_VOLUME_GRADIENT_CENTRAL\s+(\d+)", hdr).group(1)) == 1 == capi.VOLUME_GRADIENT_CENTRAL == sm.CENTRAL
    assert int(re.search(r"#define GVT_HIP_ABI_VERSION (\d+)", hdr).group(1)) == 6 == capi.ABI_VERSION  # additive: the revision stays


@pytest.fixture(scope="module")
def case():
    vol = cases.volume()
    brick = cases.bricks_of(vol, (2, 2, 2))[3]
    rays = cases.brick_rays(brick, n=500)
    clipped = rays.copy()
    clipped["depth"] |= np.where(np.arange(len(rays)) % 3 != 0, cc.CLIP, 0).astype(np.int32)
    clipped["t_max"] = (np.random.default_rng(2).random(len(rays)) * 2).astype(F)
    return vol, brick, rays, clipped


def test_kind_cell_is_the_parent_checker(case):
    vol, brick, rays, clipped = case
    t = cases.table("dense")
    for part in (vol, brick):
        B, P = sm.Brick(part, t, cases.RATE), vc.Brick(part, t, cases.RATE)
        for S, mode in ((cases.lit(), sm.SHADE_GRADIENT), (cases.surfaces(), sm.SHADE_NONE), (cases.surfaces(), sm.SHADE_GRADIENT), (None, sm.SHADE_GRADIENT)):
            for r in (rays, clipped):
                want = lc.march(P, S, r, IDENT, mode)
                n_sh, n_cr = lc.march.shaded, lc.march.crossings
                same_bits(sm.march(B, S, r, IDENT, mode, sm.CELL), want, ALL + ("t_max",))
                assert (sm.march.shaded, sm.march.crossings) == (n_sh, n_cr)
    assert n_sh == 0 and n_cr == 0  # (the last one had nothing set)
    cam = cases.camera(32, 24)
    B = sm.Brick(vol, t, cases.RATE)
    a, _ = sm.frame([B], B.lo[None], B.hi[None], IDENT, cam, cases.surfaces(), kind=sm.CELL)
    b, _ = lc.frame([B], B.lo[None], B.hi[None], IDENT, cam, cases.surfaces())
    assert (bits(a) == bits(b)).all() and sm.frame.shaded == lc.frame.shaded > 0


def test_the_kind_is_inert_where_nothing_is_shaded(case):
    vol, brick, rays, _ = case
    B = sm.Brick(brick, cases.table("dense"), cases.RATE)
    same_bits(sm.march(B, None, rays, IDENT, kind=sm.CENTRAL), vc.march(B, rays, IDENT), ("color", "w", "t_min", "depth"))
    S = cases.surfaces([])  # surfaces without lights: the normal is not used
    same_bits(sm.march(B, S, rays, IDENT, kind=sm.CENTRAL), sm.march(B, S, rays, IDENT, kind=sm.CELL))
    assert sm.march.crossings > 0


def affine(counts, a, b, c):
    nx, ny, nz = counts
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return scenes.VolumeData((a * i + b * j + c * k).astype(F), np.array([-0.25, 0.1, -0.4], F), np.array([1.0 / 18, 1.1 / 13, 0.9 / 10], F))


def test_on_an_affine_field_central_equals_cell_bit_for_bit():
    """v = a i + b j + c k with small integers: every difference is exact, (2 a) / (s * 2) and a / (s * 1) are a / s in every bit, and a lerp
    of equal values returns them -- on the global boundary too, where the difference is one-sided."""
    vol = affine(cases.COUNTS, 3, -2, 5)
    t = cases.table("dense", hi=float(vol.data.max()))
    for part in [vol] + cases.bricks_of(vol, (2, 2, 2))[:3]:
        B = sm.Brick(part, t, cases.RATE)
        rays = cases.brick_rays(part if hasattr(part, "lo") else scenes.split_volume(vol, 1, 1, 1)[0], n=400)
        for S, mode in ((cases.lit(), sm.SHADE_GRADIENT), (sm.sc.Surfaces([20.5, 40.25], [], 0.5, cases.LIGHTS), sm.SHADE_GRADIENT)):
            cell = sm.march(B, S, rays, IDENT, mode, sm.CELL)
            n_cell = (sm.march.shaded, sm.march.crossings)
            same_bits(sm.march(B, S, rays, IDENT, mode, sm.CENTRAL), cell)
            assert (sm.march.shaded, sm.march.crossings) == n_cell and n_cell[0] > 500
    assert n_cell[1] > 50
    # the gradient itself, in every cell of the grid, its boundary cells included
    B = sm.Brick(vol, t, cases.RATE)
    nx, ny, nz = cases.COUNTS
    k, j, i = (x.reshape(-1) for x in np.meshgrid(np.arange(nz - 1), np.arange(ny - 1), np.arange(nx - 1), indexing="ij"))
    c = np.stack([i, j, k], axis=1)
    f = np.random.default_rng(1).random((len(c), 3), dtype=F)
    g = sm.central_gradient(B, c, f[:, 0], f[:, 1], f[:, 2])
    want = (np.array([3, -2, 5], F) / B.sp).astype(F)
    assert (bits(g) == bits(np.broadcast_to(want, g.shape))).all()


def test_on_a_parabola_central_is_continuous_where_cell_jumps():
    """v = i * i on a grid of spacing s = 1/16 (a power of two: everything below is exact).  At vertex m the central difference is
    ((m + 1)^2 - (m - 1)^2) / (2 s) = 2 m / s.  CENTRAL at f.x = 0 of cell m is that value exactly (a + 0 * (b - a) = a); just below the
    face, at f.x = 1 - e of cell m - 1, it is lerp(2 (m - 1) / s, 2 m / s, 1 - e) = 2 m / s - e * 2 / s up to the lerp's two roundings
    (each at most half an ulp of a value below 2 m / s): within e * 2 / s + 2^-23 * (2 m / s) of it.  CELL gives (2 m - 1) / s below the face
    and (2 m + 1) / s above it: a jump of exactly 2 / s.  This is what the feature is for."""
    n, s = 12, F(1.0 / 16)
    i = np.arange(n, dtype=F)
    vol = scenes.VolumeData(np.ascontiguousarray(np.broadcast_to((i * i)[None, None, :], (6, 7, n))).astype(F), np.zeros(3, F), np.full(3, s, F))
    t = cases.table("dense", hi=float(vol.data.max()))
    ms = np.arange(1, n - 1)  # the interior vertices: faces between cell m - 1 and cell m
    e = F(2.0 ** -20)
    for part, off in ((vol, 0), (scenes.split_volume(vol, 3, 1, 1, ghosts=True)[1], None)):
        B = sm.Brick(part, t, 1.0)
        off = int(B.off[0])
        m = ms[(ms - 1 >= off) & (ms <= off + int(B.n[0]) - 2)]  # both cells are the brick's
        assert len(m) >= 2
        fy, fz = np.full(len(m), 0.3, F), np.full(len(m), 0.6, F)
        above = np.stack([m - off, np.full(len(m), 2), np.full(len(m), 3)], axis=1)
        below = above - np.array([1, 0, 0])
        vertex = (F(2) * m.astype(F) / s).astype(F)
        assert (bits(sm.vertex_gradient(B, 0, above[:, 0], above[:, 1], above[:, 2])) == bits(vertex)).all()
        g_above = sm.central_gradient(B, above, np.zeros(len(m), F), fy, fz)
        g_below = sm.central_gradient(B, below, np.full(len(m), F(1) - e, F), fy, fz)
        assert (bits(g_above[:, 0]) == bits(vertex)).all() and (g_above[:, 1:] == 0).all()
        assert (np.abs(g_below[:, 0].astype(np.float64) - vertex) <= float(e) * 2 / float(s) + 2.0 ** -23 * vertex).all()

        def cell_gradient(c, fx):
            base = [B.vox[c[:, 2] + dz, c[:, 1] + dy, c[:, 0] + dx] for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)]
            return lc.gradient(B, base, fx, fy, fz)[:, 0]

        jump = cell_gradient(above, np.zeros(len(m), F)) - cell_gradient(below, np.full(len(m), F(1) - e, F))
        assert (jump == F(2) / s).all()


@pytest.mark.parametrize("split", [(2, 2, 2), (3, 1, 2), (3, 3, 3)])
def test_split_volume_fills_the_ghosts_from_the_neighbours(split):
    vol = cases.volume()
    parts = scenes.split_volume(vol, *split, ghosts=True)
    plain = scenes.split_volume(vol, *split)
    assert all(p.ghosts is None for p in plain) and len(plain) == len(parts)
    by_offset = {tuple(int(v) for v in p.offset): p for p in parts}
    n_faces = 0
    for p, q in zip(parts, plain):
        assert (p.data == q.data).all() and (p.offset == q.offset).all() and (p.lo == q.lo).all() and (p.hi == q.hi).all()  # the default output, unchanged
        off, cnt = [int(v) for v in p.offset], [int(v) for v in p.counts]
        for a in range(3):
            for side in (0, 1):
                face = p.ghosts[2 * a + side]
                outer = off[a] == 0 if side == 0 else off[a] + cnt[a] == int(vol.counts[a])
                if outer:
                    assert face is None
                    continue
                # the neighbour across that face shares the face's vertices; the ghost is its next layer
                key = list(off)
                key[a] = off[a] + cnt[a] - 1 if side else max(o[a] for o in by_offset if o[a] < off[a])
                nb = by_offset[tuple(key)]
                layer = 1 if side else int(nb.counts[a]) - 2
                want = np.take(nb.data, layer, axis=2 - a)
                assert face.dtype == vol.data.dtype and face.shape == want.shape and (face == want).all()
                n_faces += 1
    assert n_faces == 2 * sum((split[a] - 1) * split[(a + 1) % 3] * split[(a + 2) % 3] for a in range(3))
    B = sm.Brick(parts[0], cases.table("dense"), cases.RATE)
    assert B.has_required_ghosts() and not sm.Brick(plain[0], cases.table("dense"), cases.RATE).has_required_ghosts()
    G = sm.Brick(plain[-1], cases.table("dense"), cases.RATE, grid=vol)  # ... and the checker takes them from the global grid alike
    assert all((a is None and b is None) or (a == b).all() for a, b in zip(G.ghosts, sm.Brick(parts[-1], cases.table("dense"), cases.RATE).ghosts))


@pytest.mark.parametrize("setup", ["lit", "surfaces", "both"])
def test_the_checkers_frame_does_not_depend_on_the_bricking(setup):
    """... and the inputs of the GPU frames are not vacuous: something is shaded or crossed, and CENTRAL shows."""
    vol, cam, t = cases.volume(), cases.camera(), cases.table("dense")
    S, mode = cases.SETUPS[setup]
    want, shaded, crossings = cases.frame_want(setup, sm.CENTRAL)
    cell, cell_shaded, cell_crossings = cases.frame_want(setup, sm.CELL)
    assert (shaded > 0) == (setup != "surfaces") and (crossings > 0) == (setup != "lit")
    assert (shaded, crossings) == (cell_shaded, cell_crossings)  # what is shaded does not depend on the kind
    assert want.shape == (cam.height, cam.width, 4) and np.isfinite(want).all()
    differ = (bits(want[..., :3]) != bits(cell[..., :3])).any(axis=2)
    print("%s: %d shaded, %d crossings, %d of %d pixels differ between CENTRAL and CELL" % (setup, shaded, crossings, differ.sum(), differ.size))
    assert differ.sum() >= 1 and (bits(want[..., 3]) == bits(cell[..., 3])).all()  # opacity is not shaded
    for split in cases.SPLITS[1:]:
        parts = cases.bricks_of(vol, split)
        bricks = [sm.Brick(b, t, cases.RATE) for b in parts]
        assert all(b.has_required_ghosts() for b in bricks)
        got, calls = sm.frame(bricks, [b.lo for b in parts], [b.hi for b in parts], IDENT, cam, S(), mode, kind=sm.CENTRAL)
        assert calls > 1 and (sm.frame.shaded, sm.frame.crossings) == (shaded, crossings)
        assert (bits(got) == bits(want)).all(), split


def test_the_inputs_of_the_trace_tests_are_not_vacuous():
    """One brick, lit, rate 1.3, both tables; every brick of the 3 x 3 x 3 split and of the split one cell thick along x: rays march and
    are shaded in every brick, CENTRAL differs from CELL, and every ray comes back."""
    vol = cases.volume()
    whole = scenes.split_volume(vol, 1, 1, 1)[0]
    rays = cases.brick_rays(whole, n=600)
    for kind in ("dense", "spikes"):
        B = sm.Brick(vol, cases.table(kind), cases.RATE)
        a, b = sm.march(B, cases.lit(), rays, IDENT, kind=sm.CENTRAL), sm.march(B, cases.lit(), rays, IDENT, kind=sm.CELL)
        assert len(a) == len(rays) and sm.march.shaded > 0 and (bits(a["color"]) != bits(b["color"])).any(), kind
    thin = cases.volume((10, 14, 11))
    for grid, split in ((vol, (3, 3, 3)), (thin, cases.THIN_X)):
        for part in cases.bricks_of(grid, split):
            assert split != cases.THIN_X or int(part.counts[0]) == 2
            B = sm.Brick(part, cases.table("dense"), cases.RATE)
            r = cases.brick_rays(part, n=200)
            a = sm.march(B, cases.surfaces(), r, IDENT, kind=sm.CENTRAL)
            assert len(a) == len(r) and sm.march.shaded > 0 and B.has_required_ghosts()
            assert (bits(a["color"]) != bits(sm.march(B, cases.surfaces(), r, IDENT, kind=sm.CELL)["color"])).any()
    nf = cases.nonfinite_volume()
    assert np.isnan(nf.data).any() and np.isposinf(nf.data).any() and (nf.data == F(3e38)).any() and (nf.data == F(-3e38)).any()
    B = sm.Brick(nf, cases.table("dense"), cases.RATE)
    r = cases.brick_rays(scenes.split_volume(nf, 1, 1, 1)[0], n=600)
    a = sm.march(B, cases.lit(), r, IDENT, kind=sm.CENTRAL)
    assert sm.march.shaded > 0 and np.isfinite(a["color"]).all() and np.isfinite(a["w"]).all()
