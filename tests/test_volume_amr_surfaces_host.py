"""Shaded AMR volumes without a device: the numpy checker (tests/volume_amr_surface_checker.py) against the surface and the shade
checkers on exactly refined fields and on volumes without subgrids, its bricking invariance, and the coverage the GPU tests rely on
(crossings and shaded samples in refined cells, at grid changes and in the level-2 subgrid)."""
import numpy as np
import pytest

from gravit_amd import scenes
from gravit_amd.adapter import TransferFunction
from tests import volume_amr_cases as cases
from tests import volume_amr_checker as ac
from tests import volume_amr_surface_cases as scases
from tests import volume_amr_surface_checker as asc
from tests import volume_checker as vc
from tests import volume_shade_checker as shc
from tests import volume_surface_checker as sc
from tests.test_volume_amr_host import rays_through
from tests.volume_common import IDENT, read, tf

F = np.float32
FIELDS = ("color", "w", "t_min", "depth", "t")


def same_bits(a, b, fields=FIELDS):
    for f in fields:
        assert (np.ascontiguousarray(a[f]).view(np.uint32) == np.ascontiguousarray(b[f]).view(np.uint32)).all(), f


def index_surfaces(vol):
    """Isovalues in index units (the exact scenes hold v = the vertex index), S0's plane and the light."""
    return scases.surfaces(vol, isovalues=(5.5, 7.25))


@pytest.mark.parametrize("which", ["r2", "r8", "nested"])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_exact_refinement_gives_the_plain_surface_and_lit_bits(axis, which):
    """v = the vertex index along one axis, refined exactly: the fine cell's differences and its spacing both scale by 1 / R, so the
    gradient, and with it every crossing and every shaded sample, is the plain volume's in every bit."""
    vol = cases.exact_scene(axis, which)
    t = TransferFunction(read("CoolWarm.cmap", 4), read("ramp.omap", 2), (0.0, 20.0))
    rays = np.concatenate([rays_through(vol, 400), cases.plane_rays(vol, IDENT, 150)])
    S = index_surfaces(vol)
    B = ac.AmrBrick(vol, t, 1.3)
    P = vc.Brick(scenes.VolumeData(vol.data, vol.origin, vol.spacing), t, 1.3)
    counts = {}
    same_bits(asc.march(B, S, rays, IDENT, asc.SHADE_NONE, counts), sc.march(P, S, rays, IDENT))
    assert counts["crossings"] == sc.march.crossings and counts["crossings_refined"] > 0 and counts["shaded"] == 0
    counts = {}
    same_bits(asc.march(B, S, rays, IDENT, asc.SHADE_GRADIENT, counts), shc.march(P, S, rays, IDENT))
    assert counts["crossings"] == shc.march.crossings and counts["shaded"] == shc.march.shaded
    assert counts["crossings_refined"] > 0 and counts["shaded_refined"] > 0 and 0 < counts["refined"] < counts["marched"]
    counts = {}
    L = shc.lights_only(scases.LIGHTS)
    same_bits(asc.march(B, L, rays, IDENT, asc.SHADE_GRADIENT, counts), shc.march(P, L, rays, IDENT), FIELDS[:4])
    assert counts["shaded"] == shc.march.shaded and counts["shaded_refined"] > 0 and counts["crossings"] == 0


def test_without_subgrids_the_checker_is_its_parents():
    vol = cases.level0()
    t = tf("cool")
    rays = rays_through(vol)
    S = scases.surfaces(vol)
    B, P = ac.AmrBrick(vol, t, 2.6), vc.Brick(vol, t, 2.6)
    counts = {}
    same_bits(asc.march(B, S, rays, IDENT, asc.SHADE_NONE, counts), sc.march(P, S, rays, IDENT))
    assert counts["crossings"] == sc.march.crossings > 0 and counts["refined"] == 0
    counts = {}
    same_bits(asc.march(B, S, rays, IDENT, asc.SHADE_GRADIENT, counts), shc.march(P, S, rays, IDENT))
    assert counts["crossings"] == shc.march.crossings > 0 and counts["shaded"] == shc.march.shaded > 0
    same_bits(asc.march(B, None, rays, IDENT), ac.march(B, rays, IDENT), FIELDS[:4])  # nothing set: the plain AMR march


def test_bricked_checker_equals_the_one_brick_checker():
    """Surfaces and lit fog on the checker alone: a crossing belongs to the owner of the later sample, so the bits do not depend on how
    the data is cut as long as every level-1 subgrid stays in one brick."""
    vol = cases.scene()
    t = thin()  # (opacity rising to 0.08 and surfaces of opacity 0.3: the rays reach the subgrids)
    cam = scenes.Camera((0.9, 1.3, 1.6), (0.25, 0.6, 0.0), (0.0, 1.0, 0.0), float(F(35.0 * np.pi / 180.0)), 24, 18)
    S = scases.surfaces(vol, opacity=0.3)
    whole = ac.AmrBrick(vol, t, 1.3)
    c1, c8 = {}, {}
    want, calls = asc.frame([whole], whole.lo[None], whole.hi[None], IDENT, cam, S, counts=c1)
    parts = scenes.split_amr_volume(vol, 2, 2, 2, cuts=cases.CUTS)
    bricks = [ac.AmrBrick(b, t, 1.3) for b in parts]
    got, calls8 = asc.frame(bricks, [b.lo for b in parts], [b.hi for b in parts], IDENT, cam, S, counts=c8)
    assert calls == 1 and calls8 > 1 and (want[..., 3] > 0).sum() > 50
    assert (got.view(np.uint32) == want.view(np.uint32)).all()
    assert c1["crossings"] == c8["crossings"] > 0 and c1["shaded"] == c8["shaded"] > 0 and c1["crossings_refined"] == c8["crossings_refined"] > 0


def thin():
    return TransferFunction(read("CoolWarm.cmap", 4), np.array([[0.0, 0.0], [1.0, 0.08]], F), (0.0, 1.0))


def test_the_rays_of_the_gpu_tests_cover_the_refined_cases():
    """What the device tests need from their rays, asserted on the checker's counts: crossings at refined samples, at a grid change and
    in the level-2 subgrid, plane crossings at refined samples, shaded refined samples.  The figures (printed below), under the thin
    table with one isovalue of opacity 0.3: isovalue 0.5 gives 1562 crossings, 211 at refined samples, 39 at a grid change, 2 inside S1;
    0.52 gives 1638 / 244 / 50 / 2.  The subgrids' values span 0.30 to 0.71: an isovalue outside them has no refined crossing."""
    vol = cases.scene()
    t = thin()
    B = ac.AmrBrick(vol, t, 1.3)
    rays = rays_through(vol, 1500)
    for iso in scases.ISOVALUES:
        counts = {}
        asc.march(B, scases.surfaces(vol, isovalues=(iso,), plane=False, opacity=0.3), rays, IDENT, asc.SHADE_NONE, counts)
        print("isovalue %.2f: %d crossings, %d at refined samples, %d at a grid change, per level %s"
              % (iso, counts["crossings"], counts["crossings_refined"], counts["crossings_grid_change"], counts["crossings_level"]))
        assert counts["crossings"] > counts["crossings_refined"] > 0 and counts["crossings_grid_change"] > 0
    mn = min(float(s.data.min()) for s in vol.subgrids)
    mx = max(float(s.data.max()) for s in vol.subgrids)
    for iso in (mn - 0.05, mx + 0.05):  # outside the subgrids' values: no refined crossing
        counts = {}
        asc.march(B, scases.surfaces(vol, isovalues=(iso,), plane=False), rays, IDENT, asc.SHADE_NONE, counts)
        assert counts["crossings_refined"] == 0
    # all surfaces, lit, with the rays aimed at S1: the level-2 condition and the rest
    rays = np.concatenate([rays, scases.s1_rays(vol, IDENT)])
    counts = {}
    asc.march(B, scases.surfaces(vol, opacity=0.3), rays, IDENT, asc.SHADE_GRADIENT, counts)
    print(counts)
    assert counts["crossings_level"].get(2, 0) > 0 and counts["crossings_level"].get(1, 0) > 0 and counts["crossings_level"].get(0, 0) > 0
    assert counts["crossings_refined"] > 0 and counts["crossings_grid_change"] > 0 and counts["plane_crossings_refined"] > 0
    assert counts["shaded_refined"] > 0 and counts["shaded"] > counts["shaded_refined"]


def test_the_peak_is_crossed_in_the_subgrid_only():
    vol = scases.peak_scene()
    B = ac.AmrBrick(vol, thin(), 1.3)
    counts = {}
    asc.march(B, scases.surfaces(vol, isovalues=(scases.PEAK_ISO,), plane=False), rays_through(vol, 600), IDENT, asc.SHADE_NONE, counts)
    # level 0 stays below the isovalue: at every crossing this sample or the one before it lies in the subgrid
    assert 0 < counts["crossings"] <= counts["crossings_refined"] + counts["crossings_grid_change"]
    assert counts["crossings_level"].get(1, 0) > 0
