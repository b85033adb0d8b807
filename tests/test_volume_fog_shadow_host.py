"""Shadowed fog without a device: the numpy checker (tests/volume_fog_shadow_checker.py) against the checkers that exist, the finding
about lights parallel to a grid plane, the properties of the checker's frame, and the Python surface's refusals."""
import numpy as np
import pytest

from gravit_amd import capi
from gravit_amd.scheduler import VolumeDomainTracer, VolumeTracer
from tests import volume_checker as vc
from tests import volume_fog_shadow_cases as fgc
from tests import volume_fog_shadow_checker as fg
from tests import volume_fused_cases as fc
from tests import volume_shadow_checker as sw

F = np.float32
MULTI = [s for s in fc.SPLITS if s != (1, 1, 1)]
PARALLEL_LIGHTS = tuple((p, fgc.WHITE) for p in fgc.PARALLEL)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_the_grids_hold_all_three_kinds_of_vertex():
    """Of the 15,625 vertices under the identity matrix, as A_s == 0 / 0 < A_s < 0.99 / A_s >= 0.99 (measured, grid bias 1):
    lit (3, 4, 5) 0.115 / 0.194 / 0.691, (-2, 1, 0.5) 0.115 / 0.106 / 0.779; surf_lit 0.323 / 0.644 / 0.034 and 0.430 / 0.567 / 0.003."""
    G, usable = fgc.light_grid("lit", False)
    assert usable.all() and G.shape == (2, fc.N, fc.N, fc.N)
    for j in range(2):
        assert min(fgc.shares(G[j])) >= 0.05, fgc.shares(G[j])
    G, _ = fgc.light_grid("surf_lit", False)
    for j in range(2):
        clear, partial, _ = fgc.shares(G[j])
        assert clear >= 0.2 and partial >= 0.2, fgc.shares(G[j])


@pytest.mark.parametrize("moved", [False, True])
@pytest.mark.parametrize("mode", fgc.MODES)
def test_generic_lights_the_grid_is_the_existing_bricked_walk(mode, moved):
    """For lights with three non-zero components the next-brick walk of the shadowed frame is bricking-invariant from grid vertices too:
    the checker's grid (one brick) has its bits in every split.  (Under MOVED: the (2, 2, 2) and (4, 4, 4) splits.)"""
    B, _, _, m, minv, S, _ = fgc.whole(mode, moved)
    G, _ = fgc.light_grid(mode, moved)
    ws, _ = sw.light_rays(S)
    for split in (MULTI if not moved else [(2, 2, 2), (4, 4, 4)]):
        bricks, lo, hi = fgc.setup(mode, split, "outside", moved)[:3]
        for j in range(len(ws)):
            A_s = fg.opacity(bricks, lo, hi, m, minv, S, B, ws[j], fgc.GRID_BIAS)
            assert (bits(F(1) - A_s) == bits(G[j].reshape(-1))).all(), (split, j)


@pytest.mark.parametrize("mode", fgc.MODES)
def test_parallel_lights_the_ownership_walk_is_invariant_and_the_next_brick_walk_is_not(mode):
    """The finding (include/gvt_hip.h, "shadowed surfaces", DEVIATIONS (5)): under (0, 0, 1), (0, 1, 0) and (1, 1, 0) the next-brick walk
    loses the samples of rays that run in a brick face, so its A_s depends on the bricking (measured on `lit`, of 15,625 values, (2, 2, 2) /
    (4, 4, 4): 1,128 / 3,240, 1,152 / 3,312 and 576 / 1,728 differ); the walk by sample ownership, which the bake restates, gives the one
    brick's bits in every split."""
    B, _, _, m, minv, S, _ = fgc.whole(mode, False, PARALLEL_LIGHTS)
    G, usable = fgc.light_grid(mode, False, PARALLEL_LIGHTS)
    ws, _ = sw.light_rays(S)
    assert usable.all()
    for split in MULTI:
        bricks, lo, hi = fgc.setup(mode, split, "outside", False)[:3]
        for j in range(len(ws)):
            owned = fg.opacity_owned(bricks, B, m, minv, S, ws[j], fgc.GRID_BIAS)
            assert (bits(F(1) - owned) == bits(G[j].reshape(-1))).all(), (split, j)
    bricks, lo, hi = fgc.setup(mode, (2, 2, 2), "outside", False)[:3]
    walked = fg.opacity(bricks, lo, hi, m, minv, S, B, ws[0], fgc.GRID_BIAS)
    assert (bits(F(1) - walked) != bits(G[0].reshape(-1))).sum() > 400  # the walk the bake must not inherit


@pytest.mark.parametrize("mode", fgc.MODES)
def test_generic_lights_the_ownership_walk_is_invariant(mode):
    B, _, _, m, minv, S, _ = fgc.whole(mode, True)
    G, _ = fgc.light_grid(mode, True)
    ws, _ = sw.light_rays(S)
    for split in MULTI:
        bricks = fgc.setup(mode, split, "outside", True)[0]
        for j in range(len(ws)):
            owned = fg.opacity_owned(bricks, B, m, minv, S, ws[j], fgc.GRID_BIAS)
            assert (bits(F(1) - owned) == bits(G[j].reshape(-1))).all(), (split, j)


@pytest.mark.parametrize("mode", fgc.MODES)
def test_the_cut_does_not_show_in_the_checkers_frame(mode):
    want, counters, _ = fgc.reference(mode, (1, 1, 1), "outside")
    assert want.any() and counters["samples_shaded"] > 0
    for split in MULTI:
        got, c, _ = fgc.reference(mode, split, "outside")
        assert (bits(got) == bits(want)).all(), split
        for key in ("rays_deposited", "crossings_rendered", "samples_shaded", "shadow_rays", "shadow_crossings"):
            assert c[key] == counters[key], (split, key)


@pytest.mark.parametrize("where", sorted(fgc.CAMERAS))
@pytest.mark.parametrize("mode", fgc.MODES)
def test_shadows_only_darken(mode, where):
    """Alpha is the unshadowed frame's in every bit (A never depends on G or T); every colour channel is at most the unshadowed frame's,
    and strictly below it on at least half of the pixels whose ray shades a fog sample.  Measured shares of those pixels, outside /
    inside eye: lit 1.000 / 1.000, surf_lit 1.000 / 1.000."""
    got, counters, _ = fgc.reference(mode, (2, 2, 2), where)
    plain, pc = fgc.unshadowed(mode, (2, 2, 2), where)
    assert (bits(got[..., 3]) == bits(plain[..., 3])).all()
    assert (got[..., :3] <= plain[..., :3]).all()
    assert counters["samples_shaded"] == pc["samples_shaded"] > 0
    shaded = counters["shaded_pixels"].reshape(got.shape[:2])
    darker = (got[..., :3] < plain[..., :3]).all(axis=-1)
    share = darker[shaded].mean()
    print("%s %s: %d pixels shade a sample, %.3f of them strictly darker" % (mode, where, shaded.sum(), share))
    assert shaded.sum() > 20 and share >= 0.5


def test_without_a_grid_the_frame_is_the_shadowed_frame():
    """G = None (every Tg = 1): the checker's frame is volume_shadow_checker.frame's in every bit."""
    bricks, lo, hi, minv, cam, S, shading, _, _ = fgc.setup("surf_lit", (2, 2, 2), "inside")
    got, counters = fg.frame(bricks, lo, hi, minv, cam, S, shading, None, None, fgc.BIAS)
    want, wc, _ = sw.frame(bricks, lo, hi, minv, cam, S, shading, None, fgc.BIAS)
    assert (bits(got) == bits(want)).all() and got.any()
    for key in wc:
        assert counters[key] == wc[key], key


def test_the_binding_names_the_entry_points():
    for name in ("gvt_hip_volume_light_grid_bake", "gvt_hip_volume_light_grid_download", "gvt_hip_volume_light_grid_info", "gvt_hip_volume_light_grid_release",
                 "gvt_hip_volume_frame_fog_shadowed"):
        assert name in capi.SYMBOLS
    names = [n for n, _ in capi.VolumeFogShadowStats._fields_]
    assert names[:len(capi.VolumeShadowStats._fields_)] == [n for n, _ in capi.VolumeShadowStats._fields_] and names[-1] == "fog_samples_shadowed"
    assert [n for n, _ in capi.VolumeLightGridStats._fields_][:5] == ["rays", "samples_marched", "samples_gathered", "crossings", "bytes"]


def test_fog_shadows_need_shadows_and_one_device():
    with pytest.raises(ValueError, match="fog_shadows"):
        VolumeTracer([], None, None, fog_shadows=True)
    with pytest.raises(ValueError, match="fog_shadows"):
        VolumeDomainTracer([], [], None, None, None, None, None, fog_shadows=True)
