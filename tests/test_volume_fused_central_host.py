"""tests/volume_central_shadow_checker.py on the CPU (no GPU here): the new checker pinned at both ends -- with kind CELL its frames are the
existing shadow, fog-shadow and mesh-shadow checkers' on their own main cases, with CENTRAL and no shadows they are
volume_smooth_checker.frame's -- and the cases of tests/test_gpu_volume_fused_central.py shown not to be vacuous: CENTRAL shows in the
shadowed image, the shadows show in the CENTRAL image, some pixel is partly shadowed, and the alpha plane does not depend on the kind."""
import numpy as np
import pytest

from tests import volume_central_cases as ccs
from tests import volume_central_shadow_checker as cs
from tests import volume_fog_shadow_cases as fgc
from tests import volume_mesh_shadow_cases as mc
from tests import volume_shadow_cases as swc
from tests import volume_smooth_checker as sm

SPLIT, WHERE = (2, 2, 2), "inside"
COUNTER_KEYS = ("brick_visits", "rays_deposited", "crossings_rendered", "samples_shaded", "shadow_rays", "shadow_brick_visits", "shadow_crossings")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("mode", ["surf", "surf_lit"])
def test_cell_is_the_shadow_checkers_frame(mode):
    want, counters, _, _ = swc.reference("main", SPLIT, WHERE, mode)
    got, mine, _ = ccs.reference("shadow", mode, SPLIT, WHERE, kind=cs.CELL)
    assert want.any() and (bits(got) == bits(want)).all()
    for key in COUNTER_KEYS:
        assert mine[key] == counters[key], key


@pytest.mark.parametrize("mode", fgc.MODES)
def test_cell_is_the_fog_shadow_checkers_frame(mode):
    want, counters, _ = fgc.reference(mode, SPLIT, WHERE)
    got, mine, _ = ccs.reference("fog", mode, SPLIT, WHERE, kind=cs.CELL)
    assert want.any() and (bits(got) == bits(want)).all()
    for key in COUNTER_KEYS:
        assert mine[key] == counters[key], key


@pytest.mark.parametrize("mode", ["surf_lit", "surf"])
def test_cell_is_the_mesh_shadow_checkers_frame(mode):
    want, counters, _ = mc.reference(mode, SPLIT, WHERE)
    got, mine, _ = ccs.reference("mesh", mode, SPLIT, WHERE, kind=cs.CELL)
    assert want.any() and (bits(got) == bits(want)).all()
    for key in COUNTER_KEYS:
        assert mine[key] == counters[key], key


def test_the_clipped_cell_frame_too():
    want, counters, _, plane = swc.reference("main", SPLIT, "outside", clipped=True)
    got, mine, mine_plane = ccs.reference("shadow", "surf", SPLIT, "outside", kind=cs.CELL, clipped=True)
    assert (bits(plane) == bits(mine_plane)).all() and (bits(got) == bits(want)).all()
    for key in COUNTER_KEYS:
        assert mine[key] == counters[key], key


@pytest.mark.parametrize("mode", ["surf", "surf_lit", "lit"])
def test_central_without_shadows_is_the_smooth_checkers_frame(mode):
    bricks, lo, hi, minv, cam, S, shading, _, _ = ccs.setup(mode, SPLIT, WHERE)
    want, _ = sm.frame(bricks, lo, hi, minv, cam, S, shading, kind=sm.CENTRAL)
    got, counters, _ = ccs.reference("plain", mode, SPLIT, WHERE)
    assert want.any() and (bits(got) == bits(want)).all()
    assert counters["samples_shaded"] == sm.frame.shaded and counters["crossings_rendered"] == sm.frame.crossings
    assert counters["shadow_rays"] == 0
    cell, _ = sm.frame(bricks, lo, hi, minv, cam, S, shading, kind=sm.CELL)
    assert (bits(got) != bits(cell)).any()  # the kind shows


@pytest.mark.parametrize("frame,mode", [("shadow", "surf"), ("fog", "surf_lit"), ("mesh", "surf_lit")])
def test_the_cases_are_not_vacuous(frame, mode):
    central, counters, _ = ccs.reference(frame, mode, SPLIT, WHERE)
    cell, cell_counters, _ = ccs.reference(frame, mode, SPLIT, WHERE, kind=cs.CELL)
    plain, _, _ = ccs.reference("plain", mode, SPLIT, WHERE)
    ambient, _, _ = ccs.reference("plain", mode, SPLIT, WHERE, kd=0.0)
    c, e, p, a = (bits(x).reshape(-1, 4) for x in (central, cell, plain, ambient))
    assert (c[:, :3] != e[:, :3]).any()  # CENTRAL shows in the shadowed image
    assert (c[:, :3] != p[:, :3]).any()  # the shadows show in the CENTRAL image
    partial = (c[:, :3] != p[:, :3]).any(axis=1) & (c[:, :3] != a[:, :3]).any(axis=1)
    assert partial.sum() > 50  # pixels that are neither unshadowed nor lit by the ambient term alone
    assert (c[:, 3] == e[:, 3]).all() and (c[:, 3] == p[:, 3]).all()  # the alpha plane depends on neither the kind nor the shadows
    for key in COUNTER_KEYS:  # ... and no counter depends on the kind
        assert counters[key] == cell_counters[key], key
    assert counters["shadow_rays"] > 0 and counters["shadow_crossings"] > 0
