"""tests/volume_shadow_amr_checker.py tied to the checkers it restates, and the cases of tests/volume_shadow_amr_cases.py shown not to be
vacuous -- on the CPU, no device.  Every comparison is bit for bit."""
import numpy as np
import pytest

from tests import volume_fog_shadow_checker as fg
from tests import volume_fused_amr_checker as fa
from tests import volume_mesh_shadow_checker as mg
from tests import volume_shadow_amr_cases as ac
from tests import volume_shadow_amr_checker as sa
from tests import volume_shadow_checker as sw
from tests.volume_common import IDENT

F = np.float32
KEYS = ("brick_visits", "rays_deposited", "crossings_rendered", "samples_shaded", "shadow_rays", "shadow_brick_visits", "shadow_crossings")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("bricking", ac.BRICKINGS)
def test_without_subgrids_it_is_the_existing_checkers(bricking):
    """Frames and grid of the scene with its subgrids removed: volume_shadow_checker's, volume_fog_shadow_checker's and
    volume_mesh_shadow_checker's bits and counters."""
    cam = ac.camera("outside")
    bricks, lo, hi = ac.checker_bricks("plain", bricking)
    whole, wlo, whi = ac.checker_bricks("plain", 1)
    S, shading = ac.surfaces("surf_lit", "plain")
    want, cw, _ = sw.frame(bricks, lo, hi, IDENT, cam, S, shading, None, ac.BIAS)
    got, cg = sa.frame(bricks, lo, hi, IDENT, cam, S, shading, None, None, None, ac.BIAS)
    assert (bits(got) == bits(want)).all() and want.any() and all(cg[k] == cw[k] for k in KEYS)
    Gw, uw = fg.grid(whole[0], wlo, whi, IDENT, IDENT, S, ac.GRID_BIAS)
    Gg, ug = sa.grid(whole[0], wlo, whi, IDENT, IDENT, S, ac.GRID_BIAS)
    assert (bits(Gg) == bits(Gw)).all() and (ug == uw).all()
    assert (bits(sa.grid_owned(bricks, whole[0], IDENT, IDENT, S, ac.GRID_BIAS)[0]) == bits(Gw)).all()
    O, _, blocked = mg.occluders(whole[0], IDENT, ac.mesh_scene(), S)
    assert blocked > 0
    for mode in ("surf_lit", "lit"):
        Sm, sh = ac.surfaces(mode, "plain")
        want, cw = fg.frame(bricks, lo, hi, IDENT, cam, Sm, sh, Gw, None, ac.BIAS)
        got, cg = sa.frame(bricks, lo, hi, IDENT, cam, Sm, sh, Gw, None, None, ac.BIAS)
        assert (bits(got) == bits(want)).all() and all(cg[k] == cw[k] for k in KEYS), mode
        want, cw = mg.frame(bricks, lo, hi, IDENT, cam, Sm, sh, Gw, O, None, ac.BIAS)
        got, cg = sa.frame(bricks, lo, hi, IDENT, cam, Sm, sh, Gw, O, None, ac.BIAS)
        assert (bits(got) == bits(want)).all() and all(cg[k] == cw[k] for k in KEYS), mode


@pytest.mark.parametrize("where", ac.EYES)
@pytest.mark.parametrize("mode", ["surf", "surf_lit"])
def test_without_a_usable_light_it_is_the_fused_amr_checker(mode, where):
    cam = ac.camera(where)
    bricks, lo, hi = ac.checker_bricks("scene", 8)
    S, shading = ac.surfaces(mode, lights=[((0.0, 0.0, 0.0), (1.0, 0.9, 0.8))])
    got, cg = sa.frame(bricks, lo, hi, IDENT, cam, S, shading, None, None, None, ac.BIAS)
    want, cw = fa.frame(bricks, lo, hi, IDENT, cam, S, shading)
    assert (bits(got) == bits(want)).all() and want.any()
    assert cg["shadow_rays"] == 0 and cg["brick_visits"] == cw["brick_visits"] and cg["crossings_rendered"] == cw["crossings"]
    assert cg["samples_shaded"] == cw["shaded"] and cg["amr"]["refined"] == cw["samples_refined"] > 0


@pytest.mark.parametrize("where", ac.EYES)
@pytest.mark.parametrize("kind, mode", [("shadow", "surf"), ("shadow", "surf_lit"), ("fog", "surf_lit"), ("fog", "lit"), ("mesh", "surf_lit"), ("mesh", "lit")])
def test_one_brick_equals_eight(kind, mode, where):
    one, c1, _ = ac.reference(kind, mode, 1, where)
    eight, c8, _ = ac.reference(kind, mode, 8, where)
    assert (bits(one) == bits(eight)).all() and one.any()
    for key in ("rays_deposited", "crossings_rendered", "samples_shaded", "shadow_rays", "shadow_crossings"):
        assert c1[key] == c8[key], key
    assert c8["brick_visits"] > c1["brick_visits"]
    assert c1["amr"]["refined"] == c8["amr"]["refined"] and c1["amr"]["shadow_refined"] == c8["amr"]["shadow_refined"]


@pytest.mark.parametrize("which", ["scene", "buried"])
def test_the_grid_by_ownership_is_the_one_bricks(which):
    """The bake's walk over the 8 bricks gives the definition's bits at every vertex, the shared ones included."""
    G, usable = ac.light_grid(which)
    whole, _, _ = ac.checker_bricks(which, 1)
    bricks, _, _ = ac.checker_bricks(which, 8)
    S, _ = ac.surfaces("surf_lit", which)
    Go, uo = sa.grid_owned(bricks, whole[0], IDENT, IDENT, S, ac.GRID_BIAS)
    assert usable.all() and (uo == usable).all() and (bits(Go) == bits(G)).all()


@pytest.mark.parametrize("where", ac.EYES)
def test_the_cases_are_not_vacuous(where):
    for mode in ("surf", "surf_lit"):
        fb, c, _ = ac.reference("shadow", mode, 8, where)
        amr = c["amr"]
        assert c["shadow_rays"] > 0  # shadow rays are cast
        assert amr["crossings_refined"] > 0  # a rendered crossing lies in a refined cell
        assert amr["shadow_refined"] > 0 and amr["shadow_transitions"] > 0  # shadow rays gather in refined cells and change between AMR and plain bricks
        assert (bits(fb) != bits(ac.unshadowed(mode, 8, where))).any()  # the shadows show
        A_s = c["details"]["A_s"]
        assert ((A_s > 0) & (A_s < 1)).any()
    # the fog's and the meshes' shadows show too
    fog = ac.reference("fog", "surf_lit", 8, where)[0]
    assert (bits(fog) != bits(ac.reference("shadow", "surf_lit", 8, where)[0])).any()
    assert (bits(ac.reference("mesh", "surf_lit", 8, where)[0]) != bits(fog)).any()
    assert (bits(ac.reference("mesh", "lit", 8, where)[0]) != bits(ac.reference("fog", "lit", 8, where)[0])).any()


def test_the_light_grid_is_not_vacuous():
    G, usable = ac.light_grid()
    assert usable.all() and ((G > 0) & (G < 1)).mean() > 0.5  # values strictly between 0 and 1
    whole, lo, hi = ac.checker_bricks("plain", 1)
    S, _ = ac.surfaces("surf_lit", "plain")
    G0, _ = fg.grid(whole[0], lo, hi, IDENT, IDENT, S, ac.GRID_BIAS)
    assert (bits(G) != bits(G0)).mean() > 0.01  # the subgrids change the grid
    # the buried volume: level 0 is transparent, every shadow on the grid comes from the subgrids
    Gb, _ = ac.light_grid("buried")
    assert (Gb < 1).mean() > 0.02 and (Gb == 1).mean() > 0.2
    O, _, blocked = ac.occluder_grid()
    assert 0 < blocked < O[0].size


def test_where_every_light_is_blocked_it_is_the_ambient_frame():
    """An occluder grid that is 0 everywhere: the mesh-shadowed frame has the bits of the unshadowed AMR frame with kd = 0 wherever the
    table adds no lit fog -- here everywhere, for the mode without lit fog."""
    cam = ac.camera("outside")
    bricks, lo, hi = ac.checker_bricks("scene", 8)
    S, shading = ac.surfaces("surf")
    whole = ac.checker_bricks("scene", 1)[0][0]
    dark, _ = sa.frame(bricks, lo, hi, IDENT, cam, S, shading, None, mg.constant(whole, S, 0), None, ac.BIAS)
    assert (bits(dark) == bits(ac.unshadowed("surf", 8, "outside", kd=0.0))).all()
