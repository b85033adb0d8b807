"""No GPU: the inputs of tests/test_gpu_early_deposit.py are not vacuous -- shown from the oracle's own output.  The oracle's framebuffer keeps, in a pixel's fourth
channel, the NUMBER of deposits the pixel received (one per terminal shadow ray that carries colour), un-clamped; its statistics count the shadow rays traced."""
import numpy as np
import pytest

from tests.early_deposit_cases import SIDE_FILMS, SMALL_FILMS, case


@pytest.mark.parametrize("name", SMALL_FILMS + ["400x300"] + SIDE_FILMS)
def test_soup_films_have_deposits_and_retractions_and_one_writer_per_pixel(name):
    sc, ref, st = case(name)
    deposits = int(round(float(ref[..., 3].astype(np.float64).sum())))  # shadow rays that survived and deposited
    lit = int((ref[..., 3] > 0).sum())
    print(name, "shadow rays", st.rays_any, "deposits", deposits, "lit pixels", lit, "camera rays traced", st.rays_closest)
    assert st.rays_any > 0 and 0 < deposits <= st.rays_any  # survivors exist
    assert lit == deposits and float(ref[..., 3].max()) == 1.0  # one writer per pixel: what the early store rests on
    if name.endswith("/side") or name == "200x120":
        # ... and so do shadow rays that deposit nothing: occluded ones (the grey soup shades no hit to c = 0: test_black_mesh... below is the case that does).
        # With the light AT the eye (the other films) a shadow ray runs back along its primary: 8x8, 24x16, 72x40 and 400x300 have no occluded ray at all
        assert deposits < st.rays_any
    if name == "800x600/side":  # the any-hit launch is large enough for its drain to share rays between lanes (share_min_rays, csrc/gvt_internal.h) ...
        assert st.rays_any >= 131072 and st.rays_any - deposits >= st.rays_any // 4  # ... and at least a quarter of its rays is retracted
    if name.startswith("200x120"):  # the cube covers the film's left part only: pixels no ray reaches, which must stay 0
        n_pix = sc.camera.width * sc.camera.height
        assert 0 < st.rays_closest < n_pix // 2  # (depth 1: rays_closest = the camera rays that enter the box)


def test_black_mesh_emits_shadow_rays_that_deposit_nothing():
    """kd = 0: Shade() returns c = 0 for every lit hit, the shadow ray is emitted all the same (the predicate len(c) > 0 then fails at the deposit)."""
    sc, ref, st = case("black")
    lit_soup = case("72x40")[2]
    assert st.rays_any == lit_soup.rays_any > 0  # the same rays as the grey soup on the same film ...
    assert not ref.any()                         # ... and not one deposit


def test_frames_outside_the_condition_differ_from_the_plain_soup_in_what_they_break():
    assert len(case("two_lights")[0].lights) == 2 and case("two_lights")[2].rays_any > case("72x40")[2].rays_any
    assert case("samples_2x2")[0].camera.samples == 2 and float(case("samples_2x2")[1][..., 3].max()) > 1.0  # several writers per pixel
    assert case("depth_2")[0].camera.depth == 2 and case("depth_2")[2].rays_closest > case("72x40")[2].rays_closest  # bounces were traced
    assert int(case("phong")[0].meshes[0].material["type"][0]) == 1
    assert case("two_instances")[0].n_inst == 2
