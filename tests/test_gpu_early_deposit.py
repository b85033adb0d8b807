"""Knob early_deposit (csrc/shade.inc store_shadow_early, k_trace's MODE 2 in csrc/trace_lane.inc, the condition in csrc/trace.hip single_pass): in the one-instance frame
with one light, one sample per pixel and depth 1, k_shade stores a shadow ray's deposit to its pixel itself and the any-hit launch only takes it back where the ray is
occluded.  Where a deposit is made is not a result: every frame below is the oracle's, bit for bit, with the same ray counts, with the knob on and off; the frame's
statistics say which path ran (early_deposit_launches), and every frame that breaks one of the conditions must show 0 there.  The films are those of
tests/test_gpu_xcd_stripes.py, each also with the light moved to the side of the soup (NAME/side): with the light at the eye next to no shadow ray is occluded, with it
at the side a third of them is -- deposits and retractions both happen en masse (tests/test_early_deposit_host.py shows that from the oracle's own output)."""
import numpy as np
import pytest

from gravit_amd.layouts import NORMALS_FLAT
from gravit_amd.scheduler import NativeTracer
from tests.early_deposit_cases import SMALL_FILMS, case
from tests.helpers import bits

SMALL_BOTH = SMALL_FILMS + [n + "/side" for n in SMALL_FILMS]

pytestmark = pytest.mark.gpu

CW_TRAV_OVF = 8  # counter word (csrc/gvt_device.h) as gvt_hip_counters_peek shows it
# small_rays = 0, finish_rays = 0, packet = 0: these few rays go through k_trace, a lane per ray, and not a wave per ray, as packets or through k_finish
LANES = dict(small_rays=0, finish_rays=0, packet=0)
# + class regions and parked rays.  Drain sharing needs a launch of at least share_min_rays = 131,072 rays (a tuned constant the shipped library cannot move): the
# 400x300 films' 44,583 / 36,603 shadow rays never share, the 800x600/side film's 146,961 do.  The shipped library cannot report a hand-off (no device counter); the
# diagnostics build (-DGVT_STAMP, tools/stamps.py --build; g_stamp[23]) counted, with these options and the knob on: 6,208 hand-offs in that film's frame, 0 in 400x300/side's
ORDERED = dict(LANES, shadow_order=1, shadow_order_min_rays=0, long_min_rays=0, long_steps=4, long_auto=0)


def frames(hip, sc, opts, knobs):
    """One tracer, one frame per entry of `knobs` (the value of early_deposit for that frame): [(framebuffer, frame statistics, counter words)]."""
    out = []
    try:
        for k, v in opts.items():
            hip.set_option(k, v)
        tr = NativeTracer(sc, NORMALS_FLAT)
        for knob in knobs:
            hip.set_option("early_deposit", knob)
            fb = tr().framebuffer(True).copy()
            out.append((fb, dict(tr.stats), hip.counters_peek()))
        tr.close()
    finally:
        hip.set_option("defaults", 0)
    return out


def check(name, knob, got, want_path):
    """The frame is the oracle's, ray for ray; want_path: True -- the early path ran, False -- it did not."""
    sc, ref, st = case(name)
    fb, stats, words = got
    assert np.array_equal(bits(fb), bits(ref)), "%s, early_deposit=%d: %d pixels differ from the oracle's" % (name, knob, (bits(fb) != bits(ref)).any(axis=-1).sum())
    assert stats["rays_closest"] == st.rays_closest and stats["rays_any"] == st.rays_any, (name, knob, stats["rays_closest"], stats["rays_any"], st.rays_closest, st.rays_any)
    assert words[CW_TRAV_OVF] == 0
    assert (stats["early_deposit_launches"] > 0) == want_path, (name, knob, stats["early_deposit_launches"])


def check_both(hip, name, opts, path_with_knob):
    on, off = frames(hip, case(name)[0], opts, [1])[0], frames(hip, case(name)[0], opts, [0])[0]
    check(name, 1, on, path_with_knob)
    check(name, 0, off, False)
    assert np.array_equal(bits(on[0]), bits(off[0]))


@pytest.mark.parametrize("name", SMALL_BOTH)
def test_small_films_equal_the_oracle_with_the_knob_on_and_off(hip, name):
    check_both(hip, name, LANES, True)


@pytest.mark.parametrize("name", ["400x300", "400x300/side", "800x600/side"])
def test_larger_film_with_class_regions_parked_rays_and_drain_sharing(hip, name):
    """800x600/side: 146,961 shadow rays, 36 % of them occluded, in a launch large enough for drain sharing -- several lanes on one ray, the fold of their results and
    then the retraction by the lane that carries the group's occlusion."""
    if name == "800x600/side":
        assert case(name)[2].rays_any >= 131072  # share_min_rays (csrc/gvt_internal.h)
    check_both(hip, name, ORDERED, True)


@pytest.mark.parametrize("name", ["400x300", "400x300/side", "72x40", "72x40/side"])
def test_default_options_keep_small_rounds_on_the_wave_per_ray_paths(hip, name):
    """Every option at its default.  A round of at most small_rays = 4,096 rays goes a wave per ray (k_wave_any deposits as before): the 72x40 film's 2,880 rays never take
    the early path.  The 400x300 film's round is sized by its bound of 120,000 camera rays -- beyond small_rays and finish_rays, below shadow_order_min_rays --: a lane
    per ray in arrival order, and so the early path with the knob on."""
    check_both(hip, name, {}, name.startswith("400x300"))


@pytest.mark.parametrize("name", ["two_lights", "samples_2x2", "depth_2", "phong", "two_instances"])
def test_frames_outside_the_condition_keep_the_atomics(hip, name):
    check(name, 1, frames(hip, case(name)[0], LANES, [1])[0], False)


def test_rays_that_fail_the_deposit_predicate_are_traced_and_touch_no_pixel(hip):
    """A LAMBERT colour of 0: every shadow ray is emitted with c = 0 -- traced and counted, no deposit.  The frame stays all zero (the oracle's)."""
    sc, ref, st = case("black")
    assert st.rays_any > 0 and not ref.any()
    check_both(hip, "black", LANES, True)


@pytest.mark.parametrize("order", [(1, 0), (0, 1), (1, 1)])
def test_frames_of_one_tracer_with_the_knob_switched_between_them(hip, order):
    """The per-frame clear precedes the early stores, and no state leaks from one frame into the next."""
    got = frames(hip, case("72x40/side")[0], LANES, list(order))
    for knob, g in zip(order, got):
        check("72x40/side", knob, g, knob == 1)
