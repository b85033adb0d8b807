"""Knob xcd_stripes (csrc/xcd_stripes.h, trace_lane.inc): a single-mesh k_trace launch hands its ray list out in eight stripes, one per XCD, each from a work counter of
its own, instead of front to back from one.  The order of work is not a result: every frame and every hit list below is the oracle's, bit for bit, with the knob on
and off -- on films of one tile, of fewer tiles than stripes, of nine tiles per row, on a compacted list over a partial rectangle, with the class-ordered shadow list
and the parked-ray path active, and on plain ray lists without film geometry of 1 to 4,097 rays (which stay front to back under either knob value).  The small lists run in grids of fewer than eight blocks: stripes
without a wave of their own are reached by stealing alone."""
from dataclasses import replace

import numpy as np
import pytest

from gravit_amd import scenes
from gravit_amd.adapter import HipMeshAdapter
from gravit_amd.layouts import NORMALS_FLAT
from gravit_amd.scheduler import NativeTracer
from tests.helpers import bits, oracle_meshes, oracle_render

pytestmark = pytest.mark.gpu

N_TRIS, HALF = 3000, 0.04  # a soup dense enough that most camera rays hit and about half of the shadow rays are occluded
CW_LONG, CW_TRAV_OVF, CW_LONG_FRAME, CW_SHADOW_CLS = 3, 8, 20, 24  # counter words (csrc/gvt_device.h) as gvt_hip_counters_peek shows them

FILMS = {
    "8x8": (8, 8, None),         # one tile
    "24x16": (24, 16, None),     # six tiles: fewer than eight stripes
    "72x40": (72, 40, None),     # nine tiles per row: the row is no multiple of eight units
    "200x120": (200, 120, 1.3),  # the camera moved sideways: the cube's box reaches past the film's left edge -- a partial rectangle, a compacted list
    "400x300": (400, 300, None),
}
_cache = {}


def film(name):
    """The scene at that film and the oracle's frame of it (rendered once, shared, never written to)."""
    if name not in _cache:
        w, h, eye_x = FILMS[name]
        sc = scenes.soup_scene(N_TRIS, w, h, half_extent=HALF)
        if eye_x is not None:
            sc = replace(sc, camera=replace(sc.camera, eye=(eye_x, 0.5, 3.0), focus=(eye_x, 0.5, 0.5)))
        ref, st = oracle_render(sc, NORMALS_FLAT, nthreads=8)
        ref.setflags(write=False)
        _cache[name] = (sc, ref, st)
    return _cache[name]


def render(hip, sc, stripes, opts):
    try:
        for k, v in dict(opts, xcd_stripes=stripes).items():
            hip.set_option(k, v)
        tr = NativeTracer(sc, NORMALS_FLAT)
        fb = tr().framebuffer(True).copy()
        stats, words = dict(tr.stats), hip.counters_peek()
        tr.close()
        return fb, stats, words
    finally:
        hip.set_option("defaults", 0)


def check_frame(hip, name, opts, also=None):
    sc, ref, st = film(name)
    assert st.rays_closest > 0 and st.rays_any > 0
    fbs = {}
    for stripes in (0, 1):
        fb, stats, words = render(hip, sc, stripes, opts)
        assert np.array_equal(bits(fb), bits(ref)), "%s, xcd_stripes=%d: %d pixels differ from the oracle's" % (name, stripes, (bits(fb) != bits(ref)).any(axis=-1).sum())
        assert stats["rays_closest"] == st.rays_closest and stats["rays_any"] == st.rays_any, (name, stripes, stats["rays_closest"], stats["rays_any"], st.rays_closest, st.rays_any)
        assert words[CW_TRAV_OVF] == 0
        if also:
            also(stripes, st, words)
        fbs[stripes] = fb
    assert np.array_equal(bits(fbs[0]), bits(fbs[1]))


# small_rays = 0, finish_rays = 0, packet = 0: these few rays go through k_trace, a lane per ray, and not a wave per ray or through k_finish
LANES = dict(small_rays=0, finish_rays=0, packet=0)


@pytest.mark.parametrize("name", ["8x8", "24x16", "72x40", "200x120"])
def test_small_films_equal_the_oracle_with_stripes_on_and_off(hip, name):
    sc = film(name)[0]
    if name == "200x120":  # the cube covers the film's left part only, and not every ray of the rectangle around it enters its box
        assert 0 < film(name)[2].rays_closest < sc.camera.width * sc.camera.height // 2
    check_frame(hip, name, LANES)


def test_larger_film_with_the_ordered_shadow_list_and_parked_rays(hip):
    def also(stripes, st, words):
        classes = words[CW_SHADOW_CLS:CW_SHADOW_CLS + 8]
        assert sum(classes) == st.rays_any, classes    # the class-ordered list is in use (in arrival order these words stay 0)
        assert words[CW_LONG] + words[CW_LONG_FRAME] > 0  # ... and rays were parked for a wave each

    # (long_steps 4: a ray of this small tree that takes more than four node steps is parked; long_auto 0: the threshold stays there)
    check_frame(hip, "400x300", dict(LANES, shadow_order=1, shadow_order_min_rays=0, long_min_rays=0, long_steps=4, long_auto=0), also)


@pytest.fixture(scope="module")
def mesh_pair(hip):
    sc = film("8x8")[0]
    ad = HipMeshAdapter(sc.meshes[0], NORMALS_FLAT)
    yield sc.meshes[0], ad, oracle_meshes(sc)[0]
    ad.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_plain_ray_lists_are_traced_ray_by_ray(hip, mesh_pair, n):
    """A list without film geometry (row length 0): handed out front to back from the one counter whatever the knob says (stripes need a row length), through the
    same fetch function as the striped launches.  Every ray aims at the centroid of a triangle from outside the soup, so every ray has a hit; the device's hit
    buffer is left full of MISS records by a call of the same length in front (rays that point away from the soup: prim -1, t FLT_MAX -- the sentinel), so a
    ray the launch left out would still read as a miss."""
    mesh, ad, om = mesh_pair
    rng = np.random.default_rng(n)
    cen = mesh.verts[mesh.tris[rng.integers(0, len(mesh.tris), n)]].mean(axis=1).astype(np.float32)
    org = cen.copy()
    org[:, 2] = 1.5
    org[:, :2] += rng.uniform(-0.2, 0.2, (n, 2)).astype(np.float32)
    d = cen - org
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    want = om.intersect(org, d)
    assert (want["prim"] >= 0).all()
    away = np.tile(np.float32([0, 0, 1]), (n, 1))
    for stripes in (0, 1):
        try:
            hip.set_option("xcd_stripes", stripes)
            miss = ad.intersect(org, away)
            assert (miss["prim"] == -1).all()
            got = ad.intersect(org, d)
            assert hip.counters_peek()[CW_TRAV_OVF] == 0
            assert (ad.occluded(org, d) == 1).all() and (ad.occluded(org, away) == 0).all()
        finally:
            hip.set_option("defaults", 0)
        assert (got["prim"] == want["prim"]).all(), "%d primIDs differ" % (got["prim"] != want["prim"]).sum()
        for f in ("t", "u", "v"):
            assert (bits(got[f]) == bits(want[f])).all(), f
