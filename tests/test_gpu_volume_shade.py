"""Lit volumes on the device (vol_accumulate_lit and the k_volume_march_lit / _surf_lit entry points of csrc/volume.hip) against the numpy
checker (tests/volume_shade_checker.py), bit for bit on color, w, t_min, depth and t: gvt_hip_volume_trace with and without surfaces,
the identities that give the unlit bits, macro-cell skipping against NO_SKIP, frames over several brickings, typed voxels, the clipped
frame and the mixed frame, grids that are not finite, and the argument checks."""
import numpy as np
import pytest

from gravit_amd import capi, scenes
from gravit_amd.adapter import DepthPlane, HipVolumeAdapter
from gravit_amd.scheduler import MixedTracer, VolumeTracer
from tests import volume_checker as vc
from tests import volume_clip_checker as cc
from tests import volume_shade_checker as lc
from tests import volume_surface_checker as sc
from tests.test_gpu_volume import IDENT, MOVED, camera, grid, make_rays, tf
from tests.test_gpu_volume_surfaces import ISO, LIGHTS, PLANES
from tests.test_gpu_volume_types import as_float, quantised, scaled

pytestmark = pytest.mark.gpu

F = np.float32
ALL = ("color", "w", "t_min", "depth", "t")


def same_bits(a, b, fields=ALL):
    for f in fields:
        x, y = np.ascontiguousarray(a[f]).view(np.uint32), np.ascontiguousarray(b[f]).view(np.uint32)
        assert (x == y).all(), "%s: %d of %d rays differ" % (f, (x != y).reshape(len(a), -1).any(axis=1).sum(), len(a))


def adapter(vol, t, rate, S, shading=True, skip=True, native=False):
    """A volume with S's surfaces (if any) and lights, and the shading mode."""
    ad = HipVolumeAdapter(vol, sampling_rate=rate, skip=skip, native=native)
    ad.set_transfer(t)
    if S is not None:
        if len(S):
            ad.set_surfaces(S.iso, S.planes, float(S.opacity))
        ad.set_lights(list(zip(S.lpos, S.lcol)), float(S.ka), float(S.kd))
    if shading is not None:
        ad.set_shading(shading)
    return ad


def the_surfaces(surfaces, n_lights, ka=0.4, kd=0.6):
    return sc.Surfaces(ISO, PLANES, 0.5, LIGHTS[:n_lights], ka=ka, kd=kd) if surfaces else lc.lights_only(LIGHTS[:n_lights], ka, kd)


@pytest.mark.parametrize("surfaces", [False, True])
@pytest.mark.parametrize("n_lights", [1, 3])
@pytest.mark.parametrize("moved", [False, True])
def test_trace_equals_the_checker(hip, moved, n_lights, surfaces):
    vol = grid()
    m = MOVED if moved else IDENT
    minv = scenes.instance_matrices(m)[0]
    t = tf("ramp")
    S = the_surfaces(surfaces, n_lights)
    ad = adapter(vol, t, 1.7, S)
    assert ad.shading() == capi.VOLUME_SHADE_GRADIENT
    rays = make_rays(vol, m, n=2000)
    rays["t"] = 123.0
    got = ad.trace(rays, m, minv)
    want = lc.march(vc.Brick(vol, t, 1.7), S, rays, minv)
    assert len(got) == len(rays)
    same_bits(got, want)
    print("samples shaded: device %d, checker %d" % (ad.shaded(), lc.march.shaded))
    assert ad.shaded() == lc.march.shaded > 1000
    unlit = adapter(vol, t, 1.7, S, shading=None)
    plain = unlit.trace(rays, m, minv)
    assert (plain["color"] != got["color"]).any() and unlit.shaded() == 0  # the lighting shows
    same_bits(plain, got, ("w", "t_min", "depth", "t"))  # opacity is not shaded


@pytest.mark.parametrize("surfaces", [False, True])
def test_identities_give_the_unlit_bits(hip, surfaces):
    vol = grid()
    t = tf("ramp")
    for m in (IDENT, MOVED):
        minv = scenes.instance_matrices(m)[0]
        rays = make_rays(vol, m, n=2000)
        rays["t"] = 123.0
        S = the_surfaces(surfaces, 3)
        want = adapter(vol, t, 1.7, S, shading=None).trace(rays, m, minv)  # never switched on
        off = adapter(vol, t, 1.7, S, shading=True)
        off.set_shading(False)
        same_bits(off.trace(rays, m, minv), want)
        assert off.shaded() == 0
        dark = adapter(vol, t, 1.7, the_surfaces(surfaces, 0), shading=True)  # on, no lights
        same_bits(dark.trace(rays, m, minv), adapter(vol, t, 1.7, the_surfaces(surfaces, 0), shading=None).trace(rays, m, minv))
        assert dark.shaded() == 0
        flat = adapter(vol, t, 1.7, the_surfaces(surfaces, 3, 1.0, 0.0), shading=True)  # shaded, to the same bits
        same_bits(flat.trace(rays, m, minv), adapter(vol, t, 1.7, the_surfaces(surfaces, 3, 1.0, 0.0), shading=None).trace(rays, m, minv))
        assert flat.shaded() > 1000
        if not surfaces:  # (ka and kd reach the plain march through shading only)
            same_bits(flat.trace(rays, m, minv), want)


@pytest.mark.parametrize("surfaces", [False, True])
def test_skipping_gives_the_same_bits(hip, surfaces):
    vol = grid(40)
    t = tf("spikes")
    S = sc.Surfaces([0.05, 0.93], PLANES[:1], 0.5, LIGHTS[:2]) if surfaces else lc.lights_only(LIGHTS[:2])
    a, b = adapter(vol, t, 1.0, S, skip=True), adapter(vol, t, 1.0, S, skip=False)
    rays = make_rays(vol, IDENT, n=4000, seed=11)
    ra, rb = a.trace(rays, IDENT, IDENT), b.trace(rays, IDENT, IDENT)
    same_bits(ra, rb)
    same_bits(ra, lc.march(vc.Brick(vol, t, 1.0), S, rays, IDENT))
    ia, ib = a.info(), b.info()
    print("shaded: skip %d, no skip %d, checker %d; gathered %d / %d" % (a.shaded(), b.shaded(), lc.march.shaded, ia["samples_gathered"], ib["samples_gathered"]))
    assert a.shaded() == b.shaded() == lc.march.shaded > 0
    assert ia["samples_marched"] == ib["samples_marched"] > 0
    assert ia["samples_gathered"] < ib["samples_gathered"] == ib["samples_marched"]


@pytest.fixture(scope="module")
def frame_case(hip):
    vol = grid(33)
    cam = camera(160, 128)
    t = tf("ramp")
    S = lc.lights_only(LIGHTS)
    B = vc.Brick(vol, t, 1.5)
    want, _ = lc.frame([B], B.lo[None], B.hi[None], IDENT, cam, S)
    return vol, cam, t, S, want, lc.frame.shaded


@pytest.mark.parametrize("split", [(1, 1, 1), (2, 2, 2), (3, 1, 2)])
def test_frames_equal_the_checker_whatever_the_bricking(frame_case, split):
    vol, cam, t, S, want, n_shaded = frame_case
    parts = vol if split == (1, 1, 1) else scenes.split_volume(vol, *split)
    tr = VolumeTracer(parts, cam, t, sampling_rate=1.5).set_lights(list(zip(S.lpos, S.lcol))).set_shading()
    got = tr.frame().framebuffer(False)
    assert tr.calls >= int(np.prod(split)) and tr.stats()["samples_shaded"] == n_shaded > 10000
    assert (got.view(np.uint32) == want.view(np.uint32)).all()
    unlit = tr.set_shading(False).frame().framebuffer(False)
    assert (unlit[..., :3] != got[..., :3]).any(axis=2).sum() > 2000 and (unlit[..., 3].view(np.uint32) == got[..., 3].view(np.uint32)).all()


@pytest.mark.parametrize("surfaces", [False, True])
def test_moved_bricked_frame_equals_the_checker(hip, surfaces):
    """MOVED, 25^3 at 96 x 80, split (2, 1, 2); once more with isovalues and a slice on."""
    vol = grid(25)
    cam = camera(96, 80)
    t = tf("ramp")
    S = sc.Surfaces(ISO, PLANES[:1], 0.5, LIGHTS) if surfaces else lc.lights_only(LIGHTS)
    parts = scenes.split_volume(vol, 2, 1, 2)
    tr = VolumeTracer(parts, cam, t, m=MOVED, sampling_rate=1.5).set_lights(list(zip(S.lpos, S.lcol))).set_shading()
    if surfaces:
        tr.set_surfaces(S.iso, S.planes, float(S.opacity))
    minv = scenes.instance_matrices(MOVED)[0]
    bricks = [vc.Brick(b, t, 1.5) for b in parts]
    want, calls = lc.frame(bricks, tr.inst_lo, tr.inst_hi, minv, cam, S)
    assert tr.frame().calls == calls
    assert (tr.framebuffer(False).view(np.uint32) == want.view(np.uint32)).all()
    st = tr.stats()
    assert st["samples_shaded"] == lc.frame.shaded > 10000 and (st["crossings_rendered"] > 100) == surfaces


def test_typed_voxels_are_lit_like_their_float_copy(hip):
    vol = quantised(grid(), "u8")
    t = scaled("ramp", "u8")
    S = lc.lights_only(LIGHTS)
    rays = make_rays(vol, MOVED, n=2000)
    minv = scenes.instance_matrices(MOVED)[0]
    typed, flt = adapter(vol, t, 1.7, S, native=True), adapter(as_float(vol), t, 1.7, S)
    assert typed.sample_bytes == 1 and flt.sample_bytes == 4
    got = typed.trace(rays, MOVED, minv)
    same_bits(got, flt.trace(rays, MOVED, minv))
    same_bits(got, lc.march(vc.Brick(as_float(vol), t, 1.7), S, rays, minv))
    assert typed.shaded() == flt.shaded() == lc.march.shaded > 1000


@pytest.fixture(scope="module")
def clip_case(hip):
    vol = grid(25)
    cam = camera(96, 80)
    y, x = np.mgrid[0:80, 0:96]
    keep = (x // 10 + y // 10) % 3 != 0
    plane = cc.depth_of_plane(cam, (0.3, 0.2, 1.0), 0.3 * 0.25 + 0.2 * 0.65 + 0.05, keep)  # through the grid's middle
    return vol, cam, plane, tf("ramp"), lc.lights_only(LIGHTS)


def test_clipped_lit_frame_equals_the_checker(clip_case):
    vol, cam, plane, t, S = clip_case
    parts = scenes.split_volume(vol, 2, 2, 1)
    depth = DepthPlane(cam.width, cam.height).upload(plane)
    tr = VolumeTracer(parts, cam, t, sampling_rate=1.5).set_lights(list(zip(S.lpos, S.lcol))).set_shading()
    got = tr.frame(depth).framebuffer(False)
    bricks = [vc.Brick(b, t, 1.5) for b in parts]
    want, calls = lc.frame(bricks, tr.inst_lo, tr.inst_hi, IDENT, cam, S, plane=plane)
    assert tr.calls == calls >= 4
    assert (got.view(np.uint32) == want.view(np.uint32)).all()
    assert tr.stats()["samples_shaded"] == lc.frame.shaded > 10000
    whole, _ = lc.frame(bricks, tr.inst_lo, tr.inst_hi, IDENT, cam, S)
    assert (got[..., 3] < whole[..., 3]).sum() > 300  # the clip shows


def test_mixed_tracer_passes_the_shading_through(hip):
    cam = scenes.Camera((0.0, 0.1, 0.3), (0.0, 0.1, -0.3), (0.0, 1.0, 0.0), float(F(45.0 * np.pi / 180.0)), 96, 80)
    scene = scenes.bunny_scene(96, 80)
    vol = scenes.mesh_in_volume(scene, scenes.sphere_volume(32), fill=0.6)
    t = tf("ramp")
    S = lc.lights_only(LIGHTS)
    mt = MixedTracer(scene, vol, cam, t, sampling_rate=1.0).set_lights(list(zip(S.lpos, S.lcol)))
    unlit = mt.frame().framebuffer(False).copy()
    got = mt.set_shading().frame().framebuffer(False).copy()  # the frame returns ...
    assert np.isfinite(got).all() and (got[..., :3] != unlit[..., :3]).any(axis=2).sum() > 500
    assert mt.volume.stats()["samples_shaded"] > 10000
    depth = mt.depth.download()
    fog = mt.volume.frame(mt.depth).framebuffer(False)  # ... and its volume part is the clipped lit frame
    B = vc.Brick(vol, t, 1.0)
    want, _ = lc.frame([B], B.lo[None], B.hi[None], IDENT, cam, S, plane=depth)
    assert (fog.view(np.uint32) == want.view(np.uint32)).all()
    assert (got.view(np.uint32) == cc.composite(want, mt.mesh_framebuffer(False), depth).view(np.uint32)).all()


def test_grids_that_are_not_finite_stay_finite_in_colour(hip):
    vol = grid(12)
    vol.data[5, 5, 5] = np.nan
    vol.data[6, 3, 7] = np.inf
    vol.data[3, 7, 4], vol.data[3, 7, 5] = 3e38, -3e38
    t = tf("cool")
    S = lc.lights_only(LIGHTS)
    rays = make_rays(vol, IDENT, n=2000)
    a, b = adapter(vol, t, 1.7, S, skip=True), adapter(vol, t, 1.7, S, skip=False)
    ra, rb = a.trace(rays, IDENT, IDENT), b.trace(rays, IDENT, IDENT)
    same_bits(ra, rb)
    same_bits(ra, lc.march(vc.Brick(vol, t, 1.7), S, rays, IDENT))
    assert a.shaded() == b.shaded() == lc.march.shaded > 1000
    assert np.isfinite(ra["color"]).all() and np.isfinite(ra["w"]).all()
    unlit = adapter(vol, t, 1.7, S, shading=None).trace(rays, IDENT, IDENT)
    assert (unlit["color"] != ra["color"]).any()


def test_unknown_modes_are_refused(hip):
    ad = HipVolumeAdapter(grid(8), 1.0)
    lib = capi.load()
    assert ad.shading() == capi.VOLUME_SHADE_NONE
    for now in (capi.VOLUME_SHADE_NONE, capi.VOLUME_SHADE_GRADIENT):
        assert lib.gvt_hip_volume_set_shading(ad.h, now) == 0
        for bad in (2, -1):
            assert lib.gvt_hip_volume_set_shading(ad.h, bad) == -1 and "mode" in capi.last_error()
            assert ad.shading() == now
    assert lib.gvt_hip_volume_set_shading(None, 1) == -1 and lib.gvt_hip_volume_get_shading(ad.h, None) == -1
    assert lib.gvt_hip_volume_get_shaded(ad.h, None) == -1
