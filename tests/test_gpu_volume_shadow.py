"""Shadowed surfaces on the device (csrc/volume_fused_shadow.inc, gvt_hip_volume_frame_shadowed) against the numpy checker
(tests/volume_shadow_checker.py), bit for bit: the main case of tests/volume_shadow_cases.py in every bricking at both eyes with the shadow
rays' counters, the skip flag, typed voxels, the clipped and the mixed frame, lit fog beside shadowed crossings, the identity and the
occluder properties, the inert frames and the refusals."""
import ctypes as C

import numpy as np
import pytest

from gravit_amd import capi, scenes
from gravit_amd.adapter import DepthPlane
from gravit_amd.scheduler import MixedTracer, NativeTracer, VolumeTracer
from tests import volume_checker as vc
from tests import volume_clip_checker as cc
from tests import volume_fused_cases as fc
from tests import volume_shade_checker as lc
from tests import volume_shadow_cases as swc
from tests import volume_shadow_checker as sw
from tests import volume_surface_checker as sc
from tests.volume_common import as_float, quantised, scaled, tf

pytestmark = pytest.mark.gpu

F = np.float32
BOTH = capi.FUSED_SURFACES | capi.FUSED_LIT
N_PIX = fc.FILM[0] * fc.FILM[1]
SHADOW_KEYS = ("shadow_rays", "shadow_brick_visits", "shadow_crossings")
CAMERA_KEYS = ("brick_visits", "rays_deposited", "crossings_rendered", "samples_shaded")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def dress(tr, S, on):
    if len(S):
        tr.set_surfaces(S.iso, S.planes, float(S.opacity))
    tr.set_lights(list(zip(S.lpos, S.lcol)), float(S.ka), float(S.kd))
    tr.set_shading(on)
    return tr


def tracer(case, split, where, mode="surf", moved=None, skip=True, shadows=True, bias=swc.BIAS, vol=None, native=False, t=None, S=None, kd=0.6, parts=None):
    moved = swc.CAMERAS[where] if moved is None else moved
    S0, on, table = swc.surfaces(case, mode, kd=kd)
    if parts is None:
        parts = fc.bricks_of(fc.volume() if vol is None else vol, split)
    tr = VolumeTracer(parts, fc.camera(where, moved), table if t is None else t, m=fc.matrix(moved), sampling_rate=fc.RATE, skip=skip, native=native,
                      fused=True, fused_shaded=True, shadows=shadows, shadow_bias=bias)
    return dress(tr, S0 if S is None else S, on)


@pytest.mark.parametrize("where", sorted(swc.CAMERAS))
@pytest.mark.parametrize("split", fc.SPLITS)
def test_shadowed_frame_has_the_checkers_bits_and_counts(hip, split, where):
    want, counters, _, _ = swc.reference("main", split, where)
    tr = tracer("main", split, where).frame()
    got, st = tr.framebuffer(False), tr.stats()
    assert st["shadowed"] == 1 and st["fused"] == 1 and st["adapter_calls"] == 1 and st["features"] == capi.FUSED_SURFACES
    assert got.any()
    assert (bits(got) == bits(want)).all()
    for key in SHADOW_KEYS + CAMERA_KEYS:
        assert st[key] == counters[key], key
    assert st["shadow_rays"] > 0 and st["shadow_samples_marched"] >= st["shadow_samples_gathered"] > 0
    assert all(len(q) == 0 for q in tr.queues)


@pytest.mark.parametrize("where", sorted(swc.CAMERAS))
def test_the_cut_does_not_show(hip, where):
    frames = [tracer("main", s, where).frame().framebuffer(False).copy() for s in fc.SPLITS]
    for f in frames[1:]:
        assert (bits(f) == bits(frames[0])).all()


@pytest.mark.parametrize("split", [(1, 1, 1), (4, 4, 4)])
def test_skipping_does_not_show(hip, split):
    a = tracer("main", split, "inside").frame()
    b = tracer("main", split, "inside", skip=False).frame()
    sa, sb = a.stats(), b.stats()
    assert (bits(a.framebuffer(False)) == bits(b.framebuffer(False))).all()
    assert sa["shadow_samples_marched"] == sb["shadow_samples_marched"] > 0 and sa["samples_marched"] == sb["samples_marched"]
    assert sb["shadow_samples_gathered"] == sb["shadow_samples_marched"] and sb["samples_gathered"] == sb["samples_marched"]
    assert sa["shadow_samples_gathered"] <= sa["shadow_samples_marched"]
    for key in SHADOW_KEYS:
        assert sa[key] == sb[key], key
    # a sparse table, where whole macro cells are skipped: the same holds
    c = tracer("main", split, "inside", mode="surf_lit").frame()
    d = tracer("main", split, "inside", mode="surf_lit", skip=False).frame()
    sc_, sd = c.stats(), d.stats()
    assert (bits(c.framebuffer(False)) == bits(d.framebuffer(False))).all()
    assert sc_["shadow_samples_marched"] == sd["shadow_samples_marched"] == sd["shadow_samples_gathered"] >= sc_["shadow_samples_gathered"] > 0


def test_typed_voxels(hip):
    vol, t = quantised(fc.volume(), "u8"), scaled("cool", "u8")
    S, on, _ = swc.surfaces("main", "surf", scale=255.0)
    tr = tracer("main", (2, 2, 2), "inside", vol=vol, native=True, t=t, S=S).frame()
    st = tr.stats()
    assert tr.adapters[0].dtype_name == "uint8" and st["shadowed"] == 1 and st["shadow_rays"] > 0
    flt = tracer("main", (2, 2, 2), "inside", vol=as_float(vol), t=t, S=S).frame()
    assert tr.framebuffer(False).any()
    assert (bits(tr.framebuffer(False)) == bits(flt.framebuffer(False))).all()
    for key in SHADOW_KEYS + ("shadow_samples_marched", "shadow_samples_gathered"):
        assert st[key] == flt.stats()[key], key


def test_clipped_shadowed_frame(hip):
    want, counters, _, plane = swc.reference("main", (2, 2, 2), "outside", clipped=True)
    depth = DepthPlane(fc.FILM[0], fc.FILM[1]).upload(plane)
    tr = tracer("main", (2, 2, 2), "outside", moved=False).frame(depth)
    got, st = tr.framebuffer(False).copy(), tr.stats()
    assert st["shadowed"] == 1
    assert (bits(got) == bits(want)).all()
    for key in SHADOW_KEYS + CAMERA_KEYS:
        assert st[key] == counters[key], key
    assert (bits(got) != bits(tr.frame().framebuffer(False))).any()  # the clip shows


def test_mixed_frame(hip):
    """The volume's surfaces shadowed by the volume, clipped at the scene's depth plane and composited over the meshes."""
    w, h = 64, 48
    cam = scenes.Camera((0.0, 0.1, 0.3), (0.0, 0.1, -0.3), (0.0, 1.0, 0.0), float(F(45.0 * np.pi / 180.0)), w, h)
    scene = scenes.bunny_scene(w, h)
    vol = scenes.mesh_in_volume(scene, scenes.sphere_volume(32), fill=0.6)
    parts = scenes.split_volume(vol, 2, 2, 2)
    t = tf("ramp")
    S = sc.Surfaces([0.3, 0.5], [], 0.6, swc.LIGHTS)
    mt = MixedTracer(scene, parts, cam, t, sampling_rate=1.0, shadows=True)
    mt.set_surfaces(S.iso, S.planes, float(S.opacity)).set_lights(list(zip(S.lpos, S.lcol)))
    mt.frame()
    st = mt.volume.stats()
    assert st["shadowed"] == 1 and st["shadow_rays"] > 0 and mt.volume.calls == 1
    depth = mt.depth.download().copy()
    mesh = NativeTracer(scene)().framebuffer(False)
    bricks = [vc.Brick(b, t, 1.0) for b in parts]
    lo, hi = fc.world_boxes(parts, fc.matrix(False))
    fog, counters, _ = sw.frame(bricks, lo, hi, scenes.instance_matrices(fc.matrix(False))[0], cam, S, lc.SHADE_NONE, depth, swc.BIAS)
    want = cc.composite(fog, mesh, depth)
    assert (bits(mt.framebuffer(False)) == bits(want)).all()
    for key in SHADOW_KEYS:
        assert st[key] == counters[key], key
    assert np.isfinite(depth).sum() > 100 and counters["shadow_crossings"] > 0


@pytest.mark.parametrize("split", [(2, 2, 2), (4, 4, 4)])
def test_lit_fog_beside_shadowed_crossings(hip, split):
    want, counters, _, _ = swc.reference("main", split, "inside", mode="surf_lit")
    tr = tracer("main", split, "inside", mode="surf_lit").frame()
    st = tr.stats()
    assert st["shadowed"] == 1 and st["features"] == BOTH and st["samples_shaded"] > 0
    assert (bits(tr.framebuffer(False)) == bits(want)).all()
    for key in SHADOW_KEYS + CAMERA_KEYS:
        assert st[key] == counters[key], key
    plain = tracer("main", split, "inside", mode="surf_lit", shadows=False).frame()
    assert (bits(tr.framebuffer(False)) != bits(plain.framebuffer(False))).any()  # the shadows show
    for key in CAMERA_KEYS + ("samples_marched", "samples_gathered"):  # the fog is lit as before; the camera rays' counters do not move
        assert st[key] == plain.stats()[key], key


def test_identity_case(hip):
    """No shadow ray meets a crossing: the bits and the camera rays' counters are the unshadowed frame's."""
    tr = tracer("identity", (2, 2, 2), "outside", moved=False).frame()
    got, st = tr.framebuffer(False).copy(), tr.stats()
    want, counters, _, _ = swc.reference("identity", (2, 2, 2), "outside", moved=False)
    assert (bits(got) == bits(want)).all() and got.any()
    assert st["shadowed"] == 1 and st["shadow_rays"] == counters["shadow_rays"] > 500 and st["shadow_crossings"] == 0
    assert st["shadow_brick_visits"] == counters["shadow_brick_visits"]
    plain = tracer("identity", (2, 2, 2), "outside", moved=False, shadows=False).frame()
    ps = plain.stats()
    assert (bits(got) == bits(plain.framebuffer(False))).all()
    for key in CAMERA_KEYS + ("samples_marched", "samples_gathered", "fused", "features", "adapter_calls"):
        assert st[key] == ps[key], key


def test_occluder_case(hip):
    """Where every light is blocked a pixel has the bits of the frame rendered with kd = 0."""
    want, _, details, _ = swc.reference("occluder", (2, 2, 2), "outside", moved=False)
    has, dark = swc.fully_shadowed(details, N_PIX)
    assert dark.sum() >= 0.5 * has.sum() > 250
    got = tracer("occluder", (2, 2, 2), "outside", moved=False).frame().framebuffer(False).copy()
    assert (bits(got) == bits(want)).all()
    ambient = tracer("occluder", (2, 2, 2), "outside", moved=False, shadows=False, kd=0.0).frame().framebuffer(False).copy()
    plain = tracer("occluder", (2, 2, 2), "outside", moved=False, shadows=False).frame().framebuffer(False)
    g, a, p = bits(got).reshape(-1, 4), bits(ambient).reshape(-1, 4), bits(plain).reshape(-1, 4)
    assert (g[dark] == a[dark]).all() and (g[dark] != p[dark]).any(axis=-1).all()
    assert (g[has & ~dark] == p[has & ~dark]).all()


def test_bias_shows(hip):
    one, c1, _, _ = swc.reference("main", (2, 2, 2), "outside", bias=1)
    tr = tracer("main", (2, 2, 2), "outside", bias=1).frame()
    assert (bits(tr.framebuffer(False)) == bits(one)).all()
    for key in SHADOW_KEYS:
        assert tr.stats()[key] == c1[key], key
    two = tracer("main", (2, 2, 2), "outside").frame().framebuffer(False)
    assert (bits(two) != bits(one)).any()
    far = tracer("main", (2, 2, 2), "outside", bias=64).frame()  # the largest bias is taken
    assert far.stats()["shadowed"] == 1


@pytest.mark.parametrize("what", ["no lights", "no surfaces", "plain"])
def test_inert_frames_are_the_shaded_fused_frames(hip, what):
    S, on, _ = swc.surfaces("main", "surf_lit")
    if what == "no lights":
        S = sc.Surfaces(S.iso, S.planes, S.opacity, ())
    elif what == "no surfaces":
        S = lc.lights_only(swc.LIGHTS)
    tr = tracer("main", (2, 2, 2), "inside", mode="surf_lit", S=S)
    if what == "plain":
        tr.set_surfaces().set_lights([]).set_shading(False)
    got, st = tr.frame().framebuffer(False).copy(), tr.stats()
    assert st["shadowed"] == 0 and all(st[k] == 0 for k in SHADOW_KEYS + ("shadow_samples_marched", "shadow_samples_gathered"))
    tr.shadows = False
    want, ws = tr.frame().framebuffer(False), tr.stats()
    assert (bits(got) == bits(want)).all() and got.any()
    assert st["features"] == ws["features"] == {"no lights": capi.FUSED_SURFACES, "no surfaces": capi.FUSED_LIT, "plain": 0}[what]
    for key in CAMERA_KEYS + ("samples_marched", "samples_gathered", "fused", "adapter_calls"):
        assert st[key] == ws[key], key
    assert st["fused"] == 1


def test_inert_frame_falls_back_to_the_loop(hip):
    """No lights, and a bricking the fused kernel does not take (another table on one brick): the loop, as gvt_hip_volume_frame_fused_shaded."""
    S, on, _ = swc.surfaces("main", "surf")
    tr = tracer("main", (2, 2, 2), "inside", S=sc.Surfaces(S.iso, S.planes, S.opacity, ()))
    tr.adapters[3].set_transfer(tf("spikes"))
    got, st = tr.frame().framebuffer(False).copy(), tr.stats()
    assert st["shadowed"] == 0 and st["fused"] == 0 and st["adapter_calls"] > 1
    tr.shadows = False
    assert (bits(got) == bits(tr.frame().framebuffer(False))).all() and tr.stats()["adapter_calls"] == st["adapter_calls"]


def _upload_fb(fb, img):
    """Put an image into a framebuffer (the library has no host path into one: a plain copy through the runtime it is linked against)."""
    src = capi.f32(img)
    capi.synchronize()
    rt = C.CDLL("libamdhip64.so")
    rt.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert src.nbytes == fb.w * fb.hgt * 16
    assert rt.hipMemcpy(fb.device_ptr(), capi.ptr(src), src.nbytes, 1) == 0  # hipMemcpyHostToDevice


def _raw(tr, params, stats=None):
    cam = tr.camera
    pod = capi.CameraPod((C.c_float * 3)(*cam.eye), (C.c_float * 3)(*cam.focus), (C.c_float * 3)(*cam.up), cam.fov, cam.width, cam.height, 1, 1, 0.0)
    m = np.ascontiguousarray(np.tile(tr.m, tr.n_inst), F)
    minv = np.ascontiguousarray(np.tile(tr.minv, tr.n_inst), F)
    return capi.load().gvt_hip_volume_frame_shadowed(tr.top.h, tr._arr(tr.adapters), capi.ptr(m), capi.ptr(minv), C.c_size_t(tr.n_inst), C.byref(pod), tr._arr(tr.queues),
                                                     tr.fb.h, None, None if params is None else C.byref(params), None if stats is None else C.byref(stats))


def test_refusals_change_nothing(hip):
    pattern = np.random.default_rng(11).random((fc.FILM[1], fc.FILM[0], 4)).astype(F)

    def refused(tr, word):
        _upload_fb(tr.fb, pattern)
        with pytest.raises(capi.GvtHipError, match=r"\(-1\)") as e:
            tr.frame()
        assert word in str(e.value), str(e.value)
        assert (bits(tr.framebuffer(False)) == bits(pattern)).all() and all(len(q) == 0 for q in tr.queues)

    # an AMR brick
    tr = VolumeTracer(fc.bricks_of(fc.volume(), (2, 2, 2)), fc.camera("inside", False), tf("cool"), m=fc.matrix(False), sampling_rate=fc.RATE, shadows=True)
    S, on, _ = swc.surfaces("main", "surf")
    for a in tr.adapters[1:]:  # (a brick with subgrids takes no surfaces: the others have them, and the lights)
        a.set_surfaces(S.iso, S.planes, float(S.opacity))
        a.set_lights(list(zip(S.lpos, S.lcol)))
    b = fc.bricks_of(fc.volume(), (2, 2, 2))[0]
    scenes.refine(b, np.asarray(b.offset) + 1, (2, 2, 2), 2, seed=5)
    tr.adapters[0].set_subgrids(b.subgrids)
    refused(tr, "subgrids")
    # CENTRAL on a frame with an isovalue
    tr = tracer("main", (2, 2, 2), "inside", parts=scenes.split_volume(fc.volume(), 2, 2, 2, ghosts=True))
    assert tr.frame().stats()["shadowed"] == 1
    tr.set_gradient("central")
    refused(tr, "central")
    # two bricks with different tables
    tr = tracer("main", (2, 2, 2), "inside")
    tr.adapters[5].set_transfer(tf("spikes"))
    refused(tr, "transfer")
    # the parameters
    tr = tracer("main", (2, 2, 2), "inside")
    _upload_fb(tr.fb, pattern)
    for params, word in ((capi.VolumeShadowParams(0, 0), "bias"), (capi.VolumeShadowParams(0, 65), "bias"), (capi.VolumeShadowParams(1, 2), "flag"), (None, "null")):
        st = capi.VolumeShadowStats(fused=77, shadowed=78, shadow_rays=79)
        assert _raw(tr, params, st) == -1
        assert word in capi.last_error(), capi.last_error()
        assert (st.fused, st.shadowed, st.shadow_rays) == (77, 78, 79)
        assert (bits(tr.framebuffer(False)) == bits(pattern)).all()
    assert capi.load().gvt_hip_volume_frame_shadowed(None, None, None, None, 0, None, None, None, None, None, None) == -1  # volume_frame_args' errors
    assert _raw(tr, capi.VolumeShadowParams(0, 2)) == 0  # stats may be NULL
    assert (bits(tr.framebuffer(False)) == bits(swc.reference("main", (2, 2, 2), "inside")[0])).all()
