"""Shadowed fog on the device (csrc/volume_light_grid.inc, csrc/volume_fused_fog.inc; gvt_hip_volume_light_grid_bake and
gvt_hip_volume_frame_fog_shadowed) against the numpy checker (tests/volume_fog_shadow_checker.py), bit for bit: the baked grids in every
bricking under both matrices and under lights parallel to a grid plane, the frame of both cases of tests/volume_fog_shadow_cases.py in
every bricking at both eyes, the cut, the skip flag, typed voxels, the clipped and the mixed frame, the inert frames, stale grids, the
bake's refusals, a new time step, and the untouched entry points."""
import ctypes as C

import numpy as np
import pytest

from gravit_amd import capi, scenes
from gravit_amd.adapter import DepthPlane
from gravit_amd.scheduler import MixedTracer, NativeTracer, VolumeTracer
from tests import volume_checker as vc
from tests import volume_clip_checker as cc
from tests import volume_fog_shadow_cases as fgc
from tests import volume_fog_shadow_checker as fg
from tests import volume_fused_cases as fc
from tests import volume_shade_checker as lc
from tests import volume_shadow_cases as swc
from tests import volume_surface_checker as sc
from tests.volume_common import as_float, quantised, scaled, tf

pytestmark = pytest.mark.gpu

F = np.float32
BOTH = capi.FUSED_SURFACES | capi.FUSED_LIT
FEATURES = {"lit": capi.FUSED_LIT, "surf_lit": BOTH}
SHADOW_KEYS = ("shadow_rays", "shadow_brick_visits", "shadow_crossings")
CAMERA_KEYS = ("brick_visits", "rays_deposited", "crossings_rendered", "samples_shaded")
PARALLEL_LIGHTS = tuple((p, fgc.WHITE) for p in fgc.PARALLEL)
N_VERT = fc.N ** 3


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def dress(tr, S, on):
    if len(S):
        tr.set_surfaces(S.iso, S.planes, float(S.opacity))
    tr.set_lights(list(zip(S.lpos, S.lcol)), float(S.ka), float(S.kd))
    tr.set_shading(on)
    return tr


def tracer(mode, split, where, moved=None, skip=True, fog=True, shadows=True, vol=None, native=False, t=None, S=None, kd=0.6, parts=None, lights=None):
    moved = fgc.CAMERAS[where] if moved is None else moved
    S0, on, table = swc.surfaces("main", mode, kd=kd)
    if lights is not None:
        S0 = fgc.with_lights(S0, lights)
    if parts is None:
        parts = fc.bricks_of(fc.volume() if vol is None else vol, split)
    tr = VolumeTracer(parts, fc.camera(where, moved), table if t is None else t, m=fc.matrix(moved), sampling_rate=fc.RATE, skip=skip, native=native,
                      fused=True, fused_shaded=True, shadows=shadows, shadow_bias=fgc.BIAS, fog_shadows=fog and shadows, fog_bias=fgc.GRID_BIAS)
    return dress(tr, S0 if S is None else S, on)


def grids_match(tr, G, usable):
    """Every brick's downloaded planes are its part of the checker's grid."""
    for a in tr.adapters:
        o, n = a.offset, a.counts
        for j in np.nonzero(usable)[0]:
            want = G[j, o[2]:o[2] + n[2], o[1]:o[1] + n[1], o[0]:o[0] + n[0]]
            if not (bits(a.light_grid(int(j))) == bits(want)).all():
                return False
    return True


@pytest.mark.parametrize("moved", [False, True])
@pytest.mark.parametrize("split", fc.SPLITS)
@pytest.mark.parametrize("mode", fgc.MODES)
def test_baked_grid_has_the_checkers_bits(hip, mode, split, moved):
    G, usable = fgc.light_grid(mode, moved)
    tr = tracer(mode, split, "outside", moved=moved).rebake()
    st = tr.stats()
    assert grids_match(tr, G, usable)
    n_vert = sum(int(np.prod(a.counts)) for a in tr.adapters)
    assert st["light_bakes"] == 1 and st["light_grid_rays"] == 2 * n_vert and st["light_grid_bytes"] == 8 * n_vert and st["light_grid_ms"] > 0
    g = tr.light_grid_stats
    assert 0 < g["samples_gathered"] <= g["samples_marched"]
    assert (g["crossings"] > 0) == (mode == "surf_lit")
    for a in tr.adapters:
        assert a.light_grid_info() == {"present": 1, "current": 1, "n_planes": 2, "bias": fgc.GRID_BIAS, "bytes": 8 * int(np.prod(a.counts))}
    plain = tracer(mode, split, "outside", moved=moved, skip=False).rebake()
    p = plain.light_grid_stats
    assert grids_match(plain, G, usable)
    assert p["samples_gathered"] == p["samples_marched"] == g["samples_marched"] and p["crossings"] == g["crossings"] and p["rays"] == g["rays"]


@pytest.mark.parametrize("split", fc.SPLITS)
@pytest.mark.parametrize("mode", fgc.MODES)
def test_lights_parallel_to_a_grid_plane(hip, mode, split):
    """The test the finding asks for: rays that run in brick faces get the one brick's value in every bricking."""
    G, usable = fgc.light_grid(mode, False, PARALLEL_LIGHTS)
    tr = tracer(mode, split, "outside", moved=False, lights=PARALLEL_LIGHTS).rebake()
    assert usable.all() and tr.light_grid_stats["rays"] == 3 * sum(int(np.prod(a.counts)) for a in tr.adapters)
    assert grids_match(tr, G, usable)


@pytest.mark.parametrize("where", sorted(fgc.CAMERAS))
@pytest.mark.parametrize("split", fc.SPLITS)
@pytest.mark.parametrize("mode", fgc.MODES)
def test_fog_shadowed_frame_has_the_checkers_bits_and_counts(hip, mode, split, where):
    want, counters, _ = fgc.reference(mode, split, where)
    tr = tracer(mode, split, where).frame()
    got, st = tr.framebuffer(False), tr.stats()
    assert st["shadowed"] == 1 and st["fused"] == 1 and st["adapter_calls"] == 1 and st["features"] == FEATURES[mode] and st["light_bakes"] == 1
    assert got.any()
    assert (bits(got) == bits(want)).all()
    for key in SHADOW_KEYS + CAMERA_KEYS:
        assert st[key] == counters[key], key
    assert st["fog_samples_shadowed"] == st["samples_shaded"] > 0
    assert (st["shadow_rays"] > 0) == (mode == "surf_lit")
    assert all(len(q) == 0 for q in tr.queues)
    plain, _ = fgc.unshadowed(mode, split, where) if split == (2, 2, 2) else (None, None)
    if plain is not None:
        assert (bits(got) != bits(plain)).any()  # the shadows show


@pytest.mark.parametrize("where", sorted(fgc.CAMERAS))
@pytest.mark.parametrize("mode", fgc.MODES)
def test_the_cut_does_not_show(hip, mode, where):
    frames = [tracer(mode, s, where).frame().framebuffer(False).copy() for s in fc.SPLITS]
    for f in frames[1:]:
        assert (bits(f) == bits(frames[0])).all()


@pytest.mark.parametrize("split", [(1, 1, 1), (4, 4, 4)])
@pytest.mark.parametrize("mode", fgc.MODES)
def test_skipping_does_not_show(hip, mode, split):
    a = tracer(mode, split, "inside").frame()
    b = tracer(mode, split, "inside", skip=False).frame()
    sa, sb = a.stats(), b.stats()
    assert (bits(a.framebuffer(False)) == bits(b.framebuffer(False))).all()
    assert sa["samples_marched"] == sb["samples_marched"] == sb["samples_gathered"] >= sa["samples_gathered"] > 0
    assert sa["samples_shaded"] == sb["samples_shaded"] == sa["fog_samples_shadowed"] == sb["fog_samples_shadowed"] > 0
    for key in SHADOW_KEYS + ("shadow_samples_marched",):
        assert sa[key] == sb[key], key


def test_typed_voxels(hip):
    vol, t = quantised(fc.volume(), "u8"), scaled("spikes", "u8")
    S, on, _ = swc.surfaces("main", "surf_lit", scale=255.0)
    tr = tracer("surf_lit", (2, 2, 2), "inside", vol=vol, native=True, t=t, S=S).frame()
    st = tr.stats()
    assert tr.adapters[0].dtype_name == "uint8" and st["shadowed"] == 1 and st["shadow_rays"] > 0 and st["fog_samples_shadowed"] > 0
    flt = tracer("surf_lit", (2, 2, 2), "inside", vol=as_float(vol), t=t, S=S).frame()
    assert tr.framebuffer(False).any()
    assert (bits(tr.framebuffer(False)) == bits(flt.framebuffer(False))).all()
    for a, b in zip(tr.adapters, flt.adapters):
        for j in range(2):
            assert (bits(a.light_grid(j)) == bits(b.light_grid(j))).all()
    for key in SHADOW_KEYS + CAMERA_KEYS + ("fog_samples_shadowed", "light_grid_rays"):
        assert st[key] == flt.stats()[key], key
    assert tr.light_grid_stats["samples_marched"] == flt.light_grid_stats["samples_marched"]


@pytest.mark.parametrize("mode", fgc.MODES)
def test_clipped_frame(hip, mode):
    want, counters, plane = fgc.reference(mode, (2, 2, 2), "outside", clipped=True)
    depth = DepthPlane(fc.FILM[0], fc.FILM[1]).upload(plane)
    tr = tracer(mode, (2, 2, 2), "outside", moved=False).frame(depth)
    got, st = tr.framebuffer(False).copy(), tr.stats()
    assert st["shadowed"] == 1 and st["fog_samples_shadowed"] == st["samples_shaded"] > 0
    assert (bits(got) == bits(want)).all()
    for key in SHADOW_KEYS + CAMERA_KEYS:
        assert st[key] == counters[key], key
    assert (bits(got) != bits(tr.frame().framebuffer(False))).any()  # the clip shows
    assert tr.stats()["light_bakes"] == 1  # (the camera's clip does not touch the grid)


def test_mixed_frame(hip):
    """The volume's surfaces and its lit fog shadowed by the volume, clipped at the scene's depth plane and composited over the meshes."""
    w, h = 64, 48
    cam = scenes.Camera((0.0, 0.1, 0.3), (0.0, 0.1, -0.3), (0.0, 1.0, 0.0), float(F(45.0 * np.pi / 180.0)), w, h)
    scene = scenes.bunny_scene(w, h)
    vol = scenes.mesh_in_volume(scene, scenes.sphere_volume(32), fill=0.6)
    parts = scenes.split_volume(vol, 2, 2, 2)
    t = tf("ramp")
    S = sc.Surfaces([0.3, 0.5], [], 0.6, swc.LIGHTS)
    mt = MixedTracer(scene, parts, cam, t, sampling_rate=1.0, shadows=True, fog_shadows=True)
    mt.set_surfaces(S.iso, S.planes, float(S.opacity)).set_lights(list(zip(S.lpos, S.lcol))).set_shading(True)
    mt.frame()
    st = mt.volume.stats()
    assert st["shadowed"] == 1 and st["shadow_rays"] > 0 and st["fog_samples_shadowed"] == st["samples_shaded"] > 0 and mt.volume.calls == 1 and st["light_bakes"] == 1
    depth = mt.depth.download().copy()
    mesh = NativeTracer(scene)().framebuffer(False)
    m = fc.matrix(False)
    minv = scenes.instance_matrices(m)[0]
    bricks = [vc.Brick(b, t, 1.0) for b in parts]
    lo, hi = fc.world_boxes(parts, m)
    wlo, whi = fc.world_boxes([vol], m)
    G, _ = fg.grid(vc.Brick(vol, t, 1.0), wlo, whi, m, minv, S, 1)
    fog, counters = fg.frame(bricks, lo, hi, minv, cam, S, lc.SHADE_GRADIENT, G, depth, swc.BIAS)
    want = cc.composite(fog, mesh, depth)
    assert (bits(mt.framebuffer(False)) == bits(want)).all()
    for key in SHADOW_KEYS + ("samples_shaded",):
        assert st[key] == counters[key], key
    assert np.isfinite(depth).sum() > 100 and counters["shadow_crossings"] > 0


@pytest.mark.parametrize("mode", fgc.MODES)
def test_without_diffuse_light_no_shadow_shows(hip, mode):
    """kd = 0: the frame is gvt_hip_volume_frame_fused_shaded's kd = 0 frame."""
    got = tracer(mode, (2, 2, 2), "inside", kd=0.0).frame()
    want = tracer(mode, (2, 2, 2), "inside", kd=0.0, shadows=False).frame()
    assert got.stats()["fog_samples_shadowed"] > 0 and want.stats()["fused"] == 1
    assert (bits(got.framebuffer(False)) == bits(want.framebuffer(False))).all() and got.framebuffer(False).any()


def test_without_lit_fog_the_frame_is_the_shadowed_frame(hip):
    """Mode "surf": gvt_hip_volume_frame_shadowed in every bit, and nothing is baked."""
    tr = tracer("surf", (2, 2, 2), "inside").frame()
    want = tracer("surf", (2, 2, 2), "inside", fog=False).frame()
    st, ws = tr.stats(), want.stats()
    assert (bits(tr.framebuffer(False)) == bits(want.framebuffer(False))).all() and tr.framebuffer(False).any()
    assert st["light_bakes"] == 0 and st["fog_samples_shadowed"] == 0 and st["shadowed"] == 1 and st["features"] == capi.FUSED_SURFACES
    assert all(a.light_grid_info()["present"] == 0 for a in tr.adapters)
    for key in SHADOW_KEYS + CAMERA_KEYS + ("samples_marched", "samples_gathered", "shadow_samples_marched", "shadow_samples_gathered"):
        assert st[key] == ws[key], key
    with pytest.raises(capi.GvtHipError, match="no light grid"):
        tr.adapters[0].light_grid(0)


def _upload_fb(fb, img):
    """Put an image into a framebuffer (the library has no host path into one: a plain copy through the runtime it is linked against)."""
    src = capi.f32(img)
    capi.synchronize()
    rt = C.CDLL("libamdhip64.so")
    rt.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert src.nbytes == fb.w * fb.hgt * 16
    assert rt.hipMemcpy(fb.device_ptr(), capi.ptr(src), src.nbytes, 1) == 0  # hipMemcpyHostToDevice


def _raw_frame(tr, adapters=None, m=None):
    """gvt_hip_volume_frame_fog_shadowed on tr's top level, queues and framebuffer with other volumes or another matrix."""
    cam = tr.camera
    adapters = tr.adapters if adapters is None else adapters
    n = len(adapters)
    pod = capi.CameraPod((C.c_float * 3)(*cam.eye), (C.c_float * 3)(*cam.focus), (C.c_float * 3)(*cam.up), cam.fov, cam.width, cam.height, 1, 1, 0.0)
    m1 = capi.f32(tr.m if m is None else m, 16)
    mm = np.ascontiguousarray(np.tile(m1, n), F)
    minv = np.ascontiguousarray(np.tile(scenes.instance_matrices(m1)[0], n), F)
    params = capi.VolumeShadowParams(0, fgc.BIAS)
    arr = (C.c_void_p * n)(*[a.h for a in adapters])
    return capi.load().gvt_hip_volume_frame_fog_shadowed(tr.top.h, arr, capi.ptr(mm), capi.ptr(minv), C.c_size_t(n), C.byref(pod), tr._arr(tr.queues), tr.fb.h, None,
                                                         C.byref(params), None)


def _raw_bake(adapters, m, params, stats=None):
    n = len(adapters)
    m1 = capi.f32(m, 16)
    mm = np.ascontiguousarray(np.tile(m1, n), F)
    minv = np.ascontiguousarray(np.tile(scenes.instance_matrices(m1)[0], n), F)
    arr = (C.c_void_p * max(n, 1))(*[a.h for a in adapters])
    return capi.load().gvt_hip_volume_light_grid_bake(arr, capi.ptr(mm), capi.ptr(minv), C.c_size_t(n), None if params is None else C.byref(params),
                                                      None if stats is None else C.byref(stats))


def test_a_stale_grid_is_refused_until_the_rebake(hip):
    pattern = np.random.default_rng(11).random((fc.FILM[1], fc.FILM[0], 4)).astype(F)
    split = (2, 2, 2)
    parts = fc.bricks_of(fc.volume(), split)
    S, on, table = swc.surfaces("main", "lit")
    lights = list(zip(S.lpos, S.lcol))
    want = tracer("lit", split, "inside").frame().framebuffer(False).copy()
    tr = tracer("lit", split, "inside").frame()
    assert (bits(tr.framebuffer(False)) == bits(want)).all() and want.any()
    a = tr.adapters[3]

    def subgrids():  # (an AMR volume takes no shading: off, the subgrids set and removed again, on)
        b = fc.bricks_of(fc.volume(), split)[3]
        scenes.refine(b, np.asarray(b.offset) + 1, (2, 2, 2), 2, seed=5)
        a.set_shading(False)
        a.set_subgrids(b.subgrids)
        a.set_subgrids([])
        a.set_shading(True)

    calls = {"update_samples": lambda: a.update_samples(parts[3].data), "set_transfer": lambda: a.set_transfer(table), "set_surfaces": lambda: a.set_surfaces(),
             "set_lights": lambda: a.set_lights(lights, float(S.ka), float(S.kd)), "set_subgrids": subgrids}
    bakes = 1
    for name, call in calls.items():
        call()  # on ONE brick, behind the tracer's back: the same values, and the grid is stale all the same
        assert a.light_grid_info()["present"] == 1 and a.light_grid_info()["current"] == 0, name
        assert all(b.light_grid_info()["current"] == 1 for b in tr.adapters if b is not a)
        _upload_fb(tr.fb, pattern)
        with pytest.raises(capi.GvtHipError, match=r"\(-1\)") as e:
            tr.frame()
        assert "light grid" in str(e.value), (name, str(e.value))
        assert (bits(tr.framebuffer(False)) == bits(pattern)).all() and all(len(q) == 0 for q in tr.queues), name
        tr.rebake()
        bakes += 1
        assert (bits(tr.frame().framebuffer(False)) == bits(want)).all(), name
        assert tr.stats()["light_bakes"] == bakes
    # shading off and on again: shadow rays march with shading NONE, the grid stays current
    tr.set_shading(False).set_shading(True)
    assert all(b.light_grid_info()["current"] == 1 for b in tr.adapters)
    assert (bits(tr.frame().framebuffer(False)) == bits(want)).all() and tr.stats()["light_bakes"] == bakes
    # another matrix, and one brick fewer (on a top level of its own)
    _upload_fb(tr.fb, pattern)
    assert _raw_frame(tr, m=fc.matrix(True)) == -1 and "light grid" in capi.last_error(), capi.last_error()
    assert (bits(tr.framebuffer(False)) == bits(pattern)).all()
    fewer = tracer("lit", split, "inside", parts=fc.bricks_of(fc.volume(), split)[:7])
    _upload_fb(fewer.fb, pattern)
    assert _raw_frame(fewer, adapters=tr.adapters[:7]) == -1 and "light grid" in capi.last_error(), capi.last_error()
    assert (bits(fewer.framebuffer(False)) == bits(pattern)).all()
    assert _raw_frame(tr) == 0  # stats may be NULL
    assert (bits(tr.framebuffer(False)) == bits(want)).all()


def test_refused_bakes_keep_the_old_grid(hip):
    split = (2, 2, 2)
    m = fc.matrix(False)
    tr = tracer("surf_lit", split, "inside", parts=scenes.split_volume(fc.volume(), *split, ghosts=True)).rebake()
    before = [a.light_grid(1).copy() for a in tr.adapters]
    ok = capi.VolumeLightGridParams(0, 1)

    def refused(adapters, params, word, matrix=m):
        st = capi.VolumeLightGridStats(rays=77)
        assert _raw_bake(adapters, matrix, params, st) == -1
        assert word in capi.last_error(), capi.last_error()
        assert st.rays == 77

    refused(tr.adapters, capi.VolumeLightGridParams(0, 0), "bias")
    refused(tr.adapters, capi.VolumeLightGridParams(0, 65), "bias")
    refused(tr.adapters, capi.VolumeLightGridParams(1, 1), "flag")
    refused(tr.adapters, None, "null")
    assert capi.load().gvt_hip_volume_light_grid_bake(None, None, None, C.c_size_t(0), None, None) == -1 and "null" in capi.last_error()
    refused(tr.adapters[:7], ok, "tile")  # seven of the eight bricks
    refused(tr.adapters + tr.adapters[:1], ok, "tile")  # one brick twice
    tr.set_gradient("central")  # CENTRAL on a frame with an isovalue
    refused(tr.adapters, ok, "central")
    tr.set_gradient("cell")
    assert all(a.light_grid_info() == {"present": 1, "current": 1, "n_planes": 2, "bias": 1, "bytes": 8 * int(np.prod(a.counts))} for a in tr.adapters)
    tr.set_lights([((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))])  # no usable light
    refused(tr.adapters, ok, "usable")
    for a, g in zip(tr.adapters, before):  # (stale now, and still there)
        assert a.light_grid_info()["current"] == 0 and (bits(a.light_grid(1)) == bits(g)).all()
    # an AMR brick (it takes neither surfaces nor shading: a frame of plain lit-less bricks, one of them refined)
    am = tracer("lit", split, "inside").rebake()
    kept = am.adapters[0].light_grid(0).copy()
    am.set_shading(False)
    b = fc.bricks_of(fc.volume(), split)[0]
    scenes.refine(b, np.asarray(b.offset) + 1, (2, 2, 2), 2, seed=5)
    am.adapters[0].set_subgrids(b.subgrids)
    refused(am.adapters, ok, "subgrids")
    assert (bits(am.adapters[0].light_grid(0)) == bits(kept)).all()
    assert _raw_bake(tr.adapters[:0], m, ok) == -1  # no brick at all
    # release: the grid is gone, and a second release is no error
    am.adapters[1].light_grid_release()
    am.adapters[1].light_grid_release()
    assert am.adapters[1].light_grid_info() == {"present": 0, "current": 0, "n_planes": 0, "bias": 0, "bytes": 0}


def test_a_new_time_step_is_baked_again(hip):
    split = (2, 2, 2)
    tr = tracer("surf_lit", split, "inside").frame()
    first = tr.framebuffer(False).copy()
    tr.update(fc.bricks_of(fc.volume(seed=4), split)).frame()
    want = tracer("surf_lit", split, "inside", vol=fc.volume(seed=4)).frame()
    assert (bits(tr.framebuffer(False)) == bits(want.framebuffer(False))).all() and (bits(first) != bits(want.framebuffer(False))).any()
    st = tr.stats()
    assert st["light_bakes"] == 2 and st["fog_samples_shadowed"] == want.stats()["fog_samples_shadowed"] > 0
    for a, b in zip(tr.adapters, want.adapters):
        assert (bits(a.light_grid(0)) == bits(b.light_grid(0))).all()
    tr.frame()  # (the camera alone moves nothing)
    assert tr.stats()["light_bakes"] == 2


def test_a_volume_that_holds_a_grid_renders_as_before(hip):
    tr = tracer("surf_lit", (2, 2, 2), "inside").frame()
    assert all(a.light_grid_info()["current"] == 1 for a in tr.adapters)
    tr.fog_shadows = False  # gvt_hip_volume_frame_shadowed
    want = tracer("surf_lit", (2, 2, 2), "inside", fog=False).frame()
    assert (bits(tr.frame().framebuffer(False)) == bits(want.framebuffer(False))).all() and want.framebuffer(False).any()
    for key in SHADOW_KEYS + CAMERA_KEYS:
        assert tr.stats()[key] == want.stats()[key], key
    tr.shadows = False  # gvt_hip_volume_frame_fused_shaded
    plain = tracer("surf_lit", (2, 2, 2), "inside", shadows=False).frame()
    assert (bits(tr.frame().framebuffer(False)) == bits(plain.framebuffer(False))).all() and tr.stats()["fused"] == 1
    assert (bits(plain.framebuffer(False)) != bits(want.framebuffer(False))).any()
