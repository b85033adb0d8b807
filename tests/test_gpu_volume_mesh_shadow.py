"""Meshes shadowing the volume on the device (csrc/volume_occluder_grid.inc, csrc/volume_fused_mesh.inc; gvt_hip_volume_occluder_grid_bake
and gvt_hip_volume_frame_mesh_shadowed) against the numpy checker (tests/volume_mesh_shadow_checker.py), bit for bit: the baked planes in
every bricking under both matrices, without a mesh and across chunk boundaries; the frame of the three modes of
tests/volume_mesh_shadow_cases.py in every bricking at both eyes, the skip flag, the clipped frame, typed voxels; the frame's
properties; stale grids, the bake's refusals, the mixed frame and the untouched entry points.

The chunk boundary is reached through the test-only option "occluder_chunk" of gvt_hip_set_option: 10,000 pairs per chunk, so the
2 x 15,625 pairs of the case span four chunks."""
import ctypes as C

import numpy as np
import pytest

from gravit_amd import capi, scenes
from gravit_amd.adapter import DepthPlane, HipMeshAdapter
from gravit_amd.scheduler import MixedTracer, NativeTracer, VolumeTracer
from tests import volume_checker as vc
from tests import volume_clip_checker as cc
from tests import volume_fog_shadow_checker as fg
from tests import volume_fused_cases as fc
from tests import volume_mesh_shadow_cases as mc
from tests import volume_mesh_shadow_checker as mg
from tests import volume_shade_checker as lc
from tests import volume_shadow_cases as swc
from tests import volume_surface_checker as sc
from tests.volume_common import as_float, quantised, scaled, tf

pytestmark = pytest.mark.gpu

F = np.float32
FEATURES = {"lit": capi.FUSED_LIT, "surf_lit": capi.FUSED_SURFACES | capi.FUSED_LIT, "surf": capi.FUSED_SURFACES}
COUNTER_KEYS = ("shadow_rays", "shadow_brick_visits", "shadow_crossings", "brick_visits", "rays_deposited", "crossings_rendered", "samples_shaded")
DEVICE_KEYS = COUNTER_KEYS + ("samples_marched", "samples_gathered", "shadow_samples_marched", "shadow_samples_gathered", "fog_samples_shadowed")
N_VERT = fc.N ** 3


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def dress(tr, S, on):
    if len(S):
        tr.set_surfaces(S.iso, S.planes, float(S.opacity))
    tr.set_lights(list(zip(S.lpos, S.lcol)), float(S.ka), float(S.kd))
    tr.set_shading(on)
    return tr


def tracer(mode, split, where, moved=None, skip=True, mesh=True, vol=None, native=False, t=None, S=None, kd=0.6, parts=None, which="case"):
    """The case's tracer, its occluders baked from the case's scene (which: "case", "wall", "shifted"; "none": baked without a mesh;
    None: not baked)."""
    moved = mc.CAMERAS[where] if moved is None else moved
    S0, on, table = swc.surfaces("main", mode, kd=kd)
    if parts is None:
        parts = fc.bricks_of(fc.volume() if vol is None else vol, split)
    tr = VolumeTracer(parts, fc.camera(where, moved), table if t is None else t, m=fc.matrix(moved), sampling_rate=fc.RATE, skip=skip, native=native,
                      fused=True, fused_shaded=True, shadows=True, shadow_bias=mc.BIAS, fog_shadows=True, fog_bias=mc.GRID_BIAS, mesh_shadows=mesh)
    dress(tr, S0 if S is None else S, on)
    if mesh and which == "none":
        assert _raw_bake(tr.adapters, tr.m, capi.VolumeOccluderParams(0, 0)) == 0
        tr._occluder_stale = False
    elif mesh and which is not None:
        tr.bake_occluders({"case": lambda: mc.scene(moved), "wall": lambda: mc.wall_scene(moved), "shifted": lambda: mc.scene(moved, (-0.2, 0.0, -0.15))}[which]())
    return tr


def _raw_bake(adapters, m, params, stats=None, meshes=(), mesh_minv=None):
    """gvt_hip_volume_occluder_grid_bake with the arguments as given (meshes: handles or None)."""
    n = len(adapters)
    m1 = capi.f32(m, 16)
    mm = np.ascontiguousarray(np.tile(m1, n), F)
    minv = np.ascontiguousarray(np.tile(scenes.instance_matrices(m1)[0], n), F)
    arr = (C.c_void_p * max(n, 1))(*[a.h for a in adapters])
    k = len(meshes)
    marr = (C.c_void_p * max(k, 1))(*[None if h is None else h.h for h in meshes])
    return capi.load().gvt_hip_volume_occluder_grid_bake(arr, capi.ptr(mm), capi.ptr(minv), C.c_size_t(n), marr if k else None,
                                                         None if mesh_minv is None else capi.ptr(capi.f32(mesh_minv)), C.c_size_t(k),
                                                         None if params is None else C.byref(params), None if stats is None else C.byref(stats))


def planes_match(tr, O, usable):
    """Every brick's downloaded planes are its part of the checker's grid, byte for byte."""
    for a in tr.adapters:
        o, n = a.offset, a.counts
        for j in np.nonzero(usable)[0]:
            got = a.occluder_grid(int(j))
            want = O[j, o[2]:o[2] + n[2], o[1]:o[1] + n[1], o[0]:o[0] + n[0]]
            if got.dtype != np.uint8 or got.shape != want.shape or not (got == want).all():
                return False
    return True


@pytest.mark.parametrize("moved", [False, True])
@pytest.mark.parametrize("split", fc.SPLITS)
def test_baked_planes_have_the_checkers_bytes(hip, split, moved):
    O, usable, blocked = mc.occluder_grid(moved)
    tr = tracer("lit", split, "outside", moved=moved)
    st = tr.stats()
    assert planes_match(tr, O, usable)
    n_vert = sum(int(np.prod(a.counts)) for a in tr.adapters)
    want_blocked = sum(int((fg.brick_grid(O, a) == 0).sum()) for a in [type("B", (), {"off": a.offset, "n": a.counts}) for a in tr.adapters])  # (shared layers count twice)
    assert (split != (1, 1, 1)) or want_blocked == blocked
    assert st["occluder_bakes"] == 1 and st["occluder_rays"] == 2 * n_vert and st["occluder_bytes"] == 2 * n_vert and st["occluder_ms"] > 0
    assert st["occluder_rays_blocked"] == want_blocked > 0
    assert tr.occluder_stats["any_hit_launches"] == 3  # three instances, one chunk
    for a in tr.adapters:
        assert a.occluder_grid_info() == {"present": 1, "current": 1, "n_planes": 2, "bytes": 2 * int(np.prod(a.counts))}
        assert a.light_grid_info()["present"] == 0  # (the bake of the occluders is not the light grids')


def test_without_a_mesh_every_vertex_is_clear(hip):
    tr = tracer("surf_lit", (2, 2, 2), "inside", which=None)
    st = capi.VolumeOccluderStats()
    assert _raw_bake(tr.adapters, tr.m, capi.VolumeOccluderParams(0, 0), st) == 0
    n_vert = sum(int(np.prod(a.counts)) for a in tr.adapters)
    assert st.rays == 2 * n_vert and st.rays_blocked == 0 and st.any_hit_launches == 0 and st.bytes == 2 * n_vert
    for a in tr.adapters:
        assert (a.occluder_grid(0) == 1).all() and (a.occluder_grid(1) == 1).all()


@pytest.mark.parametrize("split", [(1, 1, 1), (3, 1, 2)])
def test_chunks_do_not_show(hip, split):
    """10,000 pairs per chunk: the 31,250 pairs of one brick span four chunks, and chunk boundaries fall inside planes and bricks."""
    O, usable, _ = mc.occluder_grid(False)
    capi.set_option("occluder_chunk", 10000)
    try:
        tr = tracer("lit", split, "outside", moved=False)
    finally:
        capi.set_option("occluder_chunk", 0)
    n_pairs = 2 * sum(int(np.prod(a.counts)) for a in tr.adapters)
    assert planes_match(tr, O, usable)
    assert tr.occluder_stats["any_hit_launches"] == 3 * ((n_pairs + 9999) // 10000) >= 12
    assert tr.occluder_stats["rays"] == n_pairs


@pytest.mark.parametrize("where", sorted(mc.CAMERAS))
@pytest.mark.parametrize("split", fc.SPLITS)
@pytest.mark.parametrize("mode", mc.MODES)
def test_mesh_shadowed_frame_has_the_checkers_bits_and_counts(hip, mode, split, where):
    want, counters, _ = mc.reference(mode, split, where)
    tr = tracer(mode, split, where).frame()
    got, st = tr.framebuffer(False), tr.stats()
    assert st["mesh_shadowed"] == 1 and st["shadowed"] == 1 and st["fused"] == 1 and st["adapter_calls"] == 1 and st["features"] == FEATURES[mode]
    assert st["occluder_bakes"] == 1 and st["light_bakes"] == (0 if mode == "surf" else 1)
    assert got.any()
    assert (bits(got) == bits(want)).all()
    for key in COUNTER_KEYS:
        assert st[key] == counters[key], key
    assert all(len(q) == 0 for q in tr.queues)


@pytest.mark.parametrize("split", [(1, 1, 1), (4, 4, 4)])
@pytest.mark.parametrize("mode", mc.MODES)
def test_skipping_does_not_show(hip, mode, split):
    a = tracer(mode, split, "inside").frame()
    b = tracer(mode, split, "inside", skip=False).frame()
    sa, sb = a.stats(), b.stats()
    assert (bits(a.framebuffer(False)) == bits(b.framebuffer(False))).all() and a.framebuffer(False).any()
    assert sa["samples_marched"] == sb["samples_marched"] == sb["samples_gathered"] >= sa["samples_gathered"] > 0
    for key in COUNTER_KEYS + ("shadow_samples_marched",):
        assert sa[key] == sb[key], key


@pytest.mark.parametrize("mode", mc.MODES)
def test_clipped_frame(hip, mode):
    want, counters, plane = mc.reference(mode, (2, 2, 2), "outside", clipped=True)
    depth = DepthPlane(fc.FILM[0], fc.FILM[1]).upload(plane)
    tr = tracer(mode, (2, 2, 2), "outside", moved=False).frame(depth)
    got, st = tr.framebuffer(False).copy(), tr.stats()
    assert st["mesh_shadowed"] == 1
    assert (bits(got) == bits(want)).all()
    for key in COUNTER_KEYS:
        assert st[key] == counters[key], key
    assert (bits(got) != bits(tr.frame().framebuffer(False))).any()  # the clip shows
    assert tr.stats()["occluder_bakes"] == 1


def test_typed_voxels(hip):
    vol, t = quantised(fc.volume(), "u8"), scaled("spikes", "u8")
    S, on, _ = swc.surfaces("main", "surf_lit", scale=255.0)
    tr = tracer("surf_lit", (2, 2, 2), "inside", vol=vol, native=True, t=t, S=S).frame()
    st = tr.stats()
    assert tr.adapters[0].dtype_name == "uint8" and st["mesh_shadowed"] == 1 and st["shadow_rays"] > 0 and st["fog_samples_shadowed"] > 0
    flt = tracer("surf_lit", (2, 2, 2), "inside", vol=as_float(vol), t=t, S=S).frame()
    assert tr.framebuffer(False).any()
    assert (bits(tr.framebuffer(False)) == bits(flt.framebuffer(False))).all()
    for key in COUNTER_KEYS:
        assert st[key] == flt.stats()[key], key
    fog = tracer("surf_lit", (2, 2, 2), "inside", vol=vol, native=True, t=t, S=S, mesh=False).frame()
    assert (bits(tr.framebuffer(False)) != bits(fog.framebuffer(False))).any()  # the meshes' shadows show


@pytest.mark.parametrize("mode", mc.MODES)
def test_the_counters_are_the_fog_shadowed_frames(hip, mode):
    """No counter depends on O; with every O = 1 (baked without a mesh) the bits are gvt_hip_volume_frame_fog_shadowed's; behind a wall
    that blocks every vertex ray they are the kd = 0 frame's."""
    fog = tracer(mode, (2, 2, 2), "inside", mesh=False).frame()
    fs, want = fog.stats(), fog.framebuffer(False).copy()
    tr = tracer(mode, (2, 2, 2), "inside").frame()
    st = tr.stats()
    for key in DEVICE_KEYS:
        assert st[key] == fs[key], key
    assert st["mesh_shadowed"] == 1 and (bits(tr.framebuffer(False)) != bits(want)).any()
    clear = tracer(mode, (2, 2, 2), "inside", which="none").frame()
    assert clear.stats()["mesh_shadowed"] == 1 and (bits(clear.framebuffer(False)) == bits(want)).all() and want.any()
    dark = tracer(mode, (2, 2, 2), "inside", which="wall").frame()
    assert dark.occluder_stats["rays_blocked"] == dark.occluder_stats["rays"]
    unlit = tracer(mode, (2, 2, 2), "inside", mesh=False, kd=0.0).frame()
    assert (bits(dark.framebuffer(False)) == bits(unlit.framebuffer(False))).all() and (bits(dark.framebuffer(False)) != bits(want)).any()


def test_without_a_usable_light_the_frame_is_inert(hip):
    """No usable light: gvt_hip_volume_frame_fog_shadowed in every respect, and no occluder grid is needed."""
    S0, on, _ = swc.surfaces("main", "surf_lit")
    S = sc.Surfaces(S0.iso, S0.planes, S0.opacity, [((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))], ka=S0.ka, kd=S0.kd)
    tr = tracer("surf_lit", (2, 2, 2), "inside", S=S, which=None).frame()
    fog = tracer("surf_lit", (2, 2, 2), "inside", S=S, mesh=False).frame()
    assert tr.stats()["mesh_shadowed"] == 0 and tr.stats()["occluder_bakes"] == 0
    assert (bits(tr.framebuffer(False)) == bits(fog.framebuffer(False))).all() and fog.framebuffer(False).any()


def _upload_fb(fb, img):
    """Put an image into a framebuffer (the library has no host path into one: a plain copy through the runtime it is linked against)."""
    src = capi.f32(img)
    capi.synchronize()
    rt = C.CDLL("libamdhip64.so")
    rt.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert src.nbytes == fb.w * fb.hgt * 16
    assert rt.hipMemcpy(fb.device_ptr(), capi.ptr(src), src.nbytes, 1) == 0  # hipMemcpyHostToDevice


def _raw_frame(tr, adapters=None, m=None):
    """gvt_hip_volume_frame_mesh_shadowed on tr's top level, queues and framebuffer with other volumes or another matrix."""
    cam = tr.camera
    adapters = tr.adapters if adapters is None else adapters
    n = len(adapters)
    pod = capi.CameraPod((C.c_float * 3)(*cam.eye), (C.c_float * 3)(*cam.focus), (C.c_float * 3)(*cam.up), cam.fov, cam.width, cam.height, 1, 1, 0.0)
    m1 = capi.f32(tr.m if m is None else m, 16)
    mm = np.ascontiguousarray(np.tile(m1, n), F)
    minv = np.ascontiguousarray(np.tile(scenes.instance_matrices(m1)[0], n), F)
    params = capi.VolumeShadowParams(0, mc.BIAS)
    arr = (C.c_void_p * n)(*[a.h for a in adapters])
    return capi.load().gvt_hip_volume_frame_mesh_shadowed(tr.top.h, arr, capi.ptr(mm), capi.ptr(minv), C.c_size_t(n), C.byref(pod), tr._arr(tr.queues), tr.fb.h, None,
                                                          C.byref(params), None)


def test_a_stale_grid_is_refused_until_the_rebake(hip):
    """Mode "surf": the frame needs no light grid, so every refusal here is the occluder grids'."""
    pattern = np.random.default_rng(11).random((fc.FILM[1], fc.FILM[0], 4)).astype(F)
    split = (2, 2, 2)
    S, on, table = swc.surfaces("main", "surf")
    lights = list(zip(S.lpos, S.lcol))
    scene = mc.scene(False)
    tr = tracer("surf", split, "inside").frame()
    want = tr.framebuffer(False).copy()
    assert want.any() and (bits(want) == bits(mc.reference("surf", split, "inside")[0])).all()
    a = tr.adapters[3]
    a.set_lights(lights, float(S.ka), float(S.kd))  # on ONE brick, behind the tracer's back: the same values, and the grid is stale all the same
    assert a.occluder_grid_info()["present"] == 1 and a.occluder_grid_info()["current"] == 0
    assert all(b.occluder_grid_info()["current"] == 1 for b in tr.adapters if b is not a)
    _upload_fb(tr.fb, pattern)
    with pytest.raises(capi.GvtHipError, match=r"\(-1\)") as e:
        tr.frame()
    assert "occluder grid" in str(e.value), str(e.value)
    assert (bits(tr.framebuffer(False)) == bits(pattern)).all() and all(len(q) == 0 for q in tr.queues)
    tr.bake_occluders(scene)
    assert (bits(tr.frame().framebuffer(False)) == bits(want)).all() and tr.stats()["occluder_bakes"] == 2
    # through the tracer: set_lights bakes again by itself; the data, the table, the surfaces and the shading do not touch the occluders
    tr.set_lights(lights, float(S.ka), float(S.kd))
    assert (bits(tr.frame().framebuffer(False)) == bits(want)).all() and tr.stats()["occluder_bakes"] == 3
    tr.update(fc.bricks_of(fc.volume(), split))
    for b in tr.adapters:
        b.set_transfer(table)
    tr.set_surfaces(S.iso, S.planes, float(S.opacity)).set_shading(True).set_shading(False)
    assert all(b.occluder_grid_info()["current"] == 1 for b in tr.adapters)
    assert (bits(tr.frame().framebuffer(False)) == bits(want)).all() and tr.stats()["occluder_bakes"] == 3
    # another matrix, one brick fewer (on a top level of its own), and another order
    _upload_fb(tr.fb, pattern)
    assert _raw_frame(tr, m=fc.matrix(True)) == -1 and "occluder grid" in capi.last_error(), capi.last_error()
    fewer = tracer("surf", split, "inside", parts=fc.bricks_of(fc.volume(), split)[:7], which=None)
    _upload_fb(fewer.fb, pattern)
    assert _raw_frame(fewer, adapters=tr.adapters[:7]) == -1 and "occluder grid" in capi.last_error(), capi.last_error()
    assert (bits(fewer.framebuffer(False)) == bits(pattern)).all()
    assert _raw_frame(tr, adapters=tr.adapters[1:] + tr.adapters[:1]) == -1 and "occluder grid" in capi.last_error(), capi.last_error()
    assert (bits(tr.framebuffer(False)) == bits(pattern)).all()
    assert _raw_frame(tr) == 0  # stats may be NULL
    assert (bits(tr.framebuffer(False)) == bits(want)).all()


def test_refused_bakes_keep_the_old_grid(hip):
    split = (2, 2, 2)
    m = fc.matrix(False)
    scene = mc.scene(False)
    tr = tracer("surf_lit", split, "inside")
    before = [a.occluder_grid(1).copy() for a in tr.adapters]
    ok = capi.VolumeOccluderParams(0, 0)
    plate = HipMeshAdapter(scene.meshes[1])

    def refused(adapters, params, word, meshes=(), mesh_minv=None):
        st = capi.VolumeOccluderStats(rays=77)
        assert _raw_bake(adapters, m, params, st, meshes, mesh_minv) == -1
        assert word in capi.last_error(), capi.last_error()
        assert st.rays == 77

    refused(tr.adapters, None, "null")
    refused(tr.adapters, capi.VolumeOccluderParams(1, 0), "flag")
    refused(tr.adapters[:7], ok, "tile")  # seven of the eight bricks
    refused(tr.adapters, ok, "no mesh", meshes=[plate, None], mesh_minv=scene.minv[1:3])
    refused(tr.adapters, ok, "null", meshes=[plate], mesh_minv=None)
    assert all(a.occluder_grid_info() == {"present": 1, "current": 1, "n_planes": 2, "bytes": 2 * int(np.prod(a.counts))} for a in tr.adapters)
    for a, g in zip(tr.adapters, before):
        assert (a.occluder_grid(1) == g).all()
    # a volume with subgrids (it takes neither surfaces nor shading: a frame of plain lit-less bricks, one of them refined)
    am = tracer("lit", split, "inside")
    kept = am.adapters[0].occluder_grid(0).copy()
    am.set_shading(False)
    b = fc.bricks_of(fc.volume(), split)[0]
    scenes.refine(b, np.asarray(b.offset) + 1, (2, 2, 2), 2, seed=5)
    am.adapters[0].set_subgrids(b.subgrids)
    refused(am.adapters, ok, "subgrids")
    assert am.adapters[0].occluder_grid_info()["current"] == 0 and (am.adapters[0].occluder_grid(0) == kept).all()
    with pytest.raises(capi.GvtHipError, match="not usable"):
        am.adapters[0].occluder_grid(5)
    # release: the grid is gone, and a second release is no error
    am.adapters[1].occluder_grid_release()
    am.adapters[1].occluder_grid_release()
    assert am.adapters[1].occluder_grid_info() == {"present": 0, "current": 0, "n_planes": 0, "bytes": 0}
    with pytest.raises(capi.GvtHipError, match="no occluder grid"):
        am.adapters[1].occluder_grid(0)


def test_a_volume_that_holds_an_occluder_grid_renders_as_before(hip):
    """One case per entry point that existed: the fog-shadowed, the shadowed, the shaded fused and the plain fused frame and the loop."""
    tr = tracer("surf_lit", (2, 2, 2), "inside").frame()
    assert all(a.occluder_grid_info()["current"] == 1 for a in tr.adapters)
    plain = tracer("surf_lit", (2, 2, 2), "inside", mesh=False)
    for switch in ("mesh_shadows", "fog_shadows", "shadows", "fused_shaded", "fused"):
        setattr(tr, switch, False)
        setattr(plain, switch, False)
        got, want = tr.frame().framebuffer(False).copy(), plain.frame().framebuffer(False).copy()
        assert (bits(got) == bits(want)).all() and want.any(), switch


def _mixed(parts, scene, cam, t, lights):
    mt = MixedTracer(scene, parts, cam, t, sampling_rate=1.0, shadows=True, fog_shadows=True, mesh_shadows=True)
    mt.set_lights(lights).set_shading(True)
    return mt


def test_mixed_frame(hip):
    """The bunny inside lit fog casts its shadow into the fog: the composite of the parts, the volume part from the checker."""
    w, h = 150, 110
    cam = scenes.Camera((0.0, 0.1, 0.3), (0.0, 0.1, -0.3), (0.0, 1.0, 0.0), float(F(45.0 * np.pi / 180.0)), w, h)
    scene = scenes.bunny_scene(w, h)
    vol = scenes.mesh_in_volume(scene, scenes.sphere_volume(64), fill=0.6)
    t = tf("ramp")
    lights = [swc.LIGHTS[0]]
    S = sc.Surfaces([], [], 0.6, lights)
    mt = _mixed(scenes.split_volume(vol, 1, 1, 1), scene, cam, t, lights).frame()
    st = mt.volume.stats()
    assert st["mesh_shadowed"] == 1 and st["fog_samples_shadowed"] == st["samples_shaded"] > 0 and st["occluder_bakes"] == 1 and st["light_bakes"] == 1
    assert 0 < st["occluder_rays_blocked"] < st["occluder_rays"] == 64 ** 3
    # the mesh frame keeps its bits
    mesh = NativeTracer(scene)().framebuffer(False)
    assert (bits(mt.mesh_framebuffer(False)) == bits(mesh)).all()
    # the composite of the parts
    depth = mt.depth.download().copy()
    m = fc.matrix(False)
    minv = scenes.instance_matrices(m)[0]
    whole = vc.Brick(vol, t, 1.0)
    wlo, whi = fc.world_boxes([vol], m)
    G, _ = fg.grid(whole, wlo, whi, m, minv, S, 1)
    O, _, blocked = mg.occluders(whole, m, scene, S)
    assert blocked == st["occluder_rays_blocked"] and (mt.volume.adapters[0].occluder_grid(0) == O[0]).all()
    fog, counters = mg.frame([whole], wlo, whi, minv, cam, S, lc.SHADE_GRADIENT, G, O, depth, swc.BIAS)
    want = cc.composite(fog, mesh, depth)
    got = mt.framebuffer(False).copy()
    assert (bits(got) == bits(want)).all() and np.isfinite(depth).sum() > 100
    assert st["samples_shaded"] == counters["samples_shaded"]
    # the bricking does not show
    eight = _mixed(scenes.split_volume(vol, 2, 2, 2), scene, cam, t, lights).frame()
    assert (bits(eight.framebuffer(False)) == bits(got)).all()
    # the camera does not bake; a moved bunny does, and its shadow moves
    mt.set_camera(cam).frame()
    assert mt.volume.stats()["occluder_bakes"] == 1 and (bits(mt.framebuffer(False)) == bits(got)).all()
    shift = scenes.mat_translate_scale((0.02, 0.0, 0.01), (1, 1, 1))
    moved = scenes._assemble(scene.meshes, scene.inst_mesh, [shift], scene.lights, cam, "bunny-moved")
    mt.update_scene(moved).frame()
    assert mt.volume.stats()["occluder_bakes"] == 2
    O2 = mt.volume.adapters[0].occluder_grid(0)
    assert (O2 != O[0]).any() and (O2 == mg.occluders(whole, m, moved, S)[0][0]).all()
    mt.rebake_occluders()
    assert mt.volume.stats()["occluder_bakes"] == 3 and (mt.volume.adapters[0].occluder_grid(0) == O2).all()
