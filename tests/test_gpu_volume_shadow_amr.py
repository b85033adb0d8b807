"""Shadows on AMR bricks on the device (GVT_HIP_VOLUME_ALLOW_AMR; csrc/volume_fused_shadow_amr.inc) against the numpy checker
(tests/volume_shadow_amr_checker.py), bit for bit: the shadowed, the fog-shadowed and the mesh-shadowed frame over one brick and over
eight of which two have subgrids, from outside and from inside a subgrid, with and without skipping; the light grid's bake; merged ranges;
the clipped and the mixed frame; non-finite vertices; the gates."""
import ctypes as C
from dataclasses import replace

import numpy as np
import pytest
import torch  # noqa: F401  (before the library initialises the device, as in test_gpu_volume_amr.py)

from gravit_amd import capi, scenes
from gravit_amd.adapter import DepthPlane
from gravit_amd.scheduler import MixedTracer, NativeTracer, VolumeTracer
from tests import volume_amr_surface_cases as scases
from tests import volume_clip_checker as cc
from tests import volume_fog_shadow_checker as fg
from tests import volume_fused_amr_cases as fc
from tests import volume_shade_checker as lc
from tests import volume_shadow_amr_cases as ac
from tests import volume_shadow_amr_checker as sa
from tests import volume_shadow_cases as swc
from tests.test_gpu_volume_fog_shadow import _upload_fb
from tests.volume_common import IDENT

pytestmark = pytest.mark.gpu

F = np.float32
SURF, LIT, AMR = capi.FUSED_SURFACES, capi.FUSED_LIT, capi.FUSED_AMR
FEATURES = {"surf": SURF, "surf_lit": SURF | LIT, "lit": LIT}
SHADOW_KEYS = ("shadow_rays", "shadow_brick_visits", "shadow_crossings")
CAMERA_KEYS = ("brick_visits", "rays_deposited", "crossings_rendered", "samples_shaded")
N_PIX = ac.FILM[0] * ac.FILM[1]
FRAMES = ("gvt_hip_volume_frame_shadowed", "gvt_hip_volume_frame_fog_shadowed", "gvt_hip_volume_frame_mesh_shadowed")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def dress(tr, S, mode):
    if S.args is not None:
        tr.set_surfaces(**S.args)
    tr.set_lights(**S.light_args)
    tr.set_shading(mode in ("lit", "surf_lit"))
    return tr


def tracer(kind, mode, bricking, where="outside", which="scene", skip=True, amr=True, S=None, t=None, parts=None, cls=VolumeTracer, scene=None, **kw):
    """kind: "shadow", "fog" or "mesh" (the occluders are not baked here), or "fused": the unshadowed fused AMR frame."""
    parts = fc.parts_of(ac.volume_of(which), bricking) if parts is None else parts
    S = ac.surfaces(mode, which)[0] if S is None else S
    t = ac.table_of(which) if t is None else t
    if kind == "fused":
        how = dict(fused=True, fused_shaded=True, fused_amr=True)
    else:
        how = dict(shadows=True, shadow_bias=ac.BIAS, fog_shadows=kind in ("fog", "mesh"), fog_bias=ac.GRID_BIAS, mesh_shadows=kind == "mesh", shadow_amr=amr)
    how.update(kw)
    args = (parts, ac.camera(where), t) if scene is None else (scene, parts, ac.camera(where), t)
    return dress(cls(*args, sampling_rate=ac.RATE, skip=skip, amr_shaded=True, **how), S, mode)


def brick_counters_are_zero(tr):
    for a in tr.adapters:
        info, amr = a.info(), a.amr_info()
        assert info["samples_marched"] == info["samples_gathered"] == 0 and a.crossings() == 0 and a.shaded() == 0
        assert amr["amr_marches"] == 0 and amr["samples_refined"] == 0
    assert all(len(q) == 0 for q in tr.queues)


def check_frame(tr, mode, want, counters, kind="shadow"):
    got, st = tr.framebuffer(False), tr.stats()
    assert st["shadowed"] == 1 and st["fused"] == 1 and st["adapter_calls"] == 1 and st["features"] == AMR | FEATURES[mode]
    assert got.any() and (bits(got) == bits(want)).all()
    for key in SHADOW_KEYS + CAMERA_KEYS:
        assert st[key] == counters[key], key
    brick_counters_are_zero(tr)
    return st


# ---- 1. the shadowed frame
@pytest.mark.parametrize("skip", [True, False])
@pytest.mark.parametrize("where", ac.EYES)
@pytest.mark.parametrize("bricking", ac.BRICKINGS)
@pytest.mark.parametrize("mode", ["surf", "surf_lit"])
def test_shadowed_frame_has_the_checkers_bits_and_counts(hip, mode, bricking, where, skip):
    want, counters, _ = ac.reference("shadow", mode, bricking, where)
    st = check_frame(tracer("shadow", mode, bricking, where, skip=skip).frame(), mode, want, counters)
    assert st["shadow_rays"] > 0 and st["shadow_samples_marched"] >= st["shadow_samples_gathered"] > 0
    if not skip:
        assert st["shadow_samples_gathered"] == st["shadow_samples_marched"] and st["samples_gathered"] == st["samples_marched"]
    assert (bits(want) == bits(ac.reference("shadow", mode, 1, where)[0])).all()  # the 8-brick frame is the 1-brick frame


# ---- 2. no usable light; every light blocked
@pytest.mark.parametrize("mode", ["surf", "surf_lit"])
def test_an_unusable_light_gives_the_fused_amr_frames_bits(hip, mode):
    S = ac.surfaces(mode, lights=[((0.0, 0.0, 0.0), (1.0, 0.9, 0.8))])[0]
    tr = tracer("shadow", mode, 8, S=S).frame()
    plain = tracer("fused", mode, 8, S=S).frame()
    st, ps = tr.stats(), plain.stats()
    assert st["shadowed"] == 1 and st["shadow_rays"] == 0 and st["features"] == ps["features"] == AMR | FEATURES[mode]
    assert (bits(tr.framebuffer(False)) == bits(plain.framebuffer(False))).all() and plain.framebuffer(False).any()
    for key in CAMERA_KEYS + ("samples_marched", "samples_gathered"):
        assert st[key] == ps[key], key


def test_where_every_light_is_blocked_the_bits_are_the_ambient_frames(hip):
    want, counters = ac.blocked_reference(8)
    has, dark = swc.fully_shadowed(counters["details"], N_PIX)
    assert dark.sum() >= 0.5 * has.sum() > 100 and counters["amr"]["crossings_refined"] > 0 and counters["amr"]["shadow_refined"] > 0
    S, table = ac.blocked_surfaces()
    got = tracer("shadow", "surf", 8, S=S, t=table).frame().framebuffer(False).copy()
    assert (bits(got) == bits(want)).all()
    ambient = tracer("fused", "surf", 8, S=ac.blocked_surfaces(kd=0.0)[0], t=table).frame().framebuffer(False).copy()
    plain = tracer("fused", "surf", 8, S=S, t=table).frame().framebuffer(False)
    g, a, p = bits(got).reshape(-1, 4), bits(ambient).reshape(-1, 4), bits(plain).reshape(-1, 4)
    assert (g[dark] == a[dark]).all() and (g[dark] != p[dark]).any(axis=-1).all()


# ---- 3. the light grid's bake
def grids_match(tr, G):
    for a in tr.adapters:
        B = type("B", (), {"off": a.offset, "n": a.counts})
        assert (bits(a.light_grid(0)) == bits(fg.brick_grid(G, B)[0])).all()


def _raw_light_bake(adapters, flags, bias=ac.GRID_BIAS, stats=None):
    n = len(adapters)
    mm = np.ascontiguousarray(np.tile(capi.f32(IDENT, 16), n), F)
    arr = (C.c_void_p * max(n, 1))(*[a.h for a in adapters])
    params = capi.VolumeLightGridParams(flags, bias)
    return capi.load().gvt_hip_volume_light_grid_bake(arr, capi.ptr(mm), capi.ptr(mm), C.c_size_t(n), C.byref(params), None if stats is None else C.byref(stats))


def _raw_occluder_bake(adapters, flags):
    n = len(adapters)
    mm = np.ascontiguousarray(np.tile(capi.f32(IDENT, 16), n), F)
    arr = (C.c_void_p * max(n, 1))(*[a.h for a in adapters])
    params = capi.VolumeOccluderParams(flags, 0)
    return capi.load().gvt_hip_volume_occluder_grid_bake(arr, capi.ptr(mm), capi.ptr(mm), C.c_size_t(n), None, None, C.c_size_t(0), C.byref(params), None)


@pytest.mark.parametrize("bricking", ac.BRICKINGS)
def test_baked_grid_has_the_checkers_bits(hip, bricking):
    G, usable = ac.light_grid()
    assert usable.all()
    tr = tracer("fog", "surf_lit", bricking).rebake()
    grids_match(tr, G)
    n_vert = sum(int(np.prod(a.counts)) for a in tr.adapters)
    st, g = tr.stats(), tr.light_grid_stats
    assert st["light_bakes"] == 1 and st["light_grid_rays"] == n_vert and st["light_grid_bytes"] == 4 * n_vert and st["light_grid_ms"] > 0
    assert g["samples_marched"] >= g["samples_gathered"] > 0 and g["crossings"] > 0
    off = tracer("fog", "surf_lit", bricking, skip=False).rebake()
    grids_match(off, G)
    assert off.light_grid_stats["samples_marched"] == off.light_grid_stats["samples_gathered"] == g["samples_marched"] and off.light_grid_stats["crossings"] == g["crossings"]
    if bricking == 8:  # a layer two bricks share is stored twice, with the same bits (the bricks that meet in the plane x = CUTS[0][1])
        pairs = [(a, b) for a in tr.adapters for b in tr.adapters if a.offset[0] + a.counts[0] - 1 == b.offset[0] and (a.offset[1:] == b.offset[1:]).all()]
        assert len(pairs) == 4
        for a, b in pairs:
            assert (bits(a.light_grid(0)[:, :, -1]) == bits(b.light_grid(0)[:, :, 0])).all()
    brick_counters_are_zero(tr)
    # a refused bake -- without the flag, as ever; an unknown flag -- keeps the old grids current
    before = [a.light_grid(0).copy() for a in tr.adapters]
    for flags, word in ((0, "subgrids"), (capi.VOLUME_ALLOW_CENTRAL, "subgrids"), (5, "flag"), (8, "flag")):
        stt = capi.VolumeLightGridStats(rays=77)
        assert _raw_light_bake(tr.adapters, flags, stats=stt) == -1 and word in capi.last_error() and stt.rays == 77, capi.last_error()
    for a, g0 in zip(tr.adapters, before):
        assert a.light_grid_info()["current"] == 1 and (bits(a.light_grid(0)) == bits(g0)).all()


# ---- 4. merged ranges
@pytest.mark.parametrize("skip", [True, False])
def test_merged_ranges(hip, skip):
    """The opacity and the crossed isovalue live in the subgrids alone: a skip decision from level-0 ranges blanks grid and frame."""
    G, _ = ac.light_grid("buried")
    assert (G < 1).any()
    want, counters, _ = ac.reference("fog", "surf_lit", 8, "outside", "buried")
    tr = tracer("fog", "surf_lit", 8, which="buried", skip=skip).frame()
    grids_match(tr, G)
    st = check_frame(tr, "surf_lit", want, counters)
    assert counters["crossings_rendered"] > 0 and counters["amr"]["crossings_refined"] > 0
    g = tr.light_grid_stats
    if skip:
        assert g["samples_gathered"] < g["samples_marched"] and st["samples_gathered"] < st["samples_marched"]  # ... and the rest is skipped
    # the lean kernel reads the skip bit of the AMR cell word
    lean = tracer("fog", "lit", 8, which="buried", skip=skip).frame()
    assert (bits(lean.framebuffer(False)) == bits(ac.reference("fog", "lit", 8, "outside", "buried")[0])).all() and lean.framebuffer(False).any()


# ---- 5. the fog-shadowed frame
@pytest.mark.parametrize("where", ac.EYES)
@pytest.mark.parametrize("bricking", ac.BRICKINGS)
@pytest.mark.parametrize("mode", ["lit", "surf_lit"])
def test_fog_shadowed_frame_has_the_checkers_bits_and_counts(hip, mode, bricking, where):
    want, counters, _ = ac.reference("fog", mode, bricking, where)
    tr = tracer("fog", mode, bricking, where).frame()
    st = check_frame(tr, mode, want, counters)
    assert st["light_bakes"] == 1 and st["fog_samples_shadowed"] == st["samples_shaded"] > 0
    off = tracer("fog", mode, bricking, where, skip=False).frame()
    assert (bits(off.framebuffer(False)) == bits(want)).all()


def test_a_stale_grid_is_refused_until_the_rebake(hip):
    pattern = np.random.default_rng(11).random((ac.FILM[1], ac.FILM[0], 4)).astype(F)
    parts = fc.parts_of(ac.scene(), 8)
    want = ac.reference("fog", "surf_lit", 8, "outside")[0]
    tr = tracer("fog", "surf_lit", 8, parts=parts).frame()
    assert (bits(tr.framebuffer(False)) == bits(want)).all()
    a = tr.adapters[0]
    a.set_subgrids(parts[0].subgrids)  # the same subgrids, behind the tracer's back: the grid is stale all the same
    assert a.light_grid_info()["present"] == 1 and a.light_grid_info()["current"] == 0
    _upload_fb(tr.fb, pattern)
    with pytest.raises(capi.GvtHipError, match=r"\(-1\)") as e:
        tr.frame()
    assert "light grid" in str(e.value)
    assert (bits(tr.framebuffer(False)) == bits(pattern)).all() and all(len(q) == 0 for q in tr.queues)
    tr.rebake()
    assert (bits(tr.frame().framebuffer(False)) == bits(want)).all() and tr.stats()["light_bakes"] == 2


# ---- 6. the mesh-shadowed frame
def test_without_a_mesh_it_is_the_fog_shadowed_frame(hip):
    for mode in ("lit", "surf_lit"):
        tr = tracer("mesh", mode, 8)
        assert _raw_occluder_bake(tr.adapters, tr.param_flags) == 0, capi.last_error()
        tr._occluder_stale = False
        st = tr.frame().stats()
        assert st["mesh_shadowed"] == 1 and st["features"] == AMR | FEATURES[mode]
        assert (bits(tr.framebuffer(False)) == bits(ac.reference("fog", mode, 8, "outside")[0])).all()
        assert _raw_occluder_bake(tr.adapters, 0) == -1 and "subgrids" in capi.last_error()


@pytest.mark.parametrize("bricking", ac.BRICKINGS)
@pytest.mark.parametrize("mode", ["lit", "surf", "surf_lit"])
def test_mesh_shadowed_frame_has_the_checkers_bits_and_counts(hip, mode, bricking):
    O, usable, blocked = ac.occluder_grid()
    want, counters, _ = ac.reference("mesh", mode, bricking, "outside")
    tr = tracer("mesh", mode, bricking).bake_occluders(ac.mesh_scene()).frame()
    st = check_frame(tr, mode, want, counters)
    assert st["mesh_shadowed"] == 1 and st["occluder_rays_blocked"] >= blocked > 0
    for a in tr.adapters:  # the planes are the checker's for 1 and 8 bricks
        B = type("B", (), {"off": a.offset, "n": a.counts})
        assert (a.occluder_grid(0) == fg.brick_grid(O, B)[0]).all()
    assert (bits(want) != bits(ac.reference("fog" if mode != "surf" else "shadow", mode, bricking, "outside")[0])).any()  # the mesh's shadow shows


def test_a_stale_occluder_grid_is_refused_until_the_bake(hip):
    pattern = np.random.default_rng(14).random((ac.FILM[1], ac.FILM[0], 4)).astype(F)
    parts = fc.parts_of(ac.scene(), 8)
    want = ac.reference("mesh", "surf", 8, "outside")[0]
    tr = tracer("mesh", "surf", 8, parts=parts).bake_occluders(ac.mesh_scene()).frame()
    assert (bits(tr.framebuffer(False)) == bits(want)).all()
    a = tr.adapters[0]
    a.set_subgrids(parts[0].subgrids)  # behind the tracer's back
    assert a.occluder_grid_info()["present"] == 1 and a.occluder_grid_info()["current"] == 0
    _upload_fb(tr.fb, pattern)
    with pytest.raises(capi.GvtHipError, match=r"\(-1\)") as e:
        tr.frame()
    assert "occluder grid" in str(e.value)
    assert (bits(tr.framebuffer(False)) == bits(pattern)).all() and all(len(q) == 0 for q in tr.queues)
    tr.bake_occluders(ac.mesh_scene())
    assert (bits(tr.frame().framebuffer(False)) == bits(want)).all() and tr.stats()["occluder_bakes"] == 2


# ---- 7. the clipped and the mixed frame
def test_clipped_frame(hip):
    cam = ac.camera("outside")
    want, counters, plane = ac.reference("mesh", "surf_lit", 8, "outside", clipped=True)
    assert np.isfinite(plane).sum() > 250
    depth = DepthPlane(cam.width, cam.height).upload(plane)
    tr = tracer("mesh", "surf_lit", 8).bake_occluders(ac.mesh_scene()).frame(depth)
    check_frame(tr, "surf_lit", want, counters)
    assert (bits(want) != bits(ac.reference("mesh", "surf_lit", 8, "outside")[0])).any()  # the clip shows
    for kind, mode in (("shadow", "surf"), ("fog", "lit"), ("mesh", "lit")):
        tr = tracer(kind, mode, 8)
        if kind == "mesh":
            tr.bake_occluders(ac.mesh_scene())
        assert (bits(tr.frame(depth).framebuffer(False)) == bits(ac.reference(kind, mode, 8, "outside", clipped=True)[0])).all(), (kind, mode)


def test_mixed_frame(hip):
    """The tetrahedron inside S0's box shadows the volume, clips it at its depth plane and shows through it."""
    cam, scene = ac.camera("outside"), ac.mesh_scene()
    mt = tracer("mesh", "surf_lit", 8, cls=MixedTracer, scene=scene).frame()
    st = mt.volume.stats()
    assert st["shadowed"] == 1 and st["mesh_shadowed"] == 1 and st["features"] == AMR | SURF | LIT and mt.volume.calls == 1 and st["occluder_bakes"] == 1
    depth = mt.depth.download().copy()
    assert 5 < np.isfinite(depth).sum() < N_PIX // 2
    mesh = NativeTracer(replace(scene, camera=cam))().framebuffer(False)
    bricks, lo, hi = ac.checker_bricks("scene", 8)
    S, shading = ac.surfaces("surf_lit")
    fog, counters = sa.frame(bricks, lo, hi, IDENT, cam, S, shading, ac.light_grid()[0], ac.occluder_grid()[0], depth, ac.BIAS)
    assert (bits(mt.framebuffer(False)) == bits(cc.composite(fog, mesh, depth))).all()
    for key in SHADOW_KEYS + CAMERA_KEYS:
        assert st[key] == counters[key], key


# ---- 8. non-finite vertices
def test_non_finite_vertices(hip):
    """One NaN and one Inf vertex in S0 (tests/test_gpu_volume_fused_amr.test_non_finite_vertices), lit fog plus the slice plane, on
    the fog-shadowed frame: the checker's bits, and the kernels end."""
    vol = ac.scene()
    s0 = vol.subgrids[0]
    data = s0.data.copy()
    data[8, 5, 6] = np.nan
    data[10, 6, 9] = np.inf
    wild = scenes.VolumeData(vol.data, vol.origin, vol.spacing, [scenes.Subgrid(s0.parent, s0.ratio, s0.lo, s0.cells, data)] + vol.subgrids[1:])
    S = scases.surfaces(vol, isovalues=(), opacity=0.3)
    whole, wlo, whi = fc.checker_bricks(fc.parts_of(wild, 1))
    bricks, lo, hi = fc.checker_bricks(fc.parts_of(wild, 8))
    G, _ = sa.grid(whole[0], wlo, whi, IDENT, IDENT, S, ac.GRID_BIAS)
    want, counters = sa.frame(bricks, lo, hi, IDENT, ac.camera("outside"), S, lc.SHADE_GRADIENT, G, None, None, ac.BIAS)
    assert (bits(want) != bits(ac.reference("fog", "surf_lit", 8, "outside")[0])).any()
    for skip in (True, False):
        tr = tracer("fog", "surf_lit", 8, parts=fc.parts_of(wild, 8), S=S, skip=skip).frame()
        grids_match(tr, G)
        check_frame(tr, "surf_lit", want, counters)


# ---- 9. the gates
def _raw_frame(tr, name, flags, stats=None):
    cam = tr.camera
    n = tr.n_inst
    pod = capi.CameraPod((C.c_float * 3)(*cam.eye), (C.c_float * 3)(*cam.focus), (C.c_float * 3)(*cam.up), cam.fov, cam.width, cam.height, 1, 1, 0.0)
    mm = np.ascontiguousarray(np.tile(tr.m, n), F)
    minv = np.ascontiguousarray(np.tile(tr.minv, n), F)
    params = capi.VolumeShadowParams(flags, ac.BIAS)
    return getattr(capi.load(), name)(tr.top.h, tr._arr(tr.adapters), capi.ptr(mm), capi.ptr(minv), C.c_size_t(n), C.byref(pod), tr._arr(tr.queues), tr.fb.h, None,
                                      C.byref(params), None if stats is None else C.byref(stats))


def test_unknown_flag_bits_change_nothing(hip):
    pattern = np.random.default_rng(12).random((ac.FILM[1], ac.FILM[0], 4)).astype(F)
    tr = tracer("fog", "surf_lit", 8).rebake()
    before = [a.light_grid(0).copy() for a in tr.adapters]
    _upload_fb(tr.fb, pattern)
    for flags in (1, 3, 5, 8, 12):
        for name in FRAMES:
            assert _raw_frame(tr, name, flags) == -1 and "flag" in capi.last_error(), (name, flags, capi.last_error())
        assert _raw_light_bake(tr.adapters, flags) == -1 and "flag" in capi.last_error(), flags
        assert _raw_occluder_bake(tr.adapters, flags) == -1 and "flag" in capi.last_error(), flags
    assert (bits(tr.framebuffer(False)) == bits(pattern)).all() and all(len(q) == 0 for q in tr.queues)
    for a, g in zip(tr.adapters, before):
        assert a.light_grid_info()["current"] == 1 and (bits(a.light_grid(0)) == bits(g)).all() and a.occluder_grid_info()["present"] == 0
    brick_counters_are_zero(tr)


def test_the_flag_changes_nothing_without_subgrids(hip):
    for kind, mode in (("shadow", "surf_lit"), ("fog", "surf_lit"), ("fog", "lit")):
        a = tracer(kind, mode, 8, which="plain", amr=True).frame()
        b = tracer(kind, mode, 8, which="plain", amr=False).frame()
        assert a.param_flags == capi.VOLUME_ALLOW_AMR and b.param_flags == 0
        sa_, sb = a.stats(), b.stats()
        assert sa_["features"] == sb["features"] == FEATURES[mode] and sa_["shadowed"] == sb["shadowed"] == 1
        assert (bits(a.framebuffer(False)) == bits(b.framebuffer(False))).all() and b.framebuffer(False).any()
        for key in SHADOW_KEYS + CAMERA_KEYS + ("samples_marched", "samples_gathered"):
            assert sa_[key] == sb[key], key


def test_selection(hip):
    pattern = np.random.default_rng(13).random((ac.FILM[1], ac.FILM[0], 4)).astype(F)
    # flags = 0 on AMR bricks: refused with "subgrids", as ever; flags = 4: accepted
    tr = tracer("shadow", "surf_lit", 8)
    _upload_fb(tr.fb, pattern)
    for name in FRAMES:
        assert _raw_frame(tr, name, 0) == -1 and "subgrids" in capi.last_error(), name
        assert _raw_frame(tr, name, capi.VOLUME_ALLOW_CENTRAL) == -1 and "subgrids" in capi.last_error(), name
    assert _raw_light_bake(tr.adapters, 0) == -1 and "subgrids" in capi.last_error()
    assert (bits(tr.framebuffer(False)) == bits(pattern)).all()
    st = capi.VolumeShadowStats()
    assert _raw_frame(tr, FRAMES[0], capi.VOLUME_ALLOW_AMR, st) == 0 and st.shadowed == 1 and st.features == AMR | SURF | LIT
    assert (bits(tr.framebuffer(False)) == bits(ac.reference("shadow", "surf_lit", 8, "outside")[0])).all()
    assert _raw_frame(tr, FRAMES[0], capi.VOLUME_ALLOW_AMR | capi.VOLUME_ALLOW_CENTRAL, None) == 0  # flags 6; stats may be NULL
    assert (bits(tr.framebuffer(False)) == bits(ac.reference("shadow", "surf_lit", 8, "outside")[0])).all()
    # the inert forward: no light at all, the frame is gvt_hip_volume_frame_fused_amr's
    inert = tracer("shadow", "surf", 8, S=ac.surfaces("surf", lights=[])[0]).frame()
    plain = tracer("fused", "surf", 8, S=ac.surfaces("surf", lights=[])[0]).frame()
    st = inert.stats()
    assert st["shadowed"] == 0 and st["fused"] == 1 and st["features"] == AMR | SURF and st["shadow_rays"] == 0
    assert (bits(inert.framebuffer(False)) == bits(plain.framebuffer(False))).all() and plain.framebuffer(False).any()
    with pytest.raises(ValueError):
        VolumeTracer(fc.parts_of(ac.scene(), 8), ac.camera("outside"), fc.thin(), shadow_amr=True)
    with pytest.raises(ValueError):
        MixedTracer(ac.mesh_scene(), fc.parts_of(ac.scene(), 8), ac.camera("outside"), fc.thin(), shadow_amr=True)


def test_central_bricks_beside_amr_bricks_are_refused(hip):
    """An isovalue, CENTRAL on the bricks without subgrids, flags 6: bricks of mixed kinds, and no loop renders shadows."""
    vol = ac.scene()
    parts = fc.parts_of(vol, 8)
    for b in parts:
        if not b.subgrids:
            off = [int(v) for v in b.offset]
            b.ghosts = scenes.brick_ghosts(vol.data, off, [o + int(c) - 1 for o, c in zip(off, b.counts)])
    tr = tracer("fog", "surf_lit", 8, parts=parts, fused_central=True)
    assert tr.param_flags == capi.VOLUME_ALLOW_AMR | capi.VOLUME_ALLOW_CENTRAL == 6
    for a, b in zip(tr.adapters, parts):
        if not b.subgrids:
            a.set_gradient("central")
    for name in FRAMES:
        assert _raw_frame(tr, name, 6) == -1 and "central" in capi.last_error(), (name, capi.last_error())
    assert _raw_light_bake(tr.adapters, 6) == -1 and "central" in capi.last_error()
