"""The fused frame over bricks with AMR subgrids on the device (gvt_hip_volume_frame_fused_amr, GVT_HIP_FUSED_AMR; csrc/
volume_fused_amr.inc) against the loop (gvt_hip_volume_frame / _clipped) and the numpy checker (tests/volume_fused_amr_checker.py), bit
for bit: plain, surface and lit frames over one brick and over eight of which two have subgrids, from outside and from inside a
subgrid; the counters; the clipped and the mixed frame; merged ranges; non-finite vertices; tables replaced between frames; the gates."""
import ctypes as C
from dataclasses import replace

import numpy as np
import pytest
import torch  # noqa: F401  (before the library initialises the device, as in test_gpu_volume_amr.py)

from gravit_amd import capi, scenes
from gravit_amd.adapter import DepthPlane
from gravit_amd.scheduler import MixedTracer, NativeTracer, VolumeTracer
from tests import volume_amr_cases as cases
from tests import volume_amr_surface_cases as scases
from tests import volume_fused_amr_cases as fc
from tests.test_gpu_volume import tf
from tests.test_gpu_volume_amr import camera as amr_camera
from tests.test_gpu_volume_amr_surfaces import clear

pytestmark = pytest.mark.gpu

F = np.float32
MODES = sorted(fc.MODES)
SHADED = capi.FUSED_SURFACES | capi.FUSED_LIT
FUSED = dict(fused=True, fused_shaded=True, fused_amr=True)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def dress(tr, mode, S):
    """The mode on every brick: surfaces for surf / surf_lit, the light for everything but plain, lit fog for lit / surf_lit."""
    if mode in ("surf", "surf_lit"):
        tr.set_surfaces(**S.args)
    if mode != "plain":
        tr.set_lights(**S.light_args)
        tr.set_shading(mode in ("lit", "surf_lit"))
    return tr


def tracer(parts, cam, mode, skip=True, t=None, S=None, cls=VolumeTracer, scene=None, **kw):
    S = fc.surfaces() if S is None else S
    t = fc.thin() if t is None else t
    args = (parts, cam, t) if scene is None else (scene, parts, cam, t)
    return dress(cls(*args, sampling_rate=fc.RATE, skip=skip, amr_shaded=True, **kw), mode, S)


def brick_counters_are_zero(tr):
    for a in tr.adapters:
        info, amr = a.info(), a.amr_info()
        assert info["samples_marched"] == info["samples_gathered"] == 0 and a.crossings() == 0 and a.shaded() == 0
        assert amr["amr_marches"] == 0 and amr["samples_refined"] == 0
    assert all(len(q) == 0 for q in tr.queues)


def test_the_outside_eye_is_the_amr_tests_camera():
    assert fc.camera("outside") == amr_camera()


@pytest.mark.parametrize("skip", [True, False])
@pytest.mark.parametrize("where", fc.EYES)
@pytest.mark.parametrize("bricking", fc.BRICKINGS)
@pytest.mark.parametrize("mode", MODES)
def test_fused_amr_frame_has_the_loops_bits(hip, mode, bricking, where, skip):
    parts, cam = fc.parts_of(fc.scene(), bricking), fc.camera(where)
    want, counts, _ = fc.reference(mode, bricking, where)
    loop = tracer(parts, cam, mode, skip).frame()
    tr = tracer(parts, cam, mode, skip, **FUSED).frame()
    st = tr.stats()
    assert st["fused"] == 1 and st["adapter_calls"] == 1 and st["features"] == capi.FUSED_AMR | fc.MODES[mode]
    got = tr.framebuffer(False)
    assert (bits(got) == bits(loop.framebuffer(False))).all()
    assert (bits(got) == bits(want)).all()
    assert st["samples_refined"] > 0 and (got[..., 3] > 0).sum() > 300
    assert loop.calls == 1 if bricking == 1 else loop.calls > 1


@pytest.mark.parametrize("where", fc.EYES)
@pytest.mark.parametrize("mode", MODES)
def test_the_cut_does_not_show(hip, mode, where):
    cam = fc.camera(where)
    one = tracer(fc.parts_of(fc.scene(), 1), cam, mode, **FUSED).frame()
    eight = tracer(fc.parts_of(fc.scene(), 8), cam, mode, **FUSED).frame()
    assert one.stats()["fused"] == eight.stats()["fused"] == 1
    assert (bits(one.framebuffer(False)) == bits(eight.framebuffer(False))).all()


@pytest.mark.parametrize("skip", [True, False])
@pytest.mark.parametrize("bricking", fc.BRICKINGS)
@pytest.mark.parametrize("mode", MODES)
def test_counters(hip, mode, bricking, skip):
    parts, cam = fc.parts_of(fc.scene(), bricking), fc.camera("outside")
    _, counts, _ = fc.reference(mode, bricking, "outside")
    loop = tracer(parts, cam, mode, skip).frame().stats()
    tr = tracer(parts, cam, mode, skip, **FUSED).frame()
    st = tr.stats()
    for key in ("samples_marched", "samples_gathered", "crossings_rendered", "samples_shaded", "samples_refined"):
        assert st[key] == loop[key], key
    assert st["samples_marched"] > 0 and st["samples_refined"] > 0 and st["amr_marches"] == 0 and loop["amr_marches"] > 0
    assert st["brick_visits"] == counts["brick_visits"] and st["rays_deposited"] == counts["rays_deposited"]
    assert st["crossings_rendered"] == counts["crossings"] and st["samples_shaded"] == counts["shaded"]
    if not skip:  # (the checker interpolates every sample)
        assert st["samples_refined"] == counts["samples_refined"] and st["samples_gathered"] == st["samples_marched"]
    else:
        assert st["samples_refined"] <= counts["samples_refined"]
    assert st["amr_bricks"] == (2 if bricking == 8 else 1)
    brick_counters_are_zero(tr)


@pytest.mark.parametrize("bricking", fc.BRICKINGS)
def test_clipped_frame(hip, bricking):
    parts, cam = fc.parts_of(fc.scene(), bricking), fc.camera("outside")
    want, counts, plane = fc.reference("surf_lit", bricking, "outside", True)
    assert np.isfinite(plane).sum() > 1000
    depth = DepthPlane(cam.width, cam.height).upload(plane)
    loop = tracer(parts, cam, "surf_lit").frame(depth).framebuffer(False).copy()
    tr = tracer(parts, cam, "surf_lit", **FUSED).frame(depth)
    st = tr.stats()
    assert st["fused"] == 1 and st["features"] == capi.FUSED_AMR | SHADED and st["brick_visits"] == counts["brick_visits"]
    assert (bits(tr.framebuffer(False)) == bits(loop)).all() and (bits(loop) == bits(want)).all()
    assert (bits(loop) != bits(fc.reference("surf_lit", bricking, "outside")[0])).any()  # the clip shows
    plain = tracer(parts, cam, "plain", **FUSED).frame(depth)
    assert plain.stats()["features"] == capi.FUSED_AMR
    assert (bits(plain.framebuffer(False)) == bits(fc.reference("plain", bricking, "outside", True)[0])).all()


def test_mixed_frame(hip):
    """tests/test_gpu_volume_amr_surfaces.test_mixed_frame_over_shaded_amr_bricks' tetrahedron inside S0's box, over one brick and eight."""
    vol, cam = fc.scene(), fc.camera("outside")
    verts = np.array([[-1, -1, -1], [1, -1, -1], [0, 1, -1], [0, 0, 1]], F)
    tris = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]], np.int32)
    scene = scenes._assemble([scenes.MeshData(verts, tris)], [0], [scenes.mat_translate_scale(tuple(fc.s0_centre(vol)), (0.13, 0.13, 0.13))],
                             scenes.point_light((1.0, 2.0, 3.0)), cam, "tetrahedron")
    mesh_only = NativeTracer(replace(scene, camera=cam))().framebuffer(False).copy()
    for bricking in fc.BRICKINGS:
        parts = fc.parts_of(vol, bricking)
        want = tracer(parts, cam, "surf_lit", cls=MixedTracer, scene=scene).frame().framebuffer(False).copy()
        mt = tracer(parts, cam, "surf_lit", cls=MixedTracer, scene=scene, **FUSED).frame()
        st = mt.volume.stats()
        assert st["fused"] == 1 and st["features"] == capi.FUSED_AMR | SHADED and mt.volume.calls == 1 and st["samples_refined"] > 0
        assert (bits(mt.framebuffer(False)) == bits(want)).all()
        assert (bits(want) != bits(mesh_only)).any() and 20 < np.isfinite(mt.depth.download()).sum() < cam.width * cam.height // 2


def test_merged_ranges(hip):
    """A skip decision taken from level-0 ranges would blank both scenes: the opacity (the crossed isovalue) lives in the subgrids alone."""
    cam = fc.camera("outside")
    vol = cases.level0(np.full(cases.COUNTS[::-1], 0.2, F))
    s0 = scenes.refine(vol, cases.S0["lo"], cases.S0["cells"], cases.S0["ratio"], fn=lambda x, y, z: 0.9 + 0 * (x + y + z))
    scenes.refine(vol, cases.S1["lo"], cases.S1["cells"], cases.S1["ratio"], parent=s0, fn=lambda x, y, z: 0.9 + 0 * (x + y + z))
    peak = scases.peak_scene()
    S_peak = scases.surfaces(peak, isovalues=(scases.PEAK_ISO,), plane=False)
    for scene_vol, t, mode, S in ((vol, tf("spikes"), "plain", None), (peak, clear(), "surf_lit", S_peak)):
        parts = fc.parts_of(scene_vol, 8)
        frames = []
        for skip in (True, False):
            loop = tracer(parts, cam, mode, skip, t=t, S=S).frame().framebuffer(False).copy()
            tr = tracer(parts, cam, mode, skip, t=t, S=S, **FUSED).frame()
            st = tr.stats()
            assert st["fused"] == 1 and st["features"] & capi.FUSED_AMR and st["samples_refined"] > 0
            got = tr.framebuffer(False).copy()
            assert (bits(got) == bits(loop)).all() and (got[..., 3] > 0).sum() > 0
            frames.append((got, st))
        assert (bits(frames[0][0]) == bits(frames[1][0])).all()
        assert frames[0][1]["samples_gathered"] < frames[1][1]["samples_gathered"] == frames[1][1]["samples_marched"]  # ... and the rest is skipped


def test_non_finite_vertices(hip):
    """One NaN and one Inf vertex in S0 (tests/test_gpu_volume_amr_surfaces.test_non_finite_vertices), lit fog plus the slice plane."""
    vol, cam = fc.scene(), fc.camera("outside")
    s0 = vol.subgrids[0]
    data = s0.data.copy()
    data[8, 5, 6] = np.nan
    data[10, 6, 9] = np.inf
    wild = scenes.VolumeData(vol.data, vol.origin, vol.spacing, [scenes.Subgrid(s0.parent, s0.ratio, s0.lo, s0.cells, data)] + vol.subgrids[1:])
    S = scases.surfaces(vol, isovalues=(), opacity=0.3)
    parts = fc.parts_of(wild, 8)
    clean = tracer(fc.parts_of(vol, 8), cam, "surf_lit", S=S, **FUSED).frame().framebuffer(False).copy()
    for skip in (True, False):
        loop = tracer(parts, cam, "surf_lit", skip, S=S).frame().framebuffer(False).copy()
        tr = tracer(parts, cam, "surf_lit", skip, S=S, **FUSED).frame()
        assert tr.stats()["fused"] == 1 and tr.stats()["features"] == capi.FUSED_AMR | SHADED
        assert (bits(tr.framebuffer(False)) == bits(loop)).all()
        assert (bits(loop) != bits(clean)).any()  # the two vertices show


def test_tables_are_read_per_call(hip):
    vol, cam = fc.scene(), fc.camera("outside")
    parts = fc.parts_of(vol, 8)
    assert parts[0].subgrids and parts[7].subgrids
    tr = tracer(parts, cam, "surf_lit", **FUSED).frame()
    first = tr.framebuffer(False).copy()
    assert (bits(first) == bits(fc.reference("surf_lit", 8, "outside")[0])).all()
    # other data in the subgrids of the brick that holds S0: the old device tables are freed and replaced
    other = [scenes.Subgrid(s.parent, s.ratio, s.lo, s.cells, np.ascontiguousarray(s.data[::-1, ::-1, ::-1] * F(0.9) + F(0.03))) for s in parts[0].subgrids]
    tr.adapters[0].set_subgrids(other)
    parts2 = fc.parts_of(vol, 8)
    parts2[0].subgrids = other
    want2 = tracer(parts2, cam, "surf_lit").frame().framebuffer(False).copy()
    second = tr.frame().framebuffer(False).copy()
    assert tr.stats()["fused"] == 1 and (bits(second) == bits(want2)).all() and (bits(second) != bits(first)).any()
    # no subgrids anywhere: what gvt_hip_volume_frame_fused_shaded launches, and its bits
    for a in tr.adapters:
        a.set_subgrids([])
    st = tr.frame().stats()
    assert st["fused"] == 1 and st["features"] == SHADED and st["samples_refined"] == 0 and st["amr_bricks"] == 0
    shaded = tracer(fc.parts_of(scenes.VolumeData(vol.data, vol.origin, vol.spacing), 8), cam, "surf_lit", fused=True, fused_shaded=True).frame()
    assert shaded.stats()["fused"] == 1 and shaded.stats()["features"] == SHADED
    assert (bits(tr.framebuffer(False)) == bits(shaded.framebuffer(False))).all() and (bits(tr.framebuffer(False)) != bits(first)).any()
    # ... and the subgrids again: the first frame's bits
    for a, b in zip(tr.adapters, parts):
        if b.subgrids:
            a.set_subgrids(b.subgrids)
    st = tr.frame().stats()
    assert st["features"] == capi.FUSED_AMR | SHADED and st["amr_bricks"] == 2 and (bits(tr.framebuffer(False)) == bits(first)).all()


def _fell_back(tr, want):
    st = tr.frame().stats()
    assert st["fused"] == 0 and st["features"] == 0 and st["adapter_calls"] > 1 and st["brick_visits"] == 0 and st.get("amr_bricks", 0) == 0
    assert (bits(tr.framebuffer(False)) == bits(want)).all()


def test_selection(hip):
    cam = fc.camera("outside")
    parts = fc.parts_of(fc.scene(), 8)
    want = fc.reference("surf_lit", 8, "outside")[0]
    # without the bit: the loop, as ever; shadows on AMR bricks: refused, as ever
    _fell_back(tracer(parts, cam, "surf_lit", fused=True, fused_shaded=True), want)
    with pytest.raises(capi.GvtHipError):
        tracer(parts, cam, "surf_lit", shadows=True).frame()
    with pytest.raises(capi.GvtHipError):
        tracer(parts, cam, "surf_lit", shadows=True, **FUSED).frame()
    with pytest.raises(ValueError):
        VolumeTracer(parts, cam, fc.thin(), fused_amr=True)
    # allow = FUSED_AMR alone: the plain AMR frame is fused, the surface frame takes the loop
    only = tracer(parts, cam, "plain", fused=True, fused_amr=True)
    assert only.fused_amr_allow == capi.FUSED_AMR
    st = only.frame().stats()
    assert st["fused"] == 1 and st["features"] == capi.FUSED_AMR
    assert (bits(only.framebuffer(False)) == bits(fc.reference("plain", 8, "outside")[0])).all()
    _fell_back(tracer(parts, cam, "surf", fused=True, fused_amr=True), fc.reference("surf", 8, "outside")[0])
    _fell_back(tracer(parts, cam, "lit", fused=True, fused_amr=True), fc.reference("lit", 8, "outside")[0])
    # an unflagged AMR set still refuses surfaces
    unflagged = VolumeTracer(parts, cam, fc.thin(), sampling_rate=fc.RATE, **FUSED)
    with pytest.raises(capi.GvtHipError):
        unflagged.set_surfaces(**fc.surfaces().args)
    assert unflagged.frame().stats()["features"] == capi.FUSED_AMR


def test_unknown_allow_bits_change_nothing(hip):
    lib = capi.load()
    cam = fc.camera("outside")
    tr = tracer(fc.parts_of(fc.scene(), 8), cam, "surf_lit", **FUSED).frame()
    before = tr.framebuffer(False).copy()
    pod = capi.CameraPod((C.c_float * 3)(*cam.eye), (C.c_float * 3)(*cam.focus), (C.c_float * 3)(*cam.up), cam.fov, cam.width, cam.height, 1, 1, 0.0)
    m = np.ascontiguousarray(np.tile(tr.m, tr.n_inst), F)
    minv = np.ascontiguousarray(np.tile(tr.minv, tr.n_inst), F)
    vols, qs, n = tr._arr(tr.adapters), tr._arr(tr.queues), C.c_size_t(tr.n_inst)
    # bit 16 through the entry point that does not know it
    st = capi.VolumeFusedShadedStats(fused=77, features=78, samples_marched=79)
    assert lib.gvt_hip_volume_frame_fused_shaded(tr.top.h, vols, capi.ptr(m), capi.ptr(minv), n, C.byref(pod), qs, tr.fb.h, None, capi.FUSED_AMR | SHADED, C.byref(st)) == -1
    assert "allow" in capi.last_error() and (st.fused, st.features, st.samples_marched) == (77, 78, 79)
    assert (bits(tr.framebuffer(False)) == bits(before)).all()
    call = lib.gvt_hip_volume_frame_fused_amr
    for allow in (4, 32, 0x80000000, 4 | capi.FUSED_AMR | SHADED):
        st = capi.VolumeFusedAmrStats(fused=77, features=78, samples_marched=79, samples_refined=80, amr_bricks=81)
        assert call(tr.top.h, vols, capi.ptr(m), capi.ptr(minv), n, C.byref(pod), qs, tr.fb.h, None, allow, C.byref(st)) == -1
        assert "allow" in capi.last_error()
        assert (st.fused, st.features, st.samples_marched, st.samples_refined, st.amr_bricks) == (77, 78, 79, 80, 81)
        assert (bits(tr.framebuffer(False)) == bits(before)).all()
    brick_counters_are_zero(tr)
    assert call(None, vols, capi.ptr(m), capi.ptr(minv), n, C.byref(pod), qs, tr.fb.h, None, capi.FUSED_AMR, None) == -1  # volume_frame_args' errors
    assert call(tr.top.h, vols, capi.ptr(m), capi.ptr(minv), n, C.byref(pod), qs, tr.fb.h, None, capi.FUSED_AMR | SHADED, None) == 0  # stats may be NULL
    assert (bits(tr.framebuffer(False)) == bits(before)).all()
    # without the bit the call is gvt_hip_volume_frame_fused_shaded: the loop for this frame, the new fields 0
    st = capi.VolumeFusedAmrStats(samples_refined=80, amr_bricks=81)
    assert call(tr.top.h, vols, capi.ptr(m), capi.ptr(minv), n, C.byref(pod), qs, tr.fb.h, None, SHADED | capi.FUSED_CENTRAL, C.byref(st)) == 0
    assert st.fused == 0 and st.features == 0 and st.adapter_calls > 1 and st.samples_refined == 0 and st.amr_bricks == 0
    assert (bits(tr.framebuffer(False)) == bits(before)).all()


def test_central_bricks_beside_amr_bricks_take_the_loop(hip):
    """An isovalue, CENTRAL on the bricks without subgrids (a brick with subgrids shades with the cell gradient only), every bit set:
    bricks of mixed kinds, the loop."""
    vol, cam = fc.scene(), fc.camera("outside")
    parts = fc.parts_of(vol, 8)
    for b in parts:
        if not b.subgrids:
            off = [int(v) for v in b.offset]
            b.ghosts = scenes.brick_ghosts(vol.data, off, [o + int(c) - 1 for o, c in zip(off, b.counts)])

    def make(**kw):
        tr = tracer(parts, cam, "surf_lit", fused_central=True, **kw)
        for a, b in zip(tr.adapters, parts):
            if not b.subgrids:
                a.set_gradient("central")
        return tr

    want = make().frame().framebuffer(False).copy()
    tr = make(**FUSED)
    assert tr.fused_amr_allow == capi.FUSED_AMR | SHADED | capi.FUSED_CENTRAL
    _fell_back(tr, want)
    assert (bits(want) != bits(fc.reference("surf_lit", 8, "outside")[0])).any()  # the central gradients show
    assert sum(a.central_marches() for a in tr.adapters) > 0
