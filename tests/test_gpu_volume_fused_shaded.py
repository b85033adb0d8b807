"""The shaded fused frame on the device (csrc/volume_fused_shaded.inc, gvt_hip_volume_frame_fused_shaded) against the frame loop
(gvt_hip_volume_frame / _clipped) and the numpy per-ray checker, bit for bit: every mode, bricking, eye and skip flag of
tests/volume_fused_shaded_cases.py, the counters, the variants (no lights, ka = 1 / kd = 0, typed voxels, the clipped and the mixed
frame), the selection of the kernel and the fallbacks."""
import ctypes as C

import numpy as np
import pytest

from gravit_amd import capi, scenes
from gravit_amd.adapter import DepthPlane
from gravit_amd.scheduler import MixedTracer, VolumeTracer
from tests import volume_fused_cases as fc
from tests import volume_fused_shaded_cases as sh
from tests.volume_common import as_float, quantised, scaled, tf

pytestmark = pytest.mark.gpu

F = np.float32
BOTH = capi.FUSED_SURFACES | capi.FUSED_LIT


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def dress(tr, mode, S=None, on=None):
    """The mode's surfaces, lights and shading on every brick of a VolumeTracer or MixedTracer."""
    if S is None:
        S, on = sh.surfaces(mode)
    if len(S):
        tr.set_surfaces(S.iso, S.planes, float(S.opacity))
    tr.set_lights(list(zip(S.lpos, S.lcol)), float(S.ka), float(S.kd))
    tr.set_shading(on)
    return tr


def tracer(split, mode, where="inside", skip=True, fused=True, vol=None, native=False, t=None, parts=None, S=None, on=None):
    moved = sh.CAMERAS[where]
    if parts is None:
        parts = fc.bricks_of(fc.volume() if vol is None else vol, split)
    tr = VolumeTracer(parts, fc.camera(where, moved), tf(sh.MODES.get(mode, "cool")) if t is None else t, m=fc.matrix(moved), sampling_rate=fc.RATE, skip=skip,
                      native=native, fused=fused, fused_shaded=fused)
    return dress(tr, mode, S, on) if mode in sh.MODES or S is not None else tr


@pytest.mark.parametrize("skip", [True, False])
@pytest.mark.parametrize("where", sorted(sh.CAMERAS))
@pytest.mark.parametrize("split", fc.SPLITS)
@pytest.mark.parametrize("mode", sorted(sh.MODES))
def test_shaded_fused_frame_has_the_loops_bits(hip, mode, split, where, skip):
    want = sh.reference(split, mode, where)[0]
    loop = tracer(split, mode, where, skip, fused=False).frame().framebuffer(False).copy()
    tr = tracer(split, mode, where, skip).frame()
    got = tr.framebuffer(False)
    st = tr.stats()
    assert st["fused"] == 1 and st["adapter_calls"] == 1 and st["features"] == sh.FEATURES[mode]
    assert got.any()
    assert (bits(got) == bits(loop)).all()
    assert (bits(got) == bits(want)).all()


@pytest.mark.parametrize("mode", sorted(sh.MODES))
def test_the_cut_does_not_show(hip, mode):
    frames = [tracer(s, mode, "inside").frame().framebuffer(False).copy() for s in fc.SPLITS]
    for f in frames[1:]:
        assert (bits(f) == bits(frames[0])).all()


@pytest.mark.parametrize("split", [(2, 2, 2), (4, 4, 4)])
@pytest.mark.parametrize("mode", sorted(sh.MODES))
def test_counters(hip, mode, split):
    loop = tracer(split, mode, "inside", fused=False).frame()
    tr = tracer(split, mode, "inside").frame()
    ls, fs = loop.stats(), tr.stats()
    want = sh.reference(split, mode, "inside")[1]
    assert "fused" not in ls and "features" not in ls
    for key in ("samples_marched", "samples_gathered", "crossings_rendered", "samples_shaded"):
        assert fs[key] == ls[key], key
    assert fs["samples_marched"] > 0 and fs["samples_gathered"] > 0
    for key in ("crossings_rendered", "samples_shaded", "brick_visits", "rays_deposited"):
        assert fs[key] == want[key], key
    assert (fs["crossings_rendered"] > 0) == (mode != "lit") and (fs["samples_shaded"] > 0) == (mode != "surf")
    # the bricks' own counters are not touched
    assert sum(a.info()["samples_marched"] + a.info()["samples_gathered"] + a.crossings() + a.shaded() for a in tr.adapters) == 0
    assert all(len(q) == 0 for q in tr.queues)


def test_surfaces_without_lights(hip):
    S, _ = sh.surfaces("surf", lights=())
    loop = tracer((2, 2, 2), None, S=S, on=False, fused=False).frame().framebuffer(False).copy()
    tr = tracer((2, 2, 2), None, S=S, on=False).frame()
    st = tr.stats()
    assert st["fused"] == 1 and st["features"] == capi.FUSED_SURFACES and st["crossings_rendered"] > 0
    assert (bits(tr.framebuffer(False)) == bits(loop)).all()
    lit = tracer((2, 2, 2), "surf").frame().framebuffer(False)
    assert (bits(lit) != bits(loop)).any()  # the lights show on the crossings


@pytest.mark.parametrize("mode", ["lit", "surf_lit"])
def test_ambient_alone_gives_the_unlit_bits(hip, mode):
    """ka = 1, kd = 0: rgb * (1 + 0 * sum) = rgb"""
    S, on = sh.surfaces(mode, ka=1.0, kd=0.0)
    tr = tracer((2, 2, 2), mode, S=S, on=on).frame()
    st = tr.stats()
    assert st["fused"] == 1 and st["features"] == sh.FEATURES[mode] and st["samples_shaded"] > 0
    got = tr.framebuffer(False).copy()
    tr.set_shading(False).frame()
    st = tr.stats()
    assert st["fused"] == 1 and st["features"] == (capi.FUSED_SURFACES if mode == "surf_lit" else 0) and st["samples_shaded"] == 0
    unlit = tr.framebuffer(False)
    if mode == "surf_lit":  # (the crossings are lit with ka = 1, kd = 0 in both frames)
        assert (bits(got) == bits(unlit)).all()
    else:
        assert (bits(got) == bits(tracer((2, 2, 2), None, fused=True, t=tf("cool")).frame().framebuffer(False))).all()
        assert (bits(got) == bits(unlit)).all()


def test_typed_voxels(hip):
    vol, t = quantised(fc.volume(), "u8"), scaled(sh.MODES["surf_lit"], "u8")
    S, on = sh.surfaces("surf_lit", scale=255.0)
    loop = tracer((2, 2, 2), "surf_lit", vol=vol, native=True, t=t, S=S, on=on, fused=False).frame().framebuffer(False).copy()
    tr = tracer((2, 2, 2), "surf_lit", vol=vol, native=True, t=t, S=S, on=on).frame()
    st = tr.stats()
    assert tr.adapters[0].dtype_name == "uint8" and st["fused"] == 1 and st["features"] == BOTH
    got = tr.framebuffer(False)
    flt = tracer((2, 2, 2), "surf_lit", vol=as_float(vol), t=t, S=S, on=on).frame()
    assert flt.stats()["fused"] == 1
    assert got.any()
    assert (bits(got) == bits(loop)).all()
    assert (bits(got) == bits(flt.framebuffer(False))).all()


@pytest.mark.parametrize("mode", sorted(sh.MODES))
def test_clipped_shaded_fused_frame(hip, mode):
    want, _, plane = sh.reference((2, 2, 2), mode, "outside", True)
    depth = DepthPlane(fc.FILM[0], fc.FILM[1]).upload(plane)
    parts = fc.bricks_of(fc.volume(), (2, 2, 2))

    def make(fused):
        return dress(VolumeTracer(parts, fc.camera("outside", False), tf(sh.MODES[mode]), m=fc.matrix(False), sampling_rate=fc.RATE, fused=fused, fused_shaded=fused), mode)

    loop = make(False).frame(depth).framebuffer(False).copy()
    tr = make(True).frame(depth)
    got = tr.framebuffer(False)
    st = tr.stats()
    assert st["fused"] == 1 and st["features"] == sh.FEATURES[mode]
    assert (bits(got) == bits(loop)).all()
    assert (bits(got) == bits(want)).all()
    assert (bits(got) != bits(make(True).frame().framebuffer(False))).any()  # the clip shows


def test_mixed_frame(hip):
    cam = scenes.Camera((0.0, 0.1, 0.3), (0.0, 0.1, -0.3), (0.0, 1.0, 0.0), float(F(45.0 * np.pi / 180.0)), 150, 110)
    scene = scenes.bunny_scene(150, 110)
    parts = scenes.split_volume(scenes.mesh_in_volume(scene, scenes.sphere_volume(64), fill=0.6), 2, 2, 2)
    S, on = sh.surfaces("surf_lit")

    def make(**kw):
        mt = MixedTracer(scene, parts, cam, tf("ramp"), sampling_rate=1.0, **kw)
        mt.volume.set_surfaces([0.3, 0.5], [], 0.6)
        mt.volume.set_lights(list(zip(S.lpos, S.lcol))).set_shading(True)
        return mt

    want = make().frame().framebuffer(False).copy()
    mt = make(fused=True, fused_shaded=True).frame()
    st = mt.volume.stats()
    assert st["fused"] == 1 and st["features"] == BOTH and mt.volume.calls == 1 and st["crossings_rendered"] > 0 and st["samples_shaded"] > 0
    assert (bits(mt.framebuffer(False)) == bits(want)).all()
    only = MixedTracer(scene, parts, cam, tf("ramp"), sampling_rate=1.0, fused=True).frame().framebuffer(False)
    assert (bits(only) != bits(want)).any()  # the surfaces and the lights show


def _loop_and(tr):
    """The loop's frame and call count of the tracer as it is now, then the tracer's own frame: (loop bits, loop calls, got, stats)."""
    tr.fused = False
    loop = tr.frame().framebuffer(False).copy()
    calls = tr.calls
    tr.fused = True
    got = tr.frame().framebuffer(False).copy()
    return loop, calls, got, tr.stats()


def _fell_back(tr):
    loop, calls, got, st = _loop_and(tr)
    assert st["fused"] == 0 and st["features"] == 0 and st["adapter_calls"] == calls > 1 and st["brick_visits"] == 0  # the loop ran: a march per round
    assert got.any() and (bits(got) == bits(loop)).all()


def test_allow_decides(hip):
    tr = tracer((2, 2, 2), "surf")
    tr.fused_allow = 0
    _fell_back(tr)
    tr.fused_allow = capi.FUSED_LIT  # not the bit this frame needs
    _fell_back(tr)
    tr.fused_allow = capi.FUSED_SURFACES
    assert tr.frame().stats()["fused"] == 1
    both = tracer((2, 2, 2), "surf_lit")
    for allow in (capi.FUSED_LIT, capi.FUSED_SURFACES, 0):
        both.fused_allow = allow
        _fell_back(both)
    both.fused_allow = BOTH
    assert both.frame().stats()["features"] == BOTH
    lit = tracer((2, 2, 2), "lit")
    lit.fused_allow = capi.FUSED_SURFACES
    _fell_back(lit)
    lit.fused_allow = capi.FUSED_LIT
    assert lit.frame().stats()["features"] == capi.FUSED_LIT


def test_central_gradients_fall_back(hip):
    parts = scenes.split_volume(fc.volume(), 2, 2, 2, ghosts=True)
    tr = tracer((2, 2, 2), "surf_lit", parts=parts).frame()
    assert tr.stats()["fused"] == 1
    tr.set_gradient("central")
    _fell_back(tr)
    tr.set_surfaces().set_shading(False)  # neither an isovalue nor lit shading: the kind is inert, the plain fused kernel runs
    st = tr.frame().stats()
    assert st["fused"] == 1 and st["features"] == 0


def test_amr_falls_back(hip):
    tr = tracer((2, 2, 2), None, t=tf("cool"))
    assert tr.frame().stats()["fused"] == 1
    b = fc.bricks_of(fc.volume(), (2, 2, 2))[0]
    scenes.refine(b, np.asarray(b.offset) + 1, (2, 2, 2), 2, seed=5)
    tr.adapters[0].set_subgrids(b.subgrids)
    _fell_back(tr)


def test_bricks_that_differ_fall_back(hip):
    tr = tracer((2, 2, 2), "surf_lit").frame()
    assert tr.stats()["fused"] == 1
    right = tr.framebuffer(False).copy()
    S, on = sh.surfaces("surf_lit")
    tr.adapters[5].set_surfaces([S.iso[0], 0.7], S.planes, float(S.opacity))  # another isovalue on one brick
    _fell_back(tr)
    tr.adapters[5].set_surfaces(S.iso, S.planes, float(S.opacity))
    assert tr.frame().stats()["fused"] == 1 and (bits(tr.framebuffer(False)) == bits(right)).all()
    lights = [(tuple(p), tuple(c)) for p, c in zip(S.lpos, S.lcol)]
    tr.adapters[2].set_lights([lights[0], (lights[1][0], (0.3, 0.4, 0.8))], float(S.ka), float(S.kd))  # another light colour on one brick
    _fell_back(tr)
    tr.adapters[2].set_lights(lights, float(S.ka), float(S.kd))
    assert tr.frame().stats()["fused"] == 1 and (bits(tr.framebuffer(False)) == bits(right)).all()


def test_plain_frames_take_the_plain_fused_kernel(hip):
    plain = VolumeTracer(fc.bricks_of(fc.volume(), (2, 2, 2)), fc.camera("inside", False), tf("spikes"), m=fc.matrix(False), sampling_rate=fc.RATE,
                         fused=True).frame().framebuffer(False).copy()
    tr = tracer((2, 2, 2), "surf_lit").frame()
    assert tr.stats()["features"] == BOTH and (bits(tr.framebuffer(False)) != bits(plain)).any()
    tr.set_surfaces().set_shading(False)
    st = tr.frame().stats()
    assert st["fused"] == 1 and st["features"] == 0 and st["crossings_rendered"] == 0 and st["samples_shaded"] == 0
    assert (bits(tr.framebuffer(False)) == bits(plain)).all()


def test_unknown_allow_bits_change_nothing(hip):
    lib = capi.load()
    tr = tracer((2, 2, 2), "surf_lit").frame()
    before = tr.framebuffer(False).copy()
    cam = tr.camera
    pod = capi.CameraPod((C.c_float * 3)(*cam.eye), (C.c_float * 3)(*cam.focus), (C.c_float * 3)(*cam.up), cam.fov, cam.width, cam.height, 1, 1, 0.0)
    m = np.ascontiguousarray(np.tile(tr.m, tr.n_inst), F)
    minv = np.ascontiguousarray(np.tile(tr.minv, tr.n_inst), F)
    vols, qs, n = tr._arr(tr.adapters), tr._arr(tr.queues), C.c_size_t(tr.n_inst)
    call = lib.gvt_hip_volume_frame_fused_shaded
    for allow in (4, 7, 0x80000000):
        st = capi.VolumeFusedShadedStats(fused=77, features=78, samples_marched=79)
        assert call(tr.top.h, vols, capi.ptr(m), capi.ptr(minv), n, C.byref(pod), qs, tr.fb.h, None, allow, C.byref(st)) == -1
        assert "allow" in capi.last_error()
        assert (st.fused, st.features, st.samples_marched) == (77, 78, 79)
        assert (bits(tr.framebuffer(False)) == bits(before)).all()
    assert call(None, vols, capi.ptr(m), capi.ptr(minv), n, C.byref(pod), qs, tr.fb.h, None, BOTH, None) == -1  # volume_frame_args' errors
    assert call(tr.top.h, vols, capi.ptr(m), capi.ptr(minv), n, C.byref(pod), qs, tr.fb.h, None, BOTH, None) == 0  # stats may be NULL
    assert (bits(tr.framebuffer(False)) == bits(before)).all()
    st = capi.VolumeFusedStats()  # allow == 0 is gvt_hip_volume_frame_fused: the loop for this frame
    st2 = capi.VolumeFusedShadedStats()
    assert lib.gvt_hip_volume_frame_fused(tr.top.h, vols, capi.ptr(m), capi.ptr(minv), n, C.byref(pod), qs, tr.fb.h, None, C.byref(st)) == 0
    assert call(tr.top.h, vols, capi.ptr(m), capi.ptr(minv), n, C.byref(pod), qs, tr.fb.h, None, 0, C.byref(st2)) == 0
    assert st.fused == st2.fused == 0 and st.adapter_calls == st2.adapter_calls > 1
    assert (bits(tr.framebuffer(False)) == bits(before)).all()
