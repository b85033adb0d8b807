"""The fused frame on the device (csrc/volume_fused.inc, gvt_hip_volume_frame_fused) against the frame loop (gvt_hip_volume_frame /
_clipped) and the numpy checkers, bit for bit: every bricking, table, matrix, skip flag and eye of tests/volume_fused_cases.py, the
counters, typed voxels, the clipped and the mixed frame, rays that meet no brick, the fallbacks, a time step and the argument errors."""
import ctypes as C

import numpy as np
import pytest

from gravit_amd import capi, scenes
from gravit_amd.adapter import DepthPlane, HipVolumeAdapter
from gravit_amd.scheduler import MixedTracer, VolumeTracer
from tests import volume_fused_cases as fc
from tests.test_gpu_volume import tf
from tests.test_gpu_volume_types import as_float, quantised, scaled

pytestmark = pytest.mark.gpu

F = np.float32


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def tracer(split, table="cool", moved=False, where="outside", skip=True, fused=True, vol=None, native=False, t=None):
    parts = fc.bricks_of(fc.volume() if vol is None else vol, split)
    return VolumeTracer(parts, fc.camera(where, moved), tf(table) if t is None else t, m=fc.matrix(moved), sampling_rate=fc.RATE, skip=skip, native=native,
                        fused=fused)


@pytest.mark.parametrize("where", ["outside", "inside"])
@pytest.mark.parametrize("skip", [True, False])
@pytest.mark.parametrize("moved", [False, True])
@pytest.mark.parametrize("table", fc.TABLES)
@pytest.mark.parametrize("split", fc.SPLITS)
def test_fused_frame_has_the_loops_bits(hip, split, table, moved, skip, where):
    want = fc.reference(split, table, moved, where)[0]
    loop = tracer(split, table, moved, where, skip, fused=False).frame().framebuffer(False)
    tr = tracer(split, table, moved, where, skip).frame()
    got = tr.framebuffer(False)
    st = tr.stats()
    assert st["fused"] == 1 and st["adapter_calls"] == 1
    assert got.any()
    assert (bits(got) == bits(loop)).all()
    assert (bits(got) == bits(want)).all()


def test_the_cut_does_not_show(hip):
    frames = [tracer(s, "cool", True, "inside").frame().framebuffer(False).copy() for s in fc.SPLITS]
    for f in frames[1:]:
        assert (bits(f) == bits(frames[0])).all()


@pytest.mark.parametrize("split,table", [((1, 1, 1), "cool"), ((2, 2, 2), "spikes"), ((3, 1, 2), "opaque"), ((4, 4, 4), "cool")])
def test_counters(hip, split, table):
    _, rounds, entering = fc.reference(split, table, True, "outside")
    loop = tracer(split, table, True, fused=False).frame()
    tr = tracer(split, table, True).frame()
    ls, fs = loop.stats(), tr.stats()
    assert "fused" not in ls and ls["adapter_calls"] == len(rounds)
    assert fs["samples_marched"] == ls["samples_marched"] > 0
    assert fs["samples_gathered"] == ls["samples_gathered"] > 0
    if table == "spikes":
        assert fs["samples_gathered"] < fs["samples_marched"]  # macro cells were skipped
    assert fs["brick_visits"] == sum(n for _, n in rounds)
    assert fs["rays_deposited"] == entering
    assert all(len(q) == 0 for q in tr.queues)
    assert sum(a.info()["samples_marched"] for a in tr.adapters) == 0  # the bricks' own counters are not touched


@pytest.mark.parametrize("ty", ["u8", "i16"])
def test_typed_voxels(hip, ty):
    vol, t = quantised(fc.volume(), ty), scaled("cool", ty)
    loop = tracer((2, 2, 2), vol=vol, native=True, t=t, fused=False).frame().framebuffer(False).copy()
    tr = tracer((2, 2, 2), vol=vol, native=True, t=t).frame()
    assert tr.adapters[0].dtype_name != "float32" and tr.stats()["fused"] == 1
    got = tr.framebuffer(False)
    flt = tracer((2, 2, 2), vol=as_float(vol), t=t).frame()
    assert flt.stats()["fused"] == 1
    assert got.any()
    assert (bits(got) == bits(loop)).all()
    assert (bits(got) == bits(flt.framebuffer(False))).all()


@pytest.mark.parametrize("split", [(2, 2, 2), (4, 4, 4)])
def test_clipped_fused_frame(hip, split):
    want, plane = fc.clip_reference(split, "cool", False)
    depth = DepthPlane(fc.FILM[0], fc.FILM[1]).upload(plane)
    loop = tracer(split, fused=False).frame(depth).framebuffer(False).copy()
    tr = tracer(split).frame(depth)
    got = tr.framebuffer(False)
    assert tr.stats()["fused"] == 1
    assert (bits(got) == bits(loop)).all()
    assert (bits(got) == bits(want)).all()
    plain = fc.reference(split, "cool", False, "outside")[0]
    assert (got[..., 3] < plain[..., 3]).sum() > 200  # the clip shows


def test_mixed_frame(hip):
    cam = scenes.Camera((0.0, 0.1, 0.3), (0.0, 0.1, -0.3), (0.0, 1.0, 0.0), float(F(45.0 * np.pi / 180.0)), 150, 110)
    scene = scenes.bunny_scene(150, 110)
    parts = scenes.split_volume(scenes.mesh_in_volume(scene, scenes.sphere_volume(64), fill=0.6), 2, 2, 2)
    want = MixedTracer(scene, parts, cam, tf("ramp"), sampling_rate=1.0).frame().framebuffer(False).copy()
    mt = MixedTracer(scene, parts, cam, tf("ramp"), sampling_rate=1.0, fused=True).frame()
    assert mt.volume.stats()["fused"] == 1 and mt.volume.calls == 1
    assert np.isfinite(mt.depth.download()).sum() > 1000  # the bunny is in the picture
    assert (bits(mt.framebuffer(False)) == bits(want)).all()


def test_rays_that_find_no_brick(hip):
    tr = tracer((2, 2, 2), where="away").frame()
    st = tr.stats()
    assert st["fused"] == 1 and st["rays_deposited"] == 0 and st["brick_visits"] == 0 and st["samples_marched"] == 0
    assert (bits(tr.framebuffer(False)) == 0).all()  # all +0


def _amr_on(tr):
    b = fc.bricks_of(fc.volume(), (2, 2, 2))[0]
    scenes.refine(b, np.asarray(b.offset) + 1, (2, 2, 2), 2, seed=5)
    tr.adapters[0].set_subgrids(b.subgrids)


def _type_on(tr):
    """brick 3 replaced by the same samples at another width (uint16 beside uint8)"""
    b = fc.bricks_of(quantised(fc.volume(), "u8"), (2, 2, 2))[3]
    b.data = b.data.astype(np.uint16)
    other = HipVolumeAdapter(b, fc.RATE, True, True)
    other.set_transfer(scaled("cool", "u8"))
    tr._kept, tr.adapters[3] = tr.adapters[3], other


def _type_off(tr):
    tr.adapters[3] = tr._kept


CAUSES = {
    "surfaces": (lambda tr: tr.set_surfaces([0.5], [], 0.6), lambda tr: tr.set_surfaces()),
    "lit": (lambda tr: tr.set_lights([((3.0, 4.0, 5.0), (1.0, 0.9, 0.8))]).set_shading(True), lambda tr: tr.set_shading(False)),
    "amr": (_amr_on, lambda tr: tr.adapters[0].set_subgrids([])),
    "table": (lambda tr: tr.adapters[1].set_transfer(tf("ramp")), lambda tr: tr.adapters[1].set_transfer(tf("cool"))),
    "voxel type": (_type_on, _type_off),
}


@pytest.mark.parametrize("cause", sorted(CAUSES))
def test_fallbacks(hip, cause):
    typed = cause == "voxel type"
    vol, t = (quantised(fc.volume(), "u8"), scaled("cool", "u8")) if typed else (fc.volume(), tf("cool"))
    tr = tracer((2, 2, 2), vol=vol, native=typed, t=t).frame()
    assert tr.stats()["fused"] == 1
    plain = tr.framebuffer(False).copy()
    on, off = CAUSES[cause]
    on(tr)
    tr.fused = False
    loop = tr.frame().framebuffer(False).copy()
    loop_calls = tr.calls
    tr.fused = True
    got = tr.frame().framebuffer(False).copy()  # nothing is refused
    st = tr.stats()
    assert st["fused"] == 0 and st["adapter_calls"] == loop_calls > 1 and st["brick_visits"] == 0  # the loop ran: a march per round
    assert got.any() and (bits(got) == bits(loop)).all()
    if cause in ("surfaces", "lit", "table"):
        assert (bits(got) != bits(plain)).any()  # the cause shows in the picture
    off(tr)
    assert tr.frame().stats()["fused"] == 1
    assert (bits(tr.framebuffer(False)) == bits(plain)).all()


def test_time_step(hip):
    tr = tracer((2, 2, 2)).frame()
    first = tr.framebuffer(False).copy()
    new = fc.volume(seed=11)
    tr.update(fc.bricks_of(new, (2, 2, 2))).frame()
    assert tr.stats()["fused"] == 1
    got = tr.framebuffer(False).copy()
    fresh = tracer((2, 2, 2), vol=new).frame().framebuffer(False)
    assert (bits(got) == bits(fresh)).all()
    assert (bits(got) == bits(fc.reference((2, 2, 2), "cool", False, "outside", 11)[0])).all()
    assert (bits(got) != bits(first)).any()


def test_argument_errors_change_nothing(hip):
    lib = capi.load()
    INVALID = -1
    tr = tracer((2, 2, 2)).frame()
    before = tr.framebuffer(False).copy()
    cam = tr.camera
    pod = capi.CameraPod((C.c_float * 3)(*cam.eye), (C.c_float * 3)(*cam.focus), (C.c_float * 3)(*cam.up), cam.fov, cam.width, cam.height, 1, 1, 0.0)
    m = np.ascontiguousarray(np.tile(tr.m, tr.n_inst), F)
    minv = np.ascontiguousarray(np.tile(tr.minv, tr.n_inst), F)
    st = capi.VolumeFusedStats()
    vols, qs, n = tr._arr(tr.adapters), tr._arr(tr.queues), C.c_size_t(tr.n_inst)
    call = lib.gvt_hip_volume_frame_fused
    assert call(None, vols, capi.ptr(m), capi.ptr(minv), n, C.byref(pod), qs, tr.fb.h, None, C.byref(st)) == INVALID
    assert call(tr.top.h, None, capi.ptr(m), capi.ptr(minv), n, C.byref(pod), qs, tr.fb.h, None, C.byref(st)) == INVALID
    assert call(tr.top.h, vols, None, capi.ptr(minv), n, C.byref(pod), qs, tr.fb.h, None, C.byref(st)) == INVALID
    assert call(tr.top.h, vols, capi.ptr(m), None, n, C.byref(pod), qs, tr.fb.h, None, C.byref(st)) == INVALID
    assert call(tr.top.h, vols, capi.ptr(m), capi.ptr(minv), n, None, qs, tr.fb.h, None, C.byref(st)) == INVALID
    assert call(tr.top.h, vols, capi.ptr(m), capi.ptr(minv), n, C.byref(pod), None, tr.fb.h, None, C.byref(st)) == INVALID
    assert call(tr.top.h, vols, capi.ptr(m), capi.ptr(minv), n, C.byref(pod), qs, None, None, C.byref(st)) == INVALID
    assert call(tr.top.h, vols, capi.ptr(m), capi.ptr(minv), C.c_size_t(tr.n_inst - 1), C.byref(pod), qs, tr.fb.h, None, C.byref(st)) == INVALID  # not the top's count
    bare = HipVolumeAdapter(fc.bricks_of(fc.volume(), (2, 2, 2))[0], fc.RATE)  # a brick without a transfer function
    mixed = (C.c_void_p * tr.n_inst)(*([bare.h] + [a.h for a in tr.adapters[1:]]))
    assert call(tr.top.h, mixed, capi.ptr(m), capi.ptr(minv), n, C.byref(pod), qs, tr.fb.h, None, C.byref(st)) == INVALID
    wrong = DepthPlane(cam.width + 8, cam.height)
    assert call(tr.top.h, vols, capi.ptr(m), capi.ptr(minv), n, C.byref(pod), qs, tr.fb.h, wrong.h, C.byref(st)) == INVALID
    two = capi.CameraPod((C.c_float * 3)(*cam.eye), (C.c_float * 3)(*cam.focus), (C.c_float * 3)(*cam.up), cam.fov, cam.width, cam.height, 2, 1, 0.0)
    assert call(tr.top.h, vols, capi.ptr(m), capi.ptr(minv), n, C.byref(two), qs, tr.fb.h, DepthPlane(cam.width, cam.height).h, C.byref(st)) == INVALID
    assert (bits(tr.framebuffer(False)) == bits(before)).all()
    assert call(tr.top.h, vols, capi.ptr(m), capi.ptr(minv), n, C.byref(pod), qs, tr.fb.h, None, None) == 0  # stats may be NULL
    assert (bits(tr.framebuffer(False)) == bits(before)).all()
