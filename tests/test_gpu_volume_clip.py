"""Geometry inside a volume on the device (csrc/volume.hip, csrc/depth.hip) against the numpy checker (tests/volume_clip_checker.py) and the
oracle, bit for bit: the march clipped at a ray's t_max, skipping under the clip, the split-march property of the plain and the surface
march, the clipped frame over several brickings, the depth plane of a scene, the mixed frame, the composite and the refusals."""
import ctypes as C

import numpy as np
import pytest

from gravit_amd import capi, scenes
from gravit_amd.adapter import DepthPlane, FrameBuffer, HipVolumeAdapter
from gravit_amd.scheduler import MixedTracer, NativeTracer, VolumeTracer
from oracle import orc
from tests import volume_checker as vc
from tests import volume_clip_checker as cc
from tests import volume_surface_checker as sc
from tests.test_gpu_volume import IDENT, MOVED, grid, make_rays, tf
from tests.test_gpu_volume_types import quantised, scaled
from tests.test_volume_clip_host import clip_frame_case

pytestmark = pytest.mark.gpu

F = np.float32
PLAIN = ("color", "w", "t_min", "depth")
ALL = ("color", "w", "t_min", "depth", "t")
FLT_MAX = np.finfo(F).max


def same_bits(a, b, fields=PLAIN):
    for f in fields:
        x, y = np.ascontiguousarray(a[f]).view(np.uint32), np.ascontiguousarray(b[f]).view(np.uint32)
        assert (x == y).all(), "%s: %d of %d rays differ" % (f, (x != y).reshape(len(a), -1).any(axis=1).sum(), len(a))


def mixed_clips(rays, dt, reach, seed=5):
    """Flag the rays (all but every 7th) and give them a mix of t_max: random inside the brick's reach, exact lattice values, 0, negative,
    +Inf, NaN."""
    rng = np.random.default_rng(seed)
    n = len(rays)
    r = rays.copy()
    kind = np.arange(n) % 6
    t = (rng.random(n) * reach).astype(F)
    lattice = (rng.integers(0, int(reach / dt), n).astype(F) * dt).astype(F)
    t = np.where(kind == 1, lattice, t)
    t = np.where(kind == 2, F(0), t)
    t = np.where(kind == 3, -t, t)
    t = np.where(kind == 4, F(np.inf), t)
    t = np.where(kind == 5, F(np.nan), t)
    r["t_max"] = t.astype(F)
    r["depth"] |= np.where(np.arange(n) % 7 != 0, cc.CLIP, 0).astype(np.int32)
    return r


@pytest.mark.parametrize("kind", ["cool", "spikes", "ramp"])
@pytest.mark.parametrize("moved", [False, True])
def test_clipped_march_equals_the_checker(hip, kind, moved):
    vol = grid()
    m = MOVED if moved else IDENT
    minv = scenes.instance_matrices(m)[0]
    t = tf(kind)
    ad = HipVolumeAdapter(vol, sampling_rate=1.7)
    ad.set_transfer(t)
    B = vc.Brick(vol, t, 1.7)
    rays = mixed_clips(make_rays(vol, m), B.dt, 4.0)
    got = ad.trace(rays, m, minv)
    want = cc.march(B, rays, minv)
    same_bits(got, want)
    plain = vc.march(B, rays, minv)
    assert (got["t_min"] < plain["t_min"]).sum() > 100  # the clip shows (in w too, but the sparse table leaves most rays of this small grid transparent)
    assert (got["t_max"].view(np.uint32) == rays["t_max"].view(np.uint32)).all()


def test_skipping_gives_the_same_bits_under_the_clip(hip):
    vol = grid(40)
    t = tf("spikes")
    a, b = HipVolumeAdapter(vol, 1.0, skip=True), HipVolumeAdapter(vol, 1.0, skip=False)
    a.set_transfer(t)
    b.set_transfer(t)
    B = vc.Brick(vol, t, 1.0)
    rays = mixed_clips(make_rays(vol, IDENT, n=4000, seed=11), B.dt, 3.0)
    rays["t"] = 77.0
    ra, rb = a.trace(rays, IDENT, IDENT), b.trace(rays, IDENT, IDENT)
    same_bits(ra, rb, ALL)
    same_bits(ra, cc.march(B, rays, IDENT), ALL)
    ia, ib = a.info(), b.info()
    assert ia["samples_marched"] == ib["samples_marched"] > 0
    assert ia["samples_gathered"] < ib["samples_gathered"] == ib["samples_marched"]


@pytest.mark.parametrize("voxels", ["f32", "u8"])
@pytest.mark.parametrize("surfaces", [False, True])
def test_a_march_split_at_the_clip_equals_one_march(hip, surfaces, voxels):
    """No checker involved: march clipped at t_c, clear CLIP and BOUNDARY, march the same brick again = one unclipped march."""
    vol = grid()
    t = tf("ramp")
    iso = [0.42, 0.58]
    if voxels == "u8":
        vol, t, iso = quantised(vol, "u8"), scaled("ramp", "u8"), [0.42 * 255, 0.58 * 255]
    ad = HipVolumeAdapter(vol, sampling_rate=1.7, native=voxels == "u8")
    ad.set_transfer(t)
    if surfaces:
        S = sc.Surfaces(iso, [[0.5, 0.7, -0.4, 0.3]], 0.5, [((3.0, 4.0, 5.0), (1.0, 0.9, 0.8))], ka=0.4, kd=0.6)
        ad.set_surfaces(S.iso, S.planes, float(S.opacity))
        ad.set_lights(list(zip(S.lpos, S.lcol)), float(S.ka), float(S.kd))
    rays = make_rays(vol, IDENT, n=2000)
    rays["t"] = 55.0
    whole = ad.trace(rays, IDENT, IDENT)
    rng = np.random.default_rng(9)
    first = rays.copy()
    first["depth"] |= cc.CLIP
    first["t_max"] = np.where(np.arange(len(rays)) % 2 == 0, whole["t_min"] * rng.random(len(rays)).astype(F), (rng.random(len(rays)) * 3).astype(F)).astype(F)
    part = ad.trace(first, IDENT, IDENT)
    assert (part["depth"] & cc.CLIP).all()
    opaque = (part["depth"] & vc.OPAQUE) != 0
    part["depth"] &= ~cc.CLIP
    same_bits(part[opaque], whole[opaque], ALL)
    rest = part[~opaque].copy()
    rest["depth"] &= ~vc.BOUNDARY
    rest["t_max"] = FLT_MAX
    again = ad.trace(rest, IDENT, IDENT)
    same_bits(again, whole[~opaque], ALL)
    assert (part["w"][~opaque] < whole["w"][~opaque]).sum() > 100  # the first part stopped short
    if surfaces:
        assert ad.crossings() > 100 and (whole["depth"] & sc.SIDES).any()


def test_t_max_without_the_flag_means_nothing(hip):
    vol = grid()
    for surfaces in (False, True):
        ad = HipVolumeAdapter(vol, sampling_rate=1.7)
        ad.set_transfer(tf("cool"))
        if surfaces:
            ad.set_surfaces([0.42], [[0.0, 0.0, 1.0, 0.05]], 0.5)
        rays = make_rays(vol, MOVED)
        minv = scenes.instance_matrices(MOVED)[0]
        want = ad.trace(rays, MOVED, minv)
        r = rays.copy()
        r["t_max"] = np.random.default_rng(1).random(len(r)).astype(F) * 2 - 0.5
        r["t_max"][::5] = np.nan
        same_bits(ad.trace(r, MOVED, minv), want, ALL)


@pytest.fixture(scope="module")
def clip_frame(hip):
    vol, cam, plane = clip_frame_case()
    t = tf("cool")
    B = vc.Brick(vol, t, 1.0)
    want, calls = cc.frame([B], B.lo[None], B.hi[None], IDENT, cam, plane)
    return vol, cam, plane, t, want


@pytest.mark.parametrize("split", [(1, 1, 1), (2, 2, 2), (1, 1, 8)])
def test_clipped_frame_equals_the_checker(clip_frame, split):
    vol, cam, plane, t, want = clip_frame
    parts = vol if split == (1, 1, 1) else scenes.split_volume(vol, *split)
    depth = DepthPlane(cam.width, cam.height).upload(plane)
    assert (depth.download().view(np.uint32) == plane.view(np.uint32)).all()
    tr = VolumeTracer(parts, cam, t, sampling_rate=1.0).frame(depth)
    got = tr.framebuffer(False)
    assert tr.calls >= int(np.prod(split))
    assert (got.view(np.uint32) == want.view(np.uint32)).all()
    plain = tr.frame().framebuffer(False)
    assert (got[..., 3] < plain[..., 3]).sum() > 300


def test_null_depth_is_the_plain_frame(clip_frame):
    vol, cam, plane, t, want = clip_frame
    tr = VolumeTracer(scenes.split_volume(vol, 2, 2, 2), cam, t, sampling_rate=1.0)
    plain = tr.frame().framebuffer(False).copy()
    pod = capi.CameraPod((C.c_float * 3)(*cam.eye), (C.c_float * 3)(*cam.focus), (C.c_float * 3)(*cam.up), cam.fov, cam.width, cam.height, 1, cam.depth, cam.jitter)
    m = np.ascontiguousarray(np.tile(tr.m, tr.n_inst), F)
    minv = np.ascontiguousarray(np.tile(tr.minv, tr.n_inst), F)
    calls = C.c_uint64(0)
    capi.check(capi.load().gvt_hip_volume_frame_clipped(tr.top.h, tr._arr(tr.adapters), capi.ptr(m), capi.ptr(minv), tr.n_inst, C.byref(pod), tr._arr(tr.queues),
                                                        tr.fb.h, None, C.byref(calls)), "gvt_hip_volume_frame_clipped")
    assert calls.value == tr.calls
    assert (tr.framebuffer(False).view(np.uint32) == plain.view(np.uint32)).all()
    inf = DepthPlane(cam.width, cam.height)  # a plane of +Inf clips nothing either
    assert np.isinf(inf.download()).all()
    assert (tr.frame(inf).framebuffer(False).view(np.uint32) == plain.view(np.uint32)).all()


def oracle_depth(scene, cam):
    """min over the instances of orc.intersect's t on the camera's rays taken into each instance with vc.xfm_point / vc.xfm_vector."""
    rays = vc.camera_rays(cam)
    meshes = [orc.Mesh(m.verts, m.tris, mesh_mat=m.material) for m in scene.meshes]
    best = np.full(len(rays), np.inf, F)
    for i in range(scene.n_inst):
        o, d = vc.xfm_point(scene.minv[i], rays["origin"]), vc.xfm_vector(scene.minv[i], rays["direction"])
        h = meshes[scene.inst_mesh[i]].intersect(o, d)
        best = np.minimum(best, np.where(h["prim"] >= 0, h["t"], F(np.inf)).astype(F))
    out = np.full(cam.width * cam.height, np.inf, F)
    out[rays["id"].astype(np.int64)] = best
    return out.reshape(cam.height, cam.width)


@pytest.mark.parametrize("name", ["simple", "bunny"])
def test_depth_render_equals_the_oracle(hip, name):
    scene = scenes.simple_scene(128, 128) if name == "simple" else scenes.bunny_scene(128, 128)
    assert scene.n_inst == (25 if name == "simple" else 1)
    depth = DepthPlane(128, 128).upload(np.full((128, 128), 3.0, F))  # (render starts from +Inf, not from what the plane held)
    got = depth.render(scene).download()
    want = oracle_depth(scene, scene.camera)
    hit = np.isfinite(want)
    assert 1000 < hit.sum() < 128 * 128 - 1000
    assert (got.view(np.uint32) == want.view(np.uint32)).all()
    assert np.isposinf(got[~hit]).all()


@pytest.fixture(scope="module")
def mixed_case(hip):
    cam = scenes.Camera((0.0, 0.1, 0.3), (0.0, 0.1, -0.3), (0.0, 1.0, 0.0), float(F(45.0 * np.pi / 180.0)), 150, 110)
    scene = scenes.bunny_scene(150, 110)
    vol = scenes.mesh_in_volume(scene, scenes.sphere_volume(64), fill=0.6)
    t = tf("ramp")
    mt = MixedTracer(scene, vol, cam, t, sampling_rate=1.0).frame()
    return scene, cam, vol, t, mt.framebuffer(False).copy(), mt.depth.download().copy()


def test_mixed_frame_equals_the_composite_of_its_parts(mixed_case):
    scene, cam, vol, t, got, depth = mixed_case
    assert (depth.view(np.uint32) == oracle_depth(scene, cam).view(np.uint32)).all()
    mesh = NativeTracer(scene)().framebuffer(False)  # the mesh frame alone
    B = vc.Brick(vol, t, 1.0)
    fog, _ = cc.frame([B], B.lo[None], B.hi[None], IDENT, cam, depth)
    want = cc.composite(fog, mesh, depth)
    assert (got.view(np.uint32) == want.view(np.uint32)).all()
    wall = np.isfinite(depth)
    assert wall.sum() > 1000 and (np.abs(got[wall][:, 3] - 1) < 1e-6).all()  # geometry is opaque, shadowed or not: a + fl(1 - a), within an ulp of 1
    assert ((fog[..., 3] > 0) & wall).sum() > 500 and ((fog[..., 3] > 0) & ~wall).sum() > 500  # fog in front of the bunny and beside it
    unclipped, _ = vc.frame([B], B.lo[None], B.hi[None], IDENT, cam)
    assert (fog[wall][:, 3] < unclipped[wall][:, 3]).sum() > 500  # the bunny hides the fog behind it


def test_mixed_frame_is_independent_of_the_bricking(mixed_case):
    scene, cam, vol, t, got, depth = mixed_case
    mt = MixedTracer(scene, scenes.split_volume(vol, 2, 2, 2), cam, t, sampling_rate=1.0).frame()
    assert mt.volume.calls >= 8
    assert (mt.framebuffer(False).view(np.uint32) == got.view(np.uint32)).all()
    assert (mt.mesh_framebuffer(False).view(np.uint32) == NativeTracer(scene)().framebuffer(False).view(np.uint32)).all()  # the mesh frame is untouched


def _upload_fb(fb, img):
    """Put an image into a framebuffer (the library has no host path into one: a plain copy through the runtime it is linked against)."""
    src = capi.f32(img)
    capi.synchronize()
    rt = C.CDLL("libamdhip64.so")
    rt.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert src.nbytes == fb.w * fb.hgt * 16
    assert rt.hipMemcpy(fb.device_ptr(), capi.ptr(src), src.nbytes, 1) == 0  # hipMemcpyHostToDevice


def test_composite_alone(hip):
    rng = np.random.default_rng(4)
    h, w = 37, 53
    front = rng.random((h, w, 4)).astype(F)
    front[..., :3] *= front[..., 3:4]
    front[rng.random((h, w)) < 0.2] = 0  # pixels without volume
    back = (rng.random((h, w, 4)) * 1.4).astype(F)  # (un-clamped sums above 1)
    back[rng.random((h, w)) < 0.2, :3] = 0  # shadowed surface pixels
    depth = np.where(rng.random((h, w)) < 0.4, F(np.inf), rng.random((h, w)).astype(F) * 5).astype(F)
    for d in (depth, None):
        f, b = FrameBuffer(w, h), FrameBuffer(w, h)
        _upload_fb(f, front)
        _upload_fb(b, back)
        plane = None if d is None else DepthPlane(w, h).upload(d)
        got = f.composite_over(b, plane).download(False)
        want = cc.composite(front, back, d)
        assert (got.view(np.uint32) == want.view(np.uint32)).all()
        assert (b.download(False).view(np.uint32) == back.view(np.uint32)).all()
        none = (front == 0).all(axis=2)
        assert (got[none][:, :3].view(np.uint32) == np.minimum(back[none][:, :3], 1).view(np.uint32)).all()


def test_refusals_change_nothing(hip, clip_frame):
    vol, cam, plane, t, want = clip_frame
    lib = capi.load()
    INVALID = -1
    scene = scenes.bunny_scene(cam.width, cam.height)
    mark = np.full((cam.height, cam.width), 2.5, F)
    depth = DepthPlane(cam.width, cam.height).upload(mark)
    two = scenes.Camera(cam.eye, cam.focus, cam.up, cam.fov, cam.width, cam.height, samples=2)
    other = scenes.Camera(cam.eye, cam.focus, cam.up, cam.fov, cam.width + 8, cam.height)
    for bad in (two, other):
        with pytest.raises(capi.GvtHipError, match=r"\(-1\)"):
            depth.render(scene, bad)
        assert (depth.download() == mark).all()
    assert lib.gvt_hip_depth_render(None, None, None, None, 0, None) == INVALID
    pod = capi.CameraPod((C.c_float * 3)(*cam.eye), (C.c_float * 3)(*cam.focus), (C.c_float * 3)(*cam.up), cam.fov, cam.width, cam.height, 1, 1, 0.0)
    assert lib.gvt_hip_depth_render(depth.h, None, None, None, 1, C.byref(pod)) == INVALID
    assert lib.gvt_hip_depth_render(depth.h, None, None, None, 0, None) == INVALID
    assert (depth.download() == mark).all()
    assert lib.gvt_hip_depth_upload(depth.h, None, 0) == INVALID and lib.gvt_hip_depth_upload(depth.h, capi.ptr(mark), 2) == INVALID
    assert lib.gvt_hip_depth_download(depth.h, None) == INVALID and lib.gvt_hip_depth_clear(None) == INVALID
    assert not lib.gvt_hip_depth_create(0, 4)
    # the clipped frame
    tr = VolumeTracer(vol, cam, t, sampling_rate=1.0).frame(depth.upload(plane))
    before = tr.framebuffer(False).copy()
    assert (before.view(np.uint32) == want.view(np.uint32)).all()
    tr.camera = two
    with pytest.raises(capi.GvtHipError, match=r"\(-1\)"):
        tr.frame(depth)
    tr.camera = cam
    with pytest.raises(capi.GvtHipError, match=r"\(-1\)"):
        tr.frame(DepthPlane(cam.width + 8, cam.height))
    m, minv = capi.f32(tr.m), capi.f32(tr.minv)
    assert lib.gvt_hip_volume_frame_clipped(tr.top.h, tr._arr(tr.adapters), capi.ptr(m), capi.ptr(minv), 1, None, tr._arr(tr.queues), tr.fb.h, depth.h, None) == INVALID
    assert lib.gvt_hip_volume_frame_clipped(tr.top.h, tr._arr(tr.adapters), capi.ptr(m), capi.ptr(minv), 1, C.byref(pod), tr._arr(tr.queues), None, depth.h, None) == INVALID
    assert (tr.framebuffer(False).view(np.uint32) == before.view(np.uint32)).all()
    # the composite
    small = FrameBuffer(cam.width + 8, cam.height)
    assert lib.gvt_hip_fb_composite_over(None, tr.fb.h, None) == INVALID and lib.gvt_hip_fb_composite_over(tr.fb.h, None, depth.h) == INVALID
    assert lib.gvt_hip_fb_composite_over(tr.fb.h, small.h, None) == INVALID
    assert lib.gvt_hip_fb_composite_over(tr.fb.h, tr.fb.h, None) == INVALID
    back = FrameBuffer(cam.width, cam.height)
    assert lib.gvt_hip_fb_composite_over(tr.fb.h, back.h, DepthPlane(cam.width + 8, cam.height).h) == INVALID
    assert (tr.framebuffer(False).view(np.uint32) == before.view(np.uint32)).all()
