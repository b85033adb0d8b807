"""Volumes under instance matrices with rotation, shear and mirroring on the device (tests/volume_affine_cases.py): one brick through
gvt_hip_volume_trace -- plain, surfaces, lit, surfaces + lit, central gradients, AMR, the clip; every voxel type -- against the numpy
checkers bit for bit; the matrix convention against a march under the identity with the rays taken through minv on the host; the
rigid-motion claim of lit volumes; and bricked frames: exact under a signed axis permutation, refused under a rotation or a shear."""
import numpy as np
import pytest
import torch

from gravit_amd import capi, scenes
from gravit_amd.adapter import HipVolumeAdapter
from gravit_amd.layouts import RAY_DTYPE, default_material, point_light
from gravit_amd.scheduler import HipVolumeBackend, MixedTracer, VolumeDomainTracer, VolumeTracer
from tests import affine_cases as ac
from tests import volume_affine_cases as va
from tests import volume_domain_backend as vdb
from tests import volume_fused_cases as fc
from tests.volume_common import tf
from tests.test_gpu_volume_domains import Locked, LOCK

pytestmark = pytest.mark.gpu

F = np.float32
ALL = ("color", "w", "t_min", "depth", "t")
PLAIN = ("color", "w", "t_min", "depth")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b, fields):
    for f in fields:
        x, y = bits(a[f]), bits(b[f])
        assert (x == y).all(), "%s: %d of %d rays differ" % (f, (x != y).reshape(len(a), -1).any(axis=1).sum(), len(a))


def adapter(variant, ty="f32"):
    """The one-brick volume of a variant as the checker's reference has it: table, surfaces, lights, shading, gradient kind, subgrids."""
    vol, t, vr = va.typed(ty, variant == "amr")
    ad = HipVolumeAdapter(vol, sampling_rate=va.RATE, native=ty != "f32")
    ad.set_transfer(t)
    S, shading = va.surfaces(variant, value_range=vr)
    if S is not None:
        if len(S):
            ad.set_surfaces(S.iso, S.planes, float(S.opacity))
        ad.set_lights(list(zip(S.lpos, S.lcol)), float(S.ka), float(S.kd))
        ad.set_shading(shading)
    if variant == "central":
        ad.set_gradient("central")
    return ad


def fields_of(variant):
    return ALL if variant in ("surfaces", "surf_lit", "central") else PLAIN


@pytest.mark.parametrize("variant", va.VARIANTS)
@pytest.mark.parametrize("family", ac.FAMILIES)
def test_one_brick_march_equals_the_checker(hip, family, variant):
    """gvt_hip_volume_trace of the camera's 64 x 48 list through one 25^3 brick under a matrix of every family: vol_ray_range's object-space
    ray, the lights' directions through minv (lights_dev / surf_dev / light_dev), the planes, the clip -- the checker's bits."""
    rays, want = va.reference(family, variant)
    m = va.matrix(family)
    ad = adapter(variant)
    got = ad.trace(rays, m, scenes.instance_matrices(m)[0])
    same_bits(got, want, fields_of(variant))
    assert (got["w"] > 0).sum() > 150  # the volume is in the picture
    if variant in ("lit", "surf_lit", "central"):
        assert ad.shaded() > 1000
    if variant in ("surfaces", "surf_lit", "central"):
        assert ad.crossings() > 100
    if variant == "central":
        assert ad.central_marches() == 1
    if variant == "amr":
        assert ad.amr_info()["samples_refined"] > 500  # samples were taken from the subgrids
    if variant == "clip":
        assert (bits(got["w"]) != bits(va.reference(family, "plain")[1]["w"])).sum() > 100  # the clip shows


@pytest.mark.parametrize("variant", ["plain", "surfaces", "lit", "surf_lit", "central", "clip"])
@pytest.mark.parametrize("ty", ["u8", "i16", "u16"])
@pytest.mark.parametrize("family", ac.FAMILIES)
def test_typed_one_brick_march_equals_the_checker(hip, family, ty, variant):
    """The same through 8- and 16-bit voxels kept at their own width (the checker marches the samples as floats).  Every variant but AMR:
    gvt_hip_volume_set_subgrids refuses a volume of another voxel type than float32 (tests/test_gpu_volume_amr.py)."""
    rays, want = va.reference(family, variant, ty)
    m = va.matrix(family)
    ad = adapter(variant, ty)
    assert ad.dtype_name != "float32"
    got = ad.trace(rays, m, scenes.instance_matrices(m)[0])
    same_bits(got, want, fields_of(variant))
    assert (got["w"] > 0).sum() > 150


@pytest.mark.parametrize("variant", ["plain", "surf_lit"])
@pytest.mark.parametrize("family", ["rot", "shear", "mirror"])
def test_the_matrix_convention_against_a_march_under_the_identity(hip, family, variant):
    """A check that does not share the device's (or the checkers') reading of minv's storage: the camera list taken into the volume's own
    space on the HOST -- float32, column-major, in glm's recorded order (m0 x + m1 y) + (m2 z + m3 w) written out here -- and marched under
    the identity gives the bits of the march under m.  (The lights of the lit variant go through the same product.)"""
    rays, _ = va.reference(family, variant)
    m = va.matrix(family)
    minv = scenes.instance_matrices(m)[0]
    col = minv.reshape(4, 4)  # col[c][r]
    o, d = rays["origin"], rays["direction"]
    own = rays.copy()
    own["origin"] = np.stack([(col[0][r] * o[:, 0] + col[1][r] * o[:, 1]) + (col[2][r] * o[:, 2] + col[3][r] * F(1)) for r in range(3)], axis=1)
    own["direction"] = np.stack([(col[0][r] * d[:, 0] + col[1][r] * d[:, 1]) + (col[2][r] * d[:, 2] + col[3][r] * F(0)) for r in range(3)], axis=1)
    ident = va.matrix("ident")
    ad = adapter(variant)
    got = ad.trace(rays, m, minv)
    if variant == "surf_lit":  # the lights' directions: -position through minv as a vector, the same product; the identity case gets them as positions
        S, _ = va.surfaces(variant)
        l = -S.lpos
        moved = -np.stack([(col[0][r] * l[:, 0] + col[1][r] * l[:, 1]) + (col[2][r] * l[:, 2] + col[3][r] * F(0)) for r in range(3)], axis=1).astype(F)
        other = adapter(variant)
        other.set_lights(list(zip(moved, S.lcol)), float(S.ka), float(S.kd))
    else:
        other = adapter(variant)
    same_bits(other.trace(own, ident, ident), got, fields_of(variant))
    assert (got["w"] > 0).sum() > 150


RIGID_MEASURED = va.RIGID_MEASURED


def lit_tracer(name):
    m, cam, lights = (va.matrix("ident"), va.camera(va.matrix("ident")), va.LIGHTS) if name == "ident" else va.rotated_with_the_world(name)
    return VolumeTracer(va.volume(), cam, tf("ramp"), m=m, sampling_rate=va.RATE).set_lights(lights).set_shading()


def test_lit_fog_turned_with_its_lights_and_camera_is_the_same_picture(hip):
    """The rigid-motion claim (gvt_hip.h: object-space shading "equals world-space shading for rigid motions and uniform scales"): lit fog
    under a rotation, with the lights and the camera turned by the same R, is the unrotated frame up to rounding.  The numpy checker's own
    difference between the two formulations, measured on the CPU: largest per-channel difference 1.62e-6 (rot) and 2.15e-6 (rot@1), no
    pixel above 1e-5.  Asserted on the device: four times the larger, 8.6e-6; the pixels that may exceed it: the checker's share (0) plus
    1 % of the film, 30 pixels (a sample falling in or out at a silhouette is legitimate).  Under a shear the same construction gives
    another picture -- the documented limit."""
    base = lit_tracer("ident").frame().framebuffer(False).copy()
    assert (bits(base) == bits(va.lit_frame_reference("ident"))).all() and (base[..., 3] > 0).sum() > 500
    for name in ("rot", "rot@1"):
        tr = lit_tracer(name).frame()
        fb = tr.framebuffer(False)
        assert tr.stats()["samples_shaded"] > 10000
        assert (bits(fb) == bits(va.lit_frame_reference(name))).all()  # the device is the checker, bit for bit, under the rotation too
        d = np.abs(fb.astype(np.float64) - base).max(axis=2)
        print(name, "largest difference %.3g, pixels above the bound %d" % (d.max(), (d > 4 * RIGID_MEASURED).sum()))
        assert (d > 4 * RIGID_MEASURED).sum() <= int(0.01 * d.size)
    sheared = lit_tracer("shear").frame().framebuffer(False)
    d = np.abs(sheared.astype(np.float64) - base).max(axis=2)
    assert (d > 4 * RIGID_MEASURED).sum() > int(0.01 * d.size)


# ------------------------------------------------------------------ bricked frames
@pytest.mark.parametrize("family", ac.FAMILIES)
def test_one_brick_frames_work_under_every_family(hip, family):
    """A single brick is marched under any affine matrix, through the loop and through the fused frame: the checker's frame, bit for bit."""
    want = va.frame_reference(family, (1, 1, 1))[0]
    m = va.matrix(family)
    for fused in (False, True):
        tr = VolumeTracer(va.volume(), va.camera(m), tf("cool"), m=m, sampling_rate=va.RATE, fused=fused).frame()
        assert (bits(tr.framebuffer(False)) == bits(want)).all() and (want[..., 3] > 0).sum() > 200
        assert not fused or tr.stats()["fused"] == 1


@pytest.mark.parametrize("name", ["perm", "perm_mirror"])
def test_bricked_frames_under_an_axis_permutation(hip, name):
    """Under a signed, scaled axis permutation (with and without mirroring) the bricks' world boxes are exact: 1, 8 and 27 bricks give
    one framebuffer in every bit, through the loop and through the fused frame (which reports fused = 1), and it is the checker's."""
    m = va.matrix(name)
    want = va.frame_reference(name, (1, 1, 1))[0]
    assert (want[..., 3] > 0).sum() > 500
    for split in va.SPLITS:
        assert (bits(va.frame_reference(name, split)[0]) == bits(want)).all()
        for fused in (False, True):
            tr = VolumeTracer(fc.bricks_of(va.volume(), split), va.camera(m), tf("cool"), m=m, sampling_rate=va.RATE, fused=fused).frame()
            assert (bits(tr.framebuffer(False)) == bits(want)).all(), (split, fused)
            if fused:
                assert tr.fused_stats["fused"] == 1 and tr.calls == 1
            else:
                assert tr.calls == va.frame_reference(name, split)[1]


@pytest.mark.parametrize("name", ["perm", "perm_mirror"])
def test_mixed_frames_under_an_axis_permutation(hip, name):
    """Geometry inside the bricked volume, both under the permutation: the composite does not depend on the bricking, fused or not."""
    m = va.matrix(name)
    lo, hi = va.box()
    v, t = ac.random_mesh(7, 150, 500)
    mesh = scenes.MeshData((0.5 * (lo + hi) + v * F(0.2) * (hi - lo)).astype(F), t, default_material(kd=(0.7, 0.6, 0.5)))
    cam = va.camera(m)
    scene = scenes._assemble([mesh], [0], [m], point_light(cam.eye), cam, "mixed-" + name)
    frames = []
    for split in va.SPLITS:
        for fused in (False, True):
            mt = MixedTracer(scene, fc.bricks_of(va.volume(), split), cam, tf("ramp"), m=m, sampling_rate=va.RATE, fused=fused).frame()
            assert not fused or (mt.volume.stats()["fused"] == 1 and mt.volume.calls == 1)
            frames.append(mt.framebuffer(False).copy())
            assert np.isfinite(mt.depth.download()).sum() > 100  # the mesh is in the picture
    for f in frames[1:]:
        assert (bits(f) == bits(frames[0])).all()


@pytest.mark.parametrize("overlap", [False, True])
@pytest.mark.parametrize("world", [1, 2, 3])
@pytest.mark.parametrize("name", ["perm", "perm_mirror"])
def test_volume_domains_under_an_axis_permutation(hip, name, world, overlap):
    """The Domain scheduler over 8 and 27 bricks dealt round-robin to one, two and three in-process ranks, BSP and overlapped: rank 0's
    composited framebuffer is the one-brick frame in every bit."""
    m = va.matrix(name)
    want = va.frame_reference(name, (1, 1, 1))[0]
    cam = va.camera(m)
    for split in va.SPLITS[1:]:
        parts = fc.bricks_of(va.volume(), split)
        owner = [i % world for i in range(len(parts))]

        def make(rank, dist):
            owned = [o == rank for o in owner]
            with LOCK:
                B = HipVolumeBackend(parts, cam, tf("cool"), m, va.RATE, True, False, owned)
            return VolumeDomainTracer(parts, owner, cam, tf("cool"), dist, torch, torch.device("cuda", 0), m=m, sampling_rate=va.RATE, backend=Locked(B), overlap=overlap)

        res = vdb.run_ranks(world, make)
        assert (bits(res[0][0][0]) == bits(want)).all(), split


@pytest.mark.parametrize("family", ["rot", "rot_scale", "shear", "mirror"])
def test_several_bricks_under_a_rotation_or_a_shear_are_refused(hip, family):
    """The world boxes of rotated neighbours overlap and the next-brick rule skips bricks (tests/test_affine_host.py shows the lost samples
    on the numpy frame loop), so every multi-brick tracer refuses such a matrix and says why; the library's frame entry points refuse too."""
    import ctypes as C

    m = va.matrix(family)
    parts = fc.bricks_of(va.volume(), (2, 2, 2))
    cam = va.camera(m)
    for make in (lambda: VolumeTracer(parts, cam, tf("cool"), m=m, sampling_rate=va.RATE),
                 lambda: VolumeTracer(parts, cam, tf("cool"), m=m, sampling_rate=va.RATE, fused=True),
                 lambda: HipVolumeBackend(parts, cam, tf("cool"), m, va.RATE),
                 lambda: MixedTracer(scenes.bunny_scene(64, 48), parts, cam, tf("cool"), m=m, sampling_rate=va.RATE)):
        with pytest.raises(ValueError, match="world boxes of neighbouring bricks overlap"):
            make()
    # the C entry points themselves: a tracer built under a permutation, then called with the rotation
    tr = VolumeTracer(parts, va.camera(va.matrix("perm")), tf("cool"), m=va.matrix("perm"), sampling_rate=va.RATE).frame()
    before = tr.framebuffer(False).copy()
    pod = capi.CameraPod((C.c_float * 3)(*cam.eye), (C.c_float * 3)(*cam.focus), (C.c_float * 3)(*cam.up), cam.fov, cam.width, cam.height, 1, 1, 0.0)
    mm = np.ascontiguousarray(np.tile(m, tr.n_inst), F)
    minv = np.ascontiguousarray(np.tile(scenes.instance_matrices(m)[0], tr.n_inst), F)
    lib, calls, st = capi.load(), C.c_uint64(0), capi.VolumeFusedStats()
    vols, qs, n = tr._arr(tr.adapters), tr._arr(tr.queues), C.c_size_t(tr.n_inst)
    assert lib.gvt_hip_volume_frame(tr.top.h, vols, capi.ptr(mm), capi.ptr(minv), n, C.byref(pod), qs, tr.fb.h, C.byref(calls)) == -1
    assert "overlap" in capi.last_error()
    assert lib.gvt_hip_volume_frame_fused(tr.top.h, vols, capi.ptr(mm), capi.ptr(minv), n, C.byref(pod), qs, tr.fb.h, None, C.byref(st)) == -1
    assert (bits(tr.framebuffer(False)) == bits(before)).all()  # nothing changed


@pytest.mark.parametrize("family", ac.FAMILIES)
def test_recorded_glm_vectors_through_the_march(hip, family):
    """The volume march on rays made of the recorded glm vectors (every vector as origin with every vector as direction: -0, zero, inf and NaN
    components) under glm's own inverse as minv, a 12^3 grid laid over the object-space rays glm recorded: vol_ray_range's products give
    the checker's bits -- the checker's xfm_point / xfm_vector are held to the recorded products on the host -- and the inf and NaN rays
    leave untouched."""
    marched = 0
    for k, row in enumerate(ac.glm_rows(family)):
        o, d, O, D = ac.glm_ray_case(row)
        ok = np.isfinite(O).all(axis=1) & np.isfinite(D).all(axis=1)
        pts = np.concatenate([O[ok], O[ok] + D[ok]]).astype(np.float64)
        lo, hi = np.percentile(pts, 10, axis=0), np.percentile(pts, 90, axis=0)
        vol = scenes.noise_volume(12, seed=3)
        vol.origin, vol.spacing = lo.astype(F), ((hi - lo) / 11).astype(F)
        ad = HipVolumeAdapter(vol, sampling_rate=0.5)
        ad.set_transfer(tf("ramp"))
        rays = np.zeros(len(o), RAY_DTYPE)
        rays["origin"], rays["direction"] = o, d
        rays["t_min"], rays["t_max"], rays["id"] = F(1e-6), np.finfo(F).max, np.arange(len(o))
        got = ad.trace(rays, row["m"], row["inverse"])
        with np.errstate(all="ignore"):
            want = va.vc.march(va.vc.Brick(vol, tf("ramp"), 0.5), rays, row["inverse"])
        same_bits(got, want, PLAIN)
        special = ~(np.isfinite(o).all(axis=1) & np.isfinite(d).all(axis=1))
        assert (got["w"][special] == 0).all()
        marched += int((got["w"] > 0).sum())
    assert marched > 40  # (the checker marches 62 rays of the shear rows, the fewest, and 89 to 133 of the other families')
