"""Smooth gradients on the device (vol_gradient_central and the k_volume_march_*_central entry points of csrc/volume.hip) against the numpy
checker (tests/volume_smooth_checker.py), bit for bit on color, w, t_min, depth and t: gvt_hip_volume_trace on one brick and on every
brick of two splits (all six ghost fetches beside the brick-interior path), frames over several brickings with and without skipping, the
clipped mixed frame, typed voxels with typed ghosts, time steps, the way back to CELL, grids that are not finite, the refusals, and two
ranks.  The inputs are tests/volume_smooth_cases.py's; tests/test_volume_smooth_host.py proves them non-vacuous on the CPU."""
import ctypes as C

import numpy as np
import pytest
import torch

from gravit_amd import capi, scenes
from gravit_amd.adapter import HipVolumeAdapter, TransferFunction
from gravit_amd.scheduler import MixedTracer, VolumeTracer
from tests import volume_amr_cases as amr_cases
from tests import volume_clip_checker as cc
from tests import volume_smooth_cases as cases
from tests import volume_smooth_checker as sm

pytestmark = pytest.mark.gpu

F = np.float32
IDENT = cases.IDENT
ALL = ("color", "w", "t_min", "depth", "t")
ERR_INVALID = -1


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b, fields=ALL):
    assert len(a) == len(b)  # no ray is left out
    for f in fields:
        x, y = bits(a[f]), bits(b[f])
        assert (x == y).all(), "%s: %d of %d rays differ" % (f, (x != y).reshape(len(a), -1).any(axis=1).sum(), len(a))


def adapter(part, t, S, mode=sm.SHADE_GRADIENT, kind="central", skip=True, native=False, rate=cases.RATE):
    ad = HipVolumeAdapter(part, sampling_rate=rate, skip=skip, native=native)
    ad.set_transfer(t)
    if S is not None:
        if len(S):
            ad.set_surfaces(S.iso, S.planes, float(S.opacity))
        ad.set_lights(list(zip(S.lpos, S.lcol)), float(S.ka), float(S.kd))
    ad.set_shading(mode == sm.SHADE_GRADIENT)
    if kind is not None:
        ad.set_gradient(kind)
    return ad


def trace(ad, rays):
    return ad.trace(rays, IDENT, IDENT)


def whole_brick(vol):
    return scenes.split_volume(vol, 1, 1, 1)[0]


@pytest.mark.parametrize("skip", [True, False])
@pytest.mark.parametrize("table", ["dense", "spikes"])
def test_one_brick_lit_equals_the_checker(hip, table, skip):
    vol, t, S = cases.volume(), cases.table(table), cases.lit()
    rays = cases.brick_rays(whole_brick(vol), n=600)
    ad = adapter(vol, t, S, skip=skip)
    assert ad.gradient() == "central" and ad.central_marches() == 0
    got = trace(ad, rays)
    want = sm.march(sm.Brick(vol, t, cases.RATE), S, rays, IDENT, kind=sm.CENTRAL)
    print("shaded: device %d, checker %d" % (ad.shaded(), sm.march.shaded))
    same_bits(got, want)
    assert ad.shaded() == sm.march.shaded > 0 and ad.central_marches() == 1
    info = ad.info()
    assert (info["samples_gathered"] < info["samples_marched"]) == (skip and table == "spikes")
    cell = trace(adapter(vol, t, S, kind=None, skip=skip), rays)
    assert (bits(cell["color"]) != bits(got["color"])).any()  # the kind shows ...
    same_bits(cell, got, ("w", "t_min", "depth", "t"))  # ... in the shaded colour alone


@pytest.mark.parametrize("which", ["3x3x3", "thin_x"])
def test_every_brick_of_a_split_equals_the_checker(hip, which):
    """Surfaces and lit fog at once; thin_x: 10 vertices along x cut into 9 bricks, so that both x-neighbours of every vertex are ghosts."""
    vol, split = (cases.volume(), (3, 3, 3)) if which == "3x3x3" else (cases.volume((10, 14, 11)), cases.THIN_X)
    t, S = cases.table("dense"), cases.surfaces()
    parts = cases.bricks_of(vol, split)
    assert len(parts) == int(np.prod(split))
    shaded = crossed = 0
    for part in parts:
        rays = cases.brick_rays(part, n=200)
        ad = adapter(part, t, S)
        same_bits(trace(ad, rays), sm.march(sm.Brick(part, t, cases.RATE), S, rays, IDENT, kind=sm.CENTRAL))
        assert ad.shaded() == sm.march.shaded > 0 and ad.crossings() == sm.march.crossings
        shaded, crossed = shaded + ad.shaded(), crossed + ad.crossings()
        ad.close()
    assert shaded > 1000 and crossed > 100


@pytest.mark.parametrize("skip", [True, False])
@pytest.mark.parametrize("setup", ["lit", "surfaces", "both"])
def test_frames_equal_the_checker_whatever_the_bricking(hip, setup, skip):
    vol, cam, t = cases.volume(), cases.camera(), cases.table("dense")
    S, mode = cases.SETUPS[setup]
    S = S()
    want, shaded, crossings = cases.frame_want(setup, sm.CENTRAL)
    cell = cases.frame_want(setup, sm.CELL)[0]
    for split in cases.SPLITS:
        tr = VolumeTracer(cases.bricks_of(vol, split), cam, t, sampling_rate=cases.RATE, skip=skip).set_lights(list(zip(S.lpos, S.lcol)))
        if len(S):
            tr.set_surfaces(S.iso, S.planes, float(S.opacity))
        tr.set_shading(mode == sm.SHADE_GRADIENT).set_gradient("central")
        got = tr.frame().framebuffer(False)
        assert got.shape == want.shape and (bits(got) == bits(want)).all(), split
        st = tr.stats()
        assert st["samples_shaded"] == shaded and st["crossings_rendered"] == crossings and st["central_marches"] == tr.calls >= int(np.prod(split))
        back = tr.set_gradient("cell").frame().framebuffer(False)
        assert (bits(back) == bits(cell)).all(), split
        assert tr.stats()["central_marches"] == st["central_marches"]


def test_the_sparse_table_skips_and_keeps_the_bits(hip):
    vol, cam, t, S = cases.volume(), cases.camera(), cases.table("spikes"), cases.lit()
    want, shaded, _ = cases.frame_want("lit", sm.CENTRAL, "spikes")
    assert shaded > 0
    for split, skip in (((1, 1, 1), True), ((1, 1, 1), False), ((2, 2, 2), True)):
        tr = VolumeTracer(cases.bricks_of(vol, split), cam, t, sampling_rate=cases.RATE, skip=skip).set_lights(list(zip(S.lpos, S.lcol)))
        got = tr.set_shading().set_gradient("central").frame().framebuffer(False)
        st = tr.stats()
        assert (bits(got) == bits(want)).all() and st["samples_shaded"] == shaded
        if split == (1, 1, 1):  # (the whole grid has two macro cells the table leaves empty, the one nearest the camera among them)
            assert (st["samples_gathered"] < st["samples_marched"]) == skip


def test_clipped_mixed_frame_equals_the_checker(hip):
    cam = scenes.Camera((0.0, 0.1, 0.3), (0.0, 0.1, -0.3), (0.0, 1.0, 0.0), float(F(45.0 * np.pi / 180.0)), 64, 48)
    scene = scenes.bunny_scene(64, 48)
    vol = scenes.mesh_in_volume(scene, scenes.VolumeData(cases.volume((17, 17, 17)).data), fill=0.6)
    parts = scenes.split_volume(vol, 2, 1, 2, ghosts=True)
    t, S = cases.table("dense"), cases.lit()
    mt = MixedTracer(scene, parts, cam, t, sampling_rate=1.0).set_lights(list(zip(S.lpos, S.lcol))).set_shading().set_gradient("central")
    got = mt.frame().framebuffer(False).copy()
    depth = mt.depth.download()
    bricks = [sm.Brick(b, t, 1.0) for b in parts]
    want, _ = sm.frame(bricks, mt.volume.inst_lo, mt.volume.inst_hi, IDENT, cam, S, plane=depth, kind=sm.CENTRAL)
    whole, _ = sm.frame(bricks, mt.volume.inst_lo, mt.volume.inst_hi, IDENT, cam, S, kind=sm.CENTRAL)
    assert sm.frame.shaded > 1000 and (want[..., 3] < whole[..., 3]).sum() > 50  # the clip shows
    assert (bits(got) == bits(cc.composite(want, mt.mesh_framebuffer(False), depth))).all()
    assert mt.volume.stats()["central_marches"] == mt.volume.calls > 0


@pytest.mark.parametrize("ty", ["uint8", "int16"])
def test_typed_voxels_with_typed_ghosts_answer_like_their_float_copy(hip, ty):
    vol = cases.volume()
    if ty == "uint8":
        data, rng = np.rint(vol.data * 255).astype(np.uint8), (0.0, 255.0)
    else:
        data, rng = np.rint((vol.data - 0.5) * 60000).astype(np.int16), (-30000.0, 30000.0)
    dense = cases.table("dense")
    t = TransferFunction(dense.cmap, dense.omap, rng)
    iso = [rng[0] + (rng[1] - rng[0]) * v for v in cases.ISO]
    S = sm.sc.Surfaces(iso, cases.PLANE, 0.5, cases.LIGHTS)
    typed = scenes.split_volume(scenes.VolumeData(data, vol.origin, vol.spacing), 2, 2, 2, ghosts=True)
    flt = scenes.split_volume(scenes.VolumeData(data.astype(F), vol.origin, vol.spacing), 2, 2, 2, ghosts=True)
    for i in (0, 5):
        assert all(g is None or g.dtype == data.dtype for g in typed[i].ghosts)
        rays = cases.brick_rays(typed[i], n=300)
        a, b = adapter(typed[i], t, S, native=True), adapter(flt[i], t, S)
        assert a.sample_bytes == data.itemsize and b.sample_bytes == 4
        got = trace(a, rays)
        same_bits(got, trace(b, rays))
        same_bits(got, sm.march(sm.Brick(flt[i], t, cases.RATE), S, rays, IDENT, kind=sm.CENTRAL))
        assert a.shaded() == b.shaded() == sm.march.shaded > 0 and a.crossings() == sm.march.crossings > 0


def test_a_time_step_needs_its_ghosts(hip):
    """update_samples + set_ghosts answers like a fresh volume of the new step; update_samples alone keeps the old step's layers."""
    v0, v1 = cases.volume(seed=3), cases.volume(seed=8)
    t, S = cases.table("dense"), cases.lit()
    p0, p1 = (scenes.split_volume(v, 2, 2, 2, ghosts=True)[3] for v in (v0, v1))
    assert any(g is not None and (g != h).any() for g, h in zip(p0.ghosts, p1.ghosts))
    rays = cases.brick_rays(p0, n=300)
    ad = adapter(p0, t, S)
    ad.update_samples(p1.data)
    stale = trace(ad, rays)  # the new samples between the old layers
    mixed = sm.Brick(p1, t, cases.RATE)
    mixed.set_ghosts(p0.ghosts)
    same_bits(stale, sm.march(mixed, S, rays, IDENT, kind=sm.CENTRAL))
    ad.set_ghosts(p1.ghosts)
    got = trace(ad, rays)
    same_bits(got, trace(adapter(p1, t, S), rays))
    same_bits(got, sm.march(sm.Brick(p1, t, cases.RATE), S, rays, IDENT, kind=sm.CENTRAL))
    assert (bits(stale["color"]) != bits(got["color"])).any()
    # ... and through a tracer: update(bricks) re-sends the ghosts the new bricks carry
    cam = cases.camera(32, 24)
    tr = VolumeTracer(scenes.split_volume(v0, 2, 2, 2, ghosts=True), cam, t, sampling_rate=cases.RATE).set_lights(list(zip(S.lpos, S.lcol)))
    tr.set_shading().set_gradient("central").frame()
    new = scenes.split_volume(v1, 2, 2, 2, ghosts=True)
    fresh = VolumeTracer(new, cam, t, sampling_rate=cases.RATE).set_lights(list(zip(S.lpos, S.lcol))).set_shading().set_gradient("central")
    assert (bits(tr.update(new).frame().framebuffer(False)) == bits(fresh.frame().framebuffer(False))).all()


@pytest.mark.parametrize("ty", ["float32", "uint8"])
def test_ghosts_from_device_tensors(hip, ty):
    """GVT_HIP_VOLUME_DEVICE: the layers are copied device to device and answer like the host's."""
    vol = cases.volume()
    t, S, native = cases.table("dense"), cases.lit(), ty != "float32"
    if native:
        vol = scenes.VolumeData(np.rint(vol.data * 255).astype(np.uint8), vol.origin, vol.spacing)
        t = TransferFunction(t.cmap, t.omap, (0.0, 255.0))
    part = scenes.split_volume(vol, 2, 2, 2, ghosts=True)[5]
    bare = scenes.split_volume(vol, 2, 2, 2)[5]
    rays = cases.brick_rays(part, n=300)
    want = trace(adapter(part, t, S, native=native), rays)
    ad = adapter(bare, t, S, kind=None, native=native)
    faces = [None if g is None else torch.from_numpy(g).cuda() for g in part.ghosts]
    ad.set_ghosts(faces)
    for f in faces:
        if f is not None:
            f.zero_()  # the samples were copied
    torch.cuda.synchronize()
    ad.set_gradient("central")
    same_bits(trace(ad, rays), want)
    with pytest.raises(ValueError):
        ad.set_ghosts([faces[0]] + list(part.ghosts[1:]))  # all host arrays or all GPU tensors


def test_back_to_cell_gives_the_bits_from_before(hip):
    vol, t, S = cases.volume(), cases.table("dense"), cases.surfaces()
    part = cases.bricks_of(vol, (2, 2, 2))[6]
    rays = cases.brick_rays(part, n=300)
    never = adapter(part, t, S, kind=None)
    before = trace(never, rays)
    assert never.gradient() == "cell" and never.central_marches() == 0
    ad = adapter(part, t, S, kind=None)
    same_bits(trace(ad, rays), before)
    ad.set_gradient("central")
    for k in (1, 2, 3):
        central = trace(ad, rays)
        assert ad.central_marches() == k  # once per march launch
    assert (bits(central["color"]) != bits(before["color"])).any()
    ad.set_gradient("cell")
    same_bits(trace(ad, rays), before)
    assert ad.central_marches() == 3 and ad.gradient() == "cell"
    plain = HipVolumeAdapter(part, sampling_rate=cases.RATE)  # nothing shaded: the kind is inert and the march is the plain one
    plain.set_transfer(t)
    a = trace(plain, rays)
    plain.set_gradient("central")
    same_bits(trace(plain, rays), a)
    assert plain.central_marches() == 0


@pytest.mark.parametrize("skip", [True, False])
def test_grids_that_are_not_finite_stay_finite_in_colour(hip, skip):
    vol = cases.nonfinite_volume()
    t, S = cases.table("dense"), cases.lit()
    rays = cases.brick_rays(whole_brick(vol), n=600)
    ad = adapter(vol, t, S, skip=skip)
    got = trace(ad, rays)
    same_bits(got, sm.march(sm.Brick(vol, t, cases.RATE), S, rays, IDENT, kind=sm.CENTRAL))
    assert ad.shaded() == sm.march.shaded > 1000
    assert np.isfinite(got["color"]).all() and np.isfinite(got["w"]).all()
    part = scenes.split_volume(vol, 2, 1, 2, ghosts=True)[1]  # ... and with the vertices that are not numbers in the layers
    assert any(g is not None and not np.isfinite(g).all() for g in part.ghosts)
    rays = cases.brick_rays(part, n=300)
    got = trace(adapter(part, t, S, skip=skip), rays)
    same_bits(got, sm.march(sm.Brick(part, t, cases.RATE), S, rays, IDENT, kind=sm.CENTRAL))
    assert np.isfinite(got["color"]).all()


def faces_arg(faces):
    keep = [None if f is None else np.ascontiguousarray(f) for f in faces]
    return C.cast((C.c_void_p * 6)(*[None if f is None else f.ctypes.data for f in keep]), C.c_void_p), keep


def test_refusals_leave_the_volume_as_it_was(hip):
    lib = capi.load()
    vol, t, S = cases.volume(), cases.table("dense"), cases.surfaces()
    parts = scenes.split_volume(vol, 3, 3, 3, ghosts=True)
    inner, corner = parts[13], parts[0]
    rays = cases.brick_rays(inner, n=200)

    def refused(ad, call, word, rays=rays):
        before, kind, n = trace(ad, rays), ad.gradient(), ad.central_marches()
        assert call() == ERR_INVALID and word in capi.last_error(), capi.last_error()
        assert ad.gradient() == kind
        same_bits(trace(ad, rays), before)
        assert ad.central_marches() == n + (1 if kind == "central" else 0)

    # CENTRAL with a required face missing: never given, or all but one
    bare = scenes.split_volume(vol, 3, 3, 3)[13]
    ad = adapter(bare, t, S, kind=None)
    refused(ad, lambda: lib.gvt_hip_volume_set_gradient(ad.h, capi.VOLUME_GRADIENT_CENTRAL), "face")
    for missing in range(6):
        ptrs, keep = faces_arg([None if i == missing else g for i, g in enumerate(inner.ghosts)])
        assert lib.gvt_hip_volume_set_ghosts(ad.h, ptrs, capi.VOXEL_F32, 0) == 0
        refused(ad, lambda: lib.gvt_hip_volume_set_gradient(ad.h, capi.VOLUME_GRADIENT_CENTRAL), "face %d" % missing)
    # removing a required face while CENTRAL
    ad = adapter(inner, t, S)
    for missing in range(6):
        ptrs, keep = faces_arg([None if i == missing else g for i, g in enumerate(inner.ghosts)])
        refused(ad, lambda: lib.gvt_hip_volume_set_ghosts(ad.h, ptrs, capi.VOXEL_F32, 0), "face %d" % missing)
    full, keep_full = faces_arg(inner.ghosts)
    # a wrong voxel type, an unknown flag, an unknown kind, null arguments
    refused(ad, lambda: lib.gvt_hip_volume_set_ghosts(ad.h, full, capi.VOXEL_U8, 0), "type")
    refused(ad, lambda: lib.gvt_hip_volume_set_ghosts(ad.h, full, capi.VOXEL_F32, 2), "flag")
    refused(ad, lambda: lib.gvt_hip_volume_set_ghosts(ad.h, None, capi.VOXEL_F32, 0), "null")
    for bad in (2, -1):
        refused(ad, lambda: lib.gvt_hip_volume_set_gradient(ad.h, bad), "kind")
    assert lib.gvt_hip_volume_set_ghosts(None, full, capi.VOXEL_F32, 0) == ERR_INVALID
    assert lib.gvt_hip_volume_set_gradient(None, 1) == ERR_INVALID and lib.gvt_hip_volume_get_gradient(None, None, None) == ERR_INVALID
    assert lib.gvt_hip_volume_get_gradient(ad.h, None, None) == 0  # either may be NULL
    with pytest.raises(ValueError):
        ad.set_gradient("smooth")
    with pytest.raises(ValueError):
        ad.set_ghosts(inner.ghosts[:5])
    # a layer beyond a face on the global boundary
    crays = cases.brick_rays(corner, n=200)
    ad = adapter(corner, t, S)
    for i in (0, 2, 4):
        faces = list(corner.ghosts)
        assert faces[i] is None
        faces[i] = np.zeros_like(corner.ghosts[i + 1])
        ptrs, keep = faces_arg(faces)
        refused(ad, lambda: lib.gvt_hip_volume_set_ghosts(ad.h, ptrs, capi.VOXEL_F32, 0), "boundary", crays)
    # AMR volumes take no shading: in both directions
    amr = amr_cases.scene()
    arays = cases.brick_rays(whole_brick(amr), n=200)
    ad = HipVolumeAdapter(amr, sampling_rate=cases.RATE)
    ad.set_transfer(t)
    assert ad.amr_info()["n_subgrids"] > 0
    refused(ad, lambda: lib.gvt_hip_volume_set_gradient(ad.h, capi.VOLUME_GRADIENT_CENTRAL), "AMR", arays)
    flat = HipVolumeAdapter(scenes.VolumeData(amr.data, amr.origin, amr.spacing), sampling_rate=cases.RATE)
    flat.set_transfer(t)
    flat.set_gradient("central")
    before = trace(flat, arays)
    with pytest.raises(capi.GvtHipError, match="CENTRAL"):
        flat.set_subgrids(amr.subgrids)
    assert flat.amr_info()["n_subgrids"] == 0 and flat.gradient() == "central"
    same_bits(trace(flat, arays), before, ("color", "w", "t_min", "depth"))


@pytest.mark.parametrize("overlap", [False, True])
def test_two_ranks_equal_the_one_rank_frame(hip, overlap):
    from tests import volume_domain_backend as vdb
    from tests.test_gpu_volume_domains import gpu_run

    parts = scenes.split_volume(vdb.case_volume(), 2, 2, 2, ghosts=True)
    cam, t = vdb.case_camera("outside"), vdb.case_tf("thin")

    def setup(tr):
        tr.set_lights(cases.LIGHTS).set_shading(True).set_gradient("central")

    one = VolumeTracer(parts, cam, t, sampling_rate=vdb.RATE)
    setup(one)
    fb1, st1 = one.frame().framebuffer(False), one.stats()
    cell = one.set_gradient("cell").frame().framebuffer(False)
    assert st1["samples_shaded"] > 1000 and st1["central_marches"] >= 8 and (bits(cell) != bits(fb1)).any()
    owner = vdb.case_owner("checker", parts, 2)
    res = gpu_run(parts, owner, 2, cam, t, overlap, setup=setup)
    assert (bits(res[0][0][0]) == bits(fb1)).all()
    assert sum(res[r][0][4]["samples_shaded"] for r in range(2)) == st1["samples_shaded"]
    assert all(res[r][0][4]["central_marches"] > 0 for r in range(2)) and sum(res[r][0][1] for r in range(2)) > 0
