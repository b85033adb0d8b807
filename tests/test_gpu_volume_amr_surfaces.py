"""Shaded AMR volumes on the device (GVT_HIP_VOLUME_AMR_SHADED; k_volume_march_amr_surf / _lit / _surf_lit in csrc/volume_amr.inc) against
the numpy checker (tests/volume_amr_surface_checker.py), bit for bit: isovalues, slice planes and lit fog in refined cells through
gvt_hip_volume_trace, clipped and unclipped, with carried sides; skipping against no skipping; bricked and mixed frames; the lit rules;
removing the subgrids; non-finite vertices; and the gates."""
import ctypes as C
from dataclasses import replace

import numpy as np
import pytest
import torch  # noqa: F401  (before the library initialises the device, as in test_gpu_volume_amr.py)

from gravit_amd import capi, scenes
from gravit_amd.adapter import HipVolumeAdapter, TransferFunction
from gravit_amd.scheduler import MixedTracer, NativeTracer, VolumeTracer
from tests import volume_amr_cases as cases
from tests import volume_amr_checker as ac
from tests import volume_amr_surface_cases as scases
from tests import volume_amr_surface_checker as asc
from tests import volume_checker as vc
from tests import volume_clip_checker as cc
from tests import volume_shade_checker as shc
from tests.test_gpu_volume import IDENT, MOVED, make_rays, read, tf
from tests.test_gpu_volume_amr import _pod, _raw_set, camera, thin

pytestmark = pytest.mark.gpu

F = np.float32
ERR_INVALID = -1
FIELDS = ("color", "w", "t_min", "depth", "t")
RATE = 1.3
VARIANTS = {"surf": (True, False), "lit": (False, True), "surf_lit": (True, True)}


def same_bits(a, b, fields=FIELDS):
    for f in fields:
        assert (np.ascontiguousarray(a[f]).view(np.uint32) == np.ascontiguousarray(b[f]).view(np.uint32)).all(), f


def clear():
    """No opacity anywhere: the fog adds nothing, every macro cell is empty by the table, the surfaces alone show."""
    return TransferFunction(read("CoolWarm.cmap", 4), np.array([[0.0, 0.0], [1.0, 0.0]], F), (0.0, 1.0))


def all_rays(vol, m):
    """About 1500 rays: through the whole brick, in S0's vertex planes, and aimed at the level-2 subgrid S1."""
    return np.concatenate([make_rays(vol, m, n=1000), cases.plane_rays(vol, m, n=300), scases.s1_rays(vol, m, n=200)])


def shaded_adapter(vol, t, S, surf, lit, skip=True, rate=RATE):
    ad = HipVolumeAdapter(vol, sampling_rate=rate, skip=skip, amr_shaded=True)
    ad.set_transfer(t)
    if surf:
        ad.set_surfaces(**S.args)
    ad.set_lights(**S.light_args)
    ad.set_shading(lit)
    return ad


def checker_surfaces(S, surf):
    """What the checker sees of S on a volume whose surfaces were not set: the lights alone."""
    return S if surf else shc.lights_only(scases.LIGHTS, S.ka, S.kd)


@pytest.fixture(scope="module")
def amr_scene():
    return cases.scene()


@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("moved", [False, True])
def test_trace_equals_the_checker(hip, amr_scene, variant, clip, moved):
    vol = amr_scene
    surf, lit = VARIANTS[variant]
    m = MOVED if moved else IDENT
    minv = scenes.instance_matrices(m)[0]
    t = thin()
    S = scases.surfaces(vol, opacity=0.3)
    Sc = checker_surfaces(S, surf)
    mode = asc.SHADE_GRADIENT if lit else asc.SHADE_NONE
    rays = all_rays(vol, m)
    if clip:  # every other ray ends inside the brick (for many of them inside S0)
        rays["depth"][::2] |= cc.CLIP
        rays["t_max"][::2] = F(0.9) if not moved else F(1.2)
    B = ac.AmrBrick(vol, t, RATE)
    counts = {}
    want = asc.march(B, Sc, rays, minv, mode, counts)
    assert 0 < counts["refined"] < counts["marched"]
    if surf:
        assert counts["crossings_refined"] > 0 and counts["crossings_grid_change"] > 0 and counts["plane_crossings_refined"] > 0
        assert counts["crossings_level"].get(2, 0) > 0
    if lit:
        assert 0 < counts["shaded_refined"] < counts["shaded"]
    fields = FIELDS if surf else FIELDS[:4]
    # the continuation: the clipped rays go on from their last sample, with the sides they carry in t -- for some the next sample is refined
    go_on = want.copy()
    go_on["depth"] &= ~(cc.CLIP | vc.BOUNDARY)
    counts2 = {}
    want2 = asc.march(B, Sc, go_on, minv, mode, counts2)
    if clip and surf:
        assert counts2["carried_refined"] > 0 and counts2["crossings"] > 0
    for skip in (True, False):
        ad = shaded_adapter(vol, t, S, surf, lit, skip)
        got = ad.trace(rays, m, minv)
        same_bits(got, want, fields)
        amr = ad.amr_info()
        assert ad.crossings() == counts["crossings"] and ad.shaded() == counts["shaded"] and amr["amr_marches"] == 1
        assert ad.info()["samples_marched"] == counts["marched"]
        if not skip:
            assert amr["samples_refined"] == counts["refined"]
        else:
            assert amr["samples_refined"] <= counts["refined"]
        again = got.copy()
        again["depth"] &= ~(cc.CLIP | vc.BOUNDARY)
        same_bits(ad.trace(again, m, minv), want2, fields)
        assert ad.crossings() == counts["crossings"] + counts2["crossings"] and ad.shaded() == counts["shaded"] + counts2["shaded"]
    if clip:  # ... and the two halves are one unclipped march
        whole = rays.copy()
        whole["depth"] &= ~cc.CLIP
        one = asc.march(B, Sc, whole, minv, mode)
        open_ = (one["depth"] & vc.OPAQUE) == 0  # (an opaque ray marched again takes one more sample, as any ray that arrives opaque does)
        assert open_.sum() > len(rays) // 2
        same_bits(want2[open_], one[open_], ("color", "w", "t_min") + (("t",) if surf else ()))


@pytest.mark.parametrize("kind", ["thin", "spikes", "peak"])
def test_skipping_gives_the_same_bits(hip, amr_scene, kind):
    """skip=True against skip=False, the rays' t field included.  peak: level 0 stays below the isovalue 1.5, a block of S0's vertices holds
    2.0 and the table is empty everywhere: a surface skip table built from the level-0 ranges would skip every crossing."""
    if kind == "peak":
        vol, t = scases.peak_scene(), clear()
        S = scases.surfaces(vol, isovalues=(scases.PEAK_ISO,), plane=False)
    else:
        vol, t = amr_scene, (thin() if kind == "thin" else tf("spikes"))
        S = scases.surfaces(vol, opacity=0.3)
    rays = all_rays(vol, IDENT)
    counts = {}
    want = asc.march(ac.AmrBrick(vol, t, RATE), S, rays, IDENT, asc.SHADE_GRADIENT, counts)
    assert counts["crossings_refined"] > 0
    a, b = shaded_adapter(vol, t, S, True, True, skip=True), shaded_adapter(vol, t, S, True, True, skip=False)
    ra, rb = a.trace(rays, IDENT, IDENT), b.trace(rays, IDENT, IDENT)
    same_bits(ra, rb)
    same_bits(ra, want)
    assert a.crossings() == b.crossings() == counts["crossings"] > 0 and a.shaded() == b.shaded() == counts["shaded"]
    ia, ib = a.info(), b.info()
    assert ia["samples_marched"] == ib["samples_marched"] == counts["marched"]
    if kind != "thin":
        assert ia["n_blocks_empty"] > 0 and ia["samples_gathered"] < ib["samples_gathered"] == ib["samples_marched"]
    if kind == "peak":
        assert ia["n_blocks_empty"] == 27 and (want["w"] > 0).any()
        # setting the surfaces after the subgrids, or the subgrids after the surfaces, builds the same table
        late = HipVolumeAdapter(scenes.VolumeData(vol.data, vol.origin, vol.spacing), sampling_rate=RATE, amr_shaded=True)
        late.set_transfer(t)
        late.set_surfaces(**S.args)
        late.set_lights(**S.light_args)
        late.set_shading(True)
        late.set_subgrids(vol.subgrids)
        same_bits(late.trace(rays, IDENT, IDENT), want)
        assert late.info()["samples_gathered"] == ia["samples_gathered"]


@pytest.fixture(scope="module")
def frame_case(amr_scene):
    vol = amr_scene
    t = thin()
    cam = camera()
    S = scases.surfaces(vol, opacity=0.3)
    parts = scenes.split_amr_volume(vol, 2, 2, 2, cuts=cases.CUTS)
    bricks = [ac.AmrBrick(b, t, RATE) for b in parts]
    return vol, t, cam, S, parts, bricks


def shaded_tracer(cls, args, S, **kw):
    tr = cls(*args, sampling_rate=RATE, amr_shaded=True, **kw)
    tr.set_surfaces(**S.args)
    tr.set_lights(**S.light_args)
    tr.set_shading(True)
    return tr


def test_bricked_frame_equals_the_one_brick_frame_and_the_checker(hip, frame_case):
    vol, t, cam, S, parts, bricks = frame_case
    counts, rounds = {}, []
    want, calls = asc.frame(bricks, [b.lo for b in parts], [b.hi for b in parts], IDENT, cam, S, counts=counts, rounds=rounds)
    assert counts["crossings_refined"] > 0 and counts["shaded_refined"] > 0 and (want[..., 3] > 0).sum() > 300
    one = shaded_tracer(VolumeTracer, (vol, cam, t), S).frame()
    eight = shaded_tracer(VolumeTracer, (parts, cam, t), S).frame()
    fb1, fb8 = one.framebuffer(False), eight.framebuffer(False)
    assert (fb1.view(np.uint32) == fb8.view(np.uint32)).all()
    assert (fb8.view(np.uint32) == want.view(np.uint32)).all()
    assert eight.calls == calls > 1 and one.calls == 1
    st = eight.stats()
    assert st["samples_refined"] > 0 and st["amr_marches"] == sum(1 for brick, _ in rounds if parts[brick].subgrids) >= 2
    assert sum(a.crossings() for a in eight.adapters) == counts["crossings"] == one.adapters[0].crossings()
    assert sum(a.shaded() for a in eight.adapters) == counts["shaded"] == one.adapters[0].shaded()
    # the fused and the shadowed tracers treat a brick with subgrids as ever: the loop, or a refusal
    fused = shaded_tracer(VolumeTracer, (parts, cam, t), S, fused=True, fused_shaded=True).frame()
    assert fused.fused_stats["fused"] == 0 and (fused.framebuffer(False).view(np.uint32) == want.view(np.uint32)).all()
    with pytest.raises(capi.GvtHipError):
        shaded_tracer(VolumeTracer, (parts, cam, t), S, shadows=True).frame()


def test_mixed_frame_over_shaded_amr_bricks(hip, frame_case):
    """A small mesh inside S0's box: the clipped frame (gvt_hip_volume_frame_clipped) over one brick and over eight."""
    vol, t, cam, S, parts, bricks = frame_case
    org, sp = np.asarray(vol.origin, np.float64), np.asarray(vol.spacing, np.float64)
    mid = org + (np.array(cases.S0["lo"]) + 0.5 * np.array(cases.S0["cells"])) * sp
    verts = np.array([[-1, -1, -1], [1, -1, -1], [0, 1, -1], [0, 0, 1]], F)
    tris = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]], np.int32)
    scene = scenes._assemble([scenes.MeshData(verts, tris)], [0], [scenes.mat_translate_scale(tuple(mid), (0.13, 0.13, 0.13))],
                             scenes.point_light((1.0, 2.0, 3.0)), cam, "tetrahedron")
    mesh = NativeTracer(replace(scene, camera=cam))().framebuffer(False)
    got = None
    for bricking in (vol, parts):
        mt = shaded_tracer(MixedTracer, (scene, bricking, cam, t), S).frame()
        depth = mt.depth.download()
        wall = np.isfinite(depth)
        assert 20 < wall.sum() < cam.width * cam.height // 2
        if got is None:
            fog, _ = asc.frame(bricks, [b.lo for b in parts], [b.hi for b in parts], IDENT, cam, S, plane=depth)
            full, _ = asc.frame(bricks, [b.lo for b in parts], [b.hi for b in parts], IDENT, cam, S)
            assert (fog[wall].view(np.uint32) != full[wall].view(np.uint32)).any()
            got = cc.composite(fog, mesh, depth)
        assert (mt.framebuffer(False).view(np.uint32) == got.view(np.uint32)).all()
        assert mt.volume.stats()["amr_marches"] > 0


def test_lit_rules(hip, amr_scene):
    vol = amr_scene
    t = thin()
    rays = all_rays(vol, IDENT)
    plain = ac.march(ac.AmrBrick(vol, t, RATE), rays, IDENT)
    unflagged = HipVolumeAdapter(vol, sampling_rate=RATE)
    unflagged.set_transfer(t)
    same_bits(unflagged.trace(rays, IDENT, IDENT), plain, FIELDS[:4])
    S = scases.surfaces(vol, ka=1.0, kd=0.0)
    ad = shaded_adapter(vol, t, S, False, True)
    same_bits(ad.trace(rays, IDENT, IDENT), plain, FIELDS[:4])  # ka = 1, kd = 0: x * (1 + 0 * S) = x
    assert ad.shaded() > 0 and ad.amr_info()["amr_marches"] == 1
    ad.set_lights([])  # no lights: nothing to shade with, the plain AMR march
    same_bits(ad.trace(rays, IDENT, IDENT), plain, FIELDS[:4])
    assert ad.shading() == capi.VOLUME_SHADE_GRADIENT and ad.amr_info()["amr_marches"] == 2
    # with surfaces: no lights gives the unlit surface bits (rgb = c), shading on or off
    S = scases.surfaces(vol, opacity=0.3, lights=False)
    want = asc.march(ac.AmrBrick(vol, t, RATE), S, rays, IDENT, asc.SHADE_NONE)
    for lit in (False, True):
        same_bits(shaded_adapter(vol, t, S, True, lit).trace(rays, IDENT, IDENT), want)


def test_removing_the_subgrids_gives_the_plain_surface_volume(hip, amr_scene):
    vol = amr_scene
    t = thin()
    rays = all_rays(vol, IDENT)
    S = scases.surfaces(vol, opacity=0.3)
    plain_vol = scenes.VolumeData(vol.data, vol.origin, vol.spacing)
    want = shc.march(vc.Brick(plain_vol, t, RATE), S, rays, IDENT)
    ad = shaded_adapter(vol, t, S, True, True)
    assert not (ad.trace(rays, IDENT, IDENT)["color"].view(np.uint32) == want["color"].view(np.uint32)).all()
    assert ad.amr_info()["amr_marches"] == 1
    ad.set_subgrids([])  # (the adapter's flag: accepted on a volume that has surfaces and shading)
    same_bits(ad.trace(rays, IDENT, IDENT), want)
    info = ad.amr_info()
    assert info["amr_marches"] == 1 and info["n_subgrids"] == 0 and info["subgrid_bytes"] == 0
    never = HipVolumeAdapter(plain_vol, sampling_rate=RATE)
    never.set_transfer(t)
    assert ad.info()["n_blocks_empty"] == never.info()["n_blocks_empty"] and ad.info()["value_max"] == never.info()["value_max"]
    ad.set_subgrids(vol.subgrids)  # ... and back
    same_bits(ad.trace(rays, IDENT, IDENT), asc.march(ac.AmrBrick(vol, t, RATE), S, rays, IDENT))


def test_non_finite_vertices(hip, amr_scene):
    """One NaN and one Inf vertex in S0, lit fog and the slice plane (a crossed isovalue tests len > 0 only, so its colour may be NaN by
    the surface contract): the checker's bits and a finite C."""
    vol = amr_scene
    s0 = vol.subgrids[0]
    data = s0.data.copy()
    data[8, 5, 6] = np.nan
    data[10, 6, 9] = np.inf
    wild = scenes.VolumeData(vol.data, vol.origin, vol.spacing, [scenes.Subgrid(s0.parent, s0.ratio, s0.lo, s0.cells, data)] + vol.subgrids[1:])
    t = thin()
    rays = all_rays(vol, IDENT)
    S = scases.surfaces(vol, isovalues=(), opacity=0.3)
    want = asc.march(ac.AmrBrick(wild, t, RATE), S, rays, IDENT)
    clean = asc.march(ac.AmrBrick(vol, t, RATE), S, rays, IDENT)
    assert (want["color"].view(np.uint32) != clean["color"].view(np.uint32)).any() and np.isfinite(want["color"]).all()
    for skip in (True, False):
        got = shaded_adapter(wild, t, S, True, True, skip).trace(rays, IDENT, IDENT)
        same_bits(got, want)
        assert np.isfinite(got["color"]).all() and np.isfinite(got["w"]).all()


def test_gates(hip, amr_scene):
    vol = amr_scene
    t = thin()
    lib = capi.load()
    rays = all_rays(vol, IDENT)[::5]
    S = scases.surfaces(vol, opacity=0.3)
    B = ac.AmrBrick(vol, t, RATE)
    want = asc.march(B, S, rays, IDENT)
    plain_vol = scenes.VolumeData(vol.data, vol.origin, vol.spacing)
    ok = _pod(-1, 2, (3, 2, 1), (6, 5, 9))
    iso, pl = np.array([0.5], F), np.array([0, 0, 1, 0.1], F)
    flag = capi.VOLUME_AMR_SHADED
    assert flag == 8
    # accepted with the flag: subgrids on a volume that has surfaces and shading, n > 0 and n == 0; surfaces and shading on a flagged set
    ad = HipVolumeAdapter(plain_vol, sampling_rate=RATE)
    ad.set_transfer(t)
    ad.set_surfaces(**S.args)
    ad.set_lights(**S.light_args)
    ad.set_shading(True)
    assert _raw_set(ad, [ok]) == ERR_INVALID and "surfaces or gradient shading" in capi.last_error()  # without the flag: as ever
    assert _raw_set(ad, [ok], flags=flag) == 0 and ad.amr_info()["n_subgrids"] == 1
    assert _raw_set(ad, [], flags=0) == ERR_INVALID and ad.amr_info()["n_subgrids"] == 1  # removing them needs the flag too
    assert _raw_set(ad, [], flags=flag) == 0 and ad.amr_info()["n_subgrids"] == 0
    ad.set_subgrids(vol.subgrids, shaded=True)
    same_bits(ad.trace(rays, IDENT, IDENT), want)
    assert lib.gvt_hip_volume_set_surfaces(ad.h, capi.ptr(iso), 1, capi.ptr(pl), 1, 1.0) == 0
    assert lib.gvt_hip_volume_set_shading(ad.h, capi.VOLUME_SHADE_NONE) == 0 and lib.gvt_hip_volume_set_shading(ad.h, capi.VOLUME_SHADE_GRADIENT) == 0
    ad.set_surfaces(**S.args)
    same_bits(ad.trace(rays, IDENT, IDENT), want)
    # still refused on a flagged AMR volume, the bits unchanged: unknown flags, CENTRAL, in-place updates
    for flags in (2, 4, 2 | flag, 4 | flag, 16):
        assert _raw_set(ad, [ok], flags=flags) == ERR_INVALID and "unknown flag" in capi.last_error(), flags
    assert lib.gvt_hip_volume_set_gradient(ad.h, capi.VOLUME_GRADIENT_CENTRAL) == ERR_INVALID and ad.gradient() == "cell"
    new = np.ascontiguousarray(vol.data[::-1])
    assert lib.gvt_hip_volume_update_samples(ad.h, capi.ptr(new), C.c_size_t(new.size), 0, None) == ERR_INVALID and "subgrids" in capi.last_error()
    assert lib.gvt_hip_volume_update_samples_typed(ad.h, capi.ptr(new), capi.VOXEL_F32, C.c_size_t(new.size), 0, None) == ERR_INVALID
    assert ad.amr_info()["n_subgrids"] == 4
    same_bits(ad.trace(rays, IDENT, IDENT), want)
    # a CENTRAL volume takes no subgrids, flagged or not (one brick of the whole grid: every face is on the boundary, CENTRAL needs no ghosts)
    central = HipVolumeAdapter(plain_vol, sampling_rate=RATE)
    central.set_transfer(t)
    central.set_surfaces(**S.args)
    central.set_gradient("central")
    before = central.trace(rays, IDENT, IDENT)
    assert _raw_set(central, [ok], flags=flag) == ERR_INVALID and "CENTRAL" in capi.last_error()
    assert central.amr_info()["n_subgrids"] == 0
    same_bits(central.trace(rays, IDENT, IDENT), before)
    # a volume that is not float32
    u8 = HipVolumeAdapter(scenes.VolumeData(np.rint(vol.data * 255).astype(np.uint8), vol.origin, vol.spacing), sampling_rate=RATE, native=True)
    tu = thin()
    tu.value_range = (0.0, 255.0)
    u8.set_transfer(tu)
    before = u8.trace(rays, IDENT, IDENT)
    assert _raw_set(u8, [ok], flags=flag) == ERR_INVALID and "voxel type" in capi.last_error()
    same_bits(u8.trace(rays, IDENT, IDENT), before, FIELDS[:4])
    # an unflagged AMR volume still refuses surfaces and shading, and replacing a flagged set by an unflagged one is refused while it has them
    amr = HipVolumeAdapter(vol, sampling_rate=RATE)
    amr.set_transfer(t)
    plain = ac.march(B, rays, IDENT)
    assert lib.gvt_hip_volume_set_surfaces(amr.h, capi.ptr(iso), 1, None, 0, 1.0) == ERR_INVALID
    assert lib.gvt_hip_volume_set_surfaces(amr.h, None, 0, capi.ptr(pl), 1, 1.0) == ERR_INVALID
    assert lib.gvt_hip_volume_set_shading(amr.h, capi.VOLUME_SHADE_GRADIENT) == ERR_INVALID and amr.shading() == capi.VOLUME_SHADE_NONE
    same_bits(amr.trace(rays, IDENT, IDENT), plain, FIELDS[:4])
    assert amr.crossings() == 0 and amr.shaded() == 0
    assert _raw_set(ad, [ok], flags=0) == ERR_INVALID and ad.amr_info()["n_subgrids"] == 4
    same_bits(ad.trace(rays, IDENT, IDENT), want)
    # a flagged set replaced by an unflagged one on a volume without surfaces and shading: the plain AMR volume, refusals included
    ad.set_surfaces()
    ad.set_shading(False)
    ad.set_subgrids(vol.subgrids, shaded=False)
    same_bits(ad.trace(rays, IDENT, IDENT), plain, FIELDS[:4])
    assert lib.gvt_hip_volume_set_surfaces(ad.h, capi.ptr(iso), 1, None, 0, 1.0) == ERR_INVALID
    assert lib.gvt_hip_volume_set_shading(ad.h, capi.VOLUME_SHADE_GRADIENT) == ERR_INVALID
