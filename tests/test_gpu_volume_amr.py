"""AMR volumes on the device (csrc/volume_amr.inc, gvt_hip_volume_set_subgrids) against the numpy checker (tests/volume_amr_checker.py),
bit for bit: k_volume_march_amr through gvt_hip_volume_trace with and without skipping, the merged macro-cell ranges, vertices the
march must never read, exactly refined fields against the library's own plain march, bricked frames, the clipped frame, the plain
path of volumes without subgrids, and the refusals."""
import ctypes as C

import numpy as np
import pytest
import torch  # (before the library initialises the device, as in test_gpu_volume_update.py)

from gravit_amd import capi, scenes
from gravit_amd.adapter import DepthPlane, HipVolumeAdapter, TransferFunction
from gravit_amd.scheduler import VolumeTracer
from tests import volume_amr_cases as cases
from tests import volume_amr_checker as ac
from tests import volume_checker as vc
from tests import volume_clip_checker as vcc
from tests.test_gpu_volume import IDENT, MOVED, make_rays, read, same_bits, tf

pytestmark = pytest.mark.gpu

F = np.float32
ERR_INVALID = -1


def camera(w=64, h=48):
    return scenes.Camera((0.9, 1.3, 1.6), (0.25, 0.6, 0.0), (0.0, 1.0, 0.0), float(F(35.0 * np.pi / 180.0)), w, h)


def thin():
    """Opacity rising to 0.08: every ray crosses the whole volume, so the bricks and subgrids far from the camera get their share."""
    return TransferFunction(read("CoolWarm.cmap", 4), np.array([[0.0, 0.0], [1.0, 0.08]], F), (0.0, 1.0))


def all_rays(vol, m):
    return np.concatenate([make_rays(vol, m, n=1500), cases.plane_rays(vol, m)])


@pytest.fixture(scope="module")
def amr_scene():
    return cases.scene()


@pytest.mark.parametrize("kind", ["cool", "spikes"])
@pytest.mark.parametrize("rate,moved", [(1.3, False), (2.6, True)])
def test_trace_equals_the_checker(hip, amr_scene, kind, rate, moved):
    vol = amr_scene
    m = MOVED if moved else IDENT
    minv = scenes.instance_matrices(m)[0]
    t = tf(kind)
    rays = all_rays(vol, m)
    B = ac.AmrBrick(vol, t, rate)
    counts = {}
    want = ac.march(B, rays, minv, counts)
    assert 0 < counts["refined"] < counts["marched"]
    winfo = ac.info(B)
    for skip in (True, False):
        ad = HipVolumeAdapter(vol, sampling_rate=rate, skip=skip)
        ad.set_transfer(t)
        got = ad.trace(rays, m, minv)
        same_bits(got, want)
        info, amr = ad.info(), ad.amr_info()
        for key in ("value_min", "value_max"):
            assert F(info[key]).view(np.uint32) == F(winfo[key]).view(np.uint32), key
        assert info["n_blocks"] == winfo["n_blocks"] == 27 and info["n_blocks_empty"] == winfo["n_blocks_empty"]
        assert amr["n_subgrids"] == 4 and amr["n_levels"] == 3 and amr["amr_marches"] == 1
        assert amr["subgrid_bytes"] >= 4 * sum(s.data.size for s in vol.subgrids)
        assert info["samples_marched"] == counts["marched"]
        if not skip:
            assert amr["samples_refined"] == counts["refined"] and info["samples_gathered"] == counts["marched"]
        else:
            assert amr["samples_refined"] <= counts["refined"]
        same_bits(ad.trace(got, m, minv), ac.march(B, want, minv))  # a continuation: the same lattice goes on
    if kind == "spikes":
        assert winfo["n_blocks_empty"] > 0
    else:
        assert (want["w"][:600] > 0).any()


def test_subgrids_set_before_the_transfer_function_and_from_device_memory(hip, amr_scene):
    vol = amr_scene
    t = tf("spikes")
    rays = all_rays(vol, IDENT)
    want = ac.march(ac.AmrBrick(vol, t, 1.3), rays, IDENT)
    plain = scenes.VolumeData(vol.data, vol.origin, vol.spacing)
    late = HipVolumeAdapter(plain, sampling_rate=1.3)
    late.set_transfer(t)
    late.set_subgrids(vol.subgrids)  # after the transfer function
    same_bits(late.trace(rays, IDENT, IDENT), want)
    dev = HipVolumeAdapter(plain, sampling_rate=1.3)
    dev.set_subgrids([scenes.Subgrid(s.parent, s.ratio, s.lo, s.cells, torch.from_numpy(s.data).cuda()) for s in vol.subgrids])
    dev.set_transfer(t)
    same_bits(dev.trace(rays, IDENT, IDENT), want)
    assert dev.info()["n_blocks_empty"] == late.info()["n_blocks_empty"] == ac.info(ac.AmrBrick(vol, t, 1.3))["n_blocks_empty"]


def test_skip_trap_ranges_are_merged(hip):
    """Level 0 is transparent everywhere, the opacity lives in S0 and S1 alone: a skip table from the level-0 ranges would skip it all."""
    vol = cases.level0(np.full(cases.COUNTS[::-1], 0.2, F))
    s0 = scenes.refine(vol, cases.S0["lo"], cases.S0["cells"], cases.S0["ratio"], fn=lambda x, y, z: 0.9 + 0 * (x + y + z))
    scenes.refine(vol, cases.S1["lo"], cases.S1["cells"], cases.S1["ratio"], parent=s0, fn=lambda x, y, z: 0.9 + 0 * (x + y + z))
    t = tf("spikes")
    cam = camera()
    tr = VolumeTracer(vol, cam, t, sampling_rate=1.3).frame()
    fb = tr.framebuffer(False)
    B = ac.AmrBrick(vol, t, 1.3)
    want, _ = ac.frame([B], B.lo[None], B.hi[None], IDENT, cam)
    assert (fb[..., 3] > 0).sum() > 100
    assert (fb.view(np.uint32) == want.view(np.uint32)).all()
    mn, mx, wild = ac.ranges(B)
    touched = mx > F(0.5)  # the macro cells whose closed box holds a vertex of S0
    assert touched.sum() == 4 and touched[:2, 0, :2].all()
    info = tr.adapters[0].info()
    assert info["n_blocks_empty"] == 27 - 4 == int(ac.empty_blocks(B, mn, mx, wild).sum())
    assert info["samples_gathered"] < info["samples_marched"]  # ... and the rest is skipped
    plain = VolumeTracer(scenes.VolumeData(vol.data, vol.origin, vol.spacing), cam, t, sampling_rate=1.3).frame()
    assert (plain.framebuffer(False) == 0).all() and plain.adapters[0].info()["n_blocks_empty"] == 27


@pytest.mark.parametrize("kind", ["cool", "spikes"])
@pytest.mark.parametrize("hidden", [np.nan, 0.9])
def test_hidden_level0_vertices_are_never_read(hip, amr_scene, hidden, kind):
    """The level-0 vertices strictly inside S0's footprint, overwritten with NaN and with the value the sparse table makes opaque: no ray
    bit changes, with and without skipping (the macro cells' ranges do change: the covered vertices count for them)."""
    vol = amr_scene
    t = tf(kind)
    rays = all_rays(vol, IDENT)
    data = vol.data.copy()
    lo, cells = np.array(cases.S0["lo"]), np.array(cases.S0["cells"])
    data[lo[2] + 1:lo[2] + cells[2], lo[1] + 1:lo[1] + cells[1], lo[0] + 1:lo[0] + cells[0]] = hidden
    other = scenes.VolumeData(data, vol.origin, vol.spacing, vol.subgrids)
    want = ac.march(ac.AmrBrick(vol, t, 1.3), rays, IDENT)
    for skip in (True, False):
        ad = HipVolumeAdapter(other, sampling_rate=1.3, skip=skip)
        ad.set_transfer(t)
        same_bits(ad.trace(rays, IDENT, IDENT), want)


@pytest.mark.parametrize("which", ["r2", "r8", "nested"])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_exact_refinement_equals_the_plain_volume(hip, axis, which):
    vol = cases.exact_scene(axis, which)
    t = tf("ramp")
    t.value_range = (0.0, 20.0)
    rays = all_rays(vol, IDENT)
    amr = HipVolumeAdapter(vol, sampling_rate=1.3)
    plain = HipVolumeAdapter(scenes.VolumeData(vol.data, vol.origin, vol.spacing), sampling_rate=1.3)
    amr.set_transfer(t)
    plain.set_transfer(t)
    got = amr.trace(rays, IDENT, IDENT)
    same_bits(got, plain.trace(rays, IDENT, IDENT))
    assert (got["w"] > 0).any() and amr.amr_info()["samples_refined"] > 0 and plain.amr_info()["amr_marches"] == 0


def test_bricked_frame_equals_the_one_brick_frame_and_the_checker(hip, amr_scene):
    vol = amr_scene
    t = thin()
    cam = camera()
    one = VolumeTracer(vol, cam, t, sampling_rate=1.3).frame()
    parts = scenes.split_amr_volume(vol, 2, 2, 2, cuts=cases.CUTS)
    eight = VolumeTracer(parts, cam, t, sampling_rate=1.3).frame()
    fb1, fb8 = one.framebuffer(False), eight.framebuffer(False)
    assert (fb1.view(np.uint32) == fb8.view(np.uint32)).all()
    bricks = [ac.AmrBrick(b, t, 1.3) for b in parts]
    rounds = []
    want, calls = ac.frame(bricks, [b.lo for b in parts], [b.hi for b in parts], IDENT, cam, rounds=rounds)
    assert eight.calls == calls > 1 and one.calls == 1
    assert (fb8.view(np.uint32) == want.view(np.uint32)).all() and (fb8[..., 3] > 0).sum() > 300
    st = eight.stats()
    assert st["samples_refined"] > 0 and one.stats()["samples_refined"] > 0
    assert st["amr_marches"] == sum(1 for brick, _ in rounds if parts[brick].subgrids) >= 2  # bricks 0 and 7 hold subgrids
    assert min(n for brick, n in rounds if brick == 0) > 100  # ... and S0's brick gets its share of the rays


def test_clipped_frame_equals_the_checker(hip, amr_scene):
    """A MixedTracer-style frame: every camera ray clipped at a depth plane that cuts through S0."""
    vol = amr_scene
    t = thin()
    cam = camera()
    org, sp = np.asarray(vol.origin, np.float64), np.asarray(vol.spacing, np.float64)
    mid = org + (np.array(cases.S0["lo"]) + 0.5 * np.array(cases.S0["cells"])) * sp  # S0's centre
    normal = np.array([0.3, 0.5, 1.0])
    keep = np.ones((cam.height, cam.width), bool)
    keep[:, ::7] = False  # some rays unclipped
    plane = vcc.depth_of_plane(cam, normal, float(mid @ normal), keep)
    assert np.isfinite(plane).sum() > 1000
    depth = DepthPlane(cam.width, cam.height).upload(plane)
    parts = scenes.split_amr_volume(vol, 2, 2, 2, cuts=cases.CUTS)
    bricks = [ac.AmrBrick(b, t, 1.3) for b in parts]
    want, calls = ac.frame(bricks, [b.lo for b in parts], [b.hi for b in parts], IDENT, cam, plane)
    full, _ = ac.frame(bricks, [b.lo for b in parts], [b.hi for b in parts], IDENT, cam)
    assert (want.view(np.uint32) != full.view(np.uint32)).any()
    for scene_bricks in (vol, parts):
        tr = VolumeTracer(scene_bricks, cam, t, sampling_rate=1.3).frame(depth)
        assert (tr.framebuffer(False).view(np.uint32) == want.view(np.uint32)).all()
        assert tr.stats()["amr_marches"] > 0
    # ... and a host ray that carries the flag, through gvt_hip_volume_trace
    rays = all_rays(vol, IDENT)
    rays["depth"][::2] |= vcc.CLIP
    rays["t_max"][::2] = F(0.9)
    ad = HipVolumeAdapter(vol, sampling_rate=1.3)
    ad.set_transfer(t)
    same_bits(ad.trace(rays, IDENT, IDENT), ac.march(ac.AmrBrick(vol, t, 1.3), rays, IDENT))


def test_volumes_without_subgrids_take_the_plain_path(hip, amr_scene):
    vol = amr_scene
    t = tf("cool")
    rays = all_rays(vol, IDENT)
    plain_vol = scenes.VolumeData(vol.data, vol.origin, vol.spacing)
    want = vc.march(vc.Brick(plain_vol, t, 1.3), rays, IDENT)
    never = HipVolumeAdapter(plain_vol, sampling_rate=1.3)
    never.set_transfer(t)
    same_bits(never.trace(rays, IDENT, IDENT), want)
    assert never.amr_info() == {"n_subgrids": 0, "n_levels": 1, "subgrid_bytes": 0, "samples_refined": 0, "amr_marches": 0}
    empty = HipVolumeAdapter(plain_vol, sampling_rate=1.3)
    empty.set_subgrids([])
    empty.set_transfer(t)
    same_bits(empty.trace(rays, IDENT, IDENT), want)
    assert empty.amr_info()["amr_marches"] == 0
    # subgrids, then none again: the plain volume's bits and ranges are back
    peak = vol.subgrids[3].data.copy()
    peak[4, 4, 4] = 2.0  # a value the level-0 grid does not reach, inside S3
    subs = vol.subgrids[:3] + [scenes.Subgrid(-1, cases.S3["ratio"], vol.subgrids[3].lo, vol.subgrids[3].cells, peak)]
    ad = HipVolumeAdapter(scenes.VolumeData(vol.data, vol.origin, vol.spacing, subs), sampling_rate=1.3)
    ad.set_transfer(t)
    vol_info = ad.info()
    assert not (ad.trace(rays, IDENT, IDENT)["color"].view(np.uint32) == want["color"].view(np.uint32)).all()
    assert ad.amr_info()["amr_marches"] == 1 and ad.amr_info()["n_subgrids"] == 4
    ad.set_subgrids([])
    same_bits(ad.trace(rays, IDENT, IDENT), want)
    back, base = ad.info(), never.info()
    assert ad.amr_info()["amr_marches"] == 1 and ad.amr_info()["n_subgrids"] == 0 and ad.amr_info()["subgrid_bytes"] == 0
    assert (back["value_min"], back["value_max"], back["n_blocks_empty"]) == (base["value_min"], base["value_max"], base["n_blocks_empty"])
    assert vol_info["value_max"] == 2.0 > base["value_max"] and vol_info["value_min"] == base["value_min"]
    ad.set_surfaces([0.5])  # ... and takes surfaces again
    ad.set_surfaces()


def _pod(parent, ratio, lo, cells):
    return capi.SubgridPod(parent, ratio, (C.c_int32 * 3)(*lo), (C.c_int32 * 3)(*cells))


def _raw_set(ad, grids, flags=0, n=None, null_grids=False, null_samples=False, null_entry=None):
    """gvt_hip_volume_set_subgrids with exactly these arguments; samples of the right size, all zero."""
    k = len(grids)
    pods = (capi.SubgridPod * max(k, 1))(*grids)
    keep = [np.zeros(max(1, int(np.prod([max(int(c), 0) * max(int(g.ratio), 0) + 1 for c in g.cells]))), F) for g in grids]
    ptrs = (C.c_void_p * max(k, 1))(*[a.ctypes.data for a in keep])
    if null_entry is not None:
        ptrs[null_entry] = None
    return capi.load().gvt_hip_volume_set_subgrids(ad.h, None if null_grids else C.cast(pods, C.c_void_p), None if null_samples else C.cast(ptrs, C.c_void_p),
                                                   k if n is None else n, flags)


def test_refusals_change_nothing(hip, amr_scene):
    vol = amr_scene
    t = tf("cool")
    rays = all_rays(vol, IDENT)[::7]
    lib = capi.load()
    plain_vol = scenes.VolumeData(vol.data, vol.origin, vol.spacing)
    want_plain = vc.march(vc.Brick(plain_vol, t, 1.3), rays, IDENT)
    want_amr = ac.march(ac.AmrBrick(vol, t, 1.3), rays, IDENT)
    ok = _pod(-1, 2, (3, 2, 1), (6, 5, 9))
    chain = [ok, _pod(0, 2, (0, 0, 0), (2, 2, 2)), _pod(1, 2, (0, 0, 0), (2, 2, 2)), _pod(2, 2, (0, 0, 0), (1, 1, 1))]  # a fifth level
    bad = {
        "null grids": dict(grids=[ok], null_grids=True),
        "null samples": dict(grids=[ok], null_samples=True),
        "null samples entry": dict(grids=[ok, _pod(-1, 2, (12, 2, 1), (2, 2, 2))], null_entry=1),
        "ratio 3": dict(grids=[_pod(-1, 3, (3, 2, 1), (2, 2, 2))]),
        "ratio 16": dict(grids=[_pod(-1, 16, (3, 2, 1), (1, 1, 1))]),
        "ratio 0": dict(grids=[_pod(-1, 0, (3, 2, 1), (1, 1, 1))]),
        "parent is itself": dict(grids=[_pod(0, 2, (0, 0, 0), (1, 1, 1))]),
        "parent is later": dict(grids=[_pod(1, 2, (0, 0, 0), (1, 1, 1)), ok]),
        "parent -2": dict(grids=[_pod(-2, 2, (3, 2, 1), (1, 1, 1))]),
        "no cell": dict(grids=[_pod(-1, 2, (3, 2, 1), (6, 0, 9))]),
        "leaves the brick high": dict(grids=[_pod(-1, 2, (15, 2, 1), (6, 5, 9))]),  # x cells [15, 21) of 20
        "leaves the brick low": dict(grids=[_pod(-1, 2, (-1, 2, 1), (6, 5, 9))]),
        "child leaves its parent": dict(grids=[ok, _pod(0, 4, (10, 1, 3), (3, 3, 4))]),  # x cells [10, 13) of 12
        "siblings overlap": dict(grids=[ok, _pod(-1, 4, (8, 6, 9), (2, 2, 2))]),          # both hold cell (8, 6, 9)
        "children overlap": dict(grids=[ok, _pod(0, 2, (0, 0, 0), (2, 2, 2)), _pod(0, 4, (1, 1, 1), (1, 1, 1))]),
        "five levels": dict(grids=chain),
        "too many": dict(grids=[ok], n=capi.VOLUME_MAX_SUBGRIDS + 1),
        "negative n": dict(grids=[ok], n=-1),
        "unknown flag": dict(grids=[ok], flags=4),
    }
    plain = HipVolumeAdapter(plain_vol, sampling_rate=1.3)
    plain.set_transfer(t)
    amr = HipVolumeAdapter(vol, sampling_rate=1.3)
    amr.set_transfer(t)
    assert _raw_set(plain, chain[:3]) == 0 and plain.amr_info()["n_levels"] == 4  # (four levels are the most, and legal)
    plain.set_subgrids([])
    for why, args in bad.items():
        for ad, want, n_sub in ((plain, want_plain, 0), (amr, want_amr, 4)):
            assert _raw_set(ad, **args) == ERR_INVALID, why
            assert "volume_set_subgrids" in capi.last_error(), why
            assert ad.amr_info()["n_subgrids"] == n_sub, why
            same_bits(ad.trace(rays, IDENT, IDENT), want)
    assert lib.gvt_hip_volume_set_subgrids(None, None, None, 0, 0) == ERR_INVALID
    assert lib.gvt_hip_volume_get_amr_info(plain.h, None) == ERR_INVALID
    # a volume of another voxel type
    u8 = HipVolumeAdapter(scenes.VolumeData(np.rint(vol.data * 255).astype(np.uint8), vol.origin, vol.spacing), sampling_rate=1.3, native=True)
    tu = tf("cool")
    tu.value_range = (0.0, 255.0)
    u8.set_transfer(tu)
    before = u8.trace(rays, IDENT, IDENT)
    assert _raw_set(u8, [ok]) == ERR_INVALID and "voxel type" in capi.last_error()
    same_bits(u8.trace(rays, IDENT, IDENT), before)
    # a volume that has surfaces, or gradient shading
    surf = HipVolumeAdapter(plain_vol, sampling_rate=1.3)
    surf.set_transfer(t)
    surf.set_surfaces([0.5])
    before = surf.trace(rays, IDENT, IDENT)
    assert _raw_set(surf, [ok]) == ERR_INVALID
    same_bits(surf.trace(rays, IDENT, IDENT), before)
    surf.set_surfaces()
    surf.set_shading(True)
    assert _raw_set(surf, [ok]) == ERR_INVALID and surf.amr_info()["n_subgrids"] == 0
    surf.set_shading(False)
    assert _raw_set(surf, [ok]) == 0 and surf.amr_info()["n_subgrids"] == 1
    # conversely, on a volume that has subgrids
    iso = np.array([0.5], F)
    assert lib.gvt_hip_volume_set_surfaces(amr.h, capi.ptr(iso), 1, None, 0, 1.0) == ERR_INVALID
    pl = np.array([0, 0, 1, 0.1], F)
    assert lib.gvt_hip_volume_set_surfaces(amr.h, None, 0, capi.ptr(pl), 1, 1.0) == ERR_INVALID
    assert lib.gvt_hip_volume_set_surfaces(amr.h, None, 0, None, 0, 1.0) == 0  # no surface: nothing to refuse
    assert lib.gvt_hip_volume_set_shading(amr.h, capi.VOLUME_SHADE_GRADIENT) == ERR_INVALID and amr.shading() == capi.VOLUME_SHADE_NONE
    assert lib.gvt_hip_volume_set_shading(amr.h, capi.VOLUME_SHADE_NONE) == 0
    amr.set_lights([((3.0, 4.0, 5.0), (1.0, 1.0, 1.0))])  # lights alone shade nothing
    new = np.ascontiguousarray(vol.data[::-1])
    assert lib.gvt_hip_volume_update_samples(amr.h, capi.ptr(new), C.c_size_t(new.size), 0, None) == ERR_INVALID and "subgrids" in capi.last_error()
    assert lib.gvt_hip_volume_update_samples_typed(amr.h, capi.ptr(new), capi.VOXEL_F32, C.c_size_t(new.size), 0, None) == ERR_INVALID
    same_bits(amr.trace(rays, IDENT, IDENT), want_amr)
    assert amr.crossings() == 0 and amr.shaded() == 0
    # the way to a new time step: subgrids off, update, subgrids on
    amr.set_subgrids([])
    amr.update_samples(new)
    amr.set_subgrids(vol.subgrids)
    step = scenes.VolumeData(new, vol.origin, vol.spacing, vol.subgrids)
    same_bits(amr.trace(rays, IDENT, IDENT), ac.march(ac.AmrBrick(step, t, 1.3), rays, IDENT))
