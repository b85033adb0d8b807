"""Time-varying AMR volumes on the device (gvt_hip_volume_update_amr; k_amr_ranges_merge in csrc/volume_amr.inc): after an update in
place the volume answers like a volume freshly created from the resident samples, bit for bit -- against such a volume and against the
numpy checkers -- for whole and partial steps, designed fields only the merged ranges of the new step keep exact, non-finite samples,
device tensors, shaded AMR volumes, bricked loop / fused / shadowed frames, and every refusal."""
import ctypes as C
import math

import numpy as np
import pytest
import torch  # (before the library initialises the device, as in test_gpu_volume_update.py)

from gravit_amd import capi, scenes
from gravit_amd.adapter import HipVolumeAdapter
from gravit_amd.scheduler import MixedTracer, VolumeTracer
from tests import volume_amr_cases as cases
from tests import volume_amr_checker as ac
from tests import volume_amr_surface_cases as scases
from tests import volume_amr_update_cases as uc
from tests import volume_checker as vc
from tests import volume_fused_amr_cases as fc
from tests import volume_shadow_amr_cases as sac
from tests.test_gpu_volume import IDENT, same_bits, tf
from tests.test_gpu_volume_amr import all_rays
from tests.test_gpu_volume_amr_surfaces import FIELDS, clear, shaded_adapter
from tests.test_gpu_volume_amr_surfaces import all_rays as surface_rays
from tests.test_gpu_volume_amr_surfaces import same_bits as same_bits_t
from tests.test_gpu_volume_shadow_amr import FRAMES, _raw_frame, bits, tracer

pytestmark = pytest.mark.gpu

F = np.float32
ERR_INVALID = -1
RATE = uc.RATE
KEPT = ("n_subgrids", "n_levels", "subgrid_bytes")


def adapter(vol, t, skip=True):
    ad = HipVolumeAdapter(vol, sampling_rate=RATE, skip=skip)
    if t is not None:
        ad.set_transfer(t)
    return ad


def same_info(got, want):
    """value_min / value_max as numbers, n_blocks and n_blocks_empty."""
    for key in ("value_min", "value_max", "n_blocks", "n_blocks_empty"):
        assert got[key] == want[key], (key, got[key], want[key])


def mixed(level0, subgrids):
    """The volume of `level0`'s level-0 samples and `subgrids` (a list of Subgrid of the same tree)."""
    return scenes.VolumeData(level0.data, level0.origin, level0.spacing, list(subgrids))


@pytest.fixture(scope="module")
def rays():
    return all_rays(uc.step(0), IDENT)


@pytest.fixture(scope="module")
def checked(rays):
    """The checker's march and info of both steps under the sparse table: computed once, read-only."""
    out = []
    for k in (0, 1):
        B = ac.AmrBrick(uc.step(k), tf("spikes"), RATE)
        out.append((ac.march(B, rays, IDENT), ac.info(B)))
    return out


@pytest.mark.parametrize("skip", [True, False])
def test_a_step_in_place_equals_a_fresh_volume_and_the_checker(hip, rays, checked, skip):
    a, b = uc.step(0), uc.step(1)
    t = tf("spikes")
    ad = adapter(a, t, skip)
    same_bits(ad.trace(rays, IDENT, IDENT), checked[0][0])
    kept = ad.amr_info()
    ms = ad.update_amr(b.data, b.subgrids)
    assert math.isfinite(ms) and ms > 0
    fresh = adapter(b, t, skip)
    got = ad.trace(rays, IDENT, IDENT)
    same_bits(got, fresh.trace(rays, IDENT, IDENT))
    same_bits(got, checked[1][0])
    assert not (got["color"].view(np.uint32) == checked[0][0]["color"].view(np.uint32)).all()
    same_info(ad.info(), fresh.info())
    same_info(ad.info(), checked[1][1])
    amr = ad.amr_info()
    assert all(amr[k] == kept[k] == fresh.amr_info()[k] for k in KEPT) and amr["amr_marches"] == 2  # the counters go on
    assert ad.info()["samples_marched"] > fresh.info()["samples_marched"]
    assert ad.update_amr(a.data, a.subgrids) > 0  # ... and back
    same_bits(ad.trace(rays, IDENT, IDENT), checked[0][0])
    same_info(ad.info(), checked[0][1])


@pytest.mark.parametrize("which", sorted(uc.DESIGNED))
def test_designed_fields_only_the_new_subgrid_samples_open_the_cells(hip, which):
    a, b = uc.designed(which)
    d = uc.DESIGNED[which]
    t = uc.half()
    aimed = np.concatenate([uc.aimed_rays(a, uc.vertex_position(a, d["subgrid"], d["vertex"])), all_rays(a, IDENT)[::4]])
    skipping, gathering = adapter(a, t, True), adapter(a, t, False)
    want_empty = {id(v): ac.info(ac.AmrBrick(v, t, RATE))["n_blocks_empty"] for v in (a, b)}
    assert want_empty[id(a)] == 27 and want_empty[id(b)] == 27 - len(d["cells"])
    assert skipping.info()["n_blocks_empty"] == 27
    for vol in (b, a, b):  # both directions
        for ad in (skipping, gathering):
            ad.update_amr(subgrids=[s if i == d["subgrid"] else None for i, s in enumerate(vol.subgrids)])
            assert ad.info()["n_blocks_empty"] == want_empty[id(vol)]
        got = skipping.trace(aimed, IDENT, IDENT)
        same_bits(got, gathering.trace(aimed, IDENT, IDENT))
        assert (got["w"] > 0).any() == (vol is b)
    same_bits(got, ac.march(ac.AmrBrick(b, t, RATE), aimed, IDENT))


@pytest.mark.parametrize("part", ["level 0", "S1", "subgrids"])
def test_partial_updates_equal_the_fresh_volume_of_the_mixed_samples(hip, rays, part):
    a, b = uc.step(0), uc.step(1)
    t = tf("cool")
    ad = adapter(a, t)
    if part == "level 0":
        ad.update_amr(b.data)
        now = mixed(b, a.subgrids)
    elif part == "S1":  # the nested child alone
        ad.update_amr(subgrids=[None, b.subgrids[1].data, None, None])
        now = mixed(a, [a.subgrids[0], b.subgrids[1], a.subgrids[2], a.subgrids[3]])
    else:  # samples = NULL
        ad.update_amr(None, b.subgrids)
        now = mixed(a, b.subgrids)
    fresh = adapter(now, t)
    got = ad.trace(rays, IDENT, IDENT)
    same_bits(got, fresh.trace(rays, IDENT, IDENT))
    same_info(ad.info(), fresh.info())
    same_info(ad.info(), ac.info(ac.AmrBrick(now, t, RATE)))
    assert not (got["color"].view(np.uint32) == adapter(a, t).trace(rays, IDENT, IDENT)["color"].view(np.uint32)).all()


@pytest.mark.parametrize("kind", uc.NONFINITE)
def test_non_finite_new_samples_keep_skipping_exact(hip, rays, kind):
    a, b = uc.step(0), uc.nonfinite(kind)
    t = tf("spikes")
    skipping, gathering = adapter(a, t, True), adapter(a, t, False)
    for ad in (skipping, gathering):
        ad.update_amr(b.data, b.subgrids)
    got = skipping.trace(rays, IDENT, IDENT)
    same_bits(got, gathering.trace(rays, IDENT, IDENT))
    fresh = adapter(b, t, True)
    same_bits(got, fresh.trace(rays, IDENT, IDENT))
    same_info(skipping.info(), fresh.info())
    same_info(skipping.info(), ac.info(ac.AmrBrick(b, t, RATE)))
    if kind != "nan":
        assert skipping.info()["value_max"] == np.inf


def test_device_tensors_give_the_host_paths_bits(hip, rays, checked):
    a, b = uc.step(0), uc.step(1)
    t = tf("spikes")
    ad = adapter(a, t)
    subs = [scenes.Subgrid(s.parent, s.ratio, s.lo, s.cells, torch.from_numpy(s.data).cuda()) for s in b.subgrids]
    assert ad.update_amr(torch.from_numpy(b.data).cuda(), subs) > 0
    same_bits(ad.trace(rays, IDENT, IDENT), checked[1][0])
    same_info(ad.info(), checked[1][1])
    ad.update_amr(subgrids=[None, torch.from_numpy(a.subgrids[1].data).cuda(), None, None])  # one tensor, no Subgrid around it
    same_bits(ad.trace(rays, IDENT, IDENT), adapter(mixed(b, [b.subgrids[0], a.subgrids[1], b.subgrids[2], b.subgrids[3]]), t).trace(rays, IDENT, IDENT))
    with pytest.raises(ValueError, match="all host arrays or all GPU tensors"):
        ad.update_amr(a.data, subs)
    with pytest.raises(ValueError, match="shape"):
        ad.update_amr(subgrids=[None, a.subgrids[0].data, None, None])
    with pytest.raises(ValueError, match="shape"):
        ad.update_amr(a.data[1:])
    with pytest.raises(ValueError, match="4"):
        ad.update_amr(subgrids=a.subgrids[:3])
    with pytest.raises(ValueError, match="ratio"):
        ad.update_amr(subgrids=uc.changed_trees(a)["ratio"])
    with pytest.raises(ValueError, match="nothing"):
        ad.update_amr(subgrids=[None] * 4)
    with pytest.raises(ValueError, match="no subgrids"):
        adapter(scenes.VolumeData(a.data, a.origin, a.spacing), t).update_amr(a.data)


@pytest.mark.parametrize("table", ["clear", "thin"])
def test_shaded_amr_volume_an_isovalue_only_the_new_subgrid_data_crosses(hip, table):
    """A = cases.scene(), B = its S0 with a block at PEAK; the isovalue lies above everything else.  clear: the table is empty everywhere,
    so only surface skip words rebuilt from the MERGED ranges of B render the crossings; thin: lit fog around them."""
    a, b = cases.scene(), scases.peak_scene()
    t = clear() if table == "clear" else fc.thin()
    S = scases.surfaces(a, isovalues=(scases.PEAK_ISO,), plane=False)
    rays = surface_rays(a, IDENT)
    step = [b.subgrids[0], None, None, None]
    fresh = shaded_adapter(b, t, S, True, True, skip=True)
    want = fresh.trace(rays, IDENT, IDENT)
    assert fresh.crossings() > 0
    for skip in (True, False):
        ad = shaded_adapter(a, t, S, True, True, skip=skip)
        first = ad.trace(rays, IDENT, IDENT)
        assert ad.crossings() == 0  # nothing of A reaches the isovalue
        kept = ad.amr_info()
        ad.update_amr(subgrids=step)
        same_bits_t(ad.trace(rays, IDENT, IDENT), want, FIELDS)
        assert ad.crossings() == fresh.crossings() and all(ad.amr_info()[k] == kept[k] for k in KEPT)
        same_info(ad.info(), fresh.info())
        ad.update_amr(subgrids=[a.subgrids[0], None, None, None])
        same_bits_t(ad.trace(rays, IDENT, IDENT), first, FIELDS)
        assert ad.crossings() == fresh.crossings()  # ... and none again


def test_bricked_tracers_update_in_place_loop_and_fused(hip):
    """B -> A under the 2 x 2 x 2 bricking: the checker's frame of A (the fused AMR tests' reference) is what every path must give."""
    a, b = uc.step(0), uc.step(1)
    cam, t = fc.camera("outside"), fc.thin()
    parts_a, parts_b = fc.parts_of(a, 8), fc.parts_of(b, 8)
    want = fc.reference("plain", 8, "outside")[0]
    loop = VolumeTracer(parts_b, cam, t, sampling_rate=RATE).frame()
    fused = VolumeTracer(parts_b, cam, t, sampling_rate=RATE, fused=True, fused_amr=True).frame()
    one_b = VolumeTracer(b, cam, t, sampling_rate=RATE).frame().framebuffer(False)
    assert (bits(loop.framebuffer(False)) == bits(one_b)).all() and (bits(fused.framebuffer(False)) == bits(one_b)).all()
    assert (bits(one_b) != bits(want)).any()
    kept = [ad.amr_info() for ad in loop.adapters]
    for tr in (loop, fused):  # the same tracer objects before and after: tops, queues and the fused frame's tables held
        assert tr.update(parts_a, amr=True) is tr
        got = tr.frame().framebuffer(False)
        assert (bits(got) == bits(want)).all()
    assert fused.fused_stats["fused"] == 1 and fused.fused_stats["amr_bricks"] == 2
    assert [{k: ad.amr_info()[k] for k in KEPT} for ad in loop.adapters] == [{k: i[k] for k in KEPT} for i in kept]
    assert (bits(VolumeTracer(parts_a, cam, t, sampling_rate=RATE).frame().framebuffer(False)) == bits(want)).all()  # a fresh tracer
    assert (bits(VolumeTracer(a, cam, t, sampling_rate=RATE).frame().framebuffer(False)) == bits(want)).all()  # the one-brick frame
    # one changed tree: ValueError before the first brick changes
    bad = list(parts_b)
    bad[7] = scenes.Brick(**{**parts_b[7].__dict__, "subgrids": []})
    with pytest.raises(ValueError, match="brick 7"):
        loop.update(bad, amr=True)
    assert (bits(loop.frame().framebuffer(False)) == bits(want)).all()
    # without the keyword the library refuses a brick that has subgrids, as ever
    with pytest.raises(capi.GvtHipError):
        loop.update(parts_b)


def test_shadowed_tracer_the_light_grid_goes_stale_and_is_baked_again(hip):
    a, b = uc.step(0), uc.step(1)
    want = sac.reference("fog", "surf_lit", 8, "outside")[0]
    tr = tracer("fog", "surf_lit", 8, parts=fc.parts_of(b, 8)).frame()
    assert tr.light_bakes == 1 and all(ad.light_grid_info()["current"] for ad in tr.adapters)
    assert (bits(tr.framebuffer(False)) != bits(want)).any()
    tr.update(fc.parts_of(a, 8), amr=True)
    assert not any(ad.light_grid_info()["current"] for ad in tr.adapters)
    assert _raw_frame(tr, FRAMES[1], capi.VOLUME_ALLOW_AMR) == ERR_INVALID  # the raw frame call is refused: a stale grid
    assert tr.frame().light_bakes == 2
    got = tr.framebuffer(False)
    assert (bits(got) == bits(want)).all()
    assert (bits(got) == bits(tracer("fog", "surf_lit", 8).frame().framebuffer(False))).all()  # a fresh tracer of A


def test_mesh_shadowed_tracer_the_occluder_grid_stays_current(hip):
    a, b = uc.step(0), uc.step(1)
    mt = tracer("mesh", "surf_lit", 8, parts=fc.parts_of(b, 8), cls=MixedTracer, scene=sac.mesh_scene()).frame()
    assert mt.volume.occluder_bakes == 1 and all(ad.occluder_grid_info()["current"] for ad in mt.volume.adapters)
    mt.update(fc.parts_of(a, 8), amr=True)
    assert all(ad.occluder_grid_info()["current"] for ad in mt.volume.adapters)
    assert not any(ad.light_grid_info()["current"] for ad in mt.volume.adapters)
    mt.frame()
    assert mt.volume.occluder_bakes == 1 and mt.volume.light_bakes == 2
    fresh = tracer("mesh", "surf_lit", 8, cls=MixedTracer, scene=sac.mesh_scene()).frame()
    assert (bits(mt.framebuffer(False)) == bits(fresh.framebuffer(False))).all() and mt.framebuffer(False).any()


def test_removing_the_subgrids_after_an_update_gives_the_plain_volume_of_the_new_level0(hip, rays):
    a, b = uc.step(0), uc.step(1)
    t = tf("cool")
    ad = adapter(a, t)
    ad.update_amr(b.data, b.subgrids)
    ad.set_subgrids([])
    plain = scenes.VolumeData(b.data, b.origin, b.spacing)
    same_bits(ad.trace(rays, IDENT, IDENT), vc.march(vc.Brick(plain, t, RATE), rays, IDENT))
    same_info(ad.info(), adapter(plain, t).info())
    assert ad.amr_info()["n_subgrids"] == 0 and ad.amr_info()["subgrid_bytes"] == 0
    assert ad.update_samples(a.data) > 0  # a plain volume again: _update_samples is its call
    ad.set_subgrids(a.subgrids)  # ... and the tree may come back, and be updated (its merge tables are built anew)
    ad.update_amr(subgrids=b.subgrids)
    same_bits(ad.trace(rays, IDENT, IDENT), adapter(mixed(a, b.subgrids), t).trace(rays, IDENT, IDENT))


def _raw_update(ad, samples=None, n_samples=None, subs=None, n_subs=None, flags=0, null_volume=False):
    """gvt_hip_volume_update_amr with exactly these arguments (subs: a list of arrays or None entries)."""
    keep = [None if s is None else np.ascontiguousarray(s, F) for s in (subs or [])]
    ptrs = (C.c_void_p * max(1, len(keep)))(*[None if k is None else k.ctypes.data for k in keep])
    src = None if samples is None else np.ascontiguousarray(samples, F)
    return capi.load().gvt_hip_volume_update_amr(None if null_volume else ad.h, None if src is None else capi.ptr(src),
                                                 C.c_size_t((0 if src is None else src.size) if n_samples is None else n_samples),
                                                 None if subs is None else C.cast(ptrs, C.c_void_p), (len(keep) if n_subs is None else n_subs), C.c_uint32(flags), None)


def test_refusals_change_nothing(hip, rays):
    a, b = uc.step(0), uc.step(1)
    t = tf("cool")
    rays = rays[::5]
    amr, plain = adapter(a, t), adapter(scenes.VolumeData(a.data, a.origin, a.spacing), t)
    before, before_plain = amr.trace(rays, IDENT, IDENT), plain.trace(rays, IDENT, IDENT)
    info = amr.info()
    new = [s.data for s in b.subgrids]
    bad = {
        "null volume": dict(samples=b.data, null_volume=True),
        "another n_samples": dict(samples=b.data, n_samples=b.data.size - 1),
        "null samples with a count": dict(n_samples=b.data.size, subs=new),
        "fewer subgrids": dict(subs=new[:3]),
        "more subgrids": dict(subs=new + [new[0]]),
        "null subgrids with a count": dict(samples=b.data, n_subs=4),
        "negative count": dict(samples=b.data, subs=new, n_subs=-1),
        "nothing given": dict(),
        "nothing given, every entry null": dict(subs=[None] * 4),
        "unknown flag": dict(samples=b.data, subs=new, flags=2),
        "unknown flag beside the known one": dict(samples=b.data, subs=new, flags=5),
    }
    for why, args in bad.items():
        assert _raw_update(amr, **args) == ERR_INVALID, why
        assert "volume_update_amr" in capi.last_error(), why
        same_bits(amr.trace(rays, IDENT, IDENT), before)
        same_info(amr.info(), info)
        assert amr.amr_info()["n_subgrids"] == 4
    assert _raw_update(plain, samples=b.data) == ERR_INVALID and "update_samples" in capi.last_error()  # a volume without subgrids: the message names its call
    same_bits(plain.trace(rays, IDENT, IDENT), before_plain)
    # _update_samples[_typed] go on refusing the AMR volume
    assert capi.load().gvt_hip_volume_update_samples(amr.h, capi.ptr(b.data), C.c_size_t(b.data.size), 0, None) == ERR_INVALID and "subgrids" in capi.last_error()
    same_bits(amr.trace(rays, IDENT, IDENT), before)
    assert _raw_update(amr, samples=b.data, subs=new) == 0  # ... and the call the refusals were variations of is accepted
    same_bits(amr.trace(rays, IDENT, IDENT), adapter(b, t).trace(rays, IDENT, IDENT))


def test_update_before_any_transfer_function(hip, rays, checked):
    a, b = uc.step(0), uc.step(1)
    ad = adapter(a, None)
    assert ad.update_amr(b.data, b.subgrids) > 0
    ad.set_transfer(tf("spikes"))
    same_bits(ad.trace(rays, IDENT, IDENT), checked[1][0])
    same_info(ad.info(), checked[1][1])
