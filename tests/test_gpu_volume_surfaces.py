"""Isosurfaces and slice planes in the volume march (k_volume_march_surf, csrc/volume.hip) against the numpy checker
(tests/volume_surface_checker.py), bit for bit: gvt_hip_volume_trace with isovalues, planes, lights and opacities, macro-cell skipping
against NO_SKIP, gvt_hip_volume_frame over several brickings, the carried side mask with and without its flag and through a hop of
gvt_hip_shuffle_volume, clearing, set_transfer after set_surfaces, and the argument checks."""
import ctypes as C

import numpy as np
import pytest

from gravit_amd import capi, scenes
from gravit_amd.adapter import HipVolumeAdapter, RayQueue, TopLevel
from gravit_amd.layouts import RAY_DTYPE
from gravit_amd.scheduler import VolumeTracer
from tests import volume_checker as vc
from tests import volume_surface_checker as sc
from tests.test_gpu_volume import IDENT, MOVED, camera, grid, make_rays, tf

pytestmark = pytest.mark.gpu

F = np.float32
FIELDS = ("color", "w", "t_min", "depth", "t")
ISO = [0.42, 0.58]
PLANES = [[0.5, 0.7, -0.4, 0.3], [0.0, 0.0, 1.0, 0.05]]
LIGHTS = [((3.0, 4.0, 5.0), (1.0, 0.9, 0.8)), ((-2.0, 1.0, 0.5), (0.2, 0.3, 0.4)), ((0.0, -6.0, 1.0), (0.5, 0.1, 0.3))]


def same_bits(a, b, fields=FIELDS):
    for f in fields:
        x, y = np.ascontiguousarray(a[f]).view(np.uint32), np.ascontiguousarray(b[f]).view(np.uint32)
        assert (x == y).all(), "%s: %d of %d rays differ" % (f, (x != y).reshape(len(a), -1).any(axis=1).sum(), len(a))


def adapter(vol, t, rate, S, skip=True):
    ad = HipVolumeAdapter(vol, sampling_rate=rate, skip=skip)
    ad.set_transfer(t)
    ad.set_surfaces(S.iso, S.planes, float(S.opacity))
    ad.set_lights(list(zip(S.lpos, S.lcol)), float(S.ka), float(S.kd))
    return ad


@pytest.mark.parametrize("opacity", [1.0, 0.5])
@pytest.mark.parametrize("n_lights", [0, 1, 3])
@pytest.mark.parametrize("kind", ["iso", "planes", "both"])
@pytest.mark.parametrize("moved", [False, True])
def test_trace_equals_the_checker(hip, moved, kind, n_lights, opacity):
    vol = grid()
    m = MOVED if moved else IDENT
    minv = scenes.instance_matrices(m)[0]
    t = tf("ramp")
    S = sc.Surfaces(ISO if kind != "planes" else (), PLANES if kind != "iso" else (), opacity, LIGHTS[:n_lights], ka=0.4, kd=0.6)
    ad = adapter(vol, t, 1.7, S)
    rays = make_rays(vol, m, n=2000)
    rays["t"] = 123.0  # (not a side mask: no flag says so)
    got = ad.trace(rays, m, minv)
    B = vc.Brick(vol, t, 1.7)
    want = sc.march(B, S, rays, minv)
    assert len(got) == len(rays)
    same_bits(got, want)
    assert sc.march.crossings > 100 and ad.crossings() == sc.march.crossings
    marched = (got["depth"] & sc.SIDES) != 0
    assert marched.any() and not marched.all() and (got["t"][~marched] == 123.0).all()
    plain = HipVolumeAdapter(vol, sampling_rate=1.7)
    plain.set_transfer(t)
    assert (plain.trace(rays, m, minv)["color"] != got["color"]).any()  # the surfaces show
    # the marched rays again: nothing is left to own, the state stays
    same_bits(ad.trace(got, m, minv), sc.march(B, S, want, minv))


def test_skipping_gives_the_same_bits(hip):
    vol = grid(40)
    t = tf("spikes")
    S = sc.Surfaces([0.05, 0.93], PLANES[:1], 0.5, LIGHTS[:2])
    a, b = adapter(vol, t, 1.0, S, skip=True), adapter(vol, t, 1.0, S, skip=False)
    rays = make_rays(vol, IDENT, n=4000, seed=11)
    ra, rb = a.trace(rays, IDENT, IDENT), b.trace(rays, IDENT, IDENT)
    same_bits(ra, rb)
    same_bits(ra, sc.march(vc.Brick(vol, t, 1.0), S, rays, IDENT))
    ia, ib = a.info(), b.info()
    assert ia["samples_marched"] == ib["samples_marched"] > 0
    assert ia["samples_gathered"] < ib["samples_gathered"] == ib["samples_marched"]
    assert a.crossings() == b.crossings() == sc.march.crossings > 100
    # planes only: every empty macro cell may be skipped except where a plane passes
    S2 = sc.Surfaces((), PLANES, 1.0, LIGHTS[:1])
    a2, b2 = adapter(vol, t, 1.0, S2, skip=True), adapter(vol, t, 1.0, S2, skip=False)
    r2 = a2.trace(rays, IDENT, IDENT)
    same_bits(r2, b2.trace(rays, IDENT, IDENT))
    same_bits(r2, sc.march(vc.Brick(vol, t, 1.0), S2, rays, IDENT))
    assert a2.info()["samples_gathered"] < b2.info()["samples_gathered"]


@pytest.fixture(scope="module")
def frame_case(hip):
    vol = grid(33)
    cam = camera(160, 128)
    t = tf("ramp")
    S = sc.Surfaces(ISO, PLANES[:1], 0.5, LIGHTS)
    B = vc.Brick(vol, t, 1.5)
    want, calls = sc.frame([B], B.lo[None], B.hi[None], IDENT, cam, S)
    return vol, cam, t, S, want


@pytest.mark.parametrize("split", [(1, 1, 1), (2, 2, 2), (3, 1, 2)])
def test_frames_equal_the_checker_whatever_the_bricking(frame_case, split):
    vol, cam, t, S, want = frame_case
    parts = vol if split == (1, 1, 1) else scenes.split_volume(vol, *split)
    tr = VolumeTracer(parts, cam, t, sampling_rate=1.5)
    tr.set_surfaces(S.iso, S.planes, float(S.opacity)).set_lights(list(zip(S.lpos, S.lcol)))
    got = tr.frame().framebuffer(False)
    assert tr.calls >= int(np.prod(split)) and tr.stats()["crossings_rendered"] > 1000
    assert (got[..., 3] > 0).sum() > 2000
    assert (got.view(np.uint32) == want.view(np.uint32)).all()


def test_moved_bricked_frame_equals_the_checker(hip):
    vol = grid(25)
    cam = camera(96, 80)
    t = tf("cool")
    S = sc.Surfaces(ISO[:1], PLANES[1:], 1.0, LIGHTS[:1])
    parts = scenes.split_volume(vol, 2, 1, 2)
    tr = VolumeTracer(parts, cam, t, m=MOVED, sampling_rate=2.0)
    tr.set_surfaces(S.iso, S.planes, 1.0).set_lights(list(zip(S.lpos, S.lcol)))
    minv = scenes.instance_matrices(MOVED)[0]
    bricks = [vc.Brick(b, t, 2.0) for b in parts]
    want, calls = sc.frame(bricks, tr.inst_lo, tr.inst_hi, minv, cam, S)
    assert tr.frame().calls == calls
    assert (tr.framebuffer(False).view(np.uint32) == want.view(np.uint32)).all()


def inside_rays(vol, n=1500, seed=3):
    """Rays that start inside the grid: sample 1, the first after t_min, is the brick's first owned sample."""
    rng = np.random.default_rng(seed)
    lo = vol.origin
    ext = ((vol.counts - 1).astype(F) * vol.spacing).astype(F)
    r = np.zeros(n, RAY_DTYPE)
    r["origin"] = (lo + ext * (0.2 + 0.6 * rng.random((n, 3)))).astype(F)
    d = rng.standard_normal((n, 3))
    r["direction"] = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)
    r["t_min"] = F(1e-6)
    r["t_max"] = np.finfo(F).max
    r["id"] = np.arange(n)
    return r


def test_the_carried_sides_count_only_with_the_flag(hip):
    vol = grid()
    t = tf("ramp")
    S = sc.Surfaces(ISO, PLANES[:1], 0.5, LIGHTS[:1])
    ad = adapter(vol, t, 1.0, S)
    B = vc.Brick(vol, t, 1.0)
    rays = inside_rays(vol)
    rays["t"] = np.arange(len(rays)) % 8  # some mask of the three surfaces
    bare = ad.trace(rays, IDENT, IDENT)
    same_bits(bare, sc.march(B, S, rays, IDENT))
    flagged = rays.copy()
    flagged["depth"] |= sc.SIDES
    got = ad.trace(flagged, IDENT, IDENT)
    same_bits(got, sc.march(B, S, flagged, IDENT))
    assert (got["color"] != bare["color"]).any(axis=1).sum() > 100  # the first sample saw a previous one
    # the flag with a t_min whose next sample is not the first owned one (the ray starts outside): nothing carried
    far = make_rays(vol, IDENT, n=600)[:120]
    far["t"] = 7.0
    far["depth"] |= sc.SIDES
    off = far.copy()
    off["depth"] &= ~sc.SIDES
    a, b = ad.trace(far, IDENT, IDENT), ad.trace(off, IDENT, IDENT)
    same_bits(a, sc.march(B, S, far, IDENT))
    own = (b["depth"] & sc.SIDES) != 0
    assert own.sum() > 50
    same_bits(a[own], b[own])


def test_a_hop_through_the_shuffle_keeps_field_and_flag(hip):
    vol = grid()
    t = tf("ramp")
    S = sc.Surfaces(ISO, PLANES[:1], 0.5, LIGHTS[:2])
    parts = scenes.split_volume(vol, 2, 1, 1)
    ads = [adapter(p, t, 1.0, S) for p in parts]
    bricks = [vc.Brick(p, t, 1.0) for p in parts]
    lo, hi = np.array([p.lo for p in parts], F), np.array([p.hi for p in parts], F)
    rays = make_rays(vol, IDENT, n=3000)
    first = ads[0].trace(rays, IDENT, IDENT)
    want_first = sc.march(bricks[0], S, rays, IDENT)
    same_bits(first, want_first)
    top = TopLevel(lo, hi)
    q_in, queues = RayQueue(), [RayQueue(), RayQueue()]
    q_in.append(first, keep_state=True)
    arr = (C.c_void_p * 2)(*[q.h for q in queues])
    capi.check(capi.load().gvt_hip_shuffle_volume(top.h, q_in.h, 0, arr, None), "gvt_hip_shuffle_volume")
    hopped = queues[1].to_numpy()
    wq = [[], []]
    vc.shuffle(lo, hi, list(top.order()), want_first, 0, wq, np.zeros((len(rays), 4), F))
    want_hop = np.concatenate(wq[1])
    assert len(hopped) == len(want_hop) > 200 and (hopped["id"] == want_hop["id"]).all()
    same_bits(hopped, want_hop)
    src = first[hopped["id"]]
    assert ((hopped["depth"] & sc.SIDES) == (src["depth"] & sc.SIDES)).all() and ((hopped["depth"] & sc.SIDES) != 0).any()
    assert (hopped["t"].view(np.uint32) == src["t"].view(np.uint32)).all()
    second = ads[1].trace(hopped, IDENT, IDENT)
    same_bits(second, sc.march(bricks[1], S, want_hop, IDENT))
    # ... and the two bricks together render what the whole grid renders for those rays
    whole = sc.march(vc.Brick(vol, t, 1.0), S, rays, IDENT)[hopped["id"]]
    same_bits(second, whole, ("color", "w", "t_min", "t"))


def test_cleared_surfaces_and_a_new_transfer_function(hip):
    vol = grid()
    t = tf("spikes")
    S = sc.Surfaces(ISO, PLANES[:1], 1.0, LIGHTS[:1])
    ad = adapter(vol, t, 1.3, S)
    rays = make_rays(vol, IDENT, n=1500)
    rays["t"] = 5.0
    B = vc.Brick(vol, t, 1.3)
    same_bits(ad.trace(rays, IDENT, IDENT), sc.march(B, S, rays, IDENT))
    t2 = tf("ramp")  # set_transfer after set_surfaces: the colours, the opacities and the cells that may be skipped all change
    ad.set_transfer(t2)
    same_bits(ad.trace(rays, IDENT, IDENT), sc.march(vc.Brick(vol, t2, 1.3), S, rays, IDENT))
    ad.set_transfer(t)
    same_bits(ad.trace(rays, IDENT, IDENT), sc.march(B, S, rays, IDENT))
    ad.set_surfaces()  # cleared: the plain march, which neither reads nor writes the side mask
    got = ad.trace(rays, IDENT, IDENT)
    same_bits(got, vc.march(B, rays, IDENT))
    assert ((got["depth"] & sc.SIDES) == 0).all() and (got["t"] == 5.0).all()
    n0 = ad.crossings()
    ad.trace(rays, IDENT, IDENT)
    assert ad.crossings() == n0 > 0


def test_invalid_arguments_are_refused(hip):
    vol = grid(12)
    t = tf("ramp")
    S = sc.Surfaces(ISO[:1], (), 1.0)
    ad = adapter(vol, t, 1.0, S)
    rays = make_rays(vol, IDENT, n=500)
    want = sc.march(vc.Brick(vol, t, 1.0), S, rays, IDENT)
    lib = capi.load()

    def surf(iso, planes, opacity):
        i, p = capi.f32(iso, -1), capi.f32(planes, -1)
        return lib.gvt_hip_volume_set_surfaces(ad.h, capi.ptr(i), len(i), capi.ptr(p), len(p) // 4, opacity)

    assert surf([np.nan], [], 1.0) == -1 and "NaN" in capi.last_error()
    assert surf([0.5], [0, 0, 0, 1], 1.0) == -1 and "plane" in capi.last_error()
    assert surf([0.5], [], 0.0) == -1 and "opacity" in capi.last_error()
    assert surf([0.5], [], 1.5) == -1
    assert surf([0.5], [], float("nan")) == -1
    assert surf(np.linspace(0.1, 0.9, 17), [], 1.0) == -1 and "at most" in capi.last_error()
    assert surf(np.linspace(0.1, 0.9, 10), np.tile([1.0, 0, 0, 0.5], 7), 1.0) == -1
    assert lib.gvt_hip_volume_set_surfaces(ad.h, None, 1, None, 0, 1.0) == -1
    same_bits(ad.trace(rays, IDENT, IDENT), want)  # every refusal left the volume as it was
    pos, col = capi.f32(np.ones((9, 3))), capi.f32(np.ones((9, 3)))
    assert lib.gvt_hip_volume_set_lights(ad.h, capi.ptr(pos), capi.ptr(col), 9, 0.4, 0.6) == -1 and "at most" in capi.last_error()
    assert lib.gvt_hip_volume_set_lights(ad.h, None, None, 1, 0.4, 0.6) == -1
    bad = pos.copy()
    bad[0, 1] = np.inf
    assert lib.gvt_hip_volume_set_lights(ad.h, capi.ptr(bad), capi.ptr(col), 2, 0.4, 0.6) == -1
    same_bits(ad.trace(rays, IDENT, IDENT), want)
    assert surf(np.linspace(0.1, 0.9, 9), np.tile([1.0, 0, 0, 0.5], 7), 1.0) == 0  # 16 in all
    assert lib.gvt_hip_volume_set_lights(ad.h, capi.ptr(pos), capi.ptr(col), 8, 0.4, 0.6) == 0
    assert lib.gvt_hip_volume_get_crossings(ad.h, None) == -1
