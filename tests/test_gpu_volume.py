"""Volume domains on the device (csrc/volume.hip) against the numpy checker (tests/volume_checker.py), bit for bit: k_volume_march through
gvt_hip_volume_trace, macro-cell skipping, early termination, the volume shuffle and gvt_hip_volume_frame over several brickings, and the
argument checks."""
import ctypes as C
import os

import numpy as np
import pytest

from gravit_amd import capi, scenes
from gravit_amd.adapter import HipVolumeAdapter, TransferFunction
from gravit_amd.layouts import RAY_DTYPE
from gravit_amd.scheduler import VolumeTracer
from tests import volume_checker as vc
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu

F = np.float32
from tests.volume_common import CMAPS, IDENT, MOVED, grid, read, tf  # noqa: E402,F401  (shared with the host tests; other test modules import them from here)


def make_rays(vol, m, n=3000, seed=7):
    """Rays in world space: from outside towards the box, from inside, grazing a face, parallel to an axis, and missing."""
    rng = np.random.default_rng(seed)
    lo = vol.origin
    hi = (vol.origin + (vol.counts - 1).astype(F) * vol.spacing).astype(F)
    M = m.reshape(4, 4).T
    w = lambda p: (p @ M[:3, :3].T + M[:3, 3]).astype(F)  # noqa: E731
    ext = hi - lo
    k = n // 5
    tgt = lo + ext * rng.random((n, 3))
    org = np.zeros((n, 3), F)
    org[:k] = lo - 0.6 * ext + 2.2 * ext * rng.random((k, 3))                    # outside, aimed in
    org[:k, 2] = hi[2] + 0.7
    org[k:2 * k] = lo + ext * rng.random((k, 3))                                 # inside
    d = tgt - org
    g0, g1 = 2 * k, 3 * k                                                        # grazing the face x = lo.x
    org[g0:g1] = lo + ext * rng.random((k, 3))
    org[g0:g1, 0] = lo[0]
    org[g0:g1, 2] = hi[2] + 0.5
    d[g0:g1] = tgt[g0:g1] - org[g0:g1]
    d[g0:g1, 0] = 0
    a0, a1 = 3 * k, 4 * k                                                        # parallel to an axis
    org[a0:a1] = lo + ext * rng.random((k, 3))
    ax = rng.integers(0, 3, k)
    org[a0 + np.arange(k), ax] = lo[ax] - 0.3
    d[a0:a1] = 0
    d[a0 + np.arange(k), ax] = 1
    org[a1:] = hi + 0.5 + rng.random((n - a1, 3))                                # missing: pointing away
    d[a1:] = rng.random((n - a1, 3)) + 0.1
    r = np.zeros(n, RAY_DTYPE)
    r["origin"] = w(org)
    r["direction"] = (d @ M[:3, :3].T).astype(F)
    r["t_min"] = F(1e-6)
    r["t_max"] = np.finfo(F).max
    r["id"] = np.arange(n)
    r["w"] = 0
    r["depth"] = rng.integers(0, 2, n) * 0x1  # unrelated low bits survive
    return r


def same_bits(a, b, fields=("color", "w", "t_min", "depth")):
    for f in fields:
        assert (np.ascontiguousarray(a[f]).view(np.uint32) == np.ascontiguousarray(b[f]).view(np.uint32)).all(), f


@pytest.mark.parametrize("kind", ["cool", "spikes", "ramp"])
@pytest.mark.parametrize("moved", [False, True])
def test_march_equals_the_checker(hip, kind, moved):
    vol = grid()
    m = MOVED if moved else IDENT
    minv = scenes.instance_matrices(m)[0]
    t = tf(kind)
    ad = HipVolumeAdapter(vol, sampling_rate=1.7)
    ad.set_transfer(t)
    rays = make_rays(vol, m)
    got = ad.trace(rays, m, minv)
    want = vc.march(vc.Brick(vol, t, 1.7), rays, minv)
    assert len(got) == len(rays)
    same_bits(got, want)
    flags = got["depth"] & (vc.OPAQUE | vc.BOUNDARY)
    assert ((flags == vc.OPAQUE) | (flags == vc.BOUNDARY)).all()
    if kind != "spikes":  # (the sparse table may leave every ray of this small grid transparent)
        assert (got["w"][:600] > 0).any()
    # a continuation (t_min from the first march): the same lattice goes on
    again = ad.trace(got, m, minv)
    same_bits(again, vc.march(vc.Brick(vol, t, 1.7), want, minv))


def test_skipping_gives_the_same_bits(hip):
    vol = grid(40)
    t = tf("spikes")
    a, b = HipVolumeAdapter(vol, 1.0, skip=True), HipVolumeAdapter(vol, 1.0, skip=False)
    a.set_transfer(t)
    b.set_transfer(t)
    rays = make_rays(vol, IDENT, n=4000, seed=11)
    ra, rb = a.trace(rays, IDENT, IDENT), b.trace(rays, IDENT, IDENT)
    same_bits(ra, rb)
    same_bits(ra, vc.march(vc.Brick(vol, t, 1.0), rays, IDENT))
    ia, ib = a.info(), b.info()
    assert ia["n_blocks_empty"] > 0 and ia["n_blocks"] == 125
    assert ia["samples_marched"] == ib["samples_marched"] > 0
    assert ia["samples_gathered"] < ib["samples_gathered"] == ib["samples_marched"]


def test_opaque_transfer_function_terminates_every_entering_ray(hip):
    vol = grid()
    ad = HipVolumeAdapter(vol, 1.0)
    ad.set_transfer(tf("opaque"))
    lo, hi = vol.origin, (vol.origin + (vol.counts - 1).astype(F) * vol.spacing).astype(F)
    rng = np.random.default_rng(2)
    n = 2000
    r = np.zeros(n, RAY_DTYPE)
    r["origin"] = (lo + (hi - lo) * rng.random((n, 3)) + np.array([0, 0, 3], F)).astype(F)
    tgt = lo + (hi - lo) * (0.25 + 0.5 * rng.random((n, 3)))
    r["direction"] = (tgt - r["origin"]).astype(F)
    r["t_min"] = F(1e-6)
    r["id"] = np.arange(n)
    got = ad.trace(r, IDENT, IDENT)
    assert (got["depth"] & vc.OPAQUE).all() and (got["w"] >= F(0.99)).all()
    same_bits(got, vc.march(vc.Brick(vol, tf("opaque"), 1.0), r, IDENT))


def sphere128():
    vol = scenes.sphere_volume(128)
    vol.spacing = np.full(3, F(1.0 / 127), F)
    return vol


def camera(w=512, h=512):
    return scenes.Camera((2.3, 1.7, 3.1), (0.48, 0.51, 0.47), (0.0, 1.0, 0.0), float(F(35.0 * np.pi / 180.0)), w, h)


@pytest.fixture(scope="module")
def whole_frame(hip):
    vol = sphere128()
    cam = camera()
    tr = VolumeTracer(vol, cam, tf("cool"), sampling_rate=1.0).frame()
    fb = tr.framebuffer(False)
    return vol, cam, fb, tr.calls


def test_one_brick_frame_equals_the_checker(whole_frame):
    vol, cam, fb, calls = whole_frame
    b = vc.Brick(vol, tf("cool"), 1.0)
    want, wcalls = vc.frame([b], b.lo[None], b.hi[None], IDENT, cam)
    assert calls == wcalls == 1
    assert (fb[..., 3] > 0).sum() > 10000
    assert (fb.view(np.uint32) == want.view(np.uint32)).all()


@pytest.mark.parametrize("split", [(2, 2, 2), (4, 2, 1), (1, 1, 8)])
def test_bricked_frames_equal_the_one_brick_frame(whole_frame, split):
    vol, cam, fb, _ = whole_frame
    parts = scenes.split_volume(vol, *split)
    tr = VolumeTracer(parts, cam, tf("cool"), sampling_rate=1.0).frame()
    got = tr.framebuffer(False)
    assert (got.view(np.uint32) == fb.view(np.uint32)).all()
    # rounds: the checker's loop at a smaller film makes as many adapter calls as the device's
    small = camera(64, 64)
    tr2 = VolumeTracer(parts, small, tf("cool"), sampling_rate=1.0).frame()
    bricks = [vc.Brick(b, tf("cool"), 1.0) for b in parts]
    want, calls = vc.frame(bricks, [b.lo for b in parts], [b.hi for b in parts], IDENT, small)
    assert tr2.calls == calls > 1
    assert (tr2.framebuffer(False).view(np.uint32) == want.view(np.uint32)).all()


def test_moved_instance_frame_equals_the_checker(hip):
    vol = grid(33)
    cam = camera(96, 80)
    parts = scenes.split_volume(vol, 2, 1, 2)
    tr = VolumeTracer(parts, cam, tf("ramp"), m=MOVED, sampling_rate=2.0).frame()
    minv = scenes.instance_matrices(MOVED)[0]
    bricks = [vc.Brick(b, tf("ramp"), 2.0) for b in parts]
    want, calls = vc.frame(bricks, tr.inst_lo, tr.inst_hi, minv, cam)
    assert tr.calls == calls
    assert (tr.framebuffer(False).view(np.uint32) == want.view(np.uint32)).all()


def test_trace_equals_the_queue_path(hip):
    """One brick: every pixel of the frame holds the (C, A) gvt_hip_volume_trace gives its camera ray."""
    vol = grid(30)
    cam = camera(80, 64)
    tr = VolumeTracer(vol, cam, tf("cool"), sampling_rate=1.0).frame()
    fb = tr.framebuffer(False).reshape(-1, 4)
    rays = vc.camera_rays(cam)
    rays["w"] = 0
    rays["color"] = 0
    out = tr.adapters[0].trace(rays, IDENT, IDENT)
    lo, hi = tr.inst_lo[0], tr.inst_hi[0]
    tn, tf_ = vc.slab(lo, hi, rays["origin"], rays["direction"])
    entered = (tn <= tf_) & (tf_ > rays["t_min"])
    assert (fb[~entered] == 0).all()
    ids = out["id"][entered]
    assert (fb[ids, :3].view(np.uint32) == out["color"][entered].view(np.uint32)).all()
    assert (fb[ids, 3].view(np.uint32) == out["w"][entered].view(np.uint32)).all()


def test_trace_capacity_and_range(hip):
    vol = grid(12)
    ad = HipVolumeAdapter(vol, 1.0)
    ad.set_transfer(tf("cool"))
    rays = make_rays(vol, IDENT, n=100)
    lib = capi.load()
    out = np.zeros(10, RAY_DTYPE)
    n_out = C.c_size_t(0)
    rc = lib.gvt_hip_volume_trace(ad.h, capi.ptr(rays), C.c_size_t(100), C.c_size_t(0), C.c_size_t(0), capi.ptr(out), C.c_size_t(10), C.byref(n_out),
                                  capi.ptr(capi.f32(IDENT)), capi.ptr(capi.f32(IDENT)))
    assert rc == -3 and n_out.value == 100 and (out["id"] == 0).all()
    part = ad.trace(rays, IDENT, IDENT, begin=20, end=50)
    same_bits(part, vc.march(vc.Brick(vol, tf("cool"), 1.0), rays[20:50], IDENT))


def _create(data, counts, origin, spacing, offset, gcounts, rate=1.0):
    lib = capi.load()
    arr = lambda v, t: np.ascontiguousarray(v, t)  # noqa: E731
    keep = [arr(data, F), arr(counts, np.int32), arr(origin, F), arr(spacing, F), arr(offset, np.int32), arr(gcounts, np.int32)]
    h = lib.gvt_hip_volume_create(*[capi.ptr(k) for k in keep], rate, 0)
    if h:
        lib.gvt_hip_volume_destroy(C.c_void_p(h))
    return h, capi.last_error()


def test_invalid_arguments_are_refused(hip):
    d = np.zeros(64, F)
    ok = ([4, 4, 4], [0, 0, 0], [1, 1, 1], [0, 0, 0], [4, 4, 4])
    assert _create(d, *ok)[0]
    for bad, why in ((([1, 4, 4], [0, 0, 0], [1, 1, 1], [0, 0, 0], [4, 4, 4]), "counts"),
                     (([4, 4, 4], [0, 0, 0], [1, 0, 1], [0, 0, 0], [4, 4, 4]), "spacing"),
                     (([4, 4, 4], [0, 0, 0], [1, -1, 1], [0, 0, 0], [4, 4, 4]), "spacing"),
                     (([4, 4, 4], [0, 0, 0], [1, 1, 1], [1, 0, 0], [4, 4, 4]), "outside"),
                     (([4, 4, 4], [0, 0, 0], [1, 1, 1], [-1, 0, 0], [8, 4, 4]), "outside")):
        h, err = _create(d, *bad)
        assert not h and why in err, err
    assert not _create(d, *ok, rate=0.0)[0]
    vol = grid(8)
    ad = HipVolumeAdapter(vol, 1.0)
    lib = capi.load()
    cm, om = read("CoolWarm.cmap", 4), read("CoolWarm.omap", 2)
    set_tf = lambda c, nc, o, no, lo, hi: lib.gvt_hip_volume_set_transfer(ad.h, capi.ptr(c), nc, capi.ptr(o), no, lo, hi)  # noqa: E731
    assert set_tf(cm, 3, om, 11, 0.0, 1.0) == 0
    assert set_tf(cm, 1, om, 11, 0.0, 1.0) == -1 and "at least 2" in capi.last_error()
    assert set_tf(cm, 3, om, 1, 0.0, 1.0) == -1
    assert set_tf(cm, 3, om, 11, 1.0, 1.0) == -1 and "empty" in capi.last_error()
    assert set_tf(cm, 3, om, 11, 2.0, 1.0) == -1
    dec = om.copy()
    dec[[3, 4]] = dec[[4, 3]]
    assert set_tf(cm, 3, dec, 11, 0.0, 1.0) == -1 and "decreases" in capi.last_error()
    fresh = HipVolumeAdapter(vol, 1.0)  # no transfer function yet: tracing is refused
    with pytest.raises(capi.GvtHipError):
        fresh.trace(make_rays(vol, IDENT, n=10), IDENT, IDENT)
