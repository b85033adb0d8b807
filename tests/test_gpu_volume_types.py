"""Typed voxels (gvt_hip_volume_create_typed, HipVolumeAdapter(native=True)): a uint8 / int16 / uint16 brick stays at its own width on the
device and answers bit for bit like the float32 brick of the converted samples.  The references are the numpy checkers fed
data.astype(float32) and the library's own F32 volume of the same converted data; nothing is compared with the typed path alone."""
import ctypes as C

import numpy as np
import pytest
import torch  # (before the library initialises the device, as in test_gpu_volume_update.py)

from gravit_amd import capi, scenes
from gravit_amd.adapter import HipVolumeAdapter, TransferFunction
from gravit_amd.layouts import RAY_DTYPE
from gravit_amd.scheduler import VolumeTracer
from tests import volume_checker as vc
from tests import volume_range_checker as rc
from tests import volume_surface_checker as sc
from tests.test_gpu_volume import IDENT, MOVED, camera, grid, make_rays, tf
from tests.test_gpu_volume_surfaces import LIGHTS, PLANES, same_bits

pytestmark = pytest.mark.gpu

F = np.float32
PLAIN = ("color", "w", "t_min", "depth")
INFO = ("value_min", "value_max", "n_blocks", "n_blocks_empty")
COUNTERS = ("samples_marched", "samples_gathered")
from tests.volume_common import ALL, TYPES, as_float, quantised, scaled  # noqa: E402,F401  (shared with the host tests)


def volume(vol, t=None, rate=1.3, skip=True, native=True, S=None):
    ad = HipVolumeAdapter(vol, sampling_rate=rate, skip=skip, native=native)
    if t is not None:
        ad.set_transfer(t)
    if S is not None:
        ad.set_surfaces(S.iso, S.planes, float(S.opacity))
        ad.set_lights(list(zip(S.lpos, S.lcol)), float(S.ka), float(S.kd))
    return ad


def same_info(a, b, keys=INFO):
    ia, ib = a.info(), b.info()
    for k in keys:
        assert ia[k] == ib[k], (k, ia[k], ib[k])
    return ia


def info_equals_the_checker(info, data, t, rate):
    f = data.astype(F)
    assert info["n_blocks"] == int(np.prod(rc.blocks(f.shape)))
    assert info["n_blocks_empty"] == rc.n_blocks_empty(f, t, rate)
    assert (info["value_min"], info["value_max"]) == rc.value_range(f)


# ---- 1. the march equals the checker
@pytest.mark.parametrize("moved", [False, True])
@pytest.mark.parametrize("kind", ["cool", "spikes"])
@pytest.mark.parametrize("ty", ALL)
def test_march_equals_the_checker(hip, ty, kind, moved):
    vol = quantised(grid(24), ty)
    m = MOVED if moved else IDENT
    minv = scenes.instance_matrices(m)[0]
    t = scaled(kind, ty)
    ad = volume(vol, t, 1.7)
    assert (ad.voxel_type, ad.sample_bytes) == (TYPES[ty][1], vol.data.itemsize)
    rays = make_rays(vol, m)
    got = ad.trace(rays, m, minv)
    B = vc.Brick(as_float(vol), t, 1.7)
    want = vc.march(B, rays, minv)
    assert len(got) == len(rays)
    same_bits(got, want, PLAIN)
    if kind == "cool":
        assert (got["w"][:600] > 0).any()
    else:
        assert 0 < ad.info()["n_blocks_empty"] < ad.info()["n_blocks"]
    same_bits(ad.trace(got, m, minv), vc.march(B, want, minv), PLAIN)  # the continuation: the same lattice goes on


# ---- 2. typed equals float, with and without skipping
@pytest.mark.parametrize("ty", ALL)
def test_typed_equals_float_with_and_without_skipping(hip, ty):
    vol = quantised(grid(40), ty)
    t = scaled("spikes", ty)
    rays = make_rays(vol, IDENT, n=4000, seed=11)
    a, b = volume(vol, t, 1.0), volume(vol, t, 1.0, skip=False)
    fa, fb = volume(as_float(vol), t, 1.0, native=False), volume(as_float(vol), t, 1.0, skip=False, native=False)
    assert (a.sample_bytes, fa.sample_bytes, fa.voxel_type) == (vol.data.itemsize, 4, capi.VOXEL_F32)
    ra = a.trace(rays, IDENT, IDENT)
    for other in (b, fa, fb):
        same_bits(ra, other.trace(rays, IDENT, IDENT), PLAIN)
    assert (ra["w"] > 0).any()
    same_info(a, b)
    same_info(a, fa, INFO + COUNTERS)
    same_info(b, fb, INFO + COUNTERS)
    info = a.info()
    info_equals_the_checker(info, vol.data, t, 1.0)
    assert info["n_blocks"] == 125 and 0 < info["n_blocks_empty"] < 125
    assert 0 < info["samples_gathered"] < b.info()["samples_gathered"] == b.info()["samples_marched"] == info["samples_marched"]


# ---- 3. extremes and signedness
def axis_and_diagonal_rays(vol, per=24, seed=5):
    """Rays along every axis and diagonal, both ways: towards points inside the box, from outside."""
    rng = np.random.default_rng(seed)
    lo = np.asarray(vol.origin, F)
    ext = ((vol.counts - 1).astype(F) * vol.spacing).astype(F)
    dirs = np.array([(x, y, z) for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1) if (x, y, z) != (0, 0, 0)], F)
    d = np.repeat(dirs, per, axis=0)
    tgt = (lo + ext * rng.random((len(d), 3))).astype(F)
    r = np.zeros(len(d), RAY_DTYPE)
    r["origin"] = (tgt - d * F(3.0) * ext.max()).astype(F)
    r["direction"] = d * ext.max()
    r["t_min"] = F(1e-6)
    r["t_max"] = np.finfo(F).max
    r["id"] = np.arange(len(d))
    return r


@pytest.mark.parametrize("shape", [(2, 3, 9), (2, 2, 2)])  # (nz, ny, nx)
@pytest.mark.parametrize("ty", ALL)
def test_extremes_and_signedness(hip, ty, shape):
    np_t, _, _, _, across = TYPES[ty]
    lim = np.iinfo(np_t)
    z, y, x = np.indices(shape)
    d = np.where((x + y + z) % 2 == 0, lim.min, lim.max).astype(np_t)
    d[0, 1, shape[2] // 2] = across
    vol = scenes.VolumeData(np.ascontiguousarray(d))
    t = scaled("ramp", ty, (float(lim.min), float(lim.max)))
    rays = np.concatenate([axis_and_diagonal_rays(vol), make_rays(vol, IDENT, n=500)])
    a, f = volume(vol, t, 1.7), volume(as_float(vol), t, 1.7, native=False)
    got = a.trace(rays, IDENT, IDENT)
    same_bits(got, f.trace(rays, IDENT, IDENT), PLAIN)
    same_bits(got, vc.march(vc.Brick(as_float(vol), t, 1.7), rays, IDENT), PLAIN)
    assert (got["w"] > 0).sum() > 100
    info = same_info(a, f, INFO + COUNTERS)
    assert (info["value_min"], info["value_max"]) == (F(lim.min), F(lim.max))


# ---- 4. rows that are no multiple of 4, and long rows
def stretched(shape, ty, seed=3):
    """(nz, ny, nx) vertices of smooth noise: a 24^3 grid cut in y and z and resampled along x, contrast raised so that the sparse table
    meets some macro cells and leaves others empty."""
    nz, ny, nx = shape
    base = scenes.noise_volume(24, seed=seed).data[:nz, :ny, :].astype(np.float64)
    pos = np.linspace(0.0, 23.0, nx)
    i0 = np.minimum(pos.astype(np.int64), 22)
    w = pos - i0
    d = np.clip(0.5 + (base[:, :, i0] * (1 - w) + base[:, :, i0 + 1] * w - 0.5) * 1.6, 0.0, 1.0).astype(F)
    m = max(shape) - 1
    return quantised(scenes.VolumeData(d, np.array([-0.25, 0.1, -0.4], F), np.array([1.0 / m, 1.1 / m, 0.9 / m], F)), ty)


@pytest.mark.parametrize("shape", [(10, 9, 23), (3, 9, 301), (2, 9, 520)])
@pytest.mark.parametrize("ty", ALL)
def test_odd_and_long_rows(hip, ty, shape):
    vol = stretched(shape, ty)
    t = scaled("spikes", ty)
    rays = make_rays(vol, IDENT, n=2000)
    a, f = volume(vol, t), volume(as_float(vol), t, native=False)
    info = same_info(a, f)
    info_equals_the_checker(info, vol.data, t, 1.3)
    assert 0 < info["n_blocks_empty"] < info["n_blocks"]
    got = a.trace(rays, IDENT, IDENT)
    same_bits(got, f.trace(rays, IDENT, IDENT), PLAIN)
    same_bits(got, volume(vol, t, skip=False).trace(rays, IDENT, IDENT), PLAIN)
    same_info(a, f, COUNTERS)
    assert a.info()["samples_gathered"] > 0


# ---- 5. surfaces
@pytest.mark.parametrize("ty", ["u8", "i16"])
def test_surfaces(hip, ty):
    vol = quantised(grid(24), ty)
    lo, hi = TYPES[ty][2]
    # an isovalue many vertices hold exactly (the >= side rule meets equal values), and one between two integers
    held = 128 if ty == "u8" else int(np.bincount((vol.data.astype(np.int64) + 32768).ravel()).argmax()) - 32768
    assert (vol.data == held).sum() >= (10 if ty == "u8" else 2)
    S = sc.Surfaces([float(held), lo + 0.58 * (hi - lo) + 0.5], PLANES[:1], 0.5, LIGHTS[:2])
    t = scaled("spikes", ty)  # fivespikes.omap: the per-cell skip words matter
    rays = make_rays(vol, IDENT, n=2000)
    rays["t"] = 123.0
    fields = PLAIN + ("t",)
    a, f = volume(vol, t, 1.7, S=S), volume(as_float(vol), t, 1.7, native=False, S=S)
    got = a.trace(rays, IDENT, IDENT)
    same_bits(got, f.trace(rays, IDENT, IDENT), fields)
    same_bits(got, volume(vol, t, 1.7, skip=False, S=S).trace(rays, IDENT, IDENT), fields)
    same_bits(got, sc.march(vc.Brick(as_float(vol), t, 1.7), S, rays, IDENT), fields)
    assert a.crossings() == f.crossings() == sc.march.crossings > 0
    same_info(a, f, INFO + COUNTERS)
    assert 0 < a.info()["samples_gathered"] < a.info()["samples_marched"]


# ---- 6. update in place
def two_steps(shape, ty):
    return stretched(shape, ty, 3), stretched(shape, ty, 5)


@pytest.mark.parametrize("shape", [(10, 9, 23), (24, 24, 24)])
@pytest.mark.parametrize("ty", ALL)
def test_update_equals_a_fresh_native_create(hip, ty, shape):
    v0, v1 = two_steps(shape, ty)
    t = scaled("spikes", ty)
    rays = make_rays(v1, IDENT, n=1500)
    a, b = volume(v0, t), volume(v1, t)
    before = a.trace(rays, IDENT, IDENT)
    handle = a.h.value
    ms = a.update_samples(v1.data)
    assert np.isfinite(ms) and ms > 0 and a.h.value == handle
    ra = a.trace(rays, IDENT, IDENT)
    same_bits(ra, b.trace(rays, IDENT, IDENT), PLAIN)
    same_bits(ra, vc.march(vc.Brick(as_float(v1), t, 1.3), rays, IDENT), PLAIN)
    info_equals_the_checker(same_info(a, b), v1.data, t, 1.3)
    assert (before["w"] != ra["w"]).any()
    # before any set_transfer: the tables are built when the table arrives
    c = volume(v0)
    c.update_samples(v1.data)
    assert c.info()["n_blocks_empty"] == 0
    c.set_transfer(t)
    same_bits(c.trace(rays, IDENT, IDENT), ra, PLAIN)
    same_info(c, b)
    with pytest.raises(ValueError):
        a.update_samples(v1.data.astype(F))
    with pytest.raises(ValueError):
        a.update_samples(v1.data.astype(np.int16 if ty != "i16" else np.uint16))
    same_bits(a.trace(rays, IDENT, IDENT), ra, PLAIN)


@pytest.mark.parametrize("ty", ALL)
def test_tables_follow_the_samples_both_ways(hip, ty):
    n = 24                                            # 3 x 3 x 3 macro cells; (1, 1, 1) owns the vertices 8..16 per axis
    np_t, _, (lo, hi), _, _ = TYPES[ty]
    geo = grid(n)
    floor_, spike_ = np_t(np.rint(lo)), np_t(np.rint(lo + 0.9 * (hi - lo)))  # transparent | the spike around 0.9 of the range
    d0 = np.full((n, n, n), floor_, np_t)
    d1 = d0.copy()
    d1[9:16, 9:16, 9:16] = spike_
    d1[12, 12, 16] = spike_                           # x = 16: the layer the block shares with (2, 1, 1)
    zero, spike = scenes.VolumeData(d0, geo.origin, geo.spacing), scenes.VolumeData(d1, geo.origin, geo.spacing)
    t = scaled("spikes", ty)
    rays = make_rays(zero, IDENT, n=1500)
    a = volume(zero, t)
    r0 = a.trace(rays, IDENT, IDENT)
    assert a.info()["n_blocks_empty"] == rc.n_blocks_empty(d0.astype(F), t, 1.3) == 27 and (r0["w"] == 0).all()
    a.update_samples(d1)                              # sparser -> denser
    r1 = a.trace(rays, IDENT, IDENT)
    empty = rc.empty_blocks(d1.astype(F), t, 1.3)
    assert a.info()["n_blocks_empty"] == int(empty.sum()) == 25 and not empty[1, 1, 1] and not empty[1, 1, 2]
    same_bits(r1, vc.march(vc.Brick(as_float(spike), t, 1.3), rays, IDENT), PLAIN)
    same_bits(r1, volume(as_float(spike), t, skip=False, native=False).trace(rays, IDENT, IDENT), PLAIN)
    assert (r1["w"] > 0).sum() > 20
    a.update_samples(d0)                              # denser -> sparser
    assert a.info()["n_blocks_empty"] == 27
    same_bits(a.trace(rays, IDENT, IDENT), r0, PLAIN)


@pytest.mark.parametrize("ty", ["u8", "i16"])
def test_update_from_device_tensors(hip, ty):
    v0, v1 = two_steps((10, 9, 23), ty)
    t = scaled("spikes", ty)
    rays = make_rays(v1, IDENT, n=1500)
    dev1 = torch.from_numpy(v1.data).cuda()
    a, b = volume(v0, t), volume(v0, t)
    a.update_samples(dev1)
    b.update_samples(v1.data)
    ra = a.trace(rays, IDENT, IDENT)
    same_bits(ra, b.trace(rays, IDENT, IDENT), PLAIN)
    same_bits(ra, volume(as_float(v1), t, native=False).trace(rays, IDENT, IDENT), PLAIN)
    info_equals_the_checker(same_info(a, b), v1.data, t, 1.3)
    with pytest.raises(ValueError):
        a.update_samples(dev1.float())
    with pytest.raises(ValueError):
        a.update_samples(dev1[:, :, :-1])


def test_refused_updates_leave_the_volume_alone(hip):
    v0, v1 = two_steps((10, 9, 23), "u8")
    t = scaled("spikes", "u8")
    rays = make_rays(v0, IDENT, n=1500)
    a = volume(v0, t)
    before, info = a.trace(rays, IDENT, IDENT), a.info()
    lib = capi.load()
    d, df = np.ascontiguousarray(v1.data), np.ascontiguousarray(v1.data.astype(F))
    n = d.size
    typed = lambda p, ty, cnt, flags: lib.gvt_hip_volume_update_samples_typed(a.h, p, ty, C.c_size_t(cnt), C.c_uint32(flags), None)  # noqa: E731
    assert lib.gvt_hip_volume_update_samples(a.h, capi.ptr(df), C.c_size_t(n), C.c_uint32(0), None) == -1 and "type" in capi.last_error()
    for other in (capi.VOXEL_F32, capi.VOXEL_I16, capi.VOXEL_U16, 4, -1):
        assert typed(capi.ptr(df), other, n, 0) == -1 and "type" in capi.last_error()
    assert typed(capi.ptr(d), capi.VOXEL_U8, n - 1, 0) == -1 and "samples" in capi.last_error()
    assert typed(capi.ptr(d), capi.VOXEL_U8, n + 1, 0) == -1
    assert typed(capi.ptr(d), capi.VOXEL_U8, n, 6) == -1 and "flags" in capi.last_error()
    assert typed(None, capi.VOXEL_U8, n, 0) == -1
    same_bits(a.trace(rays, IDENT, IDENT), before, PLAIN)
    for k in INFO:
        assert a.info()[k] == info[k]
    assert typed(capi.ptr(d), capi.VOXEL_U8, n, 0) == 0
    same_bits(a.trace(rays, IDENT, IDENT), volume(v1, t).trace(rays, IDENT, IDENT), PLAIN)
    # a float volume refuses typed samples in the same way
    f = volume(as_float(v0), t, native=False)
    assert lib.gvt_hip_volume_update_samples_typed(f.h, capi.ptr(d), capi.VOXEL_U8, C.c_size_t(n), C.c_uint32(0), None) == -1
    same_bits(f.trace(rays, IDENT, IDENT), before, PLAIN)


# ---- 7. device samples at creation
@pytest.mark.parametrize("ty", ["u8", "i16"])
def test_device_samples_at_creation(hip, ty):
    vol = stretched((10, 9, 23), ty)
    t = scaled("spikes", ty)
    rays = make_rays(vol, IDENT, n=1500)
    dev = torch.from_numpy(vol.data).cuda()
    x, y = volume(scenes.VolumeData(dev, vol.origin, vol.spacing), t), volume(vol, t)
    assert (x.voxel_type, x.sample_bytes) == (TYPES[ty][1], vol.data.itemsize)
    same_bits(x.trace(rays, IDENT, IDENT), y.trace(rays, IDENT, IDENT), PLAIN)
    info_equals_the_checker(same_info(x, y), vol.data, t, 1.3)
    with pytest.raises(ValueError):
        volume(scenes.VolumeData(dev.int(), vol.origin, vol.spacing), t)


# ---- 8. a bricked frame
@pytest.fixture(scope="module")
def sphere_frames(hip):
    """Per type: the quantised sphere, its table and the F32 tracer's frame of the converted data."""
    out = {}
    base = scenes.sphere_volume(64)
    base.spacing = np.full(3, F(1.0 / 63), F)
    cam = camera(128, 128)
    for ty in ("u8", "i16"):
        vol = quantised(base, ty)
        t = scaled("cool", ty)
        out[ty] = (vol, t, cam, VolumeTracer(as_float(vol), cam, t, sampling_rate=1.0).frame().framebuffer(False).copy())
    return out


@pytest.mark.parametrize("ty", ["u8", "i16"])
def test_bricked_frame(sphere_frames, ty):
    vol, t, cam, want = sphere_frames[ty]
    parts = scenes.split_volume(vol, 2, 2, 2)
    assert all(p.data.dtype == vol.data.dtype for p in parts)
    one = VolumeTracer(vol, cam, t, sampling_rate=1.0, native=True).frame()
    eight = VolumeTracer(parts, cam, t, sampling_rate=1.0, native=True).frame()
    assert all(a.sample_bytes == vol.data.itemsize for a in one.adapters + eight.adapters)
    fb1, fb8 = one.framebuffer(False), eight.framebuffer(False)
    assert (fb1.view(np.uint32) == fb8.view(np.uint32)).all()
    assert (fb1.view(np.uint32) == want.view(np.uint32)).all()
    B = vc.Brick(as_float(vol), t, 1.0)
    ref, calls = vc.frame([B], B.lo[None], B.hi[None], IDENT, cam)
    assert one.calls == calls == 1 and eight.calls > 1
    assert (fb1.view(np.uint32) == ref.view(np.uint32)).all()
    assert (fb1[..., 3] > 0).sum() > 1000
    # another voxel type is refused before a brick is touched
    with pytest.raises(ValueError):
        eight.update([scenes.Brick(p.data.astype(F), p.offset, p.global_counts, p.origin, p.spacing, p.lo, p.hi) for p in parts])
    assert (eight.frame().framebuffer(False).view(np.uint32) == fb8.view(np.uint32)).all()


# ---- 9. arguments
def test_arguments(hip):
    lib = capi.load()
    arr = lambda v, t: np.ascontiguousarray(v, t)  # noqa: E731
    geo = [arr([4, 4, 4], np.int32), arr([0, 0, 0], F), arr([1, 1, 1], F), arr([0, 0, 0], np.int32), arr([4, 4, 4], np.int32)]
    d, room = np.zeros(64, np.uint16), np.zeros(64, F)  # (room: 256 bytes, enough for every type)

    def create(samples, ty):
        h = lib.gvt_hip_volume_create_typed(samples, ty, *[capi.ptr(g) for g in geo], 1.0, 0)
        return C.c_void_p(h) if h else None

    for bad in (4, -1, 17):
        assert create(capi.ptr(d), bad) is None and "voxel type" in capi.last_error()
    assert create(None, capi.VOXEL_U8) is None and "null" in capi.last_error()
    for ty, nbytes in ((capi.VOXEL_F32, 4), (capi.VOXEL_U8, 1), (capi.VOXEL_I16, 2), (capi.VOXEL_U16, 2)):
        h = create(capi.ptr(room), ty)
        assert h is not None
        vt, nb = C.c_int(-1), C.c_size_t(0)
        assert lib.gvt_hip_volume_get_voxel_type(h, C.byref(vt), C.byref(nb)) == 0 and (vt.value, nb.value) == (ty, nbytes)
        assert lib.gvt_hip_volume_get_voxel_type(h, None, None) == 0
        lib.gvt_hip_volume_destroy(h)
    assert lib.gvt_hip_volume_get_voxel_type(None, None, None) == -1
    vol = grid(8)
    for other in (np.float64, np.int32, np.float32, np.int8):
        with pytest.raises(ValueError):
            HipVolumeAdapter(scenes.VolumeData(vol.data.astype(other), vol.origin, vol.spacing), 1.0, native=True)
    q = quantised(vol, "u8")
    a = HipVolumeAdapter(q, 1.0)  # native=False: converted to float32, as before
    assert (a.voxel_type, a.sample_bytes) == (capi.VOXEL_F32, 4)
    b = HipVolumeAdapter(q, 1.0, native=True)
    assert (b.voxel_type, b.sample_bytes) == (capi.VOXEL_U8, 1)
    t = scaled("cool", "u8")
    a.set_transfer(t)
    b.set_transfer(t)
    rays = make_rays(q, IDENT, n=500)
    same_bits(a.trace(rays, IDENT, IDENT), b.trace(rays, IDENT, IDENT), PLAIN)
