"""Time-varying volumes on the device: gvt_hip_volume_update_samples (k_vol_ranges, csrc/volume.hip) against a volume freshly created from
the new samples, the numpy checkers (tests/volume_checker.py, tests/volume_surface_checker.py) and the restated macro-cell rules
(tests/volume_range_checker.py), bit for bit.  gvt_hip_volume_create computes its ranges with the same kernel, so the fresh volumes pin
it against the checkers too.  Grids: one cell; blocks (2, 1, 3) with a last block of one cell and an axis of exactly eight cells; two
full blocks per axis; the 24^3 noise grid; rows longer than one block's run of macro cells."""
import ctypes as C

import numpy as np
import pytest
import torch  # (before the library initialises the device, as in test_gpu_animation.py)

from gravit_amd import capi, scenes
from gravit_amd.adapter import HipVolumeAdapter
from gravit_amd.scheduler import VolumeTracer
from tests import volume_checker as vc
from tests import volume_edge_cases as ec
from tests import volume_range_checker as rc
from tests import volume_surface_checker as sc
from tests.test_gpu_volume import IDENT, camera, make_rays, tf
from tests.test_gpu_volume_surfaces import LIGHTS, PLANES, adapter, same_bits

pytestmark = pytest.mark.gpu

F = np.float32
PLAIN = ("color", "w", "t_min", "depth")
SHAPES = [(2, 2, 2), (10, 9, 18), (17, 17, 17), (24, 24, 24)]  # x y z vertices
INFO = ("value_min", "value_max", "n_blocks", "n_blocks_empty")
_cache = {}


def step(shape, seed):
    """A time step on `shape` vertices: smooth noise in [0, 1] (cut from a cube), stretched so that the sparse table meets some blocks."""
    nx, ny, nz = shape
    d = scenes.noise_volume(max(shape), seed=seed).data[:nz, :ny, :nx]
    d = np.clip(0.5 + (d - 0.5) * 1.6, 0.0, 1.0).astype(F)
    m = max(shape) - 1
    return scenes.VolumeData(np.ascontiguousarray(d), np.array([-0.25, 0.1, -0.4], F), np.array([1.0 / m, 1.1 / m, 0.9 / m], F))


def steps(shape):
    """(step 0, step 1, rays, the checker's march of step 1 under the sparse table): computed once."""
    if shape not in _cache:
        v0, v1 = step(shape, 3), step(shape, 5)
        rays = make_rays(v1, IDENT, n=1500)
        _cache[shape] = (v0, v1, rays, vc.march(vc.Brick(v1, tf("spikes"), 1.3), rays, IDENT))
    return _cache[shape]


def volume(vol, t=None, rate=1.3, skip=True):
    ad = HipVolumeAdapter(vol, sampling_rate=rate, skip=skip)
    if t is not None:
        ad.set_transfer(t)
    return ad


def same_info(a, b):
    ia, ib = a.info(), b.info()
    for k in INFO:
        assert np.array_equal(ia[k], ib[k], equal_nan=True), (k, ia[k], ib[k])
    return ia


# ---- 1. update equals fresh create
@pytest.mark.parametrize("skip", [True, False])
@pytest.mark.parametrize("shape", SHAPES)
def test_update_equals_a_fresh_create(hip, shape, skip):
    v0, v1, rays, want = steps(shape)
    t = tf("spikes")
    a, b = volume(v0, t, skip=skip), volume(v1, t, skip=skip)
    before = a.trace(rays, IDENT, IDENT)
    a.update_samples(v1.data)
    ra, rb = a.trace(rays, IDENT, IDENT), b.trace(rays, IDENT, IDENT)
    same_bits(ra, rb, PLAIN)
    same_bits(ra, want, PLAIN)
    info = same_info(a, b)
    assert info["n_blocks"] == int(np.prod(rc.blocks(v1.data.shape)))
    assert info["n_blocks_empty"] == rc.n_blocks_empty(v1.data, t, 1.3)
    assert (info["value_min"], info["value_max"]) == rc.value_range(v1.data)
    # the counters go on: A has marched both steps' rays
    assert a.info()["samples_marched"] > b.info()["samples_marched"] > 0
    if shape == (24, 24, 24):  # (not vacuous: the steps differ where rays can see it, and in what the table leaves empty)
        assert (before["w"] != ra["w"]).any()
        assert 0 < info["n_blocks_empty"] < info["n_blocks"] and rc.n_blocks_empty(v0.data, t, 1.3) != info["n_blocks_empty"]


# ---- 2. the stale-table trap, both directions
def test_tables_follow_the_samples_both_ways(hip):
    n = 24                                            # 3 x 3 x 3 macro cells; (1, 1, 1) owns the vertices 8..16 per axis
    geo = step((n, n, n), 3)
    zero = scenes.VolumeData(np.zeros((n, n, n), F), geo.origin, geo.spacing)
    d1 = np.zeros((n, n, n), F)
    d1[9:16, 9:16, 9:16] = 0.9                        # inside the block: nobody else's vertices
    d1[12, 12, 16] = 0.9                              # x = 16: the layer it shares with block (2, 1, 1)
    spike = scenes.VolumeData(d1, geo.origin, geo.spacing)
    t = tf("spikes")
    rays = make_rays(zero, IDENT, n=1500)
    a = volume(zero, t)
    r0 = a.trace(rays, IDENT, IDENT)
    assert a.info()["n_blocks_empty"] == rc.n_blocks_empty(zero.data, t, 1.3) == 27
    assert (r0["w"] == 0).all()
    a.update_samples(d1)
    r1 = a.trace(rays, IDENT, IDENT)
    empty = rc.empty_blocks(d1, t, 1.3)
    assert a.info()["n_blocks_empty"] == int(empty.sum()) == 25 and not empty[1, 1, 1] and not empty[1, 1, 2]
    same_bits(r1, vc.march(vc.Brick(spike, t, 1.3), rays, IDENT), PLAIN)
    same_bits(r1, volume(spike, t, skip=False).trace(rays, IDENT, IDENT), PLAIN)
    assert (r1["w"] > 0).sum() > 20                   # rays through the block gained opacity
    a.update_samples(zero.data)
    assert a.info()["n_blocks_empty"] == 27
    same_bits(a.trace(rays, IDENT, IDENT), r0, PLAIN)


# ---- 3. surfaces: the per-cell words are rebuilt
def test_update_with_surfaces(hip):
    v0, v1, rays, _ = steps((24, 24, 24))
    t = tf("spikes")
    S = sc.Surfaces([-0.5, 0.85], PLANES[:1], 0.5, LIGHTS[:1])  # below and above every block the sparse table leaves empty: they stay skippable
    rays = rays.copy()
    rays["t"] = 123.0
    a = adapter(v0, t, 1.3, S)
    a.update_samples(v1.data)
    ra = a.trace(rays, IDENT, IDENT)
    same_bits(ra, adapter(v1, t, 1.3, S).trace(rays, IDENT, IDENT))
    same_bits(ra, adapter(v1, t, 1.3, S, skip=False).trace(rays, IDENT, IDENT))
    same_bits(ra, sc.march(vc.Brick(v1, t, 1.3), S, rays, IDENT))
    assert sc.march.crossings > 100 and a.crossings() == sc.march.crossings
    assert a.info()["samples_gathered"] < a.info()["samples_marched"]


# ---- 4. non-finite samples arrive in an update
def huge_on_a_boundary():
    vol = ec.huge()
    vol.data[10, 4, 8], vol.data[10, 5, 8] = 3e38, -3e38  # x = 8: a pair in one cell on the face between two blocks
    return vol


@pytest.fixture(scope="module")
def edge_rays():
    return ec.edge_rays(ec.plateaus(), IDENT)


@pytest.mark.parametrize("kind,where", [("nan", "bottom"), ("pinf", "top"), ("ninf", "bottom"), ("mixed", "top"), ("mixed", "middle"), ("huge", "low"), ("huge", "top")])
def test_update_to_nonfinite_samples(hip, edge_rays, kind, where):
    """ec.NONFINITE_VERTS: a block's interior, a block face (8, 4, 12), a block corner (16, 8, 16), the brick's outer faces."""
    vol, t = (huge_on_a_boundary(), ec.huge_table(where)) if kind == "huge" else (ec.nonfinite(kind), ec.nonfinite_table(where))
    a = volume(ec.plateaus(), t, 1.0)
    a.update_samples(vol.data)
    b, n = volume(vol, t, 1.0), volume(vol, t, 1.0, skip=False)
    ra = a.trace(edge_rays, IDENT, IDENT)
    same_bits(ra, b.trace(edge_rays, IDENT, IDENT), PLAIN)
    same_bits(ra, n.trace(edge_rays, IDENT, IDENT), PLAIN)
    with np.errstate(all="ignore"):
        same_bits(ra, vc.march(vc.Brick(vol, t, 1.0), edge_rays, IDENT), PLAIN)
    info = same_info(a, b)
    assert info["n_blocks_empty"] == rc.n_blocks_empty(vol.data, t, 1.0)
    assert (info["value_min"], info["value_max"]) == rc.value_range(vol.data)
    if where != "middle":
        assert info["n_blocks_empty"] > 0 and a.info()["samples_gathered"] < a.info()["samples_marched"]


def test_only_nan_and_signed_zeros(hip):
    """A block of nothing but NaN keeps +Inf / -Inf as its bounds (value_min / value_max of an all-NaN brick show them)."""
    nan = np.full((3, 9, 10), np.nan, F)
    geo = (np.zeros(3, F), np.full(3, F(0.125), F))
    a = volume(scenes.VolumeData(np.zeros((3, 9, 10), F), *geo), tf("spikes"), 1.0)
    a.update_samples(nan)
    i = a.info()
    assert i["value_min"] == np.inf and i["value_max"] == -np.inf and i["n_blocks_empty"] == rc.n_blocks_empty(nan, tf("spikes"), 1.0)
    nan[1, 4, 9] = -0.0
    a.update_samples(nan)
    i = a.info()
    assert i["value_min"] == 0.0 and i["value_max"] == 0.0 and i["n_blocks_empty"] == rc.n_blocks_empty(nan, tf("spikes"), 1.0)


# ---- rows longer than one block's run of 32 macro cells (256 cells): the run's last boundary vertex, with and without 16-byte rows
@pytest.mark.parametrize("shape", [(264, 3, 10), (259, 2, 9), (257, 2, 2)])
def test_long_rows(hip, shape):
    nx, ny, nz = shape
    t = tf("spikes")
    geo = (np.zeros(3, F), np.full(3, F(1.0 / 64), F))
    a = volume(scenes.VolumeData(np.zeros((nz, ny, nx), F), *geo), t, 1.0)
    n_blocks = int(np.prod(rc.blocks((nz, ny, nx))))
    assert a.info()["n_blocks"] == a.info()["n_blocks_empty"] == n_blocks
    seen = set()
    for x in (0, 8, 248, 255, 256, 257, nx - 1):
        if x >= nx:
            continue
        d = np.zeros((nz, ny, nx), F)
        d[nz - 1, ny - 1, x] = 0.9                    # one vertex at the spike: the blocks that hold it, and no other, stop being empty
        d[0, 0, (x + 100) % nx] = -2.0 - x            # ... and the minimum sits somewhere else
        a.update_samples(d)
        i = a.info()
        empty = rc.empty_blocks(d, t, 1.0)
        assert i["n_blocks_empty"] == int(empty.sum()) < n_blocks
        assert i["value_min"] == F(-2.0 - x) and i["value_max"] == F(0.9)
        seen.add(n_blocks - int(empty.sum()))
    assert seen == {1, 2}                             # a vertex inside one block, and one shared by two
    rng = np.random.default_rng(1)
    d = np.clip(rng.random((nz, ny, nx), dtype=np.float32) * 0.2 + np.linspace(0.0, 0.9, nx, dtype=F)[None, None, :], 0, 1).astype(F)
    vol = scenes.VolumeData(d, *geo)
    a.update_samples(d)
    rays = make_rays(vol, IDENT, n=400)
    ra = a.trace(rays, IDENT, IDENT)
    same_bits(ra, volume(vol, t, 1.0, skip=False).trace(rays, IDENT, IDENT), PLAIN)
    same_bits(ra, vc.march(vc.Brick(vol, t, 1.0), rays, IDENT), PLAIN)
    assert 0 < a.info()["n_blocks_empty"] == rc.n_blocks_empty(d, t, 1.0)


# ---- 5. samples in device memory
@pytest.mark.parametrize("shape", [(10, 9, 18), (24, 24, 24)])
def test_device_samples(hip, shape):
    v0, v1, rays, want = steps(shape)
    t = tf("spikes")
    dev0, dev1 = torch.from_numpy(v0.data).cuda(), torch.from_numpy(v1.data).cuda()
    a, b = volume(v0, t), volume(v0, t)
    a.update_samples(dev1)
    b.update_samples(v1.data)
    ra = a.trace(rays, IDENT, IDENT)
    same_bits(ra, b.trace(rays, IDENT, IDENT), PLAIN)
    same_bits(ra, want, PLAIN)
    same_info(a, b)
    # create from a device tensor = create from the host array
    x, y = volume(scenes.VolumeData(dev0, v0.origin, v0.spacing), t), volume(v0, t)
    same_bits(x.trace(rays, IDENT, IDENT), y.trace(rays, IDENT, IDENT), PLAIN)
    assert same_info(x, y)["n_blocks_empty"] == rc.n_blocks_empty(v0.data, t, 1.3)
    with pytest.raises(ValueError):
        a.update_samples(dev1.double())
    with pytest.raises(ValueError):
        a.update_samples(dev1[:, :, :-1])


# ---- 6. a bricked frame
def test_bricked_frame_follows_the_update(hip):
    v0, v1, _, _ = steps((24, 24, 24))
    cam = camera(64, 48)
    t = tf("cool")
    tr = VolumeTracer(scenes.split_volume(v0, 2, 2, 1), cam, t, sampling_rate=1.0).frame()
    first = tr.framebuffer(False).copy()
    handles = [a.h.value for a in tr.adapters]
    assert tr.update(scenes.split_volume(v1, 2, 2, 1)) is tr
    got = tr.frame().framebuffer(False)
    fresh = VolumeTracer(scenes.split_volume(v1, 2, 2, 1), cam, t, sampling_rate=1.0).frame().framebuffer(False)
    whole = VolumeTracer(v1, cam, t, sampling_rate=1.0).frame().framebuffer(False)
    assert (got.view(np.uint32) == fresh.view(np.uint32)).all()
    assert (got.view(np.uint32) == whole.view(np.uint32)).all()
    assert (got != first).any() and (got[..., 3] > 0).sum() > 200
    assert handles == [a.h.value for a in tr.adapters]
    for other in (scenes.split_volume(v0, 1, 2, 2), v0):
        with pytest.raises(ValueError):
            tr.update(other)
    assert (tr.frame().framebuffer(False).view(np.uint32) == got.view(np.uint32)).all()  # a refused update changed nothing
    assert (tr.update(scenes.split_volume(v0, 2, 2, 1)).frame().framebuffer(False).view(np.uint32) == first.view(np.uint32)).all()


# ---- 7. argument checks
def test_invalid_arguments_leave_the_volume_alone(hip):
    v0, v1, rays, _ = steps((10, 9, 18))
    t = tf("spikes")
    a = volume(v0, t)
    before, info = a.trace(rays, IDENT, IDENT), a.info()
    lib = capi.load()
    d = np.ascontiguousarray(v1.data)
    n = d.size
    call = lambda h, p, cnt, flags: lib.gvt_hip_volume_update_samples(h, p, C.c_size_t(cnt), C.c_uint32(flags), None)  # noqa: E731
    assert call(None, capi.ptr(d), n, 0) == -1
    assert call(a.h, None, n, 0) == -1
    assert call(a.h, capi.ptr(d), n - 1, 0) == -1 and "samples" in capi.last_error()
    assert call(a.h, capi.ptr(d), n + 1, 0) == -1
    assert call(a.h, capi.ptr(d), n, 6) == -1 and "flags" in capi.last_error()
    same_bits(a.trace(rays, IDENT, IDENT), before, PLAIN)
    for k in INFO:
        assert a.info()[k] == info[k]
    with pytest.raises(ValueError):
        a.update_samples(d[:-1])
    with pytest.raises(ValueError):
        a.update_samples(d.astype(np.float64))
    assert call(a.h, capi.ptr(d), n, 0) == 0          # (ms_out may be NULL)
    same_bits(a.trace(rays, IDENT, IDENT), volume(v1, t).trace(rays, IDENT, IDENT), PLAIN)


# ---- 8. update before set_transfer
def test_update_before_the_transfer_function(hip):
    v0, v1, rays, want = steps((17, 17, 17))
    t = tf("spikes")
    a = volume(v0)
    a.update_samples(v1.data)
    assert a.info()["n_blocks_empty"] == 0 and (a.info()["value_min"], a.info()["value_max"]) == rc.value_range(v1.data)
    with pytest.raises(capi.GvtHipError):
        a.trace(rays, IDENT, IDENT)
    a.set_transfer(t)
    b = volume(v1, t)
    same_bits(a.trace(rays, IDENT, IDENT), b.trace(rays, IDENT, IDENT), PLAIN)
    same_bits(a.trace(rays, IDENT, IDENT), want, PLAIN)
    same_info(a, b)


# ---- 9. ms_out
def test_ms_out_is_finite_and_positive(hip):
    v0, v1, _, _ = steps((24, 24, 24))
    a = volume(v0, tf("spikes"))
    for d in (v1.data, v0.data):
        ms = a.update_samples(d)
        assert np.isfinite(ms) and ms > 0
