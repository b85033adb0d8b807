"""Ambient occlusion on the device (csrc/volume_ao_grid.inc, csrc/volume_fused_ao.inc; gvt_hip_volume_ao_grid_bake and
gvt_hip_volume_frame_ao) against the numpy checker (tests/volume_ao_checker.py), bit for bit: the baked grid in every bricking under both
matrices, under directions that run in brick faces, with one and with 32 directions and without a radius; the frame of both cases of
tests/volume_ao_cases.py in every bricking at both eyes with the base frame's counters; the cut, the skip flag; the grid of ones and
ka = 0 against the device's own base frames; typed voxels, the clipped and the mixed frame, CENTRAL bricks; stale grids, the bake's
refusals, the inert frames and the untouched entry points.
The checker counts a bake's crossings and nothing else of its march, so samples_marched is compared between the skipping and the plain
bake."""
import ctypes as C

import numpy as np
import pytest

from gravit_amd import capi, scenes
from gravit_amd.adapter import DepthPlane
from gravit_amd.scheduler import MixedTracer, NativeTracer, VolumeDomainTracer, VolumeTracer
from tests import volume_ao_cases as aoc
from tests import volume_ao_checker as ao
from tests import volume_checker as vc
from tests import volume_clip_checker as cc
from tests import volume_fog_shadow_cases as fgc
from tests import volume_fog_shadow_checker as fg
from tests import volume_fused_cases as fc
from tests import volume_mesh_shadow_cases as mc
from tests import volume_shade_checker as lc
from tests import volume_shadow_cases as swc
from tests import volume_surface_checker as sc
from tests.volume_common import as_float, quantised, scaled, tf

pytestmark = pytest.mark.gpu

F = np.float32
BOTH = capi.FUSED_SURFACES | capi.FUSED_LIT
FEATURES = {"lit": capi.FUSED_LIT, "surf_lit": BOTH, "surf": capi.FUSED_SURFACES}
COUNTER_KEYS = ("shadow_rays", "shadow_brick_visits", "shadow_crossings", "brick_visits", "rays_deposited", "crossings_rendered", "samples_shaded")
DEVICE_KEYS = COUNTER_KEYS + ("samples_marched", "samples_gathered", "shadow_samples_marched", "shadow_samples_gathered", "fog_samples_shadowed")
N_VERT = fc.N ** 3


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def dress(tr, S, on):
    if len(S):
        tr.set_surfaces(S.iso, S.planes, float(S.opacity))
    tr.set_lights(list(zip(S.lpos, S.lcol)), float(S.ka), float(S.kd))
    tr.set_shading(on)
    return tr


def tracer(mode, split, where, moved=None, skip=True, ao_on=True, mesh=False, which="main", steps=aoc.RADIUS_STEPS, ka=0.4, vol=None, native=False, t=None, S=None,
           parts=None, central=False, fog=True, shadows=True):
    """The case's tracer (ao_on=False: its base frame's).  mesh: the mesh-shadowed base, its occluders baked from
    tests/volume_mesh_shadow_cases.py's scene."""
    moved = aoc.CAMERAS[where] if moved is None else moved
    S0, on, table = swc.surfaces("main", mode, ka=ka)
    if parts is None:
        parts = fc.bricks_of(fc.volume() if vol is None else vol, split)
    tr = VolumeTracer(parts, fc.camera(where, moved), table if t is None else t, m=fc.matrix(moved), sampling_rate=fc.RATE, skip=skip, native=native,
                      fused=True, fused_shaded=True, shadows=shadows, shadow_bias=aoc.BIAS, fog_shadows=fog and shadows, fog_bias=aoc.GRID_BIAS, mesh_shadows=mesh,
                      fused_central=central, ao=ao_on and fog and shadows, ao_dirs=aoc.dirs(which), ao_radius=float(aoc.radius(steps)), ao_bias=aoc.GRID_BIAS)
    dress(tr, S0 if S is None else S, on)
    if mesh:
        tr.bake_occluders(mc.scene(moved))
    return tr


def grid_matches(tr, AO):
    """Every brick's downloaded plane is its part of the checker's grid."""
    for a in tr.adapters:
        o, n = a.offset, a.counts
        want = AO[o[2]:o[2] + n[2], o[1]:o[1] + n[1], o[0]:o[0] + n[0]]
        got = a.ao_grid()
        if got.shape != want.shape or not (bits(got) == bits(want)).all():
            return False
    return True


# ---- the baked grid

@pytest.mark.parametrize("moved", [False, True])
@pytest.mark.parametrize("split", fc.SPLITS)
@pytest.mark.parametrize("mode", aoc.MODES)
def test_baked_grid_has_the_checkers_bits(hip, mode, split, moved):
    AO, crossings = aoc.ao_grid(mode, moved)
    tr = tracer(mode, split, "outside", moved=moved).rebake_ao()
    st, g = tr.stats(), tr.ao_stats
    assert grid_matches(tr, AO)
    n_vert = sum(int(np.prod(a.counts)) for a in tr.adapters)
    assert st["ao_bakes"] == 1 and st["ao_rays"] == g["rays"] == 6 * n_vert and st["ao_bytes"] == 4 * n_vert and st["ao_ms"] > 0
    assert 0 < g["samples_gathered"] <= g["samples_marched"]
    if split == (1, 1, 1):  # (a shared vertex's rays are marched once per brick that stores it)
        assert g["crossings"] == crossings
    assert (g["crossings"] > 0) == (mode == "surf_lit")
    for a in tr.adapters:
        assert a.ao_grid_info() == {"present": 1, "current": 1, "n_dirs": 6, "bias": aoc.GRID_BIAS, "radius": float(aoc.radius()), "bytes": 4 * int(np.prod(a.counts))}
        assert a.light_grid_info()["present"] == 0  # (the AO bake is not the light grids')
    plain = tracer(mode, split, "outside", moved=moved, skip=False).rebake_ao()
    p = plain.ao_stats
    assert grid_matches(plain, AO)
    assert p["samples_gathered"] == p["samples_marched"] == g["samples_marched"] and p["crossings"] == g["crossings"] and p["rays"] == g["rays"]


@pytest.mark.parametrize("split", fc.SPLITS)
@pytest.mark.parametrize("mode", aoc.MODES)
def test_directions_that_run_in_brick_faces(hip, mode, split):
    AO, _ = aoc.ao_grid(mode, False, "parallel")
    tr = tracer(mode, split, "outside", moved=False, which="parallel").rebake_ao()
    assert tr.ao_stats["rays"] == 4 * sum(int(np.prod(a.counts)) for a in tr.adapters)
    assert grid_matches(tr, AO)


@pytest.mark.parametrize("which,split", [("one", (1, 1, 1)), ("one", (2, 2, 2)), ("max", (1, 1, 1))])
def test_one_direction_and_thirty_two(hip, which, split):
    AO, crossings = aoc.ao_grid("surf_lit", True, which)
    tr = tracer("surf_lit", split, "outside", moved=True, which=which).rebake_ao()
    n = len(aoc.dirs(which))
    assert n == (32 if which == "max" else 1) and tr.ao_stats["rays"] == n * sum(int(np.prod(a.counts)) for a in tr.adapters)
    assert grid_matches(tr, AO)
    assert split != (1, 1, 1) or tr.ao_stats["crossings"] == crossings
    assert all(a.ao_grid_info()["n_dirs"] == n for a in tr.adapters)


@pytest.mark.parametrize("split", [(1, 1, 1), (2, 2, 2)])
def test_without_a_radius(hip, split):
    AO, crossings = aoc.ao_grid("surf_lit", False, "main", np.inf)
    tr = tracer("surf_lit", split, "outside", moved=False, steps=np.inf).rebake_ao()
    assert grid_matches(tr, AO) and (bits(AO) != bits(aoc.ao_grid("surf_lit", False)[0])).any()
    assert split != (1, 1, 1) or tr.ao_stats["crossings"] == crossings
    assert all(a.ao_grid_info()["radius"] == np.inf for a in tr.adapters)


# ---- the frame

@pytest.mark.parametrize("where", sorted(aoc.CAMERAS))
@pytest.mark.parametrize("split", fc.SPLITS)
@pytest.mark.parametrize("mode", aoc.MODES)
def test_ao_frame_has_the_checkers_bits_and_the_base_frames_counts(hip, mode, split, where):
    want, counters, _ = aoc.reference(mode, split, where)
    tr = tracer(mode, split, where).frame()
    got, st = tr.framebuffer(False).copy(), tr.stats()
    assert st["ao"] == 1 and st["shadowed"] == 1 and st["fused"] == 1 and st["adapter_calls"] == 1 and st["features"] == FEATURES[mode]
    assert st["ao_bakes"] == 1 and st["light_bakes"] == 1
    assert got.any() and (bits(got) == bits(want)).all()
    for key in COUNTER_KEYS:
        assert st[key] == counters[key], key
    assert all(len(q) == 0 for q in tr.queues)
    base = tracer(mode, split, where, ao_on=False).frame()
    bs = base.stats()
    for key in DEVICE_KEYS:
        assert st[key] == bs[key], key
    bfb = base.framebuffer(False)
    assert (bits(got[..., 3]) == bits(bfb[..., 3])).all() and (bits(got[..., :3]) != bits(bfb[..., :3])).any()  # AO shows, in the colour alone


@pytest.mark.parametrize("where", sorted(aoc.CAMERAS))
@pytest.mark.parametrize("mode", aoc.MODES)
def test_the_cut_does_not_show(hip, mode, where):
    frames = [tracer(mode, s, where).frame().framebuffer(False).copy() for s in fc.SPLITS]
    for f in frames[1:]:
        assert (bits(f) == bits(frames[0])).all()


@pytest.mark.parametrize("split", [(1, 1, 1), (4, 4, 4)])
@pytest.mark.parametrize("mode", aoc.MODES)
def test_skipping_does_not_show(hip, mode, split):
    a = tracer(mode, split, "inside").frame()
    b = tracer(mode, split, "inside", skip=False).frame()
    sa, sb = a.stats(), b.stats()
    assert (bits(a.framebuffer(False)) == bits(b.framebuffer(False))).all() and sa["ao"] == sb["ao"] == 1
    assert sa["samples_marched"] == sb["samples_marched"] == sb["samples_gathered"] >= sa["samples_gathered"] > 0
    assert sa["samples_shaded"] == sb["samples_shaded"] > 0
    for key in COUNTER_KEYS + ("shadow_samples_marched",):
        assert sa[key] == sb[key], key


@pytest.mark.parametrize("mesh", [False, True])
@pytest.mark.parametrize("mode", ("lit", "surf_lit", "surf"))
def test_a_grid_of_ones_gives_the_devices_base_frame(hip, mode, mesh):
    """radius = dt with bias 1: no ray has a sample, AO == 1 at every vertex, ka * 1.f is ka (mode "surf": surfaces, the fog unlit)."""
    tr = tracer(mode, (2, 2, 2), "inside", mesh=mesh, steps=1.0).frame()
    base = tracer(mode, (2, 2, 2), "inside", mesh=mesh, ao_on=False).frame()
    st, bs = tr.stats(), base.stats()
    assert st["ao"] == 1 and st.get("mesh_shadowed", 0) == bs.get("mesh_shadowed", 0) == (1 if mesh else 0)
    assert all((a.ao_grid() == F(1)).all() for a in tr.adapters)
    assert base.framebuffer(False).any() and (bits(tr.framebuffer(False)) == bits(base.framebuffer(False))).all()
    for key in DEVICE_KEYS:
        assert st[key] == bs[key], key


@pytest.mark.parametrize("mesh", [False, True])
@pytest.mark.parametrize("mode", aoc.MODES)
def test_the_mesh_shadowed_base(hip, mode, mesh):
    """The AO frame over the mesh-shadowed base against the checker with the occluder grid (mesh=False: the same call over the fog base)."""
    moved = aoc.CAMERAS["inside"]
    bricks, lo, hi, minv, cam, S, shading, _, _ = aoc.setup(mode, (2, 2, 2), "inside", moved)
    O = mc.occluder_grid(moved)[0] if mesh else None
    want, counters = ao.frame(bricks, lo, hi, minv, cam, S, shading, fgc.light_grid(mode, moved)[0], O, aoc.ao_grid(mode, moved)[0], None, aoc.BIAS)
    tr = tracer(mode, (2, 2, 2), "inside", mesh=mesh).frame()
    st = tr.stats()
    assert st["ao"] == 1 and st.get("mesh_shadowed", 0) == (1 if mesh else 0)
    assert (bits(tr.framebuffer(False)) == bits(want)).all() and want.any()
    for key in COUNTER_KEYS:
        assert st[key] == counters[key], key


@pytest.mark.parametrize("mode", aoc.MODES)
def test_without_ambient_light_the_frame_is_the_base_frame(hip, mode):
    got = tracer(mode, (2, 2, 2), "inside", ka=0.0).frame()
    want = tracer(mode, (2, 2, 2), "inside", ka=0.0, ao_on=False).frame()
    assert got.stats()["ao"] == 1 and want.framebuffer(False).any()
    assert (bits(got.framebuffer(False)) == bits(want.framebuffer(False))).all()


def test_typed_voxels(hip):
    vol, t = quantised(fc.volume(), "u8"), scaled("spikes", "u8")
    S, on, _ = swc.surfaces("main", "surf_lit", scale=255.0)
    tr = tracer("surf_lit", (2, 2, 2), "inside", vol=vol, native=True, t=t, S=S).frame()
    st = tr.stats()
    assert tr.adapters[0].dtype_name == "uint8" and st["ao"] == 1 and st["shadow_rays"] > 0 and st["fog_samples_shadowed"] > 0
    flt = tracer("surf_lit", (2, 2, 2), "inside", vol=as_float(vol), t=t, S=S).frame()
    assert tr.framebuffer(False).any()
    assert (bits(tr.framebuffer(False)) == bits(flt.framebuffer(False))).all()
    for a, b in zip(tr.adapters, flt.adapters):
        assert (bits(a.ao_grid()) == bits(b.ao_grid())).all() and ((a.ao_grid() > 0) & (a.ao_grid() < 1)).any()
    for key in DEVICE_KEYS + ("ao_rays",):
        assert st[key] == flt.stats()[key], key
    assert tr.ao_stats["samples_marched"] == flt.ao_stats["samples_marched"] and tr.ao_stats["crossings"] == flt.ao_stats["crossings"]


@pytest.mark.parametrize("mode", aoc.MODES)
def test_clipped_frame(hip, mode):
    want, counters, plane = aoc.reference(mode, (2, 2, 2), "outside", clipped=True)
    depth = DepthPlane(fc.FILM[0], fc.FILM[1]).upload(plane)
    tr = tracer(mode, (2, 2, 2), "outside", moved=False).frame(depth)
    got, st = tr.framebuffer(False).copy(), tr.stats()
    assert st["ao"] == 1 and st["samples_shaded"] > 0
    assert (bits(got) == bits(want)).all()
    for key in COUNTER_KEYS:
        assert st[key] == counters[key], key
    assert (bits(got) != bits(tr.frame().framebuffer(False))).any()  # the clip shows
    assert tr.stats()["ao_bakes"] == 1  # (the camera's clip does not touch the grid)


def test_mixed_frame(hip):
    """The volume's surfaces and lit fog with baked ambient occlusion, clipped at the scene's depth plane and composited over the meshes."""
    w, h = 64, 48
    cam = scenes.Camera((0.0, 0.1, 0.3), (0.0, 0.1, -0.3), (0.0, 1.0, 0.0), float(F(45.0 * np.pi / 180.0)), w, h)
    scene = scenes.bunny_scene(w, h)
    vol = scenes.mesh_in_volume(scene, scenes.sphere_volume(32), fill=0.6)
    parts = scenes.split_volume(vol, 2, 2, 2)
    t = tf("ramp")
    S = sc.Surfaces([0.3, 0.5], [], 0.6, swc.LIGHTS)
    mt = MixedTracer(scene, parts, cam, t, sampling_rate=1.0, shadows=True, fog_shadows=True, ao=True, ao_dirs=6)  # (the radius: 16 lattice steps)
    mt.set_surfaces(S.iso, S.planes, float(S.opacity)).set_lights(list(zip(S.lpos, S.lcol))).set_shading(True)
    mt.frame()
    st = mt.volume.stats()
    assert st["ao"] == 1 and st["shadow_rays"] > 0 and st["samples_shaded"] > 0 and mt.volume.calls == 1 and st["ao_bakes"] == 1 and st["light_bakes"] == 1
    depth = mt.depth.download().copy()
    mesh = NativeTracer(scene)().framebuffer(False)
    m = fc.matrix(False)
    minv = scenes.instance_matrices(m)[0]
    bricks = [vc.Brick(b, t, 1.0) for b in parts]
    lo, hi = fc.world_boxes(parts, m)
    wlo, whi = fc.world_boxes([vol], m)
    whole = vc.Brick(vol, t, 1.0)
    G, _ = fg.grid(whole, wlo, whi, m, minv, S, 1)
    AO = ao.grid(whole, m, minv, S, scenes.ao_directions(6), F(16) * whole.dt, 1)
    assert all((bits(a.ao_grid()) == bits(ao.brick_plane(AO, type("B", (), {"off": a.offset, "n": a.counts})))).all() for a in mt.volume.adapters)
    fog, counters = ao.frame(bricks, lo, hi, minv, cam, S, lc.SHADE_GRADIENT, G, None, AO, depth, swc.BIAS)
    want = cc.composite(fog, mesh, depth)
    assert (bits(mt.framebuffer(False)) == bits(want)).all()
    for key in ("shadow_rays", "shadow_brick_visits", "shadow_crossings", "samples_shaded"):
        assert st[key] == counters[key], key
    assert np.isfinite(depth).sum() > 100 and ((AO > 0) & (AO < 1)).mean() > 0.5


@pytest.mark.parametrize("mode", aoc.MODES)
def test_central_bricks_under_the_flag(hip, mode):
    """CENTRAL bricks under GVT_HIP_VOLUME_ALLOW_CENTRAL: the alpha plane and the counters are the CELL frame's, the grid is the CELL
    bricks' (the bake reads no gradient), and with the grid of ones the frame is the device's CENTRAL fog-shadowed frame."""
    parts = scenes.split_volume(fc.volume(), 2, 2, 2, ghosts=True)
    tr = tracer(mode, (2, 2, 2), "inside", parts=parts, central=True)
    tr.set_gradient("central").frame()
    got, st = tr.framebuffer(False).copy(), tr.stats()
    assert st["ao"] == 1 and st["features"] == FEATURES[mode] | capi.FUSED_CENTRAL and grid_matches(tr, aoc.ao_grid(mode, aoc.CAMERAS["inside"])[0])
    cell = tr.set_gradient("cell").frame()
    cb, cst = cell.framebuffer(False).copy(), cell.stats()
    assert cst["features"] == FEATURES[mode] and (bits(cb[..., 3]) == bits(got[..., 3])).all() and (bits(cb[..., :3]) != bits(got[..., :3])).any()
    assert (bits(cb) == bits(aoc.reference(mode, (2, 2, 2), "inside")[0])).all()
    for key in DEVICE_KEYS:
        assert st[key] == cst[key], key
    assert cst["ao_bakes"] == 1  # (the gradient kind does not make the grid stale)
    ones = tracer(mode, (2, 2, 2), "inside", parts=scenes.split_volume(fc.volume(), 2, 2, 2, ghosts=True), central=True, steps=1.0)
    base = tracer(mode, (2, 2, 2), "inside", parts=scenes.split_volume(fc.volume(), 2, 2, 2, ghosts=True), central=True, ao_on=False)
    a, b = ones.set_gradient("central").frame().framebuffer(False), base.set_gradient("central").frame().framebuffer(False)
    assert ones.stats()["ao"] == 1 and (bits(a) == bits(b)).all() and (bits(a) != bits(got)).any()
    # without the flag the CENTRAL frame is refused, as its base is
    plain = tracer(mode, (2, 2, 2), "inside", parts=scenes.split_volume(fc.volume(), 2, 2, 2, ghosts=True)).set_gradient("central")
    with pytest.raises(capi.GvtHipError, match="central"):
        plain.frame()


# ---- currency, refusals, inert frames

def _upload_fb(fb, img):
    """Put an image into a framebuffer (the library has no host path into one: a plain copy through the runtime it is linked against)."""
    src = capi.f32(img)
    capi.synchronize()
    rt = C.CDLL("libamdhip64.so")
    rt.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert src.nbytes == fb.w * fb.hgt * 16
    assert rt.hipMemcpy(fb.device_ptr(), capi.ptr(src), src.nbytes, 1) == 0  # hipMemcpyHostToDevice


def _raw_frame(tr, adapters=None, m=None, flags=0, bias=aoc.BIAS, stats=None):
    """gvt_hip_volume_frame_ao on tr's top level, queues and framebuffer with other volumes, another matrix or other params."""
    cam = tr.camera
    adapters = tr.adapters if adapters is None else adapters
    n = len(adapters)
    pod = capi.CameraPod((C.c_float * 3)(*cam.eye), (C.c_float * 3)(*cam.focus), (C.c_float * 3)(*cam.up), cam.fov, cam.width, cam.height, 1, 1, 0.0)
    m1 = capi.f32(tr.m if m is None else m, 16)
    mm = np.ascontiguousarray(np.tile(m1, n), F)
    minv = np.ascontiguousarray(np.tile(scenes.instance_matrices(m1)[0], n), F)
    params = capi.VolumeAoFrameParams(flags, bias)
    arr = (C.c_void_p * n)(*[a.h for a in adapters])
    return capi.load().gvt_hip_volume_frame_ao(tr.top.h, arr, capi.ptr(mm), capi.ptr(minv), C.c_size_t(n), C.byref(pod), tr._arr(tr.queues), tr.fb.h, None,
                                               C.byref(params), None if stats is None else C.byref(stats))


def _params(flags=0, bias=1, dirs=None, radius=None, n_dirs=None):
    dirs = aoc.dirs() if dirs is None else np.asarray(dirs, F).reshape(-1, 3)
    p = capi.VolumeAoParams(flags, bias, len(dirs) if n_dirs is None else n_dirs, float(aoc.radius()) if radius is None else radius)
    for i, d in enumerate(dirs):
        p.dirs[i][:] = [float(x) for x in d]
    return p


def _raw_bake(adapters, m, params, stats=None):
    n = len(adapters)
    m1 = capi.f32(m, 16)
    mm = np.ascontiguousarray(np.tile(m1, n), F)
    minv = np.ascontiguousarray(np.tile(scenes.instance_matrices(m1)[0], n), F)
    arr = (C.c_void_p * max(n, 1))(*[a.h for a in adapters])
    return capi.load().gvt_hip_volume_ao_grid_bake(arr, capi.ptr(mm), capi.ptr(minv), C.c_size_t(n), None if params is None else C.byref(params),
                                                   None if stats is None else C.byref(stats))


def test_a_stale_grid_is_refused_until_the_rebake(hip):
    pattern = np.random.default_rng(11).random((fc.FILM[1], fc.FILM[0], 4)).astype(F)
    split = (2, 2, 2)
    parts = fc.bricks_of(fc.volume(), split)
    S, on, table = swc.surfaces("main", "surf_lit")
    lights = list(zip(S.lpos, S.lcol))
    want = aoc.reference("surf_lit", split, "inside")[0]
    tr = tracer("surf_lit", split, "inside").frame()
    assert (bits(tr.framebuffer(False)) == bits(want)).all() and want.any()
    a = tr.adapters[3]
    calls = {"update_samples": lambda: a.update_samples(parts[3].data), "set_transfer": lambda: a.set_transfer(table),
             "set_surfaces": lambda: a.set_surfaces(S.iso, S.planes, float(S.opacity))}
    bakes = 1
    for name, call in calls.items():
        call()  # on ONE brick, behind the tracer's back: the same values, and the grid is stale all the same
        assert a.ao_grid_info()["present"] == 1 and a.ao_grid_info()["current"] == 0, name
        assert all(b.ao_grid_info()["current"] == 1 for b in tr.adapters if b is not a)
        tr.rebake()  # (the light grids went stale too: baked again, so that the AO grid alone stands between the frame and the kernel)
        kept = a.ao_grid().copy()  # (a stale grid can still be downloaded)
        _upload_fb(tr.fb, pattern)
        with pytest.raises(capi.GvtHipError, match=r"\(-1\)") as e:
            tr.frame()
        assert "ao grid" in str(e.value), (name, str(e.value))
        assert (bits(tr.framebuffer(False)) == bits(pattern)).all() and all(len(q) == 0 for q in tr.queues), name
        tr.rebake_ao()
        bakes += 1
        assert (bits(a.ao_grid()) == bits(kept)).all()
        assert (bits(tr.frame().framebuffer(False)) == bits(want)).all(), name
        assert tr.stats()["ao_bakes"] == bakes
    # lights, shading and the gradient kind: the grid stays current (the light grids go stale with the lights: the tracer bakes THEM again)
    a.set_lights(lights, float(S.ka), float(S.kd))
    a.set_shading(False)
    a.set_shading(True)
    a.set_gradient("cell")
    assert all(b.ao_grid_info()["current"] == 1 for b in tr.adapters)
    tr.rebake()
    assert (bits(tr.frame().framebuffer(False)) == bits(want)).all() and tr.stats()["ao_bakes"] == bakes
    tr.set_lights(lights, float(S.ka), float(S.kd)).set_shading(False).set_shading(True)
    assert (bits(tr.frame().framebuffer(False)) == bits(want)).all() and tr.stats()["ao_bakes"] == bakes and tr.stats()["light_bakes"] > 1
    # the tracer's own setters: update(), set_surfaces() and set_transfer() bake again on the next frame
    tr.set_transfer(table)
    assert (bits(tr.frame().framebuffer(False)) == bits(want)).all() and tr.stats()["ao_bakes"] == bakes + 1
    tr.update(parts).set_surfaces(S.iso, S.planes, float(S.opacity))
    assert (bits(tr.frame().framebuffer(False)) == bits(want)).all() and tr.stats()["ao_bakes"] == bakes + 2
    # another matrix, and one brick fewer (on a top level of its own)
    _upload_fb(tr.fb, pattern)
    assert _raw_frame(tr, m=fc.matrix(True)) == -1 and "grid" in capi.last_error(), capi.last_error()
    assert (bits(tr.framebuffer(False)) == bits(pattern)).all()
    fewer = tracer("surf_lit", split, "inside", parts=fc.bricks_of(fc.volume(), split)[:7])
    _upload_fb(fewer.fb, pattern)
    assert _raw_frame(fewer, adapters=tr.adapters[:7]) == -1 and "grid" in capi.last_error(), capi.last_error()
    assert (bits(fewer.framebuffer(False)) == bits(pattern)).all()
    # the frame's own refusals: unknown bits, the AMR flag, the bias; then a frame without stats
    for flags, bias, word in ((16, aoc.BIAS, "flag"), (capi.VOLUME_ALLOW_AMR, aoc.BIAS, "AMR"), (1, aoc.BIAS, "flag"), (0, 0, "bias"), (0, 65, "bias")):
        _upload_fb(tr.fb, pattern)
        assert _raw_frame(tr, flags=flags, bias=bias) == -1 and word in capi.last_error(), capi.last_error()
        assert (bits(tr.framebuffer(False)) == bits(pattern)).all()
    assert _raw_frame(tr) == 0  # stats may be NULL
    assert (bits(tr.framebuffer(False)) == bits(want)).all()
    # the mesh flag without an occluder grid: the base frame's refusal
    _upload_fb(tr.fb, pattern)
    assert _raw_frame(tr, flags=capi.VOLUME_AO_MESH) == -1 and "occluder grid" in capi.last_error(), capi.last_error()
    assert (bits(tr.framebuffer(False)) == bits(pattern)).all()


def test_refused_bakes_keep_the_old_grid(hip):
    split = (2, 2, 2)
    m = fc.matrix(False)
    tr = tracer("surf_lit", split, "inside", parts=scenes.split_volume(fc.volume(), *split, ghosts=True)).rebake_ao()
    before = [a.ao_grid().copy() for a in tr.adapters]
    info = [a.ao_grid_info() for a in tr.adapters]

    def refused(adapters, params, word, matrix=m):
        st = capi.VolumeAoStats(rays=77)
        assert _raw_bake(adapters, matrix, params, st) == -1
        assert word in capi.last_error(), capi.last_error()
        assert st.rays == 77

    refused(tr.adapters, _params(n_dirs=0), "n_dirs")
    refused(tr.adapters, _params(n_dirs=33), "n_dirs")
    refused(tr.adapters, _params(dirs=[(1.0, 0.0, 0.0), (0.0, 0.0, 0.0)]), "direction 1")
    refused(tr.adapters, _params(dirs=[(np.nan, 0.0, 0.0)]), "direction 0")
    refused(tr.adapters, _params(dirs=[(np.inf, 0.0, 0.0)]), "direction 0")
    refused(tr.adapters, _params(radius=float("nan")), "radius")
    refused(tr.adapters, _params(radius=0.0), "radius")
    refused(tr.adapters, _params(radius=-1.0), "radius")
    refused(tr.adapters, _params(flags=capi.VOLUME_ALLOW_AMR), "AMR")
    refused(tr.adapters, _params(flags=1), "flag")
    refused(tr.adapters, _params(bias=0), "bias")
    refused(tr.adapters, _params(bias=65), "bias")
    refused(tr.adapters, None, "null")
    assert capi.load().gvt_hip_volume_ao_grid_bake(None, None, None, C.c_size_t(0), None, None) == -1 and "null" in capi.last_error()
    refused(tr.adapters[:7], _params(), "tile")  # seven of the eight bricks
    refused(tr.adapters + tr.adapters[:1], _params(), "tile")  # one brick twice
    assert _raw_bake(tr.adapters[:0], m, _params()) == -1  # no brick at all
    tr.set_gradient("central")  # CENTRAL on a frame with an isovalue, without the flag
    refused(tr.adapters, _params(), "central")
    assert _raw_bake(tr.adapters, m, _params(flags=capi.VOLUME_ALLOW_CENTRAL)) == 0  # ... and with it: the same grid
    tr.set_gradient("cell")
    for a, g, i in zip(tr.adapters, before, info):
        assert a.ao_grid_info() == i and i["current"] == 1 and (bits(a.ao_grid()) == bits(g)).all()
    # no light at all: the AO bake needs none
    dark = tracer("surf_lit", split, "inside")
    dark.set_lights([])
    assert _raw_bake(dark.adapters, m, _params()) == 0
    assert all((bits(a.ao_grid()) == bits(g)).all() for a, g in zip(dark.adapters, before))
    # a brick with subgrids (it takes neither surfaces nor shading: a frame of plain bricks, one of them refined)
    am = tracer("lit", split, "inside").rebake_ao()
    kept = am.adapters[0].ao_grid().copy()
    am.set_shading(False)
    b = fc.bricks_of(fc.volume(), split)[0]
    scenes.refine(b, np.asarray(b.offset) + 1, (2, 2, 2), 2, seed=5)
    am.adapters[0].set_subgrids(b.subgrids)
    assert am.adapters[0].ao_grid_info()["current"] == 0  # (_set_subgrids makes the grid stale)
    refused(am.adapters, _params(), "subgrids")
    assert (bits(am.adapters[0].ao_grid()) == bits(kept)).all()
    # release: the grid is gone, and a second release is no error
    am.adapters[1].ao_grid_release()
    am.adapters[1].ao_grid_release()
    assert am.adapters[1].ao_grid_info() == {"present": 0, "current": 0, "n_dirs": 0, "bias": 0, "radius": 0.0, "bytes": 0}
    with pytest.raises(capi.GvtHipError, match="no ao grid"):
        am.adapters[1].ao_grid()


def test_inert_frames_need_no_grid(hip):
    """No usable light, or neither surfaces nor effective lit shading: the base frame in every respect, ao = 0, nothing baked."""
    S, on, table = swc.surfaces("main", "surf_lit")
    # (1) no usable light
    tr = tracer("surf_lit", (2, 2, 2), "inside")
    tr.set_lights([((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))], float(S.ka), float(S.kd))
    base = tracer("surf_lit", (2, 2, 2), "inside", ao_on=False)
    base.set_lights([((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))], float(S.ka), float(S.kd))
    got, want = tr.frame(), base.frame()
    assert got.stats()["ao"] == 0 and got.stats()["ao_bakes"] == 0 and all(a.ao_grid_info()["present"] == 0 for a in tr.adapters)
    assert want.framebuffer(False).any() and (bits(got.framebuffer(False)) == bits(want.framebuffer(False))).all()
    for key in DEVICE_KEYS + ("shadowed",):
        assert got.stats()[key] == want.stats()[key], key
    # (2) lights, but no surfaces and shading off
    tr = tracer("lit", (2, 2, 2), "inside").set_shading(False)
    base = tracer("lit", (2, 2, 2), "inside", ao_on=False).set_shading(False)
    got, want = tr.frame(), base.frame()
    assert got.stats()["ao"] == 0 and got.stats()["shadowed"] == 0 and got.stats()["ao_bakes"] == 0
    assert want.framebuffer(False).any() and (bits(got.framebuffer(False)) == bits(want.framebuffer(False))).all()
    # (3) no lights at all
    tr = tracer("surf_lit", (2, 2, 2), "inside")
    tr.set_lights([])
    st = capi.VolumeAoFrameStats()
    assert _raw_frame(tr, stats=st) == 0 and st.ao == 0 and st.base.mesh_shadowed == 0 and st.base.fog.shadowed == 0 and tr.framebuffer(False).any()


def test_a_volume_that_holds_a_grid_renders_as_before(hip):
    tr = tracer("surf_lit", (2, 2, 2), "inside", mesh=True).frame()
    assert all(a.ao_grid_info()["current"] == 1 for a in tr.adapters) and tr.stats()["ao"] == 1
    tr.ao = False  # gvt_hip_volume_frame_mesh_shadowed
    want = tracer("surf_lit", (2, 2, 2), "inside", mesh=True, ao_on=False).frame()
    assert (bits(tr.frame().framebuffer(False)) == bits(want.framebuffer(False))).all() and want.framebuffer(False).any()
    tr.mesh_shadows = False  # gvt_hip_volume_frame_fog_shadowed
    want = tracer("surf_lit", (2, 2, 2), "inside", ao_on=False).frame()
    assert (bits(tr.frame().framebuffer(False)) == bits(want.framebuffer(False))).all()
    for key in DEVICE_KEYS:
        assert tr.stats()[key] == want.stats()[key], key
    tr.fog_shadows = False  # gvt_hip_volume_frame_shadowed
    want = tracer("surf_lit", (2, 2, 2), "inside", fog=False).frame()
    assert (bits(tr.frame().framebuffer(False)) == bits(want.framebuffer(False))).all()
    tr.shadows = False  # gvt_hip_volume_frame_fused_shaded
    plain = tracer("surf_lit", (2, 2, 2), "inside", shadows=False).frame()
    assert (bits(tr.frame().framebuffer(False)) == bits(plain.framebuffer(False))).all() and tr.stats()["fused"] == 1
    assert (bits(plain.framebuffer(False)) != bits(want.framebuffer(False))).any()
    assert all(a.ao_grid_info() == {"present": 1, "current": 1, "n_dirs": 6, "bias": 1, "radius": float(aoc.radius()), "bytes": 4 * int(np.prod(a.counts))} for a in tr.adapters)


def test_the_python_surface(hip):
    cam, t = fc.camera("inside", False), tf("cool")
    parts = fc.bricks_of(fc.volume(), (2, 2, 2))
    for kw in ({}, {"shadows": True}):
        with pytest.raises(ValueError, match="ao needs"):
            VolumeTracer(parts, cam, t, ao=True, **kw)
    with pytest.raises(ValueError, match="shadow_amr"):
        VolumeTracer(parts, cam, t, shadows=True, fog_shadows=True, shadow_amr=True, ao=True)
    with pytest.raises(ValueError, match="directions"):
        VolumeTracer(parts, cam, t, shadows=True, fog_shadows=True, ao=True, ao_dirs=33)
    with pytest.raises(ValueError, match="ao needs"):
        VolumeDomainTracer(parts, [0] * 8, cam, t, None, None, "cpu", ao=True)
    d = scenes.ao_directions(16)
    assert d.dtype == F and d.shape == (16, 3) and np.abs(np.linalg.norm(d.astype(np.float64), axis=1) - 1).max() < 1e-6 and abs(float(d[:, 2].sum())) < 1e-6
    tr = VolumeTracer(parts, cam, t, sampling_rate=fc.RATE, shadows=True, fog_shadows=True, ao=True)  # 16 directions, 16 lattice steps
    S, on, _ = swc.surfaces("main", "lit")
    dress(tr, S, on).frame()
    st = tr.stats()
    dt = tr.adapters[0].info()["dt"]
    assert st["ao"] == 1 and st["ao_bakes"] == 1 and st["ao_rays"] == 16 * sum(int(np.prod(a.counts)) for a in tr.adapters)
    assert all(a.ao_grid_info()["n_dirs"] == 16 and a.ao_grid_info()["radius"] == float(F(16.0 * dt)) for a in tr.adapters)
