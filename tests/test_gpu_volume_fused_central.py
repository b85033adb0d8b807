"""GVT_HIP_FUSED_CENTRAL and GVT_HIP_VOLUME_ALLOW_CENTRAL on the device: the CENTRAL instantiations of the shaded, shadowed, fog-shadowed
and mesh-shadowed fused kernels (csrc/volume_fused_*.inc).  The fused CENTRAL frame against the loop's CENTRAL frame, bit for bit, over
brickings whose ghost slabs differ from brick to brick and over bricks one cell thick; the three shadowed frames against the numpy
checker (tests/volume_central_shadow_checker.py; tests/test_volume_fused_central_host.py pins it on the CPU) and against their CELL
frames, whose alpha plane and counters they must share; the bakes under the flag; typed voxels; grids that are not finite; the clipped
mixed frame; the opt-in and the refusals.  Everything here uses VolumeTracer(..., fused_central=True) on bricks that carry their ghosts."""
import ctypes as C

import numpy as np
import pytest

from gravit_amd import capi, scenes
from gravit_amd.adapter import TransferFunction
from gravit_amd.scheduler import MixedTracer, NativeTracer, VolumeTracer
from tests import volume_central_cases as ccs
from tests import volume_central_shadow_checker as cs
from tests import volume_clip_checker as cc
from tests import volume_fog_shadow_cases as fgc
from tests import volume_fused_cases as fc
from tests import volume_mesh_shadow_cases as mc
from tests import volume_shadow_cases as swc
from tests import volume_smooth_cases as smc
from tests import volume_smooth_checker as sm
from tests import volume_surface_checker as sc
from tests.volume_common import tf

pytestmark = pytest.mark.gpu

F = np.float32
BOTH = capi.FUSED_SURFACES | capi.FUSED_LIT
FEATURES = {"lit": capi.FUSED_LIT, "surf_lit": BOTH, "surf": capi.FUSED_SURFACES, "surfaces": capi.FUSED_SURFACES, "both": BOTH}
SHADOW_KEYS = ("shadow_rays", "shadow_brick_visits", "shadow_crossings")
CAMERA_KEYS = ("brick_visits", "rays_deposited", "crossings_rendered", "samples_shaded")
DEVICE_KEYS = SHADOW_KEYS + CAMERA_KEYS + ("samples_marched", "samples_gathered", "shadow_samples_marched", "shadow_samples_gathered")
GRIDS = {"fused": (fc.volume, lambda: fc.camera("outside", False), fc.RATE), "smooth": (smc.volume, smc.camera, smc.RATE)}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def dress(tr, S, on, kind="central"):
    tr.set_surfaces(S.iso, S.planes, float(S.opacity)) if len(S) else tr.set_surfaces()
    tr.set_lights(list(zip(S.lpos, S.lcol)), float(S.ka), float(S.kd))
    tr.set_shading(on)
    return tr.set_gradient(kind)


def loop_frame(tr, depth=None):
    """The same tracer's frame through the per-brick loop: (framebuffer, crossings rendered, samples shaded, central marches) of that frame."""
    before = tr._brick_stats()
    keep = tr.fused, tr.shadows
    tr.fused, tr.shadows = False, False
    fb = tr.frame(depth).framebuffer(False).copy()
    tr.fused, tr.shadows = keep
    after = tr._brick_stats()
    return fb, tuple(after[k] - before[k] for k in ("crossings_rendered", "samples_shaded", "central_marches"))


# ---- 1. the fused CENTRAL frame equals the loop's

@pytest.mark.parametrize("skip", [True, False])
@pytest.mark.parametrize("split", fc.SPLITS)
@pytest.mark.parametrize("grid", sorted(GRIDS))
def test_fused_central_frame_equals_the_loops(hip, grid, split, skip):
    vol, cam, rate = GRIDS[grid]
    tr = VolumeTracer(ccs.parts_of(vol(), split), cam(), smc.table("dense"), sampling_rate=rate, skip=skip, fused=True, fused_shaded=True, fused_central=True)
    for table in ("dense", "spikes"):
        for a in tr.adapters:
            a.set_transfer(smc.table(table))
        for setup in ("surfaces", "lit", "both"):
            S, mode = smc.SETUPS[setup]
            dress(tr, S(), mode == sm.SHADE_GRADIENT)
            got, st = tr.frame().framebuffer(False).copy(), tr.stats()
            want, (crossings, shaded, marches) = loop_frame(tr)
            assert st["fused"] == 1 and st["adapter_calls"] == 1 and st["features"] == FEATURES[setup] | capi.FUSED_CENTRAL, (table, setup)
            assert got.any() and (bits(got) == bits(want)).all(), (table, setup)
            assert st["crossings_rendered"] == crossings and st["samples_shaded"] == shaded and crossings + shaded > 0, (table, setup)
            assert marches > 0  # the loop did shade with CENTRAL (central_marches counts ITS launches; the fused frame moves no brick's counter)
            # without the bit: the loop, and the same image
            tr.fused_allow = BOTH
            off, so = tr.frame().framebuffer(False), tr.stats()
            tr.fused_allow = BOTH | capi.FUSED_CENTRAL
            assert so["fused"] == 0 and so["adapter_calls"] >= 1 and (bits(off) == bits(want)).all(), (table, setup)
    cell = dress(tr, smc.surfaces(), True, "cell").frame()
    assert cell.stats()["fused"] == 1 and cell.stats()["features"] == BOTH and (bits(cell.framebuffer(False)) != bits(got)).any()  # the kind shows


# ---- 2. bricks one cell thick: both neighbours of a vertex along the axis are ghost samples

@pytest.mark.parametrize("axis", [0, 1, 2])
def test_bricks_one_cell_thick(hip, axis):
    counts, split = list(smc.COUNTS), [1, 1, 1]
    counts[axis], split[axis] = 10, 9
    vol, S = smc.volume(tuple(counts)), smc.surfaces()
    parts = ccs.parts_of(vol, split)
    assert len(parts) == 9 and all(int(p.counts[axis]) == 2 for p in parts)
    tr = dress(VolumeTracer(parts, smc.camera(), smc.table("dense"), sampling_rate=smc.RATE, fused=True, fused_shaded=True, fused_central=True), S, True)
    got, st = tr.frame().framebuffer(False).copy(), tr.stats()
    want, (crossings, shaded, _) = loop_frame(tr)
    assert st["fused"] == 1 and st["features"] == BOTH | capi.FUSED_CENTRAL
    assert got.any() and (bits(got) == bits(want)).all()
    assert st["crossings_rendered"] == crossings > 0 and st["samples_shaded"] == shaded > 0
    # a shadowed frame in the same bricking against the one-brick frame
    frames = []
    for p in (parts, ccs.parts_of(vol, (1, 1, 1))):
        sh = dress(VolumeTracer(p, smc.camera(), smc.table("dense"), sampling_rate=smc.RATE, shadows=True, fused_central=True), S, True).frame()
        assert sh.stats()["shadowed"] == 1 and sh.stats()["shadow_rays"] > 0 and sh.stats()["features"] == BOTH | capi.FUSED_CENTRAL
        frames.append(sh.framebuffer(False).copy())
    assert (bits(frames[0]) == bits(frames[1])).all() and (bits(frames[0]) != bits(got)).any()


# ---- 3. / 4. the shadowed frames

def tracer(frame, mode, split, where, moved=None, skip=True, kind="central", kd=0.6, central=True, vol=None, native=False, t=None, S=None, which="case"):
    """The tracer of a case of tests/volume_central_cases.py.  frame: "plain", "shadow", "fog" or "mesh"."""
    moved = swc.CAMERAS[where] if moved is None else moved
    S0, on, table = swc.surfaces("main", mode, kd=kd)
    parts = ccs.parts_of(fc.volume() if vol is None else vol, split)
    tr = VolumeTracer(parts, fc.camera(where, moved), table if t is None else t, m=fc.matrix(moved), sampling_rate=fc.RATE, skip=skip, native=native, fused=True,
                      fused_shaded=True, shadows=frame != "plain", shadow_bias=swc.BIAS, fog_shadows=frame in ("fog", "mesh"), fog_bias=fgc.GRID_BIAS,
                      mesh_shadows=frame == "mesh", fused_central=central)
    dress(tr, S0 if S is None else S, on, kind)
    if frame == "mesh":
        tr.bake_occluders({"case": lambda: mc.scene(moved), "wall": lambda: mc.wall_scene(moved)}[which]())
    return tr


@pytest.mark.parametrize("where", sorted(swc.CAMERAS))
@pytest.mark.parametrize("split", fc.SPLITS)
def test_shadowed_central_frame_has_the_checkers_bits_and_counts(hip, split, where):
    want, counters, _ = ccs.reference("shadow", "surf", split, where)
    tr = tracer("shadow", "surf", split, where).frame()
    got, st = tr.framebuffer(False).copy(), tr.stats()
    assert st["shadowed"] == 1 and st["fused"] == 1 and st["adapter_calls"] == 1 and st["features"] == capi.FUSED_SURFACES | capi.FUSED_CENTRAL
    assert got.any() and (bits(got) == bits(want)).all()
    for key in SHADOW_KEYS + CAMERA_KEYS:
        assert st[key] == counters[key], key
    if split == (4, 4, 4):  # the shadow rays do leave the camera ray's brick: a ghost pointer that is not restored would show
        assert st["shadow_brick_visits"] > st["shadow_rays"] > 0
    # alpha and every counter are the CELL frame's
    cell = tr.set_gradient("cell").frame()
    cb, cst = cell.framebuffer(False), cell.stats()
    assert cst["features"] == capi.FUSED_SURFACES and (bits(cb[..., 3]) == bits(got[..., 3])).all() and (bits(cb[..., :3]) != bits(got[..., :3])).any()
    for key in DEVICE_KEYS:
        assert st[key] == cst[key], key


@pytest.mark.parametrize("where", sorted(swc.CAMERAS))
def test_the_cut_and_the_skipping_do_not_show(hip, where):
    frames = [tracer("shadow", "surf_lit", s, where).frame().framebuffer(False).copy() for s in fc.SPLITS]
    frames.append(tracer("shadow", "surf_lit", (2, 2, 2), where, skip=False).frame().framebuffer(False).copy())
    assert frames[0].any() and (bits(frames[0]) == bits(ccs.reference("shadow", "surf_lit", (1, 1, 1), where)[0])).all()
    for f in frames[1:]:
        assert (bits(f) == bits(frames[0])).all()


def test_identity_and_occluder_properties(hip):
    """With no occluder the bits are the fused CENTRAL frame's; where every light is blocked, those of the frame rendered with kd = 0.
    tests/volume_shadow_cases.py's two cases have slice planes alone, which leaves the kind inert; an isovalue no sample reaches (2: the
    grid lies in [0, 1]) is added, so the CENTRAL instantiations run and no crossing changes."""

    def case_tracer(case, shadows, kd=0.6):
        S, on, table = swc.surfaces(case, kd=kd)
        S = sc.Surfaces([2.0], S.planes, S.opacity, list(zip(S.lpos, S.lcol)), ka=S.ka, kd=S.kd)
        tr = VolumeTracer(ccs.parts_of(fc.volume(), (2, 2, 2)), fc.camera("outside", False), table, m=fc.matrix(False), sampling_rate=fc.RATE, fused=True,
                          fused_shaded=True, shadows=shadows, shadow_bias=swc.BIAS, fused_central=True)
        return dress(tr, S, on)

    got = case_tracer("identity", True).frame()
    plain = case_tracer("identity", False).frame()
    assert got.stats()["features"] == plain.stats()["features"] == capi.FUSED_SURFACES | capi.FUSED_CENTRAL
    assert got.stats()["shadowed"] == 1 and got.stats()["shadow_rays"] > 500 and got.stats()["shadow_crossings"] == 0
    assert got.framebuffer(False).any() and (bits(got.framebuffer(False)) == bits(plain.framebuffer(False))).all()
    _, _, details, _ = swc.reference("occluder", (2, 2, 2), "outside", moved=False)
    has, dark = swc.fully_shadowed(details, fc.FILM[0] * fc.FILM[1])
    g = bits(case_tracer("occluder", True).frame().framebuffer(False)).reshape(-1, 4)
    a = bits(case_tracer("occluder", False, kd=0.0).frame().framebuffer(False)).reshape(-1, 4)
    p = bits(case_tracer("occluder", False).frame().framebuffer(False)).reshape(-1, 4)
    assert dark.sum() > 250 and (g[dark] == a[dark]).all() and (g[dark] != p[dark]).any(axis=-1).all() and (g[has & ~dark] == p[has & ~dark]).all()


@pytest.mark.parametrize("split", [(1, 1, 1), (2, 2, 2)])
def test_no_occluder_with_isovalues_and_lit_fog(hip, split):
    """No occluder, on a frame whose crossed isovalues and fog samples ARE shaded by the central gradient: under bias 64 a shadow ray's
    first sample lies 63 lattice steps from its origin, further than the grid's diagonal (the smooth grid measures 1.0 x 1.1 x 0.9, its
    diagonal 1.74; dt = (1 / 18) / 1.3, so 63 dt = 2.69), and the direction has unit length: every shadow ray is cast, none meets a
    sample, every T_j = 1, and the bits are the fused CENTRAL frame's (test 1's)."""
    vol, S = smc.volume(), smc.surfaces()
    ext = (np.asarray(vol.counts, np.float64) - 1) * np.asarray(vol.spacing, np.float64)
    assert 63 * float(np.asarray(vol.spacing, np.float64).min()) / smc.RATE > float(np.sqrt((ext * ext).sum()))
    frames = {}
    for shadows in (False, True):
        tr = dress(VolumeTracer(ccs.parts_of(vol, split), smc.camera(), smc.table("dense"), sampling_rate=smc.RATE, fused=True, fused_shaded=True, shadows=shadows,
                                shadow_bias=64, fused_central=True), S, True).frame()
        frames[shadows] = tr.framebuffer(False).copy(), tr.stats()
    (plain, ps), (got, st) = frames[False], frames[True]
    assert st["shadowed"] == 1 and st["features"] == ps["features"] == BOTH | capi.FUSED_CENTRAL
    assert st["shadow_rays"] > 1000  # (every sample with a rendered crossing casts its two rays)
    assert st["shadow_brick_visits"] == st["shadow_crossings"] == st["shadow_samples_marched"] == 0
    assert st["crossings_rendered"] == ps["crossings_rendered"] > 0 and st["samples_shaded"] == ps["samples_shaded"] > 0
    assert got.any() and (bits(got) == bits(plain)).all()
    near = dress(VolumeTracer(ccs.parts_of(vol, split), smc.camera(), smc.table("dense"), sampling_rate=smc.RATE, shadows=True, fused_central=True), S, True).frame()
    assert (bits(near.framebuffer(False)) != bits(got)).any()  # (under the usual bias the shadows do show)


def test_every_light_blocked_with_isovalues(hip):
    """Every light blocked, on a frame whose isovalues and fog are shaded by CENTRAL: the mesh-shadowed frame baked behind a wall that
    blocks every light has the bits of the fused CENTRAL frame rendered with kd = 0."""
    fog = tracer("fog", "surf_lit", (2, 2, 2), "inside").frame().framebuffer(False).copy()
    tr = tracer("mesh", "surf_lit", (2, 2, 2), "inside", which="wall").frame()
    assert tr.stats()["mesh_shadowed"] == 1 and tr.stats()["occluder_rays_blocked"] > 0
    dark = tr.framebuffer(False).copy()
    ambient = tracer("plain", "surf_lit", (2, 2, 2), "inside", kd=0.0).frame().framebuffer(False)
    assert (bits(dark) == bits(ambient)).all() and (bits(dark) != bits(fog)).any()


@pytest.mark.parametrize("split", [(1, 1, 1), (2, 2, 2)])
@pytest.mark.parametrize("frame,mode", [("fog", "surf_lit"), ("fog", "lit"), ("mesh", "surf_lit"), ("mesh", "lit")])
def test_fog_and_mesh_shadowed_central_frames_have_the_checkers_bits(hip, frame, mode, split):
    """(mode "lit": no surfaces -- the lean kernels)"""
    want, counters, _ = ccs.reference(frame, mode, split, "inside")
    tr = tracer(frame, mode, split, "inside").frame()
    got, st = tr.framebuffer(False).copy(), tr.stats()
    assert st["shadowed"] == 1 and st["fused"] == 1 and st["features"] == FEATURES[mode] | capi.FUSED_CENTRAL and st["fog_samples_shadowed"] > 0
    assert st.get("mesh_shadowed", 0) == (1 if frame == "mesh" else 0)
    assert got.any() and (bits(got) == bits(want)).all()
    for key in SHADOW_KEYS + CAMERA_KEYS:
        assert st[key] == counters[key], key
    # set_gradient back and forth triggers no bake, the frame is accepted, and alpha and the counters are the CELL frame's
    bakes = st["light_bakes"], st.get("occluder_bakes", 0)
    cell = tr.set_gradient("cell").frame()
    cb, cst = cell.framebuffer(False).copy(), cell.stats()
    assert cst["features"] == FEATURES[mode] and (bits(cb[..., 3]) == bits(got[..., 3])).all() and (bits(cb[..., :3]) != bits(got[..., :3])).any()
    for key in DEVICE_KEYS + ("fog_samples_shadowed",):
        assert st[key] == cst[key], key
    back = tr.set_gradient("central").frame()
    assert (bits(back.framebuffer(False)) == bits(got)).all()
    assert (back.stats()["light_bakes"], back.stats().get("occluder_bakes", 0)) == bakes == (1, 1 if frame == "mesh" else 0)
    assert all(a.light_grid_info()["current"] == 1 for a in tr.adapters)


@pytest.mark.parametrize("frame,mode", [("fog", "surf_lit"), ("mesh", "lit")])
def test_the_cut_does_not_show_in_fog_and_mesh_frames(hip, frame, mode):
    frames = [tracer(frame, mode, s, "outside").frame().framebuffer(False).copy() for s in fc.SPLITS]
    assert frames[0].any()
    for f in frames[1:]:
        assert (bits(f) == bits(frames[0])).all()


def test_planes_baked_under_the_flag_are_the_cell_bricks_planes(hip):
    central = tracer("mesh", "surf_lit", (2, 2, 2), "outside").frame()
    cell = tracer("mesh", "surf_lit", (2, 2, 2), "outside", kind="cell", central=False).frame()
    assert central.stats()["light_bakes"] == cell.stats()["light_bakes"] == 1 and central.stats()["occluder_bakes"] == cell.stats()["occluder_bakes"] == 1
    G, usable = fgc.light_grid("surf_lit", True)
    for a, b in zip(central.adapters, cell.adapters):
        o, n = a.offset, a.counts
        for j in np.nonzero(usable)[0]:
            lg = a.light_grid(int(j))
            assert (bits(lg) == bits(b.light_grid(int(j)))).all() and (a.occluder_grid(int(j)) == b.occluder_grid(int(j))).all()
            assert (bits(lg) == bits(G[j, o[2]:o[2] + n[2], o[1]:o[1] + n[1], o[0]:o[0] + n[0]])).all()
    assert central.stats()["light_grid_rays"] == cell.stats()["light_grid_rays"] and central.stats()["occluder_rays_blocked"] == cell.stats()["occluder_rays_blocked"] > 0


# ---- 5. typed voxels with typed ghosts

@pytest.mark.parametrize("ty", ["uint8", "int16"])
def test_typed_voxels_with_typed_ghosts_answer_like_their_float_copy(hip, ty):
    vol = smc.volume()
    if ty == "uint8":
        data, rng = np.rint(vol.data * 255).astype(np.uint8), (0.0, 255.0)
    else:
        data, rng = np.rint((vol.data - 0.5) * 60000).astype(np.int16), (-30000.0, 30000.0)
    dense = smc.table("dense")
    t = TransferFunction(dense.cmap, dense.omap, rng)
    S = sc.Surfaces([rng[0] + (rng[1] - rng[0]) * v for v in smc.ISO], smc.PLANE, 0.5, smc.LIGHTS)
    for shadows in (False, True):
        frames = []
        for d, native in ((data, True), (data.astype(F), False)):
            parts = ccs.parts_of(scenes.VolumeData(d, vol.origin, vol.spacing), (2, 2, 2))
            assert all(g is None or g.dtype == d.dtype for g in parts[0].ghosts)
            tr = dress(VolumeTracer(parts, smc.camera(), t, sampling_rate=smc.RATE, native=native, fused=True, fused_shaded=True, shadows=shadows, fused_central=True), S, True)
            assert tr.adapters[0].sample_bytes == d.itemsize
            frames.append((tr.frame().framebuffer(False).copy(), tr.stats()))
        (a, sa), (b, sb) = frames
        assert sa["fused"] == 1 and sa["features"] == BOTH | capi.FUSED_CENTRAL and sa.get("shadowed", 0) == int(shadows)
        assert a.any() and (bits(a) == bits(b)).all()
        for key in CAMERA_KEYS + (SHADOW_KEYS if shadows else ()):
            assert sa[key] == sb[key], key
        assert sa["crossings_rendered"] > 0 and sa["samples_shaded"] > 0


# ---- 6. the grid that is not finite

def test_the_nonfinite_grid(hip):
    vol, S = smc.nonfinite_volume(), smc.surfaces()
    parts = ccs.parts_of(vol, (2, 1, 2))
    assert any(g is not None and not np.isfinite(g).all() for p in parts for g in p.ghosts)
    tr = dress(VolumeTracer(parts, smc.camera(), smc.table("dense"), sampling_rate=smc.RATE, fused=True, fused_shaded=True, fused_central=True), S, True)
    got, st = tr.frame().framebuffer(False).copy(), tr.stats()
    want, (crossings, shaded, _) = loop_frame(tr)
    assert st["fused"] == 1 and st["features"] == BOTH | capi.FUSED_CENTRAL
    assert (bits(got) == bits(want)).all() and st["samples_shaded"] == shaded > 1000 and st["crossings_rendered"] == crossings
    lit = dress(tr, smc.lit(), True).frame()  # (lit fog alone: a gradient of infinite length shades with S = 0, the colour stays finite)
    fog = lit.framebuffer(False).copy()
    assert lit.stats()["features"] == capi.FUSED_LIT | capi.FUSED_CENTRAL and (bits(fog) == bits(loop_frame(tr)[0])).all()
    assert np.isfinite(fog).all() and fog.any()


# ---- 7. the clipped frame, through MixedTracer

def _mixed(scene, parts, cam, t, S, **kw):
    mt = MixedTracer(scene, parts, cam, t, sampling_rate=1.0, fused=True, fused_shaded=True, fused_central=True, **kw)
    mt.set_surfaces(S.iso, S.planes, float(S.opacity)).set_lights(list(zip(S.lpos, S.lcol))).set_shading(True).set_gradient("central")
    return mt


def test_the_clipped_mixed_frame(hip):
    w, h = fc.FILM
    cam = scenes.Camera((0.0, 0.1, 0.3), (0.0, 0.1, -0.3), (0.0, 1.0, 0.0), float(F(45.0 * np.pi / 180.0)), w, h)
    scene = scenes.bunny_scene(w, h)
    vol = scenes.mesh_in_volume(scene, scenes.VolumeData(smc.volume((17, 17, 17)).data), fill=0.6)
    parts = ccs.parts_of(vol, (2, 1, 2))
    t, S = smc.table("dense"), sc.Surfaces([0.42, 0.58], [], 0.5, swc.LIGHTS)
    # the fused frame against the loop
    mt = _mixed(scene, parts, cam, t, S).frame()
    got, st = mt.framebuffer(False).copy(), mt.volume.stats()
    assert st["fused"] == 1 and st["features"] == BOTH | capi.FUSED_CENTRAL and np.isfinite(mt.depth.download()).sum() > 100
    mt.volume.fused = False
    assert (bits(mt.frame().framebuffer(False)) == bits(got)).all() and mt.volume.stats()["central_marches"] > 0 and got.any()
    # the mesh-shadowed frame against the checker
    ms = _mixed(scene, parts, cam, t, S, shadows=True, fog_shadows=True, mesh_shadows=True).frame()
    st = ms.volume.stats()
    assert st["mesh_shadowed"] == 1 and st["features"] == BOTH | capi.FUSED_CENTRAL and st["shadow_rays"] > 0 and st["occluder_rays_blocked"] > 0
    depth = ms.depth.download().copy()
    ident = fc.matrix(False)
    minv = scenes.instance_matrices(ident)[0]
    lo, hi = fc.world_boxes(parts, ident)
    whole = sm.Brick(ccs.parts_of(vol, (1, 1, 1))[0], t, 1.0)
    from tests import volume_fog_shadow_checker as fg
    from tests import volume_mesh_shadow_checker as mg

    G, _ = fg.grid(whole, whole.lo[None], whole.hi[None], ident, minv, S, 1)
    O, _, blocked = mg.occluders(whole, ident, ms.scene, S)
    assert st["occluder_rays_blocked"] >= blocked > 0  # (the bake counts a vertex that two bricks share once per brick)
    fog, counters = cs.frame([sm.Brick(p, t, 1.0) for p in parts], lo, hi, minv, cam, S, sm.SHADE_GRADIENT, cs.CENTRAL, G, O, depth, swc.BIAS)
    want = cc.composite(fog, NativeTracer(scene)().framebuffer(False), depth)
    assert (bits(ms.framebuffer(False)) == bits(want)).all()
    for key in SHADOW_KEYS + CAMERA_KEYS:
        assert st[key] == counters[key], key


# ---- 8. opt-in and refusals

def test_bricks_that_count_the_grid_differently_are_not_fused(hip):
    """The CENTRAL kernels take the global grid's size from the first brick: two bricks that agree on origin and spacing but not on
    global_counts (the first one counts one more layer along y, and holds a ghost layer beyond its +y face; the second one's +y face is
    on ITS boundary and has none) take the loop under fused_shaded and are refused by the shadowed frames and the bakes."""
    parts = ccs.parts_of(smc.volume(), (2, 1, 1))
    parts[0].global_counts = np.asarray(parts[0].global_counts).copy()
    parts[0].global_counts[1] += 1
    parts[0].ghosts[3] = np.ascontiguousarray(parts[0].data[:, -1, :])
    assert parts[1].ghosts[3] is None and parts[1].ghosts[0] is not None
    tr = dress(VolumeTracer(parts, smc.camera(), smc.table("dense"), sampling_rate=smc.RATE, fused=True, fused_shaded=True, fused_central=True), smc.surfaces(), True)
    got, st = tr.frame().framebuffer(False).copy(), tr.stats()
    assert st["fused"] == 0 and st["adapter_calls"] >= 2 and got.any() and (bits(got) == bits(loop_frame(tr)[0])).all()
    cell = tr.set_gradient("cell").frame()  # (the kind that reads no global count is fused as ever)
    assert cell.stats()["fused"] == 1 and cell.stats()["features"] == BOTH
    tr.set_gradient("central")
    pattern = np.random.default_rng(12).random((smc.camera().height, smc.camera().width, 4)).astype(F)
    tr.shadows = tr.fog_shadows = True
    for call in (tr.frame, tr.rebake):
        _upload_fb(tr.fb, pattern)
        with pytest.raises(capi.GvtHipError, match=r"\(-1\)") as e:
            call()
        assert "central" in str(e.value) and "global counts" in str(e.value), str(e.value)
        assert (bits(tr.framebuffer(False)) == bits(pattern)).all() and all(len(q) == 0 for q in tr.queues)
    tr.fog_shadows = False
    _upload_fb(tr.fb, pattern)
    with pytest.raises(capi.GvtHipError, match=r"\(-1\)") as e:
        tr.frame()
    assert "central" in str(e.value) and (bits(tr.framebuffer(False)) == bits(pattern)).all()


def _upload_fb(fb, img):
    """Put an image into a framebuffer (the library has no host path into one: a plain copy through the runtime it is linked against)."""
    src = capi.f32(img)
    capi.synchronize()
    rt = C.CDLL("libamdhip64.so")
    rt.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert src.nbytes == fb.w * fb.hgt * 16
    assert rt.hipMemcpy(fb.device_ptr(), capi.ptr(src), src.nbytes, 1) == 0  # hipMemcpyHostToDevice


@pytest.mark.parametrize("frame", ["shadow", "fog", "mesh"])
def test_the_flag_with_cell_bricks_changes_nothing(hip, frame):
    a = tracer(frame, "surf_lit", (2, 2, 2), "inside", kind="cell", central=True).frame()
    b = tracer(frame, "surf_lit", (2, 2, 2), "inside", kind="cell", central=False).frame()
    assert a.param_flags == capi.VOLUME_ALLOW_CENTRAL and b.param_flags == 0
    assert a.framebuffer(False).any() and (bits(a.framebuffer(False)) == bits(b.framebuffer(False))).all()
    sa, sb = a.stats(), b.stats()
    for key in DEVICE_KEYS + ("features", "fused", "shadowed", "adapter_calls", "fog_samples_shadowed", "light_bakes"):
        if key in sb:
            assert sa[key] == sb[key], key
    assert sa["features"] == BOTH


def _raw_shadowed(tr, flags):
    cam = tr.camera
    pod = capi.CameraPod((C.c_float * 3)(*cam.eye), (C.c_float * 3)(*cam.focus), (C.c_float * 3)(*cam.up), cam.fov, cam.width, cam.height, 1, 1, 0.0)
    m = np.ascontiguousarray(np.tile(tr.m, tr.n_inst), F)
    minv = np.ascontiguousarray(np.tile(tr.minv, tr.n_inst), F)
    params = capi.VolumeShadowParams(flags, swc.BIAS)
    return capi.load().gvt_hip_volume_frame_shadowed(tr.top.h, tr._arr(tr.adapters), capi.ptr(m), capi.ptr(minv), C.c_size_t(tr.n_inst), C.byref(pod), tr._arr(tr.queues),
                                                     tr.fb.h, None, C.byref(params), None)


def test_opt_in_and_refusals(hip):
    pattern = np.random.default_rng(11).random((fc.FILM[1], fc.FILM[0], 4)).astype(F)

    def refused(tr, word, call=None):
        _upload_fb(tr.fb, pattern)
        with pytest.raises(capi.GvtHipError, match=r"\(-1\)") as e:
            (call or tr.frame)()
        assert word in str(e.value), str(e.value)
        assert (bits(tr.framebuffer(False)) == bits(pattern)).all() and all(len(q) == 0 for q in tr.queues)

    # flags = 1 and flags = 3 are refused, flags = 2 is taken; unknown allow bits too
    tr = tracer("shadow", "surf", (2, 2, 2), "inside")
    want = tr.frame().framebuffer(False).copy()
    _upload_fb(tr.fb, pattern)
    for flags in (1, 3):
        assert _raw_shadowed(tr, flags) == -1 and "flag" in capi.last_error()
        assert (bits(tr.framebuffer(False)) == bits(pattern)).all()
    assert _raw_shadowed(tr, 2) == 0 and (bits(tr.framebuffer(False)) == bits(want)).all()
    tr.shadows, tr.fused_allow = False, 4 | BOTH | capi.FUSED_CENTRAL  # (bit 2 stays undefined)
    refused(tr, "allow")
    # without the flag the CENTRAL frame is refused as ever, by the frames and by the bakes
    for frame in ("shadow", "fog", "mesh"):
        off = tracer("shadow" if frame == "mesh" else frame, "surf_lit", (2, 2, 2), "inside", central=False)
        if frame == "mesh":
            off.fog_shadows = off.mesh_shadows = True
            refused(off, "central", lambda: off.bake_occluders(mc.scene(False)))
        refused(off, "central")
    # a frame that mixes CELL and CENTRAL bricks: the loop under fused_shaded, refused by the shadowed frames and the bakes
    mixed = tracer("plain", "surf_lit", (2, 2, 2), "inside")
    mixed.adapters[3].set_gradient("cell")
    got, st = mixed.frame().framebuffer(False).copy(), mixed.stats()
    assert st["fused"] == 0 and st["adapter_calls"] > 1 and (bits(got) == bits(loop_frame(mixed)[0])).all() and got.any()
    mixed.shadows = True
    refused(mixed, "central")
    mixed.fog_shadows = True
    refused(mixed, "central", mixed.rebake)
    assert mixed.light_bakes == 0 and all(a.light_grid_info()["present"] == 0 for a in mixed.adapters)
    mixed.mesh_shadows = True
    refused(mixed, "central", lambda: mixed.bake_occluders(mc.scene(False)))
    assert all(a.occluder_grid_info()["present"] == 0 for a in mixed.adapters)
    mixed.adapters[3].set_gradient("central")
    baked = mixed.rebake().bake_occluders(mc.scene(False)).frame()  # the same bricks, all CENTRAL again: accepted
    assert baked.stats()["mesh_shadowed"] == 1 and (bits(baked.framebuffer(False)) == bits(ccs.reference("mesh", "surf_lit", (2, 2, 2), "inside")[0])).all()
    # ... and a refused bake keeps the grids: they are still current
    grids = [a.light_grid(0).copy() for a in mixed.adapters]
    mixed.adapters[5].set_gradient("cell")
    refused(mixed, "central", mixed.rebake)
    assert all((bits(a.light_grid(0)) == bits(g)).all() and a.light_grid_info()["current"] == 1 for a, g in zip(mixed.adapters, grids))
    # AMR is refused as before
    amr = VolumeTracer(fc.bricks_of(fc.volume(), (2, 2, 2)), fc.camera("inside", False), tf("cool"), m=fc.matrix(False), sampling_rate=fc.RATE, shadows=True,
                       fused_central=True)
    S, on, _ = swc.surfaces("main", "surf")
    for a in amr.adapters[1:]:
        a.set_surfaces(S.iso, S.planes, float(S.opacity))
        a.set_lights(list(zip(S.lpos, S.lcol)))
    b = fc.bricks_of(fc.volume(), (2, 2, 2))[0]
    scenes.refine(b, np.asarray(b.offset) + 1, (2, 2, 2), 2, seed=5)
    amr.adapters[0].set_subgrids(b.subgrids)
    refused(amr, "subgrids")
