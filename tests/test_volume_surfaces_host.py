"""The volume surface contract on the host: the numpy checker (tests/volume_surface_checker.py) against its parent, against itself under
different brickings, against an analytic sphere and against hand-computed shading; and the new entry points in the binding."""
import ctypes as C
import os
import re

import numpy as np

from gravit_amd import capi, scenes
from gravit_amd.adapter import TransferFunction
from gravit_amd.layouts import RAY_DTYPE
from tests import volume_checker as vc
from tests import volume_surface_checker as sc
from tests.conftest import GOLDEN, ROOT

F = np.float32
CMAPS = os.path.join(GOLDEN, "colormaps")
IDENT = scenes.mat_translate_scale((0, 0, 0), (1, 1, 1))


def cool(omap):
    return TransferFunction(TransferFunction.read_map(os.path.join(CMAPS, "CoolWarm.cmap"), 4), np.asarray(omap, F), (0.0, 1.0))


THIN = [[0.0, 0.0], [1.0, 0.05]]
CLEAR = [[0.0, 0.0], [1.0, 0.0]]


def noise(n=26):
    vol = scenes.noise_volume(n, seed=5)
    vol.origin = np.array([-0.3, 0.05, -0.2], F)
    vol.spacing = np.array([1.0 / (n - 1), 1.1 / (n - 1), 0.9 / (n - 1)], F)
    return vol


def camera(w, h, eye=(1.9, 1.6, 2.4), focus=(0.2, 0.6, 0.25)):
    return scenes.Camera(eye, focus, (0.0, 1.0, 0.0), float(F(35.0 * np.pi / 180.0)), w, h)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def by_id(chunks):
    r = np.concatenate(chunks)
    return r[np.argsort(r["id"], kind="stable")]


def test_the_binding_declares_the_surface_entry_points():
    hdr = open(os.path.join(ROOT, "include", "gvt_hip.h")).read()
    for s in ("gvt_hip_volume_set_surfaces", "gvt_hip_volume_set_lights", "gvt_hip_volume_get_crossings"):
        assert s in capi.SYMBOLS and re.search(r"\b%s\s*\(" % s, hdr)
        assert hasattr(capi.load(), s)
    assert capi.RAY_SIDES == sc.SIDES == int(re.search(r"#define GVT_HIP_RAY_SIDES (0x[0-9a-f]+)", hdr).group(1), 16) == 0x20
    assert capi.VOLUME_MAX_SURFACES == sc.MAX_SURFACES == int(re.search(r"#define GVT_HIP_VOLUME_MAX_SURFACES (\d+)", hdr).group(1))
    assert capi.VOLUME_MAX_LIGHTS == sc.MAX_LIGHTS == int(re.search(r"#define GVT_HIP_VOLUME_MAX_LIGHTS (\d+)", hdr).group(1))
    assert int(re.search(r"#define GVT_HIP_ABI_VERSION (\d+)", hdr).group(1)) == 6
    assert C.sizeof(capi.VolumeInfo) == 88  # the struct kept its layout: the crossings have a getter of their own


def test_no_surfaces_is_the_parent_checker():
    vol = noise(20)
    t = cool(THIN)
    cam = camera(24, 20)
    rays = vc.camera_rays(cam)
    rays["color"] = 0
    rays["w"] = 0
    B = vc.Brick(vol, t, 1.3)
    want = vc.march(B, rays, IDENT)
    for S in (None, sc.Surfaces()):
        got = sc.march(B, S, rays, IDENT)
        assert got.tobytes() == want.tobytes()
    assert (want["w"] > 0).any()


def test_the_checker_does_not_depend_on_the_bricking():
    vol = noise(26)
    t = cool(THIN)
    cam = camera(40, 32)
    S = sc.Surfaces([0.45, 0.6], [[0.5, 0.7, -0.4, 0.25]], opacity=0.5, lights=[((3, 4, 5), (1, 0.9, 0.8)), ((-2, 1, 0.5), (0.2, 0.3, 0.4))])
    results = []
    for split in ((1, 1, 1), (2, 2, 2), (3, 1, 2)):
        parts = scenes.split_volume(vol, *split)
        bricks = [vc.Brick(b, t, 1.5) for b in parts]
        final = []
        fb, calls = sc.frame(bricks, [b.lo for b in parts], [b.hi for b in parts], IDENT, cam, S, final)
        assert calls >= len(parts)
        results.append((fb, by_id(final)))
    fb0, r0 = results[0]
    assert ((r0["depth"] & sc.SIDES) != 0).any()
    whole = vc.Brick(vol, t, 1.5)
    plain, _ = vc.frame([whole], whole.lo[None], whole.hi[None], IDENT, cam)
    assert (bits(plain) != bits(fb0)).any()  # the surfaces show
    for fb, r in results[1:]:
        assert (bits(fb) == bits(fb0)).all()
        assert len(r) == len(r0) and (r["id"] == r0["id"]).all()
        for f in ("color", "w", "t_min", "t", "depth"):
            assert (bits(r[f]) == bits(r0[f])).all(), f


def test_nothing_is_detected_across_a_gap():
    """A ramp in x cut into three bricks along x, the middle one left out: the isovalue lies in the gap, the rays' sides differ on its
    two shores, and no surface may be rendered; with the middle brick present it is."""
    n = 25
    x = np.linspace(0.0, 1.0, n, dtype=F)
    vol = scenes.VolumeData(np.ascontiguousarray(np.broadcast_to(x[None, None, :], (n, n, n))).astype(F), np.zeros(3, F), np.full(3, F(1.0 / (n - 1)), F))
    t = cool(THIN)
    parts = scenes.split_volume(vol, 3, 1, 1)
    S = sc.Surfaces([0.5], opacity=1.0)
    cam = camera(24, 24, eye=(-2.5, 0.55, 0.45), focus=(0.5, 0.5, 0.5))

    def run(sel, surf):
        bricks = [vc.Brick(parts[i], t, 1.0) for i in sel]
        final = []
        fb, _ = sc.frame(bricks, [parts[i].lo for i in sel], [parts[i].hi for i in sel], IDENT, cam, surf, final)
        return fb, by_id(final)

    fb_gap, r_gap = run((0, 2), S)
    fb_plain, _ = run((0, 2), None)
    assert (bits(fb_gap) == bits(fb_plain)).all()
    both = r_gap[(r_gap["w"] > 0)]
    assert len(both) > 50 and (r_gap["t"][(r_gap["depth"] & sc.SIDES) != 0] == 1).any()  # rays that ended beyond the isovalue, on its far side
    fb_all, r_all = run((0, 1, 2), S)
    assert ((r_all["depth"] & vc.OPAQUE) != 0).sum() > 50 and (bits(fb_all) != bits(fb_gap)).any()


def test_the_sphere_isosurface_is_a_sphere():
    """sphere_volume: 1 - r / c, so isovalue 0.5 is the sphere of radius R = c / 2 around the centre.  With a clear table and an opaque
    surface a ray is OPAQUE iff it met the surface.  The interpolant is within one cell diagonal of the field (its value is a mean of
    vertex values no further away) and the rule renders a crossing at the next sample, so rays passing closer than R - m must be OPAQUE and
    rays further than R + m must not, m = one lattice step along the ray + one cell diagonal."""
    n, rate = 257, 2.0
    vol = scenes.sphere_volume(n)
    ctr = np.full(3, (n - 1) / 2.0)
    R = (n - 1) / 4.0
    B = vc.Brick(vol, cool(CLEAR), rate)
    cam = camera(56, 56, eye=(128.0 + 330.0, 128.0 + 240.0, 128.0 + 410.0), focus=tuple(ctr))
    cam.fov = float(F(20.0 * np.pi / 180.0))
    rays = vc.camera_rays(cam)
    rays["color"] = 0
    rays["w"] = 0
    rays["depth"] = 0
    out = sc.march(B, sc.Surfaces([0.5], opacity=1.0), rays, IDENT)
    o, d = rays["origin"].astype(np.float64), rays["direction"].astype(np.float64)
    dl = np.linalg.norm(d, axis=1)
    b = np.linalg.norm(np.cross(ctr - o, d), axis=1) / dl
    m = float(B.dt) * dl + np.sqrt(3.0)
    opaque = (out["depth"] & vc.OPAQUE) != 0
    inside, outside = b < R - m, b > R + m
    disc = b <= R
    band = ~inside & ~outside
    share = band.sum() / disc.sum()
    print("sphere anchor: %d rays, %d in the disc, %d inside, %d in the band (%.3f of the disc)" % (len(rays), disc.sum(), inside.sum(), band.sum(), share))
    assert inside.sum() > 200 and outside.sum() > 200
    assert opaque[inside].all()
    assert not opaque[outside].any()
    assert share < 0.2
    assert (out["w"][opaque] == 1).all() and (out["w"][~opaque] == 0).all()


def test_plane_shading_by_hand():
    n = 9
    vol = scenes.VolumeData(np.full((n, n, n), 0.5, F), np.zeros(3, F), np.full(3, F(0.125), F))
    B = vc.Brick(vol, cool(CLEAR), 1.0)
    rays = np.zeros(1, RAY_DTYPE)
    rays["origin"] = (-1.0, 0.53, 0.47)
    rays["direction"] = (1.0, 0.0, 0.0)
    rays["t_min"] = F(1e-6)
    c = sc.lookup(B, np.array([0.5], F))[0, :3]
    ka, kd = F(0.4), F(0.6)
    plane = [[1.0, 0.0, 0.0, 0.5]]
    cases = [(((5, 0, 0),), c * (ka + kd * F(1))), (((-5, 0, 0),), c * (ka + kd * F(1))), (((0, 5, 0),), c * (ka + kd * F(0))), ((), c)]
    for pos, want in cases:
        S = sc.Surfaces((), plane, 1.0, [(p, (1, 1, 1)) for p in pos])
        out = sc.march(B, S, rays, IDENT)
        assert sc.march.crossings == 1
        assert out["depth"][0] & vc.OPAQUE and out["w"][0] == 1
        assert (bits(out["color"][0]) == bits(want.astype(F))).all(), (pos, out["color"][0], want)
    # half opacity, two lights of different colours: the sum in light order, the ray goes on
    S = sc.Surfaces((), plane, 0.5, [((5, 0, 0), (1, 0.5, 0.25)), ((0, 0, 7), (0.5, 0.5, 0.5))])
    out = sc.march(B, S, rays, IDENT)
    want = F(0.5) * (c * (ka + kd * np.array([1, 0.5, 0.25], F)))
    assert (bits(out["color"][0]) == bits(want.astype(F))).all() and out["w"][0] == F(0.5) and out["depth"][0] & vc.BOUNDARY
    assert out["depth"][0] & sc.SIDES and out["t"][0] == 1
