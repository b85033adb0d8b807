"""Lit volumes on the host (no GPU): the new entry points in the header and the binding, and the numpy checker
(tests/volume_shade_checker.py) against its three parents bit for bit where shading cannot show, against itself under different
brickings, against a hand-computed ramp and on a clear table."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gravit_amd import capi, scenes
from tests import volume_checker as vc
from tests import volume_clip_checker as cc
from tests import volume_shade_checker as lc
from tests import volume_surface_checker as sc
from tests.conftest import ROOT
from tests.test_gpu_volume import IDENT, MOVED, grid, make_rays, tf
from tests.test_volume_surfaces_host import CLEAR, THIN, camera, cool, noise

F = np.float32
NEW = ["gvt_hip_volume_set_shading", "gvt_hip_volume_get_shading", "gvt_hip_volume_get_shaded"]
LIGHTS = [((3.0, 4.0, 5.0), (1.0, 0.9, 0.8)), ((-2.0, 1.0, 0.5), (0.2, 0.3, 0.4)), ((0.5, -3.0, 1.0), (0.3, 0.1, 0.2))]
ALL = ("color", "w", "t_min", "depth", "t")


def same_bits(a, b, fields=ALL):
    for f in fields:
        assert (np.ascontiguousarray(a[f]).view(np.uint32) == np.ascontiguousarray(b[f]).view(np.uint32)).all(), f


def surfaces(lights=LIGHTS, ka=0.4, kd=0.6):
    return sc.Surfaces([0.42, 0.58], [[0.5, 0.7, -0.4, 0.3]], 0.5, lights, ka=ka, kd=kd)


def test_header_declares_and_binding_lists_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "gvt_hip.h")).read()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in capi.SYMBOLS
    assert int(re.search(r"#define\s+GVT_HIP_VOLUME_SHADE_NONE\s+(\d+)", hdr).group(1)) == 0 == capi.VOLUME_SHADE_NONE == lc.SHADE_NONE
    assert int(re.search(r"#define\s+GVT_HIP_VOLUME_SHADE_GRADIENT\s+(\d+)", hdr).group(1)) == 1 == capi.VOLUME_SHADE_GRADIENT == lc.SHADE_GRADIENT
    assert int(re.search(r"#define GVT_HIP_ABI_VERSION (\d+)", hdr).group(1)) == 6 == capi.ABI_VERSION  # additive: the revision stays
    assert C.sizeof(capi.VolumeInfo) == 88  # the struct kept its layout: the shaded samples have a getter of their own


@pytest.fixture(scope="module")
def case():
    vol = grid(24)
    minv = scenes.instance_matrices(MOVED)[0]
    rays = make_rays(vol, MOVED, n=1500)
    rays["t"] = 55.0
    B = vc.Brick(vol, tf("ramp"), 1.7)
    clipped = rays.copy()
    clipped["depth"] |= np.where(np.arange(len(rays)) % 3 != 0, cc.CLIP, 0).astype(np.int32)
    clipped["t_max"] = (np.random.default_rng(2).random(len(rays)) * 4).astype(F)
    return B, rays, clipped, minv


def test_shading_off_or_no_lights_is_the_parent_checkers(case):
    B, rays, clipped, minv = case
    plain, surf, clip = vc.march(B, rays, minv), sc.march(B, surfaces(), rays, minv), cc.march(B, clipped, minv)
    assert (plain["w"] > 0).sum() > 300 and sc.march.crossings > 100 and (clip["t_min"] < plain["t_min"]).sum() > 100
    # shading off, with lights set
    same_bits(lc.march(B, lc.lights_only(LIGHTS), rays, minv, lc.SHADE_NONE), plain)
    same_bits(lc.march(B, surfaces(), rays, minv, lc.SHADE_NONE), surf)
    same_bits(lc.march(B, lc.lights_only(LIGHTS), clipped, minv, lc.SHADE_NONE), clip, ALL + ("t_max",))
    assert lc.march.shaded == 0
    # shading on, no lights
    same_bits(lc.march(B, None, rays, minv), plain)
    same_bits(lc.march(B, lc.lights_only([]), rays, minv), plain)
    same_bits(lc.march(B, surfaces([]), rays, minv), sc.march(B, surfaces([]), rays, minv))
    same_bits(lc.march(B, None, clipped, minv), clip)
    assert lc.march.shaded == 0


def test_ka_one_kd_zero_is_the_parent_checkers(case):
    B, rays, clipped, minv = case
    got = lc.march(B, lc.lights_only(LIGHTS, 1.0, 0.0), rays, minv)
    assert lc.march.shaded > 1000  # shaded, and to the same bits: x * (1 + 0 * S) = x
    same_bits(got, vc.march(B, rays, minv))
    same_bits(lc.march(B, surfaces(LIGHTS, 1.0, 0.0), rays, minv), sc.march(B, surfaces(LIGHTS, 1.0, 0.0), rays, minv))
    same_bits(lc.march(B, lc.lights_only(LIGHTS, 1.0, 0.0), clipped, minv), cc.march(B, clipped, minv))
    lit = lc.march(B, lc.lights_only(LIGHTS), rays, minv)  # ... while the default material shows
    assert (lit["color"] != got["color"]).any(axis=1).sum() > 300
    same_bits(lit, got, ("w", "t_min", "depth"))  # opacity is not shaded


def test_the_lit_checker_does_not_depend_on_the_bricking():
    vol = noise(26)
    t = cool(THIN)
    cam = camera(64, 48)
    S = lc.lights_only(LIGHTS)
    B = vc.Brick(vol, t, 1.3)
    whole, _ = lc.frame([B], B.lo[None], B.hi[None], IDENT, cam, S)
    n_whole = lc.frame.shaded
    unlit, _ = vc.frame([B], B.lo[None], B.hi[None], IDENT, cam)
    assert n_whole > 10000 and (whole[..., :3] != unlit[..., :3]).any(axis=2).sum() > 500
    assert (whole[..., 3].view(np.uint32) == unlit[..., 3].view(np.uint32)).all()
    for split in ((2, 2, 2), (3, 1, 2)):
        parts = scenes.split_volume(vol, *split)
        bricks = [vc.Brick(b, t, 1.3) for b in parts]
        got, calls = lc.frame(bricks, [b.lo for b in parts], [b.hi for b in parts], IDENT, cam, S)
        assert calls > 1 and lc.frame.shaded == n_whole
        assert (got.view(np.uint32) == whole.view(np.uint32)).all(), split


def test_a_ramp_along_x_is_lit_by_the_lights_x_component():
    """v = x: in every cell the differences along y and z are exactly 0 and the one along x is one value a, so g = (a / sx, 0, 0),
    len = |g.x| and n = (+-1, 0, 0) exactly, ndl = |l.x| exactly, and every shaded sample's colour is tc.rgb * m with ONE float32 vector
    m = ka + kd * (colour * |l.x|).  The lit ray sums fl(fr_k * fl(tc_k * m)), the unlit one fl(fr_k * tc_k); all terms are >= 0, the fr_k
    are the same floats in both (opacity is not shaded).  Tolerance, relative to unlit * m per channel, with u = 2^-24 and N the number of
    samples of a ray: 2 roundings per lit term and N - 1 of its sum, 1 rounding per unlit term and N - 1 of its sum; first order
    (2 N + 1) u.  N is at most the largest lattice index any ray reached; the bound used is (2 N + 4) u, the 3 u of slack for the
    second-order terms (N u < 1e-4 here)."""
    n = 20
    x = np.linspace(0.05, 0.95, n).astype(F)
    vol = scenes.VolumeData(np.ascontiguousarray(np.broadcast_to(x[None, None, :], (n, n, n))).astype(F),
                            np.array([-0.25, 0.1, -0.4], F), np.array([1.0 / (n - 1), 1.1 / (n - 1), 0.9 / (n - 1)], F))
    t = tf("ramp")
    B = vc.Brick(vol, t, 1.7)
    rays = make_rays(vol, IDENT, n=1000)
    S = lc.lights_only(LIGHTS[:1], 0.4, 0.6)
    lit, unlit = lc.march(B, S, rays, IDENT), vc.march(B, rays, IDENT)
    assert lc.march.shaded > 1000
    same_bits(lit, unlit, ("w", "t_min", "depth"))
    lx = np.abs(S.light_dirs(IDENT)[0, 0])
    m = (S.ka + S.kd * (S.lcol[0] * lx).astype(F)).astype(F)
    assert 0.1 < lx < 0.9 and ((m > 0.4) & (m < 1.0)).all()
    n_max = int(np.ceil(float((lit["t_min"] / B.dt).max()))) + 1
    assert 20 < n_max < 2000
    want = unlit["color"].astype(np.float64) * m.astype(np.float64)
    tol = (2 * n_max + 4) * 2.0 ** -24
    assert (np.abs(lit["color"] - want) <= tol * want + 1e-37).all()
    assert (unlit["color"] > 0).any(axis=1).sum() > 300 and (lit["color"] < unlit["color"]).any(axis=1).sum() > 300


def test_a_clear_table_shades_nothing():
    vol = noise(20)
    cam = camera(24, 20)
    rays = vc.camera_rays(cam)
    rays["color"] = 0
    rays["w"] = 0
    B = vc.Brick(vol, cool(CLEAR), 1.3)
    got = lc.march(B, lc.lights_only(LIGHTS), rays, IDENT)
    assert lc.march.shaded == 0
    same_bits(got, vc.march(B, rays, IDENT))
    assert (got["t_min"] > rays["t_min"]).sum() > 100 and (got["w"] == 0).all()  # marched, and nothing to show
    whole, _ = lc.frame([B], B.lo[None], B.hi[None], IDENT, cam, lc.lights_only(LIGHTS))
    assert lc.frame.shaded == 0 and (whole == 0).all()
