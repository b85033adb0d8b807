"""Geometry inside a volume, host side (no GPU): the clipped checker (tests/volume_clip_checker.py) against the existing yardstick
(tests/volume_checker.py) where no ray is flagged, the edge cases of the clip distance, the composite's two promises, and the clipped
frame's independence of the bricking."""
import os
import re

import numpy as np
import pytest

from gravit_amd import capi, scenes
from tests import volume_checker as vc
from tests import volume_clip_checker as cc
from tests.conftest import ROOT
from tests.test_gpu_volume import IDENT, MOVED, grid, make_rays, tf

F = np.float32
NEW = ["gvt_hip_depth_create", "gvt_hip_depth_destroy", "gvt_hip_depth_clear", "gvt_hip_depth_upload", "gvt_hip_depth_download", "gvt_hip_depth_render",
       "gvt_hip_volume_frame_clipped", "gvt_hip_fb_composite_over"]


def same_bits(a, b, fields=("color", "w", "t_min", "depth")):
    for f in fields:
        assert (np.ascontiguousarray(a[f]).view(np.uint32) == np.ascontiguousarray(b[f]).view(np.uint32)).all(), f


def test_header_declares_and_binding_lists_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "gvt_hip.h")).read()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in capi.SYMBOLS
    assert int(re.search(r"#define\s+GVT_HIP_RAY_CLIP\s+(0x[0-9a-f]+)", hdr).group(1), 16) == 0x40 == capi.RAY_CLIP == cc.CLIP
    assert int(re.search(r"#define GVT_HIP_ABI_VERSION (\d+)", hdr).group(1)) == 6  # additive: the revision stays


@pytest.fixture(scope="module")
def case():
    vol = grid(24)
    minv = scenes.instance_matrices(MOVED)[0]
    rays = make_rays(vol, MOVED, n=3000)
    B = vc.Brick(vol, tf("cool"), 1.7)
    return B, rays, minv, vc.march(B, rays, minv)


def test_unflagged_rays_equal_the_existing_checker(case):
    B, rays, minv, want = case
    same_bits(cc.march(B, rays, minv), want, ("color", "w", "t_min", "depth", "t_max"))
    finite = rays.copy()  # a t_max without the flag means nothing
    finite["t_max"] = np.linspace(-1, 3, len(rays)).astype(F)
    same_bits(cc.march(B, finite, minv), want)
    assert (want["w"] > 0).sum() > 500


def test_infinite_clip_equals_unflagged(case):
    B, rays, minv, want = case
    r = rays.copy()
    r["depth"] |= cc.CLIP
    r["t_max"] = np.inf
    got = cc.march(B, r, minv)
    same_bits(got, want, ("color", "w", "t_min"))
    assert (got["depth"] == (want["depth"] | cc.CLIP)).all()
    r["t_max"] = np.finfo(F).max  # beyond 2^30 steps: no cut either
    same_bits(cc.march(B, r, minv), got)


@pytest.mark.parametrize("t_max", [0.0, -0.0, -1.5, -np.inf, np.nan])
def test_clip_at_or_behind_the_origin_marches_nothing(case, t_max):
    B, rays, minv, _ = case
    r = rays.copy()
    r["depth"] |= cc.CLIP
    r["t_max"] = F(t_max)
    got = cc.march(B, r, minv)
    assert (got["w"] == 0).all() and (got["color"] == 0).all()
    assert (got["t_min"].view(np.uint32) == rays["t_min"].view(np.uint32)).all()
    assert (got["depth"] == (rays["depth"] | cc.CLIP | vc.BOUNDARY)).all()


def test_clip_exactly_on_a_lattice_value_excludes_that_sample(case):
    B, rays, minv, want = case
    ks = np.arange(0, 200)
    t = (ks.astype(F) * B.dt).astype(F)
    assert (cc.last_before(t, B.dt) == ks - 1).all()
    assert (cc.last_before(np.nextafter(t, F(np.inf)), B.dt) == ks).all()
    assert cc.last_before(np.array([np.inf, np.nan, 0.0, 1e-30], F), B.dt).tolist() == [1 << 30, -1, -1, 0]
    # a ray that marched to sample k unclipped stops at k - 1 when clipped at exactly k * dt, and at k when clipped just beyond
    k_last = np.rint(want["t_min"] / B.dt).astype(np.int64)
    marched = want["t_min"] != rays["t_min"]
    assert ((k_last.astype(F) * B.dt).astype(F)[marched] == want["t_min"][marched]).all()
    r = rays.copy()
    r["depth"] |= cc.CLIP
    r["t_max"] = want["t_min"]
    at = cc.march(B, r, minv)
    assert (at["t_min"][marched] < want["t_min"][marched]).any()
    assert (at["t_min"] <= np.maximum((k_last - 1).astype(F) * B.dt, rays["t_min"]))[marched].all()
    r["t_max"] = np.nextafter(want["t_min"], F(np.inf))
    beyond = cc.march(B, r, minv)
    full = marched & ((want["depth"] & vc.OPAQUE) == 0)  # its last sample was the brick's last: the clip just beyond it cuts nothing
    same_bits(beyond[full], want[full], ("color", "w", "t_min"))


def test_composite_promises():
    rng = np.random.default_rng(3)
    back = (rng.random((6, 7, 4)) * 1.5).astype(F)
    depth = np.where(rng.random((6, 7)) < 0.5, F(2.0), F(np.inf)).astype(F)
    none = np.zeros((6, 7, 4), F)
    out = cc.composite(none, back, depth)
    assert (out[..., :3].view(np.uint32) == np.minimum(back[..., :3], 1).view(np.uint32)).all()  # no volume: min(back, 1) exactly
    assert (out[..., 3] == np.isfinite(depth)).all()
    black = back.copy()
    black[..., :3] = 0  # a shadowed surface: opaque black where the depth is finite
    out = cc.composite(none, black, depth)
    assert (out[..., :3] == 0).all() and (out[..., 3][np.isfinite(depth)] == 1).all()
    out = cc.composite(none, back, None)
    assert (out[..., 3] == np.minimum(back[..., 3], 1)).all()


def clip_frame_case():
    """The frame the GPU test renders too: a 64^3 sphere at 150 x 110 (partial 8 x 8 tiles) behind a tilted analytic plane through the
    sphere, +Inf on a third of the film."""
    vol = scenes.sphere_volume(64)
    vol.spacing = np.full(3, F(1.0 / 63), F)
    cam = scenes.Camera((2.3, 1.7, 3.1), (0.48, 0.51, 0.47), (0.0, 1.0, 0.0), float(F(35.0 * np.pi / 180.0)), 150, 110)
    y, x = np.mgrid[0:110, 0:150]
    keep = (x // 10 + y // 10) % 3 != 0  # (blocks of 10 pixels: they straddle the 8 x 8 tiles)
    plane = cc.depth_of_plane(cam, (0.3, 0.2, 1.0), 0.3 * 0.5 + 0.2 * 0.5 + 0.45, keep)
    return vol, cam, plane


@pytest.fixture(scope="module")
def clip_frame():
    vol, cam, plane = clip_frame_case()
    t = tf("cool")
    B = vc.Brick(vol, t, 1.0)
    whole, calls = cc.frame([B], B.lo[None], B.hi[None], IDENT, cam, plane)
    return vol, cam, plane, t, whole


def test_clipped_frame_differs_from_the_plain_frame_only_where_the_plane_cuts(clip_frame):
    vol, cam, plane, t, whole = clip_frame
    B = vc.Brick(vol, t, 1.0)
    plain, _ = vc.frame([B], B.lo[None], B.hi[None], IDENT, cam)
    free = ~np.isfinite(plane)
    assert (plain[free].view(np.uint32) == whole[free].view(np.uint32)).all() and (plain[free][:, 3] > 0).sum() > 300  # +Inf: unclipped
    cut = whole[..., 3] < plain[..., 3]
    assert cut.sum() > 300 and (whole[..., 3] <= plain[..., 3]).all() and not cut[free].any()
    assert ((whole[..., 3] > 0) & cut).sum() > 300  # the plane passes THROUGH the sphere: fog in front of it stays


@pytest.mark.parametrize("split", [(2, 2, 2), (1, 1, 8)])
def test_clipped_checker_frame_is_independent_of_the_bricking(clip_frame, split):
    """(The float slab test and the cell test can disagree by an ulp, include/gvt_hip.h: this plane does not hit that case.)"""
    vol, cam, plane, t, whole = clip_frame
    parts = scenes.split_volume(vol, *split)
    bricks = [vc.Brick(b, t, 1.0) for b in parts]
    got, calls = cc.frame(bricks, [b.lo for b in parts], [b.hi for b in parts], IDENT, cam, plane)
    assert calls > 1
    assert (got.view(np.uint32) == whole.view(np.uint32)).all()
