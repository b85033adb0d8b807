"""The volume cases under the matrix families of tests/affine_cases.py, shared by tests/test_affine_host.py and
tests/test_gpu_volume_affine.py: the fused-frame tests' 25^3 noise grid with non-uniform spacing, a 64 x 48 camera placed in the
volume's own space and taken to the world by m, sampling rate 1.7, and per variant of the march -- plain, surfaces, lit, surfaces + lit,
central gradients, AMR, the clip -- the numpy checker's result on the camera's list, computed once per case and shared."""
import functools

import numpy as np

from gravit_amd import scenes
from tests import affine_cases as ac
from tests import volume_amr_checker as amr
from tests import volume_checker as vc
from tests import volume_clip_checker as cc
from tests import volume_fused_cases as fc
from tests import volume_shade_checker as lc
from tests import volume_smooth_checker as sm
from tests import volume_surface_checker as sc
from tests.volume_common import tf

F = np.float32
RATE = fc.RATE
ISO = [0.42, 0.58]
PLANES = [[0.5, 0.7, -0.4, 0.3]]
LIGHTS = [((3.0, 4.0, 5.0), (1.0, 0.9, 0.8)), ((-2.0, 1.0, 0.5), (0.2, 0.3, 0.4))]
VARIANTS = ("plain", "surfaces", "lit", "surf_lit", "central", "amr", "clip")
SPLITS = [(1, 1, 1), (2, 2, 2), (3, 3, 3)]
# lit fog turned with its lights and camera against the unturned frame: the numpy checker's own largest per-channel difference between the
# two formulations, over "rot" and "rot@1" (tests/test_affine_host.py measures it and holds this value to it)
RIGID_MEASURED = 2.146e-6


def matrix(name):
    """The matrix of a case: a family of affine_cases (its seed 0), "perm_mirror", or "ident"."""
    if name == "ident":
        return scenes.mat_translate_scale((0, 0, 0), (1, 1, 1))
    if name == "perm_mirror":
        return ac.perm_mirror(1)
    if "@" in name:  # "rot@3": another seed
        fam, seed = name.split("@")
        return ac.matrix(fam, int(seed))
    return ac.matrix(name, 0)


def volume():
    return fc.volume()


def amr_volume():
    """The grid with a refined block of 10 x 9 x 12 cells (ratio 2) in the corner nearest the camera (the fog is opaque before a ray
    reaches the middle) and a second level (ratio 2) inside it."""
    vol = fc.volume()
    s0 = scenes.refine(vol, (14, 15, 12), (10, 9, 12), 2, seed=5, detail=0.3)
    scenes.refine(vol, (9, 7, 11), (8, 9, 10), 2, parent=s0, seed=6, detail=0.3)
    return vol


def linear(m):
    M = np.asarray(m, np.float64).reshape(4, 4).T
    return M[:3, :3], M[:3, 3]


def camera(m, up=(0.0, 1.0, 0.0)):
    """An eye beside the volume looking at its middle, given in the volume's own space and placed by m; `up` is the world's."""
    vol = volume()
    lo = vol.origin.astype(np.float64)
    ext = (vol.counts - 1) * vol.spacing.astype(np.float64)
    eye, focus = lo + ext * np.array([2.3, 1.6, 3.1]), lo + ext * np.array([0.48, 0.51, 0.47])
    return scenes.Camera(fc.to_world(m, eye), fc.to_world(m, focus), tuple(up), fc.FOV, fc.FILM[0], fc.FILM[1])


def camera_list(m, clip=False):
    """The camera's rays as the adapter is handed them (no colour, no opacity, no flags).  clip: every ray but each seventh carries CLIP
    and a t_max somewhere along its way through the volume's world box."""
    rays = vc.camera_rays(camera(m))
    rays["color"], rays["w"], rays["depth"], rays["t"] = 0, 0, 0, 123.0
    if clip:
        lo, hi = scenes.instance_bbox(m, *box())
        tn, tf_ = vc.slab(lo, hi, rays["origin"].astype(F), rays["direction"].astype(F))
        hit = (tn <= tf_) & (tf_ > 0)
        u = np.random.default_rng(8).random(len(rays)).astype(F)
        rays["t_max"] = np.where(hit, np.maximum(tn, F(0)) + (tf_ - np.maximum(tn, F(0))) * u, F(1.0)).astype(F)
        rays["depth"] |= np.where(np.arange(len(rays)) % 7 != 0, cc.CLIP, 0).astype(np.int32)
    return rays


def box():
    vol = volume()
    return vol.origin.astype(F), (vol.origin + (vol.counts - 1).astype(F) * vol.spacing).astype(F)


def surfaces(variant, lights=LIGHTS, value_range=(0.0, 1.0)):
    """(Surfaces or None, shading on?) of a variant; value_range: the image of the grid's [0, 1] (typed voxels), for the isovalues."""
    if variant in ("surfaces", "surf_lit", "central"):
        iso = [value_range[0] + v * (value_range[1] - value_range[0]) for v in ISO]
        return sc.Surfaces(iso, PLANES, 0.5, lights), variant != "surfaces"
    if variant == "lit":
        return lc.lights_only(lights), True
    return None, False


def checker_march(variant, vol, t, rays, minv, value_range=(0.0, 1.0)):
    """The numpy checkers' march of a variant on `vol` (float samples)."""
    S, shading = surfaces(variant, value_range=value_range)
    mode = lc.SHADE_GRADIENT if shading else lc.SHADE_NONE
    if variant == "amr":
        return amr.march(amr.AmrBrick(vol, t, RATE), rays, minv)
    if variant == "central":
        return sm.march(sm.Brick(vol, t, RATE), S, rays, minv, mode, kind=sm.CENTRAL)
    return lc.march(vc.Brick(vol, t, RATE), S, rays, minv, mode)


def typed(ty, amr_grid=False):
    """(the grid with voxels of type ty -- "f32", "u8", "i16", "u16" --, its table, the image of [0, 1] in the type's units)."""
    from tests.volume_common import TYPES, quantised, scaled

    vol = amr_volume() if amr_grid else volume()
    if ty == "f32":
        return vol, tf("ramp"), (0.0, 1.0)
    return quantised(vol, ty), scaled("ramp", ty), TYPES[ty][2]


@functools.lru_cache(maxsize=None)
def reference(name, variant, ty="f32"):
    """(rays, the checker's marched rays) of the grid (voxel type ty, marched as floats) under matrix(name); computed once, read-only."""
    m = matrix(name)
    minv = scenes.instance_matrices(m)[0]
    rays = camera_list(m, clip=variant == "clip")
    vol, t, vr = typed(ty, variant == "amr")
    flt = scenes.VolumeData(vol.data.astype(F), vol.origin, vol.spacing, vol.subgrids)
    want = checker_march(variant, flt, t, rays, minv, vr)
    rays.setflags(write=False)
    want.setflags(write=False)
    return rays, want


@functools.lru_cache(maxsize=None)
def frame_reference(name, split, table="cool"):
    """volume_checker.frame of the grid cut into `split` bricks under matrix(name), with the eight-corner world boxes."""
    from gravit_amd.scheduler import _brick_boxes

    m = matrix(name)
    parts = fc.bricks_of(volume(), split)
    lo, hi = _brick_boxes(parts, m)
    fb, calls = vc.frame([vc.Brick(b, tf(table), RATE) for b in parts], lo, hi, scenes.instance_matrices(m)[0], camera(m))
    fb.setflags(write=False)
    return fb, calls


def rotated_with_the_world(name):
    """For the rigid-motion claim: (m, camera, lights) of matrix(name) with the identity case's camera and lights taken along by m's
    linear part A (points through m, the up vector and the lights' directions through A)."""
    m = matrix(name)
    A, _ = linear(m)
    lights = [(tuple(A @ np.asarray(p, np.float64)), c) for p, c in LIGHTS]
    return m, camera(m, up=tuple(A @ np.array([0.0, 1.0, 0.0]))), lights


@functools.lru_cache(maxsize=None)
def lit_frame_reference(name):
    """volume_shade_checker.frame of the one-brick lit fog under matrix(name), the camera and the lights moved with the volume."""
    m, cam, lights = (matrix("ident"), camera(matrix("ident")), LIGHTS) if name == "ident" else rotated_with_the_world(name)
    B = vc.Brick(volume(), tf("ramp"), RATE)
    lo, hi = scenes.instance_bbox(m, B.lo, B.hi)
    fb, _ = lc.frame([B], lo[None], hi[None], scenes.instance_matrices(m)[0], cam, lc.lights_only(lights))
    fb.setflags(write=False)
    return fb


def frame_difference(a, b):
    """(largest per-channel difference, share of pixels with a channel above 1e-5)."""
    d = np.abs(a.astype(np.float64) - b)
    return float(d.max()), float((d.max(axis=2) > 1e-5).mean())
