"""The cases of the shaded fused-frame tests (tests/test_gpu_volume_fused_shaded.py, tests/test_volume_fused_shaded_host.py), on top of
tests/volume_fused_cases.py: its 25^3 grid, 64 x 48 film, rate 1.7 and four brickings, with two isovalues and a slice plane through
the grid's middle, two lights, and three modes -- surfaces alone, lit fog alone, both.  The numpy frames are computed once per case and
shared; treat them as read-only."""
import functools

import numpy as np

from gravit_amd import scenes
from gravit_amd.layouts import RAY_DTYPE
from oracle import orc
from tests import volume_checker as vc
from tests import volume_clip_checker as cc
from tests import volume_fused_cases as fc
from tests import volume_fused_shaded_checker as fs
from tests import volume_shade_checker as lc
from tests import volume_surface_checker as sc
from tests.volume_common import tf

F = np.float32
ISO = (0.45, 0.6)
OPACITY = 0.6
LIGHTS = (((3.0, 4.0, 5.0), (1.0, 0.9, 0.8)), ((-2.0, 1.0, 0.5), (0.3, 0.4, 0.9)))
MODES = {"surf": "cool", "lit": "cool", "surf_lit": "spikes"}  # mode -> table
CAMERAS = {"outside": True, "inside": False}  # where -> under the MOVED matrix?
MULTI = [s for s in fc.SPLITS if s != (1, 1, 1)]
FEATURES = {"surf": 1, "lit": 2, "surf_lit": 3}  # gvt_hip_volume_fused_shaded_stats.features


def slice_plane():
    """(0.3, 0.5, 0.8, d), object space, through the middle of the grid."""
    vol = fc.volume()
    mid = vol.origin.astype(np.float64) + 0.5 * (vol.counts - 1) * vol.spacing.astype(np.float64)
    nrm = np.array([0.3, 0.5, 0.8])
    return (0.3, 0.5, 0.8, float(F(nrm @ mid)))


def surfaces(mode, scale=1.0, offset=0.0, lights=LIGHTS, ka=0.4, kd=0.6):
    """The mode's Surfaces (what set_surfaces + set_lights hold) and whether shading is on.  scale / offset: the isovalues in a typed
    volume's units."""
    iso = [offset + scale * v for v in ISO]
    if mode == "lit":
        return lc.lights_only(lights, ka, kd), True
    return sc.Surfaces(iso, [slice_plane()], OPACITY, lights, ka=ka, kd=kd), mode == "surf_lit"


def shade_mode(on):
    return lc.SHADE_GRADIENT if on else lc.SHADE_NONE


def setup(split, mode, where, moved=None):
    """(bricks of the checker, lo, hi, minv, camera, S, shading mode, parts) of a case.  moved: None = the camera's own matrix."""
    moved = CAMERAS[where] if moved is None else moved
    parts = fc.bricks_of(fc.volume(), split)
    m = fc.matrix(moved)
    lo, hi = fc.world_boxes(parts, m)
    S, on = surfaces(mode)
    bricks = [vc.Brick(b, tf(MODES[mode]), fc.RATE) for b in parts]
    return bricks, lo, hi, scenes.instance_matrices(m)[0], fc.camera(where, moved), S, shade_mode(on), parts


def loop_frame(bricks, lo, hi, minv, cam, S, mode, plane=None):
    """volume_shade_checker.frame -- the loop: queues, the largest first, march, shuffle -- which also sums march.crossings:
    (framebuffer, {crossings_rendered, samples_shaded, adapter_calls})."""
    lo, hi = np.asarray(lo, F).reshape(-1, 3), np.asarray(hi, F).reshape(-1, 3)
    order = orc.toplevel_order(lo, hi)
    fb = np.zeros((cam.width * cam.height, 4), F)
    queues = [[] for _ in bricks]
    flat = None if plane is None else np.ascontiguousarray(plane, F).reshape(-1)
    cc.shuffle(lo, hi, order, vc.camera_rays(cam), -1, queues, fb, flat)
    calls = crossings = shaded = 0
    while True:
        sizes = [sum(len(a) for a in q) for q in queues]
        target, best = -1, 0
        for i, s in enumerate(sizes):
            if s > best:
                best, target = s, i
        if target < 0:
            break
        rays = np.concatenate(queues[target]) if queues[target] else np.zeros(0, RAY_DTYPE)
        queues[target] = []
        rays = lc.march(bricks[target], S, rays, minv, mode)
        crossings += lc.march.crossings
        shaded += lc.march.shaded
        calls += 1
        cc.shuffle(lo, hi, order, rays, target, queues, fb)
    return fb.reshape(cam.height, cam.width, 4), {"crossings_rendered": crossings, "samples_shaded": shaded, "adapter_calls": calls}


@functools.lru_cache(maxsize=None)
def reference(split, mode, where, clipped=False):
    """The per-ray checker's frame of the case: (framebuffer, counters, depth plane or None).  clipped: under fc.depth_plane, with the
    identity matrix whatever the camera.  Computed once; read-only."""
    bricks, lo, hi, minv, cam, S, shading, parts = setup(split, mode, where, False if clipped else None)
    plane = fc.depth_plane(parts, False, where) if clipped else None
    fb, counters = fs.frame(bricks, lo, hi, minv, cam, S, shading, plane)
    fb.setflags(write=False)
    return fb, counters, plane
