"""The cases of the shadowed-fog tests (tests/test_gpu_volume_fog_shadow.py, tests/test_volume_fog_shadow_host.py), on
tests/volume_fused_cases.py's 25^3 grid, 64 x 48 film, rate 1.7 and four brickings -- the smallest shapes at which macro cells are partial
and rays, the vertices' shadow rays included, cross several bricks.

lit       table "cool", no surfaces, tests/volume_shadow_cases.py's two lights, shading on: fog alone, every sample of it shadowed.
surf_lit  table "spikes" with the shaded cases' surfaces (isovalues 0.45 and 0.6, the slice plane, opacity 0.6), the same lights, shading
          on: crossings lit through exact shadow rays (bias 2), the fog between them through the grids.
The grids are baked with bias 1.  Of the 15,625 vertices of the checker's grid under the identity matrix, as
A_s == 0 / 0 < A_s < 0.99 / A_s >= 0.99 (measured; tests/test_volume_fog_shadow_host.py asserts at least 0.05 of each for `lit`, and at
least 0.2 of each of the first two for `surf_lit`):
    lit       light (3, 4, 5)  0.115 / 0.194 / 0.691      light (-2, 1, 0.5)  0.115 / 0.106 / 0.779
    surf_lit  light (3, 4, 5)  0.323 / 0.644 / 0.034      light (-2, 1, 0.5)  0.430 / 0.567 / 0.003
and under MOVED 0.115 / 0.129 / 0.756, 0.115 / 0.077 / 0.808, 0.308 / 0.656 / 0.036 and 0.419 / 0.578 / 0.004.

PARALLEL  lights parallel to a grid plane, (0, 0, 1), (0, 1, 0) and (1, 1, 0): a vertex's ray then runs IN the brick faces it starts on,
          where the next-brick walk of the shadowed frame loses samples (include/gvt_hip.h, "shadowed surfaces", DEVIATIONS (5)); the
          bake must give the one brick's bits all the same.

The numpy grids and frames are computed once per case and shared; treat them as read-only."""
import functools

import numpy as np

from gravit_amd import scenes
from tests import volume_checker as vc
from tests import volume_fog_shadow_checker as fg
from tests import volume_fused_cases as fc
from tests import volume_fused_shaded_checker as fs
from tests import volume_shadow_cases as swc
from tests import volume_surface_checker as sc

F = np.float32
GRID_BIAS = 1
BIAS = swc.BIAS  # of the crossings' shadow rays
MODES = ("lit", "surf_lit")
LIGHTS = swc.LIGHTS
CAMERAS = swc.CAMERAS  # where -> under the MOVED matrix?
PARALLEL = ((0.0, 0.0, 1.0), (0.0, 1.0, 0.0), (1.0, 1.0, 0.0))
WHITE = (1.0, 1.0, 1.0)


def with_lights(S, lights):
    """S with another list of lights."""
    return sc.Surfaces(S.iso, S.planes, S.opacity, lights, ka=S.ka, kd=S.kd)


def whole(mode, moved, lights=None):
    """(the checker's brick of the WHOLE grid, its world lo, hi, m, minv, S, shading mode) of a mode.  lights: None = LIGHTS."""
    bricks, lo, hi, minv, _, S, shading, _, _ = swc.setup("main", (1, 1, 1), "outside", mode, moved)
    if lights is not None:
        S = with_lights(S, lights)
    return bricks[0], lo, hi, fc.matrix(moved), minv, S, shading


@functools.lru_cache(maxsize=None)
def light_grid(mode, moved, lights=None):
    """The checker's grid of a mode: (G (lights, gz, gy, gx), usable).  Computed once; read-only."""
    B, lo, hi, m, minv, S, _ = whole(mode, moved, lights)
    G, usable = fg.grid(B, lo, hi, m, minv, S, GRID_BIAS)
    G.setflags(write=False)
    return G, usable


def shares(G):
    """Of the vertices of one light's plane: (A_s == 0, 0 < A_s < 0.99, A_s >= 0.99) as fractions."""
    A = (F(1) - G).astype(F).reshape(-1)
    return float((A == 0).mean()), float(((A > 0) & (A < vc.OPAQUE_A)).mean()), float((A >= vc.OPAQUE_A).mean())


def setup(mode, split, where, moved=None):
    """volume_shadow_cases.setup of the main case: (bricks, lo, hi, minv, camera, S, shading mode, parts, table)."""
    return swc.setup("main", split, where, mode, moved)


@functools.lru_cache(maxsize=None)
def reference(mode, split, where, clipped=False):
    """The fog checker's frame of the case: (framebuffer, counters, depth plane or None).  clipped: under fc.depth_plane, with the
    identity matrix whatever the camera.  Computed once; read-only."""
    moved = False if clipped else CAMERAS[where]
    bricks, lo, hi, minv, cam, S, shading, parts, _ = setup(mode, split, where, moved)
    plane = fc.depth_plane(parts, False, where) if clipped else None
    fb, counters = fg.frame(bricks, lo, hi, minv, cam, S, shading, light_grid(mode, moved)[0], plane, BIAS)
    fb.setflags(write=False)
    return fb, counters, plane


@functools.lru_cache(maxsize=None)
def unshadowed(mode, split, where):
    """volume_fused_shaded_checker.frame of the case -- nothing shadowed: (framebuffer, counters)."""
    bricks, lo, hi, minv, cam, S, shading, _, _ = setup(mode, split, where)
    fb, counters = fs.frame(bricks, lo, hi, minv, cam, S, shading)
    fb.setflags(write=False)
    return fb, counters
