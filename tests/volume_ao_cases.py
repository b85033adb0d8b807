"""The cases of the ambient occlusion tests (tests/test_gpu_volume_ao.py, tests/test_volume_ao_host.py), on
tests/volume_fog_shadow_cases.py's shapes: the 25^3 grid, the 64 x 48 film, rate 1.7, the four brickings, both matrices and the modes
`lit` (fog alone) and `surf_lit` (surfaces and lit fog).

DIRS      scenes.ao_directions(6), radius 12.5 * dt -- about seven cells, so the rays cross whole bricks of the 4 x 4 x 4 cut -- bake
          bias 1.
PARALLEL  the three axis directions and (1, 1, 0): a vertex's ray then runs IN the brick faces it starts on; the bake must give the one
          brick's bits all the same.
Measured with the numpy march alone (tests/test_volume_ao_host.py asserts at least half in every case): the share of the 15,625
vertices with 0 < AO < 1 is 1.000 for `lit` under both matrices, 0.962 for `surf_lit` under the identity matrix and 0.910 under MOVED.
With radius = dt every vertex has AO == 1; with 1.5 * dt most have not (a ray's one sample then lies in the vertex's own cells).
Pixels with non-zero alpha on which the checker's AO frame differs from its base frame (2 x 2 x 2 bricks; asserted: at least a tenth):
lit 3,072 of 3,072 inside and 941 of 941 outside, surf_lit 3,072 of 3,072 and 761 of 761 -- every pixel that shows the volume.

The numpy grids and frames are computed once per case and shared; treat them as read-only."""
import functools

import numpy as np

from gravit_amd import scenes
from tests import volume_ao_checker as ao
from tests import volume_fog_shadow_cases as fgc
from tests import volume_fog_shadow_checker as fg
from tests import volume_fused_cases as fc
from tests import volume_shadow_cases as swc

F = np.float32
MODES = fgc.MODES  # ("lit", "surf_lit")
CAMERAS = fgc.CAMERAS
BIAS = fgc.BIAS  # of the crossings' shadow rays
GRID_BIAS = 1  # of the light grids' and the AO grid's bake
RADIUS_STEPS = 12.5
PARALLEL = ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (1.0, 1.0, 0.0))
SETS = {"main": lambda: scenes.ao_directions(6), "parallel": lambda: np.asarray(PARALLEL, F), "one": lambda: scenes.ao_directions(6)[4:5],
        "max": lambda: scenes.ao_directions(32)}


def dirs(which="main"):
    """The direction set of a case, (n, 3) float32, as the caller hands it to the bake."""
    return SETS[which]()


def radius(steps=RADIUS_STEPS):
    """steps * dt in float32 (inf stays inf), dt the grid's."""
    return F(steps) * fgc.whole("lit", False)[0].dt


@functools.lru_cache(maxsize=None)
def ao_grid(mode, moved, which="main", steps=RADIUS_STEPS):
    """The checker's AO grid of a mode: (AO (gz, gy, gx) float32, crossings its rays met).  Computed once; read-only."""
    B, _, _, m, minv, S, _ = fgc.whole(mode, moved)
    AO = ao.grid(B, m, minv, S, dirs(which), radius(steps), GRID_BIAS)
    AO.setflags(write=False)
    return AO, ao.grid.crossings


def ones():
    """The AO grid that changes nothing."""
    return np.ones((fc.N, fc.N, fc.N), F)


def setup(mode, split, where, moved=None, ka=0.4):
    """volume_shadow_cases.setup of the main case: (bricks, lo, hi, minv, camera, S, shading mode, parts, table)."""
    return swc.setup("main", split, where, mode, moved, ka=ka)


@functools.lru_cache(maxsize=None)
def reference(mode, split, where, clipped=False, ka=0.4, grid="main"):
    """The AO checker's frame of the case over the fog-shadowed base: (framebuffer, counters, depth plane or None).  grid: a key of SETS,
    or "ones".  clipped: under fc.depth_plane, with the identity matrix whatever the camera.  Computed once; read-only."""
    moved = False if clipped else CAMERAS[where]
    bricks, lo, hi, minv, cam, S, shading, parts, _ = setup(mode, split, where, moved, ka)
    plane = fc.depth_plane(parts, False, where) if clipped else None
    AO = ones() if grid == "ones" else ao_grid(mode, moved, grid)[0]
    fb, counters = ao.frame(bricks, lo, hi, minv, cam, S, shading, fgc.light_grid(mode, moved)[0], None, AO, plane, BIAS)
    fb.setflags(write=False)
    return fb, counters, plane


@functools.lru_cache(maxsize=None)
def base(mode, split, where, ka=0.4):
    """volume_fog_shadow_checker.frame of the case with ambient weight ka: (framebuffer, counters)."""
    moved = CAMERAS[where]
    bricks, lo, hi, minv, cam, S, shading, _, _ = setup(mode, split, where, moved, ka)
    fb, counters = fg.frame(bricks, lo, hi, minv, cam, S, shading, fgc.light_grid(mode, moved)[0], None, BIAS)
    fb.setflags(write=False)
    return fb, counters
