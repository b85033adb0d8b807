"""The cases of the fused / shadowed CENTRAL tests (tests/test_gpu_volume_fused_central.py, tests/test_volume_fused_central_host.py): the
main cases of tests/volume_shadow_cases.py, tests/volume_fog_shadow_cases.py and tests/volume_mesh_shadow_cases.py -- the 25^3 grid, the
64 x 48 film, rate 1.7, their surfaces, lights, tables, cameras, light grids and occluder grids, all unchanged -- with bricks that carry
their ghost layers (scenes.split_volume(..., ghosts=True)) and a gradient kind; and tests/volume_smooth_cases.py's 19 x 14 x 11 grid,
whose split at (2, 2, 2) yields bricks of 6 and 7 cells along y, so that the face slabs' offsets differ from brick to brick.

The numpy frames (tests/volume_central_shadow_checker.py) are computed once per case and shared; treat them as read-only."""
import functools

from gravit_amd import scenes
from tests import volume_central_shadow_checker as cs
from tests import volume_fog_shadow_cases as fgc
from tests import volume_fused_cases as fc
from tests import volume_mesh_shadow_cases as mc
from tests import volume_shadow_cases as swc
from tests import volume_smooth_checker as sm

CELL, CENTRAL = cs.CELL, cs.CENTRAL
BIAS = swc.BIAS
FRAMES = ("plain", "shadow", "fog", "mesh")  # the shaded fused frame, gvt_hip_volume_frame_shadowed, _fog_shadowed, _mesh_shadowed


def parts_of(vol, split):
    """The bricks of a split with their ghost layers ((1, 1, 1): one brick, every face on the global boundary, no layer)."""
    return scenes.split_volume(vol, *split, ghosts=True)


def setup(mode, split, where, moved=None, kd=0.6):
    """volume_shadow_cases.setup of the main case with ghost-carrying bricks: (checker bricks, lo, hi, minv, camera, S, shading mode,
    parts, table)."""
    _, lo, hi, minv, cam, S, shading, _, table = swc.setup("main", split, where, mode, moved, kd=kd)
    parts = parts_of(fc.volume(), split)
    return [sm.Brick(b, table, fc.RATE) for b in parts], lo, hi, minv, cam, S, shading, parts, table


@functools.lru_cache(maxsize=None)
def reference(frame, mode, split, where, kind=CENTRAL, clipped=False, kd=0.6):
    """The checker's frame of a case: (framebuffer, counters, depth plane or None).  frame: one of FRAMES; clipped: under fc.depth_plane,
    with the identity matrix whatever the camera."""
    moved = False if clipped else swc.CAMERAS[where]
    bricks, lo, hi, minv, cam, S, shading, parts, _ = setup(mode, split, where, moved, kd)
    plane = fc.depth_plane(parts, False, where) if clipped else None
    G = fgc.light_grid(mode, moved)[0] if frame in ("fog", "mesh") and mode != "surf" else None
    O = mc.occluder_grid(moved)[0] if frame == "mesh" else None
    fb, counters = cs.frame(bricks, lo, hi, minv, cam, S, shading, kind, G, O, plane, BIAS, shadows=frame != "plain")
    fb.setflags(write=False)
    return fb, counters, plane
