"""The cases of the shadowed-surface tests (tests/test_gpu_volume_shadow.py, tests/test_volume_shadow_host.py), on
tests/volume_fused_cases.py's 25^3 grid, 64 x 48 film, rate 1.7 and four brickings -- the smallest shapes at which macro cells are partial
and rays, shadow rays included, visit several bricks.

main      tests/volume_fused_shaded_cases.py's surfaces (isovalues 0.45 and 0.6, the slice plane through the middle, opacity 0.6), table
          "cool", the two lights below, bias 2.  The lights are where the shaded cases have them: there the checker alone already finds
          shadow rays of both kinds in numbers at the outside eye; of the shadow rays of the (1, 1, 1) bricking, outside eye under
          MOVED / inside eye:
              A_s == 0:  0.185 / 0.000        A_s > 0:  0.815 / 1.000
          (588 and 10,834 shadow rays).  tests/test_volume_shadow_host.py asserts at least a tenth of each at the outside eye; at the
          inside eye every crossing lies deep in the table's fog, which gives every shadow ray some opacity wherever the lights stand.
identity  a table without opacity, the slice plane alone, one light beyond the plane as seen from the outside eye: a shadow ray starts
          behind the plane and moves away from it, so no shadow ray meets a crossing and every T = 1.
occluder  the same table, two parallel planes of opacity 1 on either side of the middle, the light beyond both: a camera ray ends on the
          first plane it meets, and the shadow ray of a crossing on the near plane meets the far plane, T = 0.  Of the pixels that render
          a crossing, 0.84 have every T = 0 (asserted: at least half).

The numpy frames are computed once per case and shared; treat them as read-only."""
import functools

import numpy as np

from gravit_amd import scenes
from gravit_amd.adapter import TransferFunction
from tests import volume_checker as vc
from tests import volume_fused_cases as fc
from tests import volume_fused_shaded_cases as sh
from tests import volume_fused_shaded_checker as fs
from tests import volume_shade_checker as lc
from tests import volume_shadow_checker as sw
from tests import volume_surface_checker as sc
from tests.volume_common import read, tf

F = np.float32
BIAS = 2
LIGHTS = (((3.0, 4.0, 5.0), (1.0, 0.9, 0.8)), ((-2.0, 1.0, 0.5), (0.3, 0.4, 0.9)))
CAMERAS = sh.CAMERAS  # where -> under the MOVED matrix?
NORMAL = (0.3, 0.5, 0.8)  # of the slice planes
BEYOND = ((-1.5, -2.5, -4.0), (1.0, 0.9, 0.8))  # a light on the far side of the planes, seen from the outside eye: -5 * NORMAL
GAP = 0.06  # the occluder's planes lie at the middle's offset -+ GAP: 0.12 apart, more than five lattice steps


def clear_table():
    """[[0, 0], [1, 0]]: no opacity anywhere -- only the surfaces show."""
    return TransferFunction(read("CoolWarm.cmap", 4), np.array([[0, 0], [1, 0]], F), (0.0, 1.0))


def surfaces(case, mode="surf", ka=0.4, kd=0.6, scale=1.0):
    """(Surfaces, shading on?, table) of a case.  mode: the main case's -- "surf" or "surf_lit" (lit fog under table "spikes")."""
    if case == "main":
        S, on = sh.surfaces(mode, scale=scale, lights=LIGHTS, ka=ka, kd=kd)
        return S, on, tf(sh.MODES[mode])
    mid = sh.slice_plane()
    if case == "identity":
        return sc.Surfaces([], [mid], sh.OPACITY, [BEYOND], ka=ka, kd=kd), False, clear_table()
    if case == "occluder":
        planes = [NORMAL + (float(F(mid[3] + GAP)),), NORMAL + (float(F(mid[3] - GAP)),)]
        return sc.Surfaces([], planes, 1.0, [BEYOND], ka=ka, kd=kd), False, clear_table()
    raise KeyError(case)


def setup(case, split, where, mode="surf", moved=None, ka=0.4, kd=0.6):
    """(bricks of the checker, lo, hi, minv, camera, S, shading mode, parts, table) of a case.  moved: None = the camera's own matrix."""
    moved = CAMERAS[where] if moved is None else moved
    parts = fc.bricks_of(fc.volume(), split)
    m = fc.matrix(moved)
    lo, hi = fc.world_boxes(parts, m)
    S, on, table = surfaces(case, mode, ka, kd)
    bricks = [vc.Brick(b, table, fc.RATE) for b in parts]
    return bricks, lo, hi, scenes.instance_matrices(m)[0], fc.camera(where, moved), S, sh.shade_mode(on), parts, table


@functools.lru_cache(maxsize=None)
def reference(case, split, where, mode="surf", clipped=False, bias=BIAS, moved=None):
    """The shadow checker's frame of the case: (framebuffer, counters, details, depth plane or None).  clipped: under fc.depth_plane,
    with the identity matrix whatever the camera.  Computed once; read-only."""
    bricks, lo, hi, minv, cam, S, shading, parts, _ = setup(case, split, where, mode, False if clipped else moved)
    plane = fc.depth_plane(parts, False, where) if clipped else None
    fb, counters, details = sw.frame(bricks, lo, hi, minv, cam, S, shading, plane, bias)
    fb.setflags(write=False)
    return fb, counters, details, plane


@functools.lru_cache(maxsize=None)
def unshadowed(case, split, where, mode="surf", kd=0.6, moved=None):
    """volume_fused_shaded_checker.frame of the case (kd: the diffuse weight): (framebuffer, counters)."""
    bricks, lo, hi, minv, cam, S, shading, _, _ = setup(case, split, where, mode, moved, kd=kd)
    fb, counters = fs.frame(bricks, lo, hi, minv, cam, S, shading)
    fb.setflags(write=False)
    return fb, counters


def fully_shadowed(details, n_pix):
    """Per pixel: (renders a crossing, every shadow ray of every such sample has T = 0, i.e. A_s = 1)."""
    ids, A_s, usable = details["ids"], details["A_s"], details["usable"]
    has = np.zeros(n_pix, bool)
    has[ids] = True
    dark = np.ones(n_pix, bool)
    lit_somewhere = ~(A_s[:, usable] == F(1)).all(axis=1)
    dark[ids[lit_somewhere]] = False
    return has, has & dark
