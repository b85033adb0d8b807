"""The cases of the tests of shadows on AMR bricks (tests/test_volume_shadow_amr_host.py, tests/test_gpu_volume_shadow_amr.py):
tests/volume_fused_amr_cases.py's scene -- 21 x 19 x 18 vertices, subgrids S0 to S3, ratios 2 / 4 / 8, two levels below level 0 -- whole
and in 8 bricks by CUTS (two of them have subgrids), its two eyes, the thin table, rate 1.3, its surfaces of opacity 0.3 and its one
light; the biases of the shadow cases (2 for the crossings' rays, 1 for the light grid's).  The film is 32 x 24: the grid is what
exercises the descent and the cuts, the film only repeats it.

modes     surf, surf_lit: the shadowed frame (surf_lit: the fog lit and not shadowed) and -- surf_lit -- the fog- and mesh-shadowed
          frame's full kernels; lit: no surfaces, their lean kernels.
mesh      a tetrahedron inside S0's box (tests/test_gpu_volume_fused_amr.test_mixed_frame's), which shadows vertices inside and beyond
          the refined region.
buried    a volume whose opacity, and the one isovalue that is crossed, live in the subgrids alone: level 0 is 0.2 everywhere, which
          table "spikes" leaves transparent, S0 and S1 hold a field of 0.82 .. 0.98 that crosses the isovalue 0.9.  Only the merged ranges know.
blocked   every light blocked: blocked_surfaces below.
The numpy grids and frames are computed once per case and shared; treat them as read-only."""
import functools

import numpy as np

from gravit_amd import scenes
from tests import volume_amr_cases as cases
from tests import volume_amr_surface_cases as scases
from tests import volume_fused_amr_cases as fc
from tests import volume_mesh_shadow_checker as mg
from tests import volume_shade_checker as lc
from tests import volume_shadow_amr_checker as sa
from tests import volume_shadow_cases as swc
from tests.volume_common import IDENT, tf

F = np.float32
FILM = (32, 24)
RATE = fc.RATE
BIAS = swc.BIAS  # of the crossings' shadow rays
GRID_BIAS = 1    # of the light grid's
BRICKINGS = fc.BRICKINGS
EYES = fc.EYES
BURIED_ISO = 0.9


def camera(where):
    return fc.camera(where, *FILM)


def scene():
    return fc.scene()


def plain_scene():
    """The scene with its subgrids removed: the same level-0 grid."""
    vol = scene()
    return scenes.VolumeData(vol.data, vol.origin, vol.spacing)


def buried_scene():
    vol = cases.level0(np.full(cases.COUNTS[::-1], 0.2, F))

    def field(x, y, z):
        return 0.9 + 0.08 * np.sin(9.0 * x + 7.0 * y + 5.0 * z)

    s0 = scenes.refine(vol, cases.S0["lo"], cases.S0["cells"], cases.S0["ratio"], fn=field)
    scenes.refine(vol, cases.S1["lo"], cases.S1["cells"], cases.S1["ratio"], parent=s0, fn=field)
    return vol


def volume_of(which):
    return {"scene": scene, "plain": plain_scene, "buried": buried_scene}[which]()


def table_of(which):
    return tf("spikes") if which == "buried" else fc.thin()


def surfaces(mode, which="scene", lights=None, kd=scases.KD):
    """(S as the checkers take it, the shading mode) of a mode; .args / .light_args for the adapters where S has them."""
    vol = volume_of(which)
    if which == "buried":
        S = scases.surfaces(vol, isovalues=(BURIED_ISO,), plane=False, opacity=0.3, kd=kd)
    else:
        S = scases.surfaces(vol, opacity=0.3, kd=kd)
    if lights is not None:
        args, largs = S.args, dict(lights=list(lights), ka=S.ka, kd=S.kd)
        S = type(S)(S.iso, S.planes, S.opacity, list(lights), ka=S.ka, kd=S.kd)
        S.args, S.light_args = args, largs
    if mode == "lit":
        L = lc.lights_only(S.light_args["lights"], S.ka, S.kd)
        L.args, L.light_args = None, S.light_args
        return L, lc.SHADE_GRADIENT
    return S, (lc.SHADE_GRADIENT if mode == "surf_lit" else lc.SHADE_NONE)


def checker_bricks(which, bricking):
    return fc.checker_bricks(fc.parts_of(volume_of(which), bricking), table_of(which))


def mesh_scene(where="outside"):
    """The tetrahedron inside S0's box."""
    verts = np.array([[-1, -1, -1], [1, -1, -1], [0, 1, -1], [0, 0, 1]], F)
    tris = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]], np.int32)
    return scenes._assemble([scenes.MeshData(verts, tris)], [0], [scenes.mat_translate_scale(tuple(fc.s0_centre(scene())), (0.13, 0.13, 0.13))],
                            scenes.point_light((1.0, 2.0, 3.0)), camera(where), "tetrahedron")


@functools.lru_cache(maxsize=None)
def light_grid(which="scene", mode="surf_lit"):
    """The grid by definition -- the whole volume with its subgrids as ONE brick: (G (lights, gz, gy, gx), usable).  Read-only."""
    bricks, lo, hi = checker_bricks(which, 1)
    S, _ = surfaces(mode, which)
    G, usable = sa.grid(bricks[0], lo, hi, IDENT, IDENT, S, GRID_BIAS)
    G.setflags(write=False)
    return G, usable


@functools.lru_cache(maxsize=None)
def occluder_grid(mesh=True):
    """(O (lights, gz, gy, gx) uint8, usable, rays blocked) of the tetrahedron (mesh False: no mesh at all).  Read-only."""
    bricks, _, _ = checker_bricks("scene", 1)
    S, _ = surfaces("surf_lit")
    O, usable, blocked = mg.occluders(bricks[0], IDENT, mesh_scene() if mesh else None, S)
    O.setflags(write=False)
    return O, usable, blocked


@functools.lru_cache(maxsize=None)
def reference(kind, mode, bricking, where, which="scene", clipped=False, mesh=True):
    """The checker's frame of a case: (framebuffer, counters, depth plane or None).  kind: "shadow", "fog" or "mesh".  Read-only."""
    cam = camera(where)
    bricks, lo, hi = checker_bricks(which, bricking)
    S, shading = surfaces(mode, which)
    plane = fc.depth_plane(cam) if clipped else None
    G = light_grid(which, mode)[0] if kind in ("fog", "mesh") and shading == lc.SHADE_GRADIENT else None
    O = occluder_grid(mesh)[0] if kind == "mesh" else None
    fb, counters = sa.frame(bricks, lo, hi, IDENT, cam, S, shading, G, O, plane, BIAS)
    fb.setflags(write=False)
    return fb, counters, plane


@functools.lru_cache(maxsize=None)
def unshadowed(mode, bricking, where, kd=scases.KD):
    """tests/volume_fused_amr_checker.py's frame of the scene (kd: the diffuse weight): the framebuffer.  Read-only."""
    from tests import volume_fused_amr_checker as fa

    bricks, lo, hi = checker_bricks("scene", bricking)
    S, shading = surfaces(mode, kd=kd)
    fb, _ = fa.frame(bricks, lo, hi, IDENT, camera(where), S, shading)
    fb.setflags(write=False)
    return fb


def blocked_surfaces(kd=scases.KD):
    """tests/volume_shadow_cases.py's occluder construction on this scene: two parallel planes of opacity 1 on either side of S0's centre
    under a table without opacity, the light beyond both as seen from the outside eye.  A camera ray ends on the first plane it meets,
    and the shadow ray of a crossing on the near plane meets the far plane: T = 0.  Returns (S with .args / .light_args, table)."""
    from tests import volume_surface_checker as sc

    mid = scases.s0_plane(scene())
    planes = [mid[:3] + (float(F(mid[3] + swc.GAP)),), mid[:3] + (float(F(mid[3] - swc.GAP)),)]
    lights = [((-1.5, -2.5, -5.0), (1.0, 0.9, 0.8))]  # -5 * the planes' normal
    S = sc.Surfaces([], planes, 1.0, lights, ka=scases.KA, kd=kd)
    S.args = dict(isovalues=[], slices=planes, opacity=1.0)
    S.light_args = dict(lights=lights, ka=scases.KA, kd=kd)
    return S, swc.clear_table()


@functools.lru_cache(maxsize=None)
def blocked_reference(bricking):
    """The checker's shadowed frame of blocked_surfaces from the outside eye: (framebuffer, counters).  Read-only."""
    S, table = blocked_surfaces()
    bricks, lo, hi = fc.checker_bricks(fc.parts_of(scene(), bricking), table)
    fb, counters = sa.frame(bricks, lo, hi, IDENT, camera("outside"), S, lc.SHADE_NONE, None, None, None, BIAS)
    fb.setflags(write=False)
    return fb, counters
