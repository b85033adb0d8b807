"""The cases of the mesh-shadow tests (tests/test_gpu_volume_mesh_shadow.py, tests/test_volume_mesh_shadow_host.py), on
tests/volume_fog_shadow_cases.py's shapes: the 25^3 grid, the 64 x 48 film, rate 1.7, the four brickings, tests/volume_shadow_cases.py's
two lights, and three modes -- lit (fog alone), surf_lit (surfaces and lit fog), surf (surfaces, the fog unlit: no light grid).

THE SCENE is given in the volume's own space and placed by m, as fc.camera places the eye.  The object box is (-0.25, 0.1, -0.4) ..
(0.75, 1.2, 0.5), extent ext.  Two meshes in three instances:
    icosphere  one subdivision, 80 triangles, radius 0.3 * min(ext), centre lo + ext * (0.6, 0.55, 0.6); its instance carries a matrix
               with rotation and shear (tests/affine_cases.py, family "shear") and its vertices are pre-transformed by the inverse, so the
               world geometry is the sphere above
    plate      two triangles, centre lo + ext * (0.3, 0.35, 0.4), half-edges ext * (0.35, 0.05, 0) and ext * (0, 0.35, 0.08), under m
    plate      a second instance of it five extents below the volume: both lights stand above, so it lies outside every vertex ray and
               an instance that blocks nothing is in the loop
Measured with the CPU oracle (tests/test_volume_mesh_shadow_host.py asserts the bounds of the issue: blocked share in [0.10, 0.50],
cells with mixed corners >= 0.05, cells with all eight corners blocked >= 0.05), light (3, 4, 5) / light (-2, 1, 0.5):
    identity  blocked 0.214 / 0.150   mixed 0.103 / 0.114   all blocked 0.180 / 0.110
    MOVED     the same to three digits
Pixels of the 64 x 48 film on which the mesh-shadowed checker frame differs from the fog-shadowed one (at least 200 per mode is
asserted; inside eye, 2 x 2 x 2 bricks; measured): lit 3,072, surf_lit 3,072, surf 3,072 of 3,072 -- the plate stands between the inside
eye's view and both lights, so every pixel has a shaded sample in its shadow.

The numpy grids and frames are computed once per case and shared; treat them as read-only."""
import functools

import numpy as np

from gravit_amd import scenes
from gravit_amd.layouts import default_material
from tests import affine_cases as ac
from tests import volume_checker as vc
from tests import volume_fog_shadow_cases as fgc
from tests import volume_fused_cases as fc
from tests import volume_mesh_shadow_checker as mg
from tests import volume_shadow_cases as swc

F = np.float32
MODES = ("lit", "surf_lit", "surf")
BIAS = fgc.BIAS
GRID_BIAS = fgc.GRID_BIAS
LIGHTS = swc.LIGHTS
CAMERAS = fgc.CAMERAS
SHEAR_SEED = 1  # of the icosphere's instance matrix


def icosphere():
    """(verts float64 (42, 3) on the unit sphere, tris (80, 3)): the icosahedron, every triangle split in four."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    v = [np.asarray(p, np.float64) / np.linalg.norm(p) for p in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    mid = {}

    def middle(a, b):
        key = (min(a, b), max(a, b))
        if key not in mid:
            p = v[a] + v[b]
            v.append(p / np.linalg.norm(p))
            mid[key] = len(v) - 1
        return mid[key]

    out = []
    for a, b, c in f:
        ab, bc, ca = middle(a, b), middle(b, c), middle(c, a)
        out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
    return np.array(v, np.float64), np.array(out, np.int32)


def _apply(m16, p):
    """m (glm column-major) applied to points, in float64."""
    M = np.asarray(m16, np.float64).reshape(4, 4).T
    return np.asarray(p, np.float64) @ M[:3, :3].T + M[:3, 3]


@functools.lru_cache(maxsize=None)
def scene(moved, sphere_shift=(0.0, 0.0, 0.0)):
    """The scenes.Scene of the case under the volume's matrix.  sphere_shift: the icosphere moved by that share of ext (a moved mesh)."""
    m = fc.matrix(moved)
    vol = fc.volume()
    lo = vol.origin.astype(np.float64)
    ext = (vol.counts - 1) * vol.spacing.astype(np.float64)
    sv, st = icosphere()
    centre = lo + ext * (np.array([0.6, 0.55, 0.6]) + np.asarray(sphere_shift, np.float64))
    sphere_world = _apply(m, centre + sv * (0.3 * ext.min()))
    m_sphere = ac.matrix("shear", SHEAR_SEED)
    sphere_obj = _apply(np.linalg.inv(np.asarray(m_sphere, np.float64).reshape(4, 4).T).T.reshape(16), sphere_world)
    c = lo + ext * np.array([0.3, 0.35, 0.4])
    u, w = ext * np.array([0.35, 0.05, 0.0]), ext * np.array([0.0, 0.35, 0.08])
    plate = np.array([c - u - w, c + u - w, c + u + w, c - u + w], np.float64)
    meshes = [scenes.MeshData(sphere_obj.astype(F), st, default_material()),
              scenes.MeshData(plate.astype(F), np.array([(0, 1, 2), (0, 2, 3)], np.int32), default_material())]
    below = (np.asarray(m, np.float64).reshape(4, 4).T @ np.array([[1, 0, 0, 0], [0, 1, 0, -5.0 * ext[1]], [0, 0, 1, 0], [0, 0, 0, 1]], np.float64))
    mats = [m_sphere, np.asarray(m, F), np.ascontiguousarray(below.T, F).reshape(16)]
    from gravit_amd.layouts import point_light

    return scenes._assemble(meshes, [0, 1, 1], mats, point_light((0.0, 3.0, 3.0), (1.0, 1.0, 1.0)), fc.camera("outside", moved), "mesh-shadow-%d" % int(moved))


def wall_scene(moved):
    """A scene that blocks every vertex ray: two huge plates, each across one light's direction, beyond the volume on the lights' side."""
    m = fc.matrix(moved)
    vol = fc.volume()
    lo = vol.origin.astype(np.float64)
    ext = (vol.counts - 1) * vol.spacing.astype(np.float64)
    mid = lo + 0.5 * ext
    verts, tris = [], []
    for pos, _ in LIGHTS:
        d = np.asarray(pos, np.float64) / np.linalg.norm(pos)
        a = np.cross(d, (0.0, 0.0, 1.0))
        a /= np.linalg.norm(a)
        b = np.cross(d, a)
        c = mid + 4.0 * d
        n = len(verts)
        verts += [c + 40.0 * (-a - b), c + 40.0 * (a - b), c + 40.0 * (a + b), c + 40.0 * (-a + b)]
        tris += [(n, n + 1, n + 2), (n, n + 2, n + 3)]
    from gravit_amd.layouts import point_light

    # (the lights' directions are world directions: the plates are built in world space around the placed volume's middle, scaled with it)
    M = np.asarray(m, np.float64).reshape(4, 4).T
    world = (np.asarray(verts) - mid) * np.abs(np.diag(M[:3, :3])).max() + _apply(m, mid)
    mesh = scenes.MeshData(world.astype(F), np.array(tris, np.int32), default_material())
    return scenes._assemble([mesh], [0], [scenes.mat_translate_scale((0, 0, 0), (1, 1, 1))], point_light((0.0, 3.0, 3.0), (1.0, 1.0, 1.0)),
                            fc.camera("outside", moved), "mesh-shadow-wall")


def whole(mode, moved):
    """volume_fog_shadow_cases.whole for the three modes: (brick of the whole grid, lo, hi, m, minv, S, shading mode)."""
    bricks, lo, hi, minv, _, S, shading, _, _ = swc.setup("main", (1, 1, 1), "outside", mode, moved)
    return bricks[0], lo, hi, fc.matrix(moved), minv, S, shading


@functools.lru_cache(maxsize=None)
def occluder_grid(moved, which="case"):
    """(O (lights, gz, gy, gx) uint8, usable, rays blocked) of the case's scene (O does not depend on the mode).  which: "case", "none"
    (no mesh), "wall" (everything blocked) or "shifted" (the icosphere moved).  Computed once; read-only."""
    B, _, _, m, _, S, _ = whole("lit", moved)
    sc_ = {"case": lambda: scene(moved), "none": lambda: None, "wall": lambda: wall_scene(moved), "shifted": lambda: scene(moved, (-0.2, 0.0, -0.15))}[which]()
    O, usable, blocked = mg.occluders(B, m, sc_, S)
    O.setflags(write=False)
    return O, usable, blocked


def light_grid(mode, moved):
    """The fog checker's light grid of a mode, or None where the fog is not lit (mode "surf")."""
    return None if mode == "surf" else fgc.light_grid(mode, moved)[0]


def cell_shares(O1):
    """Of one light's plane: (blocked share of the vertices, share of the cells with mixed corners, share with all eight blocked)."""
    z = O1 == 0
    s = sum(z[k:z.shape[0] - 1 + k, j:z.shape[1] - 1 + j, i:z.shape[2] - 1 + i].astype(np.int64) for k in (0, 1) for j in (0, 1) for i in (0, 1))
    return float(z.mean()), float(((s > 0) & (s < 8)).mean()), float((s == 8).mean())


def setup(mode, split, where, moved=None, kd=0.6):
    """volume_shadow_cases.setup of the main case: (bricks, lo, hi, minv, camera, S, shading mode, parts, table)."""
    return swc.setup("main", split, where, mode, moved, kd=kd)


@functools.lru_cache(maxsize=None)
def reference(mode, split, where, clipped=False, which="case", kd=0.6):
    """The mesh checker's frame of the case: (framebuffer, counters, depth plane or None).  clipped: under fc.depth_plane, with the
    identity matrix whatever the camera.  Computed once; read-only."""
    moved = False if clipped else CAMERAS[where]
    bricks, lo, hi, minv, cam, S, shading, parts, _ = setup(mode, split, where, moved, kd)
    plane = fc.depth_plane(parts, False, where) if clipped else None
    fb, counters = mg.frame(bricks, lo, hi, minv, cam, S, shading, light_grid(mode, moved), occluder_grid(moved, which)[0], plane, BIAS)
    fb.setflags(write=False)
    return fb, counters, plane


@functools.lru_cache(maxsize=None)
def fog_reference(mode, split, where, kd=0.6):
    """volume_fog_shadow_checker.frame of the case (mode "surf": G = None, the shadowed frame): (framebuffer, counters)."""
    from tests import volume_fog_shadow_checker as fg

    moved = CAMERAS[where]
    bricks, lo, hi, minv, cam, S, shading, _, _ = setup(mode, split, where, moved, kd)
    fb, counters = fg.frame(bricks, lo, hi, minv, cam, S, shading, light_grid(mode, moved), None, BIAS)
    fb.setflags(write=False)
    return fb, counters
