"""Scene inputs for the adapter path: the reference's two golden scenes, the BASELINE.json
synthetic configurations, and tiny OBJ / PLY readers.  Pure numpy, no device code.

Citations are relative to the GraviT tree (/root/reference in the build container).
"""
import os
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

from .layouts import LIGHT_DTYPE, MATERIAL_DTYPE, default_material, point_light

F = np.float32


@dataclass
class MeshData:
    """gvt::render::data::primitives::Mesh inputs (Mesh.h:87-100): 0-based faces."""

    verts: np.ndarray  # (nV,3) f32
    tris: np.ndarray  # (nT,3) i32
    material: np.ndarray = field(default_factory=default_material)  # Mesh::mat
    vnormals: Optional[np.ndarray] = None
    vcolors: Optional[np.ndarray] = None
    materials: Optional[np.ndarray] = None  # faces_to_materials table
    face_mat: Optional[np.ndarray] = None

    def bbox(self):
        v = self.verts  # per column: a min over axis 0 of an (n, 3) array walks three-element rows (1.5 s at 30 M vertices; this: 0.1 s)
        return np.array([v[:, k].min() for k in range(3)], F), np.array([v[:, k].max() for k in range(3)], F)


@dataclass
class Camera:
    """gvtPerspectiveCamera parameters (gvtCamera.cpp:233-312); fov in radians."""

    eye: tuple
    focus: tuple
    up: tuple
    fov: float
    width: int
    height: int
    samples: int = 1
    depth: int = 1
    jitter: float = 0.0


@dataclass
class Scene:
    meshes: List[MeshData]
    inst_mesh: List[int]  # instance -> mesh index
    m: np.ndarray  # (nInst,16) glm column-major
    minv: np.ndarray  # (nInst,16)
    normi: np.ndarray  # (nInst,9)
    inst_lo: np.ndarray  # (nInst,3) world AABB (api.cpp:309-312)
    inst_hi: np.ndarray
    lights: np.ndarray  # LIGHT_DTYPE
    camera: Camera
    name: str = ""

    @property
    def n_inst(self):
        return len(self.inst_mesh)


# ------------------------------------------------------------------ matrices (glm, column-major)
def mat_translate_scale(t, s):
    """glm::scale(glm::translate(I, t), s) as 16 floats, column-major (SimpleApp.cpp:166-168)."""
    m = np.zeros((4, 4), F)  # m[col][row]
    m[0, 0], m[1, 1], m[2, 2] = F(s[0]), F(s[1]), F(s[2])
    m[3, 0], m[3, 1], m[3, 2], m[3, 3] = F(t[0]), F(t[1]), F(t[2]), F(1)
    return m.reshape(16)


def instance_matrices(m16):
    """minv = inverse(m), normi = transpose(inverse(mat3(m)))  (api.cpp:307-308)."""
    M = m16.reshape(4, 4).T.astype(np.float64)  # row-major math matrix
    Minv = np.linalg.inv(M)
    minv = Minv.T.astype(F).reshape(16)
    N = np.linalg.inv(M[:3, :3]).T  # math matrix of normi
    normi = N.T.astype(F).reshape(9)  # column-major storage
    return minv, normi


def instance_bbox(m16, lo, hi):
    """The world box of all eight corners of [lo, hi] taken through M.  A departure from the reference, which transforms only the two
    corners, Box3D(M*min, M*max) (api.cpp:309-312): it never builds a rotated instance, and under a rotation that is no multiple of 90
    degrees the box of two corners does not contain the instance -- the top level would cull rays that hit it.  Where M's 3x3 block is
    diagonal (every scene the reference builds) each world coordinate depends on one object coordinate alone, and the result is the
    two-corner box bit for bit: the corners go through the same float32 product as before."""
    M = m16.reshape(4, 4).T
    c = [(M @ np.array([x, y, z, 1], F)).astype(F)[:3] for z in (lo[2], hi[2]) for y in (lo[1], hi[1]) for x in (lo[0], hi[0])]
    a, b = c[0], c[7]  # M*min and M*max first, as before
    lo_w, hi_w = np.minimum(a, b), np.maximum(a, b)
    for p in c[1:7]:
        lo_w, hi_w = np.minimum(lo_w, p), np.maximum(hi_w, p)
    return lo_w, hi_w


def add_faces_1based(verts, faces1):
    """Mesh::addFace (Mesh.cpp:102-112): 1-based indices, faces with coincident vertices are dropped."""
    out = []
    for a, b, c in np.asarray(faces1).reshape(-1, 3):
        va, vb, vc = verts[a - 1], verts[b - 1], verts[c - 1]
        if (va == vb).all() or (vb == vc).all() or (vc == va).all():
            continue
        out.append((a - 1, b - 1, c - 1))
    return np.array(out, np.int32).reshape(-1, 3)


def _assemble(meshes, inst_mesh, mats, lights, camera, name):
    minv, normi, lo, hi = [], [], [], []
    for i, m in zip(inst_mesh, mats):
        a, b = instance_matrices(m)
        minv.append(a)
        normi.append(b)
        l, h = instance_bbox(m, *meshes[i].bbox())
        lo.append(l)
        hi.append(h)
    return Scene(meshes, list(inst_mesh), np.array(mats, F).reshape(-1, 16), np.array(minv, F).reshape(-1, 16),
                 np.array(normi, F).reshape(-1, 9), np.array(lo, F).reshape(-1, 3), np.array(hi, F).reshape(-1, 3),
                 np.ascontiguousarray(lights, LIGHT_DTYPE), camera, name)


# ------------------------------------------------------------------ golden scene 1: gvtSimple
def simple_scene(width=512, height=512):
    """The 5x5 cone/cube grid of src/apps/render/SimpleApp.cpp:82-233 (golden simple.ppm)."""
    cone_v = np.array([0.5, 0.0, 0.0, -0.5, 0.5, 0.0, -0.5, 0.25, 0.433013, -0.5, -0.25, 0.43013, -0.5, -0.5, 0.0, -0.5, -0.25,
                       -0.433013, -0.5, 0.25, -0.433013], F).reshape(-1, 3)
    cone_f = [1, 2, 3, 1, 3, 4, 1, 4, 5, 1, 5, 6, 1, 6, 7, 1, 7, 2]
    cube_v = np.array([-0.5, -0.5, 0.5, 0.5, -0.5, 0.5, 0.5, 0.5, 0.5, -0.5, 0.5, 0.5, -0.5, -0.5, -0.5, 0.5, -0.5, -0.5, 0.5, 0.5,
                       -0.5, -0.5, 0.5, -0.5, 0.5, 0.5, 0.5, -0.5, 0.5, 0.5, 0.5, 0.5, -0.5, -0.5, 0.5, -0.5, -0.5, -0.5, 0.5, 0.5,
                       -0.5, 0.5, -0.5, -0.5, -0.5, 0.5, -0.5, -0.5, 0.5, -0.5, 0.5, 0.5, 0.5, 0.5, 0.5, -0.5, -0.5, 0.5, 0.5, -0.5,
                       -0.5, -0.5, 0.5, -0.5, 0.5, 0.5, -0.5, -0.5, -0.5, -0.5, 0.5, -0.5], F).reshape(-1, 3)
    cube_f = [1, 2, 3, 1, 3, 4, 17, 19, 20, 17, 20, 18, 6, 5, 8, 6, 8, 7, 23, 21, 22, 23, 22, 24, 10, 9, 11, 10, 11, 12, 13, 15,
              16, 13, 16, 14]
    white = default_material(kd=(1.0, 1.0, 1.0))  # addMeshMaterial(LAMBERT, kd=1, alpha=1) api.cpp:228-236
    cone = MeshData(cone_v, add_faces_1based(cone_v, cone_f), white)
    cube = MeshData(cube_v, add_faces_1based(cube_v, cube_f), white)
    mats, inst_mesh = [], []
    inst = 0
    for i in range(-2, 3):
        for j in range(-2, 3):
            mats.append(mat_translate_scale((0.0, i * 0.5, j * 0.5), (0.4, 0.4, 0.4)))
            inst_mesh.append(1 if inst % 2 else 0)
            inst += 1
    cam = Camera((4.0, 0.0, 0.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), float(F(45.0 * np.pi / 180.0)), width, height, 1, 1, 0.5)
    return _assemble([cone, cube], inst_mesh, mats, point_light((1.0, 0.0, -1.0)), cam, "simple")


# ------------------------------------------------------------------ readers
def read_obj(path):
    """Vertices and triangles of a Wavefront OBJ (faces 0-based, no degenerate filter, like
    data/reader/ObjReader.cpp:122-135 which pushes tinyobj faces straight into Mesh::faces)."""
    vs, fs = [], []
    with open(path) as f:
        for line in f:
            if line.startswith("v "):
                p = line.split()
                vs.append((float(p[1]), float(p[2]), float(p[3])))
            elif line.startswith("f "):
                idx = [int(tok.split("/")[0]) for tok in line.split()[1:]]
                idx = [i - 1 if i > 0 else len(vs) + i for i in idx]
                for k in range(1, len(idx) - 1):  # fan-triangulate like tinyobj
                    fs.append((idx[0], idx[k], idx[k + 1]))
    return np.array(vs, F).reshape(-1, 3), np.array(fs, np.int32).reshape(-1, 3)


_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
              "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}


def read_ply_full(path):
    """PLY as PlyReader.cpp:54-176 takes it through ply.c: `ascii`, `binary_little_endian` or `binary_big_endian`; a `vertex` element whose
    x y z become the positions and -- when it has more than five properties (PlyReader.cpp:123) -- whose red green blue (uchar) become vertex
    colours / 255; a `face` element with one list property of 3 indices (PlyReader.cpp:163-167 copies verts[0..2]).  Other elements
    are skipped.  Returns (verts f32 [nv,3], tris i32 [nf,3], colors f32 [nv,3] or None)."""
    with open(path, "rb") as f:
        if f.readline().strip() != b"ply":
            raise ValueError("%s: not a PLY file" % path)
        fmt, elems = None, []  # elems: [name, count, [(prop name, type) | (prop name, count type, item type)]]
        while True:
            line = f.readline()
            if not line:
                raise ValueError("%s: PLY header has no end_header" % path)
            w = line.decode("ascii", "replace").split()
            if not w or w[0] in ("comment", "obj_info"):
                continue
            if w[0] == "format":
                fmt = w[1]
            elif w[0] == "element":
                elems.append([w[1], int(w[2]), []])
            elif w[0] == "property":
                elems[-1][2].append((w[-1], w[2], w[3]) if w[1] == "list" else (w[-1], w[1]))
            elif w[0] == "end_header":
                break
        if fmt not in ("ascii", "binary_little_endian", "binary_big_endian"):
            raise ValueError("%s: PLY format %r" % (path, fmt))
        body = f.read()
    verts = tris = colors = None
    end = "<" if fmt != "binary_big_endian" else ">"
    if fmt == "ascii":
        tok = body.split()
        pos = 0
    else:
        pos = 0
    for name, cnt, props in elems:
        scalar = all(len(p) == 2 for p in props)
        if fmt == "ascii":
            if scalar:
                arr = np.array(tok[pos : pos + cnt * len(props)], dtype=np.float64).reshape(cnt, len(props))
                pos += cnt * len(props)
                cols = {p[0]: arr[:, i] for i, p in enumerate(props)}
            else:
                if len(props) != 1:
                    raise ValueError("%s: element %s mixes list and scalar properties" % (path, name))
                rows = []
                for _ in range(cnt):
                    k = int(tok[pos])
                    rows.append(tok[pos + 1 : pos + 1 + k])
                    pos += 1 + k
                cols = {props[0][0]: rows}
        else:
            if scalar:
                dt = np.dtype([(p[0], end + _PLY_TYPES[p[1]]) for p in props])
                arr = np.frombuffer(body, dt, cnt, pos)
                pos += cnt * dt.itemsize
                cols = {p[0]: arr[p[0]] for p in props}
            else:
                if len(props) != 1:
                    raise ValueError("%s: element %s mixes list and scalar properties" % (path, name))
                ct, it = np.dtype(end + _PLY_TYPES[props[0][1]]), np.dtype(end + _PLY_TYPES[props[0][2]])
                k0 = int(np.frombuffer(body, ct, 1, pos)[0]) if cnt else 0
                rec = np.dtype([("n", ct), ("v", it, (k0,))])
                arr = np.frombuffer(body, rec, cnt, pos)  # the common case: every list has the first one's length (checked below)
                if cnt and not (arr["n"] == k0).all():
                    rows, q = [], pos
                    for _ in range(cnt):
                        k = int(np.frombuffer(body, ct, 1, q)[0])
                        rows.append(np.frombuffer(body, it, k, q + ct.itemsize))
                        q += ct.itemsize + k * it.itemsize
                    pos, cols = q, {props[0][0]: rows}
                else:
                    pos += cnt * rec.itemsize
                    cols = {props[0][0]: arr["v"]}
        if name == "vertex":
            verts = np.stack([np.asarray(cols[a], dtype=np.float64) for a in ("x", "y", "z")], axis=1).astype(F)
            if len(props) > 5 and all(c in cols for c in ("red", "green", "blue")):
                colors = (np.stack([np.asarray(cols[c], dtype=np.float64) for c in ("red", "green", "blue")], axis=1) / 255.0).astype(F)
        elif name == "face":
            rows = cols[props[0][0]]
            if any(len(r) != 3 for r in rows):
                raise ValueError("%s: faces must be triangles (PlyReader.cpp:163-167 reads three indices)" % path)
            tris = np.asarray(rows, dtype=np.int64).reshape(cnt, 3).astype(np.int32)
    if verts is None or tris is None:
        raise ValueError("%s: PLY needs a vertex and a face element" % path)
    if tris.size and (tris.min() < 0 or tris.max() >= len(verts)):
        raise ValueError("%s: face index out of range" % path)
    return verts, tris, colors


def read_ply(path):
    """(verts, tris) of a PLY file (data/geom/bunny/reconstruction/*.ply); colours: read_ply_full."""
    v, t, _ = read_ply_full(path)
    return v, t


def load_mesh_file(path):
    if path.endswith(".npz"):
        d = np.load(path)
        return d["verts"].astype(F), d["tris"].astype(np.int32)
    if path.endswith(".ply"):
        return read_ply(path)
    return read_obj(path)


GOLDEN_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")


# ------------------------------------------------------------------ golden scene 2: bunny.obj
def bunny_scene(width=512, height=512, path=None):
    """src/apps/render/SimpleFileLoadApp.cpp:186-241 (golden bunny.ppm): identity instance, default material."""
    v, t = load_mesh_file(path or os.path.join(GOLDEN_DIR, "bunny.obj"))
    mesh = MeshData(v, t, default_material())
    cam = Camera((0.0, 0.1, 0.3), (0.0, 0.1, -0.3), (0.0, 1.0, 0.0), float(F(45.0 * np.pi / 180.0)), width, height, 1, 1, 0.0)
    return _assemble([mesh], [0], [mat_translate_scale((0, 0, 0), (1, 1, 1))], point_light((0.0, 0.1, 0.5)), cam, "bunny")


def bunny70k_scene(width=1920, height=1080, path=None):
    """BASELINE config 2: bun_zipper (69,451 tris), single domain, depth 1, camera framing the bbox."""
    v, t = load_mesh_file(path or os.path.join(GOLDEN_DIR, "bun_zipper.npz"))
    mesh = MeshData(v, t, default_material())
    lo, hi = mesh.bbox()
    c = 0.5 * (lo + hi)
    cam = Camera((float(c[0]), float(c[1]), float(c[2] + 0.35)), (float(c[0]), float(c[1]), float(c[2])), (0.0, 1.0, 0.0),
                 float(F(30.0 * np.pi / 180.0)), width, height, 1, 1, 0.0)
    light = point_light((float(c[0]), float(c[1] + 0.1), float(c[2] + 0.5)))
    return _assemble([mesh], [0], [mat_translate_scale((0, 0, 0), (1, 1, 1))], light, cam, "bunny70k")


def bunny_grid_scene(nx=4, ny=2, pitch=0.3, width=1900, height=1080, path=None):
    """BASELINE config 4: nx*ny bunny instances on a grid (pitch like data/bunny.conf:27-29, film data/bunny.conf:8)."""
    v, t = load_mesh_file(path or os.path.join(GOLDEN_DIR, "bunny.obj"))
    mesh = MeshData(v, t, default_material())
    mats = []
    for j in range(ny):
        for i in range(nx):
            mats.append(mat_translate_scale(((i - (nx - 1) / 2) * pitch, (j - (ny - 1) / 2) * pitch, 0.0), (1, 1, 1)))
    cam = Camera((0.0, 0.1, 1.6), (0.0, 0.1, 0.0), (0.0, 1.0, 0.0), float(F(40.0 * np.pi / 180.0)), width, height, 1, 1, 0.0)
    return _assemble([mesh], [0] * (nx * ny), mats, point_light((0.9, 0.25, 0.25)), cam, "bunny-grid-%dx%d" % (nx, ny))  # light low and to the side: shadow rays cross neighbouring domains


# ------------------------------------------------------------------ synthetic soups
def triangle_soup(n_tris, seed=12345, half_extent=0.005):
    """BASELINE config 3 geometry: centres U[0,1]^3, 3 offsets U[-s,s]^3 each, unshared vertices.
    Generator: numpy Philox(seed), float32 draws."""
    rng = np.random.Generator(np.random.Philox(seed))
    c = rng.random((n_tris, 1, 3), dtype=F)
    o = rng.random((n_tris, 3, 3), dtype=F)  # (in place from here: the same float32 operations in the same order, no 360 MB temporaries)
    o *= F(2.0); o -= F(1.0); o *= F(half_extent); o += c
    tris = np.arange(n_tris * 3, dtype=np.int32).reshape(-1, 3)
    return o.reshape(-1, 3), tris


def soup_scene(n_tris=10_000_000, width=1920, height=1080, seed=12345, half_extent=0.005):
    """BASELINE config 3: eye (.5,.5,3) -> (.5,.5,.5), fov 30 deg, light at the eye, kd .5, depth 1."""
    v, t = triangle_soup(n_tris, seed, half_extent)
    mesh = MeshData(v, t, default_material())
    cam = Camera((0.5, 0.5, 3.0), (0.5, 0.5, 0.5), (0.0, 1.0, 0.0), float(F(30.0 * np.pi / 180.0)), width, height, 1, 1, 0.0)
    return _assemble([mesh], [0], [mat_translate_scale((0, 0, 0), (1, 1, 1))], point_light((0.5, 0.5, 3.0)), cam,
                     "soup-%d" % n_tris)


def cathedral_scene(width=512, height=512, samples=2, depth=2, seed=7, eye=(0.0, 1.5, 9.0), light=(0.0, 2.5, 4.0)):
    """BASELINE config 5 stand-in (sibenik.obj is missing from the reference, .MISSING_LARGE_BLOBS):
    a hall of long thin triangles (~80 K; floor, ceiling, side walls, back wall, two rows of columns; open at z = +10) --
    deep BVH, AO-style secondary rays.  The default eye stands inside the hall (adapter-level tests: the schedulers never
    assign a ray to an instance box it starts in, RayPacket.h:195-197); whole-frame tests look in from outside, e.g.
    eye=(0, 1.5, 13), with the light in front of the opening, e.g. light=(0, 2.5, 12): a shadow ray is occluded by anything on the
    whole half-line (tfar = FLT_MAX, EmbreeMeshAdapter.cpp:364-385), so a light inside the hall lights next to nothing."""
    rng = np.random.Generator(np.random.Philox(seed))
    vs, fs = [], []

    def quad_strip(p0, du, dv, nu, nv):
        base = len(vs)
        for j in range(nv + 1):
            for i in range(nu + 1):
                vs.append(p0 + du * (i / nu) + dv * (j / nv))
        for j in range(nv):
            for i in range(nu):
                a = base + j * (nu + 1) + i
                fs.append((a, a + 1, a + nu + 2))
                fs.append((a, a + nu + 2, a + nu + 1))

    X, Y, Z = 4.0, 3.0, 10.0
    e = lambda *a: np.array(a, np.float64)
    n_long, n_thin = 4, 1250  # long thin slivers along z
    quad_strip(e(-X, 0, -Z), e(2 * X, 0, 0), e(0, 0, 2 * Z), n_thin, n_long)  # floor
    quad_strip(e(-X, Y, -Z), e(0, 0, 2 * Z), e(2 * X, 0, 0), n_long, n_thin)  # ceiling
    quad_strip(e(-X, 0, -Z), e(0, 0, 2 * Z), e(0, Y, 0), n_long, n_thin)  # left wall
    quad_strip(e(X, 0, -Z), e(0, Y, 0), e(0, 0, 2 * Z), n_thin, n_long)  # right wall
    quad_strip(e(-X, 0, -Z), e(0, Y, 0), e(2 * X, 0, 0), 50, 50)  # back
    for k in range(12):  # columns: thin tall quads
        cx = (-1 if k % 2 else 1) * 2.0
        cz = -8.0 + (k // 2) * 3.0
        for s in range(16):
            a0, a1 = 2 * np.pi * s / 16, 2 * np.pi * (s + 1) / 16
            p0 = e(cx + 0.3 * np.cos(a0), 0, cz + 0.3 * np.sin(a0))
            p1 = e(cx + 0.3 * np.cos(a1), 0, cz + 0.3 * np.sin(a1))
            quad_strip(p0, p1 - p0, e(0, Y, 0), 1, 150)
    v = np.array(vs, F)
    v += (rng.random(v.shape, dtype=F) - F(0.5)) * F(1e-3)
    mesh = MeshData(v, np.array(fs, np.int32), default_material(kd=(0.8, 0.8, 0.8)))
    cam = Camera(tuple(eye), (0.0, 1.4, 0.0), (0.0, 1.0, 0.0), float(F(60.0 * np.pi / 180.0)), width, height, samples, depth, 0.0)
    return _assemble([mesh], [0], [mat_translate_scale((0, 0, 0), (1, 1, 1))], point_light(tuple(light)), cam, "cathedral")


def split_into_domains(scene, n_domains, axis=2):
    """A one-mesh scene cut into n_domains spatial domains along `axis` (triangles assigned by centroid slab, vertices
    re-indexed per domain; one Mesh + the original instance matrix each) -- what a GraviT application does when it hands the
    Domain scheduler one mesh per rank (DomainTracer.h:115-144)."""
    assert len(scene.meshes) == 1 and scene.n_inst == 1
    m = scene.meshes[0]
    lo, hi = m.bbox()
    c = m.verts[m.tris].mean(axis=1)[:, axis]
    cell = np.clip(((c - lo[axis]) / max(float(hi[axis] - lo[axis]), 1e-30) * n_domains).astype(np.int64), 0, n_domains - 1)
    meshes, mats = [], []
    for d in range(n_domains):
        sel = m.tris[cell == d]
        used, inv = np.unique(sel.reshape(-1), return_inverse=True)
        meshes.append(MeshData(np.ascontiguousarray(m.verts[used]), inv.astype(np.int32).reshape(-1, 3), m.material))
        mats.append(scene.m[0].reshape(16))
    return _assemble(meshes, list(range(n_domains)), mats, scene.lights, scene.camera, "%s-dom%d" % (scene.name, n_domains))


# ------------------------------------------------------------------ domain decomposition of the soup
def domain_grid(n_domains):
    """x-y tiling first (rays of the config-3 camera travel along -z), then z."""
    return {1: (1, 1, 1), 2: (2, 1, 1), 4: (2, 2, 1), 8: (4, 2, 1), 16: (4, 4, 1)}.get(n_domains, (n_domains, 1, 1))


def soup_domains_scene(n_tris=10_000_000, n_domains=8, width=1920, height=1080, seed=12345, half_extent=0.005):
    """The config-3 soup cut into n_domains spatial domains (one Mesh + identity instance each, triangles assigned
    by centroid cell), the layout GraviT's Domain scheduler distributes over ranks (DomainTracer.h:115-144)."""
    v, t = triangle_soup(n_tris, seed, half_extent)
    gx, gy, gz = domain_grid(n_domains)
    tv = v.reshape(-1, 3, 3)

    def cell_of(k, g):  # the centroid's cell along axis k: float32 mean over the three vertices, as np.mean(axis=1) adds them (v0 + v1 + v2, then / 3)
        if g == 1:
            return 0
        ck = (tv[:, 0, k] + tv[:, 1, k] + tv[:, 2, k]) / F(3.0)
        return np.clip((ck * g).astype(np.int32), 0, g - 1)

    cell = (cell_of(2, gz) * gy + cell_of(1, gy)) * gx + cell_of(0, gx)
    meshes, mats = [], []
    tri_verts = v.reshape(-1, 3, 3)
    for d in range(gx * gy * gz):
        sel = np.nonzero(cell == d)[0]
        dv = np.ascontiguousarray(tri_verts[sel].reshape(-1, 3))
        dt = np.arange(len(sel) * 3, dtype=np.int32).reshape(-1, 3)
        meshes.append(MeshData(dv, dt, default_material()))
        mats.append(mat_translate_scale((0, 0, 0), (1, 1, 1)))
    cam = Camera((0.5, 0.5, 3.0), (0.5, 0.5, 0.5), (0.0, 1.0, 0.0), float(F(30.0 * np.pi / 180.0)), width, height, 1, 1, 0.0)
    return _assemble(meshes, list(range(len(meshes))), mats, point_light((0.5, 0.5, 3.0)), cam, "soup-%d-dom%d" % (n_tris, n_domains))


def soup_weak_tile(d, n_tiles, n_per_tile, seed=12345, half_extent=None):
    """Tile d of the WEAK-scaling soup: n_per_tile triangles of its own (Philox(seed + 7919 (d + 1))) with centres uniform in cell d of
    domain_grid(n_tiles) -- every rank generates only what it owns.  The triangle size shrinks with the density (half_extent =
    0.005 n_tiles^(-1/3) unless given), so that the scene keeps config 3's extent-to-spacing ratio."""
    gx, gy, gz = domain_grid(n_tiles)
    he = F(0.005 * n_tiles ** (-1.0 / 3.0)) if half_extent is None else F(half_extent)
    rng = np.random.Generator(np.random.Philox(seed + 7919 * (d + 1)))
    ix, iy, iz = d % gx, (d // gx) % gy, d // (gx * gy)
    c = rng.random((n_per_tile, 1, 3), dtype=F) * np.array([1.0 / gx, 1.0 / gy, 1.0 / gz], F) + np.array([ix / gx, iy / gy, iz / gz], F)
    o = rng.random((n_per_tile, 3, 3), dtype=F)
    o *= F(2.0); o -= F(1.0); o *= he; o += c
    return o.reshape(-1, 3), np.arange(n_per_tile * 3, dtype=np.int32).reshape(-1, 3)


def soup_weak_scene(n_per_tile, n_tiles, width, height, own=None, boxes=None, seed=12345, half_extent=None):
    """Weak scaling of config 3: n_tiles domains of n_per_tile triangles EACH (camera and light of config 3, film as given).  own: the
    tiles whose geometry this process generates (None: all); boxes[d] = (lo, hi) of every tile it does not (a Domain-scheduler rank
    knows every instance's box but holds only its own meshes, DomainTracer.h:115-144) -- meshes[d] is None there."""
    own = list(range(n_tiles)) if own is None else list(own)
    meshes, lo, hi, mats = [None] * n_tiles, [None] * n_tiles, [None] * n_tiles, []
    for d in range(n_tiles):
        if d in own:
            v, t = soup_weak_tile(d, n_tiles, n_per_tile, seed, half_extent)
            meshes[d] = MeshData(v, t, default_material())
            lo[d], hi[d] = meshes[d].bbox()
        else:
            lo[d], hi[d] = np.asarray(boxes[d][0], F), np.asarray(boxes[d][1], F)
        mats.append(mat_translate_scale((0, 0, 0), (1, 1, 1)))
    minv, normi = zip(*[instance_matrices(m) for m in mats])
    cam = Camera((0.5, 0.5, 3.0), (0.5, 0.5, 0.5), (0.0, 1.0, 0.0), float(F(30.0 * np.pi / 180.0)), width, height, 1, 1, 0.0)
    return Scene(meshes, list(range(n_tiles)), np.array(mats, F).reshape(-1, 16), np.array(minv, F).reshape(-1, 16), np.array(normi, F).reshape(-1, 9),
                 np.array(lo, F).reshape(-1, 3), np.array(hi, F).reshape(-1, 3), np.ascontiguousarray(point_light((0.5, 0.5, 3.0)), LIGHT_DTYPE), cam,
                 "soup-weak-%dx%d" % (n_tiles, n_per_tile))


# ------------------------------------------------------------------ legacy .conf scenes (data/bunny.conf, data/README.conf)
def load_conf(path, geom_dirs=None, width=None, height=None):
    """Scene from one of the reference's legacy .conf files, as src/apps/render/ConfigFileLoader.cpp:70-285 reads them
    (that loader is compiled out in the reference, `#if 0` at :31, so its quirks are restated from the source):
      F w h                      film size                                         (:105-109)
      C eye(3) look(3) up(3) fov camera; the fov field is parsed but 45 degrees is stored ("TODO", :111-129)
      G file t(3) r(3) s(3)      one instance per line: translate, then scale; the rotation is computed into a temporary
                                 and never applied (:171-186); a mesh file is loaded once and shared (:139-166)
      LP pos(3) color(3)         point light (:225-238);  LA pos(3) normal(3) w h color(3)  area light (:240-262)
      ST DOMAIN | ...            scheduler hint, returned as scene.name suffix
    Mesh paths are resolved by base name in geom_dirs (default: tests/golden)."""
    geom_dirs = list(geom_dirs or [GOLDEN_DIR])
    meshes, mesh_index, inst_mesh, mats, lights = [], {}, [], [], []
    cam = None
    film = [512, 512]
    sched = "image"
    with open(path) as f:
        for line in f:
            if line.startswith("#"):
                continue
            e = line.split()
            if not e:
                continue
            if e[0] == "F" and len(e) >= 3:
                film = [int(e[1]), int(e[2])]
            elif e[0] == "C" and len(e) >= 11:
                v = [float(x) for x in e[1:10]]
                cam = (tuple(v[0:3]), tuple(v[3:6]), tuple(v[6:9]))
            elif e[0] == "G" and len(e) >= 11:
                base = os.path.basename(e[1])
                if base not in mesh_index:
                    found = None
                    for d in geom_dirs:
                        for cand in (os.path.join(d, base), os.path.join(d, os.path.splitext(base)[0] + ".npz")):
                            if os.path.exists(cand):
                                found = cand
                                break
                        if found:
                            break
                    if not found:
                        raise FileNotFoundError("%s: mesh %s not found in %s" % (path, e[1], geom_dirs))
                    v, t = load_mesh_file(found)
                    mesh_index[base] = len(meshes)
                    meshes.append(MeshData(v, t, default_material()))
                tr = [float(x) for x in e[2:5]]
                sc = [float(x) for x in e[8:11]]
                if not any(sc):
                    sc = [1.0, 1.0, 1.0]  # glm::length(t) > 0 guard (:188-192)
                mats.append(mat_translate_scale(tr, sc))
                inst_mesh.append(mesh_index[base])
            elif e[0] == "LP" and len(e) >= 7:
                lights.append(point_light([float(x) for x in e[1:4]], [float(x) for x in e[4:7]]))
            elif e[0] == "LA" and len(e) >= 12:
                from .layouts import area_light

                lights.append(area_light([float(x) for x in e[1:4]], [float(x) for x in e[9:12]], [float(x) for x in e[4:7]],
                                         float(e[7]), float(e[8])))
            elif e[0] == "ST" and len(e) >= 2 and e[1] in ("DOMAIN", "HYBRID"):
                sched = e[1].lower()
    if cam is None or not meshes:
        raise ValueError("%s: no camera or no geometry" % path)
    w, h = (width or film[0]), (height or film[1])
    camera = Camera(cam[0], cam[1], cam[2], float(F(45.0 * np.pi / 180.0)), w, h, 1, 1, 0.0)
    lights = np.concatenate(lights) if lights else np.zeros(0, LIGHT_DTYPE)
    return _assemble(meshes, inst_mesh, mats, np.ascontiguousarray(lights, LIGHT_DTYPE), camera,
                     "%s[%s]" % (os.path.basename(path), sched))


# ------------------------------------------------------------------ volumes (render/data/primitives/Volume.h; data/vol/*.bov)
@dataclass
class Subgrid:
    """One refined subgrid of an AMR volume (gvt_hip_subgrid; Volume::AddAMRGrid): it refines the cells [lo, lo + cells) of its parent --
    the level-0 grid (parent -1: lo is a GLOBAL cell index) or an EARLIER entry of the same list -- `ratio` (2, 4 or 8) times per axis.
    data[z, y, x]: cells * ratio + 1 vertices per axis, float32; vertex 0 sits on the parent's vertex lo."""

    parent: int
    ratio: int
    lo: np.ndarray  # (3,) i32, x y z
    cells: np.ndarray  # (3,) i32
    data: np.ndarray


@dataclass
class VolumeData:
    """A scalar grid: data[z, y, x] (x fastest, the BOV order), the position of vertex 0 and the vertex spacing.  subgrids: the refined
    subgrids of an AMR volume (a list of Subgrid; empty: a uniform grid)."""

    data: np.ndarray  # (nz, ny, nx); f32, or whatever the source held (uint8 / int16 / uint16 for HipVolumeAdapter(native=True))
    origin: np.ndarray = field(default_factory=lambda: np.zeros(3, F))
    spacing: np.ndarray = field(default_factory=lambda: np.ones(3, F))
    subgrids: list = field(default_factory=list)

    @property
    def counts(self):
        nz, ny, nx = self.data.shape
        return np.array([nx, ny, nz], np.int32)


@dataclass
class Brick:
    """One brick of a VolumeData (gvt_hip_volume_create's arguments): the vertices [offset, offset + counts) of the global grid, and the
    box they span in the volume's own space."""

    data: np.ndarray  # (counts[2], counts[1], counts[0]), the volume's dtype
    offset: np.ndarray  # (3,) i32, x y z
    global_counts: np.ndarray
    origin: np.ndarray  # the GLOBAL grid's vertex 0
    spacing: np.ndarray
    lo: np.ndarray
    hi: np.ndarray
    subgrids: list = field(default_factory=list)  # the AMR subgrids this brick holds (split_amr_volume); level-1 lo stays GLOBAL
    # the layers of global vertices just outside the six faces, -x +x -y +y -z +z (gvt_hip_volume_set_ghosts): +-x (nz, ny), +-y (nz, nx),
    # +-z (ny, nx); None for a face on the global boundary.  None: the brick does not know its neighbours
    ghosts: Optional[list] = None

    @property
    def counts(self):
        nz, ny, nx = self.data.shape
        return np.array([nx, ny, nz], np.int32)


_BOV_TYPES = {"FLOAT": "f4", "DOUBLE": "f8", "INT": "i4", "UCHAR": "u1", "BYTE": "u1", "SHORT": "i2", "CHAR": "i1"}


def read_bov(path, native=False):
    """A Brick-Of-Values file (data/vol/*.bov): the header's keys and the data as f32 (z, y, x); FLOAT, INT and UCHAR (and their kin) are read,
    non-float types converted on the host.  DATA_FILE is relative to the header.  native=True keeps UCHAR / BYTE as uint8 and SHORT as int16
    (in this machine's byte order, whatever the file's), for HipVolumeAdapter(native=True); every other format is f32 as before."""
    hdr = {}
    for line in open(path):
        if ":" in line:
            k, v = line.split(":", 1)
            hdr[k.strip().upper()] = v.strip()
    nx, ny, nz = (int(v) for v in hdr["DATA_SIZE"].split()[:3])
    fmt = hdr.get("DATA_FORMAT", "FLOAT").upper()
    if fmt not in _BOV_TYPES:
        raise ValueError("%s: unsupported DATA_FORMAT %s" % (path, fmt))
    endian = ">" if hdr.get("DATA_ENDIAN", "LITTLE").upper().startswith("B") else "<"
    dt = np.dtype(endian + _BOV_TYPES[fmt]) if _BOV_TYPES[fmt] != "u1" else np.dtype("u1")
    raw = os.path.join(os.path.dirname(os.path.abspath(path)), hdr["DATA_FILE"])
    a = np.fromfile(raw, dt, nx * ny * nz)
    if a.size != nx * ny * nz:
        raise ValueError("%s: %d values, the header promises %d" % (raw, a.size, nx * ny * nz))
    origin = np.array([float(v) for v in hdr.get("BRICK_ORIGIN", "0 0 0").split()[:3]], F)
    size = np.array([float(v) for v in hdr.get("BRICK_SIZE", "%d %d %d" % (nx - 1, ny - 1, nz - 1)).split()[:3]], F)
    spacing = (size / np.array([nx - 1, ny - 1, nz - 1], F)).astype(F)
    keep = native and _BOV_TYPES[fmt] in ("u1", "i2")
    a = a.astype(np.dtype(_BOV_TYPES[fmt]) if keep else F)  # (astype also brings a big-endian file into native order)
    return hdr, VolumeData(np.ascontiguousarray(a.reshape(nz, ny, nx)), origin, spacing)


def sphere_volume(n):
    """data/vol/sphere-like: a radial density on n^3 vertices, 1 at the centre falling linearly to 0 at half the width and beyond."""
    c = (n - 1) / 2.0
    x = (np.arange(n, dtype=np.float64) - c) / c
    r = np.sqrt(x[None, None, :] ** 2 + x[None, :, None] ** 2 + x[:, None, None] ** 2)
    return VolumeData(np.ascontiguousarray(np.clip(1.0 - r, 0.0, 1.0).astype(F)))


def noise_volume(n, seed=0, cell=8):
    """Smooth value noise on n^3 vertices in [0, 1]: random values on a coarse lattice (one per `cell` vertices) interpolated linearly, an
    axis at a time (slab by slab along z, so that 512^3 fits in a few GB)."""
    rng = np.random.default_rng(seed)
    m = (n - 1) // cell + 2
    coarse = rng.random((m, m, m), dtype=np.float32)
    pos = np.arange(n, dtype=np.float64) / cell
    i0 = np.minimum(pos.astype(np.int64), m - 2)
    w = (pos - i0).astype(F)
    a = coarse[:, :, i0] * (1 - w) + coarse[:, :, i0 + 1] * w        # (m, m, n)
    a = a[:, i0, :] * (1 - w)[None, :, None] + a[:, i0 + 1, :] * w[None, :, None]  # (m, n, n)
    out = np.empty((n, n, n), F)
    for z in range(n):
        out[z] = a[i0[z]] * (1 - w[z]) + a[i0[z] + 1] * w[z]
    return VolumeData(out)


def _cuts(n_vertices, parts):
    cells = n_vertices - 1
    if not 1 <= parts <= cells:
        raise ValueError("cannot cut %d cells into %d bricks" % (cells, parts))
    return [k * cells // parts for k in range(parts + 1)]


def brick_ghosts(data, off, end):
    """The six face layers beyond the vertices [off, end] (x y z, end inclusive) of the global grid data[z, y, x]: what a bricked
    simulation output carries as ghost data.  None where the face is on the grid's boundary."""
    nz, ny, nx = data.shape
    zs, ys, xs = slice(off[2], end[2] + 1), slice(off[1], end[1] + 1), slice(off[0], end[0] + 1)
    return [np.ascontiguousarray(data[zs, ys, off[0] - 1]) if off[0] > 0 else None,
            np.ascontiguousarray(data[zs, ys, end[0] + 1]) if end[0] + 1 < nx else None,
            np.ascontiguousarray(data[zs, off[1] - 1, xs]) if off[1] > 0 else None,
            np.ascontiguousarray(data[zs, end[1] + 1, xs]) if end[1] + 1 < ny else None,
            np.ascontiguousarray(data[off[2] - 1, ys, xs]) if off[2] > 0 else None,
            np.ascontiguousarray(data[end[2] + 1, ys, xs]) if end[2] + 1 < nz else None]


def split_volume(vol, bx, by, bz, ghosts=False):
    """Bricks of bx * by * bz: the cells cut evenly per axis, neighbours sharing one layer of vertices; every cell is owned by exactly one
    brick.  Order: x fastest.  Boxes in the volume's own space, computed as gvt_hip_volume_create computes them (f32).  ghosts=True:
    every brick also carries the six face layers beyond it (Brick.ghosts), for central-difference gradients."""
    cnt = vol.counts
    cx, cy, cz = _cuts(int(cnt[0]), bx), _cuts(int(cnt[1]), by), _cuts(int(cnt[2]), bz)
    org, sp = np.asarray(vol.origin, F), np.asarray(vol.spacing, F)
    out = []
    for k in range(bz):
        for j in range(by):
            for i in range(bx):
                off = np.array([cx[i], cy[j], cz[k]], np.int32)
                end = np.array([cx[i + 1], cy[j + 1], cz[k + 1]], np.int32)  # last vertex
                d = np.ascontiguousarray(vol.data[off[2]:end[2] + 1, off[1]:end[1] + 1, off[0]:end[0] + 1])
                lo = (org + off.astype(F) * sp).astype(F)
                hi = (org + end.astype(F) * sp).astype(F)
                out.append(Brick(d, off, cnt.copy(), org, sp, lo, hi))
                if ghosts:
                    out[-1].ghosts = brick_ghosts(vol.data, [int(v) for v in off], [int(v) for v in end])
    return out


def mesh_in_volume(scene, vol, fill=0.6):
    """Geometry inside a volume (scheduler.MixedTracer): `vol` placed so that its box is centred on the scene's instances and they take
    `fill` of its smallest side (the grid keeps its shape: the spacing is scaled uniformly).  Returns the VolumeData; the scene is unchanged."""
    lo, hi = np.asarray(scene.inst_lo, F).min(axis=0), np.asarray(scene.inst_hi, F).max(axis=0)
    cells = (vol.counts - 1).astype(np.float64)
    shape = cells * np.asarray(vol.spacing, np.float64)
    scale = float((hi - lo).max()) / (fill * float(shape.min()))
    spacing = (np.asarray(vol.spacing, np.float64) * scale).astype(F)
    origin = (0.5 * (lo.astype(np.float64) + hi) - 0.5 * cells * spacing).astype(F)
    return VolumeData(vol.data, origin, spacing)


def ao_directions(n):
    """The direction set of an ambient occlusion bake (gvt_hip_volume_ao_grid_bake): the n points of the Fibonacci sphere, i = arange(n) +
    0.5, z = 1 - 2 i / n, r = sqrt(1 - z^2), phi = i pi (3 - sqrt 5), computed in float64 and returned as float32 (n, 3).  The library
    normalises them again."""
    i = np.arange(int(n), dtype=np.float64) + 0.5
    z = 1.0 - 2.0 * i / float(n)
    r = np.sqrt(1.0 - z * z)
    phi = i * (np.pi * (3.0 - np.sqrt(5.0)))
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1).astype(F)


# ------------------------------------------------------------------ AMR volumes (Volume::AddAMRGrid; api::addAmrSubgrid; apps/render/AmrApp.cpp)
def subgrid_geometry(vol, index):
    """Origin (the position of vertex 0) and vertex spacing of subgrid `index` of vol (-1: the level-0 grid), in float64."""
    if index < 0:
        return np.asarray(vol.origin, np.float64), np.asarray(vol.spacing, np.float64)
    s = vol.subgrids[index]
    org, sp = subgrid_geometry(vol, s.parent)
    return org + np.asarray(s.lo, np.float64) * sp, sp / s.ratio


def _parent_cells(vol, parent):
    """The cells [lo, hi) a subgrid of `parent` may cover: the grid's own (for a brick: the global indices of the cells it owns)."""
    if parent < 0:
        off = np.asarray(getattr(vol, "offset", np.zeros(3)), np.int64)
        return off, off + np.asarray(vol.counts, np.int64) - 1
    p = vol.subgrids[parent]
    return np.zeros(3, np.int64), np.asarray(p.cells, np.int64) * p.ratio


def _prolong(data, lo, cells, ratio):
    """Trilinear prolongation: the grid `data` (z, y, x) sampled at the vertices of a subgrid that refines its cells [lo, lo + cells)."""
    out = np.asarray(data, np.float64)
    for axis, a in ((2, 0), (1, 1), (0, 2)):  # x, y, z
        pos = lo[a] + np.arange(cells[a] * ratio + 1, dtype=np.float64) / ratio
        i0 = np.minimum(pos.astype(np.int64), out.shape[axis] - 2)
        w = pos - i0
        shape = [1, 1, 1]
        shape[axis] = len(w)
        w = w.reshape(shape)
        out = np.take(out, i0, axis=axis) * (1 - w) + np.take(out, i0 + 1, axis=axis) * w
    return out


def refine(vol, lo, cells, ratio, parent=-1, fn=None, seed=0, detail=0.05):
    """Appends a Subgrid to vol.subgrids (vol: a VolumeData or a Brick) and returns its index (the `parent` of a child).  It refines
    the cells [lo, lo + cells) of `parent` (-1: the level-0 grid, lo a global cell index) `ratio` times.  fn(x, y, z): the field as a
    function of position in the volume's own space (arrays that broadcast to (nz, ny, nx)).  Without fn: the trilinear prolongation of
    the parent plus uniform detail noise of amplitude `detail` from `seed`.  ValueError for what gvt_hip_volume_set_subgrids refuses."""
    lo, cells = np.asarray(lo, np.int64).reshape(3), np.asarray(cells, np.int64).reshape(3)
    if ratio not in (2, 4, 8):
        raise ValueError("refine: ratio %r (2, 4 or 8)" % (ratio,))
    if not -1 <= parent < len(vol.subgrids):
        raise ValueError("refine: parent %d of %d subgrids" % (parent, len(vol.subgrids)))
    plo, phi = _parent_cells(vol, parent)
    if (cells < 1).any() or (lo < plo).any() or (lo + cells > phi).any():
        raise ValueError("refine: cells [%s, %s) leave the parent's [%s, %s)" % (lo.tolist(), (lo + cells).tolist(), plo.tolist(), phi.tolist()))
    for s in vol.subgrids:
        if s.parent == parent and ((lo < np.asarray(s.lo) + np.asarray(s.cells)) & (np.asarray(s.lo) < lo + cells)).all():
            raise ValueError("refine: the box overlaps another subgrid of parent %d" % parent)
    nv = cells * ratio + 1
    if fn is not None:
        org, sp = subgrid_geometry(vol, parent)
        p = [org[a] + (lo[a] + np.arange(nv[a], dtype=np.float64) / ratio) * sp[a] for a in range(3)]
        data = np.broadcast_to(np.asarray(fn(p[0][None, None, :], p[1][None, :, None], p[2][:, None, None]), np.float64), (nv[2], nv[1], nv[0]))
    else:
        src = vol.data if parent < 0 else vol.subgrids[parent].data
        rel = lo - (plo if parent < 0 else 0)  # the level-0 array starts at the brick's first vertex
        data = _prolong(src, rel, cells, ratio) + detail * (np.random.default_rng(seed).random((nv[2], nv[1], nv[0])) - 0.5)
    vol.subgrids.append(Subgrid(int(parent), int(ratio), lo.astype(np.int32), cells.astype(np.int32), np.ascontiguousarray(data, F)))
    return len(vol.subgrids) - 1


def subgrid_from_geometry(parent_origin, parent_spacing, origin, spacing, counts, tol=1e-4):
    """The reference's addAmrSubgrid(origin, spacing, counts) triple (counts: vertices per axis) against its parent grid's origin and
    spacing, as (ratio, lo, cells).  ValueError if the ratio is not 2, 4 or 8 on every axis, or the grid is not cell-aligned: vertex 0 on
    a parent vertex at or after the parent's first, and whole parent cells covered (tol: in units of a parent cell)."""
    po, ps = np.asarray(parent_origin, np.float64).reshape(3), np.asarray(parent_spacing, np.float64).reshape(3)
    o, sp, cnt = np.asarray(origin, np.float64).reshape(3), np.asarray(spacing, np.float64).reshape(3), np.asarray(counts, np.int64).reshape(3)
    r = ps / sp
    ratio = int(round(float(r[0])))
    if ratio not in (2, 4, 8) or (np.abs(r - ratio) > tol * ratio).any():
        raise ValueError("subgrid_from_geometry: spacing ratio %s is not 2, 4 or 8 on every axis" % r.tolist())
    g = (o - po) / ps
    lo = np.rint(g).astype(np.int64)
    if (np.abs(g - lo) > tol).any() or (lo < 0).any():
        raise ValueError("subgrid_from_geometry: vertex 0 at %s parent cells is not on a parent vertex" % g.tolist())
    if (cnt < ratio + 1).any() or ((cnt - 1) % ratio != 0).any():
        raise ValueError("subgrid_from_geometry: %s vertices at ratio %d do not cover whole parent cells" % (cnt.tolist(), ratio))
    return ratio, lo.astype(np.int32), ((cnt - 1) // ratio).astype(np.int32)


def split_amr_volume(vol, bx, by, bz, cuts=None):
    """split_volume, and every level-1 subgrid of vol -- with its descendants, re-indexed in the brick's own list -- handed to the brick
    that owns its cells.  ValueError if a level-1 subgrid straddles a cut (the caller cuts it, or chooses another bricking).
    cuts (optional): per axis the vertices the bricks begin and end at, ([0, ..., nx - 1], [0, ..., ny - 1], [0, ..., nz - 1]) with
    bx + 1, by + 1 and bz + 1 increasing entries, instead of split_volume's even cuts -- to keep the cuts clear of the subgrids."""
    if cuts is None:
        bricks = split_volume(vol, bx, by, bz)
    else:
        cnt = vol.counts
        for a, (c, parts) in enumerate(zip(cuts, (bx, by, bz))):
            c = [int(v) for v in c]
            if len(c) != parts + 1 or c[0] != 0 or c[-1] != int(cnt[a]) - 1 or any(q <= p for p, q in zip(c, c[1:])):
                raise ValueError("split_amr_volume: cuts %s of axis %d do not divide its %d cells into %d bricks" % (c, a, int(cnt[a]) - 1, parts))
        org, sp = np.asarray(vol.origin, F), np.asarray(vol.spacing, F)
        bricks = []
        for k in range(bz):
            for j in range(by):
                for i in range(bx):
                    off = np.array([cuts[0][i], cuts[1][j], cuts[2][k]], np.int32)
                    end = np.array([cuts[0][i + 1], cuts[1][j + 1], cuts[2][k + 1]], np.int32)  # last vertex
                    d = np.ascontiguousarray(vol.data[off[2]:end[2] + 1, off[1]:end[1] + 1, off[0]:end[0] + 1])
                    bricks.append(Brick(d, off, cnt.copy(), org, sp, (org + off.astype(F) * sp).astype(F), (org + end.astype(F) * sp).astype(F)))
    root = []  # per subgrid: its level-1 ancestor
    for i, s in enumerate(vol.subgrids):
        root.append(i if s.parent < 0 else root[s.parent])
    home = {}
    for i, s in enumerate(vol.subgrids):
        if s.parent >= 0:
            continue
        lo, hi = np.asarray(s.lo, np.int64), np.asarray(s.lo, np.int64) + np.asarray(s.cells, np.int64)
        for j, b in enumerate(bricks):
            if (lo >= b.offset).all() and (hi <= b.offset.astype(np.int64) + b.counts - 1).all():
                home[i] = j
                break
        else:
            raise ValueError("split_amr_volume: level-1 subgrid %d (cells %s to %s) straddles a cut of %d x %d x %d bricks" % (i, lo.tolist(), hi.tolist(), bx, by, bz))
    for j, b in enumerate(bricks):
        new = {}
        for i, s in enumerate(vol.subgrids):
            if home[root[i]] != j:
                continue
            new[i] = len(b.subgrids)
            b.subgrids.append(Subgrid(-1 if s.parent < 0 else new[s.parent], s.ratio, s.lo, s.cells, s.data))
    return bricks
