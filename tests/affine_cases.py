"""Instance matrices that are not diagonal, shared by the host and the GPU tests: seeded builders of the six families (column-major
float32 m[16], glm's layout, each with a translation in [-2, 2]^3), the float64 world-space brute-force triangle test that does not
depend on this project's matrix convention, and the inputs the tests of both sides build from them (a random mesh with rays aimed near
its triangles' centroids, a scene that mixes the families)."""
import numpy as np

from gravit_amd import scenes

F = np.float32
FAMILIES = ("rot", "rot_scale", "shear", "mirror", "perm", "diag")


def rotation(axis, angle):
    """Rodrigues' formula in float64: the 3x3 math matrix of the rotation about `axis` by `angle`."""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], np.float64)
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def to_m16(A, t):
    """The 3x3 math matrix A and the translation t as glm's column-major m[16], rounded to float32 once."""
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = A, t
    return np.ascontiguousarray(M.T, F).reshape(16)


def _random_rotation(rng):
    return rotation(rng.normal(size=3), rng.uniform(0.3, 2.8))


def linear_part(family, rng):
    if family == "rot":
        return _random_rotation(rng)
    if family == "rot_scale":
        return _random_rotation(rng) @ np.diag(rng.uniform(0.3, 3.0, 3))
    if family == "shear":
        S = np.eye(3)
        S[0, 1], S[0, 2], S[1, 2] = rng.uniform(-0.7, 0.7, 3)
        return _random_rotation(rng) @ S @ np.diag(rng.uniform(0.5, 2.0, 3))
    if family == "mirror":
        return _random_rotation(rng) @ np.diag([-1.3, 0.8, 2.0])
    if family == "perm":  # x -> 1.5 y, y -> 0.5 z, z -> -2 x (and its seeded kin): every entry exact
        p = rng.permutation(3)
        while (p == np.arange(3)).all():
            p = rng.permutation(3)
        A = np.zeros((3, 3))
        A[p, np.arange(3)] = rng.choice([0.5, 1.5, 2.0, 0.25], 3) * rng.choice([-1.0, 1.0], 3)
        return A
    if family == "diag":
        return np.diag(rng.uniform(0.3, 3.0, 3))
    raise KeyError(family)


def matrix(family, seed):
    """m[16] of `family` from `seed`.  perm: the translation is a multiple of 1/4, so that the products of a perm matrix are exact."""
    rng = np.random.default_rng([FAMILIES.index(family), seed])
    A = linear_part(family, rng)
    t = rng.uniform(-2, 2, 3)
    if family == "perm":
        t = np.round(t * 4) / 4
    return to_m16(A, t)


def perm_mirror(seed):
    """A perm matrix with a negative determinant (an odd number of sign flips is forced on it)."""
    m = matrix("perm", seed).reshape(4, 4).copy()
    if np.linalg.det(m[:3, :3].astype(np.float64)) > 0:
        m[0, :3] = -m[0, :3]
    return m.reshape(16)


def world_hits64(m, verts, tris, org, dirs, t_near=1e-6):
    """Closest hit of the rays org + t dirs (world space) with the triangles TRANSFORMED to world space by the float32 m, Moeller-Trumbore in
    float64 over all triangles: t per ray (inf: no hit).  m's entries are the inputs' float32 values; everything after is float64."""
    M = np.asarray(m, F).reshape(4, 4).T.astype(np.float64)
    w = np.asarray(verts, F).astype(np.float64) @ M[:3, :3].T + M[:3, 3]
    tri = w[np.asarray(tris)]
    v0, e1, e2 = tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    o, d = np.asarray(org, F).astype(np.float64), np.asarray(dirs, F).astype(np.float64)
    best = np.full(len(o), np.inf)
    with np.errstate(all="ignore"):
        for s in range(0, len(o), 256):
            oo, dd = o[s:s + 256, None, :], d[s:s + 256, None, :]
            pv = np.cross(dd, e2[None])
            det = (e1[None] * pv).sum(-1)
            inv = 1.0 / det
            tv = oo - v0[None]
            u = (tv * pv).sum(-1) * inv
            qv = np.cross(tv, e1[None])
            v = (dd * qv).sum(-1) * inv
            t = (e2[None] * qv).sum(-1) * inv
            ok = (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > t_near)
            best[s:s + 256] = np.where(ok, t, np.inf).min(axis=1)
    return best


def random_mesh(seed, n_v=400, n_t=900):
    rng = np.random.default_rng(31000 + seed)
    v = rng.normal(size=(n_v, 3)).astype(F)
    t = rng.integers(0, n_v, (n_t, 3)).astype(np.int32)
    t = t[(t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 0] != t[:, 2])]
    return v, np.ascontiguousarray(t)


def centroid_rays(m, verts, tris, n, seed, dist=4.0, spread=0.05):
    """n world-space rays aimed near the centroids of random triangles (as m places them) from `dist` units away."""
    rng = np.random.default_rng(32000 + seed)
    M = np.asarray(m, F).reshape(4, 4).T.astype(np.float64)
    c = verts[tris[rng.integers(0, len(tris), n)]].astype(np.float64).mean(axis=1) @ M[:3, :3].T + M[:3, 3]
    u = rng.normal(size=(n, 3))
    org = (c + dist * u / np.linalg.norm(u, axis=1, keepdims=True)).astype(F)
    d = c + rng.normal(size=(n, 3)) * spread - org
    return org, (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)


def check_against_world(t_got, t64):
    """The bounds of the float32 object-space result against world_hits64: (hit/miss disagreements, median relative error, share above 1e-4)."""
    hit = np.isfinite(t64)
    got_hit = t_got < np.float32(3e38)
    rel = np.abs(t_got[hit & got_hit].astype(np.float64) - t64[hit & got_hit]) / t64[hit & got_hit]
    return int((hit != got_hit).sum()), float(np.median(rel)) if len(rel) else 0.0, float((rel > 1e-4).sum()) / max(1, len(t64))


def mixed_scene(seed=0, n_inst=8, width=64, height=48):
    """Two small random meshes, n_inst instances that cycle through all six families, placed around the origin so that their boxes overlap
    along the view axis; two point lights; boxes from scenes.instance_bbox (all eight corners)."""
    from gravit_amd.layouts import default_material, point_light
    rng = np.random.default_rng(33000 + seed)
    meshes = []
    for k in range(2):
        v, t = random_mesh(seed * 2 + k, 120 + 80 * k, 300 + 300 * k)
        meshes.append(scenes.MeshData((v * F(0.35)).astype(F), t, default_material(kd=rng.uniform(0.2, 0.9, 3))))
    mats, inst_mesh = [], []
    for i in range(n_inst):
        fam = FAMILIES[i % len(FAMILIES)]
        A = linear_part(fam, np.random.default_rng([FAMILIES.index(fam), 500 + seed * 16 + i]))
        if fam != "perm":  # keep every instance on the film (perm stays exact)
            A = A / max(1.0, np.linalg.svd(A, compute_uv=False).max() / 1.5)
        mats.append(to_m16(A, np.round(rng.normal(size=3) * (0.9, 0.7, 0.9) * 4) / 4))
        inst_mesh.append(i % 2)
    lights = np.concatenate([point_light((0.8, 0.9, 7.0), (0.9, 0.8, 0.7)), point_light((-3.0, 1.0, 4.0), (0.4, 0.5, 0.6))])
    cam = scenes.Camera((0.3, 0.2, 7.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), float(np.radians(40.0)), width, height)
    return scenes._assemble(meshes, inst_mesh, mats, lights, cam, "affine-mixed-%d" % seed)


def spin(scene, frame, step=0.15):
    """The matrices of `scene` with every instance rotated by frame * step (a little more per instance) about an axis of its own through
    its own translation: m_i * R_i -- a rigid motion of the placed instance's object space."""
    out = []
    for i, m in enumerate(scene.m):
        M = np.asarray(m, F).reshape(4, 4).T.astype(np.float64)
        R = rotation(np.random.default_rng(34000 + i).normal(size=3), frame * step * (1 + 0.1 * i))
        out.append(to_m16(M[:3, :3] @ R, M[:3, 3]))
    return np.array(out, F)


def glm_rows(family):
    """The recorded glm vectors of a family (tests/golden/ref_matrix_vectors.json) as float32 arrays: per matrix a dict with m, inverse,
    normal_matrix, v (10, 3) and the recorded products point, vector, inv_point, inv_vector, mat3 (10, 3 each)."""
    import json
    import os

    f32 = lambda words: np.array(words, np.uint32).view(F)  # noqa: E731
    rows = json.load(open(os.path.join(scenes.GOLDEN_DIR, "ref_matrix_vectors.json")))[family]
    return [{k: (f32(r[k]) if k in ("m", "inverse", "normal_matrix") else np.array([f32(x) for x in r[k]])) for k in r} for r in rows]


def glm_ray_case(row):
    """Rays made of a fixture row's vectors -- every vector as an origin with every vector as a direction, 100 rays, the -0, zero, inf and NaN
    components among them -- for an instance whose m / minv / normi are glm's own triple (m, inverse(m), transpose(inverse(mat3(m)))).
    Returns (origins, directions, O, D): O / D = the object-space ray as glm computed it, minv * vec4(origin, 1) and minv * vec4(direction, 0)
    (the recorded inv_point / inv_vector)."""
    i, j = np.divmod(np.arange(100), 10)
    return row["v"][i], row["v"][j], row["inv_point"][i], row["inv_vector"][j]


def targets_mesh(O, D, seed=0):
    """A triangle across every finite object-space ray O + t D at t near 1 (a third of |D| wide), so that most finite rays hit."""
    rng = np.random.default_rng(35000 + seed)
    ok = np.isfinite(O).all(axis=1) & np.isfinite(D).all(axis=1) & (np.abs(D).max(axis=1) > 0)
    c = O[ok].astype(np.float64) + D[ok] * rng.uniform(0.7, 1.4, (int(ok.sum()), 1))
    size = np.linalg.norm(D[ok].astype(np.float64), axis=1)[:, None, None] * 0.3
    v = (c[:, None, :] + rng.normal(size=(len(c), 3, 3)) * size).reshape(-1, 3).astype(F)
    return v, np.arange(len(v), dtype=np.int32).reshape(-1, 3)
