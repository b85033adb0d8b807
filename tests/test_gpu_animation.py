"""Animated scenes: gvt_hip_mesh_update_vertices (the LBVH refitted in place), gvt_hip_top_update and gvt_hip_tracer_set_transforms, and
NativeTracer.update_scene on top of them.  The queries do not depend on the tree, so a refitted mesh must give the hits of a mesh created
from the new vertices bit for bit -- checked against the oracle and against a fresh build; a refit of unchanged vertices must give the
build's own bytes back."""
import os

import numpy as np
import pytest
import torch  # (before the library initialises the device, as in test_gpu_domain.py)

from gravit_amd import capi, scenes
from gravit_amd.adapter import HipMeshAdapter, TopLevel
from gravit_amd.layouts import NORMALS_FLAT, NORMALS_SMOOTH, point_light
from gravit_amd.scheduler import Comm, Context, NativeTracer
from oracle import orc
from tests.conftest import GOLDEN
from tests.helpers import bits, oracle_camera_rays, oracle_render, rays_equal_bits, seeded_rays_at, sort_rays

pytestmark = pytest.mark.gpu

F = np.float32
REF = [10, 11, 12, 13]  # child reference columns of a 4-wide node
BOX = [i for i in range(16) if i not in REF]


def load_mesh(name):
    if name == "bunny":
        return scenes.bunny_scene(64, 64).meshes[0]
    if name == "bun_zipper":
        z = np.load(os.path.join(GOLDEN, "bun_zipper.npz"))
        return scenes.MeshData(np.ascontiguousarray(z["verts"], F), np.ascontiguousarray(z["tris"], np.int32))
    if name == "soup":
        v, t = scenes.triangle_soup(200_000, seed=11)
        return scenes.MeshData(np.ascontiguousarray(v, F), np.ascontiguousarray(t, np.int32))
    if name == "tri":
        return scenes.MeshData(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], F), np.array([[0, 1, 2]], np.int32))
    if name == "two":  # <= leaf_max triangles: the single-node tree (k_single_node)
        return scenes.MeshData(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0.5]], F), np.array([[0, 1, 2], [1, 3, 2]], np.int32))
    raise KeyError(name)


def deform(v, kind, seed=5):
    rng = np.random.default_rng(seed)
    v = np.asarray(v, F)
    lo, hi = v.min(0), v.max(0)
    ext = float((hi - lo).max())
    if kind == "smooth":
        c = (v - lo) / max(ext, 1e-30)
        d = np.stack([np.sin(6.0 * c[:, 1]), np.cos(5.0 * c[:, 2]), np.sin(4.0 * c[:, 0] + 1.0)], 1)
        return (v + 0.05 * ext * d).astype(F)
    if kind == "jitter":
        return (v + rng.normal(scale=0.01 * ext, size=v.shape)).astype(F)
    if kind == "scale":
        return (v * F(10.0) + np.array([3.0, -2.0, 1.0], F)).astype(F)
    if kind == "permute":  # every vertex somewhere else: every box overlaps every other
        return np.ascontiguousarray(v[rng.permutation(len(v))])
    raise KeyError(kind)


def assert_hits_equal(g, c):
    assert (g["prim"] == c["prim"]).all(), "%d primIDs differ" % (g["prim"] != c["prim"]).sum()
    for f in ("t", "u", "v"):
        assert (bits(g[f]) == bits(c[f])).all(), "%s differs in %d rays" % (f, (bits(g[f]) != bits(c[f])).sum())


def snapshot(ad):
    w, s = ad.download_wide()
    c, root = ad.download_clusters()
    return {"nodes": ad.download_nodes(), "wide": w, "slots": s, "clusters": c, "root": root, "normals": ad.normals(), "info": ad.info()}


def assert_same_bytes(a, b):
    for k in ("nodes", "wide", "slots", "clusters", "normals"):
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, k
            continue
        assert a[k].shape == b[k].shape and np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), "%s differ" % k
    assert a["root"] == b["root"]
    for k in ("bbox_lo", "bbox_hi", "sah_inner", "packet", "n_nodes", "n_leaves"):
        assert np.array_equal(np.asarray(a["info"][k], F).view(np.uint32), np.asarray(b["info"][k], F).view(np.uint32)), k


def one_mesh_scene(mesh, w=96, h=96):
    lo, hi = mesh.bbox()
    c = 0.5 * (np.asarray(lo, np.float64) + np.asarray(hi, np.float64))
    ext = float(np.max(np.asarray(hi, np.float64) - np.asarray(lo, np.float64)))
    cam = scenes.Camera(tuple(c + [0.3 * ext, 0.4 * ext, 1.8 * ext]), tuple(c), (0.0, 1.0, 0.0), float(F(45.0 * np.pi / 180.0)), w, h, 1, 1, 0.0)
    light = point_light(tuple(c + [ext, 1.5 * ext, ext]))
    return scenes._assemble([mesh], [0], [np.eye(4, dtype=F).reshape(16)], light, cam, "anim")


# ------------------------------------------------------------------ a refit of unchanged vertices is a no-op
@pytest.mark.parametrize("name", ["bunny", "bun_zipper", "soup", "tri", "two"])
def test_refit_of_unchanged_vertices_gives_the_build_back(hip, name):
    mesh = load_mesh(name)
    ad = HipMeshAdapter(mesh)
    before = snapshot(ad)
    ms = ad.update_vertices(mesh.verts)
    assert ms >= 0.0
    assert_same_bytes(before, snapshot(ad))
    ad.update_vertices(deform(mesh.verts, "jitter"))  # a round trip
    ad.update_vertices(mesh.verts)
    assert_same_bytes(before, snapshot(ad))


def test_empty_mesh_updates(hip):
    mesh = scenes.MeshData(np.zeros((3, 3), F), np.zeros((0, 3), np.int32))
    ad = HipMeshAdapter(mesh)
    ad.update_vertices(np.ones((3, 3), F))
    i = ad.info()
    assert i["n_tris"] == 0 and i["n_nodes"] == 0
    assert np.isnan(ad.normals()).all()  # no faces: 0 * (1 / sqrt(0)), as at create


# ------------------------------------------------------------------ hit parity after a refit
@pytest.mark.parametrize("kind", ["smooth", "jitter", "scale", "permute"])
@pytest.mark.parametrize("name", ["bunny", "bun_zipper", "soup", "two"])
def test_refit_hits_equal_oracle_and_a_fresh_build(hip, name, kind):
    mesh = load_mesh(name)
    ad = HipMeshAdapter(mesh)
    ad.download_clusters()  # the cluster layout exists: it is refitted too
    nv = deform(mesh.verts, kind)
    ad.update_vertices(nv)
    new = scenes.MeshData(nv, mesh.tris)
    fresh = HipMeshAdapter(new)
    om = orc.Mesh(nv, mesh.tris)
    lo, hi = om.bbox()
    heavy = kind == "permute"  # every ray meets most of the triangles: the oracle's share is kept small
    org, d = seeded_rays_at(lo, hi, 1009 if heavy else 20011, 3)
    g, c = ad.intersect(org, d), om.intersect(org, d)
    assert_hits_equal(g, c)
    assert_hits_equal(g, fresh.intersect(org, d))
    occ = ad.occluded(org, d)
    assert (occ == om.occluded(org, d)).all() and (occ == fresh.occluded(org, d)).all()
    if name != "two":
        assert (g["prim"] >= 0).sum() > 50
    i, f = ad.info(), fresh.info()
    assert np.array_equal(np.asarray(i["bbox_lo"], F), np.asarray(f["bbox_lo"], F)) and np.array_equal(np.asarray(i["bbox_hi"], F), np.asarray(f["bbox_hi"], F))
    assert np.array_equal(ad.normals().view(np.uint32), fresh.normals().view(np.uint32))
    # whole adapter calls in both normal modes (shading reads the slots and the regenerated normals)
    sc = one_mesh_scene(new, *((32, 32) if heavy else (96, 96)))
    rays = oracle_camera_rays(sc)
    for mode in (NORMALS_FLAT, NORMALS_SMOOTH):
        ad.normal_mode = mode
        rg, rc = rays.copy(), rays.copy()
        og = ad.trace(rg, sc.m[0], sc.minv[0], sc.normi[0], sc.lights)
        oc = om.trace(rc, sc.m[0], sc.minv[0], sc.normi[0], sc.lights, mode)
        assert rays_equal_bits(sort_rays(og), sort_rays(oc)) and rays_equal_bits(rg, rc)


@pytest.mark.parametrize("opts", [dict(sort_rays=1), dict(long_steps=2, long_min_rays=0), dict(long_steps=0), dict(term_sink=0),
                                  dict(leaf_max=1), dict(leaf_max=4, long_steps=4, long_min_rays=0), dict(leaf_max=3)])
def test_refit_results_do_not_depend_on_tuning_knobs(hip, opts):
    sc = scenes.soup_scene(150_000, 160, 90)
    mesh = sc.meshes[0]
    try:
        for k, v in opts.items():
            hip.set_option(k, v)
        ad = HipMeshAdapter(mesh)
        bunny = load_mesh("bunny")
        ab = HipMeshAdapter(bunny)
        for kind, a, m in (("smooth", ad, mesh), ("jitter", ad, mesh), ("permute", ab, bunny)):
            nv = deform(m.verts, kind, seed=21)
            a.update_vertices(nv)
            new = scenes.MeshData(nv, m.tris, m.material)
            om = orc.Mesh(nv, m.tris, mesh_mat=m.material)
            lo, hi = om.bbox()
            heavy = kind == "permute"
            org, d = seeded_rays_at(lo, hi, 1009 if heavy else 30_001, 21)
            assert_hits_equal(a.intersect(org, d), om.intersect(org, d))
            assert (a.occluded(org, d) == om.occluded(org, d)).all()
            sc2 = one_mesh_scene(new, *((32, 32) if heavy else (160, 90)))
            rays = oracle_camera_rays(sc2)
            rg, rc = rays.copy(), rays.copy()
            og = a.trace(rg, sc2.m[0], sc2.minv[0], sc2.normi[0], sc2.lights)
            oc = om.trace(rc, sc2.m[0], sc2.minv[0], sc2.normi[0], sc2.lights, 0)
            assert rays_equal_bits(sort_rays(og), sort_rays(oc)) and rays_equal_bits(rg, rc)
    finally:
        hip.set_option("defaults", 0)


# ------------------------------------------------------------------ layout invariants after a refit
def slot_boxes(slots):
    v0 = slots[:, 0:3].astype(np.float64)
    v1 = slots[:, [7, 11, 12]].astype(np.float64)
    v2 = slots[:, 13:16].astype(np.float64)
    return np.minimum(np.minimum(v0, v1), v2), np.maximum(np.maximum(v0, v1), v2)


def leaf_range(ref):
    code = ~int(ref) & 0xFFFFFFFF
    return code >> 3, (code >> 3) + (code & 7)


@pytest.mark.parametrize("name", ["bunny", "soup"])
def test_refit_layout_invariants(hip, name):
    mesh = load_mesh(name)
    ad = HipMeshAdapter(mesh)
    c_before, root_before = ad.download_clusters()
    ad.update_vertices(deform(mesh.verts, "permute"))
    s = snapshot(ad)
    nodes, w, slots, c = s["nodes"], s["wide"], s["slots"], s["clusters"]
    tlo, thi = slot_boxes(slots)
    # binary nodes: every subtree covers a contiguous slot range (child 0 before child 1), and every child box contains its triangles
    refs = nodes[:, 12:14].view(np.int32)
    rng2 = {}

    def sub(r):
        return leaf_range(r) if r < 0 else rng2[int(r)]
    order = [0]
    k = 0
    while k < len(order):  # breadth first, then the ranges bottom-up
        for r in refs[order[k]]:
            if r >= 0:
                order.append(int(r))
        k += 1
    assert len(order) == len(nodes) and len(set(order)) == len(nodes)
    for i in reversed(order):
        a, b = sub(refs[i][0]), sub(refs[i][1])
        assert a[1] == b[0] or refs[i][1] == -1
        rng2[i] = (a[0], b[1] if refs[i][1] != -1 else a[1])
        for side, (f, e) in ((0, a), (1, b)):
            if e <= f:
                continue
            lo = nodes[i, [0 + 4 * side, 2 + 4 * side, 8 + 2 * side]].astype(np.float64)
            hi = nodes[i, [1 + 4 * side, 3 + 4 * side, 9 + 2 * side]].astype(np.float64)
            assert (lo <= tlo[f:e].min(0)).all() and (hi >= thi[f:e].max(0)).all()
    assert rng2[0] == (0, len(slots))
    # 4-wide nodes: every child box, decoded, contains its triangles
    wr = w[:, REF].view(np.int32)
    origin = w[:, 0:3].view(np.float32).astype(np.float64)
    step = w[:, [3, 14, 15]].view(np.float32).astype(np.float64)
    r4 = {}
    for i in range(len(w) - 1, -1, -1):  # breadth-first array: children after their parent
        used = [r for r in wr[i] if r != -1]
        rs = [leaf_range(r) if r < 0 else r4[int(r)] for r in used]
        srt = sorted(rs)  # (the slots are not in range order: k_collapse4 appends the right half of an expanded child)
        for a, b in zip(srt, srt[1:]):
            assert a[1] == b[0]
        r4[i] = (srt[0][0], srt[-1][1])
        for sl, (f, e) in enumerate(rs):
            ql = np.array([(int(w[i, 4 + 2 * a]) >> (8 * sl)) & 255 for a in range(3)], np.float64)
            qh = np.array([(int(w[i, 5 + 2 * a]) >> (8 * sl)) & 255 for a in range(3)], np.float64)
            assert (origin[i] + ql * step[i] <= tlo[f:e].min(0)).all() and (origin[i] + qh * step[i] >= thi[f:e].max(0)).all()
    assert r4[0] == (0, len(slots))
    # the cluster layout: the same permutation as before the refit (references unchanged) and the same node boxes as nodes4
    assert c is not None and s["root"] == root_before
    assert np.array_equal(c[:, REF], c_before[:, REF])
    key = lambda a: a[np.lexsort(a[:, BOX].T[::-1])][:, BOX]  # noqa: E731
    assert np.array_equal(key(c), key(w))


# ------------------------------------------------------------------ normals
def assert_normals_equal(a, b):
    """bit for bit; a NaN (a vertex without faces, a degenerate face) only has to be a NaN at the same place"""
    na, nb = np.isnan(a), np.isnan(b)
    assert np.array_equal(na, nb)
    assert np.array_equal(np.where(na, 0, a).view(np.uint32), np.where(nb, 0, b).view(np.uint32))


@pytest.mark.parametrize("name", ["bunny", "bun_zipper"])
def test_regenerated_normals_equal_the_host_generation(hip, name):
    mesh = load_mesh(name)
    counts = np.bincount(mesh.tris.reshape(-1), minlength=len(mesh.verts))
    assert counts.max() >= 6  # vertices shared by many faces: the order of the sum matters
    ad = HipMeshAdapter(mesh)
    for kind in ("smooth", "jitter", "permute"):
        nv = deform(mesh.verts, kind)
        ad.update_vertices(nv)
        assert_normals_equal(ad.normals(), orc.generate_normals(nv, mesh.tris))
    # normals the caller supplies are used as given
    given = np.random.default_rng(3).normal(size=mesh.verts.shape).astype(F)
    ad.update_vertices(nv, given)
    assert np.array_equal(ad.normals().view(np.uint32), given.view(np.uint32))


def test_device_pointer_path_equals_host_path(hip):
    """The same mesh updated from host arrays and from device tensors (one mesh: the 4-wide array's order is fixed at its build)."""
    mesh = load_mesh("bun_zipper")
    a = HipMeshAdapter(mesh)
    nv = deform(mesh.verts, "smooth")
    given = np.random.default_rng(4).normal(size=nv.shape).astype(F)
    for nrm in (None, given):
        a.update_vertices(nv, nrm)
        host = snapshot(a)
        a.update_vertices(deform(mesh.verts, "jitter"))
        a.update_vertices(torch.from_numpy(nv).cuda(), None if nrm is None else torch.from_numpy(nrm).cuda())
        assert_same_bytes(host, snapshot(a))


# ------------------------------------------------------------------ errors leave the mesh usable
def test_update_errors_leave_the_mesh_usable(hip):
    import ctypes as C

    mesh = load_mesh("bunny")
    ad = HipMeshAdapter(mesh)
    lib = capi.load()
    v = np.ascontiguousarray(deform(mesh.verts, "jitter"))
    n = len(v)
    assert lib.gvt_hip_mesh_update_vertices(ad.h, capi.ptr(v), C.c_size_t(n - 1), None, C.c_uint32(0), None) == -1  # wrong nV
    assert "vertices" in capi.last_error()
    assert lib.gvt_hip_mesh_update_vertices(ad.h, None, C.c_size_t(n), None, C.c_uint32(0), None) == -1  # null vertices
    assert lib.gvt_hip_mesh_update_vertices(None, capi.ptr(v), C.c_size_t(n), None, C.c_uint32(0), None) == -1  # null mesh
    assert lib.gvt_hip_mesh_update_vertices(ad.h, capi.ptr(v), C.c_size_t(n), None, C.c_uint32(6), None) == -1  # unknown flags
    with pytest.raises(capi.GvtHipError):
        ad.update_vertices(v[:-1])
    sc = scenes.bunny_grid_scene(width=64, height=36)
    top = TopLevel(sc.inst_lo, sc.inst_hi)
    with pytest.raises(capi.GvtHipError):
        top.update(sc.inst_lo[:-1], sc.inst_hi[:-1])
    assert lib.gvt_hip_top_update(top.h, None, capi.ptr(sc.inst_hi), C.c_size_t(sc.n_inst)) == -1
    om = orc.Mesh(mesh.verts, mesh.tris)
    lo, hi = om.bbox()
    org, d = seeded_rays_at(lo, hi, 4096, 7)
    assert_hits_equal(ad.intersect(org, d), om.intersect(org, d))  # the mesh is untouched
    assert np.array_equal(top.order(), TopLevel(sc.inst_lo, sc.inst_hi).order())
    tr = NativeTracer(sc, NORMALS_SMOOTH)
    with pytest.raises(capi.GvtHipError):
        tr.set_transforms(sc.m[:-1], sc.minv[:-1], sc.normi[:-1])
    fb = tr().framebuffer(True)
    ref, _ = oracle_render(sc, NORMALS_SMOOTH)
    assert np.array_equal(fb[..., :3], ref[..., :3])
    tr.close()


# ------------------------------------------------------------------ whole frames through one tracer
def animate(base, frame, kinds=("smooth",), move=0.0, seed=0):
    """Frame `frame` of an animation of `base`: every mesh deformed (kinds cycle over the frames), every instance translated a little."""
    kind = kinds[frame % len(kinds)]
    meshes = []
    for k, m in enumerate(base.meshes):
        nv = m.verts if frame == 0 else deform(m.verts, kind, seed=seed + 97 * frame + k)
        if kind == "smooth" and frame:
            nv = (m.verts + (nv - m.verts) * F(0.25 * frame)).astype(F)
        meshes.append(scenes.MeshData(np.ascontiguousarray(nv, F), m.tris, m.material, None, m.vcolors, m.materials, m.face_mat))
    mats = []
    for i in range(base.n_inst):
        t = np.eye(4, dtype=F)
        t[:3, 3] = move * frame * np.array([np.sin(i + frame), 0.5 * np.cos(2 * i + frame), 0.0], F)
        mats.append((t @ base.m[i].reshape(4, 4).T).T.reshape(16).astype(F))
    return scenes._assemble(meshes, base.inst_mesh, mats, base.lights, base.camera, "%s-f%d" % (base.name, frame))


def render_animation(base, mode, n_frames, **kw):
    tr = NativeTracer(base, mode)
    out = []
    for f in range(n_frames):
        sc = animate(base, f, **kw)
        if f:
            tr.update_scene(sc)
        out.append((sc, tr().framebuffer(True).copy()))
    tr.close()
    return out


def test_bunny_grid_animation_equals_the_oracle_every_frame(hip):
    base = scenes.bunny_grid_scene(width=380, height=216)
    for sc, fb in render_animation(base, NORMALS_SMOOTH, 8, kinds=("smooth", "jitter"), move=0.01):
        ref, _ = oracle_render(sc, NORMALS_SMOOTH)
        assert (ref[..., :3].sum(axis=2) > 0).sum() > 500
        assert np.array_equal(fb[..., :3], ref[..., :3]), sc.name


def test_cathedral_animation_equals_the_oracle_every_frame(hip):
    base = scenes.cathedral_scene(128, 128, samples=2, depth=2)
    for sc, fb in render_animation(base, NORMALS_FLAT, 8, kinds=("smooth",), move=0.0):
        ref, _ = oracle_render(sc, NORMALS_FLAT)
        assert np.abs(fb[..., :3] - ref[..., :3]).max() <= 1e-5, sc.name
        assert np.array_equal(fb[..., 3], ref[..., 3])


def test_soup_domains_animation_equals_the_oracle_every_frame(hip):
    """The soup cut into domains; one frame permutes every tile's vertices (boxes that overlap everything): its small rounds go through k_finish."""
    base = scenes.soup_domains_scene(40_000, 4, 160, 90)
    for sc, fb in render_animation(base, NORMALS_FLAT, 8, kinds=("smooth", "jitter", "scale", "permute"), move=0.002):
        ref, _ = oracle_render(sc, NORMALS_FLAT)
        assert np.array_equal(fb[..., :3], ref[..., :3]), sc.name


@pytest.mark.parametrize("world", [2, 4])
def test_animation_on_several_ranks_equals_one_rank(hip, world):
    import threading

    base = scenes.bunny_grid_scene(width=380, height=216)
    n_frames = 4
    frames = [animate(base, f, kinds=("smooth", "jitter"), move=0.01) for f in range(n_frames)]
    one = [fb for _, fb in render_animation(base, NORMALS_SMOOTH, n_frames, kinds=("smooth", "jitter"), move=0.01)]
    owner = [i % world for i in range(base.n_inst)]
    hub = capi.load().gvt_hip_hub_create(world)
    out, errs = {}, []

    def rank_main(rank):
        ctx = None
        try:
            ctx = Context(0)
            comm = Comm.local(hub, rank)
            tr = NativeTracer(frames[0], NORMALS_SMOOTH, owner, comm)
            fbs = []
            for f, sc in enumerate(frames):
                if f:
                    tr.update_scene(sc)
                B = tr()
                fbs.append(B.framebuffer(True).copy() if rank == 0 else None)
            out[rank] = fbs
            tr.close()
            comm.close()
        except Exception:  # noqa: BLE001
            import traceback
            errs.append(traceback.format_exc())
            capi.load().gvt_hip_hub_abort(hub)
        finally:
            import gc
            gc.collect()
            if ctx is not None:
                ctx.close()

    th = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
    [t.start() for t in th]
    [t.join(timeout=600) for t in th]
    capi.load().gvt_hip_hub_destroy(hub)
    assert not errs, errs[0]
    for f in range(n_frames):
        assert np.array_equal(out[0][f][..., :3], one[f][..., :3]), "frame %d" % f


# ------------------------------------------------------------------ time (reported)
def test_refit_time_on_the_10m_soup(hip):
    v, t = scenes.triangle_soup(10_000_000)
    v = np.ascontiguousarray(v, F)
    t = np.ascontiguousarray(t, np.int32)
    nrm = np.zeros_like(v)
    nrm[:, 2] = 1.0
    ad = HipMeshAdapter(scenes.MeshData(v, t, vnormals=nrm))
    build_ms = ad.info()["build_ms"]
    nv = deform(v, "jitter")
    ad.update_vertices(nv, nrm)  # first update: the range tables are derived
    first_ms = ad.update_vertices(deform(v, "smooth"), nrm)
    ms = min(ad.update_vertices(deform(v, "jitter", seed=k), nrm) for k in range(3))
    regen_first = ad.update_vertices(nv)
    regen = ad.update_vertices(nv)
    ad.update_vertices(deform(v, "permute"), nrm)
    i = ad.info()
    print("\n[refit] 10 M soup: build %.3f ms, refit %.3f ms (first refit after the tables: %.3f), with normal regeneration %.3f ms (first %.3f), "
          "sah_inner %.1f after permuting the vertices (packet %d)" % (build_ms, ms, first_ms, regen, regen_first, i["sah_inner"], i["packet"]))
    assert ms < build_ms
