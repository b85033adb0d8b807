"""Host-side mirror of GraviT's engine-adapter interface for the gfx950 adapter.

  gvt::render::Adapter                      src/gvt/render/Adapter.h:44-88
  gvt::render::adapter::embree::data::EmbreeMeshAdapter   adapter/embree/EmbreeMeshAdapter.{h,cpp}

`HipMeshAdapter` has the reference's shape: constructed from a Mesh, one `trace()` with the reference's
arguments (rayList, m, minv, normi, lights, begin, end) and the reference's output contract (moved
rays = misses + un-occluded shadow rays, rayList updated in place).  Everything runs in
libgvt_hip.so; a missing library or device raises (no CPU path).
"""
import ctypes as C

import numpy as np

from . import capi
from .layouts import HIT_DTYPE, LIGHT_DTYPE, MATERIAL_DTYPE, NORMALS_FLAT, RAY_DTYPE


class RayQueue:
    """Device-resident gvt::render::actor::RayVector (actor/Ray.h:189)."""

    def __init__(self, capacity=0):
        self.lib = capi.load()
        self.h = C.c_void_p(self.lib.gvt_hip_queue_create(C.c_size_t(capacity)))
        if not self.h:
            raise capi.GvtHipError("gvt_hip_queue_create: " + capi.last_error())

    def close(self):
        if getattr(self, "h", None):
            self.lib.gvt_hip_queue_destroy(self.h)
            self.h = None

    __del__ = close

    def __len__(self):
        n = C.c_size_t(0)
        capi.check(self.lib.gvt_hip_queue_size(self.h, C.byref(n)), "gvt_hip_queue_size")
        return n.value

    def clear(self):
        capi.check(self.lib.gvt_hip_queue_clear(self.h), "gvt_hip_queue_clear")

    def reserve(self, n):
        capi.check(self.lib.gvt_hip_queue_reserve(self.h, C.c_size_t(n)), "gvt_hip_queue_reserve")

    def append(self, rays, keep_state=False):
        """host rays; keep_state: they are rays this library exported (bytes 64..79 = stream word + known misses), else they start fresh"""
        rays = np.ascontiguousarray(rays, dtype=RAY_DTYPE)
        capi.check(self.lib.gvt_hip_queue_append_flags(self.h, capi.ptr(rays), C.c_size_t(len(rays)), C.c_int(2 if keep_state else 0)), "gvt_hip_queue_append_flags")

    def append_device(self, dptr, n, keep_state=True):
        """n 80-byte rays at device address dptr (a received wire buffer: the rays keep their state)."""
        capi.check(self.lib.gvt_hip_queue_append_flags(self.h, C.c_void_p(dptr), C.c_size_t(n), C.c_int(1 | (2 if keep_state else 0))), "gvt_hip_queue_append_flags")

    def export_device(self, dptr, cap):
        n = C.c_size_t(0)
        capi.check(self.lib.gvt_hip_queue_export(self.h, C.c_void_p(dptr), C.c_size_t(cap), C.byref(n), C.c_int(1)), "gvt_hip_queue_export")
        return n.value

    def to_numpy(self):
        n = len(self)
        out = np.zeros(n, RAY_DTYPE)
        got = C.c_size_t(0)
        capi.check(self.lib.gvt_hip_queue_export(self.h, capi.ptr(out), C.c_size_t(n), C.byref(got), C.c_int(0)), "gvt_hip_queue_export")
        return out


def queues_export_wire(queues, dptr, cap):
    """gvt_hip_queues_export_wire: the rays of `queues` (RayQueue), in that order, as 80-byte wire rays at device address dptr (room
    for cap rays), in one launch; the queues are cleared.  Returns the rays per queue.  Too small a capacity raises and changes nothing."""
    n = len(queues)
    arr = (C.c_void_p * max(1, n))(*[q.h for q in queues])
    counts = (C.c_uint64 * max(1, n))()
    total = C.c_uint64(0)
    capi.check(capi.load().gvt_hip_queues_export_wire(arr, n, C.c_void_p(dptr), cap, counts, C.byref(total)), "gvt_hip_queues_export_wire")
    return [int(c) for c in counts[:n]]


def queues_append_wire(queues, dptr, counts):
    """gvt_hip_queues_append_wire: consecutive runs of counts[i] wire rays at device address dptr appended to queues[i], their state
    kept, in one launch."""
    n = len(queues)
    arr = (C.c_void_p * max(1, n))(*[q.h for q in queues])
    cnt = (C.c_uint64 * max(1, n))(*[int(c) for c in counts])
    capi.check(capi.load().gvt_hip_queues_append_wire(arr, n, C.c_void_p(dptr), cnt), "gvt_hip_queues_append_wire")


class HipMeshAdapter:
    """gvt::render::adapter::hip::data::HipMeshAdapter -- drop-in for EmbreeMeshAdapter.

    normal_mode: NORMALS_FLAT is the current EmbreeMeshAdapter.cpp (FLAT_SHADING, :75); NORMALS_SMOOTH is
    what the reference's golden images, EmbreeStreamMeshAdapter and the OptiX adapter use.
    """

    def __init__(self, mesh, normal_mode=NORMALS_FLAT):
        self.lib = capi.load()
        self.normal_mode = int(normal_mode)
        self.verts = capi.f32(mesh.verts, (-1, 3))
        self.tris = np.ascontiguousarray(mesh.tris, dtype=np.int32).reshape(-1, 3)
        vn = None if mesh.vnormals is None else capi.f32(mesh.vnormals, (-1, 3))
        vc = None if mesh.vcolors is None else capi.f32(mesh.vcolors, (-1, 3))
        mats = None if mesh.materials is None else np.ascontiguousarray(mesh.materials, dtype=MATERIAL_DTYPE)
        fm = None if mesh.face_mat is None else np.ascontiguousarray(mesh.face_mat, dtype=np.int32)
        mm = None if mesh.material is None else np.ascontiguousarray(mesh.material, dtype=MATERIAL_DTYPE)
        self.h = C.c_void_p(self.lib.gvt_hip_mesh_create(
            capi.ptr(self.verts), C.c_size_t(len(self.verts)), capi.ptr(self.tris), C.c_size_t(len(self.tris)), capi.ptr(vn),
            capi.ptr(vc), capi.ptr(mats), C.c_size_t(0 if mats is None else len(mats)), capi.ptr(fm), capi.ptr(mm)))
        if not self.h:
            raise capi.GvtHipError("gvt_hip_mesh_create: " + capi.last_error())

    def close(self):
        if getattr(self, "h", None):
            self.lib.gvt_hip_mesh_destroy(self.h)
            self.h = None

    __del__ = close

    def info(self):
        i = capi.MeshInfo()
        capi.check(self.lib.gvt_hip_mesh_get_info(self.h, C.byref(i)), "gvt_hip_mesh_get_info")
        return {"n_tris": i.n_tris, "n_verts": i.n_verts, "n_nodes": i.n_nodes, "n_leaves": i.n_leaves, "bbox_lo": list(i.bbox_lo),
                "bbox_hi": list(i.bbox_hi), "build_ms": i.build_ms, "max_leaf": i.max_leaf, "bytes_nodes": i.bytes_nodes, "bytes_tris": i.bytes_tris,
                "packet": int(i.packet), "sah_inner": float(i.sah_inner)}

    def update_vertices(self, verts, normals=None):
        """gvt_hip_mesh_update_vertices: new positions for the same triangles, the tree refitted in place (every pointer a tracer borrowed
        stays valid).  verts / normals: (nV, 3) float32 -- numpy on the host, or torch tensors on this mesh's GPU (no host round trip).
        normals=None: regenerated as at create.  Returns the device time of the update in ms."""
        ms = C.c_float(0.0)
        if hasattr(verts, "data_ptr"):  # a torch tensor: the device path
            if not verts.is_cuda or (normals is not None and not normals.is_cuda):
                raise ValueError("update_vertices: torch tensors must be on the GPU (pass numpy arrays for host data)")
            import torch

            v = verts.detach().to(torch.float32).contiguous().reshape(-1, 3)
            nrm = None if normals is None else normals.detach().to(torch.float32).contiguous().reshape(-1, 3)
            torch.cuda.current_stream(v.device).synchronize()  # (the tensors are written on torch's stream, the update runs on the library's)
            rc = self.lib.gvt_hip_mesh_update_vertices(self.h, C.c_void_p(v.data_ptr()), C.c_size_t(v.shape[0]),
                                                       None if nrm is None else C.c_void_p(nrm.data_ptr()), C.c_uint32(1), C.byref(ms))
            capi.check(rc, "gvt_hip_mesh_update_vertices")
            self.verts = v.cpu().numpy()
        else:
            v = capi.f32(verts, (-1, 3))
            nrm = None if normals is None else capi.f32(normals, (-1, 3))
            capi.check(self.lib.gvt_hip_mesh_update_vertices(self.h, capi.ptr(v), C.c_size_t(len(v)), capi.ptr(nrm), C.c_uint32(0), C.byref(ms)),
                       "gvt_hip_mesh_update_vertices")
            self.verts = v
        return float(ms.value)

    def normals(self):
        out = np.zeros((len(self.verts), 3), np.float32)
        capi.check(self.lib.gvt_hip_mesh_get_normals(self.h, capi.ptr(out)), "gvt_hip_mesh_get_normals")
        return out

    # -- Adapter::trace (Adapter.h:82-84) ------------------------------------------------------------
    def trace(self, rayList, m, minv, normi, lights, begin=0, end=0, seed=0, write_back=True, out=None):
        """Traces rayList[begin:end) (end==0 -> all, EmbreeMeshAdapter.cpp:642).  rayList (RAY_DTYPE, C-contiguous)
        is updated in place (write_back=False: only read, GVT_HIP_TRACE_NO_WRITEBACK); returns moved_rays (misses + un-occluded
        shadow rays, order unspecified), a view of `out` when the caller brings its own buffer (like a re-used RayVector)."""
        if rayList.dtype != RAY_DTYPE or not rayList.flags.c_contiguous:
            raise ValueError("rayList must be a C-contiguous array of RAY_DTYPE (80-byte gvt Ray)")
        lights = np.ascontiguousarray(lights, dtype=LIGHT_DTYPE)
        n = len(rayList)
        e = n if end == 0 else end
        cap = max(16, (e - begin) * (1 + len(lights)))
        if out is None:
            out = np.zeros(cap, RAY_DTYPE)
        elif out.dtype != RAY_DTYPE or not out.flags.c_contiguous:
            raise ValueError("out must be a C-contiguous array of RAY_DTYPE")
        cap = len(out)
        n_out = C.c_size_t(0)
        capi.check(self.lib.gvt_hip_trace_ex(
            self.h, capi.ptr(rayList), C.c_size_t(n), C.c_size_t(begin), C.c_size_t(end), capi.ptr(out), C.c_size_t(cap),
            C.byref(n_out), capi.ptr(capi.f32(m, 16)), capi.ptr(capi.f32(minv, 16)), capi.ptr(capi.f32(normi, 9)), capi.ptr(lights),
            C.c_size_t(len(lights)), C.c_int(self.normal_mode), C.c_uint32(seed), C.c_uint32(0 if write_back else 1)), "gvt_hip_trace_ex")
        return out[: n_out.value]

    def trace_queue(self, q_in, q_out, m, minv, normi, lights, seed=0, sink=None):
        """Adapter::trace on device-resident queues: q_in is consumed, moved rays are appended to q_out.  sink=(top, from_inst, fb):
        un-occluded shadow rays that meet no other instance deposit into fb inside the adapter (gvt_hip_trace_queue_sink)."""
        lights = np.ascontiguousarray(lights, dtype=LIGHT_DTYPE)
        top, from_inst, fb = sink if sink is not None else (None, -1, None)
        capi.check(self.lib.gvt_hip_trace_queue_sink(
            self.h, q_in.h, q_out.h, capi.ptr(capi.f32(m, 16)), capi.ptr(capi.f32(minv, 16)), capi.ptr(capi.f32(normi, 9)),
            capi.ptr(lights), C.c_size_t(len(lights)), C.c_int(self.normal_mode), C.c_uint32(seed),
            top.h if top is not None else None, C.c_int(from_inst), fb.h if fb is not None else None), "gvt_hip_trace_queue_sink")

    # -- the two Embree queries underneath (EmbreeMeshAdapter.cpp:474,375) -------------------------------
    def intersect(self, org, dirs, tnear=1e-6):
        org = capi.f32(org, (-1, 3))
        dirs = capi.f32(dirs, (-1, 3))
        out = np.zeros(len(org), HIT_DTYPE)
        capi.check(self.lib.gvt_hip_intersect(self.h, capi.ptr(org), capi.ptr(dirs), C.c_size_t(len(org)), C.c_float(tnear), capi.ptr(out)),
                   "gvt_hip_intersect")
        return out

    def wide_visit_stats(self, org, dirs, width, tnear=1e-6):
        """Diagnostic: nodes a `width`-wide collapse of the tree would make each ray visit (mean), and the collapse's node count."""
        org = capi.f32(org, (-1, 3))
        dirs = capi.f32(dirs, (-1, 3))
        cnt = np.zeros(len(org), np.uint32)
        nw = C.c_uint64(0)
        capi.check(self.lib.gvt_hip_wide_visit_stats(self.h, capi.ptr(org), capi.ptr(dirs), C.c_size_t(len(org)), C.c_float(tnear), C.c_int(width),
                                                     capi.ptr(cnt), C.byref(nw)), "gvt_hip_wide_visit_stats")
        return {"width": width, "nodes_per_ray": float(cnt.mean()), "p99": float(np.percentile(cnt, 99)), "max": int(cnt.max()), "wide_nodes": int(nw.value)}

    def download_nodes(self):
        """Diagnostic: the binary LBVH as built, (n_nodes, 16) float32 rows (gvt_hip.h gvt_hip_mesh_download_nodes; child refs bit-cast in columns 12, 13)."""
        n = self.info()["n_nodes"]
        out = np.zeros((n, 16), np.float32)
        capi.check(self.lib.gvt_hip_mesh_download_nodes(self.h, capi.ptr(out), C.c_size_t(n)), "gvt_hip_mesh_download_nodes")
        return out

    def download_wide(self):
        """Measurement: the traversal layout -- (n4, 16) uint32 compressed 4-wide nodes and (n_tris, 16) float32 triangle slots in leaf order."""
        i = self.info()
        n4 = i["bytes_nodes"] // 64 - i["n_nodes"]
        nodes4 = np.zeros((n4, 16), np.uint32)
        slots = np.zeros((i["n_tris"], 16), np.float32)
        capi.check(self.lib.gvt_hip_mesh_download_wide(self.h, capi.ptr(nodes4), C.c_size_t(n4), capi.ptr(slots), C.c_size_t(i["n_tris"])), "gvt_hip_mesh_download_wide")
        return nodes4, slots

    def download_clusters(self):
        """Measurement: the cluster layout of the 4-wide nodes (built on first use) -- (n4, 16) uint32 and the root's entry, or (None, -1) when the mesh has none."""
        i = self.info()
        n4 = i["bytes_nodes"] // 64 - i["n_nodes"]
        out = np.zeros((n4, 16), np.uint32)
        root = C.c_int32(-1)
        capi.check(self.lib.gvt_hip_mesh_download_clusters(self.h, capi.ptr(out), C.c_size_t(n4), C.byref(root)), "gvt_hip_mesh_download_clusters")
        return (out, root.value) if root.value >= 0 else (None, -1)

    def upload_nodes(self, nodes):
        """Diagnostic: replace the binary nodes (visit-count diagnostics only) by a tree over the same leaves."""
        nodes = np.ascontiguousarray(nodes, np.float32)
        capi.check(self.lib.gvt_hip_mesh_upload_nodes(self.h, capi.ptr(nodes), C.c_size_t(len(nodes))), "gvt_hip_mesh_upload_nodes")

    def marked_visit_stats(self, org, dirs, marks, tnear=1e-6):
        """Diagnostic: per ray, the marked binary nodes (roots of the wide nodes of a collapse the caller chose) its closest-hit traversal visits."""
        org = capi.f32(org, (-1, 3))
        dirs = capi.f32(dirs, (-1, 3))
        marks = np.ascontiguousarray(marks, np.uint8)
        cnt = np.zeros(len(org), np.uint32)
        capi.check(self.lib.gvt_hip_marked_visit_stats(self.h, capi.ptr(org), capi.ptr(dirs), C.c_size_t(len(org)), C.c_float(tnear), capi.ptr(marks), capi.ptr(cnt)),
                   "gvt_hip_marked_visit_stats")
        return cnt

    def visit_stats(self, org, dirs, tnear=1e-6):
        """Diagnostic: per-ray (inner-node visits, leaf visits, triangle tests) of the closest-hit traversal, plus the
        number of steps a 64-lane wave executes per batch (the slowest lane's inner + leaf steps)."""
        org = capi.f32(org, (-1, 3))
        dirs = capi.f32(dirs, (-1, 3))
        n = len(org)
        cnt = np.zeros((n, 3), np.uint32)
        capi.check(self.lib.gvt_hip_visit_stats(self.h, capi.ptr(org), capi.ptr(dirs), C.c_size_t(n), C.c_float(tnear), capi.ptr(cnt)),
                   "gvt_hip_visit_stats")
        steps = (cnt[:, 0] + cnt[:, 1]).astype(np.int64)
        pad = (-n) % 64
        waves = np.concatenate([steps, np.zeros(pad, np.int64)]).reshape(-1, 64)
        return {"inner_per_ray": float(cnt[:, 0].mean()), "leaf_per_ray": float(cnt[:, 1].mean()), "tri_tests_per_ray": float(cnt[:, 2].mean()),
                "lane_steps_per_ray": float(steps.mean()), "wave_steps_per_batch": float(waves.max(axis=1).mean()),
                "simd_efficiency": float(steps.sum() / max(1, waves.max(axis=1).sum() * 64)), "counts": cnt}

    def occluded(self, org, dirs, tnear=1e-6):
        org = capi.f32(org, (-1, 3))
        dirs = capi.f32(dirs, (-1, 3))
        out = np.zeros(len(org), np.int32)
        capi.check(self.lib.gvt_hip_occluded(self.h, capi.ptr(org), capi.ptr(dirs), C.c_size_t(len(org)), C.c_float(tnear), capi.ptr(out)),
                   "gvt_hip_occluded")
        return out


class TopLevel:
    """Top-level instance set: gvt::render::data::accel::BVH (accel/BVH.h) + shuffleRays (TracerBase.h:325-414)."""

    def __init__(self, inst_lo, inst_hi):
        self.lib = capi.load()
        self.lo = capi.f32(inst_lo, (-1, 3))
        self.hi = capi.f32(inst_hi, (-1, 3))
        self.n = len(self.lo)
        self.h = C.c_void_p(self.lib.gvt_hip_top_create(capi.ptr(self.lo), capi.ptr(self.hi), C.c_size_t(self.n)))
        if not self.h:
            raise capi.GvtHipError("gvt_hip_top_create: " + capi.last_error())

    def close(self):
        if getattr(self, "h", None):
            self.lib.gvt_hip_top_destroy(self.h)
            self.h = None

    __del__ = close

    def update(self, inst_lo, inst_hi):
        """gvt_hip_top_update: new instance boxes for the same set (the order and the top BVH rebuilt in place)."""
        lo = capi.f32(inst_lo, (-1, 3))
        hi = capi.f32(inst_hi, (-1, 3))
        capi.check(self.lib.gvt_hip_top_update(self.h, capi.ptr(lo), capi.ptr(hi), C.c_size_t(len(lo))), "gvt_hip_top_update")
        self.lo, self.hi = lo, hi

    def order(self):
        out = np.zeros(self.n, np.int32)
        capi.check(self.lib.gvt_hip_top_order(self.h, capi.ptr(out)), "gvt_hip_top_order")
        return out

    def shuffle(self, q_in, from_inst, queues, fb, keep_mask=None):
        arr = (C.c_void_p * max(1, self.n))(*[q.h for q in queues])
        km = None if keep_mask is None else np.ascontiguousarray(keep_mask, dtype=np.uint8)
        capi.check(self.lib.gvt_hip_shuffle(self.h, q_in.h, C.c_int(from_inst), arr, capi.ptr(km), fb.h if fb is not None else None),
                   "gvt_hip_shuffle")


class FrameBuffer:
    """Float RGBA framebuffer: gvt::render::composite::IceTComposite (composite/IceTComposite.cpp:79-157)."""

    def __init__(self, width, height):
        self.lib = capi.load()
        self.w, self.hgt = width, height
        self.h = C.c_void_p(self.lib.gvt_hip_fb_create(C.c_int(width), C.c_int(height)))
        if not self.h:
            raise capi.GvtHipError("gvt_hip_fb_create: " + capi.last_error())

    def close(self):
        if getattr(self, "h", None):
            self.lib.gvt_hip_fb_destroy(self.h)
            self.h = None

    __del__ = close

    def clear(self):
        capi.check(self.lib.gvt_hip_fb_clear(self.h), "gvt_hip_fb_clear")

    def device_ptr(self):
        return self.lib.gvt_hip_fb_device_ptr(self.h)

    def download(self, clamp=True):
        out = np.zeros((self.hgt, self.w, 4), np.float32)
        capi.check(self.lib.gvt_hip_fb_download(self.h, capi.ptr(out), C.c_int(int(clamp))), "gvt_hip_fb_download")
        return out

    def composite_over(self, back, depth=None):
        """gvt_hip_fb_composite_over: this (a volume frame) over `back` (a mesh frame), in place; coverage from the DepthPlane `depth`, or
        from back's alpha without one."""
        capi.check(self.lib.gvt_hip_fb_composite_over(self.h, back.h, depth.h if depth is not None else None), "gvt_hip_fb_composite_over")
        return self

    def ppm_bytes(self):
        out = np.zeros((self.hgt, self.w, 3), np.uint8)
        capi.check(self.lib.gvt_hip_fb_write_ppm_bytes(self.h, capi.ptr(out)), "gvt_hip_fb_write_ppm_bytes")
        return out


def camera_pod(cam):
    """The gvt_hip_camera record of a scenes.Camera."""
    return capi.CameraPod((C.c_float * 3)(*cam.eye), (C.c_float * 3)(*cam.focus), (C.c_float * 3)(*cam.up), cam.fov, cam.width, cam.height,
                          cam.samples, cam.depth, cam.jitter)


class DepthPlane:
    """gvt_hip_depth: W*H floats on the device, t along every pixel's camera ray (+Inf: nothing there) -- what the mesh side hands to a
    clipped volume frame (VolumeTracer.frame(depth=...)) and to FrameBuffer.composite_over."""

    def __init__(self, width, height):
        self.lib = capi.load()
        self.w, self.hgt = int(width), int(height)
        self._backend = None
        self.h = C.c_void_p(self.lib.gvt_hip_depth_create(self.w, self.hgt))
        if not self.h:
            raise capi.GvtHipError("gvt_hip_depth_create: " + capi.last_error())

    def close(self):
        if getattr(self, "h", None):
            self.lib.gvt_hip_depth_destroy(self.h)
            self.h = None

    __del__ = close

    def clear(self):
        capi.check(self.lib.gvt_hip_depth_clear(self.h), "gvt_hip_depth_clear")
        return self

    def upload(self, t):
        """t: (H, W) float32 -- a numpy array, or a contiguous torch tensor on the GPU (no host round trip)."""
        if hasattr(t, "data_ptr") and t.is_cuda:
            import torch

            if not t.is_contiguous() or t.dtype != torch.float32 or t.numel() != self.w * self.hgt:
                raise ValueError("DepthPlane.upload: a device tensor must be contiguous float32 of %d x %d" % (self.hgt, self.w))
            torch.cuda.current_stream(t.device).synchronize()  # (the tensor is written on torch's stream, the copy runs on the library's)
            capi.check(self.lib.gvt_hip_depth_upload(self.h, C.c_void_p(t.data_ptr()), 1), "gvt_hip_depth_upload")
            return self
        t = capi.f32(t.numpy() if hasattr(t, "data_ptr") else t)
        if t.size != self.w * self.hgt:
            raise ValueError("DepthPlane.upload: %d values for a %d x %d plane" % (t.size, self.hgt, self.w))
        capi.check(self.lib.gvt_hip_depth_upload(self.h, capi.ptr(t), 0), "gvt_hip_depth_upload")
        return self

    def download(self):
        out = np.zeros((self.hgt, self.w), np.float32)
        capi.check(self.lib.gvt_hip_depth_download(self.h, capi.ptr(out)), "gvt_hip_depth_download")
        return out

    def render(self, scene_or_backend, cam=None):
        """gvt_hip_depth_render: the nearest hit of every camera ray over all instances.  A scheduler.HipBackend brings its scene and its
        mesh adapters; for a scenes.Scene the adapters are made here and kept for the next call with the same scene.  cam: the scene's."""
        scene, adapters, self._backend = scene_instances(scene_or_backend, self._backend)
        cam = cam or scene.camera
        pod = camera_pod(cam)
        meshes = (C.c_void_p * max(1, scene.n_inst))(*[a.h for a in adapters])
        m, minv = capi.f32(scene.m), capi.f32(scene.minv)
        capi.check(self.lib.gvt_hip_depth_render(self.h, meshes, capi.ptr(m), capi.ptr(minv), scene.n_inst, C.byref(pod)), "gvt_hip_depth_render")
        return self


def scene_instances(scene_or_backend, kept=None):
    """(scene, the mesh adapter of every instance, what to keep) of a scheduler.HipBackend, which brings its scene and its adapters, or
    of a scenes.Scene, whose adapters are made here; kept: the third result of the last call, so that the same scene's are used again."""
    B = scene_or_backend
    if hasattr(B, "adapter_cache"):
        return B.scene, [B.adapter(i) for i in range(B.scene.n_inst)], kept
    if kept is None or kept[0] is not B:
        kept = (B, {mi: HipMeshAdapter(B.meshes[mi]) for mi in sorted(set(B.inst_mesh))})
    return B, [kept[1][mi] for mi in B.inst_mesh], kept


def camera_generate(q, cam, tile=0):
    """gvtPerspectiveCamera::generateRays into a device queue; tile=8 lists the same rays in 8x8-pixel tiles."""
    capi.check(capi.load().gvt_hip_camera_generate_tiled(
        q.h, capi.ptr(capi.f32(cam.eye, 3)), capi.ptr(capi.f32(cam.focus, 3)), capi.ptr(capi.f32(cam.up, 3)), C.c_float(cam.fov),
        C.c_int(cam.width), C.c_int(cam.height), C.c_int(cam.samples), C.c_int(cam.depth), C.c_float(cam.jitter), C.c_int(tile)),
        "gvt_hip_camera_generate_tiled")


class TransferFunction:
    """gvt::render::data::primitives::TransferFunction (TransferFunction.{h,cpp}): colour rows (x r g b), opacity rows (x a) and the value
    range that maps onto them.  The 256-entry resampling and the opacity correction happen in the library (gvt_hip_volume_set_transfer)."""

    def __init__(self, cmap, omap, value_range=(0.0, 1.0)):
        self.cmap = capi.f32(cmap, (-1, 4))
        self.omap = capi.f32(omap, (-1, 2))
        self.value_range = (float(value_range[0]), float(value_range[1]))

    @staticmethod
    def read_map(path, width):
        """GraviT's .cmap / .omap format (TransferFunction::load, :91-115): a count, then that many rows of `width` numbers."""
        tok = open(path).read().split()
        if not tok:
            raise ValueError("%s: empty map" % path)
        n = int(tok[0])
        if n < 0 or len(tok) < 1 + n * width:
            raise ValueError("%s: %d rows of %d promised, %d numbers present" % (path, n, width, len(tok) - 1))
        return np.array([float(v) for v in tok[1:1 + n * width]], np.float32).reshape(n, width)

    @classmethod
    def from_files(cls, cmap_path, omap_path, value_range=(0.0, 1.0)):
        return cls(cls.read_map(cmap_path, 4), cls.read_map(omap_path, 2), value_range)


def subgrid_tree(subgrids):
    """The tree of a list of scenes.Subgrid without its data: (parent, ratio, lo, cells) per entry, plain ints.  Needs no device."""
    return [(int(s.parent), int(s.ratio), tuple(int(v) for v in s.lo), tuple(int(v) for v in s.cells)) for s in (subgrids or [])]


def same_subgrid_tree(tree, subgrids, what="subgrids"):
    """ValueError unless `subgrids` (scenes.Subgrid) have the tree `tree` (subgrid_tree's form): the same count and per entry the same
    parent, ratio, lo and cells -- what gvt_hip_volume_update_amr takes for granted.  Needs no device."""
    other = subgrid_tree(subgrids)
    if len(other) != len(tree):
        raise ValueError("%s: %d subgrids given, the brick has %d (another tree is set_subgrids)" % (what, len(other), len(tree)))
    for i, (a, b) in enumerate(zip(tree, other)):
        for name, x, y in zip(("parent", "ratio", "lo", "cells"), a, b):
            if x != y:
                raise ValueError("%s: entry %d has %s %s, the brick's has %s (another tree is set_subgrids)" % (what, i, name, y, x))


class HipVolumeAdapter:
    """A volume brick on the device (gvt_hip_volume): the counterpart of the reference's volume adapters (OSPRayAdapter, PVolAdapter).
    `brick` is a scenes.Brick (or a scenes.VolumeData: the whole grid as one brick); its data may also be a torch tensor on the GPU.
    A brick that carries `subgrids` (scenes.refine, scenes.split_amr_volume) is an AMR volume: they are set at construction (set_subgrids).
    amr_shaded: the subgrids are set with capi.VOLUME_AMR_SHADED, so the AMR brick takes set_surfaces and set_shading (isovalues, slice
    planes and lit fog in the refined cells); without it (the default) both are refused on a brick that has subgrids.
    native=False: the data is converted to float32, whatever it was.  native=True: a uint8, int16 or uint16 brick (numpy array or contiguous
    GPU tensor) is stored at its own width (gvt_hip_volume_create_typed: a vertex's value is (float)v, so transfer functions and isovalues
    are in the data's units) and answers bit for bit like the float32 brick of the converted data; any other dtype raises ValueError.
    .voxel_type / .sample_bytes: what the library holds (capi.VOXEL_*, bytes per sample on the device)."""

    @staticmethod
    def dtype_of(data):
        """The dtype's name, for numpy arrays and torch tensors alike."""
        return str(data.dtype).replace("torch.", "")

    def __init__(self, brick, sampling_rate=1.0, skip=True, native=False, amr_shaded=False):
        self.lib = capi.load()
        self.amr_shaded = bool(amr_shaded)
        self.tree = []  # subgrid_tree of the current set (set_subgrids)
        if hasattr(brick, "global_counts"):
            counts, offset, gcounts = brick.counts, brick.offset, brick.global_counts
        else:
            counts = brick.counts
            offset, gcounts = np.zeros(3, np.int32), counts
        data = brick.data
        flags = 0 if skip else capi.VOLUME_NO_SKIP
        if hasattr(data, "data_ptr") and not data.is_cuda:  # a torch tensor in host memory
            data = data.numpy()
        self.dtype_name = self.dtype_of(data) if native else "float32"
        if native and self.dtype_name not in ("uint8", "int16", "uint16"):
            raise ValueError("HipVolumeAdapter: native=True stores uint8, int16 and uint16 data, not %s (convert it, or pass native=False)" % self.dtype_name)
        if hasattr(data, "data_ptr"):  # a torch tensor on the device
            if not data.is_contiguous() or self.dtype_of(data) != self.dtype_name:
                raise ValueError("HipVolumeAdapter: a device tensor must be contiguous %s" % ("float32" if not native else "uint8, int16 or uint16"))
            self._data = data
            src = C.c_void_p(data.data_ptr())
            flags |= capi.VOLUME_DEVICE
        else:
            self._data = np.ascontiguousarray(data, dtype=np.dtype(self.dtype_name))  # (native byte order; float32 unless native)
            src = capi.ptr(self._data)
        self.counts = np.ascontiguousarray(counts, np.int32)
        self.offset = np.ascontiguousarray(offset, np.int32)
        self.global_counts = np.ascontiguousarray(gcounts, np.int32)
        self.origin = capi.f32(brick.origin, 3)
        self.spacing = capi.f32(brick.spacing, 3)
        self.sampling_rate = float(sampling_rate)
        self.h = C.c_void_p(self.lib.gvt_hip_volume_create_typed(src, capi.VOXEL_TYPES[self.dtype_name], capi.ptr(self.counts), capi.ptr(self.origin),
                                                                 capi.ptr(self.spacing), capi.ptr(self.offset), capi.ptr(self.global_counts),
                                                                 self.sampling_rate, flags))
        if not self.h:
            raise capi.GvtHipError("gvt_hip_volume_create_typed: " + capi.last_error())
        vt, nb = C.c_int(-1), C.c_size_t(0)
        capi.check(self.lib.gvt_hip_volume_get_voxel_type(self.h, C.byref(vt), C.byref(nb)), "gvt_hip_volume_get_voxel_type")
        self.voxel_type, self.sample_bytes = vt.value, nb.value
        if getattr(brick, "subgrids", None):  # an AMR brick: its subgrids come with it
            self.set_subgrids(brick.subgrids)
        if getattr(brick, "ghosts", None) is not None:  # a brick that knows its neighbours' face layers (scenes.split_volume(ghosts=True))
            self.set_ghosts(brick.ghosts)

    def set_subgrids(self, subgrids, shaded=None):
        """gvt_hip_volume_set_subgrids: the brick's whole set of refined subgrids (scenes.Subgrid; an empty list removes it).  Their data:
        numpy arrays, or contiguous float32 torch tensors on the GPU (all of them: no host round trip).  The library keeps its own copies.
        shaded: pass capi.VOLUME_AMR_SHADED (None: the adapter's amr_shaded) -- the call is then accepted on a brick that has surfaces or
        gradient shading, and the set takes both."""
        subgrids = list(subgrids)
        n = len(subgrids)
        pods = (capi.SubgridPod * max(n, 1))()
        ptrs = (C.c_void_p * max(n, 1))()
        keep, device = [], [hasattr(s.data, "data_ptr") and s.data.is_cuda for s in subgrids]
        if any(device) and not all(device):
            raise ValueError("set_subgrids: the subgrids' data must be all host arrays or all GPU tensors")
        for i, s in enumerate(subgrids):
            pods[i] = capi.SubgridPod(int(s.parent), int(s.ratio), (C.c_int32 * 3)(*[int(v) for v in s.lo]), (C.c_int32 * 3)(*[int(v) for v in s.cells]))
            shape = tuple(int(c) * int(s.ratio) + 1 for c in list(s.cells)[::-1])
            if tuple(s.data.shape) != shape:
                raise ValueError("set_subgrids: subgrid %d has data of shape %s, its cells and ratio need %s" % (i, tuple(s.data.shape), shape))
            if device[i]:
                import torch

                if not s.data.is_contiguous() or self.dtype_of(s.data) != "float32":
                    raise ValueError("set_subgrids: a device tensor must be contiguous float32")
                torch.cuda.current_stream(s.data.device).synchronize()  # (written on torch's stream, copied on the library's)
                keep.append(s.data)
                ptrs[i] = s.data.data_ptr()
            else:
                keep.append(np.ascontiguousarray(s.data.numpy() if hasattr(s.data, "data_ptr") else s.data, np.float32))
                ptrs[i] = keep[-1].ctypes.data
        flags = capi.VOLUME_DEVICE if n and all(device) else 0
        if self.amr_shaded if shaded is None else shaded:
            flags |= capi.VOLUME_AMR_SHADED
        capi.check(self.lib.gvt_hip_volume_set_subgrids(self.h, C.cast(pods, C.c_void_p), C.cast(ptrs, C.c_void_p), n, flags), "gvt_hip_volume_set_subgrids")
        self.tree = subgrid_tree(subgrids)  # what update_amr and VolumeTracer.update(amr=True) compare a new step's subgrids with

    def update_amr(self, data=None, subgrids=None):
        """gvt_hip_volume_update_amr: the next time step of an AMR brick on the same subgrid tree, in place (every pointer a tracer borrowed
        stays valid; transfer function, surfaces, lights and the occluder grid are kept, the light grid goes stale).  data: the level-0
        samples, shape (nz, ny, nx), or None to keep them.  subgrids: None to keep them all, or a list as long as the brick's set whose
        entries are scenes.Subgrid (its tree fields must be the stored ones), an array of that subgrid's shape, or None to keep that
        subgrid.  Everything given is a numpy array, or everything a contiguous float32 torch tensor on the GPU (no host round trip).
        ValueError for a shape or tree that is not the stored one, before anything changes.  Returns the device time of the update in ms."""
        tree = getattr(self, "tree", [])
        if not tree:
            raise ValueError("update_amr: the brick has no subgrids (update_samples is its call)")
        given = []  # (what, array) of everything that is not None, level 0 first
        if data is not None:
            shape = tuple(int(c) for c in self.counts[::-1])
            if tuple(data.shape) != shape:
                raise ValueError("update_amr: data of shape %s, the brick has %s" % (tuple(data.shape), shape))
            given.append(("data", data))
        entries = [None] * len(tree)
        if subgrids is not None:
            subgrids = list(subgrids)
            if len(subgrids) != len(tree):
                raise ValueError("update_amr: %d subgrids given, the brick has %d (another tree is set_subgrids)" % (len(subgrids), len(tree)))
            for i, s in enumerate(subgrids):
                if s is None:
                    continue
                if hasattr(s, "ratio"):  # a scenes.Subgrid: its tree fields must be the stored ones
                    same_subgrid_tree([tree[i]], [s], "update_amr: subgrid %d" % i)
                    s = s.data
                parent, ratio, lo, cells = tree[i]
                shape = tuple(c * ratio + 1 for c in cells[::-1])
                if tuple(s.shape) != shape:
                    raise ValueError("update_amr: subgrid %d has data of shape %s, its cells and ratio need %s" % (i, tuple(s.shape), shape))
                entries[i] = s
                given.append(("subgrid %d" % i, s))
        if not given:
            raise ValueError("update_amr: nothing given (neither data nor a subgrid)")
        device = [hasattr(a, "data_ptr") and a.is_cuda for _, a in given]
        if any(device) and not all(device):
            raise ValueError("update_amr: the arrays must be all host arrays or all GPU tensors")
        keep = []

        def pointer(what, a):
            if hasattr(a, "data_ptr") and a.is_cuda:
                import torch

                if not a.is_contiguous() or self.dtype_of(a) != "float32":
                    raise ValueError("update_amr: %s: a device tensor must be contiguous float32" % what)
                torch.cuda.current_stream(a.device).synchronize()  # (written on torch's stream, copied on the library's)
                keep.append(a)
                return a.data_ptr()
            keep.append(np.ascontiguousarray(a.numpy() if hasattr(a, "data_ptr") else a, np.float32))
            return keep[-1].ctypes.data

        src = C.c_void_p(pointer("data", data)) if data is not None else None
        ptrs = None
        if subgrids is not None:
            ptrs = (C.c_void_p * len(tree))()
            for i, s in enumerate(entries):
                if s is not None:
                    ptrs[i] = pointer("subgrid %d" % i, s)
        ms = C.c_float(0.0)
        capi.check(self.lib.gvt_hip_volume_update_amr(self.h, src, C.c_size_t(int(np.prod(self.counts)) if data is not None else 0),
                                                      None if ptrs is None else C.cast(ptrs, C.c_void_p), len(tree) if ptrs is not None else 0,
                                                      C.c_uint32(1 if all(device) else 0), C.byref(ms)), "gvt_hip_volume_update_amr")
        if data is not None:
            self._data = keep[0]
        return float(ms.value)

    GRADIENT_KINDS = {"cell": capi.VOLUME_GRADIENT_CELL, "central": capi.VOLUME_GRADIENT_CENTRAL}

    def set_ghosts(self, faces):
        """gvt_hip_volume_set_ghosts: the six layers of global vertices just outside the brick, in the order -x +x -y +y -z +z; None = no
        layer (a face on the global grid's boundary has none).  +-x: (nz, ny), +-y: (nz, nx), +-z: (ny, nx), of the adapter's dtype: numpy
        arrays, or contiguous torch tensors on the GPU (all of them: no host round trip).  The library keeps its own copies."""
        faces = list(faces)
        if len(faces) != 6:
            raise ValueError("set_ghosts: six faces (-x +x -y +y -z +z, None for a missing one), not %d" % len(faces))
        nx, ny, nz = (int(v) for v in self.counts)
        shapes = [(nz, ny), (nz, ny), (nz, nx), (nz, nx), (ny, nx), (ny, nx)]
        want = getattr(self, "dtype_name", "float32")
        present = [f for f in faces if f is not None]
        device = [hasattr(f, "data_ptr") and f.is_cuda for f in present]
        if any(device) and not all(device):
            raise ValueError("set_ghosts: the faces must be all host arrays or all GPU tensors")
        ptrs = (C.c_void_p * 6)()
        keep = []
        for i, f in enumerate(faces):
            if f is None:
                continue
            if tuple(f.shape) != shapes[i]:
                raise ValueError("set_ghosts: face %d has shape %s, the brick needs %s" % (i, tuple(f.shape), shapes[i]))
            if hasattr(f, "data_ptr") and f.is_cuda:
                import torch

                if not f.is_contiguous() or self.dtype_of(f) != want:
                    raise ValueError("set_ghosts: a device tensor must be contiguous %s" % want)
                torch.cuda.current_stream(f.device).synchronize()  # (written on torch's stream, copied on the library's)
                keep.append(f)
                ptrs[i] = f.data_ptr()
            else:
                a = np.asarray(f.numpy() if hasattr(f, "data_ptr") else f)
                keep.append(np.ascontiguousarray(a, dtype=np.dtype(want)) if self.dtype_name == "float32" else np.ascontiguousarray(a))
                if keep[-1].dtype.name != want:
                    raise ValueError("set_ghosts: face %d of dtype %s, the brick holds %s" % (i, keep[-1].dtype, want))
                ptrs[i] = keep[-1].ctypes.data
        flags = capi.VOLUME_DEVICE if device and all(device) else 0
        capi.check(self.lib.gvt_hip_volume_set_ghosts(self.h, C.cast(ptrs, C.c_void_p), self.voxel_type, flags), "gvt_hip_volume_set_ghosts")

    def set_gradient(self, kind):
        """gvt_hip_volume_set_gradient: "cell" (the interpolant's gradient in the sample's cell, the default) or "central" (central
        differences at the vertices, interpolated; every face that is not on the global boundary needs its layer: set_ghosts)."""
        if kind not in self.GRADIENT_KINDS:
            raise ValueError("set_gradient: kind %r is neither 'cell' nor 'central'" % (kind,))
        capi.check(self.lib.gvt_hip_volume_set_gradient(self.h, self.GRADIENT_KINDS[kind]), "gvt_hip_volume_set_gradient")

    def gradient(self):
        """The gradient kind, "cell" or "central"."""
        k = C.c_int(-1)
        capi.check(self.lib.gvt_hip_volume_get_gradient(self.h, C.byref(k), None), "gvt_hip_volume_get_gradient")
        return {v: n for n, v in self.GRADIENT_KINDS.items()}[k.value]

    def central_marches(self):
        """The launches of this brick that shaded with central differences so far."""
        n = C.c_uint64(0)
        capi.check(self.lib.gvt_hip_volume_get_gradient(self.h, None, C.byref(n)), "gvt_hip_volume_get_gradient")
        return n.value

    def amr_info(self):
        """n_subgrids, n_levels, subgrid_bytes, samples_refined, amr_marches (gvt_hip_volume_get_amr_info)."""
        i = capi.VolumeAmrInfo()
        capi.check(self.lib.gvt_hip_volume_get_amr_info(self.h, C.byref(i)), "gvt_hip_volume_get_amr_info")
        return i.as_dict()

    def close(self):
        if getattr(self, "h", None):
            self.lib.gvt_hip_volume_destroy(self.h)
            self.h = None

    __del__ = close

    def set_transfer(self, tf):
        capi.check(self.lib.gvt_hip_volume_set_transfer(self.h, capi.ptr(tf.cmap), len(tf.cmap), capi.ptr(tf.omap), len(tf.omap),
                                                         tf.value_range[0], tf.value_range[1]), "gvt_hip_volume_set_transfer")

    def update_samples(self, data):
        """gvt_hip_volume_update_samples: the next time step's samples for the same brick, in place (every pointer a tracer borrowed stays
        valid; transfer function, surfaces and lights are kept).  data: a numpy array of the brick's shape (nz, ny, nx) and of the
        adapter's dtype (float32; a native adapter's own), or a contiguous torch tensor of that shape and dtype on the GPU (no host round
        trip); another dtype raises ValueError.  Returns the device time of the update in ms."""
        shape = tuple(int(c) for c in self.counts[::-1])
        if tuple(data.shape) != shape:
            raise ValueError("update_samples: data of shape %s, the brick has %s" % (tuple(data.shape), shape))
        ms = C.c_float(0.0)
        want = getattr(self, "dtype_name", "float32")
        if hasattr(data, "data_ptr"):  # a torch tensor: the device path
            import torch

            if not data.is_cuda:
                raise ValueError("update_samples: torch tensors must be on the GPU (pass numpy arrays for host data)")
            if not data.is_contiguous() or HipVolumeAdapter.dtype_of(data) != want:
                raise ValueError("update_samples: a device tensor must be contiguous %s" % want)
            torch.cuda.current_stream(data.device).synchronize()  # (the tensor is written on torch's stream, the update runs on the library's)
            src, flags = C.c_void_p(data.data_ptr()), 1
        else:
            if np.asarray(data).dtype.name != want:
                raise ValueError("update_samples: data of dtype %s, the brick holds %s" % (np.asarray(data).dtype, want))
            data = np.ascontiguousarray(data, dtype=np.dtype(want))
            src, flags = capi.ptr(data), 0
        capi.check(self.lib.gvt_hip_volume_update_samples_typed(self.h, src, self.voxel_type, C.c_size_t(int(np.prod(shape))), C.c_uint32(flags),
                                                                C.byref(ms)), "gvt_hip_volume_update_samples_typed")
        self._data = data
        return float(ms.value)

    def set_surfaces(self, isovalues=(), slices=(), opacity=1.0):
        """Volume::SetIsovalues / SetSlices: isovalues, then planes (nx, ny, nz, d) in the volume's own space, rendered shaded inside the
        march with one opacity.  Nothing given: the surfaces are cleared."""
        iso = capi.f32(isovalues, -1)
        pl = capi.f32(slices, -1).reshape(len(slices), 4)
        capi.check(self.lib.gvt_hip_volume_set_surfaces(self.h, capi.ptr(iso), len(iso), capi.ptr(pl), len(pl), float(opacity)),
                   "gvt_hip_volume_set_surfaces")

    def set_lights(self, lights, ka=0.4, kd=0.6):
        """The lights of the surfaces: a LIGHT_DTYPE array (position, color) or a sequence of (position, colour) pairs, world space;
        directional, from the position towards the origin (OSPRayAdapter.cpp:245-295).  ka / kd: that adapter's material."""
        if isinstance(lights, np.ndarray) and lights.dtype.names:
            pos, col = capi.f32(lights["position"], (-1, 3)), capi.f32(lights["color"], (-1, 3))
        else:
            lights = list(lights)
            pos = capi.f32([l[0] for l in lights], -1).reshape(len(lights), 3)
            col = capi.f32([l[1] for l in lights], -1).reshape(len(lights), 3)
        capi.check(self.lib.gvt_hip_volume_set_lights(self.h, capi.ptr(pos), capi.ptr(col), len(pos), float(ka), float(kd)),
                   "gvt_hip_volume_set_lights")

    def set_shading(self, on=True):
        """Lit volume: every sample the table gives opacity is shaded by the gradient of the interpolant in its cell, with the lights and
        ka / kd of set_lights (without lights the march stays unlit).  on=False: the plain march again."""
        mode = capi.VOLUME_SHADE_GRADIENT if on else capi.VOLUME_SHADE_NONE
        capi.check(self.lib.gvt_hip_volume_set_shading(self.h, mode), "gvt_hip_volume_set_shading")

    def shading(self):
        mode = C.c_int(-1)
        capi.check(self.lib.gvt_hip_volume_get_shading(self.h, C.byref(mode)), "gvt_hip_volume_get_shading")
        return mode.value

    def info(self):
        i = capi.VolumeInfo()
        capi.check(self.lib.gvt_hip_volume_get_info(self.h, C.byref(i)), "gvt_hip_volume_get_info")
        return i.as_dict()

    def crossings(self):
        """Surfaces composited by this brick's marches so far."""
        n = C.c_uint64(0)
        capi.check(self.lib.gvt_hip_volume_get_crossings(self.h, C.byref(n)), "gvt_hip_volume_get_crossings")
        return n.value

    def shaded(self):
        """Samples shaded by this brick's marches so far."""
        n = C.c_uint64(0)
        capi.check(self.lib.gvt_hip_volume_get_shaded(self.h, C.byref(n)), "gvt_hip_volume_get_shaded")
        return n.value

    def light_grid_info(self):
        """present, current, n_planes, bias, bytes of the brick's light transmittance grid (gvt_hip_volume_light_grid_info)."""
        i = capi.VolumeLightGridState()
        capi.check(self.lib.gvt_hip_volume_light_grid_info(self.h, C.byref(i)), "gvt_hip_volume_light_grid_info")
        return i.as_dict()

    def light_grid(self, j):
        """The baked transmittance towards light j at the brick's vertices, (nz, ny, nx) float32 (gvt_hip_volume_light_grid_download); a
        light that was unusable at the bake, or no grid: GvtHipError."""
        out = np.zeros(tuple(int(c) for c in self.counts[::-1]), np.float32)
        capi.check(self.lib.gvt_hip_volume_light_grid_download(self.h, int(j), capi.ptr(out)), "gvt_hip_volume_light_grid_download")
        return out

    def light_grid_release(self):
        capi.check(self.lib.gvt_hip_volume_light_grid_release(self.h), "gvt_hip_volume_light_grid_release")

    def occluder_grid_info(self):
        """present, current, n_planes, bytes of the brick's occluder grid (gvt_hip_volume_occluder_grid_info)."""
        i = capi.VolumeOccluderState()
        capi.check(self.lib.gvt_hip_volume_occluder_grid_info(self.h, C.byref(i)), "gvt_hip_volume_occluder_grid_info")
        return i.as_dict()

    def occluder_grid(self, j):
        """The baked occlusion towards light j at the brick's vertices, (nz, ny, nx) uint8, 0 = a mesh stands between the vertex and the
        light (gvt_hip_volume_occluder_grid_download); a light that was unusable at the bake, or no grid: GvtHipError."""
        out = np.zeros(tuple(int(c) for c in self.counts[::-1]), np.uint8)
        capi.check(self.lib.gvt_hip_volume_occluder_grid_download(self.h, int(j), capi.ptr(out)), "gvt_hip_volume_occluder_grid_download")
        return out

    def occluder_grid_release(self):
        capi.check(self.lib.gvt_hip_volume_occluder_grid_release(self.h), "gvt_hip_volume_occluder_grid_release")

    def ao_grid_info(self):
        """present, current, n_dirs, bias, radius, bytes of the brick's ambient occlusion grid (gvt_hip_volume_ao_grid_info)."""
        i = capi.VolumeAoState()
        capi.check(self.lib.gvt_hip_volume_ao_grid_info(self.h, C.byref(i)), "gvt_hip_volume_ao_grid_info")
        return i.as_dict()

    def ao_grid(self):
        """The baked ambient occlusion at the brick's vertices, (nz, ny, nx) float32, 1 = open (gvt_hip_volume_ao_grid_download); no grid:
        GvtHipError."""
        out = np.zeros(tuple(int(c) for c in self.counts[::-1]), np.float32)
        capi.check(self.lib.gvt_hip_volume_ao_grid_download(self.h, capi.ptr(out)), "gvt_hip_volume_ao_grid_download")
        return out

    def ao_grid_release(self):
        capi.check(self.lib.gvt_hip_volume_ao_grid_release(self.h), "gvt_hip_volume_ao_grid_release")

    def march_queue(self, queue, minv, may_clip=False):
        """gvt_hip_volume_march_queue: Adapter::trace on a device-resident RayQueue, in place and without a host wait; the rays keep
        their flags for the volume shuffle.  may_clip: the queue may hold rays that carry RAY_CLIP."""
        capi.check(self.lib.gvt_hip_volume_march_queue(self.h, queue.h, capi.ptr(capi.f32(minv, 16)), capi.MARCH_MAY_CLIP if may_clip else 0),
                   "gvt_hip_volume_march_queue")

    def trace(self, rays, m, minv, begin=0, end=0):
        """OSPRayAdapter::trace: every ray of rays[begin, end) comes back marched through the brick, with its flags."""
        rays = np.ascontiguousarray(rays, dtype=RAY_DTYPE)
        n_in = (end or len(rays)) - begin
        out = np.zeros(max(n_in, 0), RAY_DTYPE)
        n_out = C.c_size_t(0)
        capi.check(self.lib.gvt_hip_volume_trace(self.h, capi.ptr(rays), C.c_size_t(len(rays)), C.c_size_t(begin), C.c_size_t(end), capi.ptr(out),
                                                 C.c_size_t(len(out)), C.byref(n_out), capi.ptr(capi.f32(m, 16)), capi.ptr(capi.f32(minv, 16))),
                   "gvt_hip_volume_trace")
        return out[:n_out.value]
