"""The two live GraviT schedulers around Adapter::trace, re-hosted on device-resident ray queues.

  Tracer<ImageScheduler>::operator()   src/gvt/render/algorithm/ImageTracer.h:127-269
  Tracer<DomainScheduler>::operator()  src/gvt/render/algorithm/DomainTracer.h:115-496
  AbstractTrace::shuffleRays           src/gvt/render/algorithm/TracerBase.h:325-414

The loops are the reference's (pick the fullest queue, trace it, shuffle the moved rays; Domain: trace
until the local queues are dry, exchange, test for termination).  What changes is where the data
lives: queues, the top-level test, the framebuffer and the adapter all stay in HBM; under the Domain
scheduler the MPI ray exchange (DomainTracer.h:370-496) becomes point-to-point RCCL over xGMI through
torch.distributed, carrying the reference's own 80-byte Ray image (actor/Ray.h:161-174).

The device work goes through a small backend object so that the multi-rank control flow can be
exercised on CPU (gloo) in the tests with a checker backend; the product backend is HipBackend.
"""
import numpy as np

from . import capi
from .adapter import FrameBuffer, HipMeshAdapter, RayQueue, TopLevel, camera_generate
from .layouts import LIGHT_DTYPE, NORMALS_FLAT


class HipBackend:
    """One rank's device state: adapters (cached per mesh like adapterCache, ImageTracer.h:184-233),
    per-instance queues, top-level set, framebuffer."""

    def __init__(self, scene, normal_mode=NORMALS_FLAT, owned=None):
        self.scene = scene
        self.normal_mode = normal_mode
        self.n_inst = scene.n_inst
        self.owned = [True] * self.n_inst if owned is None else list(owned)
        self.top = TopLevel(scene.inst_lo, scene.inst_hi)
        self.queues = [RayQueue() for _ in range(self.n_inst)]
        self.q_cam = RayQueue()
        self.q_moved = RayQueue()
        cam = scene.camera
        self.fb = FrameBuffer(cam.width, cam.height)
        self.adapter_cache = {}
        self.calls = 0
        for i in range(self.n_inst):  # adapters are built lazily in the reference; here up front, off the frame clock
            if self.owned[i]:
                self.adapter(i)

    def adapter(self, inst):
        mi = self.scene.inst_mesh[inst]
        if mi not in self.adapter_cache:
            self.adapter_cache[mi] = HipMeshAdapter(self.scene.meshes[mi], self.normal_mode)
        return self.adapter_cache[mi]

    # ---- frame steps
    def begin_frame(self):
        self.fb.clear()
        for q in self.queues:
            q.clear()
        self.calls = 0

    def generate_and_filter(self, keep_mask=None):
        """camera rays -> FilterRaysLocally: shuffleRays(rays,-1) (ImageTracer.h:111-125) or, with a keep mask,
        shuffleDropRays (DomainTracer.h:148-183)."""
        import ctypes as C

        cam = self.scene.camera
        pod = capi.CameraPod((C.c_float * 3)(*cam.eye), (C.c_float * 3)(*cam.focus), (C.c_float * 3)(*cam.up), cam.fov, cam.width, cam.height,
                             cam.samples, cam.depth, cam.jitter)
        queues = (C.c_void_p * max(1, self.n_inst))(*[q.h for q in self.queues])
        km = None if keep_mask is None else np.ascontiguousarray(keep_mask, dtype=np.uint8)
        capi.check(capi.load().gvt_hip_camera_filter(self.top.h, C.byref(pod), C.c_int(8), queues, capi.ptr(km)), "gvt_hip_camera_filter")

    def queue_sizes(self):
        return [len(q) for q in self.queues]

    def image_frame(self):
        """Tracer<ImageScheduler>::operator() run natively inside the library (gvt_hip_image_frame); returns the number of adapter calls."""
        import ctypes as C

        s = self.scene
        cam = s.camera
        pod = capi.CameraPod((C.c_float * 3)(*cam.eye), (C.c_float * 3)(*cam.focus), (C.c_float * 3)(*cam.up), cam.fov, cam.width, cam.height,
                             cam.samples, cam.depth, cam.jitter)
        meshes = (C.c_void_p * max(1, self.n_inst))(*[self.adapter(i).h for i in range(self.n_inst)])
        queues = (C.c_void_p * max(1, self.n_inst))(*[q.h for q in self.queues])
        lights = np.ascontiguousarray(s.lights, dtype=LIGHT_DTYPE)  # (a concatenation of records drops the dtype's padding: always the ABI's 64-byte layout)
        calls = C.c_uint64(0)
        capi.check(capi.load().gvt_hip_image_frame(
            self.top.h, meshes, capi.ptr(capi.f32(s.m)), capi.ptr(capi.f32(s.minv)), capi.ptr(capi.f32(s.normi)), C.c_size_t(self.n_inst),
            capi.ptr(lights), C.c_size_t(len(lights)), C.c_int(self.normal_mode), C.byref(pod), queues, self.q_cam.h, self.q_moved.h, self.fb.h,
            C.byref(calls)), "gvt_hip_image_frame")
        return calls.value

    def trace_and_shuffle(self, inst):
        s = self.scene
        self.adapter(inst).trace_queue(self.queues[inst], self.q_moved, s.m[inst], s.minv[inst], s.normi[inst], s.lights, seed=self.calls,
                                       sink=(self.top, inst, self.fb))
        self.calls += 1
        self.top.shuffle(self.q_moved, inst, self.queues, self.fb, None)

    # ---- exchange (wire format: the reference's 80-byte Ray image)
    def export_wire(self, insts, torch, device):
        """Concatenate the queues `insts` into one wire tensor [n, 20] f32 and clear them."""
        sizes = [len(self.queues[i]) for i in insts]
        total = sum(sizes)
        buf = torch.empty((total, 20), dtype=torch.float32, device=device)
        off = 0
        for i, n in zip(insts, sizes):
            if n:
                self.queues[i].export_device(buf.data_ptr() + off * 80, n)
                self.queues[i].clear()
            off += n
        return buf

    def append_wire(self, inst, buf, off, n):
        if n:
            self.queues[inst].append_device(buf.data_ptr() + off * 80, n)

    def fb_tensor(self, torch, device):
        """torch view of the framebuffer's device memory (un-clamped sums) for the composite reduce."""
        cam = self.scene.camera

        class _View:
            __cuda_array_interface__ = {"shape": (cam.height * cam.width * 4,), "typestr": "<f4",
                                        "data": (self.fb.device_ptr(), False), "version": 2}

        return torch.as_tensor(_View(), device=device)

    def framebuffer(self, clamp=True):
        return self.fb.download(clamp)

    def sync(self):
        capi.synchronize()


class Context:
    """gvt_hip_ctx: a stream + scratch + counters of its own, current for the calling thread (several ranks in one process).
    `with Context(0): ...` in the thread that uses it; close() releases its stream, spill arena and scratch."""

    def __init__(self, device=0):
        import ctypes as C

        self.lib = capi.load()
        self.h = C.c_void_p(self.lib.gvt_hip_ctx_create(C.c_int(device)))
        if not self.h:
            raise capi.GvtHipError("gvt_hip_ctx_create: " + capi.last_error())
        capi.check(self.lib.gvt_hip_ctx_make_current(self.h), "gvt_hip_ctx_make_current")

    def close(self):
        if getattr(self, "h", None):
            self.lib.gvt_hip_ctx_make_current(None)
            self.lib.gvt_hip_ctx_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        import gc

        gc.collect()  # wrappers created under this context release their device memory before its stream goes
        self.close()
        return False


class Comm:
    """gvt_hip_comm: one rank's endpoint of the ray exchange.  Comm.rccl(dist-like broadcast) for one process per GPU,
    Comm.local(hub, rank) for in-process ranks."""

    def __init__(self, h):
        self.lib = capi.load()
        self.h = h
        self.rank = self.lib.gvt_hip_comm_rank(h)
        self.world = self.lib.gvt_hip_comm_world(h)

    @staticmethod
    def unique_id():
        import ctypes as C

        buf = (C.c_ubyte * 128)()
        capi.check(capi.load().gvt_hip_comm_unique_id(buf), "gvt_hip_comm_unique_id")
        return bytes(buf)

    @classmethod
    def rccl(cls, uid, rank, world):
        import ctypes as C

        buf = (C.c_ubyte * 128).from_buffer_copy(uid)
        h = C.c_void_p(capi.load().gvt_hip_comm_create(buf, C.c_int(rank), C.c_int(world)))
        if not h:
            raise capi.GvtHipError("gvt_hip_comm_create: " + capi.last_error())
        return cls(h)

    @classmethod
    def local(cls, hub, rank):
        import ctypes as C

        h = C.c_void_p(capi.load().gvt_hip_comm_create_local(C.c_void_p(hub), C.c_int(rank)))
        if not h:
            raise capi.GvtHipError("gvt_hip_comm_create_local: " + capi.last_error())
        return cls(h)

    @property
    def count(self):
        """ranks the transport itself reports (ncclCommCount; the hub's world)"""
        return self.lib.gvt_hip_comm_count(self.h)

    @property
    def reserved_cus(self):
        """compute units reserved for the communicator's own stream (knob comm_cus when it was created)"""
        return self.lib.gvt_hip_comm_reserved_cus(self.h)

    def set_deadline_ms(self, ms):
        import ctypes as C

        capi.check(self.lib.gvt_hip_comm_set_deadline_ms(self.h, C.c_int(int(ms))), "gvt_hip_comm_set_deadline_ms")

    def selftest(self, nbytes=1 << 20):
        import ctypes as C

        capi.check(self.lib.gvt_hip_comm_selftest(self.h, C.c_size_t(nbytes)), "gvt_hip_comm_selftest")

    def close(self):
        if getattr(self, "h", None):
            self.lib.gvt_hip_comm_destroy(self.h)
            self.h = None


class NativeTracer:
    """gvt_hip_tracer: Tracer<ImageScheduler> / Tracer<DomainScheduler> as a native loop inside libgvt_hip.so (csrc/domain.hip): rounds
    of one merged launch chain over all local queues, one host synchronisation per round, ray exchange over RCCL (or the in-process
    transport).  owner[i] = rank of instance i (mpiInstanceMap); comm=None: one rank."""

    def __init__(self, scene, normal_mode=NORMALS_FLAT, owner=None, comm=None, backend=None, replicate=False):
        import ctypes as C

        self.lib = capi.load()
        self.scene = scene
        self.comm = comm
        rank = comm.rank if comm is not None else 0
        self.owner = [0] * scene.n_inst if owner is None else list(owner)
        owned = [True] * scene.n_inst if replicate else [o == rank for o in self.owner]  # replicate: every mesh on every rank (Image scheduler)
        self.backend = backend or HipBackend(scene, normal_mode, owned)
        B = self.backend
        cam = scene.camera
        pod = capi.CameraPod((C.c_float * 3)(*cam.eye), (C.c_float * 3)(*cam.focus), (C.c_float * 3)(*cam.up), cam.fov, cam.width, cam.height,
                             cam.samples, cam.depth, cam.jitter)
        meshes = (C.c_void_p * max(1, scene.n_inst))(*[B.adapter(i).h if owned[i] else None for i in range(scene.n_inst)])
        lights = np.ascontiguousarray(scene.lights, dtype=LIGHT_DTYPE)  # (np.concatenate of light records packs them to 48 bytes: always the ABI's 64-byte layout)
        self.h = C.c_void_p(self.lib.gvt_hip_tracer_create(
            B.top.h, meshes, capi.ptr(capi.f32(scene.m)), capi.ptr(capi.f32(scene.minv)), capi.ptr(capi.f32(scene.normi)), C.c_size_t(scene.n_inst),
            capi.ptr(lights), C.c_size_t(len(lights)), C.c_int(normal_mode), C.byref(pod), B.fb.h))
        if not self.h:
            raise capi.GvtHipError("gvt_hip_tracer_create: " + capi.last_error())
        own = np.ascontiguousarray(self.owner, dtype=np.int32)
        capi.check(self.lib.gvt_hip_tracer_set_domains(self.h, capi.ptr(own), comm.h if comm is not None else None), "gvt_hip_tracer_set_domains")
        self.frame_stats = None  # the last frame's gvt_hip_frame_stats as the library filled it (`stats`: the same as a dict, made on access)

    @property
    def stats(self):
        return self.frame_stats.as_dict() if self.frame_stats is not None else {}

    def __call__(self, bsp=False, composite=True, full_reduce=False, image=False):
        import ctypes as C

        st = capi.FrameStats()
        flags = ((capi.FRAME_BSP if bsp else 0) | (0 if composite else capi.FRAME_NO_COMPOSITE) | (capi.FRAME_FULL_REDUCE if full_reduce else 0) |
                 (capi.FRAME_IMAGE if image else 0))
        capi.check(self.lib.gvt_hip_tracer_frame(self.h, C.c_int(flags), C.byref(st)), "gvt_hip_tracer_frame")
        self.frame_stats = st
        return self.backend

    render = __call__

    def set_camera(self, cam):
        """gvt_hip_tracer_set_camera: the next frame's camera (a moving camera re-uses the tracer, its queues and its framebuffer: same film size)."""
        import ctypes as C

        if (cam.width, cam.height) != (self.scene.camera.width, self.scene.camera.height):
            raise ValueError("set_camera: the film size belongs to the tracer's framebuffer")
        pod = capi.CameraPod((C.c_float * 3)(*cam.eye), (C.c_float * 3)(*cam.focus), (C.c_float * 3)(*cam.up), cam.fov, cam.width, cam.height,
                             cam.samples, cam.depth, cam.jitter)
        capi.check(self.lib.gvt_hip_tracer_set_camera(self.h, C.byref(pod)), "gvt_hip_tracer_set_camera")

    def set_transforms(self, m, minv, normi):
        """gvt_hip_tracer_set_transforms: the next frame's instance matrices (rigid motion)."""
        import ctypes as C

        m, minv, normi = capi.f32(m, (-1, 16)), capi.f32(minv, (-1, 16)), capi.f32(normi, (-1, 9))
        capi.check(self.lib.gvt_hip_tracer_set_transforms(self.h, capi.ptr(m), capi.ptr(minv), capi.ptr(normi), C.c_size_t(len(m))),
                   "gvt_hip_tracer_set_transforms")

    def update_scene(self, scene):
        """The next frame of an animation: `scene` has this tracer's topology (instances, their meshes, the meshes' triangles) and new vertices,
        instance boxes (scenes.instance_bbox), transforms or camera.  Changed meshes are refitted in place (normals as given, else regenerated),
        the top-level set and the tracer's matrices replaced; the same tracer, queues and framebuffer render the next frame."""
        old = self.scene
        if scene.n_inst != old.n_inst or list(scene.inst_mesh) != list(old.inst_mesh) or len(scene.meshes) != len(old.meshes):
            raise ValueError("update_scene: the instance set differs (create a new tracer)")
        for a, b in zip(old.meshes, scene.meshes):
            if a.tris.shape != b.tris.shape or len(a.verts) != len(b.verts) or not np.array_equal(a.tris, b.tris):
                raise ValueError("update_scene: a mesh's topology differs (create a new mesh and tracer)")
        B = self.backend
        for mi, ad in B.adapter_cache.items():
            mesh = scene.meshes[mi]
            verts = capi.f32(mesh.verts, (-1, 3))
            if np.array_equal(verts.view(np.uint32), ad.verts.view(np.uint32)) and mesh.vnormals is old.meshes[mi].vnormals:
                continue
            ad.update_vertices(verts, mesh.vnormals)
        B.top.update(scene.inst_lo, scene.inst_hi)
        self.set_transforms(scene.m, scene.minv, scene.normi)
        self.set_camera(scene.camera)
        self.scene = scene
        B.scene = scene

    def close(self):
        if getattr(self, "h", None):
            self.lib.gvt_hip_tracer_destroy(self.h)
            self.h = None

    __del__ = close


def _pick_fullest(sizes, allowed=None):
    """ImageTracer.h:159-173 / DomainTracer.h:235-241: first queue with the strictly largest size."""
    target, cnt = -1, 0
    for i, n in enumerate(sizes):
        if (allowed is None or allowed[i]) and n > cnt:
            cnt, target = n, i
    return target


class ImageTracer:
    """Tracer<ImageScheduler>, one rank (ImageTracer.h:127-269)."""

    def __init__(self, scene, normal_mode=NORMALS_FLAT, backend=None, native=True):
        self.backend = backend or HipBackend(scene, normal_mode)
        self.adapter_calls = 0
        self.native = native  # run the loop natively (gvt_hip_image_frame) when the backend offers it

    def __call__(self):
        B = self.backend
        if hasattr(B, "image_frame") and self.native:
            self.adapter_calls = B.image_frame()  # the same loop, inside libgvt_hip.so
            return B
        B.begin_frame()  # clearBuffer
        B.generate_and_filter(None)  # FilterRaysLocally
        self.adapter_calls = 0
        while True:
            target = _pick_fullest(B.queue_sizes())
            if target < 0:
                break
            B.trace_and_shuffle(target)  # adapter->trace + shuffleRays(moved_rays, instTarget)
            self.adapter_calls += 1
        return B

    render = __call__


class DomainTracer:
    """Tracer<DomainScheduler> over torch.distributed (DomainTracer.h:185-496).

    owner[i] = rank that holds instance i's data (mpiInstanceMap, DomainTracer.h:115-144).  Per round:
    trace until the local queues are dry, then SendRays: one all-gather of the per-queue outgoing counts
    (replaces the count exchange :409-415 and, because every rank then knows how many rays are in
    flight, also the gather/scatter termination test :337-349) and one point-to-point payload exchange
    (:433-463).  The frame ends with a sum-reduce of the float framebuffers to rank 0
    (IceTComposite::composite, IceTComposite.cpp:84-101).
    """

    def __init__(self, scene, owner, dist, torch, comm_device, normal_mode=NORMALS_FLAT, backend=None, overlap=False):
        self.overlap = overlap  # post each exchange before the next local adapter call and complete it afterwards
        self.scene = scene
        self.owner = list(owner)
        self.dist, self.torch, self.dev = dist, torch, comm_device
        self.on_cuda = torch.device(comm_device).type == "cuda"
        self.rank = dist.get_rank() if dist.is_initialized() else 0
        self.world = dist.get_world_size() if dist.is_initialized() else 1
        self.owned = [o == self.rank for o in self.owner]
        self.backend = backend or HipBackend(scene, normal_mode, self.owned)
        self.rounds = 0
        self.rays_sent = 0
        self.adapter_calls = 0

    def _post_exchange(self, counts, sizes):
        """SendRays payload (:433-463) as non-blocking point-to-point operations; returns (requests, receive buffers, send buffers)."""
        B, torch, dist = self.backend, self.torch, self.dist
        n_inst = len(self.owner)
        ops, send_bufs, recv_bufs = [], {}, {}
        for p in range(self.world):
            if p == self.rank:
                continue
            outq = [i for i in range(n_inst) if self.owner[i] == p and sizes[i] > 0]
            if outq:
                send_bufs[p] = B.export_wire(outq, torch, self.dev)
                self.rays_sent += int(send_bufs[p].shape[0])
                ops.append(dist.P2POp(dist.isend, send_bufs[p], p))
            n_in = int(sum(counts[p][i] for i in range(n_inst) if self.owned[i]))
            if n_in:
                recv_bufs[p] = torch.empty((n_in, 20), dtype=torch.float32, device=self.dev)
                ops.append(dist.P2POp(dist.irecv, recv_bufs[p], p))
        B.sync()  # wire buffers were filled on the adapter stream
        reqs = dist.batch_isend_irecv(ops) if ops else []
        return reqs, recv_bufs, send_bufs

    def _complete_exchange(self, posted, counts):
        reqs, recv_bufs, _send_bufs = posted
        for req in reqs:
            req.wait()
        if self.on_cuda:
            self.torch.cuda.current_stream().synchronize()
        for p, buf in recv_bufs.items():
            self._unpack(buf, counts[p])

    def _unpack(self, buf, counts_p):
        """A received payload into queue[q] (:466-481): peer p's rays for this rank's instances lie in instance order."""
        B = self.backend
        off = 0
        for i in range(len(self.owner)):
            if self.owned[i] and counts_p[i]:
                B.append_wire(i, buf, off, int(counts_p[i]))
                off += int(counts_p[i])

    def _frame_overlapped(self):
        """The same frame with the ray exchange overlapped with traversal: every iteration all ranks exchange the outgoing counts (and
        whether they still hold local work), post the payload transfers of what has accumulated so far, run ONE local adapter call
        while those move (RCCL on its own stream), then complete the transfers.  Ends when no rank has local work and nothing is in
        flight -- the vote of the reference's asynchronous tracer (tracer/Domain/DomainTracer.cpp:109-192) folded into the count
        exchange.  Same rays, same image; only the interleaving differs."""
        B, torch, dist = self.backend, self.torch, self.dist
        n_inst = len(self.owner)
        B.begin_frame()
        B.generate_and_filter(np.array(self.owned, np.uint8))  # shuffleDropRays
        self.rounds = self.rays_sent = self.adapter_calls = 0
        while True:
            sizes = B.queue_sizes()
            target = _pick_fullest(sizes, self.owned)
            if self.world == 1:
                if target < 0:
                    break
                B.trace_and_shuffle(target)
                self.adapter_calls += 1
                continue
            mine = torch.tensor([0 if self.owned[i] else sizes[i] for i in range(n_inst)] + [1 if target >= 0 else 0], dtype=torch.int64,
                                device=self.dev)
            allc = torch.empty((self.world, n_inst + 1), dtype=torch.int64, device=self.dev)
            rows = [allc[r] for r in range(self.world)]
            dist.all_gather(rows, mine)
            counts = torch.stack(rows).cpu().numpy()
            if int(counts[:, :n_inst].sum()) == 0 and int(counts[:, n_inst].sum()) == 0:
                break
            posted = self._post_exchange(counts, sizes)
            if target >= 0:  # one local adapter call while the payload moves
                B.trace_and_shuffle(target)
                self.adapter_calls += 1
            self._complete_exchange(posted, counts)
            self.rounds += 1
        return B

    def __call__(self):
        if self.overlap:
            return self._frame_overlapped()
        B, torch, dist = self.backend, self.torch, self.dist
        n_inst = len(self.owner)
        B.begin_frame()
        B.generate_and_filter(np.array(self.owned, np.uint8))  # shuffleDropRays
        self.rounds = self.rays_sent = self.adapter_calls = 0
        while True:
            while True:  # local work until dry (:228-326)
                target = _pick_fullest(B.queue_sizes(), self.owned)
                if target < 0:
                    break
                B.trace_and_shuffle(target)
                self.adapter_calls += 1
            self.rounds += 1
            if self.world == 1:
                break
            # ---- SendRays (:370-496)
            sizes = B.queue_sizes()
            mine = torch.tensor([0 if self.owned[i] else sizes[i] for i in range(n_inst)], dtype=torch.int64, device=self.dev)
            allc = torch.empty((self.world, n_inst), dtype=torch.int64, device=self.dev)
            rows = [allc[r] for r in range(self.world)]
            dist.all_gather(rows, mine)
            counts = torch.stack(rows).cpu().numpy()
            in_flight = int(counts.sum())
            if in_flight == 0:  # all_done (:337-349)
                break
            ops, send_bufs, recv_bufs = [], {}, {}
            for p in range(self.world):
                if p == self.rank:
                    continue
                outq = [i for i in range(n_inst) if self.owner[i] == p and sizes[i] > 0]
                if outq:
                    send_bufs[p] = B.export_wire(outq, torch, self.dev)
                    self.rays_sent += int(send_bufs[p].shape[0])
                    ops.append(dist.P2POp(dist.isend, send_bufs[p], p))
                n_in = int(sum(counts[p][i] for i in range(n_inst) if self.owned[i]))
                if n_in:
                    recv_bufs[p] = torch.empty((n_in, 20), dtype=torch.float32, device=self.dev)
                    ops.append(dist.P2POp(dist.irecv, recv_bufs[p], p))
            B.sync()  # wire buffers were filled on the adapter stream
            if ops:
                for req in dist.batch_isend_irecv(ops):
                    req.wait()
            if self.on_cuda:
                torch.cuda.current_stream().synchronize()
            for p, buf in recv_bufs.items():
                self._unpack(buf, counts[p])
        return B

    render = __call__

    def composite(self, download=True, rows_only=True):
        """Sum of the per-rank float framebuffers on rank 0 (in place, in HBM), then -- if download -- the localAdd clamp and the
        copy to the host.  Returns (H,W,4) on rank 0, None elsewhere or when download is False.

        rows_only: a rank's deposits lie where its domains project, so instead of a sum-reduce of whole frames (IceT's job in the
        reference, IceTComposite.cpp:84-101) every rank sends rank 0 just the bounding rectangle of the pixels it wrote to: one
        all-gather of the rectangles, point-to-point transfers, an add per rectangle.  Same sums, rank order instead of tree order."""
        B, torch, dist = self.backend, self.torch, self.dist
        cam = self.scene.camera
        if self.world == 1:
            return B.framebuffer(True) if download else None
        B.sync()
        t = B.fb_tensor(torch, self.dev)
        if not rows_only:
            dist.reduce(t, dst=0, op=dist.ReduceOp.SUM)
        else:
            img = t.view(cam.height, cam.width, 4)
            lit = img[..., 3] > 0  # every deposit counts in the fourth component (localAdd adds 1.0)
            ys = torch.nonzero(lit.any(dim=1)).flatten()
            xs = torch.nonzero(lit.any(dim=0)).flatten()
            box = [int(ys[0].item()), int(ys[-1].item()) + 1, int(xs[0].item()), int(xs[-1].item()) + 1] if ys.numel() else [0, 0, 0, 0]
            mine = torch.tensor(box, dtype=torch.int64, device=self.dev)
            allr = torch.empty((self.world, 4), dtype=torch.int64, device=self.dev)
            parts = [allr[r] for r in range(self.world)]
            dist.all_gather(parts, mine)
            boxes = torch.stack(parts).cpu().numpy()
            ops, bufs = [], {}
            if self.rank == 0:
                for p in range(1, self.world):
                    y0, y1, x0, x1 = (int(v) for v in boxes[p])
                    if y1 > y0:
                        bufs[p] = torch.empty((y1 - y0, x1 - x0, 4), dtype=torch.float32, device=self.dev)
                        ops.append(dist.P2POp(dist.irecv, bufs[p], p))
            elif box[1] > box[0]:
                bufs[0] = img[box[0]:box[1], box[2]:box[3]].contiguous()
                ops.append(dist.P2POp(dist.isend, bufs[0], 0))
            if ops:
                for req in dist.batch_isend_irecv(ops):
                    req.wait()
            if self.rank == 0:
                for p, buf in bufs.items():
                    y0, y1, x0, x1 = (int(v) for v in boxes[p])
                    img[y0:y1, x0:x1] += buf
        if self.on_cuda:
            torch.cuda.current_stream().synchronize()
        if self.rank != 0 or not download:
            return None
        return B.framebuffer(True).reshape(cam.height, cam.width, 4)


class VolumeTracer:
    """Tracer<ImageScheduler> over the bricks of one volume instance (gvt_hip_volume_frame): bricks = scenes.split_volume(...) (or one
    VolumeData), m = the instance's matrix (None: identity).  Bricks may carry AMR subgrids (scenes.split_amr_volume, scenes.refine).  The world box of a brick is its box under m (scenes.instance_bbox).
    native: HipVolumeAdapter's (uint8 / int16 / uint16 bricks stored at their own width).
    amr_shaded: HipVolumeAdapter's -- the bricks' subgrids are set with capi.VOLUME_AMR_SHADED, so set_surfaces, set_lights and set_shading work
    on AMR bricks too (isovalues, slice planes and lit fog in the refined cells); such frames take the loop unless fused_amr is given (the
    shadowed frames and the bakes refuse a brick with subgrids unless shadow_amr is given).  Without it (the default) the setters are refused on a brick that has subgrids.
    fused: frame() goes through gvt_hip_volume_frame_fused -- every brick in ONE march launch where the frame is eligible (plain bricks of
    one grid), the loop otherwise; the image is the loop's in every bit either way.  Default: the loop.
    fused_shaded (with fused): frame() goes through gvt_hip_volume_frame_fused_shaded with both bits (fused_allow), so frames with
    isovalues, slice planes or lit fog are fused too; without it such frames take the loop, as ever.
    fused_central: fused_allow gains capi.FUSED_CENTRAL, and every VolumeShadowParams, VolumeLightGridParams and VolumeOccluderParams the
    tracer builds carries capi.VOLUME_ALLOW_CENTRAL -- frames whose bricks all have set_gradient("central") are fused, shadowed and baked
    too (the kernels' CENTRAL instantiations; the image is the loop's in every bit where a loop exists).  Without it (the default) such a
    frame takes the loop under fused_shaded and is refused by the shadowed frames and the bakes, as ever.
    fused_amr (with fused; alone it raises ValueError): frame() goes through gvt_hip_volume_frame_fused_amr with capi.FUSED_AMR, plus
    FUSED_SURFACES | FUSED_LIT if fused_shaded, plus FUSED_CENTRAL if fused_central -- frames in which some or all bricks have subgrids
    are fused too (the kernels' AMR instantiations; the image is the loop's in every bit).  Without it (the default) such frames take the
    loop, as ever.  shadows=True on bricks with subgrids stays refused unless shadow_amr is given.
    shadow_amr (with shadows; alone it raises ValueError): every VolumeShadowParams, VolumeLightGridParams and VolumeOccluderParams the
    tracer builds carries capi.VOLUME_ALLOW_AMR too -- the shadowed, fog-shadowed and mesh-shadowed frames and both bakes take bricks with
    subgrids (the kernels' AMR instantiations; features carries capi.FUSED_AMR where one ran; the light and occluder grids stay at the
    bricks' level-0 vertices).  Deliberately not derived from fused_amr: without it (the default) such frames and bakes are refused, as ever.
    shadows: frame() goes through gvt_hip_volume_frame_shadowed whatever fused says -- a crossing is lit only by the lights that reach it,
    a shadow ray per light marched inside the one launch; shadow_bias = the lattice index of a shadow ray's first sample (1 .. 64; 2 is
    a choice, not a measurement).  A frame that has surfaces and lights but cannot be fused is refused (GvtHipError): no loop renders
    shadows.  Without surfaces or without lights the frame is fused_shaded's.
    fog_shadows (with shadows; alone it raises ValueError): frame() goes through gvt_hip_volume_frame_fog_shadowed -- lit fog samples are
    shadowed too, by the transmittance towards each light interpolated from grids baked at the vertices (gvt_hip_volume_light_grid_bake;
    fog_bias = the bake's bias).  frame() bakes on the first frame that has lit fog and a usable light, and again after update(),
    set_surfaces() or set_lights() -- the cost is per change of data, table, surfaces or lights, not per frame; rebake() is explicit
    (needed after a call on a single adapter, which the tracer does not see: the library then refuses the frame).
    mesh_shadows (with shadows and fog_shadows; otherwise ValueError): frame() goes through gvt_hip_volume_frame_mesh_shadowed -- meshes
    cast shadows into the volume, from occluder grids baked at the vertices (gvt_hip_volume_occluder_grid_bake).  bake_occluders(scene)
    bakes them; frame() bakes again from the same scene after set_lights().  The library cannot see a mesh move: call bake_occluders
    again after the scene changed.  A frame that needs a grid and has none is refused (GvtHipError).
    ao (with shadows and fog_shadows, without shadow_amr; otherwise ValueError): frame() goes through gvt_hip_volume_frame_ao -- with
    capi.VOLUME_AO_MESH when mesh_shadows is set -- so the ambient term is ka times the ambient occlusion interpolated from a grid baked at
    the vertices (gvt_hip_volume_ao_grid_bake).  ao_dirs: a count (scenes.ao_directions) or an (n, 3) array of world-space directions;
    ao_radius: the AO rays' length (None: 16 lattice steps); ao_bias: the bake's bias.  frame() bakes on the first frame that needs the
    grid and again after update(), set_surfaces() and set_transfer(), not after set_lights(); rebake_ao() is explicit."""

    def __init__(self, bricks, camera, tf, m=None, sampling_rate=1.0, skip=True, native=False, fused=False, fused_shaded=False, shadows=False, shadow_bias=2,
                 fog_shadows=False, fog_bias=1, mesh_shadows=False, fused_central=False, amr_shaded=False, fused_amr=False, shadow_amr=False,
                 ao=False, ao_dirs=16, ao_radius=None, ao_bias=1):
        import ctypes as C

        from .adapter import HipVolumeAdapter
        from .scenes import instance_matrices, mat_translate_scale

        if fog_shadows and not shadows:
            raise ValueError("VolumeTracer: fog_shadows needs shadows=True (the fog-shadowed frame is the shadowed frame with one more change)")
        if mesh_shadows and not (shadows and fog_shadows):
            raise ValueError("VolumeTracer: mesh_shadows needs shadows=True and fog_shadows=True (the mesh-shadowed frame is the fog-shadowed frame with one more change)")
        if fused_amr and not fused:
            raise ValueError("VolumeTracer: fused_amr needs fused=True (it is one more allow bit of the fused frame)")
        if ao and not (shadows and fog_shadows):
            raise ValueError("VolumeTracer: ao needs shadows=True and fog_shadows=True (the AO frame is the fog-shadowed frame with one more change)")
        if ao and shadow_amr:
            raise ValueError("VolumeTracer: ao does not take shadow_amr (an AO grid never covers subgrids)")
        if shadow_amr and not shadows:
            raise ValueError("VolumeTracer: shadow_amr needs shadows=True (it is one more flag bit of the shadowed frames and their bakes)")
        bricks = list(bricks) if isinstance(bricks, (list, tuple)) else [bricks]
        self.camera = camera
        self.m = capi.f32(mat_translate_scale((0, 0, 0), (1, 1, 1)) if m is None else m, 16)
        _refuse_turned_bricks(self.m, len(bricks), "VolumeTracer")
        self.minv = instance_matrices(self.m)[0]
        self.adapters = [HipVolumeAdapter(b, sampling_rate, skip, native, amr_shaded) for b in bricks]
        for a in self.adapters:
            a.set_transfer(tf)
        self.inst_lo, self.inst_hi = _brick_boxes(bricks, self.m)
        self.n_inst = len(bricks)
        self.top = TopLevel(self.inst_lo, self.inst_hi)
        self.queues = [RayQueue() for _ in range(self.n_inst)]
        self.fb = FrameBuffer(camera.width, camera.height)
        self.calls = 0
        self.fused = bool(fused)
        self.fused_shaded = bool(fused_shaded)
        self.fused_central = bool(fused_central)
        self.fused_allow = capi.FUSED_SURFACES | capi.FUSED_LIT | (capi.FUSED_CENTRAL if self.fused_central else 0)  # fused_shaded=True: the allow word of gvt_hip_volume_frame_fused_shaded
        self.fused_amr = bool(fused_amr)
        # fused_amr=True: the allow word of gvt_hip_volume_frame_fused_amr
        self.fused_amr_allow = capi.FUSED_AMR | (capi.FUSED_SURFACES | capi.FUSED_LIT if self.fused_shaded else 0) | (capi.FUSED_CENTRAL if self.fused_central else 0)
        self.shadow_amr = bool(shadow_amr)
        # the flags word of the shadowed frames' and the bakes' params
        self.param_flags = (capi.VOLUME_ALLOW_CENTRAL if self.fused_central else 0) | (capi.VOLUME_ALLOW_AMR if self.shadow_amr else 0)
        self.fused_stats = None  # fused=True: gvt_hip_volume_fused_stats (fused_shaded: gvt_hip_volume_fused_shaded_stats; fused_amr: gvt_hip_volume_fused_amr_stats) of the last frame, as a dict
        self.shadows = bool(shadows)
        self.shadow_bias = int(shadow_bias)
        self.shadow_stats = None  # shadows=True: gvt_hip_volume_shadow_stats of the last frame, as a dict
        self.fog_shadows = bool(fog_shadows)
        self.fog_bias = int(fog_bias)
        self.light_bakes = 0
        self.light_grid_stats = None  # fog_shadows=True: gvt_hip_volume_light_grid_stats of the last bake, as a dict
        self._grid_stale = True  # nothing baked yet, or a setter / update of this tracer since the last bake
        self.mesh_shadows = bool(mesh_shadows)
        self.occluder_bakes = 0
        self.occluder_stats = None  # mesh_shadows=True: gvt_hip_volume_occluder_stats of the last bake, as a dict
        self._occluder_source = None  # the scene or backend of the last bake_occluders: what frame() bakes from again
        self._occluder_stale = True  # nothing baked yet, or set_lights since the last bake
        self._occluder_kept = None  # adapter.scene_instances' third result: the mesh adapters made here for a scenes.Scene
        self.ao = bool(ao)
        if isinstance(ao_dirs, (int, np.integer)):
            from .scenes import ao_directions

            ao_dirs = ao_directions(int(ao_dirs))
        self.ao_dirs = np.ascontiguousarray(ao_dirs, np.float32).reshape(-1, 3)
        if self.ao and not 1 <= len(self.ao_dirs) <= capi.VOLUME_AO_MAX_DIRS:
            raise ValueError("VolumeTracer: %d AO directions, 1 to %d are allowed" % (len(self.ao_dirs), capi.VOLUME_AO_MAX_DIRS))
        self.ao_radius = None if ao_radius is None else float(ao_radius)  # None: 16 lattice steps, taken from the first brick at the bake
        self.ao_bias = int(ao_bias)
        self.ao_bakes = 0
        self.ao_stats = None  # ao=True: gvt_hip_volume_ao_stats of the last bake, as a dict
        self._ao_stale = True  # nothing baked yet, or update / set_surfaces / set_transfer since the last bake
        self._surfaces = False  # set_surfaces with at least one isovalue or slice plane?
        self._lit = False  # set_shading(True)?
        self._usable_lights = 0  # lights of set_lights that cast shadow rays
        self._arr = lambda xs: (C.c_void_p * max(1, self.n_inst))(*[x.h for x in xs])

    def frame(self, depth=None):
        """One frame; depth (an adapter.DepthPlane of the film's size): every camera ray is clipped at its pixel's depth
        (gvt_hip_volume_frame_clipped: geometry inside the volume)."""
        import ctypes as C

        cam = self.camera
        pod = capi.CameraPod((C.c_float * 3)(*cam.eye), (C.c_float * 3)(*cam.focus), (C.c_float * 3)(*cam.up), cam.fov, cam.width, cam.height,
                             cam.samples, cam.depth, cam.jitter)
        m = np.ascontiguousarray(np.tile(self.m, self.n_inst), np.float32)
        minv = np.ascontiguousarray(np.tile(self.minv, self.n_inst), np.float32)
        calls = C.c_uint64(0)
        if self.ao and self.shadows and self.fog_shadows:
            if self._grid_stale and self._lit and self._usable_lights:
                self.rebake()
            if self.mesh_shadows and self._occluder_stale and self._occluder_source is not None and self._usable_lights and (self._lit or self._surfaces):
                self.bake_occluders(self._occluder_source)
            if self._ao_stale and self._usable_lights and (self._lit or self._surfaces):
                self.rebake_ao()
            st = capi.VolumeAoFrameStats()
            params = capi.VolumeAoFrameParams(self.param_flags | (capi.VOLUME_AO_MESH if self.mesh_shadows else 0), self.shadow_bias)
            capi.check(capi.load().gvt_hip_volume_frame_ao(self.top.h, self._arr(self.adapters), capi.ptr(m), capi.ptr(minv), C.c_size_t(self.n_inst),
                                                           C.byref(pod), self._arr(self.queues), self.fb.h, None if depth is None else depth.h,
                                                           C.byref(params), C.byref(st)), "gvt_hip_volume_frame_ao")
            self.shadow_stats = st.as_dict()
            calls = C.c_uint64(st.base.fog.adapter_calls)
        elif self.mesh_shadows:
            if self._grid_stale and self._lit and self._usable_lights:
                self.rebake()
            if self._occluder_stale and self._occluder_source is not None and self._usable_lights and (self._lit or self._surfaces):
                self.bake_occluders(self._occluder_source)
            st = capi.VolumeMeshShadowStats()
            params = capi.VolumeShadowParams(self.param_flags, self.shadow_bias)
            capi.check(capi.load().gvt_hip_volume_frame_mesh_shadowed(self.top.h, self._arr(self.adapters), capi.ptr(m), capi.ptr(minv), C.c_size_t(self.n_inst),
                                                                      C.byref(pod), self._arr(self.queues), self.fb.h, None if depth is None else depth.h,
                                                                      C.byref(params), C.byref(st)), "gvt_hip_volume_frame_mesh_shadowed")
            self.shadow_stats = st.as_dict()
            calls = C.c_uint64(st.fog.adapter_calls)
        elif self.shadows and self.fog_shadows:
            if self._grid_stale and self._lit and self._usable_lights:
                self.rebake()
            st = capi.VolumeFogShadowStats()
            params = capi.VolumeShadowParams(self.param_flags, self.shadow_bias)
            capi.check(capi.load().gvt_hip_volume_frame_fog_shadowed(self.top.h, self._arr(self.adapters), capi.ptr(m), capi.ptr(minv), C.c_size_t(self.n_inst),
                                                                     C.byref(pod), self._arr(self.queues), self.fb.h, None if depth is None else depth.h,
                                                                     C.byref(params), C.byref(st)), "gvt_hip_volume_frame_fog_shadowed")
            self.shadow_stats = st.as_dict()
            calls = C.c_uint64(st.adapter_calls)
        elif self.shadows:
            st = capi.VolumeShadowStats()
            params = capi.VolumeShadowParams(self.param_flags, self.shadow_bias)
            capi.check(capi.load().gvt_hip_volume_frame_shadowed(self.top.h, self._arr(self.adapters), capi.ptr(m), capi.ptr(minv), C.c_size_t(self.n_inst),
                                                                 C.byref(pod), self._arr(self.queues), self.fb.h, None if depth is None else depth.h,
                                                                 C.byref(params), C.byref(st)), "gvt_hip_volume_frame_shadowed")
            self.shadow_stats = st.as_dict()
            calls = C.c_uint64(st.adapter_calls)
        elif self.fused and self.fused_amr:
            st = capi.VolumeFusedAmrStats()
            capi.check(capi.load().gvt_hip_volume_frame_fused_amr(self.top.h, self._arr(self.adapters), capi.ptr(m), capi.ptr(minv), C.c_size_t(self.n_inst),
                                                                  C.byref(pod), self._arr(self.queues), self.fb.h, None if depth is None else depth.h,
                                                                  C.c_uint32(self.fused_amr_allow), C.byref(st)), "gvt_hip_volume_frame_fused_amr")
            self.fused_stats = st.as_dict()
            calls = C.c_uint64(st.adapter_calls)
        elif self.fused and self.fused_shaded:
            st = capi.VolumeFusedShadedStats()
            capi.check(capi.load().gvt_hip_volume_frame_fused_shaded(self.top.h, self._arr(self.adapters), capi.ptr(m), capi.ptr(minv), C.c_size_t(self.n_inst),
                                                                     C.byref(pod), self._arr(self.queues), self.fb.h, None if depth is None else depth.h,
                                                                     C.c_uint32(self.fused_allow), C.byref(st)), "gvt_hip_volume_frame_fused_shaded")
            self.fused_stats = st.as_dict()
            calls = C.c_uint64(st.adapter_calls)
        elif self.fused:
            st = capi.VolumeFusedStats()
            capi.check(capi.load().gvt_hip_volume_frame_fused(self.top.h, self._arr(self.adapters), capi.ptr(m), capi.ptr(minv), C.c_size_t(self.n_inst),
                                                              C.byref(pod), self._arr(self.queues), self.fb.h, None if depth is None else depth.h,
                                                              C.byref(st)), "gvt_hip_volume_frame_fused")
            self.fused_stats = st.as_dict()
            calls = C.c_uint64(st.adapter_calls)
        elif depth is None:
            capi.check(capi.load().gvt_hip_volume_frame(self.top.h, self._arr(self.adapters), capi.ptr(m), capi.ptr(minv), C.c_size_t(self.n_inst),
                                                        C.byref(pod), self._arr(self.queues), self.fb.h, C.byref(calls)), "gvt_hip_volume_frame")
        else:
            capi.check(capi.load().gvt_hip_volume_frame_clipped(self.top.h, self._arr(self.adapters), capi.ptr(m), capi.ptr(minv), self.n_inst,
                                                                C.byref(pod), self._arr(self.queues), self.fb.h, depth.h, C.byref(calls)),
                       "gvt_hip_volume_frame_clipped")
        self.calls = calls.value
        return self

    def rebake(self):
        """gvt_hip_volume_light_grid_bake over the tracer's bricks under its matrix: the light grids of the fog-shadowed frame."""
        import ctypes as C

        m = np.ascontiguousarray(np.tile(self.m, self.n_inst), np.float32)
        minv = np.ascontiguousarray(np.tile(self.minv, self.n_inst), np.float32)
        st = capi.VolumeLightGridStats()
        params = capi.VolumeLightGridParams(self.param_flags, self.fog_bias)
        capi.check(capi.load().gvt_hip_volume_light_grid_bake(self._arr(self.adapters), capi.ptr(m), capi.ptr(minv), C.c_size_t(self.n_inst), C.byref(params),
                                                              C.byref(st)), "gvt_hip_volume_light_grid_bake")
        self.light_grid_stats = st.as_dict()
        self.light_bakes += 1
        self._grid_stale = False
        return self

    def rebake_ao(self):
        """gvt_hip_volume_ao_grid_bake over the tracer's bricks under its matrix: the AO grid of the AO frame."""
        import ctypes as C

        m = np.ascontiguousarray(np.tile(self.m, self.n_inst), np.float32)
        minv = np.ascontiguousarray(np.tile(self.minv, self.n_inst), np.float32)
        radius = 16.0 * float(self.adapters[0].info()["dt"]) if self.ao_radius is None else self.ao_radius
        params = capi.VolumeAoParams(self.param_flags, self.ao_bias, len(self.ao_dirs), radius)
        for i, d in enumerate(self.ao_dirs):
            params.dirs[i][:] = [float(x) for x in d]
        st = capi.VolumeAoStats()
        capi.check(capi.load().gvt_hip_volume_ao_grid_bake(self._arr(self.adapters), capi.ptr(m), capi.ptr(minv), C.c_size_t(self.n_inst), C.byref(params),
                                                           C.byref(st)), "gvt_hip_volume_ao_grid_bake")
        self.ao_stats = st.as_dict()
        self.ao_bakes += 1
        self._ao_stale = False
        return self

    def bake_occluders(self, scene_or_backend):
        """gvt_hip_volume_occluder_grid_bake over the tracer's bricks under its matrix: which vertices the meshes of scene_or_backend (a
        scenes.Scene or a scheduler.HipBackend, taken as adapter.DepthPlane.render takes them) shadow from each usable light."""
        import ctypes as C

        from .adapter import scene_instances

        scene, adapters, self._occluder_kept = scene_instances(scene_or_backend, self._occluder_kept)
        m = np.ascontiguousarray(np.tile(self.m, self.n_inst), np.float32)
        minv = np.ascontiguousarray(np.tile(self.minv, self.n_inst), np.float32)
        meshes = (C.c_void_p * max(1, scene.n_inst))(*[a.h for a in adapters])
        mesh_minv = capi.f32(scene.minv)
        st = capi.VolumeOccluderStats()
        params = capi.VolumeOccluderParams(self.param_flags, 0)
        capi.check(capi.load().gvt_hip_volume_occluder_grid_bake(self._arr(self.adapters), capi.ptr(m), capi.ptr(minv), C.c_size_t(self.n_inst), meshes,
                                                                 capi.ptr(mesh_minv), C.c_size_t(scene.n_inst), C.byref(params), C.byref(st)),
                   "gvt_hip_volume_occluder_grid_bake")
        self.occluder_stats = st.as_dict()
        self.occluder_bakes += 1
        self._occluder_source = scene_or_backend
        self._occluder_stale = False
        return self

    @staticmethod
    def _same_bricking(adapters, bricks, amr=False):
        """Helper of update(), not part of the tracer's surface (static so that the check runs without a device): the bricks of another time
        step as a list, if they are the adapters' bricking (counts and offset per brick; a whole VolumeData has offset 0) and, for adapters
        that name one (dtype_name), of their dtype; with amr also of their subgrid tree (adapter.same_subgrid_tree against the adapter's
        .tree); ValueError otherwise."""
        from .adapter import same_subgrid_tree

        bricks = list(bricks) if isinstance(bricks, (list, tuple)) else [bricks]
        if len(bricks) != len(adapters):
            raise ValueError("VolumeTracer.update: %d bricks given, the tracer has %d" % (len(bricks), len(adapters)))
        for i, (a, b) in enumerate(zip(adapters, bricks)):
            counts = np.asarray(b.counts, np.int64)
            offset = np.asarray(getattr(b, "offset", np.zeros(3)), np.int64)
            if (counts != a.counts).any() or (offset != a.offset).any():
                raise ValueError("VolumeTracer.update: brick %d has counts %s at offset %s, the tracer's has %s at %s (another bricking needs a new tracer)"
                                 % (i, counts.tolist(), offset.tolist(), a.counts.tolist(), a.offset.tolist()))
            want, got = getattr(a, "dtype_name", None), str(b.data.dtype).replace("torch.", "")
            if want is not None and got != want:
                raise ValueError("VolumeTracer.update: brick %d has %s data, the tracer's holds %s (another voxel type needs a new tracer)" % (i, got, want))
            if amr:
                same_subgrid_tree(getattr(a, "tree", []), getattr(b, "subgrids", None), "VolumeTracer.update: brick %d" % i)
        return bricks

    def update(self, bricks, amr=False):
        """The next time step: the same bricking of the new data (scenes.split_volume with the same split, or one VolumeData), pushed into
        the bricks in place (gvt_hip_volume_update_samples).  Transfer function, surfaces, lights, top level, queues and framebuffer stay.
        amr=True: the bricks may carry AMR subgrids (scenes.split_amr_volume with the same split) -- every brick's subgrid tree must be
        its adapter's (ValueError before the first brick changes), and a brick that has subgrids goes through gvt_hip_volume_update_amr
        with its level-0 data and all its subgrids' (the light grids go stale, the occluder grids do not).  Without it (the default) a
        brick that has subgrids is refused by the library, as ever."""
        bricks = self._same_bricking(self.adapters, bricks, amr)  # (all of them checked before the first one changes)
        self._grid_stale = True
        self._ao_stale = True
        for a, b in zip(self.adapters, bricks):
            if amr and getattr(b, "subgrids", None):
                a.update_amr(b.data, b.subgrids)
            else:
                a.update_samples(b.data)
            if getattr(b, "ghosts", None) is not None:  # the new step's face layers travel with its bricks
                a.set_ghosts(b.ghosts)
        return self

    def set_surfaces(self, isovalues=(), slices=(), opacity=1.0):
        """The volume's isosurfaces and slice planes (object space), on every brick."""
        self._grid_stale = True
        self._ao_stale = True
        self._surfaces = bool(len(isovalues) or len(slices))
        for a in self.adapters:
            a.set_surfaces(isovalues, slices, opacity)
        return self

    def set_transfer(self, tf):
        """Another transfer function on every brick (HipVolumeAdapter.set_transfer): the light grids and the AO grid are baked again."""
        self._grid_stale = True
        self._ao_stale = True
        for a in self.adapters:
            a.set_transfer(tf)
        return self

    def set_lights(self, lights, ka=0.4, kd=0.6):
        self._grid_stale = True
        self._occluder_stale = True
        for a in self.adapters:
            a.set_lights(lights, ka, kd)
        if isinstance(lights, np.ndarray) and lights.dtype.names:
            pos = np.asarray(lights["position"], np.float32).reshape(-1, 3)
        else:
            pos = np.asarray([l[0] for l in lights], np.float32).reshape(-1, 3)
        with np.errstate(all="ignore"):
            ln = np.sqrt((pos[:, 0] * pos[:, 0] + pos[:, 1] * pos[:, 1]) + pos[:, 2] * pos[:, 2])
        self._usable_lights = int(((ln > 0) & np.isfinite(ln)).sum())
        return self

    def set_shading(self, on=True):
        """Lit fog on every brick (HipVolumeAdapter.set_shading): the lights are set_lights'."""
        for a in self.adapters:
            a.set_shading(on)
        self._lit = bool(on)
        return self

    def set_gradient(self, kind):
        """The gradient kind on every brick (HipVolumeAdapter.set_gradient): "central" needs bricks that carry their ghosts."""
        for a in self.adapters:
            a.set_gradient(kind)
        return self

    def framebuffer(self, clamp=False):
        return self.fb.download(clamp)

    def stats(self):
        """The bricks' counters summed (they accumulate over frames).  fused=True adds fused, brick_visits and rays_deposited of the last
        frame, and where that frame was fused samples_marched / samples_gathered are ITS counts: the bricks' own did not move.
        fused_shaded=True adds features and, where the frame was fused, its crossings_rendered / samples_shaded likewise.
        fused_central=True adds nothing: features carries capi.FUSED_CENTRAL where a CENTRAL instantiation ran, and central_marches goes on
        counting the LOOP's per-brick launches only (it does not move in a fused frame).
        fused_amr=True adds amr_bricks (the bricks of the last frame that had subgrids; 0 unless an AMR instantiation ran), and where that
        frame was fused with capi.FUSED_AMR in features samples_refined is ITS count, like samples_marched; amr_marches goes on counting
        the LOOP's per-brick launches only.
        shadows=True: the last frame's gvt_hip_volume_shadow_stats in fused_shaded's form (the camera rays' counters; features carries
        capi.FUSED_AMR where shadow_amr let an AMR instantiation run -- refined samples are not counted there), and beside them
        shadowed, shadow_rays, shadow_brick_visits, shadow_crossings, shadow_samples_marched and shadow_samples_gathered.
        fog_shadows=True adds fog_samples_shadowed of the last frame, light_bakes (bakes so far) and light_grid_rays / _bytes / _ms of the
        last bake (0 before the first).
        mesh_shadows=True adds mesh_shadowed of the last frame, occluder_bakes (bakes so far) and occluder_rays / _rays_blocked / _bytes /
        _ms of the last bake (0 before the first).
        ao=True adds ao of the last frame (1: the AO kernel ran), ao_bakes (bakes so far) and ao_rays / _bytes / _ms of the last bake."""
        out = self._brick_stats()
        if self.ao:
            g = self.ao_stats or {"rays": 0, "bytes": 0, "ms": 0.0}
            out.update(ao_bakes=self.ao_bakes, ao_rays=g["rays"], ao_bytes=g["bytes"], ao_ms=g["ms"],
                       ao=0 if self.shadow_stats is None else self.shadow_stats.get("ao", 0))
        if self.mesh_shadows:
            g = self.occluder_stats or {"rays": 0, "rays_blocked": 0, "bytes": 0, "ms": 0.0}
            out.update(occluder_bakes=self.occluder_bakes, occluder_rays=g["rays"], occluder_rays_blocked=g["rays_blocked"], occluder_bytes=g["bytes"],
                       occluder_ms=g["ms"], mesh_shadowed=0 if self.shadow_stats is None else self.shadow_stats["mesh_shadowed"])
        if self.fog_shadows:
            g = self.light_grid_stats or {"rays": 0, "bytes": 0, "ms": 0.0}
            out.update(light_bakes=self.light_bakes, light_grid_rays=g["rays"], light_grid_bytes=g["bytes"], light_grid_ms=g["ms"],
                       fog_samples_shadowed=0 if self.shadow_stats is None else self.shadow_stats["fog_samples_shadowed"])
        if self.shadows and self.shadow_stats is not None:
            f = self.shadow_stats
            out.update({k: v for k, v in f.items() if k.startswith("shadow")})
            out.update(fused=f["fused"], brick_visits=f["brick_visits"], rays_deposited=f["rays_deposited"], features=f["features"])
            if f["fused"]:
                out.update(samples_marched=f["samples_marched"], samples_gathered=f["samples_gathered"], crossings_rendered=f["crossings_rendered"],
                           samples_shaded=f["samples_shaded"])
        elif self.fused and self.fused_stats is not None:
            f = self.fused_stats
            out.update(fused=f["fused"], brick_visits=f["brick_visits"], rays_deposited=f["rays_deposited"])
            if f["fused"]:
                out.update(samples_marched=f["samples_marched"], samples_gathered=f["samples_gathered"])
            if "features" in f:
                out.update(features=f["features"])
                if f["fused"]:
                    out.update(crossings_rendered=f["crossings_rendered"], samples_shaded=f["samples_shaded"])
            if "amr_bricks" in f:
                out.update(amr_bricks=f["amr_bricks"])
                if f["fused"] and f["features"] & capi.FUSED_AMR:
                    out.update(samples_refined=f["samples_refined"])
        return out

    def _brick_stats(self):
        infos = [a.info() for a in self.adapters]
        amr = [a.amr_info() for a in self.adapters]
        return {"samples_refined": sum(i["samples_refined"] for i in amr), "amr_marches": sum(i["amr_marches"] for i in amr),
                "adapter_calls": self.calls, "crossings_rendered": sum(a.crossings() for a in self.adapters), "samples_marched": sum(i["samples_marched"] for i in infos),
                "samples_gathered": sum(i["samples_gathered"] for i in infos), "samples_shaded": sum(a.shaded() for a in self.adapters),
                "central_marches": sum(a.central_marches() for a in self.adapters)}


def axis_aligned_matrix(m):
    """True if the 3x3 block of the column-major m[16] is a signed, scaled axis permutation (one non-zero entry per row and column, a
    diagonal block among them): the instance's axes stay parallel to the world's, so the world box of a brick IS the brick."""
    nz = np.asarray(m, np.float32).reshape(4, 4)[:3, :3] != 0
    return bool((nz.sum(axis=0) == 1).all() and (nz.sum(axis=1) == 1).all())


def _refuse_turned_bricks(m, n_bricks, who):
    """Several bricks under a matrix that turns or shears them are refused: the world boxes of neighbouring bricks then overlap, and the
    next-brick rule (vol_next: a brick is entered only if its exit lies strictly beyond the last brick's) skips a brick whose box ends
    inside its neighbour's -- samples would be lost without a word (include/gvt_hip.h, "bricks under a matrix").  One brick is marched
    under any affine matrix."""
    if n_bricks > 1 and not axis_aligned_matrix(m):
        raise ValueError("%s: %d bricks under a matrix that rotates or shears them: the world boxes of neighbouring bricks overlap and the "
                         "next-brick rule would skip bricks (samples lost); use one brick, or a matrix whose 3x3 block is a signed, scaled "
                         "axis permutation" % (who, n_bricks))


def _brick_boxes(bricks, m):
    """The world boxes of bricks under the instance matrix m, as VolumeTracer places them."""
    from .scenes import instance_bbox

    boxes = []
    for b in bricks:
        lo = b.lo if hasattr(b, "lo") else np.asarray(b.origin, np.float32)
        hi = b.hi if hasattr(b, "hi") else (np.asarray(b.origin, np.float32) + (b.counts - 1).astype(np.float32) * np.asarray(b.spacing, np.float32)).astype(np.float32)
        boxes.append(instance_bbox(m, lo, hi))
    return np.array([b[0] for b in boxes], np.float32), np.array([b[1] for b in boxes], np.float32)


class HipVolumeBackend:
    """One rank's device state under the Domain scheduler over the bricks of one volume instance, with HipBackend's method names (the
    loops of DomainTracer drive it).  Every brick has a top-level box and a queue here; only the owned ones (owned[i], None: all) have
    an adapter.  The queue of a brick this rank does not own is its outgoing list to that brick's owner.  A ray that ends on this rank,
    OPAQUE or EXTERNAL, deposits into this rank's framebuffer.  bricks, m, sampling_rate, skip, native, amr_shaded: VolumeTracer's."""

    def __init__(self, bricks, camera, tf, m=None, sampling_rate=1.0, skip=True, native=False, owned=None, amr_shaded=False):
        from .adapter import HipVolumeAdapter
        from .scenes import instance_matrices, mat_translate_scale

        bricks = list(bricks) if isinstance(bricks, (list, tuple)) else [bricks]
        self.camera = camera
        self.m = capi.f32(mat_translate_scale((0, 0, 0), (1, 1, 1)) if m is None else m, 16)
        _refuse_turned_bricks(self.m, len(bricks), "HipVolumeBackend")
        self.minv = instance_matrices(self.m)[0]
        self.n_inst = len(bricks)
        self.owned = [True] * self.n_inst if owned is None else [bool(o) for o in owned]
        self.adapters = [HipVolumeAdapter(b, sampling_rate, skip, native, amr_shaded) if self.owned[i] else None for i, b in enumerate(bricks)]
        for a in self.local_adapters():
            a.set_transfer(tf)
        self.inst_lo, self.inst_hi = _brick_boxes(bricks, self.m)
        self.top = TopLevel(self.inst_lo, self.inst_hi)
        self.queues = [RayQueue() for _ in range(self.n_inst)]
        self.fb = FrameBuffer(camera.width, camera.height)
        self.calls = 0

    def local_adapters(self):
        return [a for a in self.adapters if a is not None]

    def _arr(self, xs):
        import ctypes as C

        return (C.c_void_p * max(1, len(xs)))(*[x.h for x in xs])

    # ---- frame steps
    def begin_frame(self):
        self.fb.clear()
        for q in self.queues:
            q.clear()
        self.calls = 0

    def generate_and_filter(self, keep_mask=None):
        """shuffleDropRays (DomainTracer.h:148-183): the camera's rays into the kept bricks they enter first (gvt_hip_volume_camera_filter)."""
        import ctypes as C

        from .adapter import camera_pod

        pod = camera_pod(self.camera)
        km = None if keep_mask is None else np.ascontiguousarray(keep_mask, dtype=np.uint8)
        capi.check(capi.load().gvt_hip_volume_camera_filter(self.top.h, C.byref(pod), self._arr(self.queues), capi.ptr(km)), "gvt_hip_volume_camera_filter")

    def queue_sizes(self):
        return [len(q) for q in self.queues]

    def trace_and_shuffle(self, inst):
        """Adapter::trace on brick inst's queue, then shuffleRays(moved_rays, inst): onward rays into the next bricks' queues, local or
        not; rays that end deposit here."""
        self.adapters[inst].march_queue(self.queues[inst], self.minv)
        self.calls += 1
        capi.check(capi.load().gvt_hip_shuffle_volume(self.top.h, self.queues[inst].h, inst, self._arr(self.queues), self.fb.h), "gvt_hip_shuffle_volume")

    # ---- exchange (the 80-byte wire image, all the queues of a message in one launch)
    def export_wire(self, insts, torch, device):
        """Concatenate the queues `insts` into one wire tensor [n, 20] f32 and clear them (gvt_hip_queues_export_wire)."""
        from .adapter import queues_export_wire

        total = sum(len(self.queues[i]) for i in insts)
        buf = torch.empty((total, 20), dtype=torch.float32, device=device)
        if insts:  # (one call: a top level holds at most capi.WIRE_MAX_QUEUES bricks)
            queues_export_wire([self.queues[i] for i in insts], buf.data_ptr(), total)
        return buf

    def append_wire(self, insts, buf, off, counts):
        """Consecutive runs of counts[k] rays of the wire tensor, from ray `off` on, appended to the queues insts[k], their state kept
        (gvt_hip_queues_append_wire)."""
        from .adapter import queues_append_wire

        if insts:
            queues_append_wire([self.queues[i] for i in insts], buf.data_ptr() + off * 80, counts)

    def fb_tensor(self, torch, device):
        """torch view of the framebuffer's device memory (un-clamped sums) for the composite."""
        cam = self.camera

        class _View:
            __cuda_array_interface__ = {"shape": (cam.height * cam.width * 4,), "typestr": "<f4", "data": (self.fb.device_ptr(), False), "version": 2}

        return torch.as_tensor(_View(), device=device)

    def framebuffer(self, clamp=False):
        return self.fb.download(clamp)

    def sync(self):
        capi.synchronize()

    # ---- the volume's controls, on the owned bricks (VolumeTracer's)
    def update(self, bricks):
        """The next time step: the same bricking of the new data (all bricks given; the owned ones are updated in place)."""
        bricks = list(bricks) if isinstance(bricks, (list, tuple)) else [bricks]
        if len(bricks) != self.n_inst:
            raise ValueError("HipVolumeBackend.update: %d bricks given, the volume has %d" % (len(bricks), self.n_inst))
        mine = VolumeTracer._same_bricking(self.local_adapters(), [b for i, b in enumerate(bricks) if self.owned[i]])
        for a, b in zip(self.local_adapters(), mine):
            a.update_samples(b.data)
            if getattr(b, "ghosts", None) is not None:
                a.set_ghosts(b.ghosts)
        return self

    def set_surfaces(self, isovalues=(), slices=(), opacity=1.0):
        for a in self.local_adapters():
            a.set_surfaces(isovalues, slices, opacity)
        return self

    def set_lights(self, lights, ka=0.4, kd=0.6):
        for a in self.local_adapters():
            a.set_lights(lights, ka, kd)
        return self

    def set_shading(self, on=True):
        for a in self.local_adapters():
            a.set_shading(on)
        return self

    def set_gradient(self, kind):
        for a in self.local_adapters():
            a.set_gradient(kind)
        return self

    def stats(self):
        """VolumeTracer.stats() summed over the owned bricks (the counters run from the adapters' creation)."""
        ads = self.local_adapters()
        infos = [a.info() for a in ads]
        amr = [a.amr_info() for a in ads]
        return {"samples_refined": sum(i["samples_refined"] for i in amr), "amr_marches": sum(i["amr_marches"] for i in amr),
                "adapter_calls": self.calls, "crossings_rendered": sum(a.crossings() for a in ads), "samples_marched": sum(i["samples_marched"] for i in infos),
                "samples_gathered": sum(i["samples_gathered"] for i in infos), "samples_shaded": sum(a.shaded() for a in ads),
                "central_marches": sum(a.central_marches() for a in ads)}


class VolumeDomainTracer(DomainTracer):
    """Tracer<DomainScheduler> over the bricks of one volume spread over the ranks of a job: DomainTracer's BSP and overlapped loops
    and its composite, over a HipVolumeBackend (or a backend with its method names: tests/volume_domain_backend.py).  owner[i] = the
    rank that holds brick i.

    With one sample per pixel rank 0's composited framebuffer equals VolumeTracer(...).frame()'s in every bit, for every owner map, world
    size and both loops (include/gvt_hip.h, "volume domains across ranks"): a pixel has one ray, so one deposit, on the rank where the
    ray ends; the sum-reduce and the rows_only rectangles add it to zeros."""

    def __init__(self, bricks, owner, camera, tf, dist, torch, comm_device, m=None, sampling_rate=1.0, skip=True, native=False, backend=None, overlap=False,
                 shadows=False, fog_shadows=False, mesh_shadows=False, ao=False):
        from types import SimpleNamespace

        if shadows:  # (a shadow ray is marched to its end by the lane that needs it: a rank does not hold the foreign bricks it crosses)
            raise ValueError("VolumeDomainTracer: shadows need every brick of the volume on one device (VolumeTracer(shadows=True))")
        if fog_shadows:  # (nor the bricks a vertex's ray crosses)
            raise ValueError("VolumeDomainTracer: fog_shadows need every brick of the volume on one device (VolumeTracer(shadows=True, fog_shadows=True))")
        if mesh_shadows:  # (the mesh-shadowed frame is the fog-shadowed frame with one more change)
            raise ValueError("VolumeDomainTracer: mesh_shadows need every brick of the volume on one device (VolumeTracer(shadows=True, fog_shadows=True, mesh_shadows=True))")
        if ao:  # (the AO frame is the fog-shadowed frame with one more change, and a vertex's AO rays cross foreign bricks)
            raise ValueError("VolumeDomainTracer: ao needs every brick of the volume on one device (VolumeTracer(shadows=True, fog_shadows=True, ao=True))")

        bricks = list(bricks) if isinstance(bricks, (list, tuple)) else [bricks]
        if m is not None:  # (whatever backend marches the bricks: the next-brick rule is the same)
            _refuse_turned_bricks(m, len(bricks), "VolumeDomainTracer")
        self.overlap = overlap
        self.scene = SimpleNamespace(camera=camera)  # (what the shared loops and the composite read of a scene)
        self.camera = camera
        self.owner = list(owner)
        self.dist, self.torch, self.dev = dist, torch, comm_device
        self.on_cuda = torch.device(comm_device).type == "cuda"
        self.rank = dist.get_rank() if dist.is_initialized() else 0
        self.world = dist.get_world_size() if dist.is_initialized() else 1
        self.owned = [o == self.rank for o in self.owner]
        self.backend = backend or HipVolumeBackend(bricks, camera, tf, m, sampling_rate, skip, native, self.owned)
        self.rounds = 0
        self.rays_sent = 0
        self.adapter_calls = 0

    def _unpack(self, buf, counts_p):
        """A peer's payload into the owned bricks' queues: one batched append instead of one per brick."""
        insts = [i for i in range(len(self.owner)) if self.owned[i] and counts_p[i]]
        self.backend.append_wire(insts, buf, 0, [int(counts_p[i]) for i in insts])

    def composite(self, download=True, rows_only=True, clamp=False):
        """DomainTracer.composite; the image comes back un-clamped (premultiplied colour, opacity) unless clamp."""
        super().composite(download=False, rows_only=rows_only)
        if self.rank != 0 or not download:
            return None
        cam = self.camera
        return self.backend.framebuffer(clamp).reshape(cam.height, cam.width, 4)

    def update(self, bricks):
        self.backend.update(bricks)
        return self

    def set_surfaces(self, isovalues=(), slices=(), opacity=1.0):
        self.backend.set_surfaces(isovalues, slices, opacity)
        return self

    def set_lights(self, lights, ka=0.4, kd=0.6):
        self.backend.set_lights(lights, ka, kd)
        return self

    def set_shading(self, on=True):
        self.backend.set_shading(on)
        return self

    def set_gradient(self, kind):
        self.backend.set_gradient(kind)
        return self

    def stats(self):
        """This rank's share: VolumeTracer.stats() over the bricks it owns, and the loop's own counts."""
        st = dict(self.backend.stats())
        st.update(adapter_calls=self.adapter_calls, rounds=self.rounds, rays_sent=self.rays_sent)
        return st


class MixedTracer:
    """A scene that holds geometry AND a volume: the meshes of `scene` inside the bricks of one volume instance.  It owns a NativeTracer
    (the mesh frame, as it is on its own), a DepthPlane and a VolumeTracer; frame() renders the mesh frame, the depth plane of the
    scene (a second closest-hit pass over the primaries), the volume frame clipped at it, and composites the volume over the meshes
    (gvt_hip_fb_composite_over; the result is in the volume tracer's framebuffer).  The reference has no such path: shuffleRays
    takes either the mesh or the volume branch.  `camera` becomes the scene's (one sample per pixel).
    mesh_shadows (with shadows and fog_shadows): the meshes cast shadows into the volume (VolumeTracer's mesh_shadows).  frame() bakes the
    occluder grids before the first volume frame that needs them and again after update_scene() and set_lights(); rebake_occluders() is
    explicit.  set_camera(), update() and set_surfaces() do not bake.
    shadow_amr (with shadows): VolumeTracer's -- the shadowed frames and both bakes take bricks with AMR subgrids.
    ao, ao_dirs, ao_radius, ao_bias: VolumeTracer's -- the volume frame is the AO frame (meshes do not occlude ambient light)."""

    def __init__(self, scene, bricks, camera, tf, m=None, sampling_rate=1.0, skip=True, native=False, normal_mode=NORMALS_FLAT, fused=False, fused_shaded=False,
                 shadows=False, shadow_bias=2, fog_shadows=False, fog_bias=1, mesh_shadows=False, fused_central=False, amr_shaded=False, fused_amr=False,
                 shadow_amr=False, ao=False, ao_dirs=16, ao_radius=None, ao_bias=1):
        from dataclasses import replace

        from .adapter import DepthPlane

        if camera.samples != 1:
            raise ValueError("MixedTracer: the depth plane holds one ray per pixel (camera.samples must be 1)")
        if m is not None:  # before the mesh tracer and the depth plane are made
            _refuse_turned_bricks(m, len(bricks) if isinstance(bricks, (list, tuple)) else 1, "MixedTracer")
        self.scene = replace(scene, camera=camera)
        self.camera = camera
        self.mesh = NativeTracer(self.scene, normal_mode)
        self.depth = DepthPlane(camera.width, camera.height)
        self.volume = VolumeTracer(bricks, camera, tf, m=m, sampling_rate=sampling_rate, skip=skip, native=native, fused=fused,
                                   fused_shaded=fused_shaded, shadows=shadows, shadow_bias=shadow_bias, fog_shadows=fog_shadows, fog_bias=fog_bias,
                                   mesh_shadows=mesh_shadows, fused_central=fused_central, amr_shaded=amr_shaded, fused_amr=fused_amr,
                                   shadow_amr=shadow_amr, ao=ao, ao_dirs=ao_dirs, ao_radius=ao_radius, ao_bias=ao_bias)
        # (shadow_amr: the shadowed frames and the bakes take AMR bricks too, VolumeTracer's; amr_shaded: AMR bricks take surfaces and lit fog, in the clipped frame too; fused_amr: AMR bricks in the fused clipped frame too; fused: its clipped frame in one launch; fused_shaded: with surfaces or lit fog too; fused_central: with CENTRAL bricks too; shadows: the volume's surfaces shadowed by the
        # volume; fog_shadows: its lit fog too, from the baked light grids; mesh_shadows: both shadowed by the meshes as well, from the baked
        # occluder grids -- without it the meshes cast no shadow into the volume)
        self.mesh_shadows = bool(mesh_shadows)
        if self.mesh_shadows:
            self.volume._occluder_source = self.mesh.backend  # (frame() bakes from it once the frame needs a grid)

    def rebake_occluders(self):
        """The occluder grids of the scene as it is now (VolumeTracer.bake_occluders over the mesh tracer's backend)."""
        self.volume.bake_occluders(self.mesh.backend)
        return self

    def frame(self):
        self.mesh()
        self.depth.render(self.mesh.backend, self.camera)
        self.volume.frame(self.depth)
        self.volume.fb.composite_over(self.mesh.backend.fb, self.depth)
        return self

    def framebuffer(self, clamp=False):
        """The composite: (H, W, 4), colour premultiplied, alpha = the volume's opacity plus what it leaves of the geometry's coverage."""
        return self.volume.framebuffer(clamp)

    def mesh_framebuffer(self, clamp=True):
        return self.mesh.backend.framebuffer(clamp)

    # the volume's controls
    def update(self, bricks, amr=False):
        """VolumeTracer.update: amr=True takes bricks with AMR subgrids in place (the occluder grids stay current)."""
        self.volume.update(bricks, amr)
        return self

    def set_surfaces(self, isovalues=(), slices=(), opacity=1.0):
        self.volume.set_surfaces(isovalues, slices, opacity)
        return self

    def set_lights(self, lights, ka=0.4, kd=0.6):
        self.volume.set_lights(lights, ka, kd)
        return self

    def set_shading(self, on=True):
        self.volume.set_shading(on)
        return self

    def set_gradient(self, kind):
        self.volume.set_gradient(kind)
        return self

    # the scene's
    def set_camera(self, cam):
        if cam.samples != 1:
            raise ValueError("MixedTracer: the depth plane holds one ray per pixel (camera.samples must be 1)")
        self.mesh.set_camera(cam)
        self.camera = self.volume.camera = self.scene.camera = self.mesh.backend.scene.camera = cam
        return self

    def update_scene(self, scene):
        if scene.camera.samples != 1:
            raise ValueError("MixedTracer: the depth plane holds one ray per pixel (camera.samples must be 1)")
        self.mesh.update_scene(scene)
        self.scene = scene
        self.volume._occluder_stale = True  # (the library cannot see a mesh move)
        self.camera = self.volume.camera = scene.camera
        return self

    def close(self):
        self.mesh.close()
        self.depth.close()
