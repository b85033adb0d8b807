// depth.hip -- geometry inside a volume: what the mesh side hands to the volume side, and the composite of the two images.
//   gvt_hip_depth_*             a depth plane: t along every pixel's camera ray, +Inf = nothing there
//   gvt_hip_depth_render        the plane of a scene: one closest-hit launch per instance over the camera's list (launch_closest, trace.hip),
//                               each followed by k_depth_min
//   gvt_hip_fb_composite_over   a volume frame OVER a mesh frame, coverage from the depth plane
// The reference renders a scene through either its mesh or its volume branch (shuffleRays, TracerBase.h:325-414, by adapter type) and has
// no counterpart; the contract is stated in include/gvt_hip.h and restated in tests/volume_clip_checker.py.
#include "gvt_internal.h"

namespace {

__global__ __launch_bounds__(256) void k_depth_fill(float *__restrict__ t, unsigned n, float v) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i < n) t[i] = v;
}

// One lane per ray of the camera's list: a pixel has one ray, so one writer; the stream orders the instances.
__global__ __launch_bounds__(256) void k_depth_min(const float4 *__restrict__ p3, const gvt_hip_hit *__restrict__ hits, unsigned n, float *__restrict__ t, unsigned n_pix) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const unsigned id = (unsigned)__float_as_int(p3[i].x);
  if (id >= n_pix) return;
  const gvt_hip_hit h = hits[i];
  t[id] = fminf(t[id], h.prim >= 0 ? h.t : INFINITY);
}

// front OVER back (gvt_hip.h); the library is compiled without contraction, so every step below is one float32 operation
__global__ __launch_bounds__(256) void k_composite_over(float4 *__restrict__ front, const float4 *__restrict__ back, const float *__restrict__ depth, unsigned n) {
  const unsigned p = blockIdx.x * 256u + threadIdx.x;
  if (p >= n) return;
  float4 f = front[p];
  const float4 b = back[p];
  const float k = 1.f - f.w;
  const float cov = depth ? (depth[p] < INFINITY ? 1.f : 0.f) : fminf(b.w, 1.f);
  f.x = f.x + k * fminf(b.x, 1.f);
  f.y = f.y + k * fminf(b.y, 1.f);
  f.z = f.z + k * fminf(b.z, 1.f);
  f.w = f.w + k * cov;
  front[p] = f;
}

inline unsigned blocks_of(size_t n) { return (unsigned)((n + 255) / 256); }

} // namespace

extern "C" gvt_hip_depth *gvt_hip_depth_create(int w, int h) {
  if (ensure_init()) return nullptr;
  if (w <= 0 || h <= 0) { set_error("depth_create: bad size %d x %d", w, h); return nullptr; }
  gvt_hip_depth *D = new gvt_hip_depth();
  D->w = w; D->h = h;
  if (hipMalloc((void **)&D->d_t, sizeof(float) * (size_t)w * h) != hipSuccess) { set_error("depth_create: hipMalloc failed"); delete D; return nullptr; }
  if (gvt_hip_depth_clear(D)) { gvt_hip_depth_destroy(D); return nullptr; }
  return D;
}

extern "C" void gvt_hip_depth_destroy(gvt_hip_depth *D) {
  if (!D) return;
  if (gctx().ready) hipStreamSynchronize(gctx().stream);
  hipFree(D->d_t);
  delete D;
}

extern "C" int gvt_hip_depth_clear(gvt_hip_depth *D) {
  if (!D) { set_error("depth_clear: null"); return GVT_HIP_ERR_INVALID; }
  const size_t n = (size_t)D->w * D->h;
  k_depth_fill<<<blocks_of(n), 256, 0, gctx().stream>>>(D->d_t, (unsigned)n, INFINITY);
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int gvt_hip_depth_upload(gvt_hip_depth *D, const float *t, uint32_t flags) {
  if (!D || !t) { set_error("depth_upload: null argument"); return GVT_HIP_ERR_INVALID; }
  if (flags & ~GVT_HIP_UPDATE_DEVICE) { set_error("depth_upload: unknown flags 0x%x", flags); return GVT_HIP_ERR_INVALID; }
  hipStream_t st = gctx().stream;
  const size_t bytes = sizeof(float) * (size_t)D->w * D->h;
  if (flags & GVT_HIP_UPDATE_DEVICE) { HIPCHK(hipMemcpyAsync(D->d_t, t, bytes, hipMemcpyDeviceToDevice, st)); return 0; }
  HIPCHK(hipMemcpyAsync(D->d_t, t, bytes, hipMemcpyHostToDevice, st));
  HIPCHK(hipStreamSynchronize(st)); // (the copy reads the caller's host buffer)
  return 0;
}

extern "C" int gvt_hip_depth_download(gvt_hip_depth *D, float *t) {
  if (!D || !t) { set_error("depth_download: null argument"); return GVT_HIP_ERR_INVALID; }
  hipStream_t st = gctx().stream;
  HIPCHK(hipMemcpyAsync(t, D->d_t, sizeof(float) * (size_t)D->w * D->h, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return 0;
}

extern "C" int gvt_hip_depth_render(gvt_hip_depth *D, gvt_hip_mesh *const *meshes, const float *m, const float *minv, size_t n_inst, const gvt_hip_camera *cam) {
  if (ensure_init()) return GVT_HIP_ERR_NODEVICE;
  (void)m; // (a trace needs minv only)
  if (!D || !cam || (n_inst && (!meshes || !minv))) { set_error("depth_render: null argument"); return GVT_HIP_ERR_INVALID; }
  for (size_t i = 0; i < n_inst; i++)
    if (!meshes[i]) { set_error("depth_render: instance %zu has no mesh", i); return GVT_HIP_ERR_INVALID; }
  if (cam->samples != 1 || cam->width != D->w || cam->height != D->h) {
    set_error("depth_render: a %d x %d plane for a %d x %d film of %d x %d samples per pixel (one is needed)", D->w, D->h, cam->width, cam->height, cam->samples, cam->samples);
    return GVT_HIP_ERR_INVALID;
  }
  Ctx &C = gctx();
  if (!staging_queues(C)) return GVT_HIP_ERR_DEVICE;
  gvt_hip_queue *q = C.abi_qout; // (a staging list of the context: the camera's rays, origins at the eye)
  const size_t n = (size_t)D->w * D->h;
  int rc;
  if ((rc = gvt_hip_depth_clear(D))) return rc;
  if ((rc = gvt_hip_camera_generate_tiled(q, cam->eye, cam->focus, cam->up, cam->fov, cam->width, cam->height, 1, 0, cam->jitter_window_size, 8))) return rc;
  gvt_hip_hit *d_hits = n_inst ? (gvt_hip_hit *)scratch_get(SCR_GENERAL, sizeof(gvt_hip_hit) * n) : nullptr;
  if (n_inst && !d_hits) return GVT_HIP_ERR_DEVICE;
  const RayPlanes P = make_planes(q->d_planes, q->cap);
  for (size_t i = 0; i < n_inst; i++) {
    Mat4 M;
    for (int k = 0; k < 16; k++) M.m[k] = minv[16 * i + k];
    if ((rc = launch_closest(meshes[i], P, nullptr, n, true, M, GVT_RAY_EPSILON, d_hits))) return rc;
    k_depth_min<<<blocks_of(n), 256, 0, C.stream>>>(P.p3, d_hits, (unsigned)n, D->d_t, (unsigned)n);
    HIPCHK(hipGetLastError());
  }
  if (n_inst && (rc = trav_overflow_fetch_async())) return rc;
  if ((rc = gvt_hip_queue_clear(q))) return rc;
  HIPCHK(hipStreamSynchronize(C.stream));
  return n_inst ? trav_overflow_result() : 0;
}

extern "C" int gvt_hip_fb_composite_over(gvt_hip_fb *front, const gvt_hip_fb *back, const gvt_hip_depth *depth) {
  if (ensure_init()) return GVT_HIP_ERR_NODEVICE;
  if (!front || !back || front == back) { set_error("fb_composite_over: null framebuffer, or one framebuffer over itself"); return GVT_HIP_ERR_INVALID; }
  if (front->w != back->w || front->h != back->h || (depth && (depth->w != front->w || depth->h != front->h))) {
    set_error("fb_composite_over: sizes differ (front %d x %d, back %d x %d%s)", front->w, front->h, back->w, back->h, depth ? ", or the depth plane's" : "");
    return GVT_HIP_ERR_INVALID;
  }
  const size_t n = (size_t)front->w * front->h;
  k_composite_over<<<blocks_of(n), 256, 0, gctx().stream>>>((float4 *)front->d_rgba, (const float4 *)back->d_rgba, depth ? depth->d_t : nullptr, (unsigned)n);
  HIPCHK(hipGetLastError());
  return 0;
}
