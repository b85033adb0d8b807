/*
 * gvt_hip.h -- C ABI of the MI355X (gfx950) engine adapter for GraviT: gvt::render::adapter::hip.
 *
 * This is the drop-in boundary.  Every entry point is what a GraviT-side binding for the
 * adapter path would call; the reference interface each one replaces is cited as file:line
 * relative to the GraviT source tree.  Plain pointers and sizes only; no C++/torch types.
 *
 * Conventions
 *   - Rays are the reference's 80-byte `gvt::render::actor::Ray` image (actor/Ray.h:68-96),
 *     16-byte aligned, exactly what Ray::pack() puts on the wire (Ray.h:161-174).
 *   - Materials are the reference's 92-byte `Material` POD (primitives/Material.h:59-90).
 *   - Matrices are glm column-major: m[16], minv[16], normi[9] (api.cpp:303-308).
 *   - Lights are 64-byte tagged PODs (the CPU reference uses virtual classes, scene/Light.h:46-104;
 *     POD precedent adapter/optix/Light.cuh:44-112).
 *   - Triangles are 0-based vertex triples (what the adapters read through std::get<>,
 *     EmbreeMeshAdapter.cpp:152-155).
 *   - Every function returning int returns 0 on success and a negative code on error; the
 *     message is available from gvt_hip_last_error().  Nothing calls exit() (the reference's
 *     Embree error handler does, EmbreeMeshAdapter.cpp:90-123).
 *   - All work of a context is issued on that context's HIP stream (gvt_hip_set_stream); a process has a default context and may
 *     create more (gvt_hip_ctx_create), one per thread; calls on one mesh/queue are serialised by the caller, as the reference's
 *     schedulers do (ImageTracer.h:241-248).
 */
#ifndef GVT_HIP_H
#define GVT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI revision of this header: bumped whenever an entry point changes meaning or an out-struct (gvt_hip_mesh_info, gvt_hip_stats, gvt_hip_frame_stats)
 * changes size.  A binding compares it with gvt_hip_abi_version() of the library it loaded before its first call (gravit_amd/capi.py, HipMeshAdapter.cpp do):
 * a caller built against another revision would have out-structs written past their end or flags read with another meaning, silently.
 *   6: gvt_hip_queue_append keeps its round-4 meaning (4th argument: the source is device memory); the flag word lives in gvt_hip_queue_append_flags */
#define GVT_HIP_ABI_VERSION 6
int gvt_hip_abi_version(void); /* GVT_HIP_ABI_VERSION the library was built from; no device access */

#define GVT_HIP_OK 0
#define GVT_HIP_ERR_INVALID (-1)  /* bad argument */
#define GVT_HIP_ERR_DEVICE (-2)   /* HIP runtime error */
#define GVT_HIP_ERR_CAPACITY (-3) /* output buffer / queue too small; nothing lost, see call */
#define GVT_HIP_ERR_NODEVICE (-4) /* no gfx950 device visible */
#define GVT_HIP_ERR_TIMEOUT (-5)  /* ray exchange: a peer did not answer within the communicator's deadline; the communicator is dead */
#define GVT_HIP_ERR_PEER (-6)     /* ray exchange: another rank reported an error in its announce; every rank leaves the frame with this */

#define GVT_HIP_NORMALS_FLAT 0   /* EmbreeMeshAdapter.cpp:75,520-522 (FLAT_SHADING) */
#define GVT_HIP_NORMALS_SMOOTH 1 /* EmbreeMeshAdapter.cpp:505-518, EmbreeStreamMeshAdapter.cpp:708, OptixMeshAdapter.cu:298 */

typedef struct gvt_hip_ray { /* actor/Ray.h:68-96 */
  float origin[3];
  float t_min;
  float direction[3];
  float t_max;
  float color[3];
  float t;
  int32_t id;
  int32_t depth;
  float w;
  int32_t type; /* 0 PRIMARY, 1 SHADOW, 2 SECONDARY */
  float pad[4];
} gvt_hip_ray;

typedef struct gvt_hip_material { /* primitives/Material.h:59-90 */
  int32_t type;                 /* 0 LAMBERT, 1 PHONG, 2 BLINN, 3 EMBREE_MATERIAL_METAL, 4 _VELVET, 5 _MATTE (Material.h:50-57) */
  float ka[3], ks[3], kd[3];
  float alpha;
  float eta[3], k[3];
  float roughness;
  float horizonScatteringColor[3];
  float backScattering, horizonScatteringFallOff;
} gvt_hip_material;

#define GVT_HIP_LIGHT_POINT 0
#define GVT_HIP_LIGHT_AREA 1
#define GVT_HIP_LIGHT_AMBIENT 2
typedef struct gvt_hip_light { /* scene/Light.h:46-104 flattened */
  int32_t type;
  float position[3];
  float color[3];
  float normal[3];
  float width, height;
  float pad[4];
} gvt_hip_light;

typedef struct gvt_hip_hit {
  float t;
  int32_t prim; /* -1 = miss */
  float u, v;
} gvt_hip_hit;

typedef struct gvt_hip_mesh gvt_hip_mesh;   /* one adapter instance: replaces EmbreeMeshAdapter */
typedef struct gvt_hip_queue gvt_hip_queue; /* device-resident RayVector */
typedef struct gvt_hip_top gvt_hip_top;     /* top-level instance set (accel/BVH.h) */
typedef struct gvt_hip_fb gvt_hip_fb;       /* float RGBA framebuffer (IceTComposite) */

/* ---- process / device ---- */
typedef struct gvt_hip_ctx gvt_hip_ctx;       /* a stream + scratch arenas + counters + statistics + knobs */
int gvt_hip_init(int device);                 /* select device, create the process's default context */
/* Additional contexts, e.g. one per rank when several ranks of a scheduler share a process (the reference runs several MPI ranks per
 * node): every API call runs on the calling thread's current context (NULL = the default one).  Device objects (meshes, queues,
 * framebuffers, top-level sets) may be used from any context of their device, by one context at a time. */
gvt_hip_ctx *gvt_hip_ctx_create(int device);
int gvt_hip_ctx_make_current(gvt_hip_ctx *);  /* for the calling thread; also selects the context's device (hipSetDevice) */
void gvt_hip_ctx_destroy(gvt_hip_ctx *);
int gvt_hip_set_stream(void *hip_stream);     /* issue all later work on this hipStream_t (NULL = own stream) */
int gvt_hip_synchronize(void);
const char *gvt_hip_last_error(void);

/* ---- adapter construction: EmbreeMeshAdapter::EmbreeMeshAdapter (EmbreeMeshAdapter.cpp:125-162) ----
 * Copies everything (no borrowed pointers), generates vertex normals when vnormals==NULL
 * (Mesh::generateNormals, Mesh.cpp:116-154) and builds the LBVH on the device. */
gvt_hip_mesh *gvt_hip_mesh_create(const float *verts, size_t nV, const int32_t *tris, size_t nT,
                                  const float *vnormals /* nV*3 or NULL */, const float *vcolors /* nV*3 or NULL */,
                                  const gvt_hip_material *materials, size_t nMat,
                                  const int32_t *face_mat /* nT or NULL, -1 = none */,
                                  const gvt_hip_material *mesh_mat /* Mesh::mat; NULL = Material() */);
void gvt_hip_mesh_destroy(gvt_hip_mesh *);

typedef struct gvt_hip_mesh_info {
  uint64_t n_tris, n_verts, n_nodes, n_leaves;
  float bbox_lo[3], bbox_hi[3];
  float build_ms; /* device time of the LBVH build */
  uint32_t max_leaf;
  uint32_t packet;   /* 1: the builder found the mesh packet-friendly -- coherent lists (camera rays in tile order and their shadow rays) are traversed a
                        packet of 64 per wave (k_packet); 0: one lane per ray.  The reference picks its packet width per build too (EmbreeMeshAdapter.cpp:50-74) */
  uint64_t bytes_nodes, bytes_tris;
  float sah_inner;   /* the statistic behind `packet`: sum over the inner nodes of area(node) / area(root) = inner nodes a random line through the mesh's
                        box pierces.  A surface stays at a few dozen whatever its triangle count, a volume-filling soup grows with N^(1/3) */
  float pad;
} gvt_hip_mesh_info;
int gvt_hip_mesh_get_info(const gvt_hip_mesh *, gvt_hip_mesh_info *);
/* vertex normals in use (device -> host copy), nV*3 floats */
int gvt_hip_mesh_get_normals(const gvt_hip_mesh *, float *out);

/* ---- animated meshes: in-place refit ----
 * New vertex positions for a mesh whose topology stays (triangles, materials and colours are kept).  nV must be the mesh's vertex count.
 * Afterwards the mesh behaves exactly like gvt_hip_mesh_create on the new vertices -- the same hits, shading inputs and mesh_info box --
 * but keeps its tree's topology and node counts: the node boxes are refitted, not rebuilt.  Every device pointer the mesh holds stays
 * valid, so tracers and contexts that borrow it keep working; the caller serialises the update against frames that use the mesh.
 * vnormals == NULL: regenerated (on the device, bit-identical to the host generation at create).  The call is ordered on the calling
 * context's stream and returns when it is done.  ms_out (may be NULL): device time of the update after the upload. */
#define GVT_HIP_UPDATE_DEVICE 1u /* verts / vnormals are device pointers on the mesh's device (in situ: no host round trip) */
int gvt_hip_mesh_update_vertices(gvt_hip_mesh *, const float *verts /* nV*3 */, size_t nV, const float *vnormals /* nV*3 or NULL */,
                                 uint32_t flags, float *ms_out);

/* ---- Adapter::trace (Adapter.h:82-84; EmbreeMeshAdapter.cpp:625-660) ----
 * rays[begin,end) are traced (end==0 -> n_rays, EmbreeMeshAdapter.cpp:642) and updated in place like the
 * reference's rayList (t, and origin/direction/w/depth/type on a bounce).  rays_out receives every
 * PRIMARY/SECONDARY ray that missed and every un-occluded SHADOW ray (moved_rays); order unspecified.
 * If cap is too small: returns GVT_HIP_ERR_CAPACITY, *n_out = needed count, rays_out untouched.
 * m / minv / normi: any affine instance matrix (rotation, non-uniform scale, shear, mirroring) and what api.cpp:307-308 makes of it.
 * Projective matrices are not supported: the bottom row (m[3], m[7], m[11], m[15]) is taken to be 0 0 0 1 and overwritten. */
int gvt_hip_trace(gvt_hip_mesh *, gvt_hip_ray *rays, size_t n_rays, size_t begin, size_t end, gvt_hip_ray *rays_out,
                  size_t cap, size_t *n_out, const float m[16], const float minv[16], const float normi[9],
                  const gvt_hip_light *lights, size_t n_lights, int normal_mode, uint32_t seed);
/* The same call with flags.  GVT_HIP_TRACE_NO_WRITEBACK: `rays` is only read.  Both of the reference's schedulers clear the traced
 * queue right after the call (ImageTracer.h:248, DomainTracer.h:316), so the rayList's in-place update is never observed there;
 * skipping it saves a third of the call's PCIe traffic (80 B per ray back to the host). */
#define GVT_HIP_TRACE_NO_WRITEBACK 1u
int gvt_hip_trace_ex(gvt_hip_mesh *, gvt_hip_ray *rays, size_t n_rays, size_t begin, size_t end, gvt_hip_ray *rays_out,
                     size_t cap, size_t *n_out, const float m[16], const float minv[16], const float normi[9],
                     const gvt_hip_light *lights, size_t n_lights, int normal_mode, uint32_t seed, uint32_t flags);

/* ---- the Embree queries the adapter is built on (rtcIntersect / rtcOccluded,
 *      EmbreeMeshAdapter.cpp:474,375): object-space rays, t in (tnear, FLT_MAX) ---- */
int gvt_hip_intersect(gvt_hip_mesh *, const float *org /* n*3 */, const float *dir /* n*3 */, size_t n, float tnear,
                      gvt_hip_hit *hits_out);
int gvt_hip_occluded(gvt_hip_mesh *, const float *org, const float *dir, size_t n, float tnear, int32_t *occluded_out);

/* ---- device-resident RayVector (actor/Ray.h:189) ---- */
gvt_hip_queue *gvt_hip_queue_create(size_t capacity);
void gvt_hip_queue_destroy(gvt_hip_queue *);
int gvt_hip_queue_reserve(gvt_hip_queue *, size_t capacity); /* grows, keeps contents */
int gvt_hip_queue_clear(gvt_hip_queue *);
int gvt_hip_queue_size(gvt_hip_queue *, size_t *n);          /* host-side count, exact between API calls; no device access */
/* append n 80-byte rays.  flags: GVT_HIP_APPEND_DEVICE -- `rays` is device memory (default: host); GVT_HIP_APPEND_KEEP_STATE -- the rays are rays this
 * library exported (gvt_hip_queue_export, the wire image of an exchange) and bytes 64..79 carry their state: the RNG stream word and the
 * instances already crossed without a hit (known misses).  Without it the rays are FRESH, whatever those bytes hold: a GraviT host leaves them
 * uninitialised (Ray.h:106-116 never writes data[64..79]), and stack garbage read as a known-miss list would make the scheduler walk a ray
 * through an instance without tracing it. */
#define GVT_HIP_APPEND_DEVICE 1
#define GVT_HIP_APPEND_KEEP_STATE 2
int gvt_hip_queue_append_flags(gvt_hip_queue *, const gvt_hip_ray *rays, size_t n, int flags);
/* The entry point of the earlier revisions, with the meaning it had there: src_on_device != 0 -- `rays` is a wire image in device memory (what an exchange
 * delivered; this library exported it): its state bytes 64..79 are kept, = GVT_HIP_APPEND_DEVICE | GVT_HIP_APPEND_KEEP_STATE; src_on_device == 0 -- host
 * rays, taken as FRESH (= flags 0); any other value: GVT_HIP_ERR_INVALID (a revision-5 caller's flag word is refused, not misread).  A caller written
 * against the boolean keeps working; new code uses gvt_hip_queue_append_flags. */
int gvt_hip_queue_append(gvt_hip_queue *, const gvt_hip_ray *rays, size_t n, int src_on_device);
/* copy the queue out as 80-byte rays (host or device destination) */
int gvt_hip_queue_export(gvt_hip_queue *, gvt_hip_ray *dst, size_t cap, size_t *n, int dst_on_device);
/* Adapter::trace on device queues: consumes q_in (left empty, like ImageTracer.h:248), appends to q_out */
int gvt_hip_trace_queue(gvt_hip_mesh *, gvt_hip_queue *q_in, gvt_hip_queue *q_out, const float m[16], const float minv[16],
                        const float normi[9], const gvt_hip_light *lights, size_t n_lights, int normal_mode, uint32_t seed);
/* The same call, with the terminal rule of the shuffleRays that would follow (TracerBase.h:396-400) applied inside the adapter: a
 * ray the adapter would append to q_out (an un-occluded shadow ray, or a ray that leaves the mesh without a hit) but that meets no
 * instance other than from_inst is not appended: a SHADOW ray that carries colour deposits color*w into fb on the spot, any other
 * such ray is dropped -- exactly what the shuffle would have done with it.  All other rays reach q_out as before, so
 * gvt_hip_shuffle(top, q_out, from_inst, ...) afterwards completes the step.  top == NULL or fb == NULL: plain gvt_hip_trace_queue. */
int gvt_hip_trace_queue_sink(gvt_hip_mesh *, gvt_hip_queue *q, gvt_hip_queue *moved, const float m[16], const float minv[16],
                             const float normi[9], const gvt_hip_light *lights, size_t n_lights, int normal_mode, uint32_t seed,
                             gvt_hip_top *top, int from_inst, gvt_hip_fb *fb);

/* ---- gvtPerspectiveCamera::generateRays (gvtCamera.cpp:89-171, 233-312): fills q with W*H*samples^2 rays ---- */
int gvt_hip_camera_generate(gvt_hip_queue *q, const float eye[3], const float focus[3], const float up[3], float fov,
                            int width, int height, int samples, int depth, float jitter_window_size);
/* The same rays, listed tile by tile (tile = 8: 8x8 pixels, i.e. one 64-wide wavefront per tile; 0 = the reference's
 * pixel-major order).  A RayVector's order carries no meaning in the reference (TBB chunks, moved_rays under a mutex);
 * the schedulers use the tiled list because the shuffle below keeps list order and coherent packets traverse faster. */
int gvt_hip_camera_generate_tiled(gvt_hip_queue *q, const float eye[3], const float focus[3], const float up[3], float fov,
                                  int width, int height, int samples, int depth, float jitter_window_size, int tile);

/* ---- top-level instance set + shuffleRays (accel/BVH.h:61-135, actor/RayPacket.h:83-211,
 *      algorithm/TracerBase.h:325-343,392-414) ----
 * inst_lo/hi: world AABBs (api.cpp:309-312).  The instances are tested in the order the reference's
 * BVH visits its leaves (BVH.cpp:77-171), so ties resolve identically. */
gvt_hip_top *gvt_hip_top_create(const float *inst_lo, const float *inst_hi, size_t n_inst);
void gvt_hip_top_destroy(gvt_hip_top *);
int gvt_hip_top_order(const gvt_hip_top *, int32_t *order_out /* n_inst */);
/* New instance boxes (n_inst as at create): the order, the device boxes and the top BVH are rebuilt in place; tracers borrowing the top
 * see them at their next frame. */
int gvt_hip_top_update(gvt_hip_top *, const float *inst_lo, const float *inst_hi, size_t n_inst);
/* shuffleRays(rays, from): consumes q_in (also when it fails: q_in is then cleared, its rays are lost); a ray whose next instance is i is advanced
 * (origin += dir * t * 0.95f) and appended to queues[i] -- unless keep_mask!=NULL and keep_mask[i]==0
 * (Tracer<DomainScheduler>::shuffleDropRays, DomainTracer.h:148-183); SHADOW rays that hit no further
 * instance deposit color*w into fb (fb may be NULL only if deposit is impossible, i.e. from<0 drop mode). */
int gvt_hip_shuffle(gvt_hip_top *, gvt_hip_queue *q_in, int from, gvt_hip_queue *const *queues /* n_inst */,
                    const uint8_t *keep_mask, gvt_hip_fb *fb);
/* sizes of n queues in one round trip */
int gvt_hip_queue_sizes(gvt_hip_queue *const *queues, size_t n, uint64_t *sizes_out);

/* ---- Tracer<ImageScheduler>::operator() (algorithm/ImageTracer.h:127-269) for one rank, natively: clearBuffer, generateRays,
 *      FilterRaysLocally, then until every queue is empty: pick the fullest queue (first strictly largest, :159-173), adapter->trace,
 *      shuffleRays.  meshes[i] / m / minv / normi are per instance (adapters may repeat: adapterCache, :184-233).  The caller
 *      owns the queues (n_inst of them), q_moved and fb; on return the queues are empty and fb holds the frame.  q_cam is not used
 *      any more (generateRays is fused into FilterRaysLocally, gvt_hip_camera_filter) and may be NULL. ---- */
typedef struct gvt_hip_camera {
  float eye[3], focus[3], up[3];
  float fov;
  int32_t width, height, samples, depth;
  float jitter_window_size;
} gvt_hip_camera;
/* generateRays (gvtCamera.cpp:233-312) + FilterRaysLocally (ImageTracer.h:111-125 / shuffleDropRays, DomainTracer.h:148-183) in one
 * step: every camera ray is appended to the queue of the instance it enters first (advanced like gvt_hip_shuffle does), without the
 * W*H*samples^2 list ever being written to memory.  tile as in gvt_hip_camera_generate_tiled. */
int gvt_hip_camera_filter(gvt_hip_top *, const gvt_hip_camera *cam, int tile, gvt_hip_queue *const *queues, const uint8_t *keep_mask);
int gvt_hip_image_frame(gvt_hip_top *, gvt_hip_mesh *const *meshes, const float *m /* n_inst*16 */, const float *minv, const float *normi /* n_inst*9 */,
                        size_t n_inst, const gvt_hip_light *lights, size_t n_lights, int normal_mode, const gvt_hip_camera *cam,
                        gvt_hip_queue *const *queues, gvt_hip_queue *q_cam, gvt_hip_queue *q_moved, gvt_hip_fb *fb, uint64_t *adapter_calls);

/* ---- the schedulers as native loops (csrc/domain.hip): Tracer<ImageScheduler>::operator() (ImageTracer.h:127-269) and
 *      Tracer<DomainScheduler>::operator() with SendRays (DomainTracer.h:185-496); asynchronous variant tracer/Domain/DomainTracer.cpp:109-192.
 *      Every round, all non-empty local queues go through ONE merged launch chain (closest hit, shade, any hit) and one shuffle, with
 *      one host synchronisation per round; the Domain scheduler's ray exchange is RCCL point-to-point on its own stream (announce =
 *      SendRays' count exchange + the termination vote, then the payload in the reference's wire format
 *      [int32 queueId][int32 nRays][80-byte Ray x nRays], :441-455). ---- */
typedef struct gvt_hip_comm gvt_hip_comm;     /* one rank's endpoint of the ray exchange */
typedef struct gvt_hip_hub gvt_hip_hub;       /* rendezvous of in-process ranks */
typedef struct gvt_hip_tracer gvt_hip_tracer; /* a Tracer<...> object for one rank */
/* RCCL transport: rank 0 calls gvt_hip_comm_unique_id, the 128 bytes reach the other ranks out of band (e.g. a torch.distributed or
 * MPI broadcast), every rank calls gvt_hip_comm_create on its own device.  Collective.  The library is resolved at first use: GVT_HIP_RCCL_LIB
 * (a path: a particular build, or a stand-in with the same entry points -- tests/fake_rccl) if set, else librccl.so.1 as the process or the system has it. */
int gvt_hip_comm_unique_id(unsigned char id[128]);
gvt_hip_comm *gvt_hip_comm_create(const unsigned char id[128], int rank, int world);
/* In-process transport: the ranks are threads of one process (one context each, gvt_hip_ctx_create) sharing a device; transfers are
 * device-to-device copies ordered by events.  Same protocol, no RCCL: several ranks per node on one GPU, and the way the Domain
 * scheduler's multi-rank control flow is exercised on a one-GPU machine. */
gvt_hip_hub *gvt_hip_hub_create(int world);
void gvt_hip_hub_abort(gvt_hip_hub *);        /* a rank failed: wake the ranks blocked in an exchange (they return an error) */
void gvt_hip_hub_destroy(gvt_hip_hub *);
gvt_hip_comm *gvt_hip_comm_create_local(gvt_hip_hub *, int rank);
void gvt_hip_comm_destroy(gvt_hip_comm *);
/* loop-back check on this rank: grouped send-to-self / receive-from-self of `bytes` bytes (+ an in-place ncclReduce under RCCL) through the
 * very calls the frame loop makes; 0 = the payload came back intact */
int gvt_hip_comm_selftest(gvt_hip_comm *, size_t bytes);
int gvt_hip_comm_rank(const gvt_hip_comm *);
/* ranks the transport itself counts (ncclCommCount; the hub's world): gvt_hip_comm_create fails unless it equals `world` */
int gvt_hip_comm_count(const gvt_hip_comm *);
/* compute units reserved for the communicator's own stream (knob "comm_cus" of the creating context at gvt_hip_comm_create[_local]; 0: none) */
int gvt_hip_comm_reserved_cus(const gvt_hip_comm *);
/* deadline of every blocking point of an exchange, in milliseconds (default: GVT_HIP_EXCHANGE_TIMEOUT_MS or 20000).  A rank that waits
 * longer returns GVT_HIP_ERR_TIMEOUT with its last announce in gvt_hip_last_error(), aborts the communicator (ncclCommAbort / hub
 * abort) and must not use it again: the process reports and exits non-zero. */
int gvt_hip_comm_set_deadline_ms(gvt_hip_comm *, int ms);
int gvt_hip_comm_world(const gvt_hip_comm *);

/* The tracer copies matrices, lights and camera, creates its own per-instance queues, and borrows top, meshes and fb. */
gvt_hip_tracer *gvt_hip_tracer_create(gvt_hip_top *, gvt_hip_mesh *const *meshes, const float *m /* n_inst*16 */, const float *minv,
                                      const float *normi /* n_inst*9 */, size_t n_inst, const gvt_hip_light *lights, size_t n_lights,
                                      int normal_mode, const gvt_hip_camera *cam, gvt_hip_fb *fb);
void gvt_hip_tracer_destroy(gvt_hip_tracer *);
int gvt_hip_tracer_set_camera(gvt_hip_tracer *, const gvt_hip_camera *cam);
/* Rigid motion: the next frame's instance matrices (n_inst as at create), replacing the tracer's copies (stream-ordered).  Any affine
 * matrix is taken (gvt_hip_trace); the caller updates the top level's boxes to match (gvt_hip_top_update). */
int gvt_hip_tracer_set_transforms(gvt_hip_tracer *, const float *m /* n_inst*16 */, const float *minv, const float *normi /* n_inst*9 */, size_t n_inst);
/* mpiInstanceMap (DomainTracer.h:115-144): owner[i] = rank holding instance i.  comm == NULL (or never called): one rank, Image scheduler. */
int gvt_hip_tracer_set_domains(gvt_hip_tracer *, const int32_t *owner /* n_inst */, gvt_hip_comm *comm);
#define GVT_HIP_FRAME_BSP 1          /* Domain: trace until the local queues are dry, then exchange (Tracer<DomainScheduler>); default:
                                        one local chain per exchange, the payload moving while the next chain runs (asynchronous tracer) */
#define GVT_HIP_FRAME_NO_COMPOSITE 2 /* leave the per-rank framebuffers un-reduced */
#define GVT_HIP_FRAME_IMAGE 8        /* several ranks, Image scheduler (ImageTracer.h:111-125): the scene is replicated (every instance's mesh on every
                                        rank), each rank traces its contiguous portion of the camera's rays to the end, then the composite */
#define GVT_HIP_FRAME_FULL_REDUCE 4  /* composite by a sum-reduce of whole frames (ncclReduce) instead of each rank's written rectangle */
typedef struct gvt_hip_frame_stats {
  uint64_t rounds;       /* exchanges (Domain) */
  uint64_t chains;       /* merged launch chains on this rank */
  uint64_t host_syncs;   /* host synchronisations of the frame */
  uint64_t rays_sent;    /* rays this rank sent to other ranks */
  uint64_t rays_closest; /* rays this rank pushed through the closest-hit kernel */
  uint64_t rays_any;     /* ... through the any-hit kernel */
  uint64_t packets_bailed; /* 64-ray packets the packet traversal handed to the one-lane-per-ray kernels (stack / step budget) */
  uint64_t bytes_sent;   /* payload bytes this rank sent to other ranks (wire format, DomainTracer.h:441-455), composite excluded */
  /* where a multi-rank frame's time goes (HIP events on the compute / communication streams, host clock for the waits); 0 on one rank, and 0
   * unless gvt_hip_set_option("frame_timing", 1): the breakdown costs five more event calls per exchange */
  double ms_chain;       /* local launch chains (incl. unpacking what arrived) */
  double ms_announce;    /* announce exchanges: group of sends / receives + the report's device-to-host copy */
  double ms_payload;     /* payload exchanges, posting to arrival (overlaps the next chain) */
  double ms_composite;   /* framebuffer composite on rank 0 */
  double ms_host_wait;   /* host time blocked in the exchanges' bounded waits */
  uint64_t exchanges;    /* transport groups (ncclGroupStart .. End) this rank issued in the frame, composite included: one per tick when every pair's
                            payload rode inside the announce ("inline_kb"), two where a payload exchange followed */
  uint64_t rays_inline;  /* of rays_sent: rays that travelled inside an announce */
  uint64_t early_deposit_launches; /* any-hit launches of the frame whose deposits were stored at shading time ("early_deposit"); added at the end of revision 6's record:
                                    * gvt_hip_tracer_frame writes the whole record, so a caller compiled against the shorter one must be rebuilt against this header */
} gvt_hip_frame_stats;
/* One frame: clearBuffer, generateRays + FilterRaysLocally / shuffleDropRays, rounds until every queue of every rank is empty, then
 * (Domain) the composite: the sum of the ranks' float framebuffers on rank 0 (IceTComposite.cpp:84-101).  Collective under a comm. */
int gvt_hip_tracer_frame(gvt_hip_tracer *, int flags, gvt_hip_frame_stats *stats);

/* ---- volume domains: Volume + TransferFunction (render/data/primitives/Volume.h, TransferFunction.{h,cpp}), the volume adapters'
 *      trace (adapter/ospray/OSPRayAdapter.cpp, adapter/pvol/PVolAdapter.cpp) and the volume branch of shuffleRays
 *      (algorithm/TracerBase.h:344-391) ----
 * A volume is one brick of a global scalar grid of global_counts vertices, x fastest (BOV order).  `origin` is the position of the GLOBAL
 * grid's vertex 0 and `spacing` its vertex spacing, in the volume's own (object) space; `offset` is the brick's first vertex in global indices
 * and the brick owns the cells [offset, offset + counts - 1) per axis, so neighbouring bricks share one layer of vertices.  A whole volume is
 * the brick with offset 0 and counts = global_counts.
 * Samples lie on ONE lattice per ray: t_k = k * dt from the ray's origin, which stays fixed, with dt = min(spacing) / sampling_rate; t is the
 * ray's own parameter (object space = minv * world, the direction not normalised, so t means the same in both).  A sample belongs to the brick
 * that owns its global cell floor((p - origin) / spacing), whatever the bricking.  Per sample, in this order: trilinear interpolation of the
 * cell's 8 vertices; the 256-entry table at clamp((v - lo) / (hi - lo), 0, 1) * 255, linear between two entries; front-to-back compositing
 * f = (1 - A) * a, C += f * c, A += f.  The ray carries its state: color = the premultiplied C, w = A, t_min = t of the last lattice sample
 * marched (the next brick goes on after it), depth = the flags.  A ray stops with GVT_HIP_RAY_OPAQUE once A >= GVT_HIP_VOLUME_OPAQUE_A, else
 * it leaves the brick with GVT_HIP_RAY_BOUNDARY.  A visit of one brick walks at most 2^22 lattice positions.
 * Samples need not be finite.  lerp(a, b, f) = a + f * (b - a) in float32, so a cell with an Inf vertex (or with finite vertices whose difference
 * overflows) gives NaN (Inf - Inf, 0 * Inf) or +-Inf samples: NaN looks up entry 0 (clamp is fminf(fmaxf(x, 0), 1)), +Inf entry 255, -Inf entry 0;
 * macro-cell skipping accounts for them.  A ray that arrives with w >= GVT_HIP_VOLUME_OPAQUE_A marches one owned sample and stops there. */
#define GVT_HIP_RAY_OPAQUE 0x2            /* actor/ORays.h */
#define GVT_HIP_RAY_BOUNDARY 0x4
#define GVT_HIP_RAY_EXTERNAL_BOUNDARY 0x10
#define GVT_HIP_VOLUME_OPAQUE_A 0.99f     /* early ray termination */
#define GVT_HIP_VOLUME_DEVICE 1           /* create: `samples` is device memory (default: host) */
#define GVT_HIP_VOLUME_NO_SKIP 2          /* create: interpolate every sample (no macro-cell skipping; the results are the same bits) */
typedef struct gvt_hip_volume gvt_hip_volume;
gvt_hip_volume *gvt_hip_volume_create(const float *samples, const int counts[3], const float origin[3], const float spacing[3], const int offset[3],
                                      const int global_counts[3], float sampling_rate, int flags);
void gvt_hip_volume_destroy(gvt_hip_volume *);
typedef struct gvt_hip_volume_info {
  float box_lo[3], box_hi[3]; /* the brick's vertices in the volume's own space */
  float dt;                   /* lattice step */
  float value_min, value_max; /* range of the brick's samples */
  int32_t blocks[3];          /* macro cells (8^3 cells each) per axis */
  float pad;
  uint64_t n_blocks, n_blocks_empty; /* macro cells, and those whose table maximum (corrected opacity over the block's value range) is 0 */
  uint64_t samples_marched;   /* lattice samples the brick owned along the rays marched so far, skipped ones included */
  uint64_t samples_gathered;  /* ... of which were interpolated (8 voxel reads each); the others lay in empty macro cells */
} gvt_hip_volume_info;
int gvt_hip_volume_get_info(gvt_hip_volume *, gvt_hip_volume_info *); /* synchronises */
/* Time-varying volumes (Volume::SetSamples, Volume.h): the next time step's samples for the same brick, in place.  n_samples must be
 * counts[0] * counts[1] * counts[2] of the brick as created; flags: 0 (samples in host memory) or GVT_HIP_UPDATE_DEVICE (a device pointer:
 * no host round trip of the grid).  A null volume, null samples, another n_samples or an unknown flag bit: GVT_HIP_ERR_INVALID, the volume
 * exactly as it was.
 * After the call the volume answers exactly like a volume freshly created from these samples with the same geometry, sampling rate and
 * skip flag and the same set_transfer / set_surfaces / set_lights calls: every ray bit of gvt_hip_volume_trace and gvt_hip_volume_frame,
 * value_min / value_max and n_blocks / n_blocks_empty.  The macro cells' value ranges are recomputed on the device (the kernel create
 * itself uses: the minimum and maximum of a cell's vertices that are not NaN, and whether one of them is not finite; a vertex on a block
 * boundary counts for both blocks) and the skip tables rebuilt from them by the rule of _set_transfer and _set_surfaces.  samples_marched,
 * samples_gathered and the crossings go on accumulating.  Every device pointer the volume holds stays valid (nothing is re-allocated), so
 * tracers, tops and queues built around it keep working.  The call waits for the calling context's stream first, as _set_transfer does,
 * and returns when it is done; the caller serialises it against frames that use the brick.  Before any _set_transfer it is legal: the
 * tables are then built when the transfer function arrives.  Samples need not be finite (the rules above).
 * The ghost layers of gvt_hip_volume_set_ghosts are left alone: they still hold the previous step's vertices, and the caller sends the
 * new step's with another _set_ghosts (until then a CENTRAL gradient next to a face mixes the two steps).
 * GVT_HIP_ERR_DEVICE (a HIP call failed part way): the samples may already be replaced while ranges and tables are not; the volume is then
 * undefined until an update succeeds, and may only be updated again or destroyed.
 * ms_out (may be NULL): time on the context's stream from the end of the upload to the end of the update (ranges, their download, the
 * tables' rebuild on the host and their upload), as for gvt_hip_mesh_update_vertices. */
int gvt_hip_volume_update_samples(gvt_hip_volume *, const float *samples, size_t n_samples, uint32_t flags, float *ms_out /* may be NULL */);
/* Typed voxels (Volume::VoxelType, Volume.h:67-75; the BOV formats of VolApp.cpp:110-160).  A volume has a voxel type, fixed at creation,
 * and its samples stay on the device at that width: a uint8 brick costs a quarter of the memory and of the upload of its float copy, a
 * 16-bit one half.  No float copy of the grid exists on the device or on the host at any time, creation and update included.
 * A vertex's value is (float)v, with no scale and no offset: the transfer function's value_lo / value_hi and the isovalues are given in
 * those units (0..255 for uint8 data).  The conversion is exact for every 8- and 16-bit integer, and everything else of the volume
 * contract (lattice, ownership, macro cells, skipping, surfaces, lights, flags) is unchanged, so a volume of type T made from samples s
 * answers like the F32 volume made from (float)s with the same other arguments and the same set_transfer / set_surfaces / set_lights
 * calls: every ray bit of gvt_hip_volume_trace, gvt_hip_shuffle_volume and gvt_hip_volume_frame, value_min / value_max, n_blocks /
 * n_blocks_empty, the march counters and the crossings.  Integer voxels are never NaN or Inf: the not-finite flag of their macro cells
 * is always clear.  DOUBLE and INT data are not exact in float32 and have no type here: the caller converts them, as before. */
#define GVT_HIP_VOXEL_F32 0
#define GVT_HIP_VOXEL_U8 1
#define GVT_HIP_VOXEL_I16 2
#define GVT_HIP_VOXEL_U16 3
/* gvt_hip_volume_create with samples of voxel_type (counts[0] * counts[1] * counts[2] of them, host memory or, with GVT_HIP_VOLUME_DEVICE,
 * device memory).  An unknown type: NULL and an error text.  gvt_hip_volume_create is this call with GVT_HIP_VOXEL_F32. */
gvt_hip_volume *gvt_hip_volume_create_typed(const void *samples, int voxel_type, const int counts[3], const float origin[3], const float spacing[3],
                                            const int offset[3], const int global_counts[3], float sampling_rate, int flags);
/* gvt_hip_volume_update_samples for a volume of voxel_type, with everything that call promises.  voxel_type must be the volume's own:
 * otherwise GVT_HIP_ERR_INVALID and nothing changes.  gvt_hip_volume_update_samples is this call with GVT_HIP_VOXEL_F32 (so on a volume of
 * another type it is refused in the same way). */
int gvt_hip_volume_update_samples_typed(gvt_hip_volume *, const void *samples, int voxel_type, size_t n_samples, uint32_t flags, float *ms_out /* may be NULL */);
/* the volume's voxel type and the bytes one sample takes on the device (4, 1, 2, 2); either pointer may be NULL (gvt_hip_volume_info
 * keeps its layout) */
int gvt_hip_volume_get_voxel_type(gvt_hip_volume *, int *type_out, size_t *sample_bytes_out);
/* TransferFunction: cmap rows (x r g b), omap rows (x a), each resampled to 256 entries as TransferFunction::DeviceCommit does
 * (TransferFunction.cpp:40-72); the opacity corrected on the host, a' = 1 - (1 - a)^(1 / sampling_rate) in double; the macro-cell table
 * rebuilt.  [value_lo, value_hi] maps onto the table.  At least 2 rows each, x not decreasing, value_lo < value_hi.
 * n_blocks_empty counts the macro cells the table leaves empty (their samples go uninterpolated unless GVT_HIP_VOLUME_NO_SKIP): with
 * e(v) = floor(clamp((v - value_lo) / (value_hi - value_lo), 0, 1) * 255) in double, a macro cell whose vertices span [min, max] is empty
 * when no entry in [max(0, e(min) - 1), min(255, e(max) + 2)] has a corrected opacity above 0.  The interval starts at entry 0 when a
 * vertex of the cell is not finite, and is the whole table when the cell has no vertex that is a number or max - min reaches 3.4e38. */
int gvt_hip_volume_set_transfer(gvt_hip_volume *, const float *cmap, int nc, const float *omap, int no, float value_lo, float value_hi);
/* OSPRayAdapter::trace on a host RayVector: rays[begin, end) (end == 0: n) are marched through the brick (m is the instance's matrix, minv
 * its inverse; the march needs minv only) and every one of them comes back in rays_out with its flags and state.  cap too small:
 * GVT_HIP_ERR_CAPACITY, *n_out = the count needed, nothing marched. */
int gvt_hip_volume_trace(gvt_hip_volume *, const gvt_hip_ray *rays, size_t n, size_t begin, size_t end, gvt_hip_ray *rays_out, size_t cap,
                         size_t *n_out, const float m[16], const float minv[16]);
/* shuffleRays, volume branch, PRIMARY rays (TracerBase.h:344-391), order-preserving; consumes q_in (which may be queues[from]).
 * from >= 0: a RAY_OPAQUE ray deposits; a RAY_BOUNDARY ray goes on to the next brick -- the nearest box (entry distance, ties in the top's
 * order) other than `from` whose exit lies beyond the exit of box `from` -- with the flag cleared, or, with none, becomes EXTERNAL and
 * deposits.  from < 0 (camera rays): every ray goes to the nearest box whose exit lies beyond its t_min, starting with C = 0, A = 0 and
 * depth 0; a ray that meets none is dropped.  A deposit adds (color, w) = (C, A) to the pixel: the colour is already premultiplied (the
 * reference adds color * w); deposits are float atomics, so the sums are bit-reproducible only with one ray per pixel.  At most 256 bricks. */
int gvt_hip_shuffle_volume(gvt_hip_top *, gvt_hip_queue *q_in, int from, gvt_hip_queue *const *queues, gvt_hip_fb *fb);
/* Tracer<ImageScheduler> over volume bricks: clearBuffer, the camera's rays into the brick each enters first (gvt_hip_shuffle_volume, from
 * -1), then until every queue is empty: march the fullest queue (first strictly largest), shuffle.  One host wait per round;
 * *adapter_calls = the marches. */
int gvt_hip_volume_frame(gvt_hip_top *, gvt_hip_volume *const *volumes, const float *m /* n_inst*16 */, const float *minv, size_t n_inst,
                         const gvt_hip_camera *cam, gvt_hip_queue *const *queues, gvt_hip_fb *fb, uint64_t *adapter_calls);

/* ---- surfaces of a volume: Volume::SetIsovalues / SetSlices (Volume.h:96-100,128-132) as OSPRayAdapter hands them to its renderer
 *      (OSPRayAdapter.cpp:70-86), with the lights that exist only for them (:245-295) ----
 * Up to GVT_HIP_VOLUME_MAX_SURFACES surfaces, indexed i: the n_iso isovalues in the order given, then the n_slices planes (nx, ny, nz, d),
 * object space.  Each is the zero set of a field sampled at the ray's lattice positions p_k = o + (k * dt) * d (per axis o + d * t with
 * t = (float)k * dt, as the march's own position):
 *   isovalue c_i: side_i(k) = (v_k >= c_i), v_k the sample's trilinear value;  plane: side_i(k) = ((nx*p.x + ny*p.y) + nz*p.z >= d).
 * A comparison with NaN is false.  sides(k) = the mask of those bits (bit i = surface i).
 * A CROSSING of surface i is detected AT sample k when the brick owns k, the ray marched k - 1, and side_i(k) != side_i(k - 1).  "Marched":
 * earlier in this visit, or k - 1 is the sample in the ray's t_min and the ray carries its sides: the flag GVT_HIP_RAY_SIDES in depth, and
 * sides(k - 1) as a float in the ray's t field (bytes 44..47; an integer in [0, 65535]).  The carried sides count only if the brick's first
 * owned sample is exactly the first lattice sample after t_min; otherwise (no flag: camera rays, whose depth the shuffle from -1 zeroes; a
 * gap between bricks) the first owned sample has no previous one and detects nothing.  A surface is thus rendered at the sample after it, at
 * most one lattice step behind: everything that shades it belongs to the brick that owns that sample, so the bricking cannot change the image.
 * A march that owned a sample writes sides(last sample) into t and sets the flag; one that owned none leaves t and the flag as they came.
 * RENDERING at sample k, before the sample's own contribution, if any surface is crossed: for each crossed surface in index order while
 * A < GVT_HIP_VOLUME_OPAQUE_A:
 *   c = the table's rgb (the sample's look-up, opacity ignored) at c_i for an isovalue, at v_k for a plane;
 *   g = for a plane (nx, ny, nz); for an isovalue the gradient of the trilinear interpolant in the sample's cell, with lerp(a, b, f) =
 *       a + f * (b - a) and f the sample's fractions:
 *         g.x = lerp(lerp(v100 - v000, v110 - v010, f.y), lerp(v101 - v001, v111 - v011, f.y), f.z) / spacing.x
 *         g.y = lerp(lerp(v010 - v000, v110 - v100, f.x), lerp(v011 - v001, v111 - v101, f.x), f.z) / spacing.y
 *         g.z = lerp(lerp(v001 - v000, v101 - v100, f.x), lerp(v011 - v010, v111 - v110, f.x), f.y) / spacing.z
 *   with lights: len = sqrt((g.x*g.x + g.y*g.y) + g.z*g.z); S = (0, 0, 0); if len > 0 (false for NaN): n = g / len and per light j in order
 *       ndl = |(n.x*l.x + n.y*l.y) + n.z*l.z|, S = S + colour_j * ndl; rgb = c * (ka + kd * S) per channel.  Without lights: rgb = c.
 *   f = (1 - A) * opacity; C = C + f * rgb; A = A + f.  No clamp.
 * If A >= GVT_HIP_VOLUME_OPAQUE_A after that, the ray stops with GVT_HIP_RAY_OPAQUE and the sample's own contribution is not added; t_min
 * records k either way.  A sample without a crossing is the plain march's.
 * LIGHTS: GraviT's positions and colours, world space.  The direction of light j is -position_j, taken to object space as a vector
 * through the instance's minv (m[r]*x + m[4+r]*y) + (m[8+r]*z + m[12+r]*0) and divided by its length sqrt((x*x + y*y) + z*z), on the HOST in
 * float32 at every march (length 0 or not finite: direction 0).  This equals world-space shading for rigid motions and uniform scales only.
 * Skipping: a macro cell is jumped only where no crossing can hide (no isovalue within its value range, no plane among the samples jumped,
 * not at a sample whose sides differ from the previous one's); the bits are those of GVT_HIP_VOLUME_NO_SKIP, the rays' t field included. */
#define GVT_HIP_RAY_SIDES 0x20            /* depth: the ray's t field holds sides(sample in t_min) (actor/ORays.h uses 0x1..0x10) */
#define GVT_HIP_VOLUME_MAX_SURFACES 16
#define GVT_HIP_VOLUME_MAX_LIGHTS 8
/* 0 isovalues and 0 slices clear the surfaces (the plain march again).  NaN isovalue, zero or non-finite plane, opacity outside (0, 1],
 * more than 16 surfaces: GVT_HIP_ERR_INVALID, the volume unchanged.  Rebuilds the per-cell skip table, as _set_transfer does. */
int gvt_hip_volume_set_surfaces(gvt_hip_volume *, const float *isovalues, int n_iso, const float *slices /* n_slices*4 */, int n_slices, float opacity);
/* n = 0: no lights (rgb = c).  More than GVT_HIP_VOLUME_MAX_LIGHTS or a non-finite value: GVT_HIP_ERR_INVALID.  The OSPRay adapter's
 * material is ka = 0.4, kd = 0.6. */
int gvt_hip_volume_set_lights(gvt_hip_volume *, const float *positions /* n*3 */, const float *colours /* n*3 */, int n, float ka, float kd);
/* surfaces composited by the marches of this volume so far (gvt_hip_volume_info keeps its layout); synchronises */
int gvt_hip_volume_get_crossings(gvt_hip_volume *, uint64_t *crossings_rendered);

/* ---- lit volumes: the fog's own samples shaded by the scalar gradient, as the volume engines behind the reference's adapters shade
 *      theirs with the lights and the ka = 0.4, kd = 0.6 material the adapters hand them (adapter/galaxy/PVolAdapter.cpp:366-397,
 *      adapter/ospray/OSPRayAdapter.cpp:249-295) ----
 * The lights, ka and kd are those of gvt_hip_volume_set_lights, prepared by the host at every march exactly as for the surfaces (unit
 * directions in object space, direction 0 for a degenerate light).  Shading applies when the mode is GVT_HIP_VOLUME_SHADE_GRADIENT AND the
 * volume has at least one light; otherwise the march is the one stated above, through the same kernels: a volume whose shading was never
 * switched on is untouched, and _set_lights without _set_shading keeps its meaning (the lights are for the surfaces only).
 * A shaded march replaces the sample's own contribution.  Sample k has value v, fractions f, cell vertices v000..v111, tc = the table's
 * look-up at v (rgb and corrected opacity tc.w):
 *   if tc.w > 0:  g = the three expressions stated above for an isovalue's gradient (same lerp nesting, divided by the spacing);
 *                 len = sqrt((g.x*g.x + g.y*g.y) + g.z*g.z);  S = (0, 0, 0);
 *                 if len > 0 and len < +Inf (false for NaN): n = g / len and per light j in order
 *                     ndl = |(n.x*l.x + n.y*l.y) + n.z*l.z|,  S = S + colour_j * ndl;
 *                 rgb = tc.rgb * (ka + kd * S) per channel
 *   otherwise:    rgb = tc.rgb (no gradient is computed, nothing is counted)
 *   then as ever: f = (1 - A) * tc.w;  C = C + f * rgb;  A = A + f.
 * Every operation is one float32 operation in this order: no contraction, no fast math.  samples_shaded counts the samples that took the
 * tc.w > 0 branch.
 * Why tc.w > 0: a sample of zero opacity adds exactly +0 whether it is shaded or not, so macro-cell skipping stays bit-exact against
 * GVT_HIP_VOLUME_NO_SKIP (a skipped sample is one of those), samples_shaded is the same with and without skipping, and on a sparse table
 * the gradient is computed only where it shows.
 * Why len < +Inf: on a grid with Inf vertices, or finite ones whose differences overflow, g has an infinite component and g / len would
 * be NaN (Inf / Inf); the guard shades such a sample with S = 0, i.e. rgb = tc.rgb * ka, and C stays finite as the non-finite part of the
 * volume contract promises.  THE SURFACE RULE DIFFERS: a crossed isosurface tests len > 0 only (its rule above is unchanged).
 * Consequences: ka = 1, kd = 0 gives the plain march's bits (x * (1 + 0 * S) = x, S being finite); so do no lights and mode NONE.
 * With surfaces, a crossing detected at sample k is rendered first, as above, and then -- unless it ended the ray -- the sample's own
 * contribution is shaded with the same g.  The clipped march and typed voxels shade alike.
 * Bricking: the interpolant's gradient in the sample's own cell needs that cell's eight vertices only, which the sample's owner holds:
 * no ghost layers, and the image is the same bits for every bricking.
 * DEVIATION from the reference's engines, in the DEFAULT gradient kind only: they shade with central differences of the vertices, a
 * gradient that is continuous across cells.  The default (GVT_HIP_VOLUME_GRADIENT_CELL) is the gradient of the trilinear interpolant:
 * continuous inside a cell, discontinuous across cell faces (facets at low resolution, plain to see on an isosurface).  A brick that
 * is given its six ghost faces can shade with central differences instead and keeps "the same bits for every bricking": smooth
 * gradients, below. */
#define GVT_HIP_VOLUME_SHADE_NONE 0
#define GVT_HIP_VOLUME_SHADE_GRADIENT 1
int gvt_hip_volume_set_shading(gvt_hip_volume *, int mode);        /* any other mode: GVT_HIP_ERR_INVALID, the volume unchanged */
int gvt_hip_volume_get_shading(gvt_hip_volume *, int *mode_out);
/* samples shaded by the marches of this volume so far (gvt_hip_volume_info keeps its layout); synchronises, as _get_crossings does */
int gvt_hip_volume_get_shaded(gvt_hip_volume *, uint64_t *samples_shaded);

/* ---- smooth gradients: central differences at the vertices, interpolated trilinearly, with one ghost layer per interior face ----
 * The gradient KIND says which gradient shades a crossed isovalue and a lit sample.  CELL (the default) is the one stated above.  CENTRAL:
 * along an axis of N = global_counts vertices and spacing s, the vertex with GLOBAL index i has im = max(i - 1, 0), ip = min(i + 1, N - 1)
 * and the component
 *     (v[ip] - v[im]) / (s * (float)(ip - im))
 * with the other two indices held and v a global vertex value (float)sample: one subtraction, one multiplication (by 2 or by 1), one
 * division.  On the global boundary the difference is one-sided.  v[ip] and v[im] are the brick's own samples where it holds them and
 * the ghost face's otherwise.  A sample's component is the trilinear interpolation of that component at the eight vertices of its cell,
 * with the sample's fractions and the value's own lerp nesting (x first, then y, then z; lerp(a, b, f) = a + f * (b - a)).  Every
 * operation is one float32 operation in this order: no contraction, no fast math.
 * From g on everything is the rule stated above, unchanged: a crossed isovalue tests len > 0; a lit sample tests tc.w > 0, then len > 0 and
 * len < +Inf; the lights, ka + kd * S and the compositing are the same.  Slice planes keep their own normal.  The kind is inert unless
 * something is shaded: the plain march has no central variant.  Crossing detection, the sides carried in t, skipping, jumps, the clip,
 * the flags and the counters do not depend on the kind, so skipping stays exact for the reasons given above (a sample is shaded only
 * where tc.w > 0 or a crossing is detected, and neither depends on g).  On a volume whose kind is CELL every ray bit is what it was
 * before the kind existed, a volume switched to CENTRAL and back included.
 * GHOSTS.  A central difference along an axis reaches one vertex beyond the cell on that axis and none on the others: six face layers
 * suffice, no edges and no corners.  faces[0..5] = the layer of global vertices just outside the brick at -x, +x, -y, +y, -z, +z;
 * +-x holds ny*nz samples at index j + ny*k, +-y nx*nz at i + nx*k, +-z nx*ny at i + nx*j (nx, ny, nz: the brick's counts; i, j, k:
 * the vertex's indices inside the brick).  The samples have the volume's voxel type and are copied; flags: 0 (host pointers) or
 * GVT_HIP_VOLUME_DEVICE (device pointers: the samples never visit the host).  A call replaces all six: NULL = no layer.  A face lies on
 * the global boundary when offset[a] == 0 (low side) or offset[a] + counts[a] == global_counts[a] (high side).
 * GVT_HIP_ERR_INVALID with an error text, the volume exactly as it was: a non-NULL face on the global boundary; a NULL face that is not on
 * it while the kind is CENTRAL; another voxel type than the volume's; unknown flag bits; a null volume or a null faces.
 * gvt_hip_volume_update_samples[_typed] leaves the layers alone (see there).
 * _set_gradient(CENTRAL) is accepted only when every face that is not on the global boundary has a layer, and refused on a volume with
 * AMR subgrids (as _set_subgrids is on a CENTRAL volume: AMR shades with the cell gradient only); an unknown kind is refused; each refusal changes nothing.
 * Bricking: with its faces a brick sees every global vertex a sample it owns can reach, so g is a function of global vertex values
 * and global indices only, and the image is the same bits for every bricking -- unconditionally, since CENTRAL cannot be set without the
 * layers.  tests/volume_smooth_checker.py restates the contract in numpy.
 * central_marches: the launches of this volume that shaded with CENTRAL so far (a march of a CENTRAL volume without surfaces and without
 * lit shading is the plain one and is not counted). */
#define GVT_HIP_VOLUME_GRADIENT_CELL 0    /* the interpolant's gradient in the sample's cell: the default */
#define GVT_HIP_VOLUME_GRADIENT_CENTRAL 1 /* central differences at the vertices, interpolated trilinearly */
int gvt_hip_volume_set_ghosts(gvt_hip_volume *, const void *const faces[6], int voxel_type, uint32_t flags);
int gvt_hip_volume_set_gradient(gvt_hip_volume *, int kind);
int gvt_hip_volume_get_gradient(gvt_hip_volume *, int *kind_out, uint64_t *central_marches_out); /* either may be NULL */

/* ---- geometry inside a volume: a march clipped at a depth plane, and the composite of the two images ----
 * The reference has no counterpart (shuffleRays takes either the mesh or the volume branch, by adapter type): this contract is the
 * project's own; tests/volume_clip_checker.py restates it in numpy.
 * CLIPPED MARCH.  A ray that carries GVT_HIP_RAY_CLIP in depth marches lattice sample k only if (float)k * dt < t_max, t_max being the
 * ray's own field (the comparison is false for NaN: a NaN t_max marches nothing, as does t_max <= 0).  k_clip = the largest k >= 0 that
 * passes (-1: none), found from floorf(t_max / dt) and corrected with that very comparison in both directions; t_max = +Inf, or a
 * k_clip that would reach 2^30, cuts nothing.  It bounds the visit last: k_hi = min(k_hi, k_clip).  Nothing changes per sample: the
 * clipped ray leaves with GVT_HIP_RAY_BOUNDARY (or _OPAQUE) and t_min at its last marched sample (unchanged where it marched none);
 * surfaces beyond the clip are not detected, their samples not being marched.  A ray without the flag gives the bits it gave before,
 * whatever its t_max holds.  gvt_hip_volume_trace honours the flag on host rays.  Marching the rest afterwards (flag and
 * GVT_HIP_RAY_BOUNDARY cleared, same brick) completes the ray to the bits of one unclipped march.
 * SHUFFLE.  For a ray that carries the flag a box is a candidate of gvt_hip_shuffle_volume only if its entry distance tn < t_max as
 * well (from < 0 and from >= 0 alike; false for NaN): a clipped ray deposits as EXTERNAL instead of hopping through bricks it cannot
 * sample, and a clipped camera ray with the wall in front of every brick is dropped.  The entry distance is the float slab test's and
 * the samples' owner the cell test's: the two can disagree by an ulp, so for a wall within an ulp of a brick's face a bricking may
 * differ from another (a measure-zero case, like a ray along a shared edge). */
#define GVT_HIP_RAY_CLIP 0x40             /* depth: march only the samples with k * dt < t_max */
/* DEPTH PLANE: W*H floats on the device, pixel-major like the framebuffer; each is t along the pixel's camera ray in the ray's own
 * parameter (the rays of gvt_hip_camera_generate_tiled: origin at the eye, unit direction), +Inf = nothing there. */
typedef struct gvt_hip_depth gvt_hip_depth;
gvt_hip_depth *gvt_hip_depth_create(int width, int height);
void gvt_hip_depth_destroy(gvt_hip_depth *);
int gvt_hip_depth_clear(gvt_hip_depth *);                                   /* every pixel +Inf */
int gvt_hip_depth_upload(gvt_hip_depth *, const float *t /* W*H */, uint32_t flags); /* 0: host memory, GVT_HIP_UPDATE_DEVICE: device memory */
int gvt_hip_depth_download(gvt_hip_depth *, float *t /* W*H, host */);
/* depth[id] = the minimum over ALL instances i of the closest hit's t (a miss: +Inf) of the camera's ray of pixel id, origin at the eye
 * and not advanced.  The ray of instance i is xfm_point(minv_i, o), xfm_vector(minv_i, d) = per row r (m[r]*x + m[4+r]*y) + (m[8+r]*z +
 * m[12+r]*w), w = 1 | 0, the direction not normalised, so t means the same in every instance; tnear = 1e-6 (GVT_RAY_EPSILON).  One
 * closest-hit launch per instance over the camera's list, in the order given, each followed by a one-writer-per-pixel minimum; one host
 * wait, at the end.  m is not read (minv is what a trace needs) and may be NULL.  cam->samples != 1, a film that is not the plane's size
 * or a null plane, camera, mesh or minv: GVT_HIP_ERR_INVALID, the plane unchanged. */
int gvt_hip_depth_render(gvt_hip_depth *, gvt_hip_mesh *const *meshes, const float *m /* n_inst*16 */, const float *minv, size_t n_inst,
                         const gvt_hip_camera *cam);
/* gvt_hip_volume_frame with every camera ray clipped at its pixel of `depth`: the camera's rays enter the queues with colour, opacity
 * and flags zeroed as before and, for pixel id, t_max = depth[id] and depth = GVT_HIP_RAY_CLIP where depth[id] < +Inf, 0 where it is not
 * (the shuffle from -1 applies the tn < t_max rule with these values).  depth == NULL: gvt_hip_volume_frame itself (one body).  Otherwise
 * cam->samples must be 1 and the film the plane's size: else GVT_HIP_ERR_INVALID, nothing changed. */
int gvt_hip_volume_frame_clipped(gvt_hip_top *, gvt_hip_volume *const *volumes, const float *m /* n_inst*16 */, const float *minv, size_t n_inst,
                                 const gvt_hip_camera *cam, gvt_hip_queue *const *queues, gvt_hip_fb *fb, const gvt_hip_depth *depth,
                                 uint64_t *adapter_calls);
/* front := front OVER back, per pixel p and in this order, every step one float32 operation (no contraction):
 *   k = 1 - front.a;   front.c = front.c + k * fminf(back.c, 1) per colour channel;   front.a = front.a + k * cov
 *   cov = depth ? (depth[p] < +Inf ? 1 : 0) : fminf(back.a, 1)
 * front is a volume frame (premultiplied colour, opacity), back a mesh frame (clamped as gvt_hip_fb_download clamps).  Coverage comes from
 * the depth plane, not from the mesh framebuffer's alpha: a shadowed surface pixel (colour 0, depth finite) is opaque black.  A pixel
 * without volume (front all zero) becomes min(back, 1) exactly.  Sizes must agree, front and back must not be NULL (GVT_HIP_ERR_INVALID). */
int gvt_hip_fb_composite_over(gvt_hip_fb *front, const gvt_hip_fb *back, const gvt_hip_depth *depth);

/* ---- AMR volumes: nested refined subgrids inside a brick (Volume::griddata / AddAMRGrid / is_AMR, render/data/primitives/Volume.h:40-58,
 *      101-135; api::createVolume(name, amr) and api::addAmrSubgrid, api.cpp:543-612; one domain = one level-0 grid with its descendants,
 *      all handed to one trace call, adapter/galaxy/PVolAdapter.cpp:74-107) ----
 * A volume (a level-0 brick) holds a set of subgrids, a tree: entry i refines a box of cells of its parent -- the brick's own grid
 * (parent -1) or an EARLIER entry -- `ratio` times per axis.  tests/volume_amr_checker.py restates what follows in numpy.
 * Everything of the volume contract stays: ONE lattice per ray for all levels, t_k = k * dt with dt = min(level-0 spacing) /
 * sampling_rate; a sample is owned by the brick whose level-0 cell floor((p - origin) / spacing) it lies in.  What is new is WHICH CELL
 * IS INTERPOLATED.  With g = (p - origin) / spacing, fl = floor(g) and f = g - fl as ever, start at the level-0 grid with the cell
 * ci = (int)fl (a global index) and the fractions f.  While a subgrid S of the current grid covers ci (S.lo[a] <= ci[a] < S.lo[a] +
 * S.cells[a] on every axis; there is at most one), per axis:
 *   h = f * (float)ratio;   j = (int)floorf(h);   ci = (ci - S.lo) * ratio + j;   f = h - (float)j;   the current grid = S
 * The final grid's cell ci, its 8 vertices and f go through the same trilinear expression, table look-up and compositing as before.
 * Every step of the descent is exact in float32 (f < 1, the ratio a power of two), so the choice between parent and child at a shared
 * face is made on integer cell indices and cannot differ between bricks, runs or skip modes.  Level-0 vertices strictly inside a
 * subgrid's footprint (and a subgrid's strictly inside a child's) are never read by the march.
 * MACRO CELLS.  The grid of level-0 macro cells (8^3 level-0 cells) stays.  The value range of a macro cell, and its not-finite flag, is
 * the union over every vertex whose position lies in the macro cell's closed box: the level-0 vertices, covered ones included, and the
 * vertices of every subgrid of every level (subgrids are cell-aligned, so per subgrid these form an index rectangle).  The empty rule of
 * _set_transfer is applied to that union, so skipping stays exact (GVT_HIP_VOLUME_NO_SKIP gives the same bits), and
 * gvt_hip_volume_info's n_blocks_empty, value_min and value_max follow the union.
 * DEVIATIONS.  One lattice for all levels: a refined region is not sampled more densely by itself (raise sampling_rate; the opacity
 * correction keeps the look).  The field is discontinuous across coarse-fine faces (no ghost or blend cells), as a cell-wise AMR
 * sampler's is.  A level-1 subgrid must lie inside one brick: the caller cuts it otherwise.
 * SURFACES AND LIT FOG (the flag GVT_HIP_VOLUME_AMR_SHADED of _set_subgrids; Volume::SetIsovalues / SetSlices and the AMR grids live on
 * one object in the reference).  A set of subgrids given with the flag takes isovalues, slice planes and GVT_HIP_VOLUME_SHADE_GRADIENT.
 * Everything of "surfaces of a volume" and "lit volumes" holds with these substitutions: v_k, the eight corner values v000..v111 and the
 * fractions f are those of the FINAL grid's cell after the descent; the gradient's divisor is the final grid's spacing per axis,
 * s_a = spacing.a / (float)R with R the product of the ratios down to the final grid (1 at level 0; a power of two up to 512, so s_a is
 * exact), i.e. g.a = (the lerp nest of corner differences stated there) / s_a.  Plane sides use the lattice point p_k as ever, a plane's
 * colour is looked up at the descended v_k, the isosurface rule len > 0 and the fog rule 0 < len < +Inf stay, and so do the side-mask
 * carry (GVT_HIP_RAY_SIDES, the t field), "a crossing is rendered at the sample after it", GVT_HIP_RAY_OPAQUE and GVT_HIP_RAY_CLIP.
 * tests/volume_amr_surface_checker.py restates this in numpy.  Skipping stays exact: the surface skip word of a macro cell is built from
 * the union range above, and a fine cell lies inside one macro cell, so with no isovalue within that range no sample of any level in
 * the cell changes an isovalue side; GVT_HIP_VOLUME_NO_SKIP gives the same bits, the rays' t field included.  _get_crossings, _get_shaded
 * and _get_amr_info count these marches too (samples_refined as before; amr_marches counts every AMR entry point).
 * DEVIATION.  The field is discontinuous across coarse-fine faces, so a crossing can be detected between a coarse and a fine sample
 * where a continuous field would have none.  It is deterministic and belongs to the owner of the later sample: the image is the same
 * bits for every bricking that keeps each level-1 subgrid in one brick.
 * Without the flag (the default) a volume that has subgrids takes no surfaces and no gradient shading: _set_surfaces with any surface
 * and _set_shading with GVT_HIP_VOLUME_SHADE_GRADIENT return GVT_HIP_ERR_INVALID and change nothing, as _set_subgrids without the flag
 * does on a volume that has either.
 * OUT OF SCOPE, refused on every AMR volume, flagged or not, with GVT_HIP_ERR_INVALID and nothing changed: central gradients
 * (_set_gradient(CENTRAL), and _set_subgrids on a CENTRAL volume), and _update_samples / _update_samples_typed, which know one grid.  A
 * new time step of an AMR volume on the same tree is gvt_hip_volume_update_amr ("time-varying AMR volumes" below), in place; a step
 * whose tree changes is _set_subgrids (with n = 0, _update_samples and _set_subgrids again where level 0 changes too), or a new volume.  The
 * shadowed, fog-shadowed and mesh-shadowed frames and both bakes do not take bricks with subgrids (they refuse, as stated with each),
 * and neither do gvt_hip_volume_frame_fused and _fused_shaded (they fall back to the loop); gvt_hip_volume_frame_fused_amr with
 * GVT_HIP_FUSED_AMR marches such bricks in the fused frame ("fused frame: AMR bricks" below).  The clipped march (GVT_HIP_RAY_CLIP, gvt_hip_volume_frame_clipped) works on AMR volumes, shaded ones
 * included. */
#define GVT_HIP_VOLUME_AMR_SHADED 8          /* _set_subgrids: this set takes surfaces and gradient shading (2 and 4 stay unknown bits) */
#define GVT_HIP_VOLUME_MAX_SUBGRIDS 4096
#define GVT_HIP_VOLUME_MAX_LEVELS 4          /* level 0 and up to three levels of subgrids */
typedef struct gvt_hip_subgrid {
  int32_t parent;    /* -1: the brick's own grid; else the index of an EARLIER entry of the same array */
  int32_t ratio;     /* 2, 4 or 8: cells per parent cell and axis (a power of two keeps every coordinate of the descent exact) */
  int32_t lo[3];     /* first parent cell covered; for parent -1 a GLOBAL cell index (as `offset` is), else a cell of the parent subgrid */
  int32_t cells[3];  /* parent cells covered per axis, >= 1 */
} gvt_hip_subgrid;    /* vertices: cells[a] * ratio + 1 per axis, float32, x fastest; vertex 0 sits on the parent's vertex lo; spacing = parent's / ratio */
/* Replaces the volume's whole set of subgrids (n == 0 removes it: the plain volume again, through the kernels it launched before).
 * samples[i]: the vertices of grids[i], in host memory or, with flags = GVT_HIP_VOLUME_DEVICE, in device memory (they never visit the
 * host); the volume keeps copies of its own.  Legal before and after _set_transfer; waits for the calling context's stream first, as
 * _set_transfer does; the macro cells' ranges are rebuilt on the device (the min / max / not-finite rule of the level-0 ranges).
 * GVT_HIP_ERR_INVALID, the volume exactly as it was: a null argument; a volume that is not GVT_HIP_VOXEL_F32; a ratio other than 2, 4
 * or 8; a parent outside [-1, own index); cells < 1 on an axis; a box that leaves its parent's cells (for parent -1: the cells the brick
 * owns, [offset, offset + counts - 1)); two subgrids of one parent that share a cell; more than GVT_HIP_VOLUME_MAX_LEVELS levels;
 * n < 0 or n > GVT_HIP_VOLUME_MAX_SUBGRIDS; an unknown flag bit; a subgrid of 2^24 or more vertices on an axis or 2^32 - 1 or more in
 * all; without GVT_HIP_VOLUME_AMR_SHADED a volume that has surfaces or GVT_HIP_VOLUME_SHADE_GRADIENT; a CENTRAL volume (n > 0).
 * flags: GVT_HIP_VOLUME_DEVICE | GVT_HIP_VOLUME_AMR_SHADED.  The volume remembers the flags of its current set.  With _AMR_SHADED the call
 * is accepted on a volume that already has surfaces and / or gradient shading, for n > 0 and for n == 0 (n == 0: the plain surface /
 * lit volume again, through the kernels it launched before), and while the volume holds the flagged set _set_surfaces and
 * _set_shading(GRADIENT) are accepted; they rebuild the per-cell skip table from the merged ranges, as on a plain volume. */
int gvt_hip_volume_set_subgrids(gvt_hip_volume *, const gvt_hip_subgrid *grids, const float *const *samples, int n, int flags);
typedef struct gvt_hip_volume_amr_info {
  int32_t n_subgrids, n_levels; /* n_levels: level 0 and the deepest subgrid's (1 without subgrids) */
  uint64_t subgrid_bytes;       /* device memory of the subgrids' samples and tables */
  uint64_t samples_refined;     /* gathered samples whose final grid was a subgrid, so far */
  uint64_t amr_marches;         /* marches that ran an AMR entry point, so far (0 on a volume that never had subgrids) */
} gvt_hip_volume_amr_info;
int gvt_hip_volume_get_amr_info(gvt_hip_volume *, gvt_hip_volume_amr_info *); /* synchronises */
/* ---- time-varying AMR volumes (additive: the ABI revision stays 6, no entry point above changes its rule; _update_samples[_typed] go
 *      on refusing a volume that has subgrids) ----
 * The next time step of an AMR volume on the SAME subgrid tree (parents, ratios, lo, cells, and so every size), in place: new samples
 * for the level-0 grid (samples; NULL with n_samples = 0 keeps them), for any of the subgrids (subgrid_samples[i], laid out as
 * _set_subgrids takes them; an entry NULL keeps that subgrid, subgrid_samples NULL with n_subgrids = 0 keeps them all), or for both.
 * flags: 0 (every pointer given is host memory) or GVT_HIP_UPDATE_DEVICE (every pointer given is device memory: no host round trip).
 * After the call the volume answers exactly like a volume freshly created from the resident samples -- the new ones where given, the
 * old ones elsewhere -- with the same _set_subgrids (same flags) and the same set_transfer / set_surfaces / set_lights / set_shading
 * calls: every ray bit of gvt_hip_volume_trace, every framebuffer bit of gvt_hip_volume_frame, _clipped, _frame_fused_amr and the
 * shadowed frames under GVT_HIP_VOLUME_ALLOW_AMR, value_min / value_max as numbers, n_blocks / n_blocks_empty.  Legal before any
 * _set_transfer: the tables are then built when the transfer function arrives.  Samples need not be finite.
 * WHAT STAYS.  Nothing a march reads is re-allocated: the level-0 samples, the subgrids' samples and tables, the skip table and the
 * surface skip words keep their addresses, so tracers, tops, queues and fused frames built around the volume keep working.
 * _get_amr_info reports the same n_subgrids, n_levels and subgrid_bytes; every counter goes on accumulating.
 * WHAT GOES STALE.  The light grid (as with _update_samples: _get_light_grid says current = 0 and the fog-shadowed frames refuse until
 * the next bake).  The occluder grid stays current: it depends on the meshes, the lights and the tree only.
 * RANGES AND TABLES.  The macro cells' merged ranges ("MACRO CELLS" above) are recomputed from everything resident, on the device: the
 * level-0 ranges by the kernel of _update_samples, then every subgrid's vertices merged into them by the min / max / not-finite rule of
 * the level-0 ranges (a vertex on a macro-cell boundary counts for both cells), then one download of 9 bytes per macro cell; the skip
 * table, the AMR cell words' skip bit and the surface skip words are rebuilt from them by the rule of _set_transfer and _set_surfaces.
 * The volume keeps no other copy of the subgrids' ranges, so a later _set_subgrids(n = 0) gives the plain volume of the current
 * level-0 samples.  The first update of a tree builds the merge's work list (freed with the tree; not part of subgrid_bytes).
 * REFUSALS, GVT_HIP_ERR_INVALID, the volume exactly as it was, all checked before the first byte moves: a null volume; a volume without
 * subgrids (its steps are gvt_hip_volume_update_samples'); samples with an n_samples that is not counts[0] * counts[1] * counts[2], or
 * NULL with a non-zero n_samples; subgrid_samples with an n_subgrids that is not the volume's count, or NULL with a non-zero
 * n_subgrids; nothing given at all (no level-0 samples and no subgrid entry); an unknown flag bit.
 * GVT_HIP_ERR_DEVICE (a HIP call failed part way): samples may already be replaced while ranges and tables are not; the volume is then
 * undefined until an update succeeds, and may only be updated again or destroyed.
 * The call waits for the calling context's stream first and returns when it is done; the caller serialises it against frames that use
 * the brick.  ms_out (may be NULL): time on the context's stream from the end of the uploads to the end of the update (ranges, their
 * download, the tables' rebuild on the host and their upload), as for _update_samples.
 * OUT OF SCOPE.  A step whose tree changes (regridding: _set_subgrids); typed voxels with subgrids; CENTRAL gradients on AMR volumes;
 * the Domain scheduler's volume backend. */
int gvt_hip_volume_update_amr(gvt_hip_volume *, const float *samples /* level 0; NULL: keep */, size_t n_samples /* the brick's vertex count, or 0 with NULL */,
                              const float *const *subgrid_samples /* NULL: keep all; an entry NULL: keep that subgrid */,
                              int n_subgrids /* the volume's subgrid count, or 0 with NULL */, uint32_t flags /* GVT_HIP_UPDATE_DEVICE: every pointer given is device memory */,
                              float *ms_out /* may be NULL */);

/* ---- volume domains across ranks: Tracer<DomainScheduler> taking the volume branch of shuffleRays (TracerBase.h:325-414,
 *      DomainTracer.h:148-496).  The bricks of one volume are spread over the ranks of a job (owner[brick] = rank); every rank holds a
 *      queue and a top-level box for EVERY brick and a gvt_hip_volume for the bricks it owns.  The queue of a brick a rank does not own
 *      is its outgoing list to that brick's owner.  The frame loop itself lives in the caller (gravit_amd/scheduler.py
 *      VolumeDomainTracer); the library supplies its four steps. ----
 * CONTRACT.  With ONE sample per pixel, for every assignment of bricks to ranks, every number of ranks and any interleaving of marches
 * and exchanges, the sum of the ranks' framebuffers equals the framebuffer of gvt_hip_volume_frame over the same bricks IN EVERY BIT,
 * and the bricks' counters (samples_marched, samples_gathered, crossings, shaded samples) sum to the one-rank frame's.  Why:
 *   - a ray keeps one sample lattice from brick to brick, and its whole state (colour, opacity, flags, side mask, t_min, t_max) lies in
 *     the 80-byte wire image, which the exchange moves unchanged (gvt_hip_queues_export_wire / _append_wire, state kept);
 *   - the march and the shuffle of a ray read that ray alone: neither its position in a queue, nor the rank, nor what else the launch
 *     holds enters its result;
 *   - a pixel has exactly one ray, so exactly one deposit, on the rank where the ray ends (OPAQUE or EXTERNAL): the composite adds that
 *     value to zeros, x + 0 = x.
 * With several samples per pixel the deposits of a pixel meet in float atomics in an unspecified order, as they do in the one-rank frame:
 * not bit-exact, and not promised.
 * OUT OF SCOPE.  A native frame loop over gvt_hip_comm for volumes; the clipped (mixed) frame across ranks; a ray marching through
 * several locally owned bricks inside one launch. */
/* Adapter::trace on a device-resident queue: the march of the queue's rays through the brick, in place, on the calling context's stream,
 * without a host wait -- what gvt_hip_volume_frame does per target, and the same kernels.  flags: GVT_HIP_MARCH_MAY_CLIP -- the queue may
 * hold rays that carry GVT_HIP_RAY_CLIP (without it the launch ignores that flag, as gvt_hip_volume_frame's does).  The rays stay in the
 * queue with their flags (OPAQUE / BOUNDARY) for gvt_hip_shuffle_volume.  An empty queue: nothing is launched.  A null argument, a volume
 * without a transfer function or an unknown flag bit: GVT_HIP_ERR_INVALID, nothing changed. */
#define GVT_HIP_MARCH_MAY_CLIP 1
int gvt_hip_volume_march_queue(gvt_hip_volume *, gvt_hip_queue *queue, const float minv[16], uint32_t flags);
/* shuffleDropRays for volumes (DomainTracer.h:148-183): the camera's rays, generated exactly as gvt_hip_volume_frame generates them (8x8
 * tiles, origins left at the eye: one lattice per ray), shuffled from -1 into queues[] (one per brick of the top, appended to).  A ray
 * whose first brick b has keep_mask[b] == 0 is dropped: that brick's owner generates the same ray.  A ray that meets no brick is dropped
 * everywhere.  keep_mask == NULL keeps everything.  A kept brick's queue receives the same rays in the same order as in the camera step
 * of gvt_hip_volume_frame; the other queues are not touched.  The framebuffer is not involved (a camera ray deposits nothing). */
int gvt_hip_volume_camera_filter(gvt_hip_top *, const gvt_hip_camera *cam, gvt_hip_queue *const *queues, const uint8_t *keep_mask /* n bricks, or NULL */);
/* The ray exchange's two ends, batched: ONE kernel launch for all the queues of a message, whatever n is (1..256).
 * _export_wire: the rays of queues[0], queues[1], ... laid end to end in dst_device (device memory, cap_rays rays of 80 bytes), byte
 * for byte what gvt_hip_queue_export(queues[i], ..., dst_on_device = 1) writes per queue; counts_out[i] (optional) = rays of queue i,
 * *total_out = their sum; the queues are cleared; waits for the stream, so the buffer is complete on return.  total > cap_rays:
 * GVT_HIP_ERR_CAPACITY, *total_out = the count needed, nothing changed.  A queue may appear once.
 * _append_wire: consecutive runs of counts[i] rays of src_device are appended to queues[i], state bytes 64..79 kept, the queues grown as
 * gvt_hip_queue_append grows them: the result of gvt_hip_queue_append(queues[i], run i, counts[i], 1) per queue.  No host wait; the
 * source must stay valid until the stream has passed the launch.
 * Null arguments (queues, an entry of it, total_out / counts, a buffer where rays exist) or n outside 1..256: GVT_HIP_ERR_INVALID. */
int gvt_hip_queues_export_wire(gvt_hip_queue *const *queues, size_t n, gvt_hip_ray *dst_device, size_t cap_rays, uint64_t *counts_out /* n, may be NULL */,
                               uint64_t *total_out);
int gvt_hip_queues_append_wire(gvt_hip_queue *const *queues, size_t n, const gvt_hip_ray *src_device, const uint64_t *counts /* n */);

/* ---- fused frame: every brick of a bricked volume marched in ONE launch (opt-in; gvt_hip_volume_frame stays the default) ----
 * gvt_hip_volume_frame renders a bricked volume brick by brick: one march launch, one three-kernel shuffle and one host wait per round.
 * The fused frame generates the camera's list once (gvt_hip_camera_generate_tiled into the context's staging list, as the loop does),
 * launches ONE kernel in which every lane carries its ray from brick to brick until it deposits, and waits for the host once.
 * CONTRACT.  The fused frame is DEFINED BY THE LOOP.  For every eligible input (below) with ONE sample per pixel, the framebuffer after
 * gvt_hip_volume_frame_fused equals the framebuffer after gvt_hip_volume_frame (depth == NULL) / gvt_hip_volume_frame_clipped on the
 * same arguments IN EVERY BIT; no tolerance applies.  Why: a ray's march and its next-brick decision read that ray alone, so the fused
 * ray passes through exactly the states the loop's ray passes through between its visits:
 *   - first brick: a camera ray starts with colour 0, opacity 0 and flags 0; under a depth plane with t_max = depth[id] and
 *     GVT_HIP_RAY_CLIP where that is below +Inf (the loop's scatter of fresh rays).  Its first brick is the shuffle's rule from -1 (the
 *     nearest box the ray enters, tn < t_max under the clip).  With no first brick the ray is dropped and deposits nothing;
 *   - visit of brick b: the lattice range of the ray in b's vertex box from the ray's current t_min (and its clip), then the plain
 *     march's per-sample steps -- the same device functions as gvt_hip_volume_trace's kernels, once in the source: cell ownership, the
 *     macro-cell test and its verified jump, the trilinear gather, the front-to-back accumulation; the arrives-opaque rule, the
 *     contiguity rule and the limit of 2^22 lattice positions per visit apply;
 *   - leaving b: t_min = (float)k_last * dt if the visit owned a sample, unchanged otherwise.  opacity >= GVT_HIP_VOLUME_OPAQUE_A ends
 *     the ray: it deposits.  Otherwise the shuffle's rule from b names the next brick; none (EXTERNAL): it deposits;
 *   - progress: the next visit's first lattice index comes from t_min on the float (the first k with k * dt > t_min), not from
 *     k_last + 1: one statement of the lattice;
 *   - deposit: four atomic adds (r, g, b, opacity) into the cleared framebuffer at the ray's pixel (id < width * height), as the shuffle
 *     deposits.  With samples > 1 a pixel's deposits meet in arrival order, as in the loop: not bit-exact, not promised.
 * ELIGIBILITY is decided at every call from the volumes' current state (no object is kept between frames): 1 <= n_inst <= 256; every
 * volume has a transfer function; all bricks have one voxel type; no brick has surfaces, subgrids or effective lit shading
 * (GVT_HIP_VOLUME_SHADE_GRADIENT with at least one light; the gradient kind is inert otherwise); and the bricks are bricks of ONE grid:
 * global origin, spacing, dt, the 256-entry table, the table's value range, the skip flag and the minv of every instance are equal as
 * bits across the bricks.  An ineligible call is NOT an error: the loop runs with the queues given and stats->fused = 0.
 * Argument errors are gvt_hip_volume_frame's / _clipped's (GVT_HIP_ERR_INVALID, nothing changed).
 * BRICKS UNDER A MATRIX (the loop, the clipped and the fused frame alike).  One brick is marched under any affine matrix.  SEVERAL bricks
 * need a matrix whose 3x3 block is a signed, scaled axis permutation (one non-zero entry per row and column; a diagonal block among
 * them): then the world box of a brick is the brick, and neighbours share a face.  Under a rotation by anything but a multiple of 90
 * degrees, or a shear, the world boxes of neighbouring bricks overlap, and the next-brick rule -- a brick is entered only if the ray
 * leaves it strictly later than it left the last one -- skips a brick whose box ends inside its neighbour's: samples are lost (measured
 * on the numpy restatement: up to 94 of 932 lit pixels of a 64 x 48 film differ from the one-brick frame, by up to 0.99).  The three
 * frame entry points refuse such a call (n_inst > 1) with GVT_HIP_ERR_INVALID.  The refusal looks at the matrices alone and is
 * conservative: it also refuses instances that are not bricks of one grid and whose world boxes happen to be disjoint, which would be
 * marched correctly.  gvt_hip_shuffle_volume, which sees boxes only, cannot refuse: a caller that drives the bricks itself (the Domain
 * scheduler's backend) must make the same check.
 * queues are used by the fallback only; a fused frame leaves them cleared.  The per-brick counters of the volumes (gvt_hip_volume_info's
 * samples_marched / samples_gathered) are NOT touched by a fused frame: its counters are the call's own, below.
 * Surfaces and lit shading are taken by gvt_hip_volume_frame_fused_shaded, below; this entry point keeps its rule.
 * OUT OF SCOPE.  Subgrids without GVT_HIP_FUSED_AMR and central gradients without GVT_HIP_FUSED_CENTRAL, both below (such frames take the loop); bricks of
 * different grids, tables or matrices; the Domain scheduler (a rank fusing the bricks it owns needs rays that leave for foreign bricks
 * appended to outgoing queues inside the kernel); fused as the default. */
typedef struct {
  uint32_t fused;            /* 1: the fused kernel ran; 0: the loop did (the frame was not eligible) */
  uint32_t pad;
  uint64_t samples_marched;  /* fused: the sums over the bricks of what the loop adds to each brick's gvt_hip_volume_info for the same */
  uint64_t samples_gathered; /*        frame; 0 after the loop (the bricks' own counters moved instead) */
  uint64_t brick_visits;     /* fused: (ray, brick) visits = the sum of the loop's queue sizes over its rounds; 0 after the loop */
  uint64_t rays_deposited;   /* fused: deposits; 0 after the loop */
  uint64_t adapter_calls;    /* march launches: 1 for a fused frame, the loop's count otherwise */
} gvt_hip_volume_fused_stats;
int gvt_hip_volume_frame_fused(gvt_hip_top *, gvt_hip_volume *const *volumes, const float *m /* n_inst*16 */, const float *minv, size_t n_inst,
                               const gvt_hip_camera *cam, gvt_hip_queue *const *queues, gvt_hip_fb *fb, const gvt_hip_depth *depth /* may be NULL */,
                               gvt_hip_volume_fused_stats *stats /* may be NULL */);

/* ---- fused frame: surfaces and lit fog (a further opt-in beside gvt_hip_volume_frame_fused, whose rule does not change) ----
 * allow: which frames beyond the plain ones the fused kernel may take.  allow == 0 is gvt_hip_volume_frame_fused in every respect.
 * Bits other than the three below (4 among them): GVT_HIP_ERR_INVALID, nothing changed.  Argument errors are gvt_hip_volume_frame's / _clipped's.
 * ELIGIBILITY is gvt_hip_volume_frame_fused's with two clauses relaxed: "no brick has surfaces" is dropped with
 * GVT_HIP_FUSED_SURFACES, "no effective lit shading" with GVT_HIP_FUSED_LIT.  What the bricks must share is then compared as bits
 * too: n_iso, n_pl, the isovalues, the planes and the surfaces' opacity; the number of lights, their positions and colours, ka, kd and
 * the shading mode.  Still ineligible -- the loop runs, fused = 0, no error: subgrids on any brick (this entry point refuses the bit
 * that would take them, GVT_HIP_FUSED_AMR of gvt_hip_volume_frame_fused_amr below); without GVT_HIP_FUSED_CENTRAL,
 * GVT_HIP_VOLUME_GRADIENT_CENTRAL on any brick of a frame that has an isovalue or effective lit shading (in a frame that has neither
 * -- no isovalue and no lit shading, or planes only -- the kind stays inert, as ever, whatever the bit); a frame that needs a bit
 * `allow` lacks; everything ineligible above.
 * GVT_HIP_FUSED_CENTRAL drops the gradient clause for frames in which EVERY brick has the same kind: a frame that has an isovalue or
 * effective lit shading and whose bricks are all CENTRAL is then eligible and is marched by the CENTRAL instantiation of the kernel,
 * which shades with the gradient of "smooth gradients" above from the bricks' ghost layers; features carries the bit exactly when that
 * instantiation ran.  Such a frame's bricks must also agree, as bits, on the global grid's vertex counts (global_counts at creation: where
 * the one-sided differences lie); bricks that do not take the loop, or are refused by the shadowed frames ("central" in the message).  A frame that mixes CELL and CENTRAL bricks takes the loop, with or without the bit, and with the bit a frame of
 * CELL bricks launches what it launches without it.  central_marches of the bricks (gvt_hip_volume_get_gradient) keeps its meaning:
 * it counts per-volume launches of the LOOP's march and does not move in a fused frame.
 * CONTRACT.  As above: for every eligible input at one sample per pixel the framebuffer equals gvt_hip_volume_frame's / _clipped's on the
 * same arguments in every bit.  The visit of a brick is the surface / lit march's (the crossings of a sample composited in front of it,
 * the sample shaded by the cell gradient), and between two visits the ray carries what the loop's ray carries: beyond t_min, colour and
 * opacity, the side mask of its last owned sample with GVT_HIP_RAY_SIDES once a visit has owned one (a camera ray carries none; a visit
 * that owns no sample leaves mask, flag and t_min as they were).  On entering a brick the mask counts only for the sample right after
 * the one in t_min (the first lattice index after t_min); at any other first sample the ray has no previous sides.
 * A frame that has neither surfaces nor lit shading launches the plain fused kernel (features = 0).  The bricks' own counters
 * (gvt_hip_volume_info, gvt_hip_volume_get_crossings, gvt_hip_volume_get_shaded) are not touched by a fused frame.  samples > 1:
 * arrival order, as in the loop. */
#define GVT_HIP_FUSED_SURFACES 1u   /* the fused kernel may take frames whose bricks have isovalues / slice planes */
#define GVT_HIP_FUSED_LIT      2u   /* ... and frames with effective lit shading (SHADE_GRADIENT and >= 1 light)   */
#define GVT_HIP_FUSED_CENTRAL  8u   /* ... and such frames whose bricks all have GVT_HIP_VOLUME_GRADIENT_CENTRAL (bit 2, value 4, stays undefined and refused, as it was) */
typedef struct {
  uint32_t fused;      /* as gvt_hip_volume_fused_stats */
  uint32_t features;   /* bits of the kernel that ran: 0 = the plain fused kernel, or the loop */
  uint64_t samples_marched, samples_gathered, brick_visits, rays_deposited, adapter_calls;
  uint64_t crossings_rendered;  /* fused: the sum of what the loop adds to the bricks' gvt_hip_volume_get_crossings; 0 after the loop */
  uint64_t samples_shaded;      /* fused: likewise for gvt_hip_volume_get_shaded */
} gvt_hip_volume_fused_shaded_stats;
int gvt_hip_volume_frame_fused_shaded(gvt_hip_top *, gvt_hip_volume *const *volumes, const float *m, const float *minv, size_t n_inst,
                                      const gvt_hip_camera *cam, gvt_hip_queue *const *queues, gvt_hip_fb *fb,
                                      const gvt_hip_depth *depth /* may be NULL */, uint32_t allow,
                                      gvt_hip_volume_fused_shaded_stats *stats /* may be NULL */);

/* ---- fused frame: AMR bricks (one more opt-in; additive: the ABI revision stays 6, no entry point above changes its rule) ----
 * gvt_hip_volume_frame_fused_amr is gvt_hip_volume_frame_fused_shaded with one more allow bit.  It is an entry point of its own because
 * the caller allocates the stats struct, which has to grow.  allow: GVT_HIP_FUSED_SURFACES | _LIT | _CENTRAL | _AMR; any other bit (4
 * among them): GVT_HIP_ERR_INVALID ("allow" in the message), nothing changed.  Without GVT_HIP_FUSED_AMR the call is
 * gvt_hip_volume_frame_fused_shaded in every respect, and samples_refined and amr_bricks are 0.  gvt_hip_volume_frame_fused_shaded
 * goes on refusing bit 16.
 * ELIGIBILITY, decided per call from the volumes' current state: GVT_HIP_FUSED_AMR drops the clause "no brick has subgrids" and nothing
 * else -- one grid, table, matrix and voxel type, surfaces and lights equal as bits, the allow bits the frame needs and the gradient
 * clauses stay.  Subgrids exist on float32 CELL volumes only and take surfaces and lit shading only when set with
 * GVT_HIP_VOLUME_AMR_SHADED (the setters see to both).  A frame that MIXES bricks with and without subgrids is the normal case and is
 * eligible.  A frame that reads a gradient (an isovalue, or effective lit shading) and mixes bricks with subgrids with CENTRAL bricks is
 * a frame of mixed kinds: the loop, with every bit set.  An ineligible frame is not an error: the loop runs, fused = 0.  A frame in which
 * no brick has subgrids launches exactly what gvt_hip_volume_frame_fused_shaded launches; features carries GVT_HIP_FUSED_AMR exactly
 * when an AMR instantiation of the kernels ran.
 * CONTRACT.  The fused frame's: for every eligible input at one sample per pixel the framebuffer equals gvt_hip_volume_frame's /
 * _clipped's on the same arguments in every bit.  The visit of a brick that has subgrids is the AMR march's per-sample sequence ("AMR
 * volumes" above): the skip bit from the brick's AMR cell word (with surfaces: from its per-cell word, built from the merged ranges),
 * the descent between the skip decision and the gather, the gather, the corners and the spacing of the FINAL grid.  The visit of a
 * brick without subgrids is what the fused kernels do today.  Between two visits the ray carries what it carries in the fused frames
 * above; the descent adds no state to a ray.  The bricks' AMR tables are read from the volumes at every call: a _set_subgrids between
 * two frames is seen by the next one.
 * COUNTERS.  The bricks' own counters (gvt_hip_volume_info, _get_crossings, _get_shaded, and _get_amr_info's samples_refined and
 * amr_marches) are not touched by a fused frame.  samples_refined below is the sum of what the loop would have added to the bricks'
 * samples_refined for the same frame.
 * OUT OF SCOPE.  The shadowed, fog-shadowed and mesh-shadowed frames and both bakes on bricks with subgrids (they go on refusing);
 * CENTRAL gradients on AMR volumes; typed voxels with subgrids; the Domain scheduler; fused as the default.  (In-place updates of AMR volumes: gvt_hip_volume_update_amr.) */
#define GVT_HIP_FUSED_AMR 16u       /* the fused kernels may take frames in which some or all bricks have subgrids */
typedef struct {
  uint32_t fused, features;  /* the fields of gvt_hip_volume_fused_shaded_stats, same order and meaning */
  uint64_t samples_marched, samples_gathered, brick_visits, rays_deposited, adapter_calls;
  uint64_t crossings_rendered, samples_shaded;
  uint64_t samples_refined;  /* fused with GVT_HIP_FUSED_AMR in features: gathered samples whose final grid was a subgrid; 0 otherwise */
  uint32_t amr_bricks;       /* ... and the bricks of the frame that had subgrids; 0 otherwise */
  uint32_t pad;
} gvt_hip_volume_fused_amr_stats;
int gvt_hip_volume_frame_fused_amr(gvt_hip_top *, gvt_hip_volume *const *volumes, const float *m, const float *minv, size_t n_inst,
                                   const gvt_hip_camera *cam, gvt_hip_queue *const *queues, gvt_hip_fb *fb,
                                   const gvt_hip_depth *depth /* may be NULL */, uint32_t allow,
                                   gvt_hip_volume_fused_amr_stats *stats /* may be NULL */);

/* ---- shadowed surfaces: shadow rays marched inside the fused frame (additive: the ABI revision stays 6, no entry point above changes) ----
 * gvt_hip_volume_frame_shadowed is the shaded fused frame in which a crossing is lit only by the light that reaches it.  A shadow ray
 * crosses bricks; it is marched to its end by the lane whose camera ray needs it, inside the one launch, so a pixel keeps ONE writer
 * and the image stays the same bits however the volume is bricked.
 * INERT.  A frame in which no brick has a surface, or no brick has a light, cannot show a shadow: the call is then
 * gvt_hip_volume_frame_fused_shaded with allow = GVT_HIP_FUSED_SURFACES | GVT_HIP_FUSED_LIT in every respect, its fallback to the loop
 * included; shadowed = 0 and the shadow counters are 0.
 * REFUSED.  A frame that has a surface and a light but is not eligible for the shaded fused kernel under that allow word (subgrids;
 * GVT_HIP_VOLUME_GRADIENT_CENTRAL on a brick of a frame with an isovalue, unless flags allows it, below; bricks of different grids,
 * tables, matrices, surfaces or lights; more than 256 bricks): no loop renders shadows, so the call returns GVT_HIP_ERR_INVALID with a
 * message that names the clause.  A null params pointer, flag bits other than GVT_HIP_VOLUME_ALLOW_CENTRAL and GVT_HIP_VOLUME_ALLOW_AMR
 * (the accepted words are 0, 2, 4 and 6; "flag" in the message) and a bias outside 1 .. 64 are refused likewise.
 * CENTRAL.  flags = GVT_HIP_VOLUME_ALLOW_CENTRAL (the first defined bit of the flags word of gvt_hip_volume_shadow_params,
 * gvt_hip_volume_light_grid_params and gvt_hip_volume_occluder_params; bit 0 stays undefined and refused) adds GVT_HIP_FUSED_CENTRAL
 * to the allow word of the three shadowed frames, the inert forward included: a frame whose bricks are ALL CENTRAL is accepted, a frame
 * that mixes the kinds is refused (the message says "central"), and a frame of CELL bricks launches what it launches with flags = 0.
 * The contract changes in one place: the g that shades a crossed isovalue and a lit fog sample is vol_gradient_central's ("smooth
 * gradients").  T_j, Tg, Og, every counter and the opacity do not depend on g.  So the alpha plane and every counter -- the camera
 * rays' and the shadow rays' -- of a CENTRAL shadowed frame equal those of the same frame with the bricks switched to CELL; only the
 * colour planes differ.  The two bakes accept CENTRAL bricks under the flag and write the bits they write for the same bricks under
 * CELL: their rays march with shading NONE and read no gradient.  Neither gvt_hip_volume_set_gradient nor gvt_hip_volume_set_ghosts
 * makes a light grid or an occluder grid stale.  A refusal changes nothing: the framebuffer is not
 * cleared, the queues are untouched.  Argument errors are gvt_hip_volume_frame's / _clipped's.
 * CONTRACT.  The shadowed frame is the shaded fused frame with one change.  At a lattice sample k of a camera ray at which at least one
 * crossing is rendered, a transmittance T_j is found once per light j before the first crossing is composited; all crossings of that
 * sample share it, and the light loop of the crossing's shading becomes
 *     ndl_s = ndl * T_j;   sum[a] = sum[a] + lcol[j][a] * ndl_s;
 * Everything else is as it was: the len > 0 rule, ka + kd * sum, f, C and A.  Lit fog samples are lit as before and are NOT shadowed.
 * T_j is defined by the contract that exists.  The shadow ray has the world origin wp[a] = wo[a] + wd[a] * t with t = (float)k * dt (the
 * world ray as it stands in the camera's list), the world direction ws_j = lpos_j / sqrt((x*x + y*y) + z*z) computed on the host in
 * float32 (the lights are directional; this is the direction towards the light), t_min = (float)(bias - 1) * dt, and no colour, no
 * opacity, no flags and no clip.  Let A_s be the opacity this ray would deposit as a camera ray of the shaded fused frame over the same
 * bricks with the same surfaces and shading mode NONE -- its first brick by the next-brick rule from none, the surface visits, the
 * carried side mask, the arrives-opaque rule, the contiguity rule, the 2^22 limit, GVT_HIP_VOLUME_OPAQUE_A ending it, exits growing
 * from hop to hop.  Then T_j = 1 - A_s.  A ray that meets no brick has A_s = 0.  A light whose ws_j is zero or not finite casts no ray:
 * its T_j = 1.  (Opacity never depends on colour in the march, so the kernel runs its own visit with the colour dead.)
 * CONSEQUENCES.  The image is the same bits for every bricking and with or without macro-cell skipping: wp, ws_j and every shadow sample
 * are functions of global vertex values.  With T_j = 1 everywhere the bits are gvt_hip_volume_frame_fused_shaded's.  Where every T_j = 0
 * a pixel has the bits of the same frame rendered with kd = 0.
 * DEVIATIONS.  (1) A surface is rendered at the far sample of its step, so a shadow ray towards a light on the camera's side would
 * cross its own sheet again; bias is the remedy: the first shadow sample is lattice index `bias`, and a first sample has no previous
 * sides, so nothing within `bias` steps casts a shadow.  (2) The geometry of a mixed frame casts no shadow into the volume in THIS frame: the depth
 * plane clips camera rays only (gvt_hip_volume_frame_mesh_shadowed below lets it).  (3) The fog is not shadowed (gvt_hip_volume_frame_fog_shadowed below shadows it).  (4) At samples > 1
 * deposits meet in arrival order, as ever.  (5) A shadow ray that runs IN a face two bricks share -- its origin on the face, ws_j with a
 * zero component along the face's axis -- has its samples owned by one of the two bricks (cell floor), while the next-brick rule enters
 * a brick only if the ray leaves it strictly later than it left the last one; the two neighbours share their exit, so the owner is
 * skipped after the non-owner and those samples are lost: A_s then depends on the bricking.  For crossing points this is a measure-zero
 * case and the rule is kept; for rays from grid vertices under an axis-aligned light it is systematic, and the light grids below are
 * defined and walked otherwise.
 * COUNTERS.  shadow_rays = (samples with at least one rendered crossing) x (lights with a usable ws_j); shadow_brick_visits,
 * shadow_crossings and shadow_samples_marched / _gathered are the fused frame's counters applied to the shadow rays.  They are kept
 * apart from the camera rays' counters, which equal those of the unshadowed frame whenever the two images agree.
 * OUT OF SCOPE.  Ambient occlusion in this frame (see "ambient occlusion" below); shadowed fog and geometry shadowing the volume (both below); the volume attenuating mesh shadow rays; the Domain
 * scheduler (a rank does not hold the foreign bricks a shadow ray needs); AMR frames without GVT_HIP_VOLUME_ALLOW_AMR, and CENTRAL
 * frames without GVT_HIP_VOLUME_ALLOW_CENTRAL; shadows in the per-brick loop.
 *
 * ---- shadows on AMR bricks (additive: one more flag bit; no struct changes size, no entry point is added, the ABI revision stays 6) ----
 * flags | GVT_HIP_VOLUME_ALLOW_AMR (the second defined bit of the same word) adds GVT_HIP_FUSED_AMR to the allow word of the three
 * shadowed frames, the inert forward included (which then is gvt_hip_volume_frame_fused_amr's path), and drops the clause "no brick has
 * subgrids" -- and nothing else -- from the eligibility of the two bakes.  Without the bit every call answers as it did, message for
 * message.  A frame in which no brick has subgrids launches exactly what it launches with the bit clear (flags 6 on an all-CENTRAL
 * frame without subgrids is flags 2).  A brick with subgrids is float32 and CELL: a frame that reads a gradient and mixes such bricks
 * with CENTRAL bricks is refused by the mixed-kinds clause ("central" in the message), whatever the flags.  features of
 * gvt_hip_volume_shadow_stats carries GVT_HIP_FUSED_AMR exactly when an AMR instantiation ran.  Refined samples are NOT reported by the
 * shadowed frames: the stats struct has no field for them (gvt_hip_volume_frame_fused_amr counts them for the unshadowed frame).
 * CONTRACT.  T_j on AMR bricks is defined by the contract that exists: T_j = 1 - A_s, A_s the opacity the shadow ray would deposit as a
 * camera ray of gvt_hip_volume_frame_fused_amr over the same bricks with the same surfaces and shading NONE.  The shadow ray therefore
 * takes the AMR visit: the skip decision from the per-cell word built from the MERGED ranges (every level's vertices in the macro
 * cell), then the descent, then the final grid's value.  The camera ray's crossing is shaded as the fused AMR frame shades it -- the
 * final cell's corners, the descended fractions, the final grid's spacing -- with the one change above: ndl * T_j.
 * LIGHT GRID.  G_j stays a float32 plane at the brick's own LEVEL-0 vertices: "a light grid never covers subgrids" remains true of its
 * resolution.  Its rays start at level-0 vertices and are marched over the whole grid with all its subgrids as one brick, by the
 * ownership walk of "shadowed fog", with the AMR visit on bricks that have subgrids.  The planes are the one brick's bits for every
 * bricking that keeps each level-1 subgrid in one brick (the AMR sections' condition).
 * Tg AND Og IN THE FRAME are interpolated at the sample's level-0 cell c with its level-0 fractions -- the fractions BEFORE the descent
 * replaces them -- while the gradient that shades the sample is the final cell's.  DEVIATION: a shadow's edge on the fog is one LEVEL-0
 * cell soft on an AMR brick too, however fine the cell that is shaded.
 * OCCLUDER GRID.  The bake reads no sample; only its gate changes.  O stays at level-0 vertices.
 * STALENESS is unchanged: gvt_hip_volume_set_subgrids makes both grids of the brick stale.
 * CONSEQUENCES.  The same bits for every admissible bricking, and with or without macro-cell skipping.  With every T_j = 1 the bits are
 * gvt_hip_volume_frame_fused_amr's.  Where every light is blocked the bits are the kd = 0 frame's.  With no mesh the mesh-shadowed
 * frame has the fog-shadowed frame's bits.
 * OUT OF SCOPE.  CENTRAL gradients or typed voxels on AMR volumes; light or occluder planes at subgrid resolution;
 * refined-sample counters in the shadow stats; shadows across ranks. */
#define GVT_HIP_VOLUME_ALLOW_CENTRAL 2u /* flags of the shadowed frames and the two bakes: accept frames whose bricks are all CENTRAL */
#define GVT_HIP_VOLUME_ALLOW_AMR 4u     /* ... accept frames in which some or all bricks have AMR subgrids ("shadows on AMR bricks") */
typedef struct {
  uint32_t flags; /* 0, or GVT_HIP_VOLUME_ALLOW_CENTRAL and GVT_HIP_VOLUME_ALLOW_AMR ORed */
  int32_t bias;   /* 1 .. 64, lattice steps */
} gvt_hip_volume_shadow_params;
typedef struct {
  uint32_t fused, features;  /* the fields of gvt_hip_volume_fused_shaded_stats, same order and meaning (the camera rays' counters) */
  uint64_t samples_marched, samples_gathered, brick_visits, rays_deposited, adapter_calls;
  uint64_t crossings_rendered, samples_shaded;
  uint32_t shadowed;         /* 1: the shadow kernel ran; 0: shadows were inert (above) */
  uint32_t pad;
  uint64_t shadow_rays, shadow_brick_visits, shadow_crossings, shadow_samples_marched, shadow_samples_gathered;
} gvt_hip_volume_shadow_stats;
int gvt_hip_volume_frame_shadowed(gvt_hip_top *, gvt_hip_volume *const *volumes, const float *m, const float *minv, size_t n_inst,
                                  const gvt_hip_camera *cam, gvt_hip_queue *const *queues, gvt_hip_fb *fb,
                                  const gvt_hip_depth *depth /* may be NULL */, const gvt_hip_volume_shadow_params *params,
                                  gvt_hip_volume_shadow_stats *stats /* may be NULL */);

/* ---- shadowed fog: light transmittance grids baked on the device (additive: the ABI revision stays 6, no entry point above changes) ----
 * Marching a shadow ray per light at every lit fog sample would multiply the frame by hundreds.  Instead the transmittance towards each
 * light is computed ONCE at every grid vertex (gvt_hip_volume_light_grid_bake), kept on the device beside the samples and interpolated
 * at each lit sample (gvt_hip_volume_frame_fog_shadowed).  It is rebuilt when the data, the table, the surfaces or the lights change,
 * not when the camera moves.
 * THE GRID.  For a frame of bricks of ONE grid, every usable light j (ws_j finite and not zero, as above) has a float32 value G_j at
 * every global vertex I = (I0, I1, I2):
 *   p[a] = origin[a] + (float)I[a] * spacing[a]                      object space: one multiply, one add
 *   wp   = (m[r]*p.x + m[4+r]*p.y) + (m[8+r]*p.z + m[12+r]*1)         m applied as a point
 *   the ray: origin wp, direction ws_j, t_min = (float)(bias - 1) * dt, no colour, no opacity, no flags, no clip
 *   A_s  = the opacity this ray deposits when it is marched over the WHOLE grid as ONE brick (offset 0, counts = global_counts) with
 *          the frame's surfaces and shading NONE
 *   G_j(I) = 1 - A_s
 * For every ray on which the walk of "shadowed surfaces" is bricking-invariant this is that section's T_j; for a ray in a brick face
 * (DEVIATIONS (5) there) it pins the value down.  The bake gives these bits for every bricking: its walk is driven by sample ownership.
 * The lattice range is taken once from the global vertex box; the next visit goes to the brick that owns the global cell of the first
 * lattice index after t_min; a visit ends by the contiguity rule; the ray ends when that cell lies outside the grid (the one brick's
 * rules: before its first sample the next index is tried, after it the ray is over) or when A >= GVT_HIP_VOLUME_OPAQUE_A.  The side
 * mask is carried from visit to visit.  A brick stores G_j at its own vertices, the shared layers twice with the same bits.  An
 * unusable light has no grid; its transmittance is 1.
 * THE BAKE.  Eligibility is the shaded fused frame's "bricks of one grid" comparison (allow = both bits) and, on top of it: m equal as
 * bits on every brick; surfaces and lights equal on every brick whatever the shading; at least one usable light; no subgrids; no
 * CENTRAL kind on a brick of a frame with an isovalue or lit shading unless flags is GVT_HIP_VOLUME_ALLOW_CENTRAL and every brick has
 * it; the bricks' owned cells tile the global grid exactly (disjoint, and their sum is
 * the global cell count); at most 2^32 - 1 (vertex, light) pairs; flags 0 or that bit; bias 1 .. 64; no null pointer.  Anything else:
 * GVT_HIP_ERR_INVALID with a message that names the clause, the old grids kept.  Planes that cannot be allocated: GVT_HIP_ERR_CAPACITY;
 * a HIP call that fails: GVT_HIP_ERR_DEVICE; in both cases every brick keeps the grid it had (all planes are allocated and filled
 * before the first brick changes).  The call waits for the launch.
 * CURRENT.  A frame's grids are current if ONE bake covered exactly these volumes in this order with the same m and minv bits, and since
 * then no brick has had _update_samples[_typed], _set_transfer, _set_surfaces, _set_lights or _set_subgrids.  _set_shading and
 * _set_gradient do not make a grid stale: shadow rays march with shading NONE.
 * THE FRAME.  gvt_hip_volume_frame_fog_shadowed is gvt_hip_volume_frame_shadowed -- same arguments, same refusals, crossings lit
 * through exact in-kernel shadow rays with the bias of its params -- with one more change.  In a lit fog sample that is shaded
 * (tc.w > 0, 0 < len < +Inf) the light loop becomes
 *     Tg = trilinear interpolation of G_j at the cell's eight vertices (the sample's fractions; the value's nesting: x, then y, then z)
 *     ndl_s = ndl * Tg;   sum[a] = sum[a] + lcol[j][a] * ndl_s;
 * with Tg = 1 and nothing read for an unusable light.  G is read only inside that branch, so skipping stays exact against
 * GVT_HIP_VOLUME_NO_SKIP and samples_shaded does not change; A never depends on G.  The frame takes the depth plane as its siblings do.
 * INERT.  No light, or neither surfaces nor effective lit shading: gvt_hip_volume_frame_fused_shaded with both allow bits.  Surfaces and
 * lights but no effective lit shading: gvt_hip_volume_frame_shadowed with the same bias in every bit; no grid is needed.
 * REFUSED (GVT_HIP_ERR_INVALID, the message names the clause, nothing changed, the framebuffer not cleared): everything
 * gvt_hip_volume_frame_shadowed refuses -- with lit fog alone a frame that is not eligible for the fused kernel is refused too, no loop
 * shadows fog -- and a frame with effective lit shading and a usable light whose bricks do not all hold a CURRENT grid ("light grid").
 * DEVIATIONS.  (1) Transmittance is interpolated from vertices: a shadow's edge is one cell soft, and an occluder thinner than a cell
 * leaks.  (2) Crossings keep exact rays, so the two kinds of shadow meet at slightly different softness.  (3) Meshes cast no shadow
 * into the volume in this frame (gvt_hip_volume_frame_mesh_shadowed below).  (4) The grid's bias is the bake's, the crossings' bias the frame's.
 * COUNTERS.  Bake: rays = (vertices summed over the bricks) x (usable lights); samples_marched / _gathered and crossings as the fused
 * frames count them; bytes = the planes' size; ms = the launch's event time.  Frame: gvt_hip_volume_shadow_stats, and
 * fog_samples_shadowed = samples_shaded when the fog kernel ran (else 0).
 * A volume that holds a grid renders through every other entry point with the bits it had.  gvt_hip_volume_destroy frees the grid.
 * OUT OF SCOPE.  A coarser or compressed grid; pruning vertices no sample reads; ambient occlusion in this frame (see "ambient occlusion" below); the
 * Domain scheduler; AMR frames, and CENTRAL frames without GVT_HIP_VOLUME_ALLOW_CENTRAL ("shadowed surfaces", CENTRAL); moving the
 * crossings' shadow rays onto the grid. */
typedef struct {
  uint32_t flags; /* 0, or GVT_HIP_VOLUME_ALLOW_CENTRAL and GVT_HIP_VOLUME_ALLOW_AMR ORed */
  int32_t bias;   /* 1 .. 64, lattice steps */
} gvt_hip_volume_light_grid_params;
typedef struct {
  uint64_t rays, samples_marched, samples_gathered, crossings, bytes;
  float ms;
  uint32_t pad;
} gvt_hip_volume_light_grid_stats;
typedef struct {
  uint32_t present, current; /* a grid is held | ... and no call has made it stale since its bake */
  int32_t n_planes, bias;    /* usable lights at the bake | the bake's bias */
  uint64_t bytes;
} gvt_hip_volume_light_grid_state;
typedef struct {
  gvt_hip_volume_shadow_stats frame; /* the shadowed frame's counters, same meaning */
  uint64_t fog_samples_shadowed;
} gvt_hip_volume_fog_shadow_stats;
int gvt_hip_volume_light_grid_bake(gvt_hip_volume *const *volumes, const float *m, const float *minv, size_t n_inst,
                                   const gvt_hip_volume_light_grid_params *params, gvt_hip_volume_light_grid_stats *stats /* may be NULL */);
/* out: host memory, counts[0] * counts[1] * counts[2] floats at i + nx * (j + ny * k).  No grid, or a light that was unusable at the
 * bake: GVT_HIP_ERR_INVALID.  A stale grid can still be downloaded. */
int gvt_hip_volume_light_grid_download(gvt_hip_volume *, int light, float *out);
int gvt_hip_volume_light_grid_info(gvt_hip_volume *, gvt_hip_volume_light_grid_state *out);
int gvt_hip_volume_light_grid_release(gvt_hip_volume *); /* frees the planes; a volume without a grid: 0 */
int gvt_hip_volume_frame_fog_shadowed(gvt_hip_top *, gvt_hip_volume *const *volumes, const float *m, const float *minv, size_t n_inst,
                                      const gvt_hip_camera *cam, gvt_hip_queue *const *queues, gvt_hip_fb *fb,
                                      const gvt_hip_depth *depth /* may be NULL */, const gvt_hip_volume_shadow_params *params,
                                      gvt_hip_volume_fog_shadow_stats *stats /* may be NULL */);

/* ---- meshes shadowing the volume: occluder grids baked on the device (additive: the ABI revision stays 6, no entry point above changes) ----
 * The two halves of a mixed frame now agree about light: whether a mesh stands between a point of the volume and a light is computed
 * ONCE at every grid vertex (gvt_hip_volume_occluder_grid_bake), kept beside the samples as uint8 planes and interpolated wherever the
 * fog-shadowed frame uses a transmittance (gvt_hip_volume_frame_mesh_shadowed).
 * THE GRID.  For a frame of bricks of ONE grid, every usable light j (ws_j finite and not zero, as in "shadowed surfaces") has a uint8
 * value O_j at every global vertex I:
 *   wp     = the vertex in world space, exactly as "shadowed fog" computes it (p[a] = origin[a] + (float)I[a] * spacing[a]; m as a point)
 *   the ray: origin wp, direction ws_j, t_min = GVT_RAY_EPSILON, no far limit (the words of an object-space query, gvt_hip_occluded)
 *   taken into every mesh instance i by that instance's minv, exactly as gvt_hip_depth_render's rays are
 *   O_j(I) = 0 if the any-hit traversal reports a hit in at least one instance, else 1
 * A brick stores O_j at its own vertices, at the samples' own index: one plane per usable light in the order of their bits, the shared
 * layers twice with the same bits.  An unusable light has no plane; its factor is 1.  O does not depend on the volume's data, table or
 * surfaces; (float)O is exact, and the planes take a quarter of a light grid's memory.
 * THE BAKE.  Eligibility is gvt_hip_volume_light_grid_bake's, clause for clause (the library checks both through one function), without
 * the bias.  n_mesh_inst == 0 is allowed: every O is 1 and no traversal is launched.  A null mesh among the instances is refused.
 * Refusals: GVT_HIP_ERR_INVALID, the message names the clause.  Planes that cannot be allocated: GVT_HIP_ERR_CAPACITY.  A HIP call that
 * fails, or the traversal's overflow word: GVT_HIP_ERR_DEVICE.  In every failing case each brick keeps the occluder grid it had (all
 * planes are allocated and filled before the first brick changes).  The call waits for its last launch.  The work is done in chunks of
 * (vertex, light) pairs: one kernel writes the chunk's rays, one any-hit launch per mesh instance runs over them, each followed by a
 * fold (O &= !flag), and one kernel packs the chunk into the bricks' planes.
 * CURRENT.  A frame's occluder grids are current if ONE bake covered exactly these volumes in this order with the same m and minv bits
 * and since then no brick has had _set_lights or _set_subgrids.  _update_samples[_typed], _set_transfer, _set_surfaces, _set_shading and
 * _set_gradient do NOT make them stale.  THE LIBRARY CANNOT SEE A MESH MOVE: the caller bakes again after gvt_hip_mesh_update_vertices,
 * gvt_hip_top_update or any change of the instance matrices.
 * THE FRAME.  gvt_hip_volume_frame_mesh_shadowed is gvt_hip_volume_frame_fog_shadowed -- same arguments, same refusals, crossings lit
 * through exact in-kernel shadow rays -- with one more change.  At a sample whose cell is c and whose fractions are f, for every usable
 * light
 *     Og = trilinear interpolation of (float)O_j at the cell's eight vertices (the sample's c and f; nesting x, then y, then z)
 *     lit fog sample:        ndl_s = ndl * (Tg * Og)
 *     crossing at sample k:  ndl_s = ndl * (T_j * Og)     Og from sample k's own cell, the sample at which the crossing is rendered
 * with Og = 1 and nothing read for an unusable light.  O is read only where G or T_j is used; A never depends on O, and no shadow ray
 * is cast or skipped because of O, so every counter of gvt_hip_volume_fog_shadow_stats equals the fog-shadowed frame's and skipping stays
 * exact against GVT_HIP_VOLUME_NO_SKIP.  A frame with surfaces but no effective lit shading needs no light grid, as today.
 * INERT.  No usable light, or neither surfaces nor effective lit shading: the call is gvt_hip_volume_frame_fog_shadowed in every respect;
 * no occluder grid is needed.
 * REFUSED (GVT_HIP_ERR_INVALID, the message names the clause, nothing changed, the framebuffer not cleared): everything the fog-shadowed
 * frame refuses, and a frame that is not inert and whose bricks do not all hold a CURRENT occluder grid ("occluder grid").
 * CONSEQUENCES.  With every O = 1 (no mesh, or meshes outside every vertex ray) the bits are the fog-shadowed frame's.  Where every O of
 * a sample's cell is 0 for every light -- and that holds for every shaded sample of the pixel -- the pixel has the bits of the same
 * frame rendered with kd = 0.  The image is the same bits for every bricking and with or without skipping.
 * DEVIATIONS.  (1) Mesh shadows are interpolated from vertices: one cell soft, and an occluder thinner than a cell leaks -- on crossings
 * too, where the volume's own shadows are exact.  (2) The volume's lights are directional and the scene's own lights are not; the mesh
 * frame is untouched, so the fog neither attenuates mesh shadow rays nor shades the meshes.  (3) The mesh frame's framebuffer keeps its
 * bits.
 * COUNTERS.  Bake: rays = (vertices summed over the bricks) x (usable lights); rays_blocked = those with O = 0; any_hit_launches;
 * bytes = the planes' size; ms = the event time from the first to the last launch.  Frame: the fog-shadowed frame's, and mesh_shadowed
 * = 1 when the mesh kernel ran (0: inert).
 * A volume that holds an occluder grid renders through every other entry point with the bits it had.  gvt_hip_volume_destroy frees it.
 * OUT OF SCOPE.  The fog attenuating mesh shadow rays; exact per-crossing mesh shadow rays; skipping volume shadow rays where O = 0;
 * the Domain scheduler; AMR frames, and CENTRAL frames without GVT_HIP_VOLUME_ALLOW_CENTRAL ("shadowed surfaces", CENTRAL). */
typedef struct {
  uint32_t flags; /* 0, or GVT_HIP_VOLUME_ALLOW_CENTRAL and GVT_HIP_VOLUME_ALLOW_AMR ORed */
  uint32_t pad;
} gvt_hip_volume_occluder_params;
typedef struct {
  uint64_t rays, rays_blocked, any_hit_launches, bytes;
  float ms;
  uint32_t pad;
} gvt_hip_volume_occluder_stats;
typedef struct {
  uint32_t present, current; /* a grid is held | ... and no call has made it stale since its bake */
  int32_t n_planes, pad;     /* usable lights at the bake */
  uint64_t bytes;
} gvt_hip_volume_occluder_state;
typedef struct {
  gvt_hip_volume_fog_shadow_stats fog; /* the fog-shadowed frame's counters, same meaning */
  uint32_t mesh_shadowed, pad;
} gvt_hip_volume_mesh_shadow_stats;
int gvt_hip_volume_occluder_grid_bake(gvt_hip_volume *const *volumes, const float *m, const float *minv, size_t n_inst,
                                      gvt_hip_mesh *const *meshes, const float *mesh_minv /* 16 floats per mesh instance */, size_t n_mesh_inst,
                                      const gvt_hip_volume_occluder_params *params, gvt_hip_volume_occluder_stats *stats /* may be NULL */);
/* out: host memory, counts[0] * counts[1] * counts[2] bytes at i + nx * (j + ny * k).  No grid, or a light that was unusable at the
 * bake: GVT_HIP_ERR_INVALID.  A stale grid can still be downloaded. */
int gvt_hip_volume_occluder_grid_download(gvt_hip_volume *, int light, uint8_t *out);
int gvt_hip_volume_occluder_grid_info(gvt_hip_volume *, gvt_hip_volume_occluder_state *out);
int gvt_hip_volume_occluder_grid_release(gvt_hip_volume *); /* frees the planes; a volume without a grid: 0 */
int gvt_hip_volume_frame_mesh_shadowed(gvt_hip_top *, gvt_hip_volume *const *volumes, const float *m, const float *minv, size_t n_inst,
                                       const gvt_hip_camera *cam, gvt_hip_queue *const *queues, gvt_hip_fb *fb,
                                       const gvt_hip_depth *depth /* may be NULL */, const gvt_hip_volume_shadow_params *params,
                                       gvt_hip_volume_mesh_shadow_stats *stats /* may be NULL */);

/* ---- ambient occlusion: AO grids baked on the device, read in-frame (additive: the ABI revision stays 6, no entry point above changes) ----
 * The ambient term of the shadowed frames stops being a constant: how open a point of the volume is to its surroundings is computed
 * ONCE at every grid vertex (gvt_hip_volume_ao_grid_bake), kept beside the samples as one float32 plane and interpolated wherever ka is
 * used (gvt_hip_volume_frame_ao).
 * THE GRID.  For a frame of bricks of ONE grid, every global vertex I has one float32 value AO(I):
 *   wp     = the vertex in world space, exactly as "shadowed fog" computes it (p[a] = origin[a] + (float)I[a] * spacing[a]; m as a point)
 *   d_i    = the caller's direction i of n_dirs (1 .. GVT_HIP_VOLUME_AO_MAX_DIRS, world space), normalised by the host in float32 the way
 *            the lights are: d / sqrtf((x * x + y * y) + z * z); a zero or non-finite direction is refused
 *   ray i: origin wp, direction d_i, t_min = (float)(bias - 1) * dt, no colour, no opacity, flag GVT_HIP_RAY_CLIP with t_max = radius
 *          (sample k is taken while (float)k * dt < radius); with radius = +Inf no flag and no clip
 *   A_i    = the opacity this ray deposits when marched over the WHOLE grid as ONE brick with the frame's surfaces and shading NONE: the
 *            definition of G_j ("shadowed fog") with the clip added, nothing else -- the side mask is carried, the arrives-opaque rule
 *            holds, GVT_HIP_VOLUME_OPAQUE_A ends the ray
 *   AO(I)  : s = 0.f; for i = 0 .. n_dirs - 1 in order: s = s + (1.f - A_i); AO = s / (float)n_dirs   (the order is part of the contract)
 * A brick stores AO at its own vertices, at the samples' own index, in one plane; shared layers twice with the same bits.  The bits are
 * the one brick's for every bricking: the walk is the light bake's walk by sample ownership, not the next-brick rule, so directions that
 * run in a brick face, axis-parallel ones included, are legal.
 * THE BAKE.  Eligibility is gvt_hip_volume_light_grid_bake's without its two light clauses (an AO bake needs no light and compares
 * none): flags 0 or GVT_HIP_VOLUME_ALLOW_CENTRAL (GVT_HIP_VOLUME_ALLOW_AMR is refused, and so are bricks with subgrids); bias 1 .. 64;
 * n_dirs 1 .. 32; radius > 0 and not NaN; at most 2^32 - 1 (vertex, direction) pairs.  Refusals: GVT_HIP_ERR_INVALID, the message names
 * the clause.  A plane that cannot be allocated: GVT_HIP_ERR_CAPACITY.  A HIP call that fails: GVT_HIP_ERR_DEVICE.  In every failing
 * case each brick keeps the AO grid it had.  The call waits for its launch.  One lane per vertex walks the vertex's rays one after
 * another (volume_ao_grid.inc).
 * CURRENT.  A frame's AO grids are current if ONE bake covered exactly these volumes in this order with the same m and minv bits and
 * since then no brick has had _update_samples[_typed], _update_amr, _set_transfer, _set_surfaces or _set_subgrids.  _set_lights,
 * _set_shading, _set_gradient and _set_ghosts do NOT make them stale.
 * THE FRAME.  gvt_hip_volume_frame_ao is its BASE frame -- gvt_hip_volume_frame_fog_shadowed, or with GVT_HIP_VOLUME_AO_MESH in the flags
 * gvt_hip_volume_frame_mesh_shadowed: same arguments, same refusals, crossings lit through exact in-kernel shadow rays, the fog through
 * Tg (and Og) -- with ONE more change.  At a sample whose cell is c and whose fractions are f
 *     AOg  = trilinear interpolation of AO at the cell's eight vertices (the sample's c and f; nesting x, then y, then z, as Tg)
 *     ka_s = ka * AOg
 *     shaded lit fog sample (tc.w > 0):  rgb[a] = tc.rgb[a] * (ka_s + kd * sum[a])     (a NaN or zero gradient: tc.rgb * ka_s)
 *     crossing at sample k:              the same ka_s in ka's place, AOg from sample k's own cell, shared by all its crossings
 * AO is read only where ka is used; A never depends on it and no ray is cast or skipped because of it, so every counter of `base`
 * equals the base frame's, skipping stays exact against GVT_HIP_VOLUME_NO_SKIP and the image is the same bits for every bricking.
 * INERT.  No usable light, or neither surfaces nor effective lit shading: the call is the base frame in every respect; ao = 0 and no AO
 * grid is needed.
 * REFUSED (GVT_HIP_ERR_INVALID, the message names the clause, nothing changed, the framebuffer not cleared): everything the base frame
 * refuses; unknown flag bits; GVT_HIP_VOLUME_ALLOW_AMR; a frame that is not inert and whose bricks do not all hold a CURRENT AO grid
 * ("ao grid").
 * CONSEQUENCES.  With AO = 1 at every vertex the bits are the base frame's (ka * 1.f is ka); radius <= dt with bias 1 gives that grid
 * (t_min = 0 puts the ray's first sample at k = 1, and (float)1 * dt < radius fails: no sample, A_i = 0).  With ka = 0 the bits are the
 * base frame's at ka = 0.
 * DEVIATIONS.  (1) AO is interpolated from level-0 vertices: one cell soft, and a vertex just behind a sheet sees the sheet; bias is the
 * remedy, as for shadows.  (2) Meshes do not occlude ambient light, and the mesh frame is untouched.  (3) The direction set is fixed per
 * bake and not rotated per vertex: with few directions banding follows the set.
 * COUNTERS.  Bake: rays = (vertices summed over the bricks) x n_dirs; samples_marched / _gathered / crossings as the light bake's;
 * bytes = the planes' size; ms = the event time around the launch.  Frame: the base frame's, and ao = 1 when the AO kernel ran.
 * A volume that holds an AO grid renders through every other entry point with the bits it had.  gvt_hip_volume_destroy frees it.
 * OUT OF SCOPE.  AMR bricks; AO in the unshadowed fused frames and in the per-brick loop; uint8 or coarser planes; the Domain scheduler. */
#define GVT_HIP_VOLUME_AO_MAX_DIRS 32
#define GVT_HIP_VOLUME_AO_MESH 8u /* flags of gvt_hip_volume_ao_frame_params only: the base frame is the mesh-shadowed frame */
typedef struct {
  uint32_t flags; /* 0 or GVT_HIP_VOLUME_ALLOW_CENTRAL */
  int32_t bias;   /* the first sample of a vertex's AO rays, 1 .. 64 */
  int32_t n_dirs; /* 1 .. GVT_HIP_VOLUME_AO_MAX_DIRS */
  float radius;   /* > 0; +Inf: no clip */
  float dirs[GVT_HIP_VOLUME_AO_MAX_DIRS][3];
} gvt_hip_volume_ao_params;
typedef struct {
  uint64_t rays, samples_marched, samples_gathered, crossings, bytes; /* rays = vertices x n_dirs */
  float ms;
  uint32_t pad;
} gvt_hip_volume_ao_stats;
typedef struct {
  uint32_t present, current; /* a grid is held | ... and no call has made it stale since its bake */
  int32_t n_dirs, bias;      /* of the bake */
  float radius;
  uint32_t pad;
  uint64_t bytes;
} gvt_hip_volume_ao_state;
typedef struct {
  uint32_t flags; /* 0, GVT_HIP_VOLUME_ALLOW_CENTRAL, GVT_HIP_VOLUME_AO_MESH, or both */
  int32_t bias;   /* the crossings' shadow rays', 1 .. 64 */
} gvt_hip_volume_ao_frame_params;
typedef struct {
  gvt_hip_volume_mesh_shadow_stats base; /* the base frame's counters, same meaning */
  uint32_t ao, pad;                      /* ao = 1: the AO kernel ran */
} gvt_hip_volume_ao_frame_stats;
int gvt_hip_volume_ao_grid_bake(gvt_hip_volume *const *volumes, const float *m, const float *minv, size_t n_inst,
                                const gvt_hip_volume_ao_params *params, gvt_hip_volume_ao_stats *stats /* may be NULL */);
/* out: host memory, counts[0] * counts[1] * counts[2] floats at i + nx * (j + ny * k).  No grid: GVT_HIP_ERR_INVALID.  A stale grid
 * can still be downloaded. */
int gvt_hip_volume_ao_grid_download(gvt_hip_volume *, float *out);
int gvt_hip_volume_ao_grid_info(gvt_hip_volume *, gvt_hip_volume_ao_state *out);
int gvt_hip_volume_ao_grid_release(gvt_hip_volume *); /* frees the plane; a volume without a grid: 0 */
int gvt_hip_volume_frame_ao(gvt_hip_top *, gvt_hip_volume *const *volumes, const float *m, const float *minv, size_t n_inst,
                            const gvt_hip_camera *cam, gvt_hip_queue *const *queues, gvt_hip_fb *fb, const gvt_hip_depth *depth /* may be NULL */,
                            const gvt_hip_volume_ao_frame_params *params, gvt_hip_volume_ao_frame_stats *stats /* may be NULL */);

/* ---- framebuffer: IceTComposite (composite/IceTComposite.cpp:79-157) ---- */
gvt_hip_fb *gvt_hip_fb_create(int width, int height);
void gvt_hip_fb_destroy(gvt_hip_fb *);
int gvt_hip_fb_clear(gvt_hip_fb *);                              /* reset(), :79-82 */
int gvt_hip_fb_download(gvt_hip_fb *, float *rgba /* W*H*4 */, int clamp); /* clamp: c>1 -> 1 (localAdd :111-117) */
void *gvt_hip_fb_device_ptr(gvt_hip_fb *);                       /* float[W*H*4], un-clamped sums: for the RCCL reduce */
int gvt_hip_fb_write_ppm_bytes(gvt_hip_fb *, unsigned char *rgb /* W*H*3, rows flipped, (uchar)(c*255) :119-157 */);

/* ---- measurement ---- */
typedef struct gvt_hip_stats {
  uint64_t rays_closest; /* rays pushed through the closest-hit kernel */
  uint64_t rays_any;     /* rays pushed through the any-hit kernel */
  uint64_t rays_shaded, rays_forwarded, trace_calls;
  /* HIP-event time per kernel class, ms, accumulated while profiling is enabled */
  double ms_closest, ms_any, ms_shade, ms_convert, ms_shuffle, ms_camera, ms_build;
  uint64_t launches_closest, launches_any;
  double ms_sort; /* ray sorting inside the adapter */
  double ms_long; /* k_long_closest: parked long rays, a wave per ray (not part of ms_closest) */
} gvt_hip_stats;
int gvt_hip_profile(int enable);           /* 1: bracket every kernel with HIP events on the launch stream; 2: the traversal kernels only; 3 / 4: the
                                            * closest-hit / any-hit launches only (an event pair costs a few microseconds of the stream); 0: off */
int gvt_hip_stats_read(gvt_hip_stats *);   /* synchronises */
int gvt_hip_stats_reset(void);
/* diagnostic, not on the hot path: per-ray visit counts of the closest-hit traversal over n object-space rays:
 * counts[3*j + 0..2] = inner-node visits / leaf visits / triangle tests of ray j. */
int gvt_hip_visit_stats(gvt_hip_mesh *, const float *org, const float *dir, size_t n, float tnear, uint32_t *counts);
/* diagnostic, not on the hot path: the number of nodes a `width`-wide collapse of the mesh's tree (width 2..8, the collapse rule of the
 * 4-wide layout the traversal uses) would make each ray visit; *n_wide_nodes (optional) = nodes of that collapse. */
int gvt_hip_wide_visit_stats(gvt_hip_mesh *, const float *org, const float *dir, size_t n, float tnear, int width, uint32_t *counts /* n */,
                             uint64_t *n_wide_nodes);
/* measurement: the traversal layout as the kernels walk it -- (bytes_nodes / 64 - n_nodes) compressed 4-wide nodes of 64 bytes {origin.xyz, step.x | qlo.x[4], qhi.x[4],
 * qlo.y[4], qhi.y[4] | qlo.z[4], qhi.z[4], ref0, ref1 | ref2, ref3, step.y, step.z} (child box plane = origin + q * step; ref >= 0: node, < 0: leaf, ~ref =
 * first slot << 3 | triangles) and n_tris triangle slots of 64 bytes {v0, primID | e1 = v0 - v1, v1.x | e2 = v2 - v0, v1.y | v1.z, v2.xyz} in leaf order -- for the SIMD CPU
 * baseline of bench.py (oracle/simd_baseline.c) */
int gvt_hip_mesh_download_wide(gvt_hip_mesh *, void *nodes4, size_t n_nodes4, void *slots, size_t n_slots);
/* ... and the CLUSTER layout of the same nodes (built on first use; the Domain scheduler's small rounds, k_finish, walk it -- knob finish_clusters): a permutation of
 * nodes4 in which every node of an even level is followed by its inner children, the references of the odd-level nodes to inner nodes being (slot << 4) | mask
 * of the grandchild's inner children; *root_entry = the root's (slot 0).  rc 0 with *root_entry = -1: the mesh has no such layout (too deep or too large), the
 * traversals walk nodes4 */
int gvt_hip_mesh_download_clusters(gvt_hip_mesh *, void *nodes4c, size_t n_nodes4, int32_t *root_entry);
/* diagnostics behind tools/wide_dp.py (is a cost-optimal wide collapse of the tree worth building?): the binary LBVH as built -- n_nodes x 64 bytes,
 * per node {c0.lo.x, c0.hi.x, c0.lo.y, c0.hi.y | c1.lo.x, c1.hi.x, c1.lo.y, c1.hi.y | c0.lo.z, c0.hi.z, c1.lo.z, c1.hi.z | child0, child1 (int32; < 0: leaf), -, -} --
 * and the visits of a collapse the CALLER chose: marks[k] = 1 where binary node k is the root of a wide node, counts[j] = marked nodes ray j visits */
int gvt_hip_mesh_download_nodes(gvt_hip_mesh *, void *out, size_t n_nodes);
/* ... and back: a tree of the caller's over the SAME leaves (same node count, root = node 0) for the visit-count diagnostics only -- the 4-wide layout the
 * product kernels traverse is not rebuilt from it */
int gvt_hip_mesh_upload_nodes(gvt_hip_mesh *, const void *in, size_t n_nodes);
int gvt_hip_marked_visit_stats(gvt_hip_mesh *, const float *org, const float *dir, size_t n, float tnear, const unsigned char *marks /* n_nodes */, uint32_t *counts /* n */);
/* diagnostic, not on the hot path: include/gvt_math.h evaluated on the device, element-wise over n floats -- kind 0 gvt_sinf(x),
 * 1 gvt_cosf(x), 2 (float)gvt_acos(sqrt(1.0 - x)) -- so that a test can compare the device's bits with the host's for the
 * functions the bounce path (EmbreeMeshAdapter.cpp:289-318) is built on. */
int gvt_hip_math_probe(int kind, const float *in, size_t n, float *out);
/* Knobs of the library (gvt_internal.h `struct Knobs` lists them with their defaults; ("defaults", 0) restores all of them).  Results never
 * depend on them -- except "skip_known" = 1, an opt-in approximation of the shuffle rule (below).  The shipped surface, 23 knobs:
 *   behaviour    "skip_known"   0 (default): the reference's hop-by-hop shuffleRays, ray for ray -- 1: the known-miss shortcut (a ray is not traced / sent again into an
 *                               instance it has already crossed without a hit on the same straight segment).  The shortcut saves the hand-back hops between
 *                               overlapping boxes but is an APPROXIMATION: where a re-trace from the advanced origin would flip an edge-grazing triangle test,
 *                               the reference finds a hit the shortcut skips (measured: 2 of 147,456 pixels of the hall in 8 slabs; none on the soup tiles)
 *                "term_sink"    1: gvt_hip_trace_queue_sink applies shuffleRays' terminal rule inside the kernels -- 0: every moved ray goes through the shuffle
 *                "sort_rays"    1: Morton-sort a list before traversal (pays on incoherent lists; off)
 *                "frame_timing" 1: fill gvt_hip_frame_stats' per-phase milliseconds (five more event calls per exchange)
 *                "packet"       closest hits of coherent lists (camera rays in tile order) a packet of 64 rays per wave: 0 never, 1 (default) on meshes the builder
 *                               found packet-friendly (gvt_hip_mesh_info::packet), in launches of at least "packet_min_rays" rays, 2 always (and shadow rays too)
 *                "shadow_order" 1 (default): a single-mesh round with one light lists its shadow rays by how many node steps the primaries of their 64-ray tile
 *                               took, the longest first (a shadow ray's step count follows its primary's), so that the any-hit launch's drain is left to
 *                               short rays -- in launches of at least "shadow_order_min_rays" rays; 0: in arrival order.  Results do not depend on it
 *                "early_deposit" 1 (default): the one-instance frame of gvt_hip_tracer_frame with one light, one sample per pixel, depth 1 and a plain LAMBERT mesh stores a shadow
 *                               ray's deposit to its pixel at shading time (one writer per pixel, into the frame's own clear) and the any-hit launch only takes it back where
 *                               the ray is occluded -- no survivor list, no float atomics; 0: deposits by the any-hit launch.  Results do not depend on it;
 *                               gvt_hip_frame_stats::early_deposit_launches counts the launches that took the path
 *   build time   "leaf_max"     triangles per leaf of meshes created afterwards (1..4, default 2)
 *                "packet_sah_max"  meshes created afterwards are packet-friendly when gvt_hip_mesh_info::sah_inner is at most this (default 128)
 *   budgets      "long_steps" / "long_min_rays" / "long_auto"  closest hit: node steps after which a ray is parked for a whole wave (0: never), launches it
 *                               applies to, and whether gvt_hip_tracer_frame raises it from frame to frame on scenes that park more than 0.3 % of their rays
 *                "small_rays" / "finish_rays"    rounds of at most so many rays: a wave per ray / the whole round in one launch (k_finish)
 *                "finish_auto"                   1: on one rank with several instances gvt_hip_tracer_frame times a few frames with and without k_finish and keeps
 *                                                the faster (a hop that is a long traversal of its own is better served by per-hop rounds)
 *                "round_room_mb"                 memory a round's worst-case reservation may add before it falls back to exact growth
 *                "payload_overlap_kb"            Domain scheduler: payloads of at least this size move on the communicator's own stream beside the next chain
 *                "inline_kb"                     Domain scheduler: a pair's payload of at most this many KiB per tick travels inside the announce message (one exchange
 *                                                per tick; default 16; the same on every rank; 0: the two-step exchange of SendRays, counts then rays)
 *                "comm_cus"                      Domain scheduler: compute units reserved for the communicator's own stream (CU mask; the persistent traversal grids
 *                                                are sized for the rest); set before gvt_hip_comm_create; default 0
 *                "spec_ticks"                    Domain scheduler, asynchronous ticks: 1 (default) = the next tick's small round and report are enqueued behind the
 *                                                current exchange before its result is read (the device voids them when the result needs the host); 0 = never
 *                "hop_local"                     Domain / Image scheduler, merged launches over several instances: a ray that leaves its instance without a hit and has another
 *                                                instance of THIS rank ahead goes on there inside the traversal launch (shuffleRays' rule applied by the lane) instead of waiting
 *                                                for the next round -- 0 never, 2 always, 3 early: in the closest-hit launch only and only while it still has rays to hand out (a ray that
 *                                                goes on during the launch's drain stretches its tail), 1 (default) per tracer: never / early / always timed like finish_auto on one rank, on several
 *                                                by the meshes' kind (surfaces always, volume-filling soups never).  Results never depend on it
 *                "finish_clusters"               small rounds of several instances (k_finish, a wave per ray): 1 (default) = walk the cluster layout of the 4-wide nodes
 *                                                (two tree levels per memory round trip; built per mesh when such a tracer is created, + 64 bytes per node); 0 = the plain nodes
 *                "comm_stream"                   Domain scheduler: 1 = every exchange of a frame on the communicator's own stream, ordered against the compute stream
 *                                                by events (also GVT_HIP_COMM_STREAM in the environment); default 0: on the compute stream, large payloads beside it
 *                "abi_lanes" / "abi_chunk"     gvt_hip_trace on a host RayVector: pipeline lanes (0: one shot), rays per chunk
 *   test hooks   "inject_fail_tick"; "occluder_chunk": (vertex, light) pairs per chunk of gvt_hip_volume_occluder_grid_bake (0, the default: the
 *                               library's own constant), so that a test's small grid spans several chunks.  Results never depend on it
 * Everything else -- the tuned constants of the kernels (refill / phase thresholds, grid sizes, drain sharing ...) and the alternative arms that
 * were measured and lost but stay in the code (merged kernels for one queue, compacted shadow slots, non-lean frames, camera rays in
 * generateRays' pixel-major order ("camera_tile" = 0) ...: EXPERIMENTS.md) -- can be moved only in the experiments build of the library
 * (libgvt_hip_exp.so, -DGVT_EXPERIMENTS), where the knob sweeps run; the shipped library answers GVT_HIP_ERR_INVALID when one of them is
 * switched away from its default.  Any other name is an unknown option in both builds. */
int gvt_hip_set_option(const char *name, int value);
/* 1 in the experiments build (the tuned constants movable), 0 in the shipped library */
int gvt_hip_is_experiments_build(void);
/* diagnostic: the calling thread's context counter words (32) after a stream synchronisation; [3] = rays the last closest-hit launch
   parked for k_long_closest, [8] = traversal overflow flags */
int gvt_hip_counters_peek(uint32_t out[32]);

#ifdef __cplusplus
}
#endif
#endif
