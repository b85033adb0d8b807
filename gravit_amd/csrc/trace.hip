// trace.hip -- the adapter hot path on gfx950: Adapter::trace
// (src/gvt/render/Adapter.h:82-84, adapter/embree/EmbreeMeshAdapter.cpp:436-660).
//
// The kernels live in include files by family (all inside this translation unit's anonymous namespace):
//   trace_lane.inc     k_trace: ONE LANE PER RAY, persistent waves with lane refill.  k_trace<false,..> = rtcIntersect (EmbreeMeshAdapter.cpp:474):
//                      ray -> object space, nearest hit in (1e-6, inf); k_trace<true,..> = rtcOccluded (:364-385): un-occluded shadow rays are
//                      appended to moved_rays -- or, with a sink, end right there by the terminal rule of the shuffleRays that would follow
//   trace_wave.inc     A WAVE PER RAY: k_long_closest (the few rays k_trace parks after `long_steps` node steps), k_long_seed / k_wave_any (small rounds)
//   shade.inc          k_shade: the per-lane block :483-609 -- miss forward / shadow drop / normal / material / Shade / shadow-ray generation
//                      (:320-358) / Russian-roulette bounce (:584-602)
//   finish_kernel.inc  k_finish: a small scheduler round in one launch, every ray followed to its end on this rank
//   convert.inc        80-byte Ray AoS <-> planes, ray sort keys, bookkeeping kernels;  diag_kernels.inc: the visit-count diagnostic
// and this file keeps the host side:
//   closest_step, any_step, shade_args, chain_bufs, ...   the steps every chain is made of, each written once
//   trace_core         one Adapter::trace call: closest -> shade -> any per pass, one read-back per pass
//   wave_trace_chain   the same chain for a whole scheduler ROUND, ray counts in device memory, no host round trip: single_pass (one non-empty
//                      local queue: the single-mesh kernels) or merged_pass (all of them at once: the MULTI variants);  finish_round: k_finish
//
// k_trace in one paragraph: a wave pulls index ranges from a device counter (an exit every wave reaches), refills lanes whose ray has finished
// while the others go on, alternates a tight loop over the compressed 4-wide nodes with a leaf phase, keeps its traversal stacks in LDS
// (stack[level][lane]: lane-contiguous, bank conflict free) and compacts survivors per wave (__ballot + mbcnt, one atomic per >= 64 rays).
// EXPERIMENTS.md lists the variants that were measured on the way and lost; their code is in the history.
#include "gvt_internal.h"

#ifndef TRAV_BLOCK
#define TRAV_BLOCK 256   // threads per traversal block (64: every wave is its own block and gives its registers / LDS back when IT ends)
#endif
#define TRAV_WAVES_PER_BLOCK (TRAV_BLOCK / 64) // (the blocks-per-CU knobs count 256-thread blocks = waves per SIMD)
#ifndef TRAV_STACK
#define TRAV_STACK 24   // LDS entries per lane; deeper levels spill to a per-thread global area
#endif
#ifndef KT_BLOCKS_CLOSEST
#define KT_BLOCKS_CLOSEST 5 // resident 256-thread blocks per CU the compiler must leave room for (register budget 512 / waves per SIMD)
#endif
#ifndef RETIRE_BATCH
#define RETIRE_BATCH 1
#endif
#ifndef KT_BLOCKS_ANY
#define KT_BLOCKS_ANY 4
#endif
#define TRAV_SPILL 128  // 24 + 128 = 152 pending entries: > 63 + 24 levels of a 63-bit Karras tree with index tie-breaks, and > 3 x 44, the
                        // worst case of its 4-wide collapse; k_trace reports an error beyond that instead of losing entries

namespace {

struct Trav {
  const BvhNode *__restrict__ nodes;
  const float4 *__restrict__ tris;
  const uint4 *__restrict__ nodes4;  // compressed 4-wide collapse (64 B per node) or null
};

#include "diag_kernels.inc" // visit counts

#include "trace_lane.inc" // the lane-per-ray traversal

#include "trace_wave.inc" // the wave-per-ray traversal

#include "packet_kernel.inc" // k_packet: a wave walks the BVH for a packet of 64 coherent rays (meshes the builder found packet-friendly)

#include "shade.inc" // Shade(), lights, the bounce direction, k_shade

#include "finish_kernel.inc" // k_finish: a small round in one launch, every ray followed to its end on this rank

#include "convert.inc" // layout conversions at the ABI boundary, ray sort keys, the small bookkeeping kernels of a trace call

inline unsigned blocks_for(size_t n, unsigned b = 256) { return (unsigned)((n + b - 1) / b); }

int trav_grid(size_t n) {
  Ctx &C = gctx();
  size_t need = (n + TRAV_BLOCK - 1) / TRAV_BLOCK;
  return (int)(need < (size_t)C.trav_blocks ? (need ? need : 1) : (size_t)C.trav_blocks);
}

template <bool ANY, bool XFORM, int MODE, bool MULTI = false, typename... Args> void launch_trace(int grid, hipStream_t st, RayPlanes q, const unsigned *idx, unsigned n, Mat4 minv, Args... args) {
  // k_trace never reads the matrix's bottom row (an instance matrix is affine); it carries the direction transform's `translation x 0` terms there instead
  // (xfm_vector: m[12..14] * 0.0f, kept for parity with glm's mat4 * vec4(d, 0)): kernel arguments live in SCALAR registers, where the products computed on
  // the device sat in three vector registers for the whole launch -- spilled to scratch in the shipped closest-hit kernel
  minv.m[3] = minv.m[12] * 0.0f; minv.m[7] = minv.m[13] * 0.0f; minv.m[11] = minv.m[14] * 0.0f;
  k_trace<ANY, XFORM, MODE, MULTI><<<grid, TRAV_BLOCK, 0, st>>>(q, idx, n, minv, args...); // a mesh without 4-wide nodes has no triangles: every ray retires as a miss
}

// scratch of a closest-hit launch's parked rays: n records, then LONG_SAVE stack entries for each of the first LONG_STK_CAP of them
static size_t long_scratch_bytes(size_t n) { return sizeof(LongRec) * n + sizeof(int) * LONG_SAVE * (size_t)LONG_STK_CAP; }
static LongQ long_queue(LongRec *recs, size_t n) { // k_trace parks its long rays in recs[0, n), counted in CW_LONG
  Ctx &C = gctx();
  LongQ LQ{};
  LQ.recs = recs; LQ.count = C.d_counters + CW_LONG;
  LQ.steps = C.long_steps_override > 0 ? C.long_steps_override : C.long_steps;
  LQ.steps_drain = C.long_steps_drain > 0 && C.long_steps_drain < LQ.steps ? C.long_steps_drain : LQ.steps;
  LQ.stk = C.long_save ? (int *)(LQ.recs + n) : nullptr;
  LQ.stk_cap = LONG_STK_CAP;
  return LQ;
}

// persistent-wave kernel: fewer, longer-lived waves so that every lane is refilled several times
int trav_grid2(size_t n, bool closest = false) {
  Ctx &C = gctx();
  size_t want = (size_t)C.n_cu * (((size_t)((closest && C.blocks_per_cu_closest) ? C.blocks_per_cu_closest : C.blocks_per_cu) * 4) / TRAV_WAVES_PER_BLOCK);
  if (!want) want = C.n_cu;
  size_t need = (n + TRAV_BLOCK - 1) / TRAV_BLOCK;
  if (want > (size_t)C.trav_blocks) want = (size_t)C.trav_blocks;
  return (int)(need < want ? (need ? need : 1) : want);
}

} // namespace

int debug_stamps(unsigned long long *out, int reset) {
#if GVT_STAMP
  hipDeviceSynchronize();
  hipMemcpyFromSymbol(out, HIP_SYMBOL(g_stamp), sizeof(unsigned long long) * 24);
  if (reset) { unsigned long long z[24] = { 0 }; hipMemcpyToSymbol(HIP_SYMBOL(g_stamp), z, sizeof z); }
  return 0;
#else
  for (int i = 0; i < 24; i++) out[i] = 0;
  return -1;
#endif
}
// queued behind the traversal launches on the stream; read after the caller's next synchronisation through trav_overflow_result()
int trav_overflow_fetch_async() {
  Ctx &C = gctx();
  HIPCHK(hipMemcpyAsync(C.h_pinned + 8, C.d_counters + CW_TRAV_OVF, sizeof(unsigned), hipMemcpyDeviceToHost, C.stream));
  return 0;
}
int trav_overflow_result() {
  Ctx &C = gctx();
  if (!C.h_pinned[8]) return 0;
  C.h_pinned[8] = 0;
  hipMemsetAsync(C.d_counters + CW_TRAV_OVF, 0, sizeof(unsigned), C.stream);
  set_error("BVH traversal stack overflow (more than %d pending entries for one ray): results of this call are incomplete", TRAV_STACK + TRAV_SPILL);
  return GVT_HIP_ERR_DEVICE;
}
size_t trav_spill_ints_per_thread() { return TRAV_SPILL; }
int trav_block_threads() { return TRAV_BLOCK; }

int convert_aos_to_planes(const gvt_hip_ray *d_src, size_t n, RayPlanes dst, size_t dst_off, bool keep_state) {
  if (!n) return 0;
  ProfScope ps(KC_CONVERT);
  k_aos_to_planes<<<blocks_for(n), 256, 0, gctx().stream>>>((const float4 *)d_src, (unsigned)n, dst, dst_off, keep_state ? 1 : 0);
  HIPCHK(hipGetLastError());
  return 0;
}
int convert_planes_to_aos(RayPlanes src, size_t src_off, size_t n, gvt_hip_ray *d_dst) {
  if (!n) return 0;
  ProfScope ps(KC_CONVERT);
  k_planes_to_aos<<<blocks_for(n), 256, 0, gctx().stream>>>(src, src_off, (unsigned)n, (float4 *)d_dst);
  HIPCHK(hipGetLastError());
  return 0;
}
int convert_od_to_planes(const float *d_org, const float *d_dir, size_t n, RayPlanes dst) {
  if (!n) return 0;
  ProfScope ps(KC_CONVERT);
  k_od_to_planes<<<blocks_for(n), 256, 0, gctx().stream>>>(d_org, d_dir, (unsigned)n, dst);
  HIPCHK(hipGetLastError());
  return 0;
}

// ---- the steps the launch chains below are made of ----
MeshView mesh_view(const gvt_hip_mesh *M) {
  MeshView mv;
  mv.slots = M->d_tri; mv.slot_of = M->d_slot_of; mv.verts = M->d_verts; mv.tris = M->d_tris; mv.normals = M->d_normals; mv.vcolors = M->d_vcolors;
  mv.materials = M->d_materials; mv.n_mat = (unsigned)M->nMat; mv.face_mat = M->d_face_mat; mv.mat = M->mesh_mat;
  return mv;
}
// knob packet: 0 never, 1 the mesh's own choice (gvt_hip_mesh::packet_ok) in launches of at least packet_min_rays, 2 always
bool walks_packets(const Ctx &C, const gvt_hip_mesh *M, size_t n) { return C.packet == 2 || (C.packet == 1 && M->packet_ok && n >= (size_t)C.packet_min_rays); }
bool plain_lambert(const gvt_hip_mesh *M) { return !M->d_vcolors && !M->d_face_mat && M->mesh_mat.type == 0; }
bool no_area_light(const gvt_hip_light *lights, int nL) { return std::all_of(lights, lights + nL, [](const gvt_hip_light &l) { return l.type != GVT_HIP_LIGHT_AREA; }); }

// The light list rarely changes between calls: the context keeps a device copy (SCR_LIGHTS) and the host bytes it was made from.
static bool lights_cached_at(const Ctx &C, const void *dst, const gvt_hip_light *lights_host, int nL) {
  const size_t bytes = sizeof(gvt_hip_light) * (size_t)nL;
  return C.lights_cached_dst == dst && C.lights_cached.size() == bytes && std::memcmp(C.lights_cached.data(), lights_host, bytes) == 0;
}
// the context's device copy of the light list is this list: a launch may use it without a copy
bool finish_lights_resident(const gvt_hip_light *lights_host, int nL) {
  Ctx &C = gctx();
  return !nL || (C.scratch[SCR_LIGHTS] && lights_cached_at(C, C.scratch[SCR_LIGHTS], lights_host, nL));
}
// ... uploaded when it (or its scratch buffer) changed; may_upload = false: it must be resident already (no upload, no synchronisation in here)
static int lights_on_device(const gvt_hip_light *lights_host, int nL, gvt_hip_light **d_lights, bool may_upload = true) {
  Ctx &C = gctx();
  *d_lights = (gvt_hip_light *)scratch_get(SCR_LIGHTS, sizeof(gvt_hip_light) * (nL > 0 ? nL : 1));
  if (!*d_lights) return GVT_HIP_ERR_DEVICE;
  if (!nL || lights_cached_at(C, *d_lights, lights_host, nL)) return 0;
  if (!may_upload) { set_error("finish_round: a speculative launch needs the light list resident"); return GVT_HIP_ERR_INVALID; }
  const size_t bytes = sizeof(gvt_hip_light) * (size_t)nL;
  C.lights_cached.assign((const unsigned char *)lights_host, (const unsigned char *)lights_host + bytes);
  C.lights_cached_dst = *d_lights;
  HIPCHK(hipMemcpyAsync(*d_lights, C.lights_cached.data(), bytes, hipMemcpyHostToDevice, C.stream));
  HIPCHK(hipStreamSynchronize(C.stream)); // pageable source: finish the copy before the cached bytes can change
  return 0;
}

// The scratch a chain over n rays needs whatever its kernels: hits, the pass's shadow list, the two bounce index lists, the lights.
struct ChainBufs {
  gvt_hip_hit *hits; unsigned *idx_a, *idx_b; gvt_hip_light *lights;
  size_t shadow_cap; RayPlanes shadow; // shadow rays a pass can emit, and their list: shadow_cap slots, or ordered_slots
  unsigned char *steps;                // non-null: the class-ordered list was asked for and granted
};
// ordered_slots != 0: the class-ordered shadow list of that many slots (8 x 64 bytes per ray: 0.5 GB at the benchmark's 1.04 M rays) and the step counts it is
// ordered by.  The ordering is an optimisation whose results do not depend on it: it must never make a frame fail that fits without it.  A device that
// cannot give the 8x list falls back to arrival order with the plain list, for this context from then on (no allocation attempt per frame).
static int chain_bufs(ChainBufs &B, size_t n, int nL, const gvt_hip_light *lights_host, size_t ordered_slots = 0) {
  Ctx &C = gctx();
  B.hits = (gvt_hip_hit *)scratch_get(SCR_GENERAL, sizeof(gvt_hip_hit) * n);
  B.shadow_cap = n * (size_t)(nL > 0 ? nL : 1);
  size_t slots = ordered_slots ? ordered_slots : B.shadow_cap;
  float4 *d_shadow = (float4 *)scratch_get(SCR_SHADOW, sizeof(float4) * 4 * slots);
  B.steps = (ordered_slots && d_shadow) ? (unsigned char *)scratch_get(SCR_STEPS, n) : nullptr;
  if (ordered_slots && (!d_shadow || !B.steps)) {
    (void)hipGetLastError(); // (the failed hipMalloc's sticky-less error)
    C.shadow_order_denied = true;
    B.steps = nullptr;
    slots = B.shadow_cap;
    d_shadow = (float4 *)scratch_get(SCR_SHADOW, sizeof(float4) * 4 * slots);
  }
  B.idx_a = (unsigned *)scratch_get(SCR_IDX_A, sizeof(unsigned) * n);
  B.idx_b = (unsigned *)scratch_get(SCR_IDX_B, sizeof(unsigned) * n);
  if (!B.hits || !d_shadow || !B.idx_a || !B.idx_b) return GVT_HIP_ERR_DEVICE;
  B.shadow = make_planes(d_shadow, slots);
  B.shadow.p4 = nullptr; B.shadow.p5 = nullptr; // shadow rays carry no stream and no list
  return lights_on_device(lights_host, nL, &B.lights);
}

// Ray sorting (knob sort_rays): *idx becomes the list's first n entries (of a list of at most n_cap) in the order of k_ray_keys' key -- direction octant, then
// the Morton cell of the object-space origin in M's box.  n_dev: the length where only the device knows it (the unused entries sort last).
static int sort_ray_list(const gvt_hip_mesh *M, RayPlanes q, const unsigned **idx, size_t n, size_t n_cap, const Mat4 &minv, const unsigned *n_dev = nullptr) {
  Ctx &C = gctx();
  unsigned *k_in = (unsigned *)scratch_get(SCR_SORT_KEYS_IN, sizeof(unsigned) * n_cap), *k_out = (unsigned *)scratch_get(SCR_SORT_KEYS_OUT, sizeof(unsigned) * n_cap);
  unsigned *v_in = (unsigned *)scratch_get(SCR_SORT_VALS_IN, sizeof(unsigned) * n_cap), *v_out = (unsigned *)scratch_get(SCR_SORT_VALS_OUT, sizeof(unsigned) * n_cap);
  if (!k_in || !k_out || !v_in || !v_out) return GVT_HIP_ERR_DEVICE;
  const float ex = M->hi[0] - M->lo[0], ey = M->hi[1] - M->lo[1], ez = M->hi[2] - M->lo[2];
  const float3 blo = make_float3(M->lo[0], M->lo[1], M->lo[2]);
  const float3 inv = make_float3(ex > 0 ? 1.f / ex : 0.f, ey > 0 ? 1.f / ey : 0.f, ez > 0 ? 1.f / ez : 0.f);
  {
    ProfScope ps(KC_SORT);
    k_ray_keys<<<blocks_for(n), 256, 0, C.stream>>>(q, *idx, (unsigned)n, minv, blo, inv, k_in, v_in, C.sort_bits, n_dev);
    if (int rc = sort_pairs_u32(k_in, k_out, v_in, v_out, n, C.sort_bits)) return rc;
  }
  HIPCHK(hipGetLastError());
  *idx = v_out;
  return 0;
}

// Where a traversal step's rays and geometry come from: one mesh (q, minv, T; W empty) or a round's segments (MULTI kernels: W; q, minv, T empty).
struct TraceSrc { RayPlanes q; Mat4 minv; Trav T; WaveSet W; TermSink sink; MultiSrc MS; const int *hop; unsigned row; }; // hop: MultiSrc::hop_inst for the wave-per-ray kernels; row: the list's row length in rays where it has film geometry (xcd_stripes.h), else 0
// k_trace's stripe_row for a single-mesh launch over a list of that row length (knob xcd_stripes).  A list without film geometry (row 0: bounce and index lists, shadow
// lists, the adapter's queries) is handed out front to back: stripes over default rows group the rays as that order already does -- the any-hit launch showed the same
// L2 counters either way, profiles/xcd_stripes.txt -- and cost a wave up to eight atomics at its end where the one counter costs one.  So only the launch over the camera's
// coherent list draws from the eight counters, and only the kernels in front of THAT launch (k_wave_pass_begin, k_cam1_scatter) have to zero them all (cw_zero_work).
static unsigned stripe_arg(unsigned row) { return (gctx().xcd_stripes && row) ? row : XCD_STRIPES_OFF; }
enum StepMode { BY_LANES, BY_PACKETS, BY_WAVES }; // k_trace (+ its parked rays a wave each) | k_packet (+ the packets that bailed out) | a wave per ray (small launches)
static int wave_grid(size_t n) { return (int)std::min<size_t>((n + 3) / 4, (size_t)gctx().n_cu * 3); }

// The closest-hit step over idx[0, n) (null: the identity; n_dev: the count where only the device knows it) into d_hits.  LQ.steps != 0: k_trace parks long rays;
// d_long: the parked-ray records (BY_PACKETS and BY_WAVES use them whatever LQ says).  `later_pass`: a merged chain's bounce pass (the rays' hops are read).
template <bool XFORM, bool MULTI>
static void closest_step(StepMode mode, const TraceSrc &S, const unsigned *idx, size_t n, const unsigned *n_dev, float tnear, gvt_hip_hit *d_hits, const LongQ &LQ,
                         LongRec *d_long, bool later_pass = false) {
  Ctx &C = gctx();
  hipStream_t st = C.stream;
  unsigned *c = C.d_counters;
  const int tail_grid = C.n_cu * 3; // 48 KiB of LDS per block
  RayPlanes none{};
  if (mode == BY_PACKETS) {
    ProfScope ps(KC_CLOSEST);
    LongQ LP{ d_long, c + CW_LONG, nullptr, 0u, 0, 0 };
    if constexpr (MULTI) k_packet_multi<<<blocks_for(n), 256, 0, st>>>(S.W, (unsigned)n, n_dev, tnear, d_hits, LP, c + CW_PACKETS);
    else k_packet<false><<<blocks_for(n), 256, 0, st>>>(S.q, (unsigned)n, n_dev, S.minv, S.T, tnear, d_hits, nullptr, none, nullptr, TermSink{}, LP, nullptr, nullptr, nullptr, c + CW_PACKETS);
    k_long_closest<XFORM, MULTI><<<tail_grid, 256, 0, st>>>(S.q, d_long, c + CW_LONG, S.minv, S.T, tnear, d_hits, c + CW_LONG_WORK, S.W); // packets that bailed out
  } else if (mode == BY_WAVES) {
    ProfScope ps(KC_CLOSEST);
    k_long_seed<<<blocks_for(n), 256, 0, st>>>(d_long, c + CW_LONG, idx, (unsigned)n, n_dev);
    k_long_closest<XFORM, MULTI><<<wave_grid(n), 256, 0, st>>>(S.q, d_long, c + CW_LONG, S.minv, S.T, tnear, d_hits, c + CW_LONG_WORK, S.W, nullptr, later_pass ? S.hop : nullptr);
  } else {
    {
      ProfScope ps(KC_CLOSEST);
      launch_trace<false, XFORM, 0, MULTI>(trav_grid2(n, true), st, S.q, idx, (unsigned)n, S.minv, S.T, tnear, d_hits, nullptr, none, nullptr, c + CW_WORK, C.d_spill,
                                           C.refill_min, C.inner_min, n_dev, C.share, (unsigned)C.share_min_rays, S.sink, LQ, S.MS, MULTI ? XCD_STRIPES_OFF : stripe_arg(S.row));
    }
    if (LQ.steps) {
      ProfScope ps(KC_LONG);
      k_long_closest<XFORM, MULTI><<<tail_grid, 256, 0, st>>>(S.q, LQ.recs, LQ.count, S.minv, S.T, tnear, d_hits, c + CW_LONG_WORK, S.W, LQ.stk, S.hop);
    }
  }
}

// The any-hit step over the shadow list S.q: un-occluded rays are appended to `out` or end in S.sink.  BY_LANES: idx / n / n_dev as k_trace takes them (n = 0: the
// count is *n_dev), the grid sized for grid_rays;  BY_WAVES: the list's first CW_SHADOW rays.  (Any-hit packets are the single-mesh chain's own: any_packets.)
// early (single-mesh chains, BY_LANES; the conditions: single_pass): k_shade has stored every ray's deposit already and S.q holds thin rays (shade.inc store_shadow_early) --
// k_trace's MODE 2, which only takes an occluded ray's deposit back; `out` is not written.
template <bool MULTI>
static void any_step(StepMode mode, const TraceSrc &S, const unsigned *idx, size_t grid_rays, unsigned n, const unsigned *n_dev, RayPlanes out, unsigned *out_count, bool early = false) {
  Ctx &C = gctx();
  unsigned *c = C.d_counters;
  ProfScope ps(KC_ANY);
  if constexpr (!MULTI) {
    if (early && mode == BY_LANES) {
      launch_trace<true, true, 2, false>(trav_grid2(grid_rays), C.stream, S.q, idx, n, S.minv, S.T, GVT_RAY_EPSILON, nullptr, nullptr, out, out_count, c + CW_WORK, C.d_spill,
                                         C.refill_min, C.inner_min, n_dev, C.share, (unsigned)C.share_min_rays, S.sink, LongQ{}, S.MS, stripe_arg(S.row));
      C.early_deposit_launches++;
      return;
    }
  }
  if (mode == BY_WAVES) k_wave_any<MULTI><<<wave_grid(grid_rays), 256, 0, C.stream>>>(S.q, c + CW_SHADOW, S.minv, S.T, GVT_RAY_EPSILON, out, out_count, c + CW_WORK, S.sink, S.MS);
  else launch_trace<true, true, 1, MULTI>(trav_grid2(grid_rays), C.stream, S.q, idx, n, S.minv, S.T, GVT_RAY_EPSILON, nullptr, nullptr, out, out_count, c + CW_WORK, C.d_spill,
                                          C.refill_min, C.inner_min, n_dev, C.share, (unsigned)C.share_min_rays, S.sink, LongQ{}, S.MS, MULTI ? XCD_STRIPES_OFF : stripe_arg(S.row));
}

// The fields of ShadeArgs every chain sets alike (the rest is zero); the caller adds its source (in or W), and what else differs.
static ShadeArgs shade_args(const ChainBufs &B, const unsigned *idx, size_t n, int pass, const unsigned *n_dev, unsigned *next, unsigned *c_next, RayPlanes outp,
                            unsigned *out_count, const TraceParams &P) {
  unsigned *c = gctx().d_counters;
  ShadeArgs A{};
  A.idx = idx; A.n = (unsigned)n; A.hits = B.hits; A.first_pass = (pass == 0); A.carried_rng = 1; A.out = outp; A.out_count = out_count;
  A.shadow = B.shadow; A.shadow_count = c + CW_SHADOW; A.next_idx = next; A.next_count = c_next; A.lights = B.lights; A.normi = P.normi; A.normal_mode = P.normal_mode;
  A.n_lights = P.n_lights; A.seed = P.seed; A.zero_word = c + CW_WORK; A.sink = P.sink; A.n_dev = n_dev;
  return A;
}

// The shade step over A.n rays; lean: k_shade's LEAN instantiation (shade.inc; the callers' conditions)
template <bool MULTI>
static void shade_step(const ShadeArgs &A, const MeshView &mv, bool lean = false) {
  ProfScope ps(KC_SHADE);
  if (lean) k_shade<MULTI, true><<<blocks_for(A.n, SHADE_BLOCK), SHADE_BLOCK, 0, gctx().stream>>>(A, mv);
  else k_shade<MULTI><<<blocks_for(A.n, SHADE_BLOCK), SHADE_BLOCK, 0, gctx().stream>>>(A, mv);
}

int launch_closest(gvt_hip_mesh *M, RayPlanes q, const unsigned *idx, size_t n, bool xform, const Mat4 &minv, float tnear,
                   gvt_hip_hit *d_hits, bool counter_is_zero) {
  if (!n) return 0;
  Ctx &C = gctx();
  if (!M->d_nodes4) { int rc4 = build_nodes4(M); if (rc4) return rc4; }
  if (!counter_is_zero) HIPCHK(hipMemsetAsync(C.d_counters, 0, (CW_LONG_WORK + 1) * sizeof(unsigned), C.stream)); // CW_WORK .. CW_LONG_WORK
  LongQ LQ{};
  if (M->d_nodes4 && C.long_steps > 0 && n >= (size_t)C.long_min_rays) { // long rays are parked and traversed a wave per ray
    LongRec *recs = (LongRec *)scratch_get(SCR_LONG, long_scratch_bytes(n));
    if (!recs) return GVT_HIP_ERR_DEVICE;
    LQ = long_queue(recs, n);
  }
  TraceSrc S{};
  S.q = q; S.minv = minv; S.T = Trav{ M->d_nodes, M->d_tri, M->d_nodes4 };
  if (xform) closest_step<true, false>(BY_LANES, S, idx, n, nullptr, tnear, d_hits, LQ, LQ.recs);
  else closest_step<false, false>(BY_LANES, S, idx, n, nullptr, tnear, d_hits, LQ, LQ.recs);
  HIPCHK(hipGetLastError());
  C.stats.rays_closest += n;
  C.stats.launches_closest++;
  return 0;
}

int launch_visit_stats(gvt_hip_mesh *M, RayPlanes q, size_t n, float tnear, unsigned *d_out) {
  if (!n) return 0;
  Ctx &C = gctx();
  if (!M->d_nodes4) { int rc4 = build_nodes4(M); if (rc4) return rc4; }
  Trav T{ M->d_nodes, M->d_tri, M->d_nodes4 };
  unsigned *counter = C.d_counters + CW_WORK;
  HIPCHK(hipMemsetAsync(counter, 0, sizeof(unsigned), C.stream));
  k_visit_stats<<<trav_grid(n), TRAV_BLOCK, 0, C.stream>>>(q, (unsigned)n, T, tnear, d_out, counter, C.d_spill);
  HIPCHK(hipGetLastError());
  return 0;
}

int launch_wide_visit_stats(gvt_hip_mesh *M, RayPlanes q, size_t n, float tnear, const unsigned char *d_marks, unsigned *d_out) {
  if (!n) return 0;
  Ctx &C = gctx();
  Trav T{ M->d_nodes, M->d_tri, M->d_nodes4 };
  unsigned *counter = C.d_counters + CW_WORK;
  HIPCHK(hipMemsetAsync(counter, 0, sizeof(unsigned), C.stream));
  k_wide_visit_stats<<<trav_grid(n), TRAV_BLOCK, 0, C.stream>>>(q, (unsigned)n, T, tnear, d_marks, d_out, counter, C.d_spill);
  HIPCHK(hipGetLastError());
  return 0;
}

int launch_any_flags(gvt_hip_mesh *M, RayPlanes q, size_t n, bool xform, const Mat4 &minv, float tnear, int *d_flags) {
  if (!n) return 0;
  Ctx &C = gctx();
  if (!M->d_nodes4) { int rc4 = build_nodes4(M); if (rc4) return rc4; }
  Trav T{ M->d_nodes, M->d_tri, M->d_nodes4 };
  unsigned *counter = C.d_counters + CW_WORK;
  HIPCHK(hipMemsetAsync(counter, 0, sizeof(unsigned), C.stream));
  RayPlanes none{};
  {
    ProfScope ps(KC_ANY);
    if (xform) launch_trace<true, true, 0>(trav_grid2(n), C.stream, q, nullptr, (unsigned)n, minv, T, tnear, nullptr, d_flags, none, nullptr, counter, C.d_spill, C.refill_min, C.inner_min, nullptr, C.share, (unsigned)C.share_min_rays, TermSink{}, LongQ{}, MultiSrc{}, stripe_arg(0u));
    else launch_trace<true, false, 0>(trav_grid2(n), C.stream, q, nullptr, (unsigned)n, minv, T, tnear, nullptr, d_flags, none, nullptr, counter, C.d_spill, C.refill_min, C.inner_min, nullptr, C.share, (unsigned)C.share_min_rays, TermSink{}, LongQ{}, MultiSrc{}, stripe_arg(0u));
  }
  HIPCHK(hipGetLastError());
  C.stats.rays_any += n;
  C.stats.launches_any++;
  return 0;
}

// Adapter::trace on device planes.  `in` holds n rays at [0,n); `out` must have been reserved for
// out->size + n*(1+n_lights) -- what the first pass can emit; further passes (bounces) grow it themselves.  On return out->size is exact (one small read-back).
int trace_core(gvt_hip_mesh *M, RayPlanes in, size_t n, uint64_t index_base, gvt_hip_queue *out, const TraceParams &P,
               const gvt_hip_light *lights_host) {
  Ctx &C = gctx();
  C.stats.trace_calls++;
  if (!n) return 0;
  hipStream_t st = C.stream;
  const int nL = P.n_lights;
  ChainBufs B;
  int rc = chain_bufs(B, n, nL, lights_host);
  if (rc) return rc;
  RayPlanes outp = make_planes(out->d_planes, out->cap);
  unsigned *c = C.d_counters;
  static_assert(CW_BOUNCE_A == CW_SHADOW + 1, "the pass's two counts are reset and read back as one run");
  k_trace_begin<<<1, 64, 0, st>>>(out->d_count, (unsigned)out->size, c); // CW_WORK .. CW_LONG_WORK
  const MeshView mv = mesh_view(M);
  TraceSrc SA{}; // the shadow rays' any-hit step
  SA.q = B.shadow; SA.minv = P.minv; SA.T = Trav{ M->d_nodes, M->d_tri, M->d_nodes4 }; SA.sink = P.sink;

  size_t n_active = n;
  const size_t out_size0 = out->size;
  const unsigned *idx = nullptr;
  unsigned *next = B.idx_a;
  int pass = 0;
  while (n_active) { // while (validRayLeft) :465
    // ray sorting: traverse in Morton order of the object-space origin
    if (C.sort_rays && n_active >= 8192 && (rc = sort_ray_list(M, in, &idx, n_active, n, P.minv))) return rc;
    if (idx && C.sort_rays && C.sort_gather && n_active >= 8192) {
      float4 *od = (float4 *)scratch_get(SCR_SORT_GATHER, sizeof(float4) * 2 * n);
      if (!od) return GVT_HIP_ERR_DEVICE;
      {
        ProfScope ps(KC_SORT);
        k_gather_od<<<blocks_for(n_active), 256, 0, st>>>(in, idx, (unsigned)n_active, P.minv, od, od + n);
      }
      HIPCHK(hipGetLastError());
      RayPlanes sorted{ od, od + n, nullptr, nullptr, nullptr };
      rc = launch_closest(M, sorted, nullptr, n_active, false, P.minv, GVT_RAY_EPSILON, B.hits, pass == 0);
    } else
      rc = launch_closest(M, in, idx, n_active, true, P.minv, GVT_RAY_EPSILON, B.hits, pass == 0);
    if (rc) return rc;
    if (pass > 0) HIPCHK(hipMemsetAsync(c + CW_SHADOW, 0, 2 * sizeof(unsigned), st)); // CW_SHADOW, CW_BOUNCE_A (pass 0: k_trace_begin)
    ShadeArgs A = shade_args(B, idx, n_active, pass, nullptr, next, c + CW_BOUNCE_A, outp, out->d_count, P);
    A.in = in; A.index_base = index_base; A.carried_rng = P.carried_rng; A.update_in_place = P.update_in_place;
    shade_step<false>(A, mv);
    HIPCHK(hipGetLastError());
    C.stats.rays_shaded += n_active;
    // traceShadowRays :364-385.  The shadow-ray count stays on the device (the persistent kernel reads it, the grid does not depend on it);
    // the host learns the counts of the pass in ONE read-back afterwards.
    const size_t shadow_ub = n_active * (size_t)nL;
    if (shadow_ub) {
      any_step<false>(BY_LANES, SA, nullptr, shadow_ub, 0u, c + CW_SHADOW, outp, out->d_count); // (the work counter: zeroed by k_shade)
      HIPCHK(hipGetLastError());
      C.stats.launches_any++;
    }
    HIPCHK(hipMemcpyAsync(C.h_pinned, c + CW_SHADOW, 2 * sizeof(unsigned), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(C.h_pinned + 2, out->d_count, sizeof(unsigned), hipMemcpyDeviceToHost, st));
    if ((rc = trav_overflow_fetch_async())) return rc;
    HIPCHK(hipStreamSynchronize(st));
    if ((rc = trav_overflow_result())) return rc;
    const unsigned n_shadow = C.h_pinned[0], n_next = C.h_pinned[1];
    C.stats.rays_any += n_shadow;
    n_active = n_next;
    idx = next;
    next = (next == B.idx_a) ? B.idx_b : B.idx_a;
    pass++;
    if (n_active) { // a further pass (bounces): room for everything IT can emit -- a forward or nL shadow rays per ray -- behind what is there
      out->size = C.h_pinned[2];
      if ((rc = queue_reserve(out, out->size + n_active * (size_t)(1 + nL)))) return rc;
      outp = make_planes(out->d_planes, out->cap);
    }
  }
  C.stats.rays_forwarded += C.h_pinned[2] - out_size0; // read back with the last pass
  out->size = C.h_pinned[2];
  return 0;
}

extern "C" int gvt_hip_math_probe(int kind, const float *in, size_t n, float *out) {
  if (ensure_init()) return GVT_HIP_ERR_NODEVICE;
  if (kind < 0 || kind > 2 || (n && (!in || !out)) || n > 0xffffffffull) { set_error("math_probe: bad argument"); return GVT_HIP_ERR_INVALID; }
  if (!n) return 0;
  Ctx &C = gctx();
  float *d = (float *)scratch_get(SCR_GENERAL, sizeof(float) * 2 * n);
  if (!d) return GVT_HIP_ERR_DEVICE;
  HIPCHK(hipMemcpyAsync(d, in, sizeof(float) * n, hipMemcpyHostToDevice, C.stream));
  k_math_probe<<<blocks_for(n), 256, 0, C.stream>>>(kind, d, (unsigned)n, d + n);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(out, d + n, sizeof(float) * n, hipMemcpyDeviceToHost, C.stream));
  HIPCHK(hipStreamSynchronize(C.stream));
  return 0;
}

// ------------------------------------------------------------------------------------------------
// Merged launch chain of one scheduler round (gvt_internal.h "wave"): closest hit -> shade -> any hit over the rays of all local
// queues at once, `passes` times (bounces), WITHOUT any host round trip: later passes read their ray count from device memory.
// ------------------------------------------------------------------------------------------------
namespace {
// segs (pass 0 of a merged chain whose queues were filled by the camera filter without a read-back; the host uploaded the segments with
// the BOUNDS it knows): each segment's length is its queue's count word, its beginning the sum of the lengths before it, the list's
// length goes to *n_dev0 (a handful of segments: one thread)
__global__ void k_wave_pass_begin(unsigned *c, int pass, unsigned n_host, unsigned *out_count, const unsigned *n_dev0 = nullptr, WaveSeg *segs = nullptr, int n_seg = 0,
                                  unsigned *const *__restrict__ count_ptr = nullptr) {
  if (blockIdx.x || threadIdx.x) return;
  if (segs) {
    unsigned run = 0;
    for (int k = 0; k < n_seg; k++) { const unsigned n = *count_ptr[segs[k].inst]; segs[k].begin = run; segs[k].n = n; run += n; }
    *const_cast<unsigned *>(n_dev0) = run;
  }
  unsigned long long *tot = cw_totals(c);
  const int cur = cw_bounce(pass), prev = cw_bounce(pass + 1);
  if (pass == 0) { *out_count = 0u; c[CW_BOUNCE_A] = 0u; c[CW_BOUNCE_B] = 0u; tot[TOT_CLOSEST] += n_dev0 ? *n_dev0 : n_host; }
  else { tot[TOT_ANY] += c[CW_SHADOW]; tot[TOT_CLOSEST] += c[prev]; c[cur] = 0u; }
  c[CW_LONG_FRAME] += c[CW_LONG]; // rays parked by the launch before (the frame's total: the tracer adapts its parking threshold to it)
  cw_zero_work(c); c[CW_SHADOW] = 0u; c[CW_LONG] = 0u; c[CW_LONG_WORK] = 0u; c[CW_PKT_RETRY] = 0u;
  for (int k = 0; k < SHADOW_CLASSES; k++) c[CW_SHADOW_CLS + k] = 0u; // the shadow list's class counts (shade.inc)
}
// end of a round's chain: the last pass's shadow rays into the frame total; and the traced queues' clear() (count words of the
// queues whose mask byte is set) in the same launch
__global__ void k_wave_end(unsigned *c, unsigned *const *__restrict__ count_ptr, const unsigned char *__restrict__ mask, int n_inst) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) cw_totals(c)[TOT_ANY] += c[CW_SHADOW];
  if (count_ptr && i < n_inst && mask[i]) *count_ptr[i] = 0u;
}
} // namespace

// what the passes of a round's chain share, whichever kernels they use
struct Chain {
  size_t n; int passes; // rays of pass 0 (or their bound): what every launch is sized by
  const TraceParams &P; const gvt_hip_light *lights_host; gvt_hip_queue *out; RayPlanes outp;
  ChainBufs B;
  int *d_shadow_inst;   // instance of every shadow ray (merged kernels; any-hit packets: < 0 marks an empty slot)
  LongRec *d_long;
  bool use_long, small; // k_trace parks long rays | a wave per ray (see k_long_seed)
  const unsigned *nd0;  // pass 0's ray count where only the device knows it
};
// a pass's ray count on the device (null: K.n), its list (null: the identity), the bounce list it writes and that list's count word
struct Pass { int pass; const unsigned *n_dev, *idx; unsigned *next, *c_next; };

// shadow rays as packets (single-mesh chains, knob packet = 2): the direct-mapped list a packet of 64 per wave, then the rays of packets that bailed out a
// lane per ray (an empty list costs a few microseconds)
static int any_packets(const Chain &K, const TraceSrc &S) {
  Ctx &C = gctx();
  unsigned *c = C.d_counters;
  unsigned *d_retry = (unsigned *)scratch_get(SCR_PKT_RETRY, sizeof(unsigned) * K.B.shadow_cap);
  if (!d_retry) return GVT_HIP_ERR_DEVICE;
  ProfScope ps(KC_ANY);
  k_packet<true><<<blocks_for(K.B.shadow_cap), 256, 0, C.stream>>>(S.q, (unsigned)K.B.shadow_cap, nullptr, S.minv, S.T, GVT_RAY_EPSILON, nullptr, K.d_shadow_inst, K.outp, K.out->d_count,
                                                                 S.sink, LongQ{}, d_retry, c + CW_PKT_RETRY, cw_totals(c) + TOT_ANY, c + CW_PACKETS);
  launch_trace<true, true, 1>(trav_grid2(4096), C.stream, S.q, d_retry, 0u, S.minv, S.T, GVT_RAY_EPSILON, nullptr, nullptr, K.outp, K.out->d_count, c + CW_WORK, C.d_spill,
                              C.refill_min, C.inner_min, c + CW_PKT_RETRY, C.share, (unsigned)C.share_min_rays, S.sink, LongQ{}, MultiSrc{}, stripe_arg(0u));
  return 0;
}

// One segment (a single non-empty local queue, e.g. the one-domain benchmark): the single-mesh kernels -- no segment lookup and no per-ray table loads at a
// refill -- with the same device-side counts.  Its own: bounce sorting, packets for the shadow rays, the class-ordered shadow list (cls_stride slots per class).
static int single_pass(const Chain &K, Pass p, const WaveSingle &W1, size_t cls_stride) {
  Ctx &C = gctx();
  unsigned *c = C.d_counters;
  gvt_hip_mesh *M = W1.mesh;
  const size_t n = K.n;
  const int nL = K.P.n_lights;
  const bool have4 = M->d_nodes4 != nullptr, by_class = K.B.steps != nullptr;
  // ray sorting where it should pay (knob sort_rays, off by default: measured, profiles/r06_sort_cfg5.txt): a BOUNCE list -- secondary rays in their parents'
  // order, i.e. neighbours in the list leave neighbouring surface points in unrelated directions -- is reordered by direction octant, then the Morton cell of the
  // ray's origin (k_ray_keys) before the closest-hit launch; the pass's shadow rays inherit the order (k_shade allocates their slots in list order).  The list's
  // length lives on the device: all n entries of the bound are sorted, the unused ones with the largest key
  if (C.sort_rays && p.pass > 0 && n >= 8192 && have4)
    if (int rc = sort_ray_list(M, W1.planes, &p.idx, n, n, W1.minv, p.n_dev)) return rc;
  TraceSrc S{};
  S.q = W1.planes; S.minv = W1.minv; S.T = Trav{ M->d_nodes, M->d_tri, M->d_nodes4 };
  S.row = (W1.coherent && p.pass == 0 && !p.idx) ? W1.row_rays : 0u; // the camera's list in tile order; bounce lists have no film geometry
  LongQ LQ{};
  if (K.use_long && have4) LQ = long_queue(K.d_long, n);
  LQ.steps_out = K.B.steps;
  const bool small1 = K.small && have4;
  // a coherent list (camera rays in 8x8 tiles, straight from the filter) over a mesh the builder found packet-friendly (walks_packets): a wave walks the tree
  // ONCE for 64 rays (k_packet) -- the reference chooses its packet width per build as well (EmbreeMeshAdapter.cpp:50-74)
  const bool pkt = walks_packets(C, M, n) && W1.coherent && p.pass == 0 && have4 && !small1;
  // ... the CLOSEST hit, that is.  Shadow rays as packets lost on both surfaces they were measured on (bun_zipper any hit 0.162 -> 0.189 ms, the hall
  // 1.23 -> 1.33: an any-hit packet goes on until its LAST ray is occluded or through): under the per-mesh choice they stay a lane per ray; 2 forces both
  const bool pkt_any = pkt && C.packet == 2;
  closest_step<true, false>(pkt ? BY_PACKETS : small1 ? BY_WAVES : BY_LANES, S, p.idx, n, p.n_dev, GVT_RAY_EPSILON, K.B.hits, LQ, K.d_long);
  ShadeArgs A = shade_args(K.B, p.idx, n, p.pass, p.n_dev, p.next, p.c_next, K.outp, K.out->d_count, K.P);
  A.in = W1.planes; A.normi = W1.normi; A.sink.from = W1.inst;
  if (pkt_any) { A.shadow_inst = K.d_shadow_inst; A.shadow_stride = (unsigned)n; } // shadow rays in the primaries' order: packets again
  A.steps = K.B.steps; A.cls_cnt = by_class ? c + CW_SHADOW_CLS : nullptr; A.cls_stride = (unsigned)cls_stride; A.cls_lo = C.shadow_cls_lo; A.cls_shift = C.shadow_cls_shift;
  // the simple frame (k_shade's LEAN instantiation): camera rays of the scene's only instance, depth 1, no area light, a LAMBERT mesh material
  const bool lean_shade = W1.coherent && p.pass == 0 && K.passes == 1 && K.P.sink.fb && K.P.sink.top.n_inst == 1 && nL >= 1 && plain_lambert(M) && no_area_light(K.lights_host, nL);
  // ... and of it the frame in which every pixel has one writer -- one light, and the frame loop's word that these are the camera's rays, one per pixel, over a
  // framebuffer it has just cleared (TraceParams::one_writer) --, its shadow rays a lane per ray: the deposit is stored by k_shade and taken back by the any-hit launch
  // where the ray is occluded (knob early_deposit; shade.inc store_shadow_early, k_trace's MODE 2)
  const bool early_deposit = lean_shade && nL == 1 && K.P.one_writer && !small1 && !pkt_any && C.early_deposit;
  A.early_deposit = early_deposit ? 1 : 0;
  shade_step<false>(A, mesh_view(M), lean_shade);
  if (!nL) return 0;
  TraceSrc SA = S;
  SA.q = K.B.shadow; SA.sink = A.sink; SA.row = 0u;
  if (pkt_any) return any_packets(K, SA);
  if (by_class) { SA.MS.cls_cnt = c + CW_SHADOW_CLS; SA.MS.cls_stride = (unsigned)cls_stride; SA.MS.cls_total = c + CW_SHADOW; }
  any_step<false>(small1 ? BY_WAVES : BY_LANES, SA, nullptr, K.B.shadow_cap, 0u, by_class ? nullptr : c + CW_SHADOW, K.outp, K.out->d_count, early_deposit);
  return 0;
}

// Several segments: the MULTI kernels.  Their own: hops (d_hop), direct-mapped shadow slots, the source instance of every ray appended (d_out_from).
static void merged_pass(const Chain &K, const Pass &p, const WaveSet &W, const ChainOpts &O, int *d_hop, int *d_out_from) {
  Ctx &C = gctx();
  unsigned *c = C.d_counters;
  const TraceParams &P = K.P;
  const size_t n = K.n;
  const int nL = P.n_lights;
  TraceSrc S{};
  S.W = W; S.MS.W = W; S.hop = d_hop;
  if (d_hop) {
    S.sink = P.sink;
    S.MS.hop_inst = d_hop; S.MS.hop_read = p.pass > 0; S.MS.hop_owner = P.hop_owner; S.MS.hop_rank = P.hop_rank; S.MS.hop_tot = cw_totals(c) + TOT_CLOSEST; S.MS.hop_early = P.hop == 1 ? 1 : 0;
  }
  LongQ LQ{};
  if (K.use_long) LQ = long_queue(K.d_long, n);
  // the round's queues hold camera rays in tile order, over packet-friendly meshes only: the closest hits a packet of 64 rays per wave
  const bool pktm = O.multi_packets && p.pass == 0 && !K.small && p.idx == nullptr;
  closest_step<true, true>(pktm ? BY_PACKETS : K.small ? BY_WAVES : BY_LANES, S, p.idx, n, p.n_dev, GVT_RAY_EPSILON, K.B.hits, LQ, K.d_long, p.pass > 0);
  ShadeArgs A = shade_args(K.B, p.idx, n, p.pass, p.n_dev, p.next, p.c_next, K.outp, K.out->d_count, P);
  A.W = W; A.out_from = d_out_from; A.shadow_inst = K.d_shadow_inst; A.hop_inst = d_hop;
  const bool direct = C.shadow_direct && p.pass == 0 && !K.small; // later passes and small rounds hold few rays: compacted slots
  // (k_shade marks every slot below the stride -- the bound -- empty or taken; with one light the list is as long as the traced one,
  // and where only the device knows that length the any-hit launch stops there instead of skipping empty slots up to the bound)
  const bool direct_dev = direct && K.nd0 != nullptr && nL == 1;
  A.shadow_stride = direct ? (unsigned)n : 0u;
  // (k_shade's LEAN instantiation for the merged chain: depth 1, no area light, plain LAMBERT meshes; a missing ray still walks the instances ahead of it)
  const bool lean_multi = O.simple_meshes && p.pass == 0 && K.passes == 1 && nL >= 1 && no_area_light(K.lights_host, nL);
  shade_step<true>(A, MeshView{}, lean_multi);
  if (!nL) return;
  TraceSrc SA{};
  SA.q = K.B.shadow; SA.sink = P.sink;
  SA.MS = MultiSrc{ W, K.d_shadow_inst, d_out_from, direct ? cw_totals(c) + TOT_ANY : nullptr };
  // (an un-occluded shadow ray goes on the same way -- not in the early mode: 1.372 -> 1.340 ms on the soup tiles without)
  if (d_hop && P.sink.fb && P.hop == 2) { SA.MS.hop_owner = P.hop_owner; SA.MS.hop_rank = P.hop_rank; SA.MS.hop_tot = cw_totals(c) + TOT_CLOSEST; }
  if (K.small) any_step<true>(BY_WAVES, SA, nullptr, K.B.shadow_cap, 0u, nullptr, K.outp, K.out->d_count);
  else any_step<true>(BY_LANES, SA, nullptr, K.B.shadow_cap, direct ? (unsigned)K.B.shadow_cap : 0u, direct ? (direct_dev ? K.nd0 : nullptr) : c + CW_SHADOW, K.outp, K.out->d_count);
}

int wave_trace_chain(const WaveSet &W, size_t n_total, int passes, gvt_hip_queue *out, int *d_out_from, const TraceParams &P,
                     const gvt_hip_light *lights_host, const WaveSingle *single, const ChainOpts &O) {
  Ctx &C = gctx();
  if (!n_total) return 0;
  hipStream_t st = C.stream;
  const int nL = P.n_lights;
  const size_t n = n_total;
  // a single-mesh round with one light: the shadow rays listed by how long their primaries' tiles took, the longest first (knob shadow_order; shade.inc) --
  // SHADOW_CLASSES regions of `cls_stride` slots; not for packets (no per-ray step counts) nor small rounds (a wave per ray)
  const bool by_class_wanted = single && single->mesh->d_nodes4 && C.shadow_order && nL == 1 && n >= (size_t)C.shadow_order_min_rays && n > (size_t)C.small_rays &&
                               C.long_steps > 0 && n >= (size_t)C.long_min_rays && !(walks_packets(C, single->mesh, n) && single->coherent);
  const size_t cls_stride = (n + 63) & ~(size_t)63;
  // (every region has room for the whole list; beyond 8 GiB the list stays in arrival order -- and after one refusal: chain_bufs)
  const size_t ordered_slots = (by_class_wanted && !C.shadow_order_denied && cls_stride * SHADOW_CLASSES * 64 <= ((size_t)8 << 30)) ? cls_stride * SHADOW_CLASSES : 0;
  const size_t shadow_slots = ordered_slots ? ordered_slots : n * (size_t)(nL > 0 ? nL : 1);
  if (shadow_slots >= 0xffffffffull) { set_error("round: %zu shadow slots exceed the 32-bit slot counters", shadow_slots); return GVT_HIP_ERR_INVALID; }
  Chain K{ n, passes, P, lights_host, out, make_planes(out->d_planes, out->cap) };
  int rc = chain_bufs(K.B, n, nL, lights_host, ordered_slots);
  if (rc) return rc;
  K.d_shadow_inst = (int *)scratch_get(SCR_SHADOW_INST, sizeof(int) * K.B.shadow_cap);
  K.d_long = (LongRec *)scratch_get(SCR_LONG, long_scratch_bytes(n));
  if (!K.d_shadow_inst || !K.d_long) return GVT_HIP_ERR_DEVICE;
  // hops (MultiSrc, trace_lane.inc): in a merged chain a ray that leaves its instance without a hit goes on into the next instance of this rank inside the launch;
  // d_hop[virtual index] = the instance it is in now (-1: its segment's), for the kernels behind (k_long_closest, k_shade, the next pass's refill)
  int *d_hop = nullptr;
  if (!single && P.hop && P.sink.fb) {
    d_hop = (int *)scratch_get(SCR_HOP, sizeof(int) * n);
    if (!d_hop) return GVT_HIP_ERR_DEVICE;
    HIPCHK(hipMemsetAsync(d_hop, 0xff, sizeof(int) * n, st));
  }
  unsigned *c = C.d_counters;
  K.use_long = C.long_steps > 0 && n >= (size_t)C.long_min_rays;
  K.small = n <= (size_t)C.small_rays;
  // pass 0's ray count where only the device knows it (the chain straight behind the camera filter): the single queue's count word, or
  // the word the caller's segment kernel left the merged list's length in (n_total is then the bound the launches are sized by)
  K.nd0 = single ? single->n_dev : O.n_dev0_multi;
  for (int pass = 0; pass < passes; pass++) {
    unsigned *const lists[2] = { K.B.idx_a, K.B.idx_b };
    // (the count written by the previous pass's k_shade and its bounce list)
    const Pass p{ pass, pass ? c + cw_bounce(pass - 1) : K.nd0, pass ? lists[(pass - 1) & 1] : nullptr, lists[pass & 1], c + cw_bounce(pass) };
    if (!(pass == 0 && single && single->pass0_begun))
      k_wave_pass_begin<<<1, 64, 0, st>>>(c, pass, (unsigned)n, out->d_count, K.nd0, (pass == 0 && O.n_dev0_multi && !single) ? const_cast<WaveSeg *>(W.segs) : nullptr, W.n_seg, O.d_count_ptr);
    if (!single) merged_pass(K, p, W, O, d_hop, d_out_from);
    else if ((rc = single_pass(K, p, *single, cls_stride))) return rc;
    HIPCHK(hipGetLastError());
    C.stats.launches_closest++;
    C.stats.launches_any++;
  }
  if (!O.defer_end) k_wave_end<<<(unsigned)((std::max(O.n_inst, 1) + 255) / 256), 256, 0, st>>>(c, O.d_count_ptr, O.d_mask, O.n_inst); // + queue[instTarget].clear()
  HIPCHK(hipGetLastError());
  C.stats.trace_calls++;
  return 0;
}

// A small round in ONE launch (finish_kernel.inc): the rays of the segments in W are traced, shaded, their shadow rays traced and
// everything that moves on is followed through this rank's instances; rays for other ranks' instances are appended to their queues
// (which must have room: n_total * (1 + n_lights * depth) each), everything else ends in the framebuffer.  No shuffle follows.
// spec_words != nullptr: the launch is enqueued ahead of the host's knowledge (domain.hip): n_total is only the bound its grid is sized by, the count is
// spec_words[2], the launch is void unless spec_words[1]; the light list must be resident already (no upload, no synchronisation in here)
int finish_round(const WaveSet &W, size_t n_total, const TraceParams &P, const gvt_hip_light *lights_host, const void *d_qdesc, const int *d_owner, int rank,
                 unsigned *d_queue_overflow, unsigned *const *d_count_ptr, const unsigned char *d_mask, const unsigned *spec_words) {
  Ctx &C = gctx();
  if (!n_total) return 0;
  const int nL = P.n_lights;
  gvt_hip_light *d_lights;
  if (int rc = lights_on_device(lights_host, nL, &d_lights, spec_words == nullptr)) return rc;
  FinishArgs A;
  A.n_dev = spec_words ? spec_words + 2 : nullptr; A.valid = spec_words ? spec_words + 1 : nullptr;
  A.W = W; A.n = (unsigned)n_total; A.lights = d_lights; A.n_lights = nL; A.normal_mode = P.normal_mode;
  A.top = P.sink.top; A.fb = P.sink.fb; A.n_pix = P.sink.n_pix;
  A.queues = (const QueueDesc *)d_qdesc; A.owner = d_owner; A.rank = rank;
  A.counter = C.d_counters + CW_WORK; A.tot = cw_totals(C.d_counters); // (FinishArgs::tot: [TOT_CLOSEST], [TOT_ANY])
  A.queue_overflow = d_queue_overflow; A.trav_overflow = C.d_counters + CW_TRAV_OVF;
  A.seed = P.seed; A.index_base = 0ull; A.skip_known = C.skip_known;
  A.count_ptr = d_count_ptr; A.clear_mask = d_mask; A.n_inst = W.n_inst;
  // (the work counter is 0: the frame's start and every round's report leave it so -- k_zero_totals, k_round_report)
  {
    ProfScope ps(KC_CLOSEST);
    k_finish<<<(int)std::min<size_t>((n_total + 3) / 4, (size_t)C.n_cu * 4), 256, 0, C.stream>>>(A); // 40 KiB of LDS per block: four blocks per CU
  }
  HIPCHK(hipGetLastError());
  C.stats.launches_closest++;
  C.stats.trace_calls++;
  return 0;
}

int set_device_u32(unsigned *p, unsigned v) {
  k_set_u32<<<1, 64, 0, gctx().stream>>>(p, v);
  HIPCHK(hipGetLastError());
  return 0;
}

// ---- the batched wire pair: all the queues of one exchange message through ONE launch (convert.inc k_queues_to_wire / k_wire_to_queues)
#define WIRE_MAX_QUEUES 256
static_assert(sizeof(QueueDesc) * WIRE_MAX_QUEUES + sizeof(unsigned) * (3 * WIRE_MAX_QUEUES + 1) <= PINNED_STAGE_BYTES, "the queue table fits the staging block");

int pinned_stage_begin(void **h) {
  Ctx &C = gctx();
  if (!C.h_wire) {
    HIPCHK(hipHostMalloc(&C.h_wire, PINNED_STAGE_BYTES, hipHostMallocDefault));
    HIPCHK(hipEventCreateWithFlags(&C.wire_ev, hipEventDisableTiming));
  }
  if (C.wire_busy) HIPCHK(hipEventSynchronize(C.wire_ev));
  *h = C.h_wire;
  return 0;
}
int pinned_stage_end() {
  Ctx &C = gctx();
  HIPCHK(hipEventRecord(C.wire_ev, C.stream));
  C.wire_busy = true;
  return 0;
}

namespace {
// The launch's queue table: built in the context's pinned staging block (one block: the event says when its last upload has been read),
// copied to the context's device copy on the stream.  runs[i]: rays of queue i in the message; append: they go behind the queue's fill
int wire_table(gvt_hip_queue *const *queues, size_t n, const uint64_t *runs, bool append, WireTable &W) {
  Ctx &C = gctx();
  const size_t o_begin = sizeof(QueueDesc) * n, o_off = o_begin + sizeof(unsigned) * (n + 1), o_fill = o_off + sizeof(unsigned) * n,
               bytes = o_fill + sizeof(unsigned) * n;
  char *d = (char *)scratch_get(SCR_WIRE_TABLE, bytes);
  if (!d) return GVT_HIP_ERR_DEVICE;
  void *stage = nullptr;
  int rc;
  if ((rc = pinned_stage_begin(&stage))) return rc;
  char *h = (char *)stage;
  QueueDesc *q = (QueueDesc *)h;
  unsigned *begin = (unsigned *)(h + o_begin), *off = (unsigned *)(h + o_off), *fill = (unsigned *)(h + o_fill);
  unsigned at = 0;
  for (size_t i = 0; i < n; i++) {
    q[i].planes = queues[i]->d_planes; q[i].cap = queues[i]->cap; q[i].count = queues[i]->d_count; q[i].keep = 0u;
    begin[i] = at;
    off[i] = append ? (unsigned)queues[i]->size : 0u;
    fill[i] = append ? (unsigned)(queues[i]->size + runs[i]) : 0u;
    at += (unsigned)runs[i];
  }
  begin[n] = at;
  HIPCHK(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, C.stream));
  if ((rc = pinned_stage_end())) return rc;
  W.q = (const QueueDesc *)d; W.begin = (const unsigned *)(d + o_begin); W.off = (const unsigned *)(d + o_off); W.fill = (const unsigned *)(d + o_fill);
  W.n = (int)n;
  return 0;
}
} // namespace

extern "C" int gvt_hip_queues_export_wire(gvt_hip_queue *const *queues, size_t n, gvt_hip_ray *dst_device, size_t cap_rays, uint64_t *counts_out,
                                          uint64_t *total_out) {
  if (ensure_init()) return GVT_HIP_ERR_NODEVICE;
  if (!queues || !total_out || n < 1 || n > WIRE_MAX_QUEUES) { set_error("queues_export_wire: null argument or %zu queues (1..%d)", n, WIRE_MAX_QUEUES); return GVT_HIP_ERR_INVALID; }
  uint64_t runs[WIRE_MAX_QUEUES];
  uint64_t total = 0;
  for (size_t i = 0; i < n; i++) {
    if (!queues[i]) { set_error("queues_export_wire: queue %zu is null", i); return GVT_HIP_ERR_INVALID; }
    runs[i] = queues[i]->size;
    total += runs[i];
  }
  *total_out = total;
  if (counts_out) std::copy(runs, runs + n, counts_out);
  if (total > cap_rays) { set_error("queues_export_wire: %llu rays, capacity %zu", (unsigned long long)total, cap_rays); return GVT_HIP_ERR_CAPACITY; }
  if (!total) return 0;
  if (!dst_device) { set_error("queues_export_wire: null destination"); return GVT_HIP_ERR_INVALID; }
  if (total >= 0xffffffffull) { set_error("queues_export_wire: %llu rays exceed the 32-bit ray index", (unsigned long long)total); return GVT_HIP_ERR_INVALID; }
  Ctx &C = gctx();
  WireTable W;
  int rc = wire_table(queues, n, runs, false, W);
  if (rc) return rc;
  {
    ProfScope ps(KC_CONVERT);
    const unsigned blocks = (unsigned)((total + WIRE_BLOCK - 1) / WIRE_BLOCK);
    k_queues_to_wire<<<blocks, WIRE_BLOCK, 0, C.stream>>>(W, (unsigned)total, (float4 *)dst_device);
  }
  HIPCHK(hipGetLastError());
  for (size_t i = 0; i < n; i++) queues[i]->size = 0; // (the launch cleared the count words)
  HIPCHK(hipStreamSynchronize(C.stream));
  return 0;
}

extern "C" int gvt_hip_queues_append_wire(gvt_hip_queue *const *queues, size_t n, const gvt_hip_ray *src_device, const uint64_t *counts) {
  if (ensure_init()) return GVT_HIP_ERR_NODEVICE;
  if (!queues || !counts || n < 1 || n > WIRE_MAX_QUEUES) { set_error("queues_append_wire: null argument or %zu queues (1..%d)", n, WIRE_MAX_QUEUES); return GVT_HIP_ERR_INVALID; }
  uint64_t total = 0;
  for (size_t i = 0; i < n; i++) {
    if (!queues[i]) { set_error("queues_append_wire: queue %zu is null", i); return GVT_HIP_ERR_INVALID; }
    for (size_t k = 0; k < i && counts[i]; k++)
      if (queues[k] == queues[i] && counts[k]) { set_error("queues_append_wire: queue %zu appears twice", i); return GVT_HIP_ERR_INVALID; }
    total += counts[i];
  }
  if (!total) return 0;
  if (!src_device) { set_error("queues_append_wire: null source"); return GVT_HIP_ERR_INVALID; }
  if (total >= 0xffffffffull) { set_error("queues_append_wire: %llu rays exceed the 32-bit ray index", (unsigned long long)total); return GVT_HIP_ERR_INVALID; }
  int rc;
  for (size_t i = 0; i < n; i++)
    if (counts[i] && (rc = queue_reserve(queues[i], queues[i]->size + counts[i]))) return rc;
  Ctx &C = gctx();
  WireTable W;
  if ((rc = wire_table(queues, n, counts, true, W))) return rc;
  {
    ProfScope ps(KC_CONVERT);
    const unsigned blocks = (unsigned)((total + WIRE_BLOCK - 1) / WIRE_BLOCK);
    k_wire_to_queues<<<blocks, WIRE_BLOCK, 0, C.stream>>>((const float4 *)src_device, (unsigned)total, W);
  }
  HIPCHK(hipGetLastError());
  for (size_t i = 0; i < n; i++) queues[i]->size += counts[i];
  return 0;
}
