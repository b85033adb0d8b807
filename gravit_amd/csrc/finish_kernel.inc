// finish_kernel.inc -- k_finish: a SMALL scheduler round in one launch, a whole wave per ray, every ray followed to its end on this
// rank (included by trace.hip).
//
// After the first round of a multi-domain frame a rank holds a few hundred to a few thousand rays: misses and un-occluded shadow
// rays that move on to a neighbouring domain, bounce rays.  As rounds -- closest hit, shade, any hit, shuffle, report, once per hop --
// each of them costs the latency floors of five launches and a host synchronisation whatever it carries (8 soup tiles on one rank:
// 7 such rounds behind the first one).  Here ONE kernel gives every queued ray a wave and runs the ray's whole life on this rank:
//   closest hit in its instance (the wave opens 64 pending nodes per step: k_long_closest's scheme)
//   -> miss: shuffleRays' rule (TracerBase.h:392-400) at once -- no other instance ahead: a SHADOW ray deposits, anything else ends;
//            an instance of THIS rank: the ray goes on there in the same wave; another rank's: appended to that instance's queue
//   -> hit:  a SHADOW ray is dropped (EmbreeMeshAdapter.cpp:486-488); otherwise normal / material / Shade per light (k_shade's code),
//            each shadow ray traced at once (any hit, a wave per ray like k_wave_any) and, un-occluded, followed through the
//            instances ahead of it the same way; then the Russian-roulette bounce (:584-602) continues the loop with the new ray.
// The same rays are traced, in the same instances, with the same arithmetic and RNG streams as the rounds would trace them (the
// ray counters agree with the oracle's restated schedulers); only the order of framebuffer deposits differs.  RNG: every ray the
// schedulers produce carries its stream word (camera_stream_word is never 0); a ray injected with word 0 is keyed like k_shade's first
// pass on (seed, index in THIS round's list) and keeps that key while it moves between this rank's instances inside the launch --
// the rounds would key it again on its index in the next round's list: such rays shade differently with finish_rays on and off.  Used for rounds of at
// most `finish_rays` rays when the terminal sink is on.
struct FinishArgs {
  WaveSet W;                    // the non-empty local queues (segments) + the per-instance table
  unsigned n;                   // rays of the round (host-known)
  const gvt_hip_light *lights;
  int n_lights, normal_mode;
  TopDev top;                   // the instance boxes (shuffleRays)
  float *fb;
  unsigned n_pix;
  const QueueDesc *queues;      // every instance's queue (rays for other ranks are appended there)
  const int *owner;             // owner[i] = rank of instance i; rank < 0: every instance is local (replicated scene)
  int rank;
  unsigned *counter;            // work counter (zeroed by the caller)
  unsigned long long *tot;      // frame totals: [0] closest-hit rays, [1] any-hit rays
  unsigned *queue_overflow;     // bit 0: a destination queue without room
  unsigned *trav_overflow;      // traversal list overflow flag word
  uint32_t seed;                // k_shade's first-pass rule for a ray that carries no stream word yet: keyed on (seed, index_base + index in
  unsigned long long index_base; // the round's list) -- the same key the rounds' k_shade uses for this list
  int skip_known;               // shuffleRays' known-miss shortcut (gvt_device.h)
  unsigned *const *count_ptr;   // the count words of all queues and the mask of the traced ones: their clear() (ImageTracer.h:248) is done here --
  const unsigned char *clear_mask; // the rays come from the segment table (host-known sizes), nothing in this launch reads or appends to a traced queue
  int n_inst;
  // a launch enqueued AHEAD of the host's knowledge (domain.hip, the speculative part of a Domain tick): the ray count comes from device memory (k_spec_begin
  // filled the segment table from the queues' count words and cleared them), and the whole launch is void unless *valid
  const unsigned *n_dev;
  const unsigned *valid;
};

// Everything a wave knows about ITS ray is the same in all 64 lanes, but it comes out of per-lane loads and vector arithmetic, so the compiler
// keeps it in vector registers -- ~75 of them live across the traversal loops (the ray, its shadow ray, the normal, the material), which
// is what pushed this kernel to 168 VGPRs + 448 bytes of scratch per lane (69 scratch loads / 68 stores in the ISA).  uni() moves such a
// value into a SCALAR register (v_readfirstlane): the state then lives in SGPRs -- spilled, where they run out, into the lanes of a
// VGPR (one VGPR holds 64 of them, v_writelane / v_readlane, no memory traffic) -- and the vector registers are left to the traversal.
__device__ __forceinline__ int uni(int x) { return __builtin_amdgcn_readfirstlane(x); }
__device__ __forceinline__ unsigned uni(unsigned x) { return (unsigned)__builtin_amdgcn_readfirstlane((int)x); }
__device__ __forceinline__ float uni(float x) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(x))); }
__device__ __forceinline__ V3 uni(V3 v) { return mk3(uni(v.x), uni(v.y), uni(v.z)); }
__device__ __forceinline__ void uni_ray(RayRec &r) {
  r.o = uni(r.o); r.t_min = uni(r.t_min); r.d = uni(r.d); r.t_max = uni(r.t_max); r.c = uni(r.c); r.t = uni(r.t);
  r.id = uni(r.id); r.depth = uni(r.depth); r.w = uni(r.w); r.type = uni(r.type); r.rng = uni(r.rng);
  r.km[0] = uni(r.km[0]); r.km[1] = uni(r.km[1]); r.km[2] = uni(r.km[2]);
}

// closest hit / any hit of ONE ray by a whole wave, from the root: the two layouts' instantiations of wave_run / wave_any_run (trace_wave.inc)
#define FIN_CAP 384           // lists of 640 entries: 10 KiB of LDS per wave, 16 waves per CU = 4 per SIMD (128 VGPRs, 50 spilled outside the traversal loops).  Round 6, against
#define FIN_PHYS (FIN_CAP + 256) // k_long_closest's 768 entries / 12 waves per CU: --domains 8 1.477 -> 1.458 ms (3 alternated pairs): a step waits for memory more than for issue
                              // slots (profiles/r06_finish_clusters.txt).  Lists of 256 entries (24 waves per CU, 84 VGPRs) were slower, 0.53 vs 0.47 ms on the 8-tile soup's 25 K hops
// (nodes4c != null, wave-uniform: the instance carries the cluster layout -- two levels per memory round trip, trace_wave.inc)
template <int CAP, int PHYS>
__device__ inline void wave_closest(const uint4 *__restrict__ nodes4, const uint4 *__restrict__ nodes4c, int root_entry, const float4 *__restrict__ tris, V3 O, V3 D, float tnear,
                                    const WaveLists &L, float &bt, int &bp, float &bu, float &bv, float &bden, unsigned *ovf_word) {
  bt = GVT_FLT_MAX; bu = 0.f; bv = 0.f; bden = 1.f; bp = -1;
  if (lane_id() == 0) { L.s_ref[0] = nodes4c ? root_entry : 0; L.s_tn[0] = 0.f; }
  __builtin_amdgcn_wave_barrier();
  if (nodes4c) wave_run<false, true, CAP, PHYS>(nodes4c, tris, O, D, slab_of(O, D), tnear, L, 1, 0, bt, bp, bu, bv, bden, ovf_word);
  else wave_run<false, false, CAP, PHYS>(nodes4, tris, O, D, slab_of(O, D), tnear, L, nodes4 ? 1 : 0, 0, bt, bp, bu, bv, bden, ovf_word);
  bt = uni(bt); bp = uni(bp); bu = uni(bu); bv = uni(bv); bden = uni(bden); // (the wave's reduction left the same values in every lane)
}
template <int CAP, int PHYS>
__device__ inline bool wave_any(const uint4 *__restrict__ nodes4, const uint4 *__restrict__ nodes4c, int root_entry, const float4 *__restrict__ tris, V3 O, V3 D, float tnear,
                                volatile int *s_ref, volatile int *l_ref, unsigned *ovf_word) {
  if (nodes4c) return wave_any_run<true, CAP, PHYS>(nodes4c, root_entry, tris, O, D, slab_of(O, D), tnear, s_ref, l_ref, ovf_word);
  return wave_any_run<false, CAP, PHYS>(nodes4, 0, tris, O, D, slab_of(O, D), tnear, s_ref, l_ref, ovf_word);
}

__global__ __launch_bounds__(256, 4) void k_finish(FinishArgs A) { // 4 waves per SIMD = the 16 waves per CU the LDS lists allow (unbounded: 230 VGPRs, 2 per SIMD; 3 per SIMD: 156)
  __shared__ int s_ref_all[4][FIN_PHYS];
  __shared__ float s_tn_all[4][FIN_PHYS];
  __shared__ int l_ref_all[4][FIN_PHYS];
  __shared__ float l_tn_all[4][FIN_PHYS];
  const int wv = threadIdx.x >> 6;
  const int lane = (int)lane_id();
  volatile int *s_ref = s_ref_all[wv];
  volatile float *s_tn = s_tn_all[wv];
  volatile int *l_ref = l_ref_all[wv];
  volatile float *l_tn = l_tn_all[wv];
  const WaveLists L = { s_ref, s_tn, l_ref, l_tn };
  if (A.valid && !*A.valid) return;
  const unsigned n_rays = A.n_dev ? *A.n_dev : A.n;
  if (blockIdx.x == 0 && A.count_ptr)
    for (int i = threadIdx.x; i < A.n_inst; i += 256)
      if (A.clear_mask[i]) *A.count_ptr[i] = 0u;
  bool first = true;
  unsigned n_closest = 0, n_any = 0; // wave-uniform
  // shuffleRays for one ray leaving instance `from` (TracerBase.h:392-400): 0 = the ray ended here (deposited if it is a SHADOW ray that
  // carries colour), 1 = it goes on in instance `next` of this rank (origin advanced), 2 = appended to another rank's queue
  auto move_on = [&](RayRec &r, int from, int &next) -> int {
    float ret_t;
    bool walked = false;
    float4 ra = make_float4(r.o.x, r.o.y, r.o.z, r.t_min);
    const float4 rb = make_float4(r.d.x, r.d.y, r.d.z, r.t_max);
    if (A.skip_known) {
      next = shuffle_walk(ra, rb, A.top, from, r.km, ret_t, walked);
      walked = uni((int)walked) != 0;
      if (walked) r.o = uni(mk3(ra.x, ra.y, ra.z));
      r.km[0] = uni(r.km[0]); r.km[1] = uni(r.km[1]); r.km[2] = uni(r.km[2]);
    } else next = top_nearest(ra, rb, A.top, from, ret_t);
    next = uni(next); ret_t = uni(ret_t);
    if (next < 0) {
      if (lane == 0) deposit_shadow(A.fb, A.n_pix, r.type, r.c, r.w, (unsigned)r.id);
      return 0;
    }
    if (!walked) r.o = uni(add3(r.o, scl3(r.d, ret_t * 0.95f))); // :393
    if (A.rank < 0 || A.owner[next] == A.rank) return 1;
    if (lane == 0) {
      const QueueDesc Q = A.queues[next];
      const unsigned slot = atomicAdd(Q.count, 1u);
      if (slot < Q.cap) store_ray(make_planes(Q.planes, Q.cap), slot, r);
      else atomicOr(A.queue_overflow, 1u);
    }
    return 2;
  };
  for (;;) {
    const unsigned g = wave_ticket(first, A.counter, wv);
    if (g >= n_rays) break;
    const WaveSeg sg = A.W.segs[wave_find_seg(A.W, g)];
    RayRec r = load_ray(make_planes(sg.planes, sg.cap), g - sg.begin);
    uni_ray(r);
    int inst = uni(sg.inst);
    bool fresh = true; // the ray as it came out of its queue: a stream word of 0 is keyed on its index (k_shade's first-pass rule)
    for (;;) { // the life of this ray on this rank
      const WaveInst *wi = A.W.insts + inst;
      float bt, bu, bv, bden;
      int bp;
      wave_closest<FIN_CAP, FIN_PHYS>(wi->nodes4, wi->nodes4c, wi->root_entry4c, wi->tris, xfm_point(wi->minv, r.o), xfm_vector(wi->minv, r.d), GVT_RAY_EPSILON, L, bt, bp, bu, bv, bden, A.trav_overflow);
      n_closest++;
      if (bp < 0) { // miss: forwarded as it is
        int next;
        if (move_on(r, inst, next) != 1) break;
        inst = next; fresh = true;
        continue;
      }
      if (r.type == 1) break; // a SHADOW ray that hits is dropped (:486-488)
      // ---- k_shade's block for one ray (every lane computes the same values)
      const float hu = bu / bden, hv = bv / bden;
      uint32_t g_seed = (fresh && r.rng == 0u) ? ray_stream_seed(A.seed, A.index_base + (uint64_t)g) : r.rng;
      fresh = false;
      const MeshView *M = &wi->mv;
      float t = bt;
      r.t = t; // :491
      const float4 *sl = M->slots + 4 * (size_t)M->slot_of[bp];
      const float4 q0 = sl[0], q1 = sl[1], q2 = sl[2], q3 = sl[3];
      const V3 v0 = mk3(q0.x, q0.y, q0.z), v1 = mk3(q1.w, q2.w, q3.x), v2 = mk3(q3.y, q3.z, q3.w);
      int ia = 0, ib = 0, ic = 0;
      if (A.normal_mode == GVT_HIP_NORMALS_SMOOTH || M->vcolors) { ia = M->tris[3 * bp]; ib = M->tris[3 * bp + 1]; ic = M->tris[3 * bp + 2]; }
      const V3 negNg = cross3(sub3(v1, v0), sub3(v2, v0));
      const V3 normalflat = norm3(mat3_mul(wi->normi, negNg)); // :504
      V3 N;
      if (A.normal_mode == GVT_HIP_NORMALS_SMOOTH) { // :505-518
        const V3 a = ld3(M->normals + 3 * ib), b = ld3(M->normals + 3 * ic), c = ld3(M->normals + 3 * ia);
        const V3 mn = add3(add3(scl3(a, hu), scl3(b, hv)), scl3(c, 1.0f - hu - hv));
        N = norm3(mat3_mul(wi->normi, mn));
      } else N = normalflat;
      if (dot3(neg3(r.d), normalflat) <= 0.f) N = neg3(N); // :527-529
      MatEval me = mat_eval(M->mat);
      if (M->vcolors) { // :534-569
        const V3 c0 = ld3(M->vcolors + 3 * ia), c1 = ld3(M->vcolors + 3 * ib), c2 = ld3(M->vcolors + 3 * ic);
        me.kd = add3(add3(scl3(c0, 1.f - hu - hv), scl3(c1, hu)), scl3(c2, hv));
        me.type = 0; me.ks = mk3(.5f, .5f, .5f); me.alpha = 1.f;
      } else if (M->face_mat && M->face_mat[bp] >= 0 && (unsigned)M->face_mat[bp] < M->n_mat) {
        me = mat_eval(M->materials[M->face_mat[bp]]);
      }
      if (r.type == 2) { // SECONDARY :572-575
        t = (t > 1) ? 1.f / t : t;
        r.w = r.w * t;
      }
      // what outlives the traversals below, as scalars
      N = uni(N); r.w = uni(r.w); r.t = uni(r.t); g_seed = uni(g_seed);
      me.type = uni(me.type); me.kd = uni(me.kd); me.ks = uni(me.ks); me.alpha = uni(me.alpha); me.eta = uni(me.eta); me.k = uni(me.k);
      me.roughness = uni(me.roughness); me.hsc = uni(me.hsc); me.back = uni(me.back); me.falloff = uni(me.falloff);
      for (int li = 0; li < A.n_lights; li++) { // generateShadowRays :320-358, traceShadowRays :364-385
        const gvt_hip_light L = A.lights[li];
        const V3 lightPos = (L.type == GVT_HIP_LIGHT_AREA) ? area_light_position(L, g_seed) : ld3(L.position);
        V3 c;
        if (!shade(me, r, N, L, lightPos, c)) continue;
        RayRec s;
        const float multiplier = 1.0f - GVT_RAY_EPSILON * 16;
        const float t_shadow = multiplier * r.t;
        const V3 origin = add3(r.o, scl3(r.d, t_shadow));
        const V3 dir = sub3(lightPos, origin);
        s.o = origin; s.t_min = GVT_RAY_EPSILON;
        s.d = norm3(dir);
        s.t_max = 3.0f;
        s.c = c; s.t = r.t;
        s.id = r.id; s.depth = r.depth; s.w = r.w; s.type = 1;
        s.rng = 0u;
        s.km[0] = 0u; s.km[1] = 0u; s.km[2] = 0u;
        uni_ray(s);
        g_seed = uni(g_seed);
        n_any++;
        if (wave_any<FIN_CAP, FIN_PHYS>(wi->nodes4, wi->nodes4c, wi->root_entry4c, wi->tris, xfm_point(wi->minv, s.o), xfm_vector(wi->minv, s.d), GVT_RAY_EPSILON, s_ref, l_ref, A.trav_overflow)) continue;
        int s_inst = inst; // un-occluded: through the instances ahead of it; it ends where it hits something, or in the framebuffer
        for (;;) {
          int next;
          if (move_on(s, s_inst, next) != 1) break;
          s_inst = next;
          const WaveInst *wj = A.W.insts + s_inst;
          // (the reference traces it like any ray of that instance's queue -- a closest-hit trace, counted as one -- and drops it if it hit: only WHETHER it hits
          //  matters, which the any-hit traversal answers over the same interval (tnear, FLT_MAX] with the same triangle test, in half the steps and stopping at the first)
          n_closest++;
          if (wave_any<FIN_CAP, FIN_PHYS>(wj->nodes4, wj->nodes4c, wj->root_entry4c, wj->tris, xfm_point(wj->minv, s.o), xfm_vector(wj->minv, s.d), GVT_RAY_EPSILON, s_ref, l_ref, A.trav_overflow)) break; // dropped
        }
      }
      // :584-602
      const int ndepth = r.depth - 1;
      const float p = 1.f - gvt_fastrand01(g_seed);
      if (!(ndepth > 0 && r.w > p)) break;
      r.type = 2;
      const float multiplier = 1.0f - 16.0f * GVT_FLT_EPSILON;
      const float t_secondary = multiplier * r.t;
      r.o = add3(r.o, scl3(r.d, t_secondary));
      const V3 nd = cos_weighted_dir(N, g_seed);
      r.d = nd;
      r.w = r.w * dot3(nd, N);
      r.depth = ndepth;
      r.rng = g_seed;
      r.km[0] = 0u; r.km[1] = 0u; r.km[2] = 0u; // a new straight segment
      uni_ray(r);
    }
    __builtin_amdgcn_wave_barrier(); // (convergent: the lanes meet again here -- move_on's lane-0 blocks -- not at the loop header's readfirstlane: wave_ticket)
  }
  if (lane == 0 && (n_closest || n_any)) { atomicAdd(A.tot + TOT_CLOSEST, (unsigned long long)n_closest); atomicAdd(A.tot + TOT_ANY, (unsigned long long)n_any); }
}
