// shade.inc -- Shade(), lights, the bounce direction and k_shade (EmbreeMeshAdapter.cpp:483-609) (included by trace.hip inside its anonymous namespace)
// ------------------------------------------------------------------------------------------------
// Shading (Material.cpp:50-139, Light.cpp:58-133), in the oracle's evaluation order
// ------------------------------------------------------------------------------------------------
__device__ inline V3 light_contribution(const gvt_hip_light &L, V3 hit, V3 samplePos) {
  V3 c = ld3(L.color);
  if (L.type == GVT_HIP_LIGHT_AMBIENT) return c; // Light.cpp:70
  V3 p = (L.type == GVT_HIP_LIGHT_AREA) ? samplePos : ld3(L.position);
  float distance = 1.f / len3(sub3(p, hit));
  distance = (distance > 1.f) ? 1.f : distance;
  return scl3(c, distance);
}

__device__ inline V3 area_light_position(const gvt_hip_light &L, uint32_t &seed) { // Light.cpp:72-99,115-127
  V3 v = ld3(L.normal), u, w;
  if (v.x == 0.f && v.y == 1.f && v.z == 0.f) {
    u = mk3(1, 0, 0); w = mk3(0, 0, 1);
  } else {
    const V3 up = mk3(0, 1, 0);
    u.x = up.y * v.z - v.y * up.z; u.y = up.z * v.x - v.z * up.x; u.z = up.x * v.y - v.x * up.y;
    w.x = v.y * u.z - u.y * v.z; w.y = v.z * u.x - u.z * v.x; w.z = v.x * u.y - u.x * v.y;
  }
  float xLocation = (float)(((double)gvt_fastrand_lcg(seed, 0, 1) - 0.5) * (double)L.width);
  float zLocation = (float)(((double)gvt_fastrand_lcg(seed, 0, 1) - 0.5) * (double)L.height);
  float xCoord = xLocation * u.x + zLocation * w.x;
  float yCoord = xLocation * u.y + zLocation * w.y;
  float zCoord = xLocation * u.z + zLocation * w.z;
  return mk3(L.position[0] + xCoord, L.position[1] + yCoord, L.position[2] + zCoord);
}

// primitives::Shade (Material.cpp:90-139)
// the material as Shade() sees it (per-face material, Mesh::mat, or the vertex-colour Lambert of EmbreeMeshAdapter.cpp:534-569)
struct MatEval {
  int type;
  V3 kd, ks;
  float alpha;
  V3 eta, k;
  float roughness;
  V3 hsc;
  float back, falloff;
};
__device__ inline MatEval mat_eval(const gvt_hip_material &m) {
  MatEval e;
  e.type = m.type; e.kd = ld3(m.kd); e.ks = ld3(m.ks); e.alpha = m.alpha; e.eta = ld3(m.eta); e.k = ld3(m.k); e.roughness = m.roughness;
  e.hsc = ld3(m.horizonScatteringColor); e.back = m.backScattering; e.falloff = m.horizonScatteringFallOff;
  return e;
}
__device__ inline float clamp01(float x) { const float a = (x < 0.f) ? 0.f : x; return (1.f < a) ? 1.f : a; } // embree clamp(x)

// LAMBERT: the material is known to be LAMBERT (type 0) when the kernel is compiled -- the other models' code and registers are not in it; same arithmetic
template <bool LAMBERT = false>
__device__ inline bool shade(const MatEval &m, const RayRec &ray, V3 N, const gvt_hip_light &L, V3 lightPos, V3 &out) {
  const int mtype = LAMBERT ? 0 : m.type;
  const V3 kd = m.kd, ks = m.ks;
  const float alpha = m.alpha;
  V3 hitPoint = add3(ray.o, scl3(ray.d, ray.t));
  V3 wi = norm3(sub3(lightPos, hitPoint));
  float dNw = dot3(N, wi);
  float NdotL = (0.f < dNw) ? dNw : 0.f;
  V3 Li = light_contribution(L, hitPoint, lightPos);
  if (NdotL == 0.f || (Li.x == 0.f && Li.y == 0.f && Li.z == 0.f)) return false;
  V3 color;
  if (mtype == 0) { // lambertShade :50-57
    color = scl3(kd, NdotL * ray.w);
  } else if (mtype == 1) { // phongShade :59-70
    V3 R = sub3(scl3(scl3(N, 2.f), NdotL), wi);
    float vr = dot3(R, neg3(ray.d));
    float VdotR = (0.f < vr) ? vr : 0.f;
    float power = VdotR * powf(VdotR, alpha);
    color = scl3(kd, NdotL * ray.w);
    color = add3(color, scl3(ks, power * ray.w));
  } else if (mtype == 2) { // blinnPhongShade :72-87
    V3 H = norm3(sub3(wi, ray.d));
    float hn = dot3(H, N);
    float NdotH = (0.f < hn) ? hn : 0.f;
    float power = NdotH * powf(NdotH, alpha);
    V3 diffuse = scl3(kd, NdotL * ray.w);
    V3 specular = scl3(ks, power * ray.w);
    color = add3(diffuse, specular);
  } else if (mtype >= 3 && mtype <= 5) {
    // EMBREE_MATERIAL_METAL / VELVET / MATTE: Material.cpp:106-122 -> Material__eval (adapter/embree/EmbreeMaterial.h:289-314), the
    // Embree tutorials' BRDFs; dg.Ns = N, wo = -ray.direction.  Embree's rcp/rsqrt (SSE estimate + Newton step) are 1/x, 1/sqrt(x)
    // here: parity with the reference is ~1e-6 relative for these types (checked against its own build through the oracle).
    const V3 wo = neg3(ray.d);
    const float one_over_pi = 0.31830988618379069122f;
    V3 r = mk3(0, 0, 0);
    if (mtype == 5) { // MatteMaterial__eval :168-172
      r = scl3(kd, clamp01(dot3(wi, N)));
    } else if (mtype == 4) { // VelvetMaterial__eval :246-253 = Minneart :188-192 + Velvety :222-228
      const float cosThetaI = clamp01(dot3(wi, N));
      const float backScatter = powf(clamp01(dot3(wo, wi)), m.back);
      const V3 a = scl3(ks, backScatter * cosThetaI * one_over_pi);
      const float cosThetaO = clamp01(dot3(wo, N));
      const float sinThetaO = sqrtf(1.0f - cosThetaO * cosThetaO);
      const float horizonScatter = powf(sinThetaO, m.falloff);
      const V3 b = scl3(m.hsc, horizonScatter * cosThetaI * one_over_pi);
      r = add3(a, b);
    } else { // MetalMaterial__eval :259-277; optics.h:75-83 fresnelConductor, :131-137 PowerCosineDistribution
      const float expo = 1.0f / m.roughness;
      const float cosThetaO = dot3(wo, N), cosThetaI = dot3(wi, N);
      if (!(cosThetaI <= 0.0f || cosThetaO <= 0.0f)) {
        const V3 s_ = add3(wi, wo);
        const V3 wh = scl3(s_, 1.0f / sqrtf(dot3(s_, s_)));
        const float cosThetaH = dot3(wh, N);
        const float cosTheta = dot3(wi, wh);
        const float cosi = cosTheta, c2 = cosi * cosi;
        const V3 tmp = add3(mul3(m.eta, m.eta), mul3(m.k, m.k));
        const V3 two_eta_c = scl3(scl3(m.eta, 2.0f), cosi);
        const V3 one = mk3(1.0f, 1.0f, 1.0f), vc2 = mk3(c2, c2, c2);
        const V3 num1 = add3(sub3(scl3(tmp, c2), two_eta_c), one), den1 = add3(add3(scl3(tmp, c2), two_eta_c), one);
        const V3 num2 = add3(sub3(tmp, two_eta_c), vc2), den2 = add3(add3(tmp, two_eta_c), vc2);
        const V3 Rpar = mk3(num1.x / den1.x, num1.y / den1.y, num1.z / den1.z);
        const V3 Rper = mk3(num2.x / den2.x, num2.y / den2.y, num2.z / den2.z);
        const V3 F = scl3(add3(Rpar, Rper), 0.5f);
        const float D = (expo + 2) * (1.0f / (2.0f * 3.14159265358979323846f)) * powf(fabsf(cosThetaH), expo);
        const float g1 = 2.0f * cosThetaH * cosThetaO / cosTheta, g2 = 2.0f * cosThetaH * cosThetaI / cosTheta;
        const float gm = (g1 < g2) ? g1 : g2;
        const float G = (1.0f < gm) ? 1.0f : gm;
        r = scl3(scl3(scl3(mul3(ks, F), D), G), 1.0f / (4.0f * cosThetaO));
      }
    }
    color = scl3(scl3(r, 2.f), ray.w); // 2.f * glm::vec3(r) * ray.w :120
  } else {
    color = mk3(0, 0, 0);
  }
  color = mul3(color, Li);
  float c[3] = { color.x, color.y, color.z };
  for (int i = 0; i < 3; i++) {
    float a = (c[i] < 0.f) ? 0.f : c[i];
    c[i] = (1.f < a) ? 1.f : a;
  }
  out = mk3(c[0], c[1], c[2]);
  return true;
}

// CosWeightedRandomHemisphereDirection2 (EmbreeMeshAdapter.cpp:289-318)
__device__ inline V3 cos_weighted_dir(V3 n, uint32_t &seed) {
  float Xi1 = gvt_fastrand01(seed);
  float Xi2 = gvt_fastrand01(seed);
  // acos / sinf / cosf: include/gvt_math.h, the definitions shared with the checker (no ocml call: bit-identical on both sides)
  float theta = (float)gvt_acos(__builtin_sqrt(1.0 - (double)Xi1));
  float phi = (float)(2.0 * 3.1415926535897932384626433832795 * (double)Xi2);
  float xs = gvt_sinf(theta) * gvt_cosf(phi);
  float ys = gvt_cosf(theta);
  float zs = gvt_sinf(theta) * gvt_sinf(phi);
  V3 y = n, h = y;
  if (fabsf(h.x) <= fabsf(h.y) && fabsf(h.x) <= fabsf(h.z)) h.x = 1.0f;
  else if (fabsf(h.y) <= fabsf(h.x) && fabsf(h.y) <= fabsf(h.z)) h.y = 1.0f;
  else h.z = 1.0f;
  V3 x = cross3(h, y);
  V3 z = cross3(x, y);
  V3 d = add3(add3(scl3(x, xs), scl3(y, ys)), scl3(z, zs));
  return norm3(d);
}

struct ShadeArgs {
  RayPlanes in;            // rayList (updated in place)
  const unsigned *idx;     // active list or null (identity)
  unsigned n;
  unsigned long long index_base;
  const gvt_hip_hit *hits;
  int first_pass;
  int carried_rng;         // 1: a ray's stream is the word it carries (plane 4); 0: first pass keyed on (seed, index in rayList)
  RayPlanes out; unsigned *out_count;       // moved_rays
  RayPlanes shadow; unsigned *shadow_count; // shadowRays of this pass
  unsigned *next_idx; unsigned *next_count; // rays that bounce (valid[pi] stays set)
  const gvt_hip_light *lights;
  Mat3 normi;
  int normal_mode, n_lights;
  uint32_t seed;
  unsigned *zero_word;     // reset for the launch that follows (the any-hit kernel's work counter)
  TermSink sink;           // terminal rule of the shuffle for rays that leave this instance without a hit (fb == nullptr: off)
  int update_in_place;     // 1: every shaded ray is written back (gvt_hip_trace: the caller reads rayList); 0: only rays that bounce
  const unsigned *n_dev;   // ray count of this pass in device memory (a pass launched without a host round trip); null: n
  // merged launch (k_shade<true>): rays are virtual indices into W's segments; per-ray mesh / normi from W.insts
  WaveSet W;
  const int *hop_inst;     // merged launch: per virtual ray index, the instance the ray went on into inside the closest-hit launch (-1 / null: its segment's; MultiSrc::hop_inst)
  int *out_from;           // source instance of every ray appended to `out`
  int *shadow_inst;        // instance of every ray appended to `shadow`
  unsigned shadow_stride;  // != 0: the shadow list is direct-mapped -- light li's ray of thread j at slot li * stride + j, in the order of the
                           // traced list (its tile coherence kept for the any-hit launch, no slot atomics); shadow_inst < 0 marks empty slots
  // single-mesh round, one light (knob shadow_order): the shadow list in SHADOW_CLASSES regions of cls_stride slots, by how long the primaries of the
  // wave's 64-ray tile took (steps[j]: the closest-hit launch's node steps of ray j; 255 = parked) -- the any-hit launch takes the highest class first,
  // so that its drain is left to the short rays (a shadow ray's step count follows its primary's: correlation 0.84 on the benchmark soup)
  const unsigned char *steps;
  unsigned *cls_cnt;       // SHADOW_CLASSES counters (null: off); shadow_count still receives the total
  unsigned cls_stride;
  int cls_lo, cls_shift;   // class = (steps - cls_lo) >> cls_shift, clamped
  int early_deposit;       // k_shade<false, LEAN> only (the host's conditions, trace.hip single_pass): one light, one camera ray per pixel, the framebuffer cleared by this
                           // frame -- store_shadow_early below instead of store_ray
};

// The early deposit of a frame in which every pixel has ONE writer: the any-hit launch would only decide WHETHER shadow ray s deposits c * w in its pixel (and for nearly every
// ray it does), so the value is stored now -- deposit_shadow's predicate, and `0.0f + x`, which is what its atomic makes of a cleared pixel, bit for bit (x = -0 included) --
// and k_trace<true, true, 2> stores zeros again where the ray turns out occluded.  The ray itself is THIN: origin and direction, which the traversal reads, and one word in
// the third plane's place -- the pixel, or ~0 where the predicate failed: such a ray is traced and counted like the others and touches no pixel.  (A 4-byte word and not the
// fourth plane as it was: a quarter of the bytes to write here, and the kernel behind reads one word per OCCLUDED ray and needs no n_pix, type or colour test of its own.)
__device__ __forceinline__ void store_shadow_early(const ShadeArgs &A, unsigned slot, const RayRec &s) {
  A.shadow.p0[slot] = make_float4(s.o.x, s.o.y, s.o.z, s.t_min);
  A.shadow.p1[slot] = make_float4(s.d.x, s.d.y, s.d.z, s.t_max);
  const bool dep = len3(s.c) > 0.f && (unsigned)s.id < A.sink.n_pix; // (s.type is 1)
  if (dep) {
    const V3 cw = scl3(s.c, s.w);
    ((float4 *)A.sink.fb)[(unsigned)s.id] = make_float4(0.0f + cw.x, 0.0f + cw.y, 0.0f + cw.z, 1.0f);
  }
  ((uint32_t *)A.shadow.p2)[slot] = dep ? (uint32_t)s.id : 0xffffffffu;
}

// class of a tile whose longest primary took `steps` node steps (4-wide nodes; the benchmark soup: mean 26, parked at 96)
__device__ __forceinline__ unsigned shadow_class(int steps, int lo, int shift) {
  const int c = (steps - lo) >> shift; // 24, 3: 24..31 -> 0, 32..39 -> 1, ... 80 and more (and parked rays) -> 7
  return (unsigned)(c < 0 ? 0 : (c > SHADOW_CLASSES - 1 ? SHADOW_CLASSES - 1 : c));
}

#define SHADE_BLOCK 512
// LEAN (the host's conditions, trace.hip): the frame is the simple case -- depth 1 (no ray can bounce), point / ambient lights, LAMBERT mesh materials without
// vertex colours or per-face materials; on a single-mesh chain also ONE instance in the scene and the terminal sink on (a missing ray is then simply dropped).  The general kernel carries the
// other material models, area lights, the bounce with its random numbers and the top-level walk of a missing ray through 128 VGPRs and 18 spilled ones;
// this instantiation compiles them out.  Same arithmetic on what is left: same bits.
template <bool MULTI, bool LEAN = false>
__global__ __launch_bounds__(SHADE_BLOCK, 4) void k_shade(ShadeArgs A, MeshView M1) { // 128 VGPRs: 4 waves per SIMD (unbounded: 134-148, 3)
  // one LDS (count, base) pair per output list use: moved_rays, next list, one per light
  __shared__ unsigned sh_alloc[2 * (2 + 64)];
  __shared__ unsigned sh_cls[2 * SHADOW_CLASSES]; // per class: rays of this block, then the block's first slot in the class's region
  for (int k = threadIdx.x; k < 2 * (2 + 64); k += SHADE_BLOCK) sh_alloc[k] = 0u;
  if (threadIdx.x < 2 * SHADOW_CLASSES) sh_cls[threadIdx.x] = 0u;
  __syncthreads();
  const unsigned j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j == 0 && A.zero_word) *A.zero_word = 0u;
  const unsigned n = A.n_dev ? *A.n_dev : A.n;
  const bool in_range = j < n;
  __shared__ unsigned sh_wcls[SHADE_BLOCK / 64]; // the class of each wave's 64-ray tile (ShadeArgs::steps), parked in LDS until the slots are allocated:
  if (!MULTI && A.cls_cnt) {                     // no register is held across the shading code for it
    int st = in_range ? (int)A.steps[j] : 0;
    for (int o = 32; o >= 1; o >>= 1) st = max(st, __shfl_xor(st, o));
    if (lane_id() == 0) sh_wcls[threadIdx.x >> 6] = shadow_class(st, A.cls_lo, A.cls_shift);
  }
  unsigned i = in_range ? (A.idx ? A.idx[j] : j) : 0u; // index in rayList (MULTI: virtual index, then index in the ray's queue)
  const unsigned gi = i;
  RayPlanes in = A.in;
  const MeshView *M = &M1;
  Mat3 normi = A.normi;
  int inst = A.sink.from;
  if (MULTI && in_range) {
    const WaveSeg sg = A.W.segs[wave_find_seg(A.W, i)];
    in = make_planes(sg.planes, sg.cap);
    i -= sg.begin;
    inst = sg.inst;
    if (A.hop_inst) { const int h_ = A.hop_inst[gi]; if (h_ >= 0) inst = h_; }
    M = &A.W.insts[inst].mv;
    normi = A.W.insts[inst].normi;
  }
  RayRec r;
  gvt_hip_hit h;
  h.prim = -1; h.t = 0.f; h.u = 0.f; h.v = 0.f;
  bool miss = false, shaded = false, bounce = false;
  uint32_t g_seed = 0;
  V3 N = mk3(0, 0, 0);
  MatEval me = mat_eval(M->mat);
  if (in_range) {
    r = load_ray(in, i);
    h = A.hits[j];
    if (!LEAN) g_seed = (A.first_pass && (!A.carried_rng || r.rng == 0u)) ? ray_stream_seed(A.seed, A.index_base + gi) : r.rng;
    if (h.prim < 0) {
      miss = true; // :605-609
    } else if (r.type != 1) { // a SHADOW ray that hits is dropped :486-488
      shaded = true;
      float t = h.t;
      r.t = t; // :491
      // the triangle's vertices from the 64-byte slot the traversal has just intersected (one line, usually still in L2) instead of
      // three index words and three vertices gathered from the mesh's own arrays; the indices only where per-vertex attributes are used
      const float4 *sl = M->slots + 4 * (size_t)M->slot_of[h.prim];
      const float4 s0 = sl[0], s1 = sl[1], s2 = sl[2], s3 = sl[3];
      const V3 v0 = mk3(s0.x, s0.y, s0.z), v1 = mk3(s1.w, s2.w, s3.x), v2 = mk3(s3.y, s3.z, s3.w);
      int ia = 0, ib = 0, ic = 0;
      if (A.normal_mode == GVT_HIP_NORMALS_SMOOTH || (!LEAN && M->vcolors)) { ia = M->tris[3 * h.prim]; ib = M->tris[3 * h.prim + 1]; ic = M->tris[3 * h.prim + 2]; }
      const V3 negNg = cross3(sub3(v1, v0), sub3(v2, v0)); // -Ng of Embree (cf. OptixMeshAdapter.cu:280-287)
      const V3 normalflat = norm3(mat3_mul(normi, negNg)); // :504
      if (A.normal_mode == GVT_HIP_NORMALS_SMOOTH) { // :505-518
        const V3 a = ld3(M->normals + 3 * ib), b = ld3(M->normals + 3 * ic), c = ld3(M->normals + 3 * ia);
        const V3 mn = add3(add3(scl3(a, h.u), scl3(b, h.v)), scl3(c, 1.0f - h.u - h.v));
        N = norm3(mat3_mul(normi, mn));
      } else {
        N = normalflat; // :520-522
      }
      if (dot3(neg3(r.d), normalflat) <= 0.f) N = neg3(N); // :527-529
      // material pick :534-569
      if (LEAN) {
      } else if (M->vcolors) {
        const V3 c0 = ld3(M->vcolors + 3 * ia), c1 = ld3(M->vcolors + 3 * ib), c2 = ld3(M->vcolors + 3 * ic);
        me.kd = add3(add3(scl3(c0, 1.f - h.u - h.v), scl3(c1, h.u)), scl3(c2, h.v));
        me.type = 0; me.ks = mk3(.5f, .5f, .5f); me.alpha = 1.f;
      } else if (M->face_mat && M->face_mat[h.prim] >= 0 && (unsigned)M->face_mat[h.prim] < M->n_mat) {
        me = mat_eval(M->materials[M->face_mat[h.prim]]);
      }
      if (r.type == 2) { // SECONDARY :572-575
        t = (t > 1) ? 1.f / t : t;
        r.w = r.w * t;
      }
    }
  }
  // moved_rays: misses are forwarded as they are -- unless the sink is on and no other instance lies ahead: then shuffleRays would
  // only drop the ray (or, for a SHADOW ray that carries colour, deposit it: TracerBase.h:396-400), which is done here at once
  if (!(LEAN && !MULTI)) { // (LEAN on a single-mesh chain: nothing lies ahead of a ray that leaves the scene's only instance, and a camera ray carries no colour to deposit: dropped)
    bool forward = miss;
    if (miss && A.sink.fb) {
      float ret_t;
      const float4 a = make_float4(r.o.x, r.o.y, r.o.z, r.t_min), b = make_float4(r.d.x, r.d.y, r.d.z, r.t_max);
      if (top_nearest(a, b, A.sink.top, inst, ret_t) < 0) {
        forward = false;
        deposit_shadow(A.sink.fb, A.sink.n_pix, r.type, r.c, r.w, (unsigned)r.id);
      }
    }
    const unsigned slot = block_alloc(A.out_count, forward, &sh_alloc[0]);
    if (forward) { store_ray(A.out, slot, r); if (MULTI) A.out_from[slot] = inst; }
  }
  // generateShadowRays :320-358 -- one pass per light so that the wave allocates slots together
  for (int li = 0; li < A.n_lights; li++) {
    bool emit = false;
    RayRec s;
    if (shaded) {
      const gvt_hip_light L = A.lights[li];
      const V3 lightPos = (!LEAN && L.type == GVT_HIP_LIGHT_AREA) ? area_light_position(L, g_seed) : ld3(L.position);
      V3 c;
      if (shade<LEAN>(me, r, N, L, lightPos, c)) {
        emit = true;
        const float multiplier = 1.0f - GVT_RAY_EPSILON * 16;
        const float t_shadow = multiplier * r.t;
        const V3 origin = add3(r.o, scl3(r.d, t_shadow));
        const V3 dir = sub3(lightPos, origin);
        s.o = origin; s.t_min = GVT_RAY_EPSILON;
        s.d = norm3(dir); // Ray ctor normalizes, Ray.h:109
        s.t_max = 3.0f;   // dir.length() == glm component count (:347,355)
        s.c = c; s.t = r.t;
        s.id = r.id; s.depth = r.depth; s.w = r.w; s.type = 1;
        s.rng = 0u;
        s.km[0] = 0u; s.km[1] = 0u; s.km[2] = 0u;
      }
    }
    if (A.shadow_stride) {
      if (j < A.shadow_stride) {
        const unsigned slot = (unsigned)li * A.shadow_stride + j;
        A.shadow_inst[slot] = emit ? (MULTI ? inst : 0) : -1;
        if (emit) store_ray(A.shadow, slot, s);
      }
    } else if (!MULTI && A.cls_cnt) { // (one light: the host's condition)
      const unsigned cls = (unsigned)__builtin_amdgcn_readfirstlane((int)sh_wcls[threadIdx.x >> 6]);
      const unsigned long long mask = ballot64(emit);
      unsigned woff = 0;
      if (mask) {
        if ((int)lane_id() == __ffsll((long long)mask) - 1) woff = atomicAdd(&sh_cls[cls], (unsigned)__popcll(mask));
        woff = (unsigned)__builtin_amdgcn_readlane((int)woff, __ffsll((long long)mask) - 1);
      }
      __syncthreads();
      // (the list's length is the sum of the class counts: the any-hit launch adds them up and leaves the total in *shadow_count for what reads it later)
      if (threadIdx.x < SHADOW_CLASSES && sh_cls[threadIdx.x]) sh_cls[SHADOW_CLASSES + threadIdx.x] = atomicAdd(&A.cls_cnt[threadIdx.x], sh_cls[threadIdx.x]);
      __syncthreads();
      if (emit) {
        const unsigned slot = cls * A.cls_stride + sh_cls[SHADOW_CLASSES + cls] + woff + lanes_below(mask);
        if (LEAN && A.early_deposit) store_shadow_early(A, slot, s);
        else store_ray(A.shadow, slot, s);
      }
    } else {
      const unsigned slot = block_alloc(A.shadow_count, emit, &sh_alloc[2 * (2 + li)]);
      if (emit) {
        if (LEAN && !MULTI && A.early_deposit) store_shadow_early(A, slot, s);
        else store_ray(A.shadow, slot, s);
        if (MULTI) A.shadow_inst[slot] = inst;
      }
    }
  }
  if (!LEAN && shaded) { // :584-602
    const int ndepth = r.depth - 1;
    const float p = 1.f - gvt_fastrand01(g_seed);
    if (ndepth > 0 && r.w > p) {
      r.type = 2;
      const float multiplier = 1.0f - 16.0f * GVT_FLT_EPSILON;
      const float t_secondary = multiplier * r.t;
      r.o = add3(r.o, scl3(r.d, t_secondary));
      const V3 nd = cos_weighted_dir(N, g_seed);
      r.d = nd;
      r.w = r.w * dot3(nd, N);
      r.depth = ndepth;
      r.km[0] = 0u; r.km[1] = 0u; r.km[2] = 0u; // a new straight segment: nothing is known about it
      bounce = true;
    }
    if (bounce || A.update_in_place) { // rayList is updated in place; a list the caller discards anyway (device queues) only needs it for the next pass
      r.rng = g_seed; // the stream goes on with the ray
      store_ray(in, i, r);
    }
  }
  if (!LEAN) {
    const unsigned slot = block_alloc(A.next_count, bounce, &sh_alloc[2]);
    if (bounce) A.next_idx[slot] = gi;
  }
}
