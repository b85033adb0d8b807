// trace_lane.inc -- the lane-per-ray traversal: k_trace (persistent waves with lane refill, closest hit / any hit, single mesh or merged launch) (included by trace.hip inside its anonymous namespace)
// ------------------------------------------------------------------------------------------------
// Persistent-wave traversal with lane refill ("wavefront compaction of active rays").
//
// A 64-ray batch finishes when its slowest ray does (measured on the 10 M-triangle soup: mean 54 steps per
// ray, but 125 per batch -- 43 % of the lanes do useful work).  Here a wave keeps a private range of ray
// indices [c_next, c_end) taken CHUNK at a time from the device counter; whenever refill_min lanes have
// retired their ray (__ballot), the idle lanes are handed the next indices of that range (rank by mbcnt)
// and start a fresh ray with an empty stack while their neighbours continue.  Traversal is while-while:
// all lanes that still have an inner node descend together, then the lanes that reached a leaf intersect
// their triangles together.  Every wave exits once the counter has passed n and its lanes are empty.
// ------------------------------------------------------------------------------------------------
#ifndef GVT_TRI_NG_FROM_SLOT
#define GVT_TRI_NG_FROM_SLOT 1 // measured: reading 48 of the 64 slot bytes and rebuilding Ng is not faster (same cache line either way)
#endif
#ifndef GVT_STAMP
#define GVT_STAMP 0
#endif
#if GVT_STAMP
__device__ unsigned long long g_stamp[24];
#endif
// CW_TRAV_OVF of the launching context is set by k_trace / k_long_closest when a traversal stack would have exceeded LDS levels + spill entries
// (k_trace's `counter` is d_counters + CW_WORK, k_long_closest's d_counters + CW_LONG_WORK)
#ifndef TRAV_CHUNK
#define TRAV_CHUNK 256
#endif
#ifndef KT_SHARE_DELAY
#define KT_SHARE_DELAY 24 // drain-phase work sharing starts after this many iterations of a wave's drain
#endif
#define TRAV_DONE ((int)0x80000000) // ~code with count 7: never a valid leaf reference

// Long rays.  Per-ray cost is heavy-tailed (10 M soup, binary visits: mean 53, p99 130, p99.9 206, max 711) and one traversal step is
// a dependent memory access of ~1.5 us, so a handful of rays used to set the duration of a whole closest-hit launch (capping
// rays at 100 steps -- 0.1 % of them -- shortened it by 18 %).  k_trace therefore parks a ray that exceeds `steps` inner steps,
// with its best hit so far, in `recs`; k_long_closest then traverses each parked ray with a whole wave: 64 pending nodes per step
// instead of one.  The result is the same minimum over (t, primID) -- it does not depend on the order in which boxes are opened.
// LongRec.ns > 0: the record carries the ray's pending stack (LongQ.stk[slot * LONG_SAVE + k], bottom first) and k_long_closest goes
// on from there; 0: it starts again at the root with the best hit so far as its bound.
#define LONG_SAVE 48
#define LONG_STK_CAP 65536u // records that may carry a stack (12 MiB); later ones start again at the root
struct LongRec { unsigned j, i; float bt; int bp; float bu, bv, bden; unsigned ns; };
struct LongQ {
  LongRec *recs;
  unsigned *count;
  int *stk;          // null: no stacks are saved
  unsigned stk_cap;
  int steps; // 0: off
  int steps_drain; // ... once the wave's work counter is exhausted (no refills left to hide a long ray behind): the launch then ends
                   // ~1 us per remaining step of its longest ray, so the few long rays still in flight are parked earlier
  unsigned char *steps_out; // null, or one byte per ray of the list: the node steps the ray took (254 = that many or more, 255 = parked) -- what the
                            // shadow rays' launch is ordered by (shade.inc: their own step counts follow their primaries', correlation 0.84)
};

// One compressed 4-wide node against one ray: entry distances of the children the ray enters within [0, lim], GVT_FLT_MAX for the
// others (misses and unused slots, whose boxes are stored inverted), and their references.
//   plane t = (origin + q*scale - O) / d = q * (scale*inv_d) + (origin*inv_d - O*inv_d); scale is a power of two, so scale*inv_d is
//   exact.  The rounding of the two fused steps is covered by widening every slab by 2^-21 |O*inv_d| (about 5e-7 |O| in space, on
//   top of the padded boxes): RaySlab keeps O*inv_d moved out by that margin for the near planes (.x) and in for the far planes (.y).
// CDNA packed FP32: the four children are decoded two at a time (v_pk_fma_f32: 12 instead of 24 fused multiply-adds per node).
typedef float f2 __attribute__((ext_vector_type(2)));
struct RaySlab {
  float ix, iy, iz; // 1 / direction
  f2 ox, oy, oz;    // (O*inv_d + e, O*inv_d - e), e = 2^-21 |O*inv_d|
};
__device__ __forceinline__ RaySlab make_slab(float ix, float iy, float iz, float ox, float oy, float oz) {
  RaySlab S;
  S.ix = ix; S.iy = iy; S.iz = iz;
  const float ex = fabsf(ox) * 4.76837158e-7f, ey = fabsf(oy) * 4.76837158e-7f, ez = fabsf(oz) * 4.76837158e-7f;
  S.ox = (f2){ ox + ex, ox - ex }; S.oy = (f2){ oy + ey, oy - ey }; S.oz = (f2){ oz + ez, oz - ez };
  return S;
}
__device__ __forceinline__ f2 splat2(float v) { return (f2){ v, v }; }
// hit[k] (optional): child k is entered -- the same predicate as tn[k] < GVT_FLT_MAX, for callers that need no distances (any hit: saves
// the select and the second compare per child)
// LIM false: the children are tested against the ray's own interval only (tn = entry distance where the ray passes through the box at all); the caller applies
// the best hit's limit to the sorted distances itself -- one compare per child it had to make anyway, instead of a v_min per child in here (closest hit)
template <bool LIM = true>
__device__ __forceinline__ void node4_test(const uint4 *__restrict__ nd, const RaySlab &S, float lim, float tn[4], int rr[4], bool *hit = nullptr) {
  if (LIM) lim = cull_bound(lim); // (the best hit's t with its slack, gvt_device.h; FLT_MAX stays "no limit")
  const uint4 w0 = nd[0], w1 = nd[1], w2 = nd[2], w3 = nd[3];
  const float sx = __uint_as_float(w0.w) * S.ix, sy = __uint_as_float(w3.z) * S.iy, sz = __uint_as_float(w3.w) * S.iz;
  const f2 bx = __builtin_elementwise_fma(splat2(__uint_as_float(w0.x)), splat2(S.ix), -S.ox); // (near offset, far offset)
  const f2 by = __builtin_elementwise_fma(splat2(__uint_as_float(w0.y)), splat2(S.iy), -S.oy);
  const f2 bz = __builtin_elementwise_fma(splat2(__uint_as_float(w0.z)), splat2(S.iz), -S.oz);
  const unsigned qnx = S.ix >= 0.f ? w1.x : w1.y, qfx = S.ix >= 0.f ? w1.y : w1.x; // near / far planes by ray direction
  const unsigned qny = S.iy >= 0.f ? w1.z : w1.w, qfy = S.iy >= 0.f ? w1.w : w1.z;
  const unsigned qnz = S.iz >= 0.f ? w2.x : w2.y, qfz = S.iz >= 0.f ? w2.y : w2.x;
  rr[0] = (int)w2.z; rr[1] = (int)w2.w; rr[2] = (int)w3.x; rr[3] = (int)w3.y;
#define GVT_Q2(Q, SH) ((f2){ (float)(((Q) >> (SH)) & 0xffu), (float)(((Q) >> ((SH) + 8)) & 0xffu) })
#define GVT_SLAB2(SH, A, B)                                                                                          \
  {                                                                                                                  \
    const f2 nx_ = __builtin_elementwise_fma(GVT_Q2(qnx, SH), splat2(sx), splat2(bx.x));                              \
    const f2 ny_ = __builtin_elementwise_fma(GVT_Q2(qny, SH), splat2(sy), splat2(by.x));                              \
    const f2 nz_ = __builtin_elementwise_fma(GVT_Q2(qnz, SH), splat2(sz), splat2(bz.x));                              \
    const f2 fx_ = __builtin_elementwise_fma(GVT_Q2(qfx, SH), splat2(sx), splat2(bx.y));                              \
    const f2 fy_ = __builtin_elementwise_fma(GVT_Q2(qfy, SH), splat2(sy), splat2(by.y));                              \
    const f2 fz_ = __builtin_elementwise_fma(GVT_Q2(qfz, SH), splat2(sz), splat2(bz.y));                              \
    const float na_ = fmaxf(fmaxf(nx_.x, ny_.x), fmaxf(nz_.x, 0.f)), nb_ = fmaxf(fmaxf(nx_.y, ny_.y), fmaxf(nz_.y, 0.f)); \
    const float fa_ = fminf(fminf(fx_.x, fy_.x), fz_.x) * 1.0000004f, fb_ = fminf(fminf(fx_.y, fy_.y), fz_.y) * 1.0000004f; \
    const bool ha_ = na_ <= (LIM ? fminf(fa_, lim) : fa_), hb_ = nb_ <= (LIM ? fminf(fb_, lim) : fb_);                \
    tn[A] = ha_ ? na_ : GVT_FLT_MAX; /* a miss sorts last */                                                         \
    tn[B] = hb_ ? nb_ : GVT_FLT_MAX;                                                                                 \
    if (hit) { hit[A] = ha_; hit[B] = hb_; }                                                                         \
  }
  GVT_SLAB2(0, 0, 1) GVT_SLAB2(16, 2, 3)
#undef GVT_SLAB2
#undef GVT_Q2
}

// tn / rr of the four children by ascending distance (a 5-compare network; equal distances keep their order, a miss -- GVT_FLT_MAX -- sorts last)
__device__ __forceinline__ void sort4(float (&tn)[4], int (&rr)[4]) {
  auto ce = [&](int a, int b) {
    const bool sw = tn[b] < tn[a];
    const float ta = sw ? tn[b] : tn[a], tb = sw ? tn[a] : tn[b];
    const int ra = sw ? rr[b] : rr[a], rb = sw ? rr[a] : rr[b];
    tn[a] = ta; tn[b] = tb; rr[a] = ra; rr[b] = rb;
  };
  ce(0, 1); ce(2, 3); ce(0, 2); ce(1, 3); ce(1, 2);
}

__device__ __forceinline__ int *kt_spill_ptr(int *spill_base, int k) {
  unsigned t = threadIdx.x;
  asm volatile("" : "+v"(t));
  return spill_base + ((size_t)(blockIdx.x * TRAV_BLOCK + t) * TRAV_SPILL + (size_t)k);
}

// merged launches: segment of virtual ray index g (segments sorted by `begin`, n_seg small)
__device__ inline int wave_find_seg(const WaveSet &W, unsigned g) {
  int lo = 0, hi = W.n_seg - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (W.segs[mid].begin <= g) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// copies the rays whose indices are parked in the wave's LDS list to consecutive slots of `out`; with a sink, rays that meet no
// other instance end here (shuffleRays' terminal rule) and only the others are copied
// ray_inst / out_from (merged launches): instance a shadow ray was generated in, per ray of q / per ray of out (shuffleRays' `from`)
__device__ inline void flush_pending(volatile unsigned *pend, int n_pend, const RayPlanes &q, const RayPlanes &out, unsigned *out_count, const TermSink &K,
                                     const int *__restrict__ ray_inst = nullptr, int *__restrict__ out_from = nullptr) {
  if (!K.fb) {
    unsigned base = 0;
    if (lane_id() == 0) base = atomicAdd(out_count, (unsigned)n_pend);
    base = (unsigned)__builtin_amdgcn_readfirstlane((int)base);
    for (int k = (int)lane_id(); k < n_pend; k += 64) {
      const unsigned src = pend[k];
      out.p0[base + k] = q.p0[src]; out.p1[base + k] = q.p1[src]; out.p2[base + k] = q.p2[src]; out.p3[base + k] = q.p3[src];
      if (out.p4) out.p4[base + k] = 0u; // shadow rays never draw: their stream word is 0
      store_no_known(out, base + k);     // ... and have crossed nothing yet
      if (out_from) out_from[base + k] = ray_inst[src];
    }
    return;
  }
  // a scene of ONE instance whose rays these are: there is nothing ahead of any of them -- no origin / direction fetch, no box test
  const bool alone = K.top.n_inst == 1 && !ray_inst && K.from >= 0;
  for (int k0 = 0; k0 < n_pend; k0 += 64) {
    const int k = k0 + (int)lane_id();
    bool go_on = false;
    float4 a, b, c, d;
    int from = K.from;
    if (k < n_pend) {
      const unsigned src = pend[k];
      c = q.p2[src]; d = q.p3[src];
      if (!alone) {
        a = q.p0[src]; b = q.p1[src];
        if (ray_inst) from = ray_inst[src];
        float ret_t;
        go_on = top_nearest(a, b, K.top, from, ret_t) >= 0;
      }
      if (!go_on) deposit_shadow(K.fb, K.n_pix, __float_as_int(d.w), mk3(c.x, c.y, c.z), d.z, (unsigned)__float_as_int(d.x));
    }
    const unsigned long long m = ballot64(go_on);
    if (m) {
      unsigned base = 0;
      if (lane_id() == 0) base = atomicAdd(out_count, (unsigned)__popcll(m));
      base = (unsigned)__builtin_amdgcn_readfirstlane((int)base);
      if (go_on) { const unsigned slot = base + lanes_below(m); out.p0[slot] = a; out.p1[slot] = b; out.p2[slot] = c; out.p3[slot] = d; if (out.p4) out.p4[slot] = 0u; store_no_known(out, slot); if (out_from) out_from[slot] = from; }
    }
  }
}

// k_trace's work distribution for the single-mesh launches (see there): the wave's next range [ub, ue) of the list, or ub > ue: nothing is left.  Wave-uniform.
//   row == XCD_STRIPES_OFF: front to back -- first the wave's static chunk, then `dyn` rays at a time from the one counter;
//   otherwise the stripes of xcd_stripes.h -- first the wave's static units in its home stripe, then units from that stripe's counter, then from the other stripes'.
// A function of its own and not inlined: its divisions and 64-bit products otherwise take part in the register allocation of the whole kernel, which the
// closest-hit instantiation, at its budget of 96, pays for with scratch spills.
// state: the wave's progress, 0 at first -- bits 0..3: it draws from stripe (home + that) & 7, 8 = every stripe is used up; bit 4: set after the first fetch;
// bits 5..: static units it has yet to take.  Returns (ub, ue, new state); the caller makes the three words scalar again (readfirstlane).
template <unsigned frac8> __device__ __noinline__ uint3 kt_fetch(unsigned *counter, unsigned n, unsigned row, unsigned state) {
  // chunk is a fraction of a wave's fair share (frac8 / 8), never less than one wave's width; dyn is 1/16 of the share, at least 64 (32: the counter word saturates)
  const unsigned wpb = (unsigned)(TRAV_BLOCK / 64), n_waves_total = gridDim.x * wpb, share_w = n / n_waves_total;
  const unsigned chunk = max(64u, ((share_w * frac8 / 8u) + 16u) & ~31u), dyn = max(64u, (share_w / 16u) & ~63u);
  unsigned ub = 1u, ue = 0u;
  if (row == XCD_STRIPES_OFF) { // KEEP IN STEP with the merged launches' copy of this order in k_trace's refill (chunk, dyn, first_chunk there): knob 0 promises their order
    unsigned base = 0, len = chunk;
    if (!(state & 16u)) base = (blockIdx.x * wpb + (threadIdx.x >> 6)) * chunk;
    else {
      if (lane_id() == 0) base = atomicAdd(counter, dyn);
      base = (unsigned)__builtin_amdgcn_readfirstlane((int)base) + n_waves_total * chunk;
      len = dyn;
    }
    if (base < n) { ub = base; ue = min(base + len, n); }
    return make_uint3(ub, ue, 16u);
  }
  const XcdStripeMap SM = xcd_stripe_map(n, dyn, row);
  const unsigned ks = max(1u, (chunk + dyn / 2u) / dyn), home = blockIdx.x & 7u; // the static part in units
  unsigned st_steal = state & 15u, st_left = (state & 16u) ? state >> 5 : ks;
  bool got = false;
  if (st_left) { // this wave's static units; one beyond the stripe's end: so are the rest
    const unsigned s = (blockIdx.x >> 3) * wpb + (threadIdx.x >> 6);
    got = xcd_stripe_unit(SM, home, s * ks + (ks - st_left), &ub, &ue);
    st_left = got ? st_left - 1u : 0u;
  }
  while (!got && st_steal < XCD_STRIPES) {
    const unsigned x = (home + st_steal) & 7u;
    unsigned t = 0;
    if (lane_id() == 0) t = atomicAdd(counter + cw_work_stripe(x), 1u);
    // (behind the static units of the stripe's own waves: those of the blocks x, x + 8, ... of this grid)
    t = (unsigned)__builtin_amdgcn_readfirstlane((int)t) + ((gridDim.x + 7u - x) >> 3) * wpb * ks;
    got = xcd_stripe_unit(SM, x, t, &ub, &ue);
    if (!got) st_steal++;
  }
  if (!got) { ub = 1u; ue = 0u; }
  return make_uint3(ub, ue, st_steal | 16u | (st_left << 5));
}

// MULTI (merged launch, gvt_internal.h): closest hit -- ray j is virtual index (idx ? idx[j] : j) of the segment table MS.W; any hit --
// ray j of q was generated in instance MS.ray_inst[j]; either way the lane takes transform and acceleration structure from
// MS.W.insts[instance].  out_from receives the source instance of every survivor appended to `out`.
// per-block LDS copies of the round's tables (<= KT_TAB segments and instances): a refill then costs one memory round trip -- the
// ray itself -- instead of a binary search over the segment table plus the segment's and the instance's rows, each a dependent load
#define KT_TAB 32
struct KtInst { Mat4 minv; const uint4 *nodes4; const float4 *tris; };
struct KtSeg { float4 *planes; unsigned long long cap; unsigned begin; int inst; };
struct MultiSrc {
  WaveSet W;
  int *ray_inst;                // any hit: instance per ray of q; < 0 = an empty slot of a direct-mapped shadow list (skipped).  A hop (below) writes the ray's new instance here
  int *out_from;
  unsigned long long *tot_any;  // any hit over a direct-mapped list: the rays actually traced are added here (one atomic per wave)
  // single-mesh any hit (MULTI false): the list lies in SHADOW_CLASSES regions of cls_stride slots each, cls_cnt[c] rays in region c (k_shade, shade.inc);
  // ray j of the launch counts through the regions from the highest class down
  const unsigned *cls_cnt;
  unsigned cls_stride;
  unsigned *cls_total;
  // HOPS (merged launches, round 6): a ray that leaves its instance without a hit and has another instance OF THIS RANK ahead of it goes on there inside the launch --
  // shuffleRays' rule (TracerBase.h:392-400) applied by the lane: the origin advanced by 95 % of the entry distance and written back to the ray's slot, the
  // traversal started again in the next instance -- instead of waiting in that instance's queue for the next round.  Same rays, same traces, same order per ray.
  int *hop_inst;               // closest hit: per virtual ray index, the instance the ray is in now (-1: its segment's); null: no hops
  int hop_read;                // ... and whether a refill has to look there (the chain's later passes: a bounce starts in the instance its parent was hit in)
  const int *hop_owner;        // instance -> rank (null: every instance is this rank's)
  int hop_rank;
  int hop_early;               // 1: only while the wave still has rays to fetch (a ray that goes on during the drain would stretch the launch's tail: it is left to the next round)
  unsigned long long *hop_tot; // the traces hops add (closest-hit traces, like the rounds they replace); any hit: non-null = hops on
};
template <bool ANY, bool XFORM, int MODE, bool MULTI = false>
__global__ __launch_bounds__(TRAV_BLOCK, (ANY ? KT_BLOCKS_ANY : KT_BLOCKS_CLOSEST)) void k_trace(RayPlanes q, const unsigned *__restrict__ idx, unsigned n, Mat4 minv, Trav T, float tnear,
                                                       gvt_hip_hit *__restrict__ hits, int *__restrict__ flags, RayPlanes out, unsigned *out_count,
                                                       unsigned *counter, int *spill_base, int refill_min, int inner_min, const unsigned *__restrict__ n_dev, int share, unsigned share_min, TermSink sink, LongQ LQ,
                                                       MultiSrc MS = MultiSrc{}, unsigned stripe_row = XCD_STRIPES_OFF) {
  // Work distribution, stripes off (stripe_row == XCD_STRIPES_OFF; the merged launches always): wave w first takes the static range [w*chunk, (w+1)*chunk) -- no atomic, see the refill below -- and after that
  // dynamic ranges of `dyn` rays from the counter.  chunk is a fraction of a wave's fair share (3/8 for closest-hit launches, whose
  // per-ray cost varies most, 5/8 for any-hit; measured at 1 M rays: 96/128/160 rays -> 0.542/0.549/0.579 ms closest, 0.400/0.400/0.384
  // any), never less than one wave's width; dyn is 1/16 of the share, at least 64 (32: the counter word saturates).
  // (refill_min / inner_min / share stay kernel arguments in the shipped library too, although only the experiments build can move them: as
  // compile-time constants they cost 1.5 % of the any-hit launch -- 0.3555 against 0.3500 ms, the register allocation changes)
  // Stripes on (single-mesh launches, knob xcd_stripes; stripe_row = the list's row length, 0: none known): the list is handed out in UNITS of `dyn` rays through
  // the mapping of xcd_stripes.h, a stripe and a work counter (cw_work_stripe) per XCD.  Blocks are dealt to the XCDs round-robin, so a wave's home stripe is
  // blockIdx.x & 7.  Its static first part, again without an atomic, are the units [s * ks, (s + 1) * ks) of that stripe -- s = its number among the stripe's waves,
  // ks = chunk in units --; the stripe's counter hands out the units behind those of all its waves.  A wave whose stripe is used up goes on to the next stripe's
  // counter, and so on round all eight (a grid of fewer than eight blocks reaches the stripes without waves of their own in this way): at most one atomic per
  // stripe it finds used up, never a wait.  All of it is scalar code in the refill path.
  const unsigned n_waves_total = gridDim.x * (unsigned)(TRAV_BLOCK / 64);
  // glm's mat4 * vec4(d, 0) keeps the terms m[12..14] * 0 (they matter for -0 / inf / NaN only; parity keeps them).  launch_trace computes them on the host and
  // hands them over in the matrix's unused bottom row (m[3], m[7], m[11]): scalar registers, not three vector registers held -- and spilled -- for the whole launch
  const float z12 = minv.m[3], z13 = minv.m[7], z14 = minv.m[11];
  if (n_dev) n = *n_dev; // ray count produced by the previous kernel on this stream (no host round trip)
  constexpr int N_CLS = (ANY && !MULTI) ? SHADOW_CLASSES : 0; // (the other instantiations carry one unused word)
  __shared__ unsigned s_cls[N_CLS + 1];
  const bool by_class = N_CLS > 0 && MS.cls_cnt != nullptr; // block-uniform
  if (by_class) {
    if (threadIdx.x == 0) {
      unsigned acc = 0;
      for (int k = 0; k < N_CLS; k++) { s_cls[k] = acc; acc += MS.cls_cnt[N_CLS - 1 - k]; }
      s_cls[N_CLS] = acc;
      if (blockIdx.x == 0 && MS.cls_total) *MS.cls_total = acc; // the list's length, where the kernels behind this launch look for it (the pass's shadow count)
    }
    __syncthreads();
    n = s_cls[N_CLS];
  }
  const unsigned share_w = n / n_waves_total;
  const unsigned chunk = max(64u, ((share_w * (ANY ? 5u : 3u) / 8u) + 16u) & ~31u);
  const unsigned dyn = max(64u, (share_w / 16u) & ~63u);
  __shared__ int stack[TRAV_STACK * TRAV_BLOCK];
  int *lds = &stack[threadIdx.x];
  // the lane's spill area (levels beyond the LDS part: rare).  Its address is built WHERE it is used, from a thread index the compiler cannot see through (an
  // empty asm): otherwise the pointer -- and the offsets the loop optimiser derives from it -- are hoisted out of the loops and held in vector registers for the
  // whole launch, which the closest-hit kernel, right at its 96-register budget for five waves per SIMD, paid for with scratch spills
  // (the merged kernels keep the plain pointer: there the compiler's allocation came out worse with the opaque form -- 9 spilled registers instead of 4)
  int *spill_m = spill_base + (size_t)(blockIdx.x * TRAV_BLOCK + threadIdx.x) * TRAV_SPILL;
#define KT_SPILL(K) (*(MULTI ? spill_m + (K) : kt_spill_ptr(spill_base, (K))))
  __shared__ KtInst s_inst[MULTI ? KT_TAB : 1];
  __shared__ KtSeg s_seg[(MULTI && !ANY) ? KT_TAB : 1];
  bool tab = false; // block-uniform
  if (MULTI) {
    tab = MS.W.n_inst > 0 && MS.W.n_inst <= KT_TAB && MS.W.n_seg <= KT_TAB;
    if (tab) {
      for (int t = (int)threadIdx.x; t < MS.W.n_inst; t += TRAV_BLOCK) { const WaveInst *wi = MS.W.insts + t; s_inst[t].minv = wi->minv; s_inst[t].nodes4 = wi->nodes4; s_inst[t].tris = wi->tris; }
      if (!ANY) // (strided from the far end of the block, so that with >= 64 threads other lanes than the instance rows' load these)
        for (int t = TRAV_BLOCK - 1 - (int)threadIdx.x; t < MS.W.n_seg; t += TRAV_BLOCK) { const WaveSeg sg = MS.W.segs[t]; KtSeg k; k.planes = sg.planes; k.cap = sg.cap; k.begin = sg.begin; k.inst = sg.inst; s_seg[t] = k; }
      __syncthreads();
    }
  }
#define KT_PUSH(REF)                                                                  \
  {                                                                                   \
    if (sp < TRAV_STACK) { lds[sp * TRAV_BLOCK] = (REF); sp++; }                      \
    else if (sp - TRAV_STACK < TRAV_SPILL) { KT_SPILL(sp - TRAV_STACK) = (REF); sp++; }  \
    else atomicOr(counter + (CW_TRAV_OVF - CW_WORK), 1u); /* reported, never silent */          \
  }
#define KT_POP()                                                                      \
  {                                                                                   \
    if (sp == sb) cur = TRAV_DONE;                                                    \
    else { sp--; if (sp < TRAV_STACK) cur = lds[sp * TRAV_BLOCK]; else cur = KT_SPILL(sp - TRAV_STACK); } \
  }
  __shared__ unsigned pend_all[(TRAV_BLOCK / 64) * 128];
  volatile unsigned *pend = &pend_all[(threadIdx.x >> 6) * 128];
  int n_pend = 0;                 // wave-uniform
  unsigned c_next = 0, c_end = 0; // wave-uniform
  bool exhausted = false;         // wave-uniform
  bool first_chunk = true;        // wave-uniform
  unsigned st_state = 0;          // wave-uniform, single-mesh launches: where the wave stands in its work distribution (kt_fetch)
  bool active = false;
  unsigned j = 0;
  V3 O = mk3(0, 0, 0), D = mk3(0, 0, 1);
  RaySlab S = make_slab(0.f, 0.f, 0.f, 0.f, 0.f, 0.f);
  float bt = GVT_FLT_MAX, bu = 0.f, bv = 0.f, bden = 1.f; // bu, bv: un-divided U, V of the best hit; bden its |den|
  int bp = -1, sp = 0, cur = TRAV_DONE;
  int sb = 0;           // bottom of this lane's stack window [sb, sp): entries below sb were given away to helper lanes
  bool sharing = false; // wave-uniform (any hit): some ray of this wave is being traversed by more than one lane
  int drain_iters = 0;  // wave-uniform: outer iterations since the wave's work range ran dry
  int nsteps = 0;       // closest hit: inner steps of this lane's ray; beyond LQ.steps the ray is parked for k_long_closest (nsteps = -1 from then on)
#define KT_PARKED (nsteps < 0)
  const uint4 *nodes4_l = T.nodes4; // MULTI: this lane's ray's instance
  const float4 *tris_l = T.tris;
  int inst_l = 0;
  unsigned gidx = 0;                // MULTI closest: virtual index of the lane's ray
  unsigned n_started = 0;           // MULTI any hit: rays this wave really traced (wave-uniform)
  unsigned n_hops = 0;              // MULTI: hops of this wave's rays (wave-uniform)
#if GVT_STAMP
  unsigned long long st_refill = 0, st_inner = 0, st_leaf = 0, st_retire = 0, n_inner_it = 0, n_outer_it = 0, t_mark = 0, t_begin = __builtin_amdgcn_s_memtime();
  unsigned long long t_exh = 0, it_exh = 0, out_exh = 0, act_exh = 0, n_inner_lanes = 0, n_leaf_lanes = 0;
#endif
  for (;;) {
    // ---- refill idle lanes from the wave's private index range
#if GVT_STAMP == 1
    { unsigned long long t_ = __builtin_amdgcn_s_memtime(); if (n_outer_it) st_retire += t_ - t_mark; t_mark = t_; }
#endif
    unsigned long long idle = ballot64(!active);
    int nidle = __popcll(idle);
    if (!exhausted && (nidle >= refill_min || nidle == 64)) {
      while (nidle > 0) {
        if (c_next == c_end) {
          // the first chunk of every wave is assigned statically (chunk number = wave number): 4096 waves hitting one counter word at
          // launch would queue for ~45 us (a single word sustains ~90 atomics/us); the dynamic chunks start behind those
          if constexpr (!MULTI) {
            const uint3 f = kt_fetch<ANY ? 5u : 3u>(counter, n, stripe_row, st_state);
            const unsigned ub = (unsigned)__builtin_amdgcn_readfirstlane((int)f.x), ue = (unsigned)__builtin_amdgcn_readfirstlane((int)f.y);
            st_state = (unsigned)__builtin_amdgcn_readfirstlane((int)f.z);
            if (ub > ue) {
              exhausted = true;
#if GVT_STAMP
              if (!t_exh) { t_exh = __builtin_amdgcn_s_memtime(); it_exh = n_inner_it; out_exh = n_outer_it; act_exh = 64 - nidle; }
#endif
              break;
            }
            c_next = ub; c_end = ue;
            if (ub == ue) continue; // an empty unit (a part shorter than the row's longest): the next one
          } else { // the merged launches: front to back, inline -- KEEP IN STEP with kt_fetch's XCD_STRIPES_OFF branch (routing them through kt_fetch changes the
                   // register allocation of the merged kernels, which this change leaves as they were)
          unsigned base = 0;
          unsigned this_chunk = chunk;
          if (first_chunk) {
            first_chunk = false;
            base = (blockIdx.x * (unsigned)(TRAV_BLOCK / 64) + (threadIdx.x >> 6)) * chunk;
          } else {
            if (lane_id() == 0) base = atomicAdd(counter, dyn);
            base = (unsigned)__builtin_amdgcn_readfirstlane((int)base) + n_waves_total * chunk;
            this_chunk = dyn;
          }
          if (base >= n) {
            exhausted = true;
#if GVT_STAMP
            if (!t_exh) { t_exh = __builtin_amdgcn_s_memtime(); it_exh = n_inner_it; out_exh = n_outer_it; act_exh = 64 - nidle; }
#endif
            break;
          }
          c_next = base;
          c_end = min(base + this_chunk, n);
          }
        }
        const unsigned take = min(c_end - c_next, (unsigned)nidle);
        const unsigned rank = lanes_below(idle);
        bool start = false;
        if (!active && rank < take) {
          j = c_next + rank;
          unsigned i = idx ? idx[j] : j;
          if (by_class) { // k = the regions that end at or before j
            int k = 0;
#pragma unroll
            for (int t = 1; t < N_CLS; t++) k += (j >= s_cls[t]) ? 1 : 0;
            i = (unsigned)(N_CLS - 1 - k) * MS.cls_stride + (j - s_cls[k]);
          }
          float4 a, b;
          start = true;
          if (MULTI) {
            if (ANY) {
              inst_l = MS.ray_inst[i];
              start = inst_l >= 0; // direct-mapped shadow list: a slot whose primary emitted nothing
              if (start) { a = q.p0[i]; b = q.p1[i]; }
            } else if (tab) {
              int lo = 0, hi = MS.W.n_seg - 1;
              while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (s_seg[mid].begin <= i) lo = mid; else hi = mid - 1; }
              const unsigned local = i - s_seg[lo].begin;
              const float4 *pl = s_seg[lo].planes;
              a = pl[local]; b = pl[s_seg[lo].cap + local];
              inst_l = s_seg[lo].inst; gidx = i;
              if (MS.hop_read) { const int h_ = MS.hop_inst[i]; if (h_ >= 0) inst_l = h_; }
            } else {
              const WaveSeg sg = MS.W.segs[wave_find_seg(MS.W, i)];
              const unsigned local = i - sg.begin;
              a = sg.planes[local]; b = sg.planes[sg.cap + local];
              inst_l = sg.inst; gidx = i;
              if (MS.hop_read) { const int h_ = MS.hop_inst[i]; if (h_ >= 0) inst_l = h_; }
            }
            if (start && tab) {
              nodes4_l = s_inst[inst_l].nodes4; tris_l = s_inst[inst_l].tris;
              O = xfm_point(s_inst[inst_l].minv, mk3(a.x, a.y, a.z)); D = xfm_vector(s_inst[inst_l].minv, mk3(b.x, b.y, b.z));
            } else if (start) {
              const WaveInst *wi = MS.W.insts + inst_l;
              nodes4_l = wi->nodes4; tris_l = wi->tris;
              O = xfm_point(wi->minv, mk3(a.x, a.y, a.z)); D = xfm_vector(wi->minv, mk3(b.x, b.y, b.z));
            }
          } else {
            a = q.p0[i]; b = q.p1[i];
            O = mk3(a.x, a.y, a.z); D = mk3(b.x, b.y, b.z);
            if (XFORM) { // xfm_point / xfm_vector (gvt_device.h) with the direction's `translation x 0` terms taken from scalar registers (z12..z14 above)
              const float *m = minv.m;
              O = xfm_point(minv, O);
              D = mk3((m[0] * D.x + m[4] * D.y) + (m[8] * D.z + z12), (m[1] * D.x + m[5] * D.y) + (m[9] * D.z + z13), (m[2] * D.x + m[6] * D.y) + (m[10] * D.z + z14));
            }
            if (ANY && MODE >= 1) j = i; // a survivor is copied out of q by its slot there (an index list or the class regions: not its number in the launch); MODE 2 reads an occluded ray's pixel there
          }
          if (start) {
            const float dx = fabsf(D.x) < 1e-30f ? copysignf(1e-30f, D.x) : D.x;
            const float dy = fabsf(D.y) < 1e-30f ? copysignf(1e-30f, D.y) : D.y;
            const float dz = fabsf(D.z) < 1e-30f ? copysignf(1e-30f, D.z) : D.z;
            const float ix = 1.0f / dx, iy = 1.0f / dy, iz = 1.0f / dz;
            S = make_slab(ix, iy, iz, O.x * ix, O.y * iy, O.z * iz);
            bt = GVT_FLT_MAX; bu = 0.f; bv = 0.f; bden = 1.f; bp = -1;
            sp = 0; sb = 0; nsteps = 0;
            cur = (MULTI ? nodes4_l : T.nodes4) != nullptr ? 0 : TRAV_DONE;
            active = true;
          }
        }
        if (MULTI && ANY) n_started += (unsigned)__popcll(ballot64(start));
        c_next += take;
        idle = ballot64(!active);
        nidle = __popcll(idle);
      }
    }
    if (nidle == 64) break; // nothing left in flight and nothing left to fetch
    // ---- drain phase of an any-hit launch: work sharing inside the wave.  Once the work counter is exhausted, a wave used to finish at
    //      the pace of its slowest ray (measured: up to 536 more inner steps at ~2.5 K cycles each while 63 lanes idle -- the fixed ~0.5 ms
    //      of every launch).  Now an idle lane takes the BOTTOM entry (the largest pending subtree) of a busy lane's stack together with a
    //      copy of its ray, and traverses that subtree as a helper; an occluder found by any lane of a ray ends them all when they retire.
    //      (Sharing for closest hit lost, EXPERIMENTS.md: the pending subtrees of a closest-hit ray are mostly pruned by its eventual hit.)
    const bool share_on = ANY && (share & 1) != 0;
    // ... but only once the wave has been draining for KT_SHARE_DELAY iterations: where shadow rays are short -- surface meshes: they leave or are
    // occluded within a few steps -- a wave's drain is over before then and never pays for the pairing (bun_zipper 0.557 -> 0.514 ms per
    // frame, bunny.conf 0.338 -> 0.291, the 8-bunny grid 0.502 -> 0.459 without sharing); in a dense soup the drain is a hundred steps long
    if (exhausted) drain_iters++;
    const bool share_now = share_on && exhausted && drain_iters > KT_SHARE_DELAY && n >= share_min;
    if (share_now && nidle > 0) { // small launches: the hand-off costs more than the tail it trims (15 K shadow rays: 83 -> 66 us)
      unsigned long long idle_m = idle;
      unsigned long long don_m = ballot64(active && cur != TRAV_DONE && (sp - sb) >= 2);
      const unsigned wave_tid0 = threadIdx.x & ~63u;
      for (int pairs = 0; idle_m && don_m && pairs < 16; pairs++) {
        const int h = __ffsll((long long)idle_m) - 1, d = __ffsll((long long)don_m) - 1;
        // the bottom entry = the largest pending subtree
        const int sbd = __shfl(sb, d);
        const unsigned gj = (unsigned)__shfl((int)j, d);
        const float gOx = __shfl(O.x, d), gOy = __shfl(O.y, d), gOz = __shfl(O.z, d);
        const float gDx = __shfl(D.x, d), gDy = __shfl(D.y, d), gDz = __shfl(D.z, d);
        RaySlab gS;
        gS.ix = __shfl(S.ix, d); gS.iy = __shfl(S.iy, d); gS.iz = __shfl(S.iz, d);
        gS.ox = (f2){ __shfl(S.ox.x, d), __shfl(S.ox.y, d) }; gS.oy = (f2){ __shfl(S.oy.x, d), __shfl(S.oy.y, d) }; gS.oz = (f2){ __shfl(S.oz.x, d), __shfl(S.oz.y, d) };
        const int gbp = __shfl(bp, d);
        const int ginst = __shfl(inst_l, d);
        if ((int)lane_id() == h) {
          if (MULTI) { inst_l = ginst; nodes4_l = MS.W.insts[ginst].nodes4; tris_l = MS.W.insts[ginst].tris; }
          const unsigned tid_d = wave_tid0 + (unsigned)d;
          cur = (sbd < TRAV_STACK) ? stack[sbd * TRAV_BLOCK + tid_d]
                                   : spill_base[((size_t)blockIdx.x * TRAV_BLOCK + tid_d) * TRAV_SPILL + (sbd - TRAV_STACK)];
          j = gj; O = mk3(gOx, gOy, gOz); D = mk3(gDx, gDy, gDz);
          S = gS; bp = gbp;
          sp = 0; sb = 0;
          active = true;
        }
        if ((int)lane_id() == d) sb++;
        idle_m &= idle_m - 1;
        don_m &= don_m - 1; // one entry per donor and round: spread the helpers over the busy lanes
        sharing = true;
#if GVT_STAMP
        if (lane_id() == 0) atomicAdd(&g_stamp[23], 1ull); // hand-offs: subtrees given to a helper lane
#endif
      }
    }
#if GVT_STAMP == 1
    { unsigned long long t_ = __builtin_amdgcn_s_memtime(); st_refill += t_ - t_mark; t_mark = t_; n_outer_it++; }
#endif
    // ---- inner nodes: the lanes holding one descend level by level in a tight loop; the loop is left as soon as
    //      fewer than inner_min lanes still descend (the others wait at a leaf, have finished, or are idle), so that
    //      both this loop and the dearer leaf phase below run at high lane utilisation.
    // (an idle lane's `cur` is TRAV_DONE -- every path that clears `active` leaves it there, a lane that never started was initialised so --: `cur >= 0`
    //  alone says "this lane is at an inner node"; the vote is then ONE v_cmp into a scalar pair instead of and + select + compare, round 6's census)
    unsigned long long im = ballot64(cur >= 0);
    // closest hit: the children are culled against the best hit AFTER the sort (one compare per child, instead of a v_min per child in the slab test and a compare
    // here); lim2 = the best t with its slack, kept below FLT_MAX so that a child the ray misses (tn = FLT_MAX) fails the same compare.  bt changes in the leaf phase only
    const float lim2 = fminf(cull_bound(bt), 3.40282326e38f);
    while (im) {
      const bool at_inner = cur >= 0;
      if (at_inner) { // one 64-byte fetch decides four children (8-bit boxes on the node's own grid)
        float tn[4];
        int rr[4];
        bool entered[4];
        // (node address from a 32-bit byte offset: one shift, and the load takes base + offset -- the builder refuses trees of 2^26 nodes or more)
        node4_test<ANY>((const uint4 *)((const char *)(MULTI ? nodes4_l : T.nodes4) + ((unsigned)cur << 6)), S, GVT_FLT_MAX, tn, rr, ANY ? entered : nullptr);
#define KT_ENTERED(K) (ANY ? entered[K] : (tn[K] <= lim2)) // (closest hit: tn / rr are sorted below, the flags are not)
        if (!ANY) sort4(tn, rr); // nearest first; for any-hit the order does not matter
        // push the hit children farthest first (closest hit: sorted), continue with the first hit one
        int nxt = TRAV_DONE;
        bool have = false;
        if (sp + 3 <= TRAV_STACK) { // room for three entries in the LDS part: no bounds checks, no spill path
#pragma unroll
          for (int c4 = 3; c4 >= 0; c4--) {
            if (KT_ENTERED(c4)) {
              if (have) { lds[sp * TRAV_BLOCK] = nxt; sp++; }
              nxt = rr[c4]; have = true;
            }
          }
        } else {
#pragma unroll
          for (int c4 = 3; c4 >= 0; c4--) {
            if (KT_ENTERED(c4)) {
              if (have) KT_PUSH(nxt)
              nxt = rr[c4]; have = true;
            }
          }
        }
        if (have) cur = nxt;
        else KT_POP()
#undef KT_ENTERED
      }
#if GVT_STAMP == 1
      n_inner_it++; n_inner_lanes += (unsigned long long)__popcll(ballot64(at_inner));
#endif
      if (!ANY && at_inner && LQ.steps && ++nsteps > (exhausted ? LQ.steps_drain : LQ.steps) && cur != TRAV_DONE) { KT_PUSH(cur) cur = TRAV_DONE; nsteps = -1; } // the pending stack, `cur` on top, goes into the record
      im = ballot64(cur >= 0);
      if (__popcll(im) < inner_min) break;
    }
#if GVT_STAMP == 1
    { unsigned long long t_ = __builtin_amdgcn_s_memtime(); st_inner += t_ - t_mark; t_mark = t_; }
#endif
    // ---- leaves: every lane waiting at one intersects its triangles (64-byte slots: v0|prim, e1, e2, Ng).
    //      Measured with s_memtime stamps: a leaf phase that fetches and tests one triangle after the other costs ~6 K
    //      cycles (four dependent round trips at the loaded memory latency), an inner step ~1.9 K.  So the triangles are
    //      fetched two per round trip (48 of the 64 slot bytes each; fetching all four at once needs > 128 VGPRs and costs
    //      a wave per SIMD).
    {
      const bool at_leaf = cur < 0 && cur != TRAV_DONE;
#if GVT_STAMP == 1
      n_leaf_lanes += (unsigned long long)__popcll(ballot64(at_leaf));
#endif
      if (at_leaf) {
        const unsigned code = (unsigned)~cur;
        const unsigned first = code >> 3, ntri = code & 7u;
        const float4 *ts = (MULTI ? tris_l : T.tris) + 4 * (size_t)first;
        bool occluded = false;
        for (unsigned kb = 0; kb < ntri && !(ANY && occluded); kb += 2) { // two triangles per round trip
          float4 s0[2], s1[2], s2[2];
#pragma unroll
          for (unsigned k = 0; k < 2; k++)
            if (kb + k < ntri) { s0[k] = ts[4 * (kb + k)]; s1[k] = ts[4 * (kb + k) + 1]; s2[k] = ts[4 * (kb + k) + 2]; }
#pragma unroll
          for (unsigned k = 0; k < 2; k++) {
            if (kb + k < ntri && !(ANY && occluded)) {
              const V3 e1 = mk3(s1[k].x, s1[k].y, s1[k].z), e2 = mk3(s2[k].x, s2[k].y, s2[k].z);
              float TT, U, V, aden;
              if (tri_test_raw(O, D, mk3(s0[k].x, s0[k].y, s0[k].z), e1, e2, cross3(e1, e2), tnear, TT, U, V, aden)) {
                const float t = TT / aden;
                if (t <= GVT_FLT_MAX) {
                  if (ANY) occluded = true;
                  else {
                    const int prim = __float_as_int(s0[k].w);
                    if (bp < 0 || t < bt || (t == bt && prim < bp)) { bt = t; bp = prim; bu = U; bv = V; bden = aden; }
                  }
                }
              }
            }
          }
        }
        if (ANY && occluded) bp = 0;
      }
      if (at_leaf) {
        if (ANY && bp == 0) cur = TRAV_DONE;
        else KT_POP()
      }
    }
#if GVT_STAMP == 1
    { unsigned long long t_ = __builtin_amdgcn_s_memtime(); st_leaf += t_ - t_mark; t_mark = t_; }
#endif
    // ---- retire finished rays.  Retirement is batched: a finished lane costs nothing while it waits, so the block below (result
    //      stores with their two divisions, the parked-ray and survivor lists) runs only when a refill is due, when nothing is left
    //      in flight, or -- while lanes of a drained wave share rays -- at once, because a finished helper's result ends its group
    {
      const int nfin_w = __popcll(ballot64(active && cur == TRAV_DONE)), nidle_w = __popcll(ballot64(!active));
      const bool retire_now = RETIRE_BATCH == 0 || share_now || nfin_w + nidle_w >= (exhausted ? 64 : refill_min);
      if (!retire_now) continue;
    }
    if (sharing) { // lanes of one ray (any hit): the last one to finish carries the merged result, the others fold theirs into a partner
      const unsigned long long FM = ballot64(active && cur == TRAV_DONE);
      unsigned long long fm = FM;
      while (fm) {
        const int f = __ffsll((long long)fm) - 1;
        const unsigned jf = (unsigned)__shfl((int)j, f);
        const unsigned long long G = ballot64(active && j == jf);
        const unsigned long long Gf = G & FM, A = G & ~FM;
        const int tgt = A ? __ffsll((long long)A) - 1 : __ffsll((long long)Gf) - 1;
        unsigned long long src = Gf & ~(1ull << tgt);
        bool merged_occluded = false;
        while (src) {
          const int sidx = __ffsll((long long)src) - 1;
          if (__shfl(bp, sidx) >= 0) merged_occluded = true;
          if ((int)lane_id() == sidx) active = false; // folded into tgt: retires without writing
          src &= src - 1;
        }
        if (merged_occluded && ((G >> lane_id()) & 1ull) && active) { bp = 0; cur = TRAV_DONE; } // one occluder ends the whole group
        fm &= ~Gf;
      }
    }
    if (MULTI && (ANY ? (MODE == 1 && MS.hop_tot != nullptr) : (MS.hop_inst != nullptr))) { // hops (MultiSrc): a ray without a hit here goes on in the next instance of this rank
      const bool cand = active && cur == TRAV_DONE && bp < 0 && (ANY || !KT_PARKED) && !(exhausted && MS.hop_early);
      if (ballot64(cand)) {
        bool hopped = false;
        if (cand) {
          float4 *slot0;
          float4 a, b;
          if (ANY) { slot0 = q.p0 + j; b = q.p1[j]; }
          else {
            const WaveSeg sg = MS.W.segs[wave_find_seg(MS.W, gidx)];
            const unsigned local = gidx - sg.begin;
            slot0 = sg.planes + local; b = sg.planes[sg.cap + local];
          }
          a = *slot0;
          float ret_t;
          const int next = top_nearest(a, b, sink.top, inst_l, ret_t);
          if (next >= 0 && (!MS.hop_owner || MS.hop_owner[next] == MS.hop_rank)) {
            const V3 o = add3(mk3(a.x, a.y, a.z), scl3(mk3(b.x, b.y, b.z), ret_t * 0.95f)); // TracerBase.h:393
            a.x = o.x; a.y = o.y; a.z = o.z;
            *slot0 = a; // the ray as the next round would have found it in that instance's queue
            if (ANY) MS.ray_inst[j] = next; else MS.hop_inst[gidx] = next;
            inst_l = next;
            const WaveInst *wi = MS.W.insts + next;
            nodes4_l = wi->nodes4; tris_l = wi->tris;
            O = xfm_point(wi->minv, o); D = xfm_vector(wi->minv, mk3(b.x, b.y, b.z));
            const float dx = fabsf(D.x) < 1e-30f ? copysignf(1e-30f, D.x) : D.x;
            const float dy = fabsf(D.y) < 1e-30f ? copysignf(1e-30f, D.y) : D.y;
            const float dz = fabsf(D.z) < 1e-30f ? copysignf(1e-30f, D.z) : D.z;
            const float ix = 1.0f / dx, iy = 1.0f / dy, iz = 1.0f / dz;
            S = make_slab(ix, iy, iz, O.x * ix, O.y * iy, O.z * iz);
            bt = GVT_FLT_MAX; bu = 0.f; bv = 0.f; bden = 1.f; bp = -1;
            sp = 0; sb = 0; nsteps = 0;
            cur = nodes4_l != nullptr ? 0 : TRAV_DONE; // (an instance without a tree: a miss at once -- the next retirement looks further)
            hopped = true;
          }
        }
        n_hops += (unsigned)__popcll(ballot64(hopped));
      }
    }
    const bool fin = active && cur == TRAV_DONE;
    if (ANY && MODE == 1) {
      // un-occluded shadow rays go to moved_rays.  Their indices are parked in a per-wave LDS list and flushed 64+
      // at a time: one atomic on the queue counter per flush instead of one per retirement (a single counter
      // word sustains only ~90 atomics/us chip-wide).
      const bool survive = fin && bp < 0;
      const unsigned long long sm = ballot64(survive);
      if (sm) {
        if (survive) pend[n_pend + lanes_below(sm)] = j;
        n_pend += __popcll(sm);
      }
      if (n_pend >= 64) { flush_pending(pend, n_pend, q, out, out_count, sink, MULTI ? MS.ray_inst : nullptr, MULTI ? MS.out_from : nullptr); n_pend = 0; }
    }
    if (!ANY && LQ.steps) {
      const unsigned long long pm = ballot64(fin && KT_PARKED);
      if (pm) {
        unsigned base = 0;
        if ((int)lane_id() == __ffsll((long long)pm) - 1) base = atomicAdd(LQ.count, (unsigned)__popcll(pm));
        base = __shfl(base, __ffsll((long long)pm) - 1);
        if (fin && KT_PARKED) {
          const unsigned slot = base + lanes_below(pm);
          LongRec R; R.j = j; R.i = MULTI ? gidx : (idx ? idx[j] : j); R.bt = bt; R.bp = bp; R.bu = bu; R.bv = bv; R.bden = bden; R.ns = 0u;
          const int depth = sp - sb;
          if (LQ.stk && depth > 0 && depth <= LONG_SAVE && slot < LQ.stk_cap) {
            int *dst = LQ.stk + (size_t)slot * LONG_SAVE;
            for (int k = 0; k < depth; k++) dst[k] = (sb + k < TRAV_STACK) ? lds[(sb + k) * TRAV_BLOCK] : KT_SPILL(sb + k - TRAV_STACK);
            R.ns = (unsigned)depth;
          }
          LQ.recs[slot] = R;
        }
      }
    }
    if (ANY && MODE == 2) {
      // early deposits (k_shade, shade.inc): every ray's colour already lies in its pixel, stored there before this launch began -- one writer per pixel, the host's
      // condition.  A survivor has nothing left to do: no list, no flush, no atomics.  An occluded ray takes its deposit back: the pixel is what the frame's clear left.
      // Its word of the thin ray's third plane is the pixel, or ~0 where the shading kernel's predicate (deposit_shadow's own) failed and nothing was stored.
      // (lanes that shared a ray: the survivors of the merge above carry the group's occlusion; a second store of the same zeros would change nothing)
      if (fin && bp >= 0) {
        const unsigned px = ((const unsigned *)q.p2)[j];
        if (px != 0xffffffffu) ((float4 *)sink.fb)[px] = make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
    if (fin) {
      if (ANY) { if (MODE == 0) flags[j] = (bp >= 0) ? 1 : 0; }
      else {
        if (!KT_PARKED) { gvt_hip_hit h; h.t = bt; h.prim = bp; h.u = (bp >= 0) ? bu / bden : 0.f; h.v = (bp >= 0) ? bv / bden : 0.f; hits[j] = h; }
        if (LQ.steps_out) LQ.steps_out[j] = (unsigned char)(KT_PARKED ? 255 : min(nsteps, 254));
      }
      active = false;
    }
  }
#if GVT_STAMP
  if (lane_id() == 0) { atomicAdd(&g_stamp[0], st_refill); atomicAdd(&g_stamp[1], st_inner); atomicAdd(&g_stamp[2], st_leaf); atomicAdd(&g_stamp[3], st_retire); atomicAdd(&g_stamp[4], n_inner_it); atomicAdd(&g_stamp[5], n_outer_it); atomicAdd(&g_stamp[6], 1ull); atomicAdd(&g_stamp[7], (unsigned long long)__builtin_amdgcn_s_memtime() - t_begin); atomicAdd(&g_stamp[14], n_inner_lanes); atomicAdd(&g_stamp[15], n_leaf_lanes); atomicMax(&g_stamp[16], ~t_begin); atomicMax(&g_stamp[17], (unsigned long long)__builtin_amdgcn_s_memtime()); atomicMax(&g_stamp[18], t_exh); atomicAdd(&g_stamp[19], t_exh ? t_exh - t_begin : 0ull); atomicMax(&g_stamp[20], (unsigned long long)__builtin_amdgcn_s_memtime() - t_begin); atomicMax(&g_stamp[21], t_exh ? t_exh - t_begin : 0ull); atomicMax(&g_stamp[22], ~(t_exh ? t_exh - t_begin : ~0ull));
    if (t_exh) { atomicAdd(&g_stamp[8], (unsigned long long)__builtin_amdgcn_s_memtime() - t_exh); atomicAdd(&g_stamp[9], n_inner_it - it_exh); atomicAdd(&g_stamp[10], n_outer_it - out_exh); atomicAdd(&g_stamp[11], act_exh); atomicMax(&g_stamp[12], (unsigned long long)__builtin_amdgcn_s_memtime() - t_exh); atomicMax(&g_stamp[13], n_inner_it - it_exh); } }
#endif
  if (ANY && MODE == 1) { if (n_pend) flush_pending(pend, n_pend, q, out, out_count, sink, MULTI ? MS.ray_inst : nullptr, MULTI ? MS.out_from : nullptr); }
  if (MULTI && ANY && MS.tot_any && n_started && lane_id() == 0) atomicAdd(MS.tot_any, (unsigned long long)n_started);
  if (MULTI && MS.hop_tot && n_hops && lane_id() == 0) atomicAdd(MS.hop_tot, (unsigned long long)n_hops);
#undef KT_PUSH
#undef KT_POP
#undef KT_SPILL
#undef KT_PARKED
}
