// trace_wave.inc -- the wave-per-ray traversal: wave_run (one loop: closest / any hit, flat / cluster nodes), k_long_closest (parked long rays), k_long_seed + k_wave_any (small rounds) (included by trace.hip inside its anonymous namespace)
// A whole wave per parked ray.  The pending nodes live in a per-wave LDS list; each step the 64 lanes open up to 64 of them (newest
// first), append the children the ray enters to the node list or the leaf list, and when enough leaves have gathered (or no node is
// left) every lane intersects one leaf and the wave reduces to the best (t, primID).  Entries farther than the best hit are dropped
// when they are taken.  LONG_CAP throttles the number of nodes opened per step so that the lists cannot outgrow LONG_PHYS.
#define LONG_CAP 512
#define LONG_PHYS (LONG_CAP + 256)

// The wave's pending lists: node entries and leaf references with their entry distances.  Any hit keeps no distances (s_tn, l_tn: null, never touched).
struct WaveLists { volatile int *s_ref; volatile float *s_tn; volatile int *l_ref; volatile float *l_tn; };

// The two rules every closest-hit phase below applies, each written once:
// an entry is still wanted while its distance lies within the best hit's t with its slack (closest hit only; any hit drops nothing)
__device__ __forceinline__ bool within_best(float etn, float bt) { return etn <= cull_bound(bt); }
// (t, p) replaces the best so far (bt, bp; bp < 0: none yet): nearer, or as near with the lower primID
__device__ __forceinline__ bool closer(float t, int p, float bt, int bp) { return bp < 0 || t < bt || (t == bt && p < bp); }

// ---- the CLUSTER layout (lbvh.hip build_nodes4c): two levels per memory round trip.
// A list entry is (slot of an even-level node << 4) | mask of its inner children.  A step takes up to 12 entries; five lanes serve one: role 0 fetches and tests the
// node itself, roles 1..4 fetch and test its inner children -- their slots follow from the entry alone, so all five fetches are issued together, BEFORE anyone knows
// which children the ray enters; role 0 then tells its group (one shuffle of a 4-bit verdict) and the roles whose child was not entered drop their results.
// What is appended: the entered grandchildren (inner: entries again; leaves) and the node's own entered leaf children.  Same boxes, same triangle test: same hits.
// The flat layout: an entry is a node's index, every lane serves one.
#define CL_GROUPS 12
template <bool CLUSTER>
struct WaveFan {
  static constexpr int OPEN = CLUSTER ? CL_GROUPS : 64; // entries one step can open
  static constexpr int NODES = CLUSTER ? 16 : 3;        // what one opened entry can add to the node list (it leaves the list itself) ...
  static constexpr int LEAVES = CLUSTER ? 20 : 4;       // ... and to the leaf list
};

// Node phase: the newest `take` entries are opened and the children the ray enters appended (closest hit: nearest last -- the lists are taken from their end).
template <bool ANY, bool CLUSTER>
__device__ __forceinline__ void wave_nodes(const uint4 *__restrict__ nodes, const RaySlab &S, const WaveLists &L, int take, int &ns, int &nl, float bt) {
  const int lane = (int)lane_id();
  const int g = CLUSTER ? lane / 5 : lane, role = CLUSTER ? lane - 5 * g : 0; // this lane serves entry g (cluster lanes 60..63: g = 12, never in a group)
  const bool mine = g < take;
  int ent = 0;
  float etn = 0.f;
  if (mine) { ent = L.s_ref[ns - 1 - g]; if constexpr (!ANY) etn = L.s_tn[ns - 1 - g]; }
  __builtin_amdgcn_wave_barrier();
  ns -= take;
  bool act = mine && (ANY || within_best(etn, bt));
  const uint4 *nd;
  if constexpr (CLUSTER) {
    const unsigned mask = (unsigned)ent & 15u;
    act = act && (role == 0 || ((mask >> (role - 1)) & 1u));
    const unsigned slot = ((unsigned)ent >> 4) + (role ? 1u + (unsigned)__popc(mask & ((1u << (role - 1)) - 1u)) : 0u);
    nd = nodes + (size_t)GVT_NODE4_F4 * slot;
  } else nd = nodes + (size_t)GVT_NODE4_F4 * ent;
  float tn[4];
  int rr[4];
  bool entered[4] = { false, false, false, false }; // any hit (closest hit reads it off the distances)
  auto in = [&](int c) { return ANY ? entered[c] : tn[c] < GVT_FLT_MAX; };
  unsigned verdict = 0u; // cluster, role 0: bit c = the ray enters child c (before the sort below forgets which child is which)
  if (act) {
    if constexpr (ANY) node4_test(nd, S, GVT_FLT_MAX, tn, rr, entered);
    else node4_test(nd, S, bt, tn, rr);
    if (CLUSTER && role == 0) verdict = (in(0) ? 1u : 0u) | (in(1) ? 2u : 0u) | (in(2) ? 4u : 0u) | (in(3) ? 8u : 0u);
    if constexpr (!ANY) sort4(tn, rr);
  }
  bool open = act;
  if constexpr (CLUSTER) {
    const unsigned pv = (unsigned)__shfl((int)verdict, 5 * g);
    open = act && (role == 0 || ((pv >> (role - 1)) & 1u));
  }
#pragma unroll
  for (int c = 3; c >= 0; c--) {
    const bool hit = open && in(c);
    const bool inner = hit && rr[c] >= 0 && !(CLUSTER && role == 0), leaf = hit && rr[c] < 0; // (cluster, role 0's inner children: their roles speak for them)
    const unsigned long long mi = ballot64(inner), ml = ballot64(leaf);
    if (inner) { const int pos = ns + (int)lanes_below(mi); L.s_ref[pos] = rr[c]; if constexpr (!ANY) L.s_tn[pos] = tn[c]; }
    if (leaf) { const int pos = nl + (int)lanes_below(ml); L.l_ref[pos] = rr[c]; if constexpr (!ANY) L.l_tn[pos] = tn[c]; }
    ns += __popcll(mi);
    nl += __popcll(ml);
  }
  __builtin_amdgcn_wave_barrier();
}

// Leaf phase: every lane intersects one of the newest 64 leaves.  Closest hit: the wave's best candidate, then against the ray's best so far.
// Any hit: a lane stops at its first hit; returns whether some lane found one.
template <bool ANY>
__device__ __forceinline__ bool wave_leaves(const float4 *__restrict__ tris, V3 O, V3 D, float tnear, const WaveLists &L, int &nl,
                                            float &bt, int &bp, float &bu, float &bv, float &bden) {
  const int lane = (int)lane_id();
  const int take = min(nl, 64);
  const bool mine = lane < take;
  int ref = -1;
  float etn = 0.f;
  if (mine) { ref = L.l_ref[nl - 1 - lane]; if constexpr (!ANY) etn = L.l_tn[nl - 1 - lane]; }
  __builtin_amdgcn_wave_barrier();
  nl -= take;
  float lt = GVT_FLT_MAX, lu = 0.f, lv = 0.f, ld = 1.f;
  int lp = -1;
  bool hit_any = false;
  if (mine && (ANY || within_best(etn, bt))) {
    const unsigned code = (unsigned)~ref;
    const unsigned first = code >> 3, ntri = code & 7u;
    const float4 *ts = tris + 4 * (size_t)first;
    for (unsigned k = 0; k < ntri && !hit_any; k++) {
      const float4 s0 = ts[4 * k], s1 = ts[4 * k + 1], s2 = ts[4 * k + 2];
      const V3 e1 = mk3(s1.x, s1.y, s1.z), e2 = mk3(s2.x, s2.y, s2.z);
      float TT, U, V, aden;
      if (tri_test_raw(O, D, mk3(s0.x, s0.y, s0.z), e1, e2, cross3(e1, e2), tnear, TT, U, V, aden)) {
        const float t = TT / aden;
        if (t <= GVT_FLT_MAX) {
          if constexpr (ANY) hit_any = true;
          else {
            const int prim = __float_as_int(s0.w);
            if (closer(t, prim, lt, lp)) { lt = t; lp = prim; lu = U; lv = V; ld = aden; }
          }
        }
      }
    }
  }
  if constexpr (ANY) return ballot64(hit_any) != 0ull;
  if (ballot64(lp >= 0)) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const float ot = __shfl_xor(lt, off), ou = __shfl_xor(lu, off), ov = __shfl_xor(lv, off), od = __shfl_xor(ld, off);
      const int op = __shfl_xor(lp, off);
      if (op >= 0 && closer(ot, op, lt, lp)) { lt = ot; lp = op; lu = ou; lv = ov; ld = od; }
    }
    if (lp >= 0 && closer(lt, lp, bt, bp)) { bt = lt; bp = lp; bu = lu; bv = lv; bden = ld; }
  }
  return false;
}

// The traversal of ONE ray by a whole wave (every lane holds the same O, D): shared by k_long_closest, k_wave_any and k_finish.
// The caller has put the pending nodes / leaves into the wave's LDS lists (ns / nl entries).  A node step opens up to WaveFan::OPEN entries;
// `take` is throttled so that the lists stay within CAP, and PHYS = CAP + 256 leaves room for the one step that may exceed it -- the bound
// is checked ONCE per step for the wave (a list that would outgrow PHYS: flag word set, the ray's traversal ends; reported, never silent),
// not per store.  Closest hit: the best hit so far comes in and goes out through (bt, bp, bu, bv, bden).  Any hit: true = occluded.
template <bool ANY, bool CLUSTER, int CAP, int PHYS>
__device__ __forceinline__ bool wave_run(const uint4 *__restrict__ nodes, const float4 *__restrict__ tris, V3 O, V3 D, const RaySlab &S, float tnear, const WaveLists &L,
                                          int ns, int nl, float &bt, int &bp, float &bu, float &bv, float &bden, unsigned *ovf_word) {
  using F = WaveFan<CLUSTER>;
  const int lane = (int)lane_id();
  bool occluded = false; // wave-uniform
  while (!occluded && (ns > 0 || nl > 0)) {
    const bool do_leaf = nl > 0 && (ns == 0 || nl >= 64 || nl > CAP - 256);
    if (!do_leaf) {
      int take = min(min(ns, F::OPEN), min((CAP - ns) / F::NODES, (CAP - nl) / F::LEAVES));
      take = max(take, 1);
      if (ns + F::NODES * take > PHYS || nl + F::LEAVES * take > PHYS) { if (lane == 0) atomicOr(ovf_word, 1u); break; }
      wave_nodes<ANY, CLUSTER>(nodes, S, L, take, ns, nl, bt);
    } else occluded = wave_leaves<ANY>(tris, O, D, tnear, L, nl, bt, bp, bu, bv, bden);
  }
  return occluded;
}
// any hit of one ray by a whole wave, from the root (flat: node 0 of a mesh that has nodes; cluster: root_entry): true = occluded
template <bool CLUSTER, int CAP, int PHYS>
__device__ __forceinline__ bool wave_any_run(const uint4 *__restrict__ nodes, int root_entry, const float4 *__restrict__ tris, V3 O, V3 D, const RaySlab &S, float tnear,
                                              volatile int *s_ref, volatile int *l_ref, unsigned *ovf_word) {
  if (lane_id() == 0) s_ref[0] = CLUSTER ? root_entry : 0;
  __builtin_amdgcn_wave_barrier();
  float bt = GVT_FLT_MAX, bu = 0.f, bv = 0.f, bden = 1.f; // (no best hit: unused)
  int bp = -1;
  return wave_run<true, CLUSTER, CAP, PHYS>(nodes, tris, O, D, S, tnear, WaveLists{ s_ref, nullptr, l_ref, nullptr }, (CLUSTER || nodes) ? 1 : 0, 0, bt, bp, bu, bv, bden, ovf_word);
}
__device__ __forceinline__ RaySlab slab_of(V3 O, V3 D) {
  const float dx = fabsf(D.x) < 1e-30f ? copysignf(1e-30f, D.x) : D.x;
  const float dy = fabsf(D.y) < 1e-30f ? copysignf(1e-30f, D.y) : D.y;
  const float dz = fabsf(D.z) < 1e-30f ? copysignf(1e-30f, D.z) : D.z;
  const float ix = 1.0f / dx, iy = 1.0f / dy, iz = 1.0f / dz;
  return make_slab(ix, iy, iz, O.x * ix, O.y * iy, O.z * iz);
}

// The number of the next ray of wave `wv` of a 256-thread block: the first one is the wave's own number, later ones come through the counter, behind those.
// The caller's loop must END in a statement every lane executes (a wave barrier, or a store made by all lanes).  A lane-0-only block as the LAST statement of a
// loop whose header takes the next ray with readfirstlane lets hipcc send lane 0 and the other 63 lanes round the loop separately (seen in an experiment that
// finished the parked rays inside k_trace: the 63 lanes then read a ticket no lane had taken and traced the same record for ever).
__device__ __forceinline__ unsigned wave_ticket(bool &first, unsigned *counter, int wv) {
  if (first) { first = false; return blockIdx.x * 4u + (unsigned)wv; }
  unsigned r = 0;
  if (lane_id() == 0) r = atomicAdd(counter, 1u);
  return (unsigned)__builtin_amdgcn_readfirstlane((int)r) + gridDim.x * 4u;
}

template <bool XFORM, bool MULTI = false>
__global__ __launch_bounds__(256) void k_long_closest(RayPlanes q, const LongRec *__restrict__ recs, const unsigned *__restrict__ n_recs, Mat4 minv,
                                                       Trav T, float tnear, gvt_hip_hit *__restrict__ hits, unsigned *counter, WaveSet W = WaveSet{},
                                                       const int *__restrict__ stk = nullptr, const int *__restrict__ hop_inst = nullptr) {
  __shared__ int s_ref_all[4][LONG_PHYS];
  __shared__ float s_tn_all[4][LONG_PHYS];
  __shared__ int l_ref_all[4][LONG_PHYS];
  __shared__ float l_tn_all[4][LONG_PHYS];
  const int wv = threadIdx.x >> 6;
  const int lane = (int)lane_id();
  volatile int *s_ref = s_ref_all[wv];
  volatile float *s_tn = s_tn_all[wv];
  volatile int *l_ref = l_ref_all[wv];
  volatile float *l_tn = l_tn_all[wv];
  const unsigned n = *n_recs;
  bool first = true;
  for (;;) {
    const unsigned r = wave_ticket(first, counter, wv);
    if (r >= n) break;
    const LongRec R = recs[r];
    float4 a, b;
    V3 O, D;
    if (MULTI) {
      const WaveSeg sg = W.segs[wave_find_seg(W, R.i)];
      const unsigned local = R.i - sg.begin;
      a = sg.planes[local]; b = sg.planes[sg.cap + local];
      int inst = sg.inst;
      if (hop_inst) { const int h_ = hop_inst[R.i]; if (h_ >= 0) inst = h_; } // the ray has gone on into another instance inside a launch of this chain (MultiSrc::hop_inst)
      const WaveInst *wi = W.insts + inst;
      T.nodes4 = wi->nodes4; T.tris = wi->tris;
      O = xfm_point(wi->minv, mk3(a.x, a.y, a.z)); D = xfm_vector(wi->minv, mk3(b.x, b.y, b.z));
    } else {
      a = q.p0[R.i]; b = q.p1[R.i];
      O = mk3(a.x, a.y, a.z); D = mk3(b.x, b.y, b.z);
      if (XFORM) { O = xfm_point(minv, O); D = xfm_vector(minv, D); }
    }
    const RaySlab S = slab_of(O, D);
    float bt = R.bt, bu = R.bu, bv = R.bv, bden = R.bden; // the same in every lane
    int bp = R.bp;
    int ns = T.nodes4 ? 1 : 0, nl = 0;                    // wave-uniform (an instance whose mesh has no nodes: the ray retires as a miss)
    if (stk && R.ns && T.nodes4) { // go on from the parked ray's pending stack (bottom first, so the nearest entries are taken first); entry distances unknown: 0
      const int e = lane < (int)R.ns ? stk[(size_t)r * LONG_SAVE + lane] : TRAV_DONE;
      const bool is_node = lane < (int)R.ns && e >= 0, is_leaf = lane < (int)R.ns && e < 0 && e != TRAV_DONE;
      const unsigned long long mi = ballot64(is_node), ml = ballot64(is_leaf);
      if (is_node) { s_ref[lanes_below(mi)] = e; s_tn[lanes_below(mi)] = 0.f; }
      if (is_leaf) { l_ref[lanes_below(ml)] = e; l_tn[lanes_below(ml)] = 0.f; }
      ns = __popcll(mi); nl = __popcll(ml);
    } else if (lane == 0) { s_ref[0] = 0; s_tn[0] = 0.f; }
    __builtin_amdgcn_wave_barrier();
    wave_run<false, false, LONG_CAP, LONG_PHYS>(T.nodes4, T.tris, O, D, S, tnear, WaveLists{ s_ref, s_tn, l_ref, l_tn }, ns, nl, bt, bp, bu, bv, bden, counter + (CW_TRAV_OVF - CW_LONG_WORK));
    // every lane stores the (same) result: no lane-0-only block at the end of this loop (wave_ticket)
    { gvt_hip_hit h; h.t = bt; h.prim = bp; h.u = (bp >= 0) ? bu / bden : 0.f; h.v = (bp >= 0) ? bv / bden : 0.f; hits[R.j] = h; }
  }
}

// Small launches.  A persistent one-lane-per-ray launch cannot be faster than its slowest ray's chain of dependent fetches
// (100-350 steps of ~1 us): a round that holds a few hundred rays -- every later round of a multi-domain frame -- cost ~150 us
// per traversal launch whatever its size.  Below `small_rays` the rounds therefore give EVERY ray a whole wave (the k_long_closest
// scheme: 64 pending nodes opened per step, ~15-25 steps per ray): k_long_seed turns the ray list into LongRecs, k_long_closest
// finds the closest hits, k_wave_any below is the same traversal for shadow rays (stops at the first occluder).
__global__ __launch_bounds__(256) void k_long_seed(LongRec *__restrict__ recs, unsigned *__restrict__ count, const unsigned *__restrict__ idx, unsigned n,
                                                    const unsigned *__restrict__ n_dev) {
  if (n_dev) n = *n_dev;
  const unsigned j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j == 0) *count = n;
  if (j >= n) return;
  LongRec R; R.j = j; R.i = idx ? idx[j] : j; R.bt = GVT_FLT_MAX; R.bp = -1; R.bu = 0.f; R.bv = 0.f; R.bden = 1.f; R.ns = 0u;
  recs[j] = R;
}

template <bool MULTI>
__global__ __launch_bounds__(256) void k_wave_any(RayPlanes q, const unsigned *__restrict__ n_dev, Mat4 minv, Trav T, float tnear, RayPlanes out,
                                                   unsigned *out_count, unsigned *counter, TermSink sink, MultiSrc MS) {
  __shared__ int s_ref_all[4][LONG_PHYS];
  __shared__ int l_ref_all[4][LONG_PHYS];
  const int wv = threadIdx.x >> 6;
  const int lane = (int)lane_id();
  volatile int *s_ref = s_ref_all[wv];
  volatile int *l_ref = l_ref_all[wv];
  const unsigned n = *n_dev;
  bool first = true;
  for (;;) {
    const unsigned r = wave_ticket(first, counter, wv);
    if (r >= n) break;
    const float4 a = q.p0[r], b = q.p1[r];
    int inst = sink.from;
    V3 O, D;
    if (MULTI) {
      inst = MS.ray_inst[r];
      const WaveInst *wi = MS.W.insts + inst;
      T.nodes4 = wi->nodes4; T.tris = wi->tris;
      O = xfm_point(wi->minv, mk3(a.x, a.y, a.z)); D = xfm_vector(wi->minv, mk3(b.x, b.y, b.z));
    } else {
      O = xfm_point(minv, mk3(a.x, a.y, a.z)); D = xfm_vector(minv, mk3(b.x, b.y, b.z));
    }
    const bool occluded = wave_any_run<false, LONG_CAP, LONG_PHYS>(T.nodes4, 0, T.tris, O, D, slab_of(O, D), tnear, s_ref, l_ref, counter + (CW_TRAV_OVF - CW_WORK));
    if (!occluded && lane == 0) { // un-occluded: moved on, or ended here by shuffleRays' terminal rule (TracerBase.h:396-400)
      const float4 c = q.p2[r], d = q.p3[r];
      bool go_on = true;
      if (sink.fb) {
        float ret_t;
        go_on = top_nearest(a, b, sink.top, inst, ret_t) >= 0;
        if (!go_on) deposit_shadow(sink.fb, sink.n_pix, __float_as_int(d.w), mk3(c.x, c.y, c.z), d.z, (unsigned)__float_as_int(d.x));
      }
      if (go_on) {
        const unsigned slot = atomicAdd(out_count, 1u);
        out.p0[slot] = a; out.p1[slot] = b; out.p2[slot] = c; out.p3[slot] = d;
        if (out.p4) out.p4[slot] = 0u;
        store_no_known(out, slot);
        if (MULTI && MS.out_from) MS.out_from[slot] = inst;
      }
    }
    __builtin_amdgcn_wave_barrier(); // (convergent: the lanes meet again here, not at the loop header's readfirstlane -- see wave_ticket)
  }
}
