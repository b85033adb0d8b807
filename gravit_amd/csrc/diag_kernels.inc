// diag_kernels.inc -- included by trace.hip inside its anonymous namespace.  NOT the hot path: the per-ray visit-count diagnostics
// (gvt_hip_visit_stats, gvt_hip_wide_visit_stats), one 64-ray batch per wave over the binary LBVH.
// closest-hit traversal of the binary nodes, counting: cnt[0] inner-node visits, cnt[1] leaf visits, cnt[2] triangle tests, cnt[3] visits of marked nodes
__device__ inline void traverse_count(const Trav &T, V3 O, V3 D, float tnear, int *__restrict__ lds /* &stack[0][tid] */, int *__restrict__ spill,
                                      float &best_t, int &best_prim, float &best_u, float &best_v, unsigned *cnt,
                                      const unsigned char *__restrict__ marks = nullptr) {
  // reciprocal direction for the slab test only (never feeds a result)
  float dx = fabsf(D.x) < 1e-30f ? copysignf(1e-30f, D.x) : D.x;
  float dy = fabsf(D.y) < 1e-30f ? copysignf(1e-30f, D.y) : D.y;
  float dz = fabsf(D.z) < 1e-30f ? copysignf(1e-30f, D.z) : D.z;
  const float ix = 1.0f / dx, iy = 1.0f / dy, iz = 1.0f / dz;
  const float ox = O.x * ix, oy = O.y * iy, oz = O.z * iz;
  int sp = 0;
  int cur = 0;
  for (;;) {
    if (cur >= 0) {
      cnt[0]++; if (marks && marks[cur]) cnt[3]++;
      const BvhNode *nd = T.nodes + cur;
      const float4 n0 = nd->n0, n1 = nd->n1, n2 = nd->n2, n3 = nd->n3;
      float a0 = __builtin_fmaf(n0.x, ix, -ox), a1 = __builtin_fmaf(n0.y, ix, -ox);
      float b0 = __builtin_fmaf(n0.z, iy, -oy), b1 = __builtin_fmaf(n0.w, iy, -oy);
      float c0 = __builtin_fmaf(n2.x, iz, -oz), c1 = __builtin_fmaf(n2.y, iz, -oz);
      float tn0 = fmaxf(fmaxf(fminf(a0, a1), fminf(b0, b1)), fmaxf(fminf(c0, c1), 0.f));
      float tf0 = fminf(fminf(fmaxf(a0, a1), fmaxf(b0, b1)), fmaxf(c0, c1)) * 1.0000004f;
      a0 = __builtin_fmaf(n1.x, ix, -ox); a1 = __builtin_fmaf(n1.y, ix, -ox);
      b0 = __builtin_fmaf(n1.z, iy, -oy); b1 = __builtin_fmaf(n1.w, iy, -oy);
      c0 = __builtin_fmaf(n2.z, iz, -oz); c1 = __builtin_fmaf(n2.w, iz, -oz);
      float tn1 = fmaxf(fmaxf(fminf(a0, a1), fminf(b0, b1)), fmaxf(fminf(c0, c1), 0.f));
      float tf1 = fminf(fminf(fmaxf(a0, a1), fmaxf(b0, b1)), fmaxf(c0, c1)) * 1.0000004f;
      const float lim = cull_bound(best_t);
      const bool h0 = (tn0 <= tf0) && (tn0 <= lim);
      const bool h1 = (tn1 <= tf1) && (tn1 <= lim);
      const int r0 = __float_as_int(n3.x), r1 = __float_as_int(n3.y);
      if (h0 && h1) {
        const bool swap = tn1 < tn0;
        const int nearc = swap ? r1 : r0, farc = swap ? r0 : r1;
        if (sp < TRAV_STACK) lds[sp * TRAV_BLOCK] = farc; else spill[sp - TRAV_STACK] = farc;
        sp++;
        cur = nearc;
      } else if (h0) {
        cur = r0;
      } else if (h1) {
        cur = r1;
      } else {
        if (sp == 0) break;
        sp--;
        cur = (sp < TRAV_STACK) ? lds[sp * TRAV_BLOCK] : spill[sp - TRAV_STACK];
      }
    } else {
      const unsigned code = (unsigned)~cur;
      const unsigned first = code >> 3, ntri = code & 7u;
      cnt[1]++; cnt[2] += ntri;
      for (unsigned k = 0; k < ntri; k++) {
        const float4 t0 = T.tris[4 * (first + k)], t1 = T.tris[4 * (first + k) + 1], t2 = T.tris[4 * (first + k) + 2];
        float t, u, v;
        if (tri_test(O, D, mk3(t0.x, t0.y, t0.z), mk3(t1.x, t1.y, t1.z), mk3(t2.x, t2.y, t2.z), tnear, t, u, v)) {
          const int prim = __float_as_int(t0.w);
          if (best_prim < 0 || t < best_t || (t == best_t && prim < best_prim)) { best_t = t; best_prim = prim; best_u = u; best_v = v; }
        }
      }
      if (sp == 0) break;
      sp--;
      cur = (sp < TRAV_STACK) ? lds[sp * TRAV_BLOCK] : spill[sp - TRAV_STACK];
    }
  }
}

// wave-level work fetch: 64 rays per grab; every wave leaves as soon as the counter passes n
__device__ inline unsigned fetch_batch(unsigned *counter) {
  unsigned base = 0;
  if (lane_id() == 0) base = atomicAdd(counter, 64u);
  return (unsigned)__builtin_amdgcn_readfirstlane((int)base);
}

// diagnostic: how many nodes would a W-wide collapse of the tree make this ray visit?  marks[k] = binary node k is the root of a
// W-wide node (lbvh.hip wide_root_marks: the very collapse rule of build_nodes4, run for width W); a wide node is visited exactly
// when the binary traversal visits its root.  out[j] = marked visits of ray j.
__global__ __launch_bounds__(TRAV_BLOCK) void k_wide_visit_stats(RayPlanes q, unsigned n, Trav T, float tnear, const unsigned char *__restrict__ marks,
                                                                  unsigned *__restrict__ out, unsigned *counter, int *spill_base) {
  __shared__ int stack[TRAV_STACK * TRAV_BLOCK];
  int *lds = &stack[threadIdx.x];
  int *spill = spill_base + (size_t)(blockIdx.x * TRAV_BLOCK + threadIdx.x) * TRAV_SPILL;
  for (;;) {
    const unsigned base = fetch_batch(counter);
    if (base >= n) break;
    const unsigned j = base + lane_id();
    if (j < n) {
      unsigned c[4] = { 0, 0, 0, 0 };
      if (T.nodes) {
        const float4 a = q.p0[j], b = q.p1[j];
        float bt = GVT_FLT_MAX, bu, bv;
        int bp = -1;
        traverse_count(T, mk3(a.x, a.y, a.z), mk3(b.x, b.y, b.z), tnear, lds, spill, bt, bp, bu, bv, c, marks);
      }
      out[j] = c[3];
    }
  }
}

// diagnostic (not on the hot path): per-ray visit counts of the closest-hit traversal.
// out[3*j + 0..2] = inner-node visits / leaf visits / triangle tests of ray j (reduced on the host).
__global__ __launch_bounds__(TRAV_BLOCK) void k_visit_stats(RayPlanes q, unsigned n, Trav T, float tnear, unsigned *__restrict__ out,
                                                             unsigned *counter, int *spill_base) {
  __shared__ int stack[TRAV_STACK * TRAV_BLOCK];
  int *lds = &stack[threadIdx.x];
  int *spill = spill_base + (size_t)(blockIdx.x * TRAV_BLOCK + threadIdx.x) * TRAV_SPILL;
  for (;;) {
    const unsigned base = fetch_batch(counter);
    if (base >= n) break;
    const unsigned j = base + lane_id();
    if (j < n) {
      unsigned c[4] = { 0, 0, 0, 0 };
      if (T.nodes) {
        const float4 a = q.p0[j], b = q.p1[j];
        float bt = GVT_FLT_MAX, bu, bv;
        int bp = -1;
        traverse_count(T, mk3(a.x, a.y, a.z), mk3(b.x, b.y, b.z), tnear, lds, spill, bt, bp, bu, bv, c);
      }
      out[3 * j] = c[0]; out[3 * j + 1] = c[1]; out[3 * j + 2] = c[2];
    }
  }
}
