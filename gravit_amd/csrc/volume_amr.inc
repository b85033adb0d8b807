// volume_amr.inc -- AMR volumes: nested refined subgrids inside a brick (Volume::griddata / AddAMRGrid, render/data/primitives/Volume.h:40-58,
// 101-135; api::addAmrSubgrid, api.cpp:543-612).  Included by volume.hip, inside its anonymous namespace, behind the steps of the march.
//   k_volume_march_amr<CLIP>   the plain F32 march with the descent: per gathered sample, from the level-0 cell down the subgrids that cover it
//   k_volume_march_amr_surf / _lit / _surf_lit <CLIP>   the same body with the surface and lit steps of volume_march_body, for volumes whose
//                              subgrids were set with GVT_HIP_VOLUME_AMR_SHADED: crossings and shading read the FINAL grid's cell
//   k_amr_ranges               every subgrid's vertices reduced into the level-0 macro cells whose closed box they lie in
//   k_amr_ranges_merge         the same reduction per macro cell, merged into the level-0 ranges on the device (gvt_hip_volume_update_amr)
// The contract is stated in include/gvt_hip.h ("AMR volumes"); tests/volume_amr_checker.py restates it in numpy.
//
// Device tables (built by amr_build on the host):
//   mc[b]    per level-0 macro cell, ONE 8-byte word: x = first entry of its level-1 subgrids in `list`, y = their count | bit 31 = the macro
//            cell is not empty (what d_mc holds for the plain march: a sample of a macro cell without subgrids pays this one load, as before)
//   list     subgrid ids: the level-1 subgrids per macro cell, then every subgrid's children
//   desc     4 x int4 per subgrid: (lo.xyz in cells of its parent -- for a level-1 subgrid relative to the BRICK's first cell --, log2 ratio),
//            (cells.xyz, vertices per row), (vertices per slice, first child in `list`, children, 0), (sample offset in `vox`: low, high, 0, 0)
//   vox      the subgrids' samples, one allocation, float32, x fastest
// The index of a descriptor is lane-divergent, so the tables are read with ordinary vector loads.
struct AmrDev {
  const uint2 *mc;
  const int *list;
  const int4 *desc;
  const float *vox;
};

// vol_gather for a grid given by its first vertex of the cell and its strides (the same expression, term for term)
__device__ __forceinline__ float amr_gather(const float *p, size_t sy, size_t sz, const float f[3]) {
  const float v000 = p[0], v100 = p[1], v010 = p[sy], v110 = p[sy + 1];
  const float v001 = p[sz], v101 = p[sz + 1], v011 = p[sz + sy], v111 = p[sz + sy + 1];
  const float c00 = lerp_(v000, v100, f[0]), c10 = lerp_(v010, v110, f[0]);
  const float c01 = lerp_(v001, v101, f[0]), c11 = lerp_(v011, v111, f[0]);
  const float c0 = lerp_(c00, c10, f[1]), c1 = lerp_(c01, c11, f[1]);
  return lerp_(c0, c1, f[2]);
}
// ... and the eight corners it has just read, for the gradient of the shaded marches: the same addresses, so the loads are the gather's.
// (Handed back by amr_gather itself, through a reference or a pointer, the plain AMR kernels schedule two moves the other way round, and
// they are to stay what they were; a function of its own leaves them alone)
__device__ __forceinline__ void amr_corners(const float *p, size_t sy, size_t sz, VolCorners &G) {
  G.v000 = p[0]; G.v100 = p[1]; G.v010 = p[sy]; G.v110 = p[sy + 1];
  G.v001 = p[sz]; G.v101 = p[sz + 1]; G.v011 = p[sz + sy]; G.v111 = p[sz + sy + 1];
}

// The descent: cell c (relative to the brick) and fractions f of the level-0 grid become the cell and fractions of the finest grid that
// covers the sample; p / sy / sz = that grid's first vertex of the cell and its strides.  Every step is exact in float32 (f < 1, the
// ratio a power of two), so which grid a sample falls into is decided on integer cell indices.  log2_r: log2 of R, the product of the
// ratios down to the final grid (0 at level 0, at most 9).  Returns true if the final grid is a subgrid
__device__ __forceinline__ bool amr_descend(const VolDev &V, const AmrDev &A, uint2 word, const int c[3], float f[3], const float *&p, size_t &sy, size_t &sz,
                                            int &log2_r) {
  int ci[3] = { c[0], c[1], c[2] };
  int first = (int)word.x, cnt = (int)(word.y & 0x7fffffffu);
  sy = (size_t)V.nx; sz = (size_t)V.nx * (size_t)V.ny;
  const float *base = (const float *)V.vox;
  bool refined = false;
  log2_r = 0;
  for (int level = 1; level < GVT_HIP_VOLUME_MAX_LEVELS && cnt > 0; level++) {
    int found = -1;
    int4 d0 = make_int4(0, 0, 0, 0);
    for (int i = 0; i < cnt && found < 0; i++) { // (at most one covers the cell)
      const int id = A.list[first + i];
      d0 = A.desc[4 * (size_t)id];
      const int4 d1 = A.desc[4 * (size_t)id + 1];
      if (ci[0] >= d0.x && ci[0] < d0.x + d1.x && ci[1] >= d0.y && ci[1] < d0.y + d1.y && ci[2] >= d0.z && ci[2] < d0.z + d1.z) found = id;
    }
    if (found < 0) break;
    const int4 d1 = A.desc[4 * (size_t)found + 1], d2 = A.desc[4 * (size_t)found + 2], d3 = A.desc[4 * (size_t)found + 3];
    const int shift = d0.w, ratio = 1 << shift, lo[3] = { d0.x, d0.y, d0.z };
    for (int a = 0; a < 3; a++) {
      const float h = f[a] * (float)ratio;
      const int j = min((int)floorf(h), ratio - 1); // (h < ratio, as f < 1: the min only keeps the index inside the grid whatever f holds)
      ci[a] = ((ci[a] - lo[a]) << shift) + j;
      f[a] = h - (float)j;
    }
    sy = (size_t)(unsigned)d1.w; sz = (size_t)(unsigned)d2.x;
    base = A.vox + (((size_t)(unsigned)d3.y << 32) | (size_t)(unsigned)d3.x);
    first = d2.y; cnt = d2.z;
    log2_r += shift;
    refined = true;
  }
  p = base + (size_t)ci[0] + sy * (size_t)ci[1] + sz * (size_t)ci[2];
  return refined;
}

// The final grid's spacing per axis, s_a = spacing.a / (float)R, in a copy of V: what vol_gradient and vol_accumulate_lit divide by.  R is a
// power of two, so the product with 2^-log2_r is that quotient, bit for bit (both are the one correctly rounded value)
__device__ __forceinline__ VolDev amr_fine_spacing(const VolDev &V, int log2_r) {
  const float inv_r = __int_as_float((127 - log2_r) << 23);
  VolDev F = V;
  F.sx = V.sx * inv_r; F.sy = V.sy * inv_r; F.sz = V.sz * inv_r;
  return F;
}

// volume_march_body<float, SURF, CLIP, LIT> with the descent between the skip decision and the gather: lattice, ownership, skipping,
// jumps, sides, crossings, look-up, shading, compositing and write-back are the plain marches', through the same functions.  The corners,
// the fractions and the spacing a gradient reads are the FINAL grid's (amr_corners, the descended f, amr_fine_spacing); the plane sides
// and a plane's normal read the lattice point as ever.  stats[4] counts the refined samples.  Without SURF and LIT: the plain AMR march as
// it was, instruction for instruction (S is NoSurf, nothing of the shaded steps is instantiated).
// KEEP IN STEP: the per-sample steps for SURF / LIT are volume_march_body's (volume.hip); a change to the visit there is a change here.
template <bool SURF, bool LIT, bool CLIP>
__device__ __forceinline__ void volume_march_amr_body(const VolDev &V, const AmrDev &Am, const MarchTable<SURF, LIT> &S, RayPlanes q, unsigned n, const Mat4 &minv,
                                                      unsigned *__restrict__ work, unsigned long long *__restrict__ stats) {
  bool active = false, exhausted = false;
  unsigned idx = 0;
  float o[3] = { 0.f, 0.f, 0.f }, d[3] = { 0.f, 0.f, 0.f }, C[3] = { 0.f, 0.f, 0.f }, A = 0.f;
  int k = 0, k_hi = -1, k_last = -1, k_carry = -1, prev = -1; // (k_carry, prev, n_crossed: SURF only)
  bool seen = false;
  unsigned long long n_marched = 0, n_gathered = 0, n_refined = 0;
  unsigned n_crossed = 0;
  unsigned long long n_shaded = 0; // (LIT only)
  for (;;) {
    const unsigned long long idle = ballot64(!active);
    if (idle && !exhausted && (__popcll(idle) >= VOL_REFILL_MIN || idle == ballot64(true))) {
      const unsigned slot = wave_alloc(work, !active);
      if (ballot64(!active && slot >= n)) exhausted = true; // (wave-uniform)
      if (!active && slot < n) {
        idx = slot;
        active = true;
        const float4 a = q.p0[idx], b = q.p1[idx], c = q.p2[idx], e = q.p3[idx];
        const int k_prog = vol_ray_range<CLIP>(V, minv, a, b, __float_as_int(e.y), o, d, k, k_hi);
        C[0] = c.x; C[1] = c.y; C[2] = c.z;
        A = e.z;
        k_last = -1;
        seen = false;
        if constexpr (SURF) { // the sides of the sample in t_min count only for the sample right after it
          const bool carried = (__float_as_int(e.y) & GVT_HIP_RAY_SIDES) != 0;
          prev = carried ? ((int)c.w & 0xffff) : -1;
          k_carry = carried ? k_prog : -1;
        }
      }
    }
    if (!ballot64(active)) break;
    if (active) {
      bool done = false;
      for (int s = 0; s < VOL_STEP; s++) {
        if (k > k_hi) { done = true; break; }
        int c[3];
        float f[3];
        if (!vol_cell(V, o, d, k, c, f)) {
          if (seen) { done = true; break; }
          k++;
          continue;
        }
        if constexpr (SURF)
          if (!seen && k != k_carry) prev = -1;
        seen = true;
        k_last = k;
        n_marched++;
        const int bi = ((c[2] >> 3) * V.nby + (c[1] >> 3)) * V.nbx + (c[0] >> 3);
        const uint2 word = Am.mc[bi];
        // Plain: empty by the union of every level's vertices in the macro cell: +0 per sample, whatever grid it is in.  SURF: the cell word
        // is built from that union too (upload_cells reads the merged ranges), so no sample of any level in it changes an isovalue side
        unsigned pl = 0u;
        bool skip;
        if constexpr (SURF) {
          float p[3];
          vol_point(V, o, d, k, p);
          pl = surf_plane_sides(S, p);
          const unsigned cell = V.skip ? S.cells[bi] : 0u;
          skip = (cell & VOL_CELL_SKIP) && (prev < 0 || prev == (int)((cell & 0xffffu) | pl));
          if (skip) prev = (int)((cell & 0xffffu) | pl);
        } else {
          skip = V.skip && !(word.y >> 31);
        }
        if (skip) {
          if (A >= GVT_HIP_VOLUME_OPAQUE_A) { k++; done = true; break; }
          const int kj = vol_jump_target(V, o, d, k, k_hi, c);
          bool jump = kj > k;
          if constexpr (SURF) jump = jump && surf_planes_clear(V, S, o, d, k, kj);
          if (jump) {
            n_marched += (unsigned long long)(kj - k);
            k_last = kj;
            k = kj;
          }
          k++;
          continue;
        }
        n_gathered++;
        const float *p;
        size_t sy, sz;
        int log2_r;
        if (amr_descend(V, Am, word, c, f, p, sy, sz, log2_r)) n_refined++;
        const float v = amr_gather(p, sy, sz, f);
        VolCorners G;
        if constexpr (SURF || LIT) amr_corners(p, sy, sz, G);
        if constexpr (SURF) {
          unsigned sides = pl;
          for (int i = 0; i < S.n_iso; i++)
            if (v >= S.iso[i]) sides |= 1u << i;
          unsigned crossed = prev < 0 ? 0u : (sides ^ (unsigned)prev);
          prev = (int)sides;
          if (crossed) {
            float gc[3] = { 0.f, 0.f, 0.f }; // the isovalues crossed here share one gradient: the final cell's
            if (crossed & ((1u << S.n_iso) - 1u)) vol_gradient(amr_fine_spacing(V, log2_r), G, f, gc);
            while (crossed && A < GVT_HIP_VOLUME_OPAQUE_A) {
              const int i = __ffs((int)crossed) - 1;
              crossed &= crossed - 1u;
              n_crossed++;
              if (i < S.n_iso) {
                surf_composite(S, vol_lookup(V, S.iso[i]), gc, C, A);
              } else {
                const float4 P = S.plane[i - S.n_iso];
                const float g[3] = { P.x, P.y, P.z };
                surf_composite(S, vol_lookup(V, v), g, C, A);
              }
            }
            if (A >= GVT_HIP_VOLUME_OPAQUE_A) { k++; done = true; break; } // the surface ends the ray: the sample itself adds nothing
          }
        }
        if constexpr (LIT) n_shaded += vol_accumulate_lit<float, false>(amr_fine_spacing(V, log2_r), S, NoGhost{}, c, v, G, f, C, A);
        else vol_accumulate(V, v, C, A);
        k++;
        if (A >= GVT_HIP_VOLUME_OPAQUE_A) { done = true; break; }
      }
      if (done) {
        vol_write_back<SURF>(V, q, idx, k_last, C, A, prev);
        active = false;
      }
    }
  }
  unsigned long long n_cr = n_crossed;
  for (int s = 32; s >= 1; s >>= 1) {
    n_marched += __shfl_xor(n_marched, s);
    n_gathered += __shfl_xor(n_gathered, s);
    n_refined += __shfl_xor(n_refined, s);
    if constexpr (SURF) n_cr += __shfl_xor(n_cr, s);
    if constexpr (LIT) n_shaded += __shfl_xor(n_shaded, s);
  }
  if (lane_id() == 0 && n_marched) {
    atomicAdd(&stats[0], n_marched);
    atomicAdd(&stats[1], n_gathered);
    if (n_refined) atomicAdd(&stats[4], n_refined);
    if constexpr (SURF)
      if (n_cr) atomicAdd(&stats[2], n_cr);
    if constexpr (LIT)
      if (n_shaded) atomicAdd(&stats[3], n_shaded);
  }
}

// The entry points.  The plain one is the march AMR volumes always had; the three shaded ones (GVT_HIP_VOLUME_AMR_SHADED) receive the
// tables the plain shaded marches receive: SurfDev with surfaces, the lights alone (LightDev) without
template <bool CLIP>
__global__ __launch_bounds__(VOL_BLOCK) void k_volume_march_amr(VolDev V, AmrDev Am, RayPlanes q, unsigned n, Mat4 minv, unsigned *__restrict__ work,
                                                                unsigned long long *__restrict__ stats) {
  volume_march_amr_body<false, false, CLIP>(V, Am, NoSurf{}, q, n, minv, work, stats);
}
template <bool CLIP>
__global__ __launch_bounds__(VOL_BLOCK) void k_volume_march_amr_surf(VolDev V, AmrDev Am, SurfDev S, RayPlanes q, unsigned n, Mat4 minv, unsigned *__restrict__ work,
                                                                     unsigned long long *__restrict__ stats) {
  volume_march_amr_body<true, false, CLIP>(V, Am, S, q, n, minv, work, stats);
}
template <bool CLIP>
__global__ __launch_bounds__(VOL_BLOCK) void k_volume_march_amr_lit(VolDev V, AmrDev Am, LightDev L, RayPlanes q, unsigned n, Mat4 minv, unsigned *__restrict__ work,
                                                                    unsigned long long *__restrict__ stats) {
  volume_march_amr_body<false, true, CLIP>(V, Am, L, q, n, minv, work, stats);
}
template <bool CLIP>
__global__ __launch_bounds__(VOL_BLOCK) void k_volume_march_amr_surf_lit(VolDev V, AmrDev Am, SurfDev S, RayPlanes q, unsigned n, Mat4 minv, unsigned *__restrict__ work,
                                                                         unsigned long long *__restrict__ stats) {
  volume_march_amr_body<true, true, CLIP>(V, Am, S, q, n, minv, work, stats);
}

// ---- the subgrids' part of the macro cells' value ranges.  A work item is (subgrid, level-0 macro cell whose closed box holds some of its
// vertices); subgrids are cell-aligned, so those vertices are the index rectangle [i0, i1] per axis (both ends included).  One block per
// item (grid-stride), vr_add's rule per vertex, the wave's shuffles and the block's LDS; out[item] has ONE writer.  The host merges the
// items into the level-0 ranges (a macro cell may have several).
struct AmrRangeItem {
  unsigned long long base; // the subgrid's first sample in vox
  unsigned nx, nxy;        // its vertices per row and per slice
  unsigned i0[3], ext[3];  // the rectangle's first vertex and its extent (>= 1) per axis
};
struct AmrRangeOut { float mn, mx; unsigned wild; };

__global__ __launch_bounds__(VOL_BLOCK) void k_amr_ranges(const float *__restrict__ vox, const AmrRangeItem *__restrict__ items, unsigned n_items,
                                                          AmrRangeOut *__restrict__ out) {
  constexpr int WAVES = VOL_BLOCK / 64;
  __shared__ float s_mn[WAVES], s_mx[WAVES];
  __shared__ unsigned s_w[WAVES];
  for (unsigned it = blockIdx.x; it < n_items; it += gridDim.x) { // (block-uniform)
    const AmrRangeItem I = items[it];
    const size_t ex = I.ext[0], exy = ex * I.ext[1], total = exy * I.ext[2];
    const float *g = vox + I.base;
    VRange r = vr_none();
    for (size_t t = threadIdx.x; t < total; t += VOL_BLOCK) {
      const size_t z = t / exy, rem = t - z * exy, y = rem / ex, x = rem - y * ex;
      vr_add(r, g[(size_t)(I.i0[0] + x) + (size_t)I.nx * (I.i0[1] + y) + (size_t)I.nxy * (I.i0[2] + z)]);
    }
    r = vr_wave_all(r);
    if ((threadIdx.x & 63u) == 0u) { s_mn[threadIdx.x >> 6] = r.mn; s_mx[threadIdx.x >> 6] = r.mx; s_w[threadIdx.x >> 6] = r.wild; }
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int w = 1; w < WAVES; w++) vr_merge(r, VRange{ s_mn[w], s_mx[w], s_w[w] });
      out[it] = AmrRangeOut{ r.mn, r.mx, r.wild };
    }
    __syncthreads(); // (the next round writes the LDS again)
  }
}

// ---- gvt_hip_volume_update_amr: the same reduction per time step, merged on the device.  The items of k_amr_ranges, grouped by macro
// cell (built once per tree, amr_merge_tables); a block takes a macro cell that has items (grid-stride), reduces ALL of its rectangles
// and merges the result into the level-0 range k_vol_ranges has just written for that cell: bmin / bmax / bnan then hold the union the
// host used to form (amr_refresh_ranges), by the same rule (vr_merge).  ONE writer per macro cell, no atomics.
// A rectangle is walked by rows: a wave per (y, z) row, its lanes along x, so neighbouring lanes read neighbouring floats and the row's
// address costs one 32-bit division per row (the item is block-uniform: its words are scalar).  ext[1] * ext[2] fits 32 bits: a
// rectangle lies in one macro cell, at most 8 * 512 + 1 vertices per axis.
struct AmrMergeCell { unsigned cell, first, count; }; // the macro cell | its items in the grouped list

__global__ __launch_bounds__(VOL_BLOCK) void k_amr_ranges_merge(const float *__restrict__ vox, const AmrRangeItem *__restrict__ items,
                                                                const AmrMergeCell *__restrict__ cells, unsigned n_cells, float *__restrict__ bmin,
                                                                float *__restrict__ bmax, uint8_t *__restrict__ bnan) {
  constexpr unsigned WAVES = VOL_BLOCK / 64;
  __shared__ float s_mn[WAVES], s_mx[WAVES];
  __shared__ unsigned s_w[WAVES];
  const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  for (unsigned c = blockIdx.x; c < n_cells; c += gridDim.x) { // (block-uniform)
    const AmrMergeCell M = cells[c];
    VRange r = vr_none();
    for (unsigned k = 0; k < M.count; k++) {
      const AmrRangeItem I = items[M.first + k];
      const float *g = vox + I.base + I.i0[0] + (size_t)I.nx * I.i0[1] + (size_t)I.nxy * I.i0[2];
      const unsigned rows = I.ext[1] * I.ext[2];
      for (unsigned row = wave; row < rows; row += WAVES) {
        const unsigned z = row / I.ext[1], y = row - z * I.ext[1];
        const float *p = g + (size_t)I.nx * y + (size_t)I.nxy * z;
        for (unsigned x = lane; x < I.ext[0]; x += 64u) vr_add(r, p[x]);
      }
    }
    r = vr_wave_all(r);
    if (lane == 0u) { s_mn[wave] = r.mn; s_mx[wave] = r.mx; s_w[wave] = r.wild; }
    __syncthreads();
    if (threadIdx.x == 0) { // the one writer of this macro cell
      for (unsigned w = 1; w < WAVES; w++) vr_merge(r, VRange{ s_mn[w], s_mx[w], s_w[w] });
      vr_merge(r, VRange{ bmin[M.cell], bmax[M.cell], bnan[M.cell] });
      bmin[M.cell] = r.mn; bmax[M.cell] = r.mx; bnan[M.cell] = (uint8_t)r.wild;
    }
    __syncthreads(); // (the next round writes the LDS again)
  }
}
