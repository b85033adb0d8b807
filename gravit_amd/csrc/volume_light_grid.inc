// volume_light_grid.inc -- the light transmittance grids of the fog-shadowed frame (gvt_hip_volume_light_grid_bake; the contract:
// include/gvt_hip.h, "shadowed fog").  Included by volume.hip behind volume_fused_shadow.inc, whose shadow-ray visit it restates.
//   k_volume_bake_light<T>   one lane per (vertex, usable light): the shadow ray from the vertex towards the light, marched to its end,
//                            G = 1 - A_s stored at the vertex.  Persistent waves with the fused kernels' refill, because a ray from a
//                            vertex under the light's face has no sample and one from the far corner crosses the whole grid.
// The walk is driven by SAMPLE OWNERSHIP, not by box exits: the lattice range is taken once from the global vertex box (the one brick's
// vol_ray_range), and whenever the lane's brick does not own sample k the brick that owns k's global cell is looked up in the brick
// table (at most 256 records, read with a uniform index).  So a ray that runs IN a face two bricks share is marched by the brick that
// owns its samples, which the next-brick rule of the frames skips (gvt_hip.h, "shadowed surfaces", DEVIATIONS (5)), and the grid has the
// one brick's bits in every bricking.  Every change of brick is followed by a sample that brick owns, so the walk terminates.
// KEEP IN STEP with the shadow-ray mode (mode > 0) of k_volume_march_fused_shadow: opacity alone, the colour dead.
#define VOL_BAKE_STATS 3 // samples marched, samples gathered, crossings

// a brick's part of the work list and where its planes go: items [first, first + n_vert * usable lights), x fastest, one plane per light
struct LightGridBrick {
  float *grid;
  unsigned first;
  unsigned pad;
};

template <typename T>
__global__ __launch_bounds__(VOL_BLOCK) void k_volume_bake_light(VolDev U, SurfDev S, ShadowDev H, const FusedBrick *__restrict__ bricks,
                                                                 const LightGridBrick *__restrict__ parts, unsigned n_bricks, unsigned n, Mat4 m, Mat4 minv,
                                                                 unsigned *__restrict__ work, unsigned long long *__restrict__ stats) {
  // U: the WHOLE grid as one brick (offset 0, counts = the global counts, lo / hi the global vertex box); V: the lane's brick
  bool active = false, exhausted = false;
  VolDev V = U;
  V.nx = 0; V.ny = 0; V.nz = 0; // (owns nothing: the first sample looks its brick up)
  float o[3] = { 0.f, 0.f, 0.f }, d[3] = { 0.f, 0.f, 0.f }, C[3] = { 0.f, 0.f, 0.f }, A = 0.f;
  int k = 0, k_hi = -1, prev = -1;
  bool seen = false;
  float *out = nullptr;
  unsigned n_marched = 0, n_gathered = 0, n_crossed = 0;
  for (;;) {
    const unsigned long long idle = ballot64(!active);
    if (idle && !exhausted && (__popcll(idle) >= VOL_REFILL_MIN || idle == ballot64(true))) {
      const unsigned slot = wave_alloc(work, !active);
      if (ballot64(!active && slot >= n)) exhausted = true; // (wave-uniform)
      if (n_marched >= 0x40000000u || n_crossed >= 0x40000000u) {
        atomicAdd(&stats[0], (unsigned long long)n_marched); atomicAdd(&stats[1], (unsigned long long)n_gathered);
        atomicAdd(&stats[2], (unsigned long long)n_crossed);
        n_marched = 0; n_gathered = 0; n_crossed = 0;
      }
      if (!active && slot < n) { // the ray of work item `slot`: its brick, its light, its vertex
        unsigned b = 0;
        while (b + 1 < n_bricks && parts[b + 1].first <= slot) b++;
        const FusedBrick R = bricks[b];
        const LightGridBrick Q = parts[b];
        const unsigned local = slot - Q.first;
        const unsigned n_vert = (unsigned)R.nx * (unsigned)R.ny * (unsigned)R.nz;
        const unsigned l = local / n_vert, v = local - l * n_vert;
        const unsigned row = (unsigned)R.nx * (unsigned)R.ny;
        const unsigned vz = v / row, vy = (v - vz * row) / (unsigned)R.nx, vx = v - vz * row - vy * (unsigned)R.nx;
        out = Q.grid + local;
        // the l-th usable light
        unsigned rest = H.usable;
        for (unsigned i = 0; i < l; i++) rest &= rest - 1u;
        const int lj = __ffs((int)rest) - 1;
        float ws[3] = { 0.f, 0.f, 0.f };
        for (int j = 0; j < S.n_lights; j++)
          if (j == lj) { ws[0] = H.ws[j][0]; ws[1] = H.ws[j][1]; ws[2] = H.ws[j][2]; }
        // the vertex in object space (one multiply, one add), in world space (the point transform), and the ray's range over the whole grid
        const V3 p = mk3(U.gox + (float)(R.ox + (int)vx) * U.sx, U.goy + (float)(R.oy + (int)vy) * U.sy, U.goz + (float)(R.oz + (int)vz) * U.sz);
        const V3 wp = xfm_point(m, p);
        vol_ray_range<false>(U, minv, make_float4(wp.x, wp.y, wp.z, H.t0), make_float4(ws[0], ws[1], ws[2], INFINITY), 0, o, d, k, k_hi);
        active = true;
        seen = false;
        prev = -1;
        A = 0.f;
        V.nx = 0; V.ny = 0; V.nz = 0;
      }
    }
    if (!ballot64(active)) {
      if (exhausted) break;
      continue;
    }
    if (active) {
      bool done = false;
      for (int s = 0; s < VOL_STEP; s++) {
        if (k > k_hi) { done = true; break; }
        int c[3];
        float f[3];
        if (!vol_cell(V, o, d, k, c, f)) {
          // not this brick's: whose?  Outside the grid the one brick's rules hold (nothing seen yet: the next index; else the ray ends)
          int gc[3];
          if (!vol_cell(U, o, d, k, gc, f)) {
            if (seen) { done = true; break; }
            k++;
            continue;
          }
          unsigned b = 0;
          for (; b < n_bricks; b++) {
            const FusedBrick R = bricks[b];
            if (gc[0] >= R.ox && gc[0] <= R.ox + R.nx - 2 && gc[1] >= R.oy && gc[1] <= R.oy + R.ny - 2 && gc[2] >= R.oz && gc[2] <= R.oz + R.nz - 2) break;
          }
          if (b == n_bricks) { done = true; break; } // (the bake's bricks tile the grid: not reached)
          const FusedBrick R = bricks[b];
          V.vox = R.vox; V.mc = R.mc;
          V.nx = R.nx; V.ny = R.ny; V.nz = R.nz; V.ox = R.ox; V.oy = R.oy; V.oz = R.oz;
          if (!vol_cell(V, o, d, k, c, f)) { done = true; break; } // (the same g, the same test: not reached)
        }
        seen = true;
        n_marched++;
        // (fused_macro_cell's expression, restated: through the function, by value or by reference, this kernel comes out two VGPRs
        // larger -- profiles/volume_hoist.txt)
        const int bi = ((c[2] >> 3) * ((V.ny + 6) >> 3) + (c[1] >> 3)) * ((V.nx + 6) >> 3) + (c[0] >> 3); // (nby, nbx of this brick)
        float p[3];
        vol_point(V, o, d, k, p);
        const unsigned pl = surf_plane_sides(S, p);
        const unsigned cell = V.skip ? ((const uint32_t *)V.mc)[bi] : 0u;
        const bool skip = (cell & VOL_CELL_SKIP) && (prev < 0 || prev == (int)((cell & 0xffffu) | pl));
        if (skip) {
          prev = (int)((cell & 0xffffu) | pl);
          if (A >= GVT_HIP_VOLUME_OPAQUE_A) { k++; done = true; break; } // (the arrives-opaque rule; a ray here ends at the sample that makes it opaque)
          const int kj = vol_jump_target(V, o, d, k, k_hi, c);
          if (kj > k && surf_planes_clear(V, S, o, d, k, kj)) {
            n_marched += (unsigned)(kj - k);
            k = kj;
          }
          k++;
          continue;
        }
        n_gathered++;
        VolCorners G;
        const float v = vol_gather<T>(V, c, f, G);
        unsigned sides = pl;
        for (int i = 0; i < S.n_iso; i++)
          if (v >= S.iso[i]) sides |= 1u << i;
        unsigned crossed = prev < 0 ? 0u : (sides ^ (unsigned)prev);
        prev = (int)sides;
        if (crossed) {
          while (crossed && A < GVT_HIP_VOLUME_OPAQUE_A) {
            crossed &= crossed - 1u;
            n_crossed++;
            A = A + (1.f - A) * S.alpha;
          }
          if (A >= GVT_HIP_VOLUME_OPAQUE_A) { k++; done = true; break; } // the surface ends the ray: the sample itself adds nothing
        }
        vol_accumulate(V, v, C, A); // (shading NONE; the colour is dead)
        k++;
        if (A >= GVT_HIP_VOLUME_OPAQUE_A) { done = true; break; }
      }
      if (done) {
        *out = 1.f - A;
        active = false;
      }
    }
  }
  unsigned long long w_marched = n_marched, w_gathered = n_gathered, w_crossed = n_crossed;
  for (int s = 32; s >= 1; s >>= 1) {
    w_marched += __shfl_xor(w_marched, s);
    w_gathered += __shfl_xor(w_gathered, s);
    w_crossed += __shfl_xor(w_crossed, s);
  }
  if (lane_id() == 0) {
    if (w_marched) atomicAdd(&stats[0], w_marched);
    if (w_gathered) atomicAdd(&stats[1], w_gathered);
    if (w_crossed) atomicAdd(&stats[2], w_crossed);
  }
}
