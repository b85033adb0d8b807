// volume_ao_grid.inc -- the ambient occlusion grid of the AO frame (gvt_hip_volume_ao_grid_bake; the contract: include/gvt_hip.h, "ambient
// occlusion").  Included by volume.hip behind volume_light_grid.inc, whose kernel it restates.
//   k_volume_bake_ao<T>   one lane per VERTEX: the lane walks the vertex's n_dirs rays one after another -- k_volume_bake_light's ray, clipped
//                         at the radius (GVT_HIP_RAY_CLIP with t_max = radius; none with radius = +Inf) -- and keeps the direction's index i
//                         and the sum s in registers: when a ray ends s = s + (1 - A), and after the last one AO = s / (float)n_dirs is
//                         stored at the vertex.  So the sum has the contract's order without a second kernel and without n_dirs planes of
//                         intermediate memory, and neighbouring lanes march neighbouring vertices in the same direction for as long as
//                         their rays are equally long.
// KEEP IN STEP with k_volume_bake_light: persistent waves, the same refill, the same ownership walk and visit, the VOL_BAKE_STATS counters.
// The differences: the work item is a vertex, not a (vertex, light) pair; the ray's setup stands at the head of the loop, where it serves
// the fresh vertex and the next direction alike; the directions come from a small device table (n_dirs x 3 floats, normalised by the
// host), because a lane's index i is NOT wave-uniform -- by-value kernel arguments indexed per lane would be copied to scratch.
// Termination: every change of brick is followed by a sample that brick owns, a visit walks at most 2^22 positions (vol_ray_range), a
// lane walks n_dirs <= GVT_HIP_VOLUME_AO_MAX_DIRS rays per vertex; no lane waits for another wave.

template <typename T>
__global__ __launch_bounds__(VOL_BLOCK) void k_volume_bake_ao(VolDev U, SurfDev S, const FusedBrick *__restrict__ bricks, const LightGridBrick *__restrict__ parts,
                                                              unsigned n_bricks, unsigned n, Mat4 m, Mat4 minv, const float *__restrict__ dirs, int n_dirs, float t0,
                                                              float radius, unsigned *__restrict__ work, unsigned long long *__restrict__ stats) {
  // U: the WHOLE grid as one brick (offset 0, counts = the global counts, lo / hi the global vertex box); V: the lane's brick
  bool active = false, exhausted = false;
  bool fresh = false; // the lane's ray i is not set up yet
  VolDev V = U;
  V.nx = 0; V.ny = 0; V.nz = 0; // (owns nothing: the first sample looks its brick up)
  float o[3] = { 0.f, 0.f, 0.f }, d[3] = { 0.f, 0.f, 0.f }, C[3] = { 0.f, 0.f, 0.f }, A = 0.f;
  float wp[3] = { 0.f, 0.f, 0.f }; // the vertex in world space: the origin of all its rays
  float sum = 0.f;
  int dir = 0;
  int k = 0, k_hi = -1, prev = -1;
  bool seen = false;
  float *out = nullptr;
  unsigned n_marched = 0, n_gathered = 0, n_crossed = 0;
  const int clip_flag = radius < INFINITY ? GVT_HIP_RAY_CLIP : 0;
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
      if (!active && slot < n) { // the vertex of work item `slot`: its brick, its place in the plane, its world position
        unsigned b = 0;
        while (b + 1 < n_bricks && parts[b + 1].first <= slot) b++;
        const FusedBrick R = bricks[b];
        const LightGridBrick Q = parts[b];
        const unsigned v = slot - Q.first;
        const unsigned row = (unsigned)R.nx * (unsigned)R.ny;
        const unsigned vz = v / row, vy = (v - vz * row) / (unsigned)R.nx, vx = v - vz * row - vy * (unsigned)R.nx;
        out = Q.grid + v;
        // the vertex in object space (one multiply, one add) and in world space (the point transform)
        const V3 p = mk3(U.gox + (float)(R.ox + (int)vx) * U.sx, U.goy + (float)(R.oy + (int)vy) * U.sy, U.goz + (float)(R.oz + (int)vz) * U.sz);
        const V3 w = xfm_point(m, p);
        wp[0] = w.x; wp[1] = w.y; wp[2] = w.z;
        active = true;
        fresh = true;
        dir = 0;
        sum = 0.f;
      }
    }
    if (!ballot64(active)) {
      if (exhausted) break;
      continue;
    }
    if (active && fresh) { // ray `dir` of the vertex: its range over the whole grid, clipped at the radius
      fresh = false;
      const float *w = dirs + 3 * dir;
      vol_ray_range<true>(U, minv, make_float4(wp[0], wp[1], wp[2], t0), make_float4(w[0], w[1], w[2], radius), clip_flag, o, d, k, k_hi);
      seen = false;
      prev = -1;
      A = 0.f;
      V.nx = 0; V.ny = 0; V.nz = 0;
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
        const int bi = ((c[2] >> 3) * ((V.ny + 6) >> 3) + (c[1] >> 3)) * ((V.nx + 6) >> 3) + (c[0] >> 3); // (fused_macro_cell's expression, as in the light bake)
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
      if (done) { // the ray's part of the sum, in the directions' order; then the next direction, or the vertex is finished
        sum = sum + (1.f - A);
        dir++;
        if (dir < n_dirs) {
          fresh = true;
        } else {
          *out = sum / (float)n_dirs;
          active = false;
        }
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
