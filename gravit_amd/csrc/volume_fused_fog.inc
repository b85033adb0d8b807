// volume_fused_fog.inc -- the fog-shadowed fused frame (gvt_hip_volume_frame_fog_shadowed; the contract: include/gvt_hip.h, "shadowed fog").
// Included by volume.hip behind volume_light_grid.inc, which bakes the grids this kernel reads.
//   k_volume_march_fused_fog<T, CLIP, CENTRAL>   k_volume_march_fused_shadow<T, CLIP, true, CENTRAL> with ONE change: a lit fog sample multiplies each light's
//                                   n . l by the transmittance towards that light, interpolated from the baked grid G_j at the eight
//                                   vertices of the sample's cell (the sample's fractions, vol_gather's nesting).  Crossings keep their
//                                   exact in-kernel shadow rays.
// KEEP IN STEP with k_volume_march_fused_shadow (and through it with k_volume_march_fused_shaded and volume_march_body): the kernel below
// is that kernel restated, for the reason that one restates its parents -- the kernels that exist are to stay what they are, instruction
// for instruction.  The differences: LIT is always on; the brick's grid pointer travels beside its record, in a parallel device table
// loaded where the record is loaded (FusedBrick is unchanged); the camera ray's lit sample is vol_accumulate_lit_grids'.
//   k_volume_march_fused_fog_lean<T, CLIP, CENTRAL>   the same change on k_volume_march_fused_shaded<T, CLIP, false, true, CENTRAL>, for a frame WITHOUT
//                                   surfaces: no crossing exists, so no shadow ray is ever cast and the park, the modes and the side masks
//                                   fall away with their registers and their LDS.  Measured before it existed (profiles/
//                                   volume_fog_shadows.txt, 3): the surface-capable kernel on a frame without surfaces took 1.40 to 1.46
//                                   times the lit fused frame under a table that shades 0.1 % of the samples -- the kernel's shape, not
//                                   the grid's reads.
// CENTRAL: as in k_volume_march_fused_shadow -- the lane's ghost pointer is loaded beside the grid pointer, with every record.
// G is read only inside the branch that shades (tc.w > 0, 0 < len < Inf), so skipping stays exact and samples_shaded does not move; A
// never depends on G.

// a brick's grid planes: float32, one plane of nx * ny * nz per usable light in the order of their bits, at the samples' own index
struct FogBrick {
  const float *grid;
};

// Og of the l-th usable light at cell c, fractions f: (float)O at the eight vertices of the occluder grid's plane (uint8, laid out as
// the light grid's), in the nesting of Tg below
__device__ __forceinline__ float occluder_lerp(const VolDev &V, const uint8_t *__restrict__ occ, int l, const int c[3], const float f[3]) {
  const size_t sy = (size_t)V.nx, sz = (size_t)V.nx * (size_t)V.ny, plane = sz * (size_t)V.nz;
  const uint8_t *p = occ + plane * (size_t)l + ((size_t)c[0] + sy * (size_t)c[1] + sz * (size_t)c[2]);
  const float c00 = lerp_((float)p[0], (float)p[1], f[0]), c10 = lerp_((float)p[sy], (float)p[sy + 1], f[0]);
  const float c01 = lerp_((float)p[sz], (float)p[sz + 1], f[0]), c11 = lerp_((float)p[sz + sy], (float)p[sz + sy + 1], f[0]);
  return lerp_(lerp_(c00, c10, f[1]), lerp_(c01, c11, f[1]), f[2]);
}

// vol_accumulate_lit<T, false> with a factor per light from the bricks' planes: ndl_s = ndl * Tg, with MESH (the mesh-shadowed frames)
// ndl * (Tg * Og) (an unusable light: 1, nothing read).  The planes are read at cell c of brick V with the fractions f0; the gradient
// is taken from the corners G and fractions f at the spacing of Vf.  Outside an AMR visit Vf is V and f0 is f; in one
// (volume_fused_shadow_amr.inc) G, f and Vf are the final cell's, c and f0 the level-0 cell's
template <typename T, bool CENTRAL, bool MESH, typename LT> // (LT: SurfDev or LightDev; CENTRAL: the gradient is vol_gradient_central's, from Hg)
__device__ __forceinline__ unsigned vol_accumulate_lit_grids(const VolDev &Vf, const VolDev &V, const LT &L, const GhostTable<CENTRAL> &Hg, unsigned usable,
                                                             const float *__restrict__ grid, const uint8_t *__restrict__ occ, const int c[3], const float f0[3], float v,
                                                             const VolCorners &G, const float f[3], float C[3], float &A) {
  const float4 tc = vol_lookup(V, v);
  float rgb[3] = { tc.x, tc.y, tc.z };
  const bool shaded = tc.w > 0.f; // (false for NaN)
  if (shaded) {
    float g[3], sum[3] = { 0.f, 0.f, 0.f };
    if constexpr (CENTRAL) vol_gradient_central<T>(V, Hg, c, G, f, g);
    else vol_gradient(Vf, G, f, g);
    const float len = sqrtf((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]);
    if (len > 0.f && len < INFINITY) { // (false for NaN)
      const float n[3] = { g[0] / len, g[1] / len, g[2] / len };
      const size_t sy = (size_t)V.nx, sz = (size_t)V.nx * (size_t)V.ny, plane = sz * (size_t)V.nz;
      const float *p = grid + ((size_t)c[0] + sy * (size_t)c[1] + sz * (size_t)c[2]);
      int l = 0;
      for (int j = 0; j < L.n_lights; j++) {
        const float ndl = fabsf((n[0] * L.ldir[j][0] + n[1] * L.ldir[j][1]) + n[2] * L.ldir[j][2]);
        float Ts = 1.f;
        if ((usable >> j) & 1u) { // (wave-uniform)
          const float c00 = lerp_(p[0], p[1], f0[0]), c10 = lerp_(p[sy], p[sy + 1], f0[0]);
          const float c01 = lerp_(p[sz], p[sz + 1], f0[0]), c11 = lerp_(p[sz + sy], p[sz + sy + 1], f0[0]);
          Ts = lerp_(lerp_(c00, c10, f0[1]), lerp_(c01, c11, f0[1]), f0[2]);
          if constexpr (MESH) Ts = Ts * occluder_lerp(V, occ, l, c, f0);
          p += plane;
          l++;
        }
        const float ndl_s = ndl * Ts;
        for (int a = 0; a < 3; a++) sum[a] = sum[a] + L.lcol[j][a] * ndl_s;
      }
    }
    for (int a = 0; a < 3; a++) rgb[a] = rgb[a] * (L.ka + L.kd * sum[a]);
  }
  const float fr = (1.f - A) * tc.w;
  C[0] = C[0] + fr * rgb[0]; C[1] = C[1] + fr * rgb[1]; C[2] = C[2] + fr * rgb[2];
  A = A + fr;
  return shaded ? 1u : 0u;
}

template <typename T, bool CLIP, bool CENTRAL>
__global__ __launch_bounds__(VOL_BLOCK) void k_volume_march_fused_fog(VolDev U, SurfDev S, ShadowDev H, const FusedBrick *__restrict__ bricks, const FogBrick *__restrict__ grids, TopDev top, RayPlanes q,
                                                                      unsigned n, Mat4 minv, const float *__restrict__ clip_plane, unsigned n_clip,
                                                                      float *__restrict__ fb, unsigned n_pix, unsigned *__restrict__ work,
                                                                      unsigned long long *__restrict__ stats, FusedGhostArg<CENTRAL> HG) {
  __shared__ float park[VOL_SHADOW_WORDS][VOL_BLOCK];
  float *const P = &park[0][threadIdx.x]; // the lane's column: word w at P[w * VOL_BLOCK]
  enum { P_K = 0, P_BRICK = 1, P_PREV = 2, P_C = 3, P_A = 6, P_TMIN = 7, P_T = 8 };
  bool active = false, exhausted = false;
  bool hop = false;
  unsigned idx = 0;
  VolDev V = U;
  const float *grid = nullptr; // the lane's brick's planes
  GhostTable<CENTRAL> Hl = fused_ghost_init<CENTRAL>(HG); // (CENTRAL only) the lane's brick's ghost layers: the pointer changes wherever the brick does
  int brick = -1;
  int mode = 0;
  float o[3] = { 0.f, 0.f, 0.f }, d[3] = { 0.f, 0.f, 0.f }, C[3] = { 0.f, 0.f, 0.f }, A = 0.f;
  int k = 0, k_hi = -1, k_last = -1, k_carry = -1, prev = -1;
  // (32 bits per lane, flushed between two bricks before they can wrap, as in the shaded kernel; the shadow rays' own beside them)
  unsigned n_marched = 0, n_gathered = 0, n_crossed = 0;
  unsigned n_shaded = 0;
  unsigned s_marched = 0, s_gathered = 0, s_crossed = 0;
  unsigned n_visits = 0, n_deposits = 0, s_visits = 0, s_rays = 0; // (wave-uniform: counted from ballots where the wave is converged)
  for (;;) {
    const unsigned long long idle = ballot64(!active);
    if (idle && !exhausted && (__popcll(idle) >= VOL_REFILL_MIN || idle == ballot64(true))) {
      const unsigned slot = wave_alloc(work, !active);
      if (ballot64(!active && slot >= n)) exhausted = true; // (wave-uniform)
      if (!active && slot < n) { // a camera ray: no colour, no opacity, no flags (so no side mask), no brick yet
        idx = slot;
        active = true;
        hop = true;
        brick = -1;
        mode = 0;
        C[0] = 0.f; C[1] = 0.f; C[2] = 0.f;
        A = 0.f;
        prev = -1;
      }
    }
    if (!ballot64(active)) {
      if (exhausted) break;
      continue; // (every ray of the refill met no brick: the wave fetches again)
    }
    // ---- between two bricks: k_volume_march_fused_shadow's block, for the camera ray of the list or for the shadow ray it casts
    bool entered = false, deposited = false, s_entered = false, s_cast = false;
    if (active && hop) {
      hop = false;
      const float4 a = q.p0[idx], b = q.p1[idx];
      const int id = __float_as_int(q.p3[idx].x);
      float t_clip;
      const bool cam_clip = fused_clip<CLIP>(id, clip_plane, n_clip, t_clip);
      if (n_marched >= 0x40000000u || n_crossed >= 0x40000000u) {
        atomicAdd(&stats[0], (unsigned long long)n_marched); atomicAdd(&stats[1], (unsigned long long)n_gathered);
        atomicAdd(&stats[4], (unsigned long long)n_crossed);
        atomicAdd(&stats[5], (unsigned long long)n_shaded);
        n_marched = 0; n_gathered = 0; n_crossed = 0; n_shaded = 0;
      }
      if (s_marched >= 0x40000000u || s_crossed >= 0x40000000u) {
        atomicAdd(&stats[8], (unsigned long long)s_crossed); atomicAdd(&stats[9], (unsigned long long)s_marched);
        atomicAdd(&stats[10], (unsigned long long)s_gathered);
        s_marched = 0; s_gathered = 0; s_crossed = 0;
      }
      // the ray this lane walks now, in the list's form: origin | t_min, direction, the clip
      float wo[3] = { a.x, a.y, a.z }, wd[3] = { b.x, b.y, b.z };
      float t_min = a.w; // (the end of a camera ray's visit has stored it there, as vol_write_back does)
      bool clip = cam_clip;
      if (mode > 0) { // the shadow ray: from the camera ray's sample (vol_point's form on the world ray) towards light mode - 1
        const float t = (float)__float_as_int(P[P_K * VOL_BLOCK]) * U.dt;
        for (int x = 0; x < 3; x++) wo[x] = wo[x] + wd[x] * t;
        for (int j = 0; j < S.n_lights; j++)
          if (j == mode - 1) { wd[0] = H.ws[j][0]; wd[1] = H.ws[j][1]; wd[2] = H.ws[j][2]; }
        t_min = P[P_TMIN * VOL_BLOCK];
        clip = false;
      }
      int next = -1;
      if (A < GVT_HIP_VOLUME_OPAQUE_A) next = vol_next(top, brick, wo, wd, t_min, clip, clip ? t_clip : INFINITY);
      bool resume = false;
      if (next < 0 && mode > 0) { // the shadow ray ends: T_j = 1 - A_s; the next usable light's ray, or back to the camera ray
        P[(P_T + mode - 1) * VOL_BLOCK] = 1.f - A;
        const unsigned rest = H.usable & ~((2u << (mode - 1)) - 1u);
        A = 0.f;
        prev = -1;
        brick = -1;
        if (rest) {
          mode = __ffs((int)rest);
          P[P_TMIN * VOL_BLOCK] = H.t0;
          s_cast = true;
          hop = true; // (its first brick: the next iteration)
        } else {
          resume = true;
          mode = -1;
          next = __float_as_int(P[P_BRICK * VOL_BLOCK]);
          wo[0] = a.x; wo[1] = a.y; wo[2] = a.z; wd[0] = b.x; wd[1] = b.y; wd[2] = b.z;
          t_min = a.w;
          clip = cam_clip;
        }
      }
      if (next >= 0) {
        const FusedBrick R = bricks[next];
        grid = grids[next].grid;
        if constexpr (CENTRAL) Hl.faces = HG.faces[next];
        V.vox = R.vox; V.mc = R.mc;
        V.nx = R.nx; V.ny = R.ny; V.nz = R.nz; V.ox = R.ox; V.oy = R.oy; V.oz = R.oz;
        for (int x = 0; x < 3; x++) { V.lo[x] = R.lo[x]; V.hi[x] = R.hi[x]; }
        const int k_prog = vol_ray_range<CLIP>(V, minv, make_float4(wo[0], wo[1], wo[2], t_min), make_float4(wd[0], wd[1], wd[2], clip ? t_clip : INFINITY),
                                               clip ? GVT_HIP_RAY_CLIP : 0, o, d, k, k_hi);
        k_last = -1;
        k_carry = prev >= 0 ? k_prog : -1; // the sides of the sample in t_min count only for the sample right after it
        if (resume) { // the camera ray is back in its brick, before sample k of the visit it had begun (k_last >= 0: no first-sample rule)
          k = __float_as_int(P[P_K * VOL_BLOCK]);
          k_last = k;
          k_carry = -1;
          prev = __float_as_int(P[P_PREV * VOL_BLOCK]);
          C[0] = P[(P_C + 0) * VOL_BLOCK]; C[1] = P[(P_C + 1) * VOL_BLOCK]; C[2] = P[(P_C + 2) * VOL_BLOCK];
          A = P[P_A * VOL_BLOCK];
        } else if (mode > 0) {
          s_entered = true;
        } else {
          entered = true;
        }
        brick = next;
      } else if (mode <= 0) {
        if (brick >= 0) { // OPAQUE, or EXTERNAL: the ray leaves the volume (a camera ray that meets no brick deposits nothing)
          deposited = true;
          fused_deposit(fb, n_pix, id, C, A);
        }
        active = false;
        // (the lane's march state is dead now; saying so frees its registers for this block's temporaries)
        V.vox = nullptr; V.mc = nullptr;
        grid = nullptr;
        if constexpr (CENTRAL) Hl.faces = nullptr;
        V.nx = V.ny = V.nz = V.ox = V.oy = V.oz = 0;
        for (int x = 0; x < 3; x++) { o[x] = 0.f; d[x] = 0.f; }
        k = 0; k_hi = -1; k_last = -1; k_carry = -1; prev = -1;
        brick = -1;
      }
    }
    n_visits += (unsigned)__popcll(ballot64(entered));
    n_deposits += (unsigned)__popcll(ballot64(deposited));
    s_visits += (unsigned)__popcll(ballot64(s_entered));
    s_rays += (unsigned)__popcll(ballot64(s_cast));
    // ---- the visit: k_volume_march_fused_shadow<T, CLIP, true>'s, step for step (KEEP IN STEP), for camera and shadow rays alike
    bool parked = false;
    if (active && !hop) {
      bool done = false;
      for (int s = 0; s < VOL_STEP; s++) {
        if (k > k_hi) { done = true; break; }
        int c[3];
        float f[3];
        if (!vol_cell(V, o, d, k, c, f)) {
          if (k_last >= 0) { done = true; break; } // a brick's samples along a line are contiguous: the rest belongs to others
          k++;
          continue;
        }
        if (k_last < 0 && k != k_carry) prev = -1;
        k_last = k;
        if (mode > 0) s_marched++; else n_marched++;
        const int bi = fused_macro_cell(V.nx, V.ny, c);
        float p[3];
        vol_point(V, o, d, k, p);
        const unsigned pl = surf_plane_sides(S, p);
        const unsigned cell = V.skip ? ((const uint32_t *)V.mc)[bi] : 0u;
        const bool skip = (cell & VOL_CELL_SKIP) && (prev < 0 || prev == (int)((cell & 0xffffu) | pl));
        if (skip) {
          prev = (int)((cell & 0xffffu) | pl);
          if (A >= GVT_HIP_VOLUME_OPAQUE_A) { k++; done = true; break; } // the ray arrived opaque: this sample adds +0 and ends it, as any sample does
          const int kj = vol_jump_target(V, o, d, k, k_hi, c);
          if (kj > k && surf_planes_clear(V, S, o, d, k, kj)) {
            if (mode > 0) s_marched += (unsigned)(kj - k); else n_marched += (unsigned)(kj - k);
            k_last = kj;
            k = kj;
          }
          k++;
          continue;
        }
        if (mode > 0) s_gathered++; else n_gathered++;
        VolCorners G;
        const float v = vol_gather<T>(V, c, f, G);
        unsigned sides = pl;
        for (int i = 0; i < S.n_iso; i++)
          if (v >= S.iso[i]) sides |= 1u << i;
        unsigned crossed = prev < 0 ? 0u : (sides ^ (unsigned)prev);
        if (crossed && mode == 0 && H.usable) {
          // a rendered crossing (A < OPAQUE_A at every sample a visit reaches) and no T_j yet: park, and become the first shadow ray.
          // prev is still the mask before this sample; what this pass counted is taken back, the re-run counts it
          n_marched--; n_gathered--;
          P[P_K * VOL_BLOCK] = __int_as_float(k);
          P[P_BRICK * VOL_BLOCK] = __int_as_float(brick);
          P[P_PREV * VOL_BLOCK] = __int_as_float(prev);
          P[(P_C + 0) * VOL_BLOCK] = C[0]; P[(P_C + 1) * VOL_BLOCK] = C[1]; P[(P_C + 2) * VOL_BLOCK] = C[2];
          P[P_A * VOL_BLOCK] = A;
          P[P_TMIN * VOL_BLOCK] = H.t0;
          for (int j = 0; j < S.n_lights; j++) P[(P_T + j) * VOL_BLOCK] = 1.f; // (a light that casts no ray: T_j = 1)
          mode = __ffs((int)H.usable);
          A = 0.f;
          prev = -1;
          brick = -1;
          hop = true;
          parked = true;
          break;
        }
        prev = (int)sides;
        const bool have_T = mode < 0; // (the re-run of the parked sample, and that sample alone)
        if (have_T) mode = 0;
        if constexpr (CENTRAL) { // the same loop with the gradient of the ghost table (stated apart: the loop below is to compile to what it was)
          if (crossed) {
            float gc[3] = { 0.f, 0.f, 0.f }; // the isovalues a camera ray crosses here share one gradient, fetched once, ahead of the loop
            if (mode <= 0 && (crossed & ((1u << S.n_iso) - 1u))) vol_gradient_central<T>(V, Hl, c, G, f, gc);
            while (crossed && A < GVT_HIP_VOLUME_OPAQUE_A) {
              const int i = __ffs((int)crossed) - 1;
              crossed &= crossed - 1u;
              if (mode > 0) { // the shadow ray: opacity alone
                s_crossed++;
                A = A + (1.f - A) * S.alpha;
                continue;
              }
              n_crossed++;
              float4 col;
              float g[3];
              if (i < S.n_iso) {
                g[0] = gc[0]; g[1] = gc[1]; g[2] = gc[2];
                col = vol_lookup(V, S.iso[i]);
              } else {
                const float4 Q = S.plane[i - S.n_iso];
                g[0] = Q.x; g[1] = Q.y; g[2] = Q.z;
                col = vol_lookup(V, v);
              }
              if (have_T) surf_composite_shadowed(S, col, g, P + P_T * VOL_BLOCK, C, A);
              else surf_composite(S, col, g, C, A); // (no usable light: every T_j = 1)
            }
            if (A >= GVT_HIP_VOLUME_OPAQUE_A) { k++; done = true; break; } // the surface ends the ray: the sample itself adds nothing
          }
        } else
        if (crossed) {
          while (crossed && A < GVT_HIP_VOLUME_OPAQUE_A) { // (at most 16 bits are set: sides and prev stay below 2^16)
            const int i = __ffs((int)crossed) - 1;
            crossed &= crossed - 1u;
            if (mode > 0) { // the shadow ray: opacity alone
              s_crossed++;
              A = A + (1.f - A) * S.alpha;
              continue;
            }
            n_crossed++;
            float4 col;
            float g[3];
            if (i < S.n_iso) {
              vol_gradient(V, G, f, g);
              col = vol_lookup(V, S.iso[i]);
            } else {
              const float4 Q = S.plane[i - S.n_iso];
              g[0] = Q.x; g[1] = Q.y; g[2] = Q.z;
              col = vol_lookup(V, v);
            }
            if (have_T) surf_composite_shadowed(S, col, g, P + P_T * VOL_BLOCK, C, A);
            else surf_composite(S, col, g, C, A); // (no usable light: every T_j = 1)
          }
          if (A >= GVT_HIP_VOLUME_OPAQUE_A) { k++; done = true; break; } // the surface ends the ray: the sample itself adds nothing
        }
        if (mode > 0) vol_accumulate(V, v, C, A); // (shading NONE; the colour is dead)
        else n_shaded += vol_accumulate_lit_grids<T, CENTRAL, false>(V, V, S, Hl, H.usable, grid, nullptr, c, f, v, G, f, C, A);
        k++;
        if (A >= GVT_HIP_VOLUME_OPAQUE_A) { done = true; break; }
      }
      if (done) { // the ray leaves the brick (vol_write_back's t_min; its side mask and flag are prev): the next iteration decides where it goes
        if (k_last >= 0) {
          const float t_last = (float)k_last * V.dt;
          if (mode > 0) P[P_TMIN * VOL_BLOCK] = t_last;
          else q.p0[idx].w = t_last;
        }
        hop = true;
      }
    }
    s_rays += (unsigned)__popcll(ballot64(parked));
  }
  unsigned long long w_marched = n_marched, w_gathered = n_gathered, w_crossed = n_crossed, w_shaded = n_shaded;
  unsigned long long ws_marched = s_marched, ws_gathered = s_gathered, ws_crossed = s_crossed;
  for (int s = 32; s >= 1; s >>= 1) {
    w_marched += __shfl_xor(w_marched, s);
    w_gathered += __shfl_xor(w_gathered, s);
    w_crossed += __shfl_xor(w_crossed, s);
    w_shaded += __shfl_xor(w_shaded, s);
    ws_marched += __shfl_xor(ws_marched, s);
    ws_gathered += __shfl_xor(ws_gathered, s);
    ws_crossed += __shfl_xor(ws_crossed, s);
  }
  if (lane_id() == 0 && n_visits) {
    atomicAdd(&stats[0], w_marched);
    atomicAdd(&stats[1], w_gathered);
    atomicAdd(&stats[2], (unsigned long long)n_visits);
    atomicAdd(&stats[3], (unsigned long long)n_deposits);
    if (w_crossed) atomicAdd(&stats[4], w_crossed);
    if (w_shaded) atomicAdd(&stats[5], w_shaded);
    if (s_rays) {
      atomicAdd(&stats[6], (unsigned long long)s_rays);
      atomicAdd(&stats[7], (unsigned long long)s_visits);
      atomicAdd(&stats[8], ws_crossed);
      atomicAdd(&stats[9], ws_marched);
      atomicAdd(&stats[10], ws_gathered);
    }
  }
}

// KEEP IN STEP with k_volume_march_fused_shaded<T, CLIP, false, true>: that kernel restated, with the brick's planes loaded beside its
// record and vol_accumulate_lit_grids in vol_accumulate_lit's place
template <typename T, bool CLIP, bool CENTRAL>
__global__ __launch_bounds__(VOL_BLOCK) void k_volume_march_fused_fog_lean(VolDev U, LightDev S, unsigned usable, const FusedBrick *__restrict__ bricks,
                                                                           const FogBrick *__restrict__ grids, TopDev top, RayPlanes q, unsigned n, Mat4 minv,
                                                                           const float *__restrict__ clip_plane, unsigned n_clip, float *__restrict__ fb, unsigned n_pix,
                                                                           unsigned *__restrict__ work, unsigned long long *__restrict__ stats, FusedGhostArg<CENTRAL> HG) {
  bool active = false, exhausted = false;
  bool hop = false;  // the lane's ray is between two bricks: fresh from the list (brick < 0) or at the end of a visit
  unsigned idx = 0;
  VolDev V = U;      // the lane's brick: U with the record's fields
  const float *grid = nullptr; // ... and its planes
  GhostTable<CENTRAL> Hl = fused_ghost_init<CENTRAL>(HG); // (CENTRAL only) the lane's brick's ghost layers: the pointer changes wherever the brick does
  int brick = -1;
  float o[3] = { 0.f, 0.f, 0.f }, d[3] = { 0.f, 0.f, 0.f }, C[3] = { 0.f, 0.f, 0.f }, A = 0.f;
  int k = 0, k_hi = -1, k_last = -1;
  unsigned n_marched = 0, n_gathered = 0, n_shaded = 0; // (32 bits per lane: flushed between two bricks before they can wrap)
  unsigned n_visits = 0, n_deposits = 0; // (wave-uniform: counted from ballots where the wave is converged)
  for (;;) {
    const unsigned long long idle = ballot64(!active);
    if (idle && !exhausted && (__popcll(idle) >= VOL_REFILL_MIN || idle == ballot64(true))) {
      const unsigned slot = wave_alloc(work, !active);
      if (ballot64(!active && slot >= n)) exhausted = true; // (wave-uniform)
      if (!active && slot < n) { // a camera ray: no colour, no opacity, no flags, no brick yet
        idx = slot;
        active = true;
        hop = true;
        brick = -1;
        C[0] = 0.f; C[1] = 0.f; C[2] = 0.f;
        A = 0.f;
      }
    }
    if (!ballot64(active)) {
      if (exhausted) break;
      continue; // (every ray of the refill met no brick: the wave fetches again)
    }
    // ---- between two bricks: k_volume_march_fused's block (the shuffle's rule, evaluated by the lane)
    bool entered = false, deposited = false;
    if (active && hop) {
      hop = false;
      const float4 a = q.p0[idx], b = q.p1[idx];
      const int id = __float_as_int(q.p3[idx].x);
      const float wo[3] = { a.x, a.y, a.z }, wd[3] = { b.x, b.y, b.z };
      float t_clip;
      const bool clip = fused_clip<CLIP>(id, clip_plane, n_clip, t_clip);
      const float t_min = a.w; // (the end of a visit has stored it there, as vol_write_back does)
      if (n_marched >= 0x40000000u) {
        atomicAdd(&stats[0], (unsigned long long)n_marched); atomicAdd(&stats[1], (unsigned long long)n_gathered);
        atomicAdd(&stats[5], (unsigned long long)n_shaded);
        n_marched = 0; n_gathered = 0; n_shaded = 0;
      }
      int next = -1;
      if (A < GVT_HIP_VOLUME_OPAQUE_A) next = vol_next(top, brick, wo, wd, t_min, clip, t_clip);
      if (next >= 0) {
        const FusedBrick R = bricks[next];
        grid = grids[next].grid;
        if constexpr (CENTRAL) Hl.faces = HG.faces[next];
        V.vox = R.vox; V.mc = R.mc;
        V.nx = R.nx; V.ny = R.ny; V.nz = R.nz; V.ox = R.ox; V.oy = R.oy; V.oz = R.oz;
        for (int x = 0; x < 3; x++) { V.lo[x] = R.lo[x]; V.hi[x] = R.hi[x]; }
        vol_ray_range<CLIP>(V, minv, make_float4(a.x, a.y, a.z, t_min), make_float4(b.x, b.y, b.z, t_clip), clip ? GVT_HIP_RAY_CLIP : 0, o, d, k, k_hi);
        k_last = -1;
        entered = true;
      } else {
        if (brick >= 0) { // OPAQUE, or EXTERNAL: the ray leaves the volume (a camera ray that meets no brick deposits nothing)
          deposited = true;
          fused_deposit(fb, n_pix, id, C, A);
        }
        active = false;
        // (the lane's march state is dead now; saying so frees its registers for this block's temporaries)
        V.vox = nullptr; V.mc = nullptr;
        grid = nullptr;
        if constexpr (CENTRAL) Hl.faces = nullptr;
        V.nx = V.ny = V.nz = V.ox = V.oy = V.oz = 0;
        for (int x = 0; x < 3; x++) { o[x] = 0.f; d[x] = 0.f; }
        k = 0; k_hi = -1; k_last = -1;
      }
      brick = next;
    }
    n_visits += (unsigned)__popcll(ballot64(entered));
    n_deposits += (unsigned)__popcll(ballot64(deposited));
    // ---- the visit: k_volume_march_fused_shaded<T, CLIP, false, true>'s, step for step (KEEP IN STEP)
    if (active) {
      bool done = false;
      for (int s = 0; s < VOL_STEP; s++) {
        if (k > k_hi) { done = true; break; }
        int c[3];
        float f[3];
        if (!vol_cell(V, o, d, k, c, f)) {
          if (k_last >= 0) { done = true; break; } // a brick's samples along a line are contiguous: the rest belongs to others
          k++;
          continue;
        }
        k_last = k;
        n_marched++;
        const int bi = fused_macro_cell(V.nx, V.ny, c);
        if (V.skip && !V.mc[bi]) { // an empty macro cell adds +0 per sample
          if (A >= GVT_HIP_VOLUME_OPAQUE_A) { k++; done = true; break; } // the ray arrived opaque: this sample adds +0 and ends it, as any sample does
          const int kj = vol_jump_target(V, o, d, k, k_hi, c);
          if (kj > k) {
            n_marched += (unsigned)(kj - k);
            k_last = kj;
            k = kj;
          }
          k++;
          continue;
        }
        n_gathered++;
        VolCorners G;
        const float v = vol_gather<T>(V, c, f, G);
        n_shaded += vol_accumulate_lit_grids<T, CENTRAL, false>(V, V, S, Hl, usable, grid, nullptr, c, f, v, G, f, C, A);
        k++;
        if (A >= GVT_HIP_VOLUME_OPAQUE_A) { done = true; break; }
      }
      if (done) { // the ray leaves the brick (vol_write_back's t_min): the next iteration decides where it goes
        if (k_last >= 0) q.p0[idx].w = (float)k_last * V.dt;
        hop = true;
      }
    }
  }
  unsigned long long w_marched = n_marched, w_gathered = n_gathered, w_shaded = n_shaded;
  for (int s = 32; s >= 1; s >>= 1) {
    w_marched += __shfl_xor(w_marched, s);
    w_gathered += __shfl_xor(w_gathered, s);
    w_shaded += __shfl_xor(w_shaded, s);
  }
  if (lane_id() == 0 && n_visits) {
    atomicAdd(&stats[0], w_marched);
    atomicAdd(&stats[1], w_gathered);
    atomicAdd(&stats[2], (unsigned long long)n_visits);
    atomicAdd(&stats[3], (unsigned long long)n_deposits);
    if (w_shaded) atomicAdd(&stats[5], w_shaded);
  }
}
