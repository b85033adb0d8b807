// volume_fused_ao.inc -- the AO frame (gvt_hip_volume_frame_ao; the contract: include/gvt_hip.h, "ambient occlusion").  Included by
// volume.hip behind volume_fused_mesh.inc, whose kernels it restates, and volume_ao_grid.inc, which bakes the plane these kernels read.
//   k_volume_march_fused_ao<T, CLIP, LIT, CENTRAL, MESH>   k_volume_march_fused_mesh<T, CLIP, LIT, CENTRAL> with ONE more change: wherever the
//                                   ambient coefficient ka is used it is ka_s = ka * AOg, the AO plane interpolated at the sample's cell
//                                   (x, then y, then z, as Tg).  For the fog that is inside the shading branch (tc.w > 0), outside the
//                                   gradient's guard; for a crossing the camera ray reads AOg once when it re-runs its parked sample, and
//                                   keeps ka_s in a register across that sample's crossings (VOL_SHADOW_WORDS does not grow).
//   k_volume_march_fused_ao_lean<T, CLIP, CENTRAL, MESH>   the same change on k_volume_march_fused_mesh_lean, for a frame WITHOUT surfaces.
// KEEP IN STEP with k_volume_march_fused_mesh and k_volume_march_fused_mesh_lean (and through them with the shadowed, the fog and the
// shaded kernels): the kernels below are those kernels restated, for the reason they restate their parents -- the kernels that exist are
// to stay what they are, instruction for instruction.  The differences: the brick's three plane pointers travel in the parallel table
// (AoBrick); ka_s; and MESH, the base frame, is a template argument: without it the base is the fog-shadowed frame, occ is null and never
// read.  As a kernel argument tested per wave it halved the 96 instantiations and cost 2.5 to 4 % of the frame over the mesh-shadowed base
// and up to 2 % over the fog-shadowed one (profiles/volume_ao.txt, 6).
// The AO kernels run only in a frame with a usable light (else the call is the base frame), so a camera ray's crossing always parks and is
// always rendered with its T_j in hand.
// AO is read only where ka is used, so skipping stays exact and no counter moves; A never depends on AO; no ray is cast or skipped
// because of AO.

// a brick's planes: the light grid (float32; null without lit fog), the occluder grid (uint8; null without mesh) and the AO grid
// (float32, ONE plane of nx * ny * nz at the samples' own index)
struct AoBrick {
  const float *grid;
  const uint8_t *occ;
  const float *ao;
};

// AOg at cell c, fractions f: the AO plane at the cell's eight vertices, in Tg's nesting
__device__ __forceinline__ float ao_lerp(const VolDev &V, const float *__restrict__ ao, const int c[3], const float f[3]) {
  const size_t sy = (size_t)V.nx, sz = (size_t)V.nx * (size_t)V.ny;
  const float *p = ao + ((size_t)c[0] + sy * (size_t)c[1] + sz * (size_t)c[2]);
  const float c00 = lerp_(p[0], p[1], f[0]), c10 = lerp_(p[sy], p[sy + 1], f[0]);
  const float c01 = lerp_(p[sz], p[sz + 1], f[0]), c11 = lerp_(p[sz + sy], p[sz + sy + 1], f[0]);
  return lerp_(lerp_(c00, c10, f[1]), lerp_(c01, c11, f[1]), f[2]);
}

// surf_composite_shadowed with the sample's ambient coefficient ka_s in S.ka's place
__device__ inline void surf_composite_ao(const SurfDev &S, float ka_s, float4 c, const float g[3], const float *T, float C[3], float &A) {
  float rgb[3] = { c.x, c.y, c.z };
  float sum[3] = { 0.f, 0.f, 0.f };
  const float len = sqrtf((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]);
  if (len > 0.f) { // (false for NaN)
    const float n[3] = { g[0] / len, g[1] / len, g[2] / len };
    for (int j = 0; j < S.n_lights; j++) {
      const float ndl = fabsf((n[0] * S.ldir[j][0] + n[1] * S.ldir[j][1]) + n[2] * S.ldir[j][2]);
      const float ndl_s = ndl * T[j * VOL_BLOCK];
      for (int a = 0; a < 3; a++) sum[a] = sum[a] + S.lcol[j][a] * ndl_s;
    }
  }
  for (int a = 0; a < 3; a++) rgb[a] = rgb[a] * (ka_s + S.kd * sum[a]);
  const float f = (1.f - A) * S.alpha;
  C[0] = C[0] + f * rgb[0]; C[1] = C[1] + f * rgb[1]; C[2] = C[2] + f * rgb[2];
  A = A + f;
}

// vol_accumulate_lit_grids (outside an AMR visit) with ka_s = ka * AOg: AOg is read inside the branch that shades, outside the gradient's
// guard (a NaN or zero gradient: rgb * ka_s).  MESH: the occluder grid multiplies Tg
template <typename T, bool CENTRAL, bool MESH, typename LT> // (LT: SurfDev or LightDev; CENTRAL: the gradient is vol_gradient_central's, from Hg)
__device__ __forceinline__ unsigned vol_accumulate_lit_ao(const VolDev &V, const LT &L, const GhostTable<CENTRAL> &Hg, unsigned usable, const AoBrick &B,
                                                          const int c[3], const float f[3], float v, const VolCorners &G, float C[3], float &A) {
  const float4 tc = vol_lookup(V, v);
  float rgb[3] = { tc.x, tc.y, tc.z };
  const bool shaded = tc.w > 0.f; // (false for NaN)
  if (shaded) {
    const float ka_s = L.ka * ao_lerp(V, B.ao, c, f);
    float g[3], sum[3] = { 0.f, 0.f, 0.f };
    if constexpr (CENTRAL) vol_gradient_central<T>(V, Hg, c, G, f, g);
    else vol_gradient(V, G, f, g);
    const float len = sqrtf((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]);
    if (len > 0.f && len < INFINITY) { // (false for NaN)
      const float n[3] = { g[0] / len, g[1] / len, g[2] / len };
      const size_t sy = (size_t)V.nx, sz = (size_t)V.nx * (size_t)V.ny, plane = sz * (size_t)V.nz;
      const float *p = B.grid + ((size_t)c[0] + sy * (size_t)c[1] + sz * (size_t)c[2]);
      int l = 0;
      for (int j = 0; j < L.n_lights; j++) {
        const float ndl = fabsf((n[0] * L.ldir[j][0] + n[1] * L.ldir[j][1]) + n[2] * L.ldir[j][2]);
        float Ts = 1.f;
        if ((usable >> j) & 1u) { // (wave-uniform)
          const float c00 = lerp_(p[0], p[1], f[0]), c10 = lerp_(p[sy], p[sy + 1], f[0]);
          const float c01 = lerp_(p[sz], p[sz + 1], f[0]), c11 = lerp_(p[sz + sy], p[sz + sy + 1], f[0]);
          Ts = lerp_(lerp_(c00, c10, f[1]), lerp_(c01, c11, f[1]), f[2]);
          if constexpr (MESH) Ts = Ts * occluder_lerp(V, B.occ, l, c, f);
          p += plane;
          l++;
        }
        const float ndl_s = ndl * Ts;
        for (int a = 0; a < 3; a++) sum[a] = sum[a] + L.lcol[j][a] * ndl_s;
      }
    }
    for (int a = 0; a < 3; a++) rgb[a] = rgb[a] * (ka_s + L.kd * sum[a]);
  }
  const float fr = (1.f - A) * tc.w;
  C[0] = C[0] + fr * rgb[0]; C[1] = C[1] + fr * rgb[1]; C[2] = C[2] + fr * rgb[2];
  A = A + fr;
  return shaded ? 1u : 0u;
}

template <typename T, bool CLIP, bool LIT, bool CENTRAL, bool MESH>
__global__ __launch_bounds__(VOL_BLOCK) void k_volume_march_fused_ao(VolDev U, SurfDev S, ShadowDev H, const FusedBrick *__restrict__ bricks, const AoBrick *__restrict__ grids,
                                                                     TopDev top, RayPlanes q, unsigned n, Mat4 minv, const float *__restrict__ clip_plane, unsigned n_clip,
                                                                     float *__restrict__ fb, unsigned n_pix, unsigned *__restrict__ work,
                                                                     unsigned long long *__restrict__ stats, FusedGhostArg<CENTRAL> HG) {
  __shared__ float park[VOL_SHADOW_WORDS][VOL_BLOCK];
  float *const P = &park[0][threadIdx.x]; // the lane's column: word w at P[w * VOL_BLOCK]
  enum { P_K = 0, P_BRICK = 1, P_PREV = 2, P_C = 3, P_A = 6, P_TMIN = 7, P_T = 8 };
  bool active = false, exhausted = false;
  bool hop = false;
  unsigned idx = 0;
  VolDev V = U;
  AoBrick grid{ nullptr, nullptr, nullptr }; // the lane's brick's planes: the light grid's (LIT only), the occluder grid's (MESH only), the AO grid's
  GhostTable<CENTRAL> Hl = fused_ghost_init<CENTRAL>(HG); // (CENTRAL only) the lane's brick's ghost layers: the pointer changes wherever the brick does
  int brick = -1;
  int mode = 0;
  float o[3] = { 0.f, 0.f, 0.f }, d[3] = { 0.f, 0.f, 0.f }, C[3] = { 0.f, 0.f, 0.f }, A = 0.f;
  int k = 0, k_hi = -1, k_last = -1, k_carry = -1, prev = -1;
  // (32 bits per lane, flushed between two bricks before they can wrap, as in the shaded kernel; the shadow rays' own beside them)
  unsigned n_marched = 0, n_gathered = 0, n_crossed = 0;
  unsigned n_shaded = 0; // (LIT only)
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
    // ---- between two bricks: k_volume_march_fused_mesh's block, for the camera ray of the list or for the shadow ray it casts
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
        if constexpr (LIT) atomicAdd(&stats[5], (unsigned long long)n_shaded);
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
        grid = grids[next];
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
        grid = AoBrick{ nullptr, nullptr, nullptr };
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
    // ---- the visit: k_volume_march_fused_mesh<T, CLIP, LIT>'s, step for step (KEEP IN STEP), for camera and shadow rays alike
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
        float ka_s = S.ka; // the sample's ambient coefficient: ka * AOg, found once for all its crossings
        if (have_T && crossed) {
          ka_s = S.ka * ao_lerp(V, grid.ao, c, f);
          if constexpr (MESH) // the mesh's part of this sample's light: T_j * Og in the lane's T words (an unusable light: T_j = 1 stays)
            for (int j = 0, l = 0; j < S.n_lights; j++)
              if ((H.usable >> j) & 1u) { // (wave-uniform)
                P[(P_T + j) * VOL_BLOCK] = P[(P_T + j) * VOL_BLOCK] * occluder_lerp(V, grid.occ, l, c, f);
                l++;
              }
        }
        if (crossed) {
          float gc[3] = { 0.f, 0.f, 0.f }; // (CENTRAL) the isovalues a camera ray crosses here share one gradient, fetched once, ahead of the loop
          if constexpr (CENTRAL)
            if (mode <= 0 && (crossed & ((1u << S.n_iso) - 1u))) vol_gradient_central<T>(V, Hl, c, G, f, gc);
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
              if constexpr (CENTRAL) { g[0] = gc[0]; g[1] = gc[1]; g[2] = gc[2]; }
              else vol_gradient(V, G, f, g);
              col = vol_lookup(V, S.iso[i]);
            } else {
              const float4 Q = S.plane[i - S.n_iso];
              g[0] = Q.x; g[1] = Q.y; g[2] = Q.z;
              col = vol_lookup(V, v);
            }
            if (have_T) surf_composite_ao(S, ka_s, col, g, P + P_T * VOL_BLOCK, C, A);
            else surf_composite(S, col, g, C, A); // (no usable light: not reached in this kernel)
          }
          if (A >= GVT_HIP_VOLUME_OPAQUE_A) { k++; done = true; break; } // the surface ends the ray: the sample itself adds nothing
        }
        if constexpr (LIT) {
          if (mode > 0) vol_accumulate(V, v, C, A); // (shading NONE; the colour is dead)
          else n_shaded += vol_accumulate_lit_ao<T, CENTRAL, MESH>(V, S, Hl, H.usable, grid, c, f, v, G, C, A);
        } else {
          vol_accumulate(V, v, C, A);
        }
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
    if constexpr (LIT) w_shaded += __shfl_xor(w_shaded, s);
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
    if constexpr (LIT)
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

// KEEP IN STEP with k_volume_march_fused_mesh_lean (and through it with k_volume_march_fused_fog_lean and
// k_volume_march_fused_shaded<T, CLIP, false, true>): that kernel restated, with the brick's three plane pointers loaded beside its record
// and vol_accumulate_lit_ao in vol_accumulate_lit_grids' place
template <typename T, bool CLIP, bool CENTRAL, bool MESH>
__global__ __launch_bounds__(VOL_BLOCK) void k_volume_march_fused_ao_lean(VolDev U, LightDev S, unsigned usable, const FusedBrick *__restrict__ bricks,
                                                                          const AoBrick *__restrict__ grids, TopDev top, RayPlanes q, unsigned n, Mat4 minv,
                                                                          const float *__restrict__ clip_plane, unsigned n_clip, float *__restrict__ fb, unsigned n_pix,
                                                                          unsigned *__restrict__ work, unsigned long long *__restrict__ stats, FusedGhostArg<CENTRAL> HG) {
  bool active = false, exhausted = false;
  bool hop = false;  // the lane's ray is between two bricks: fresh from the list (brick < 0) or at the end of a visit
  unsigned idx = 0;
  VolDev V = U;      // the lane's brick: U with the record's fields
  AoBrick grid{ nullptr, nullptr, nullptr }; // ... and its planes
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
        grid = grids[next];
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
        grid = AoBrick{ nullptr, nullptr, nullptr };
        if constexpr (CENTRAL) Hl.faces = nullptr;
        V.nx = V.ny = V.nz = V.ox = V.oy = V.oz = 0;
        for (int x = 0; x < 3; x++) { o[x] = 0.f; d[x] = 0.f; }
        k = 0; k_hi = -1; k_last = -1;
      }
      brick = next;
    }
    n_visits += (unsigned)__popcll(ballot64(entered));
    n_deposits += (unsigned)__popcll(ballot64(deposited));
    // ---- the visit: k_volume_march_fused_mesh_lean's, step for step (KEEP IN STEP)
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
        n_shaded += vol_accumulate_lit_ao<T, CENTRAL, MESH>(V, S, Hl, usable, grid, c, f, v, G, C, A);
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
