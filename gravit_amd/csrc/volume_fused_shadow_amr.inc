// volume_fused_shadow_amr.inc -- the shadowed frames and the light grid's bake over bricks with AMR subgrids (GVT_HIP_VOLUME_ALLOW_AMR in
// the flags of gvt_hip_volume_frame_shadowed / _fog_shadowed / _mesh_shadowed and gvt_hip_volume_light_grid_bake; the contract:
// include/gvt_hip.h, "shadows on AMR bricks").  Included by volume.hip behind volume_fused_mesh.inc: it uses ShadowDev, the counters, the
// parked words and surf_composite_shadowed (volume_fused_shadow.inc), LightGridBrick (volume_light_grid.inc), MeshBrick and occluder_lerp
// (volume_fused_mesh.inc) and the AMR table and descent (volume_amr.inc, volume_fused_amr.inc).
//   k_volume_march_fused_shadow_amr<CLIP, LIT>   k_volume_march_fused_shadow<float, CLIP, LIT, false>'s structure -- "shadow ray" is a mode
//                                   of the lane -- around k_volume_march_fused_shaded_amr<CLIP, true, LIT>'s visit, under its null-table rule
//   k_volume_march_fused_fog_amr<CLIP>           k_volume_march_fused_fog<float, CLIP, false>'s one change on that: a lit fog sample's n . l
//                                   times Tg, interpolated from the light grid at the sample's LEVEL-0 cell with its level-0 fractions
//   k_volume_march_fused_mesh_amr<CLIP, LIT>     k_volume_march_fused_mesh<float, CLIP, LIT, false>'s one more: Og, read the same way
//   k_volume_march_fused_fog_lean_amr<CLIP>, k_volume_march_fused_mesh_lean_amr<CLIP>   the frames without surfaces:
//                                   k_volume_march_fused_fog_lean's / _mesh_lean's change on k_volume_march_fused_shaded_amr<CLIP, false, true>
//   k_volume_bake_light_amr         k_volume_bake_light<float>'s ownership walk with the AMR visit on bricks that have subgrids
// The three surface-capable kernels are ONE device body (volume_shadow_amr_body<CLIP, LIT, GRIDS>; GRIDS: 0 no planes, 1 the light grid,
// 2 the occluder grid and -- LIT -- the light grid), the two lean ones another (volume_lean_amr_body<CLIP, MESH>), as volume_amr.inc's
// four kernels are one body: what differs between them is what differs between their non-AMR siblings, stated once.
// Float32 and CELL gradients only, as subgrids are.  The frame may mix bricks with and without subgrids, and so may one shadow ray.
// KEEP IN STEP with BOTH parents: the "between two bricks" block, the parking and the resume are k_volume_march_fused_shadow's (_fog's,
// _mesh's), word for word; the per-sample steps -- the skip decision from the per-cell word (built from the merged ranges on a brick with
// subgrids), amr_descend between it and the gather, amr_gather, amr_corners, one gradient at amr_fine_spacing for the isovalues a sample
// crosses, the lit accumulation at amr_fine_spacing -- are k_volume_march_fused_shaded_amr's.  Restated, not hoisted: every kernel that
// existed before this file stays what it was, instruction for instruction (profiles/volume_shadow_amr.txt, 2).
//
// The lane carries AmrDev Am beside V.  It is loaded with EVERY record: for a shadow ray's brick and, on resume, for the parked camera
// ray's brick again (where the CENTRAL kernels reload the ghost pointer), and cleared where the lane goes idle.  Nothing new is parked in
// LDS: the brick index already is.  A shadow ray takes opacity alone and reads no gradient, so amr_corners runs for mode <= 0 only.
// T_j is therefore the opacity the shadow ray would deposit as a camera ray of gvt_hip_volume_frame_fused_amr over the same bricks with
// the same surfaces and shading NONE.  Refined samples are not counted: gvt_hip_volume_shadow_stats has no field for them.
//
// The planes of a light or occluder grid stay at the brick's own level-0 vertices.  A sample reads them at its level-0 cell c with the
// fractions f0 it had BEFORE amr_descend overwrote f (kept in three registers across the descent; vol_cell is not run again); the
// gradient that shades it is the final cell's.  On a brick without subgrids f0 == f and amr_fine_spacing multiplies by 1.0f: the bits are
// the non-AMR kernels'.
//
// Termination: k_volume_march_fused_shadow's argument; the descent is bounded by the levels of a brick and adds no state to a ray.

template <bool CLIP, bool LIT, int GRIDS>
__device__ __forceinline__ void volume_shadow_amr_body(const VolDev &U, const SurfDev &S, const ShadowDev &H, const FusedBrick *__restrict__ bricks,
                                                       const AmrDev *__restrict__ amr, const MeshBrick *__restrict__ grids, const TopDev &top, RayPlanes q, unsigned n,
                                                       const Mat4 &minv, const float *__restrict__ clip_plane, unsigned n_clip, float *__restrict__ fb, unsigned n_pix,
                                                       unsigned *__restrict__ work, unsigned long long *__restrict__ stats) {
  static_assert(GRIDS == 0 || GRIDS == 2 || LIT, "the fog-shadowed kernel has lit fog");
  __shared__ float park[VOL_SHADOW_WORDS][VOL_BLOCK];
  float *const P = &park[0][threadIdx.x]; // the lane's column: word w at P[w * VOL_BLOCK]
  enum { P_K = 0, P_BRICK = 1, P_PREV = 2, P_C = 3, P_A = 6, P_TMIN = 7, P_T = 8 };
  bool active = false, exhausted = false;
  bool hop = false;
  unsigned idx = 0;
  VolDev V = U;
  AmrDev Am{ nullptr, nullptr, nullptr, nullptr }; // the lane's brick's AMR tables: all null on a brick without subgrids; they change wherever the brick does
  MeshBrick grid{ nullptr, nullptr }; // (GRIDS only) the lane's brick's planes: the light grid's (LIT only) and the occluder grid's (GRIDS == 2 only)
  int brick = -1;
  int mode = 0;
  float o[3] = { 0.f, 0.f, 0.f }, d[3] = { 0.f, 0.f, 0.f }, C[3] = { 0.f, 0.f, 0.f }, A = 0.f;
  int k = 0, k_hi = -1, k_last = -1, k_carry = -1, prev = -1;
  // (32 bits per lane, flushed between two bricks before they can wrap, as in the shadowed kernel; the shadow rays' own beside them)
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
        Am = amr[next]; // (a shadow ray's brick, or -- resume -- the parked camera ray's again)
        if constexpr (GRIDS != 0) grid = grids[next];
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
        Am = AmrDev{ nullptr, nullptr, nullptr, nullptr };
        if constexpr (GRIDS != 0) grid = MeshBrick{ nullptr, nullptr };
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
    // ---- the visit: k_volume_march_fused_shaded_amr<CLIP, true, LIT>'s, step for step (KEEP IN STEP), for camera and shadow rays alike,
    // with k_volume_march_fused_shadow's parking at a rendered crossing
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
        // the cell word is built from the merged ranges: no sample of any level in the macro cell changes an isovalue side
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
        uint2 word = make_uint2(0u, 0u);
        if (Am.mc) word = Am.mc[bi]; // (the descent's entry: read for a gathered sample only)
        if (mode > 0) s_gathered++; else n_gathered++;
        const float *gp;
        size_t sy, sz;
        int log2_r;
        const float f0[3] = { f[0], f[1], f[2] }; // the level-0 fractions: the planes of a light or occluder grid are read at cell c with these
        amr_descend(V, Am, word, c, f, gp, sy, sz, log2_r);
        const float v = amr_gather(gp, sy, sz, f);
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
        VolCorners G{};
        if (mode <= 0) amr_corners(gp, sy, sz, G); // (a shadow ray reads no gradient)
        if constexpr (GRIDS == 2)
          if (have_T && crossed) // the mesh's part of this sample's light: T_j * Og in the lane's T words, once for all its crossings (an unusable light: T_j = 1 stays)
            for (int j = 0, l = 0; j < S.n_lights; j++)
              if ((H.usable >> j) & 1u) { // (wave-uniform)
                P[(P_T + j) * VOL_BLOCK] = P[(P_T + j) * VOL_BLOCK] * occluder_lerp(V, grid.occ, l, c, f0);
                l++;
              }
        if (crossed) {
          float gc[3] = { 0.f, 0.f, 0.f }; // the isovalues a camera ray crosses here share one gradient: the final cell's
          if (mode <= 0 && (crossed & ((1u << S.n_iso) - 1u))) vol_gradient(amr_fine_spacing(V, log2_r), G, f, gc);
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
        if constexpr (LIT) {
          if (mode > 0) vol_accumulate(V, v, C, A); // (shading NONE; the colour is dead)
          else if constexpr (GRIDS != 0) n_shaded += vol_accumulate_lit_grids<float, false, GRIDS == 2>(amr_fine_spacing(V, log2_r), V, S, NoGhost{}, H.usable, grid.grid, grid.occ, c, f0, v, G, f, C, A);
          else n_shaded += vol_accumulate_lit<float, false>(amr_fine_spacing(V, log2_r), S, NoGhost{}, c, v, G, f, C, A);
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

template <bool CLIP, bool LIT>
__global__ __launch_bounds__(VOL_BLOCK) void k_volume_march_fused_shadow_amr(VolDev U, SurfDev S, ShadowDev H, const FusedBrick *__restrict__ bricks,
                                                                             const AmrDev *__restrict__ amr, TopDev top, RayPlanes q, unsigned n, Mat4 minv,
                                                                             const float *__restrict__ clip_plane, unsigned n_clip, float *__restrict__ fb,
                                                                             unsigned n_pix, unsigned *__restrict__ work, unsigned long long *__restrict__ stats) {
  volume_shadow_amr_body<CLIP, LIT, 0>(U, S, H, bricks, amr, nullptr, top, q, n, minv, clip_plane, n_clip, fb, n_pix, work, stats);
}
template <bool CLIP>
__global__ __launch_bounds__(VOL_BLOCK) void k_volume_march_fused_fog_amr(VolDev U, SurfDev S, ShadowDev H, const FusedBrick *__restrict__ bricks,
                                                                          const AmrDev *__restrict__ amr, const MeshBrick *__restrict__ grids, TopDev top, RayPlanes q,
                                                                          unsigned n, Mat4 minv, const float *__restrict__ clip_plane, unsigned n_clip,
                                                                          float *__restrict__ fb, unsigned n_pix, unsigned *__restrict__ work,
                                                                          unsigned long long *__restrict__ stats) {
  volume_shadow_amr_body<CLIP, true, 1>(U, S, H, bricks, amr, grids, top, q, n, minv, clip_plane, n_clip, fb, n_pix, work, stats);
}
template <bool CLIP, bool LIT>
__global__ __launch_bounds__(VOL_BLOCK) void k_volume_march_fused_mesh_amr(VolDev U, SurfDev S, ShadowDev H, const FusedBrick *__restrict__ bricks,
                                                                           const AmrDev *__restrict__ amr, const MeshBrick *__restrict__ grids, TopDev top, RayPlanes q,
                                                                           unsigned n, Mat4 minv, const float *__restrict__ clip_plane, unsigned n_clip,
                                                                           float *__restrict__ fb, unsigned n_pix, unsigned *__restrict__ work,
                                                                           unsigned long long *__restrict__ stats) {
  volume_shadow_amr_body<CLIP, LIT, 2>(U, S, H, bricks, amr, grids, top, q, n, minv, clip_plane, n_clip, fb, n_pix, work, stats);
}

// KEEP IN STEP with k_volume_march_fused_shaded_amr<CLIP, false, true> (the visit, the null-table rule: the skip bit of a brick with
// subgrids is bit 31 of its AMR cell word, of a brick without its skip byte) and with k_volume_march_fused_fog_lean / _mesh_lean (the
// planes loaded beside the record): that kernel restated, with vol_accumulate_lit_grids (volume_fused_fog.inc) in vol_accumulate_lit's place
template <bool CLIP, bool MESH>
__device__ __forceinline__ void volume_lean_amr_body(const VolDev &U, const LightDev &S, unsigned usable, const FusedBrick *__restrict__ bricks, const AmrDev *__restrict__ amr,
                                                     const MeshBrick *__restrict__ grids, const TopDev &top, RayPlanes q, unsigned n, const Mat4 &minv,
                                                     const float *__restrict__ clip_plane, unsigned n_clip, float *__restrict__ fb, unsigned n_pix,
                                                     unsigned *__restrict__ work, unsigned long long *__restrict__ stats) {
  bool active = false, exhausted = false;
  bool hop = false;  // the lane's ray is between two bricks: fresh from the list (brick < 0) or at the end of a visit
  unsigned idx = 0;
  VolDev V = U;      // the lane's brick: U with the record's fields
  AmrDev Am{ nullptr, nullptr, nullptr, nullptr }; // ... its AMR tables: all null on a brick without subgrids
  MeshBrick grid{ nullptr, nullptr }; // ... and its planes (the occluder grid's: MESH only)
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
        Am = amr[next];
        grid = grids[next];
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
        Am = AmrDev{ nullptr, nullptr, nullptr, nullptr };
        grid = MeshBrick{ nullptr, nullptr };
        V.nx = V.ny = V.nz = V.ox = V.oy = V.oz = 0;
        for (int x = 0; x < 3; x++) { o[x] = 0.f; d[x] = 0.f; }
        k = 0; k_hi = -1; k_last = -1;
      }
      brick = next;
    }
    n_visits += (unsigned)__popcll(ballot64(entered));
    n_deposits += (unsigned)__popcll(ballot64(deposited));
    // ---- the visit: k_volume_march_fused_shaded_amr<CLIP, false, true>'s, step for step (KEEP IN STEP), under its null-table rule
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
        uint2 word = make_uint2(0u, 0u);
        bool skip;
        if (Am.mc) { // empty by the union of every level's vertices in the macro cell: +0 per sample, whatever grid it is in
          word = Am.mc[bi];
          skip = V.skip && !(word.y >> 31);
        } else {
          skip = V.skip && !V.mc[bi];
        }
        if (skip) {
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
        const float *gp;
        size_t sy, sz;
        int log2_r;
        const float f0[3] = { f[0], f[1], f[2] }; // the level-0 fractions: the planes are read at cell c with these
        amr_descend(V, Am, word, c, f, gp, sy, sz, log2_r);
        const float v = amr_gather(gp, sy, sz, f);
        VolCorners G;
        amr_corners(gp, sy, sz, G);
        n_shaded += vol_accumulate_lit_grids<float, false, MESH>(amr_fine_spacing(V, log2_r), V, S, NoGhost{}, usable, grid.grid, grid.occ, c, f0, v, G, f, C, A);
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

template <bool CLIP>
__global__ __launch_bounds__(VOL_BLOCK) void k_volume_march_fused_fog_lean_amr(VolDev U, LightDev S, unsigned usable, const FusedBrick *__restrict__ bricks,
                                                                               const AmrDev *__restrict__ amr, const MeshBrick *__restrict__ grids, TopDev top, RayPlanes q,
                                                                               unsigned n, Mat4 minv, const float *__restrict__ clip_plane, unsigned n_clip,
                                                                               float *__restrict__ fb, unsigned n_pix, unsigned *__restrict__ work,
                                                                               unsigned long long *__restrict__ stats) {
  volume_lean_amr_body<CLIP, false>(U, S, usable, bricks, amr, grids, top, q, n, minv, clip_plane, n_clip, fb, n_pix, work, stats);
}
template <bool CLIP>
__global__ __launch_bounds__(VOL_BLOCK) void k_volume_march_fused_mesh_lean_amr(VolDev U, LightDev S, unsigned usable, const FusedBrick *__restrict__ bricks,
                                                                                const AmrDev *__restrict__ amr, const MeshBrick *__restrict__ grids, TopDev top, RayPlanes q,
                                                                                unsigned n, Mat4 minv, const float *__restrict__ clip_plane, unsigned n_clip,
                                                                                float *__restrict__ fb, unsigned n_pix, unsigned *__restrict__ work,
                                                                                unsigned long long *__restrict__ stats) {
  volume_lean_amr_body<CLIP, true>(U, S, usable, bricks, amr, grids, top, q, n, minv, clip_plane, n_clip, fb, n_pix, work, stats);
}

// KEEP IN STEP with k_volume_bake_light<float> (the work items, the ownership walk, the end of a ray) and with the shadow-ray mode of
// volume_shadow_amr_body above (the visit: opacity alone, the colour dead).  The rays start at level-0 vertices and are marched over the
// whole grid with all its subgrids as one brick: Am is loaded wherever the ownership walk changes the lane's brick, and is null at a
// fresh work item, as V.nx = 0 is.  The skip decision reads the brick's per-cell word, which is built from the merged ranges.
__global__ __launch_bounds__(VOL_BLOCK) void k_volume_bake_light_amr(VolDev U, SurfDev S, ShadowDev H, const FusedBrick *__restrict__ bricks, const AmrDev *__restrict__ amr,
                                                                     const LightGridBrick *__restrict__ parts, unsigned n_bricks, unsigned n, Mat4 m, Mat4 minv,
                                                                     unsigned *__restrict__ work, unsigned long long *__restrict__ stats) {
  // U: the WHOLE grid as one brick (offset 0, counts = the global counts, lo / hi the global vertex box); V: the lane's brick
  bool active = false, exhausted = false;
  VolDev V = U;
  V.nx = 0; V.ny = 0; V.nz = 0; // (owns nothing: the first sample looks its brick up)
  AmrDev Am{ nullptr, nullptr, nullptr, nullptr };
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
        Am = AmrDev{ nullptr, nullptr, nullptr, nullptr };
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
          Am = amr[b];
          V.vox = R.vox; V.mc = R.mc;
          V.nx = R.nx; V.ny = R.ny; V.nz = R.nz; V.ox = R.ox; V.oy = R.oy; V.oz = R.oz;
          if (!vol_cell(V, o, d, k, c, f)) { done = true; break; } // (the same g, the same test: not reached)
        }
        seen = true;
        n_marched++;
        const int bi = fused_macro_cell(V.nx, V.ny, c);
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
        uint2 word = make_uint2(0u, 0u);
        if (Am.mc) word = Am.mc[bi]; // (the descent's entry: read for a gathered sample only)
        n_gathered++;
        const float *gp;
        size_t sy, sz;
        int log2_r;
        amr_descend(V, Am, word, c, f, gp, sy, sz, log2_r);
        const float v = amr_gather(gp, sy, sz, f);
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
