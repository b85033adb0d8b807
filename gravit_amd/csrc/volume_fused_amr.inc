// volume_fused_amr.inc -- the fused frame for bricks with AMR subgrids (gvt_hip_volume_frame_fused_amr, GVT_HIP_FUSED_AMR).  Included by
// volume.hip behind volume_fused_shaded.inc (FusedBrick, the counters, fused_clip) and volume_amr.inc (AmrDev, the descent).
//   k_volume_march_fused_amr<CLIP>                    k_volume_march_fused<float, CLIP>'s structure around the plain AMR visit
//   k_volume_march_fused_shaded_amr<CLIP, SURF, LIT>  k_volume_march_fused_shaded<float, CLIP, SURF, LIT, false>'s around the shaded AMR visit
// Float32 and CELL gradients only, as subgrids are.  The frame may MIX bricks with and without subgrids: that is the shape of refined
// simulation output (many bricks, refinement in a few of them).
// KEEP IN STEP with volume_march_amr_body (volume_amr.inc) and, through it, volume_march_body (volume.hip): the visit below restates the
// per-sample steps -- the skip decision, amr_descend between it and the gather, amr_gather / amr_corners, the crossing loop and the lit
// accumulation at amr_fine_spacing -- through the same device functions, in the same order.  The "between two bricks" block is
// k_volume_march_fused's / _fused_shaded's.  Restated, not hoisted: every kernel that existed before this file stays what it was,
// instruction for instruction (profiles/volume_fused_amr.txt, 2).  tests/test_gpu_volume_fused_amr.py compares the framebuffers with the
// loop's in every bit.
//
// Per brick, beside the 64-byte record: the brick's four AMR tables (AmrDev) as a second device table indexed like the records, filled
// by the host at every call from the volumes as they are then (gvt_hip_volume_set_subgrids frees and replaces them) and loaded where the
// record is loaded, as the ghost table is for CENTRAL.  The entry of a brick without subgrids is all null, and the NULL-TABLE RULE is:
//   - the skip bit of such a brick comes from where the fused kernels read it today (the skip byte; SURF: the per-cell word, which the
//     record's mc slot carries for every brick, with or without subgrids -- S.cells of the loop's march is the same d_cells);
//   - its cell word is (0, 0): no level-1 subgrid, so amr_descend's loop does not run and hands back the brick's own grid (base = vox,
//     strides nx and nx * ny, log2_r = 0).  amr_gather on that is vol_gather<float> term for term, amr_corners reads the same eight
//     addresses, and amr_fine_spacing(V, 0) multiplies the spacing by 1.0f: the bits are the plain / shaded fused visit's.
// So nothing is allocated or built per macro cell at a call, and a lane pays one null test per sample instead of a second visit's code.
// The descent adds no state to a ray: between two visits the lane carries what the fused kernels carry.
#define VOL_FUSED_AMR_STATS 7 // VOL_FUSED_SHADED_STATS' six words, then the gathered samples whose final grid was a subgrid
#define VOL_FUSED_AMR_REFINED 6

template <bool CLIP>
__global__ __launch_bounds__(VOL_BLOCK) void k_volume_march_fused_amr(VolDev U, const FusedBrick *__restrict__ bricks, const AmrDev *__restrict__ amr, TopDev top, RayPlanes q,
                                                                      unsigned n, Mat4 minv, const float *__restrict__ clip_plane, unsigned n_clip, float *__restrict__ fb,
                                                                      unsigned n_pix, unsigned *__restrict__ work, unsigned long long *__restrict__ stats) {
  bool active = false, exhausted = false;
  bool hop = false;  // the lane's ray is between two bricks: fresh from the list (brick < 0) or at the end of a visit
  unsigned idx = 0;
  VolDev V = U;      // the lane's brick: U with the record's fields
  AmrDev Am{ nullptr, nullptr, nullptr, nullptr }; // ... and its AMR tables: all null on a brick without subgrids
  int brick = -1;
  float o[3] = { 0.f, 0.f, 0.f }, d[3] = { 0.f, 0.f, 0.f }, C[3] = { 0.f, 0.f, 0.f }, A = 0.f;
  int k = 0, k_hi = -1, k_last = -1;
  unsigned n_marched = 0, n_gathered = 0, n_refined = 0; // (32 bits per lane: flushed between two bricks long before they can wrap, a visit adds at most 2^23)
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
        atomicAdd(&stats[VOL_FUSED_AMR_REFINED], (unsigned long long)n_refined);
        n_marched = 0; n_gathered = 0; n_refined = 0;
      }
      int next = -1;
      if (A < GVT_HIP_VOLUME_OPAQUE_A) next = vol_next(top, brick, wo, wd, t_min, clip, t_clip);
      if (next >= 0) {
        const FusedBrick R = bricks[next];
        Am = amr[next];
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
        V.nx = V.ny = V.nz = V.ox = V.oy = V.oz = 0;
        for (int x = 0; x < 3; x++) { o[x] = 0.f; d[x] = 0.f; }
        k = 0; k_hi = -1; k_last = -1;
      }
      brick = next;
    }
    n_visits += (unsigned)__popcll(ballot64(entered));
    n_deposits += (unsigned)__popcll(ballot64(deposited));
    // ---- the visit: volume_march_amr_body<false, false, CLIP>'s, step for step (KEEP IN STEP; `seen` there is k_last >= 0 here; nbx and
    // nby are recomputed: fused_macro_cell), under the null-table rule above
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
        const float *p;
        size_t sy, sz;
        int log2_r;
        if (amr_descend(V, Am, word, c, f, p, sy, sz, log2_r)) n_refined++;
        const float v = amr_gather(p, sy, sz, f);
        vol_accumulate(V, v, C, A);
        k++;
        if (A >= GVT_HIP_VOLUME_OPAQUE_A) { done = true; break; }
      }
      if (done) { // the ray leaves the brick (vol_write_back's t_min): the next iteration decides where it goes
        if (k_last >= 0) q.p0[idx].w = (float)k_last * V.dt;
        hop = true;
      }
    }
  }
  unsigned long long w_marched = n_marched, w_gathered = n_gathered, w_refined = n_refined;
  for (int s = 32; s >= 1; s >>= 1) {
    w_marched += __shfl_xor(w_marched, s);
    w_gathered += __shfl_xor(w_gathered, s);
    w_refined += __shfl_xor(w_refined, s);
  }
  if (lane_id() == 0 && n_visits) {
    atomicAdd(&stats[0], w_marched);
    atomicAdd(&stats[1], w_gathered);
    atomicAdd(&stats[2], (unsigned long long)n_visits);
    atomicAdd(&stats[3], (unsigned long long)n_deposits);
    if (w_refined) atomicAdd(&stats[VOL_FUSED_AMR_REFINED], w_refined);
  }
}

// What a ray carries between two visits is k_volume_march_fused_shaded's: prev, the side mask of its last owned sample (-1: none), and
// k_carry on entering a brick.  SURF: the record's mc slot carries d_cells for every brick (the per-cell words, built from the merged
// ranges on a brick with subgrids); the AMR cell word is read from the second table, and only for a sample that is gathered.
template <bool CLIP, bool SURF, bool LIT>
__global__ __launch_bounds__(VOL_BLOCK) void k_volume_march_fused_shaded_amr(VolDev U, MarchTable<SURF, LIT> S, const FusedBrick *__restrict__ bricks, const AmrDev *__restrict__ amr,
                                                                             TopDev top, RayPlanes q, unsigned n, Mat4 minv, const float *__restrict__ clip_plane,
                                                                             unsigned n_clip, float *__restrict__ fb, unsigned n_pix, unsigned *__restrict__ work,
                                                                             unsigned long long *__restrict__ stats) {
  static_assert(SURF || LIT, "the plain frame is k_volume_march_fused_amr's");
  bool active = false, exhausted = false;
  bool hop = false;  // the lane's ray is between two bricks: fresh from the list (brick < 0) or at the end of a visit
  unsigned idx = 0;
  VolDev V = U;      // the lane's brick: U with the record's fields (SURF: V.mc points at the brick's per-cell words)
  AmrDev Am{ nullptr, nullptr, nullptr, nullptr }; // ... and its AMR tables: all null on a brick without subgrids
  int brick = -1;
  float o[3] = { 0.f, 0.f, 0.f }, d[3] = { 0.f, 0.f, 0.f }, C[3] = { 0.f, 0.f, 0.f }, A = 0.f;
  int k = 0, k_hi = -1, k_last = -1, k_carry = -1, prev = -1; // (k_carry, prev, n_crossed: SURF only)
  // (32 bits per lane, flushed between two bricks before they can wrap: k_volume_march_fused_shaded's bound; n_refined <= n_gathered)
  unsigned n_marched = 0, n_gathered = 0, n_crossed = 0, n_refined = 0;
  unsigned n_shaded = 0; // (LIT only)
  unsigned n_visits = 0, n_deposits = 0; // (wave-uniform: counted from ballots where the wave is converged)
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
        C[0] = 0.f; C[1] = 0.f; C[2] = 0.f;
        A = 0.f;
        prev = -1;
      }
    }
    if (!ballot64(active)) {
      if (exhausted) break;
      continue; // (every ray of the refill met no brick: the wave fetches again)
    }
    // ---- between two bricks: k_volume_march_fused_shaded's block (the shuffle's rule, evaluated by the lane)
    bool entered = false, deposited = false;
    if (active && hop) {
      hop = false;
      const float4 a = q.p0[idx], b = q.p1[idx];
      const int id = __float_as_int(q.p3[idx].x);
      const float wo[3] = { a.x, a.y, a.z }, wd[3] = { b.x, b.y, b.z };
      float t_clip;
      const bool clip = fused_clip<CLIP>(id, clip_plane, n_clip, t_clip);
      const float t_min = a.w; // (the end of a visit has stored it there, as vol_write_back does)
      if (n_marched >= 0x40000000u || n_crossed >= 0x40000000u) {
        atomicAdd(&stats[0], (unsigned long long)n_marched); atomicAdd(&stats[1], (unsigned long long)n_gathered);
        if constexpr (SURF) atomicAdd(&stats[4], (unsigned long long)n_crossed);
        if constexpr (LIT) atomicAdd(&stats[5], (unsigned long long)n_shaded);
        atomicAdd(&stats[VOL_FUSED_AMR_REFINED], (unsigned long long)n_refined);
        n_marched = 0; n_gathered = 0; n_crossed = 0; n_shaded = 0; n_refined = 0;
      }
      int next = -1;
      if (A < GVT_HIP_VOLUME_OPAQUE_A) next = vol_next(top, brick, wo, wd, t_min, clip, t_clip);
      if (next >= 0) {
        const FusedBrick R = bricks[next];
        Am = amr[next];
        V.vox = R.vox; V.mc = R.mc;
        V.nx = R.nx; V.ny = R.ny; V.nz = R.nz; V.ox = R.ox; V.oy = R.oy; V.oz = R.oz;
        for (int x = 0; x < 3; x++) { V.lo[x] = R.lo[x]; V.hi[x] = R.hi[x]; }
        const int k_prog = vol_ray_range<CLIP>(V, minv, make_float4(a.x, a.y, a.z, t_min), make_float4(b.x, b.y, b.z, t_clip), clip ? GVT_HIP_RAY_CLIP : 0, o, d, k, k_hi);
        k_last = -1;
        if constexpr (SURF) k_carry = prev >= 0 ? k_prog : -1; // the sides of the sample in t_min count only for the sample right after it
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
        V.nx = V.ny = V.nz = V.ox = V.oy = V.oz = 0;
        for (int x = 0; x < 3; x++) { o[x] = 0.f; d[x] = 0.f; }
        k = 0; k_hi = -1; k_last = -1; k_carry = -1; prev = -1;
      }
      brick = next;
    }
    n_visits += (unsigned)__popcll(ballot64(entered));
    n_deposits += (unsigned)__popcll(ballot64(deposited));
    // ---- the visit: volume_march_amr_body<SURF, LIT, CLIP>'s, step for step (KEEP IN STEP; `seen` there is k_last >= 0 here; nbx and nby
    // are recomputed: fused_macro_cell), under the null-table rule above
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
        if constexpr (SURF)
          if (k_last < 0 && k != k_carry) prev = -1;
        k_last = k;
        n_marched++;
        const int bi = fused_macro_cell(V.nx, V.ny, c);
        uint2 word = make_uint2(0u, 0u);
        unsigned pl = 0u;
        bool skip;
        if constexpr (SURF) { // the cell word is built from the merged ranges: no sample of any level in the macro cell changes an isovalue side
          float p[3];
          vol_point(V, o, d, k, p);
          pl = surf_plane_sides(S, p);
          const unsigned cell = V.skip ? ((const uint32_t *)V.mc)[bi] : 0u;
          skip = (cell & VOL_CELL_SKIP) && (prev < 0 || prev == (int)((cell & 0xffffu) | pl));
          if (skip) prev = (int)((cell & 0xffffu) | pl);
          if (!skip && Am.mc) word = Am.mc[bi]; // (the descent's entry: read for a gathered sample only)
        } else if (Am.mc) {
          word = Am.mc[bi];
          skip = V.skip && !(word.y >> 31);
        } else {
          skip = V.skip && !V.mc[bi];
        }
        if (skip) {
          if (A >= GVT_HIP_VOLUME_OPAQUE_A) { k++; done = true; break; } // the ray arrived opaque: this sample adds +0 and ends it, as any sample does
          const int kj = vol_jump_target(V, o, d, k, k_hi, c);
          bool jump = kj > k;
          if constexpr (SURF) jump = jump && surf_planes_clear(V, S, o, d, k, kj);
          if (jump) {
            n_marched += (unsigned)(kj - k);
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
        amr_corners(p, sy, sz, G);
        if constexpr (SURF) {
          unsigned sides = pl;
          for (int i = 0; i < S.n_iso; i++)
            if (v >= S.iso[i]) sides |= 1u << i;
          unsigned crossed = prev < 0 ? 0u : (sides ^ (unsigned)prev);
          prev = (int)sides;
          if (crossed) {
            float gc[3] = { 0.f, 0.f, 0.f }; // the isovalues crossed here share one gradient: the final cell's
            if (crossed & ((1u << S.n_iso) - 1u)) vol_gradient(amr_fine_spacing(V, log2_r), G, f, gc);
            while (crossed && A < GVT_HIP_VOLUME_OPAQUE_A) { // (at most 16 bits are set: sides and prev stay below 2^16)
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
      if (done) { // the ray leaves the brick (vol_write_back's t_min; its side mask and flag are prev): the next iteration decides where it goes
        if (k_last >= 0) q.p0[idx].w = (float)k_last * V.dt;
        hop = true;
      }
    }
  }
  unsigned long long w_marched = n_marched, w_gathered = n_gathered, w_crossed = n_crossed, w_shaded = n_shaded, w_refined = n_refined;
  for (int s = 32; s >= 1; s >>= 1) {
    w_marched += __shfl_xor(w_marched, s);
    w_gathered += __shfl_xor(w_gathered, s);
    w_refined += __shfl_xor(w_refined, s);
    if constexpr (SURF) w_crossed += __shfl_xor(w_crossed, s);
    if constexpr (LIT) w_shaded += __shfl_xor(w_shaded, s);
  }
  if (lane_id() == 0 && n_visits) {
    atomicAdd(&stats[0], w_marched);
    atomicAdd(&stats[1], w_gathered);
    atomicAdd(&stats[2], (unsigned long long)n_visits);
    atomicAdd(&stats[3], (unsigned long long)n_deposits);
    if (w_refined) atomicAdd(&stats[VOL_FUSED_AMR_REFINED], w_refined);
    if constexpr (SURF)
      if (w_crossed) atomicAdd(&stats[4], w_crossed);
    if constexpr (LIT)
      if (w_shaded) atomicAdd(&stats[5], w_shaded);
  }
}
