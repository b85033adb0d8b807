// volume_fused_shaded.inc -- the fused frame for bricks that have isovalues / slice planes or lit fog (gvt_hip_volume_frame_fused_shaded).
// Included by volume.hip behind volume_fused.inc, whose FusedBrick record, counters and fused_clip it uses.
//   k_volume_march_fused_shaded<T, CLIP, SURF, LIT, CENTRAL>   k_volume_march_fused's structure (persistent waves, lane refill, the "between
//                                   two bricks" block, a VOL_STEP inner loop) around the visit of volume_march_body<T, SURF, CLIP, LIT, CENTRAL>
// CENTRAL (GVT_HIP_FUSED_CENTRAL: every brick's gradient kind is CENTRAL): the gradient of a crossed isovalue and of a lit sample is
// vol_gradient_central's, from the lane's ghost table (FusedGhost, volume_fused.inc); nothing else reads it.  Without CENTRAL the kernel
// is what it was before the parameter existed, instruction for instruction (profiles/volume_fused_central.txt, 1).
// KEEP IN STEP with volume_march_body (volume.hip): the visit below restates its per-sample steps -- the sides, the skip decision on the
// per-cell word, surf_planes_clear, the crossing loop, the lit accumulation -- through the same device functions, in the same order.
// They are restated, not hoisted: the march kernels of volume.hip are to stay what they were, instruction for instruction
// (profiles/volume_fused_shaded.txt, 1).  A change to one of the two is a change to both; tests/test_gpu_volume_fused_shaded.py compares
// their framebuffers in every bit.
//
// What a ray carries between two visits beyond the plain fused frame's (the loop's states, vol_write_back<true> and the refill of
// volume_march_body): the side mask of its last owned sample.  It lives in one register, prev: -1 for a camera ray and until a visit has
// owned a sample; afterwards the sides of sample k_last, below 2^16 -- so "the ray carries GVT_HIP_RAY_SIDES" is prev >= 0, and a visit
// that owns no sample leaves it as it was.  On entering a brick k_carry = k_prog where the ray is flagged, else -1; at the first owned
// sample prev = -1 unless k == k_carry.
//
// Per brick, the SURF visit reads the per-cell words (d_cells) and never the skip bytes: the record's mc slot carries d_cells then, and
// the four 16-byte loads per visit stay four.  Isovalues, planes, lights, alpha, ka, kd are uniform over the bricks (the host compares
// them as bits) and travel by value, as in k_volume_march_surf; S.cells is not read here.
#define VOL_FUSED_SHADED_STATS 6 // VOL_FUSED_STATS' four words, then surface crossings rendered and samples shaded

template <typename T, bool CLIP, bool SURF, bool LIT, bool CENTRAL>
__global__ __launch_bounds__(VOL_BLOCK) void k_volume_march_fused_shaded(VolDev U, MarchTable<SURF, LIT> S, const FusedBrick *__restrict__ bricks, TopDev top, RayPlanes q,
                                                                         unsigned n, Mat4 minv, const float *__restrict__ clip_plane, unsigned n_clip,
                                                                         float *__restrict__ fb, unsigned n_pix, unsigned *__restrict__ work,
                                                                         unsigned long long *__restrict__ stats, FusedGhostArg<CENTRAL> HG) {
  static_assert(SURF || LIT, "the plain frame is k_volume_march_fused's");
  bool active = false, exhausted = false;
  bool hop = false;  // the lane's ray is between two bricks: fresh from the list (brick < 0) or at the end of a visit
  unsigned idx = 0;
  VolDev V = U;      // the lane's brick: U with the record's fields (SURF: V.mc points at the brick's per-cell words)
  GhostTable<CENTRAL> Hl = fused_ghost_init<CENTRAL>(HG); // ... and, CENTRAL only, its ghost layers: the pointer changes with the brick
  int brick = -1;
  float o[3] = { 0.f, 0.f, 0.f }, d[3] = { 0.f, 0.f, 0.f }, C[3] = { 0.f, 0.f, 0.f }, A = 0.f;
  int k = 0, k_hi = -1, k_last = -1, k_carry = -1, prev = -1; // (k_carry, prev, n_crossed: SURF only)
  // (32 bits per lane: flushed between two bricks before they can wrap.  A visit walks at most 2^22 lattice positions, a jump counts at
  // most as many again, and a sample renders at most 16 crossings: below 2^27 per visit on top of a threshold of 2^30)
  unsigned n_marched = 0, n_gathered = 0, n_crossed = 0;
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
      if (n_marched >= 0x40000000u || n_crossed >= 0x40000000u) {
        atomicAdd(&stats[0], (unsigned long long)n_marched); atomicAdd(&stats[1], (unsigned long long)n_gathered);
        if constexpr (SURF) atomicAdd(&stats[4], (unsigned long long)n_crossed);
        if constexpr (LIT) atomicAdd(&stats[5], (unsigned long long)n_shaded);
        n_marched = 0; n_gathered = 0; n_crossed = 0; n_shaded = 0;
      }
      int next = -1;
      if (A < GVT_HIP_VOLUME_OPAQUE_A) next = vol_next(top, brick, wo, wd, t_min, clip, t_clip);
      if (next >= 0) {
        const FusedBrick R = bricks[next];
        if constexpr (CENTRAL) Hl.faces = HG.faces[next];
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
        if constexpr (CENTRAL) Hl.faces = nullptr;
        V.nx = V.ny = V.nz = V.ox = V.oy = V.oz = 0;
        for (int x = 0; x < 3; x++) { o[x] = 0.f; d[x] = 0.f; }
        k = 0; k_hi = -1; k_last = -1; k_carry = -1; prev = -1;
      }
      brick = next;
    }
    n_visits += (unsigned)__popcll(ballot64(entered));
    n_deposits += (unsigned)__popcll(ballot64(deposited));
    // ---- the visit: volume_march_body<T, SURF, CLIP, LIT, CENTRAL>'s, step for step (KEEP IN STEP; `seen` there is k_last >= 0 here)
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
        unsigned pl = 0u;
        bool skip;
        if constexpr (SURF) {
          float p[3];
          vol_point(V, o, d, k, p);
          pl = surf_plane_sides(S, p);
          const unsigned cell = V.skip ? ((const uint32_t *)V.mc)[bi] : 0u;
          skip = (cell & VOL_CELL_SKIP) && (prev < 0 || prev == (int)((cell & 0xffffu) | pl));
          if (skip) prev = (int)((cell & 0xffffu) | pl);
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
        VolCorners G;
        const float v = vol_gather<T>(V, c, f, G);
        if constexpr (SURF) {
          unsigned sides = pl;
          for (int i = 0; i < S.n_iso; i++)
            if (v >= S.iso[i]) sides |= 1u << i;
          unsigned crossed = prev < 0 ? 0u : (sides ^ (unsigned)prev);
          prev = (int)sides;
          if constexpr (CENTRAL) { // the same loop with the gradient of the ghost table (stated apart: the loop below is to compile to what it was)
            if (crossed) {
              float gc[3] = { 0.f, 0.f, 0.f }; // the isovalues crossed here share one gradient, fetched once, ahead of the loop, as in the body
              if (crossed & ((1u << S.n_iso) - 1u)) vol_gradient_central<T>(V, Hl, c, G, f, gc);
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
          } else
          if (crossed) {
            while (crossed && A < GVT_HIP_VOLUME_OPAQUE_A) { // (at most 16 bits are set: sides and prev stay below 2^16)
              const int i = __ffs((int)crossed) - 1;
              crossed &= crossed - 1u;
              n_crossed++;
              if (i < S.n_iso) {
                float g[3];
                vol_gradient(V, G, f, g); // (the body's three expressions)
                surf_composite(S, vol_lookup(V, S.iso[i]), g, C, A);
              } else {
                const float4 P = S.plane[i - S.n_iso];
                const float g[3] = { P.x, P.y, P.z };
                surf_composite(S, vol_lookup(V, v), g, C, A);
              }
            }
            if (A >= GVT_HIP_VOLUME_OPAQUE_A) { k++; done = true; break; } // the surface ends the ray: the sample itself adds nothing
          }
        }
        if constexpr (LIT) n_shaded += vol_accumulate_lit<T, CENTRAL>(V, S, Hl, c, v, G, f, C, A);
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
  unsigned long long w_marched = n_marched, w_gathered = n_gathered, w_crossed = n_crossed, w_shaded = n_shaded;
  for (int s = 32; s >= 1; s >>= 1) {
    w_marched += __shfl_xor(w_marched, s);
    w_gathered += __shfl_xor(w_gathered, s);
    if constexpr (SURF) w_crossed += __shfl_xor(w_crossed, s);
    if constexpr (LIT) w_shaded += __shfl_xor(w_shaded, s);
  }
  if (lane_id() == 0 && n_visits) {
    atomicAdd(&stats[0], w_marched);
    atomicAdd(&stats[1], w_gathered);
    atomicAdd(&stats[2], (unsigned long long)n_visits);
    atomicAdd(&stats[3], (unsigned long long)n_deposits);
    if constexpr (SURF)
      if (w_crossed) atomicAdd(&stats[4], w_crossed);
    if constexpr (LIT)
      if (w_shaded) atomicAdd(&stats[5], w_shaded);
  }
}
