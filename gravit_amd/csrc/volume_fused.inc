// volume_fused.inc -- the fused frame: every brick of a bricked volume marched in ONE launch (gvt_hip_volume_frame_fused).  Included by
// volume.hip, inside its anonymous namespace, behind the steps of the march and the shuffle's vol_next.
//   k_volume_march_fused<T, CLIP>   one lane per camera ray, persistent waves with lane refill as in volume_march_body; a lane carries its
//                                   ray from brick to brick (vol_next in registers) until it deposits, and the wave refills only then
// The contract is stated in include/gvt_hip.h ("fused frame"): the fused frame is DEFINED by the loop of gvt_hip_volume_frame, a ray passes
// through the states the loop's ray passes through between its visits; tests/volume_fused_checker.py restates it in numpy.
//
// What is uniform over the bricks of one grid (table, global origin, spacing, dt, value range, skip flag, minv) stays in the kernel's
// VolDev argument, in scalar registers as in the plain march.  What differs per brick is a record of a device table indexed by instance
// (the host fills it per call), loaded into vector registers when the lane enters the brick: four 16-byte loads per visit.  The macro
// cells per axis are not in it: nbx and nby are (n - 1 + 7) / 8 of nx and ny, recomputed per sample (fused_macro_cell: two shifts and adds against
// two vector registers held through the march).
struct FusedBrick {
  const void *vox;     // the brick's samples
  const uint8_t *mc;   // its macro cells' skip bytes
  int nx, ny, nz, ox, oy, oz;
  float lo[3], hi[3];  // the vertex box, object space: read by vol_ray_range on entry, dead afterwards
};
static_assert(sizeof(FusedBrick) == 64, "four 16-byte loads per record");
// ... and what the CENTRAL instantiations of the shaded, shadowed, fog and mesh kernels receive beside it (GVT_HIP_FUSED_CENTRAL,
// GVT_HIP_VOLUME_ALLOW_CENTRAL): the bricks' ghost layers as a further device table of face pointers (gvt_hip_volume::d_ghost; null for a
// brick without an interior face, whose layers are never read), indexed like the records and loaded where they are loaded -- the pointer
// is part of the lane's brick state -- and the global grid's size, uniform, by value.  Every other instantiation receives NoGhost
struct FusedGhost {
  const void *const *faces;
  int gnx, gny, gnz;
};
template <bool CENTRAL>
using FusedGhostArg = std::conditional_t<CENTRAL, FusedGhost, NoGhost>;
// the lane's ghost table: the uniform sizes from the argument, the pointer of no brick yet
template <bool CENTRAL>
__device__ __forceinline__ GhostTable<CENTRAL> fused_ghost_init(const FusedGhostArg<CENTRAL> &HG) {
  if constexpr (CENTRAL) return GhostDev{ nullptr, HG.gnx, HG.gny, HG.gnz };
  else return NoGhost{};
}
#define VOL_FUSED_STATS 4 // words of the launch's counters: samples marched, samples gathered, brick visits, rays deposited

// the depth plane's word for ray idx: what k_vol_scatter (fresh == 2) gives the ray as t_max and GVT_HIP_RAY_CLIP, read again at every
// brick change instead of carried (the pixel's id is the ray's own, plane 3)
template <bool CLIP>
__device__ __forceinline__ bool fused_clip(int id, const float *__restrict__ clip_plane, unsigned n_clip, float &t_clip) {
  t_clip = INFINITY;
  if constexpr (CLIP) {
    if ((unsigned)id < n_clip) t_clip = clip_plane[(unsigned)id];
    return t_clip < INFINITY;
  }
  return false;
}

// the macro cell of cell c in a brick of nx * ny * .. vertices: nby and nbx of THIS brick, (n - 1 + 7) / 8, recomputed (above).  Every
// fused kernel and both light grid bakes index the skip bytes and the per-cell words through it
__device__ __forceinline__ int fused_macro_cell(int nx, int ny, const int c[3]) {
  return ((c[2] >> 3) * ((ny + 6) >> 3) + (c[1] >> 3)) * ((nx + 6) >> 3) + (c[0] >> 3);
}

// the end of a camera ray: its colour and opacity into its pixel (four atomic adds; a pixel id beyond the film deposits nothing)
__device__ __forceinline__ void fused_deposit(float *__restrict__ fb, unsigned n_pix, int id, const float C[3], float A) {
  if ((unsigned)id < n_pix) {
    float *px = fb + (size_t)4 * (unsigned)id;
    atomicAdd(px + 0, C[0]); atomicAdd(px + 1, C[1]); atomicAdd(px + 2, C[2]); atomicAdd(px + 3, A);
  }
}

template <typename T, bool CLIP>
__global__ __launch_bounds__(VOL_BLOCK) void k_volume_march_fused(VolDev U, const FusedBrick *__restrict__ bricks, TopDev top, RayPlanes q, unsigned n, Mat4 minv,
                                                                  const float *__restrict__ clip_plane, unsigned n_clip, float *__restrict__ fb, unsigned n_pix,
                                                                  unsigned *__restrict__ work, unsigned long long *__restrict__ stats) {
  bool active = false, exhausted = false;
  bool hop = false;  // the lane's ray is between two bricks: fresh from the list (brick < 0) or at the end of a visit
  unsigned idx = 0;
  VolDev V = U;      // the lane's brick: U with the record's fields
  int brick = -1;
  float o[3] = { 0.f, 0.f, 0.f }, d[3] = { 0.f, 0.f, 0.f }, C[3] = { 0.f, 0.f, 0.f }, A = 0.f;
  int k = 0, k_hi = -1, k_last = -1;
  unsigned n_marched = 0, n_gathered = 0; // (32 bits per lane: flushed between two bricks long before they can wrap, a visit adds at most 2^23)
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
    // ---- between two bricks: the shuffle's rule (k_vol_classify), evaluated by the lane.  The ray's world origin and direction and its
    // pixel are read from the camera's list again: they are not carried through the march
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
        n_marched = 0; n_gathered = 0;
      }
      int next = -1;
      if (A < GVT_HIP_VOLUME_OPAQUE_A) next = vol_next(top, brick, wo, wd, t_min, clip, t_clip);
      if (next >= 0) {
        const FusedBrick R = bricks[next];
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
        V.nx = V.ny = V.nz = V.ox = V.oy = V.oz = 0;
        for (int x = 0; x < 3; x++) { o[x] = 0.f; d[x] = 0.f; }
        k = 0; k_hi = -1; k_last = -1;
      }
      brick = next;
    }
    n_visits += (unsigned)__popcll(ballot64(entered));
    n_deposits += (unsigned)__popcll(ballot64(deposited));
    // ---- the visit: volume_march_body's plain march, step for step through the same device functions
    if (active) {
      bool done = false;
      for (int s = 0; s < VOL_STEP; s++) {
        if (k > k_hi) { done = true; break; }
        int c[3];
        float f[3];
        if (!vol_cell(V, o, d, k, c, f)) {
          if (k_last >= 0) { done = true; break; } // (the march's `seen`: set with k_last)  A brick's samples along a line are contiguous: the rest belongs to others
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
  unsigned long long w_marched = n_marched, w_gathered = n_gathered;
  for (int s = 32; s >= 1; s >>= 1) {
    w_marched += __shfl_xor(w_marched, s);
    w_gathered += __shfl_xor(w_gathered, s);
  }
  if (lane_id() == 0 && n_visits) {
    atomicAdd(&stats[0], w_marched);
    atomicAdd(&stats[1], w_gathered);
    atomicAdd(&stats[2], (unsigned long long)n_visits);
    atomicAdd(&stats[3], (unsigned long long)n_deposits);
  }
}
