// volume_occluder_grid.inc -- the occluder grids of the mesh-shadowed frame (gvt_hip_volume_occluder_grid_bake; the contract:
// include/gvt_hip.h, "meshes shadowing the volume").  Included by volume.hip behind volume_fused_fog.inc.
// The work list is volume_light_grid.inc's: one item per (vertex, usable light) pair, a brick's items contiguous, plane after plane, x
// fastest.  It is walked in CHUNKS of VOL_OCC_CHUNK pairs so that the rays' planes stay bounded (at 256^3 the whole list would be 0.5 GB):
//   k_occluder_rays   one lane per pair of the chunk: the ray from the vertex towards the light, in the list's form -- the p0 / p1 words
//                     k_od_to_planes writes (origin | GVT_RAY_EPSILON, direction | GVT_FLT_MAX)
//   (launch_any_flags per mesh instance, xform = true: the existing any-hit traversal, unchanged)
//   k_occluder_fold   O &= !flag, after every instance
//   k_occluder_pack   the chunk's O into the bricks' planes, at the samples' own index; counts the blocked rays
// No kernel here loops, and each lane's stores stay inside the chunk (i < n) or inside its brick's planes (local < the brick's pairs).
#define VOL_OCC_CHUNK (1u << 20) // pairs per chunk: 32 MiB of ray planes, 4 MiB of flags, 1 MiB of O

// a brick's part of the work list and where its planes go: items [first, first + n_vert * usable lights)
struct OccluderBrick {
  uint8_t *out;
  unsigned first;
  int nx, ny, nz, ox, oy, oz;
};

// the brick of work item `slot` (the parts are in the order of their first items; at most VOL_DEST_MAX of them)
__device__ __forceinline__ unsigned occluder_part(const OccluderBrick *__restrict__ parts, unsigned n_bricks, unsigned slot) {
  unsigned b = 0;
  while (b + 1 < n_bricks && parts[b + 1].first <= slot) b++;
  return b;
}

// KEEP IN STEP with k_volume_bake_light's refill: the item's brick, light and vertex, and the vertex in world space
__global__ __launch_bounds__(VOL_BLOCK) void k_occluder_rays(float gox, float goy, float goz, float sx, float sy, float sz, ShadowDev H,
                                                             const OccluderBrick *__restrict__ parts, unsigned n_bricks, unsigned base, unsigned n, Mat4 m,
                                                             float4 *__restrict__ p0, float4 *__restrict__ p1) {
  const unsigned i = blockIdx.x * VOL_BLOCK + threadIdx.x;
  if (i >= n) return;
  const unsigned slot = base + i;
  const OccluderBrick Q = parts[occluder_part(parts, n_bricks, slot)];
  const unsigned local = slot - Q.first;
  const unsigned n_vert = (unsigned)Q.nx * (unsigned)Q.ny * (unsigned)Q.nz;
  const unsigned l = local / n_vert, v = local - l * n_vert;
  const unsigned row = (unsigned)Q.nx * (unsigned)Q.ny;
  const unsigned vz = v / row, vy = (v - vz * row) / (unsigned)Q.nx, vx = v - vz * row - vy * (unsigned)Q.nx;
  // the l-th usable light
  unsigned rest = H.usable;
  for (unsigned u = 0; u < l; u++) rest &= rest - 1u;
  const int lj = __ffs((int)rest) - 1;
  float ws[3] = { 0.f, 0.f, 0.f };
  for (int j = 0; j < GVT_HIP_VOLUME_MAX_LIGHTS; j++)
    if (j == lj) { ws[0] = H.ws[j][0]; ws[1] = H.ws[j][1]; ws[2] = H.ws[j][2]; }
  const V3 p = mk3(gox + (float)(Q.ox + (int)vx) * sx, goy + (float)(Q.oy + (int)vy) * sy, goz + (float)(Q.oz + (int)vz) * sz);
  const V3 wp = xfm_point(m, p);
  p0[i] = make_float4(wp.x, wp.y, wp.z, GVT_RAY_EPSILON);
  p1[i] = make_float4(ws[0], ws[1], ws[2], GVT_FLT_MAX);
}

__global__ __launch_bounds__(VOL_BLOCK) void k_occluder_fold(const int *__restrict__ flags, unsigned n, uint8_t *__restrict__ O) {
  const unsigned i = blockIdx.x * VOL_BLOCK + threadIdx.x;
  if (i >= n) return;
  if (flags[i]) O[i] = 0;
}

__global__ __launch_bounds__(VOL_BLOCK) void k_occluder_pack(const uint8_t *__restrict__ O, const OccluderBrick *__restrict__ parts, unsigned n_bricks, unsigned base,
                                                             unsigned n, unsigned long long *__restrict__ blocked) {
  const unsigned i = blockIdx.x * VOL_BLOCK + threadIdx.x;
  bool is_blocked = false;
  if (i < n) {
    const unsigned slot = base + i;
    const OccluderBrick Q = parts[occluder_part(parts, n_bricks, slot)];
    const uint8_t o = O[i];
    Q.out[slot - Q.first] = o;
    is_blocked = o == 0;
  }
  const unsigned long long b = ballot64(is_blocked);
  if (b && lane_id() == 0) atomicAdd(blocked, (unsigned long long)__popcll(b));
}
