// volume.hip -- volume domains: scalar bricks rendered with a transfer function.
//   gvt_hip_volume_create / _set_transfer   Volume + TransferFunction (render/data/primitives/Volume.h, TransferFunction.cpp:40-72)
//   gvt_hip_volume_create_typed             ... with 8- and 16-bit integer voxels kept at their own width (Volume::VoxelType, Volume.h:67-75):
//                                           the kernels that read voxels are templates over the voxel's C type, a vertex's value is (float)v
//   k_vol_ranges / k_vol_range_total        the macro cells' value ranges and the brick's, on the device (create and gvt_hip_volume_update_samples)
//   k_volume_march / k_volume_march_surf    the volume adapters' trace (adapter/ospray/OSPRayAdapter.cpp, adapter/pvol/PVolAdapter.cpp): entry
//   k_volume_march_lit / _surf_lit          points of one body, volume_march_body<T, SURF, CLIP, LIT> (SURF: isovalues and slice planes;
//                                           CLIP: the launch may hold rays clipped at their t_max, GVT_HIP_RAY_CLIP; LIT: every contributing
//                                           sample is shaded by the interpolant's gradient, gvt_hip_volume_set_shading)
//   k_volume_march_surf_central / _lit_central / _surf_lit_central   the three shaded marches with GVT_HIP_VOLUME_GRADIENT_CENTRAL: the
//                                           same body with CENTRAL, the gradient from central differences at the vertices, which read
//                                           one ghost layer beyond the brick's interior faces (gvt_hip_volume_set_ghosts / _set_gradient)
//   k_vol_classify / k_vol_scatter          AbstractTrace::shuffleRays, volume branch, PRIMARY rays (algorithm/TracerBase.h:344-391), around
//                                           the mesh shuffle's k_dest_scan (ordered_scan.inc)
//   k_volume_march_amr / k_amr_ranges       AMR volumes (Volume::AddAMRGrid): nested refined subgrids inside a brick, volume_amr.inc
//   k_amr_ranges_merge                      ... and their time steps in place (gvt_hip_volume_update_amr)
//   k_volume_march_amr_surf / _lit / _surf_lit   ... with isovalues, slice planes and lit fog in the refined cells (GVT_HIP_VOLUME_AMR_SHADED)
//   gvt_hip_volume_frame [_clipped]         Tracer<ImageScheduler>::operator() (algorithm/ImageTracer.h:127-269) over bricks; clipped: every camera
//                                           ray ends at its pixel of a depth plane (depth.hip) -- geometry inside the volume
//   gvt_hip_volume_frame_fused / k_volume_march_fused   the same frame over bricks of ONE grid in one launch: a lane carries its ray from brick to
//                                           brick (volume_fused.inc); every other frame takes the loop
//   gvt_hip_volume_frame_fused_shaded / k_volume_march_fused_shaded   ... and, where the caller allows it, frames whose bricks have isovalues,
//                                           slice planes or lit fog: the same structure around the surface / lit visit (volume_fused_shaded.inc).
//                                           GVT_HIP_FUSED_CENTRAL / GVT_HIP_VOLUME_ALLOW_CENTRAL: the CENTRAL instantiations of this kernel
//                                           and of the three shadowed ones below, for frames whose bricks all shade with central
//                                           differences; a lane carries its brick's ghost pointer from brick to brick (FusedGhost)
//   gvt_hip_volume_frame_fused_amr / k_volume_march_fused_amr, k_volume_march_fused_shaded_amr   ... and, with GVT_HIP_FUSED_AMR, frames in
//                                           which some or all bricks have subgrids: the same structure around the AMR visit; a lane carries
//                                           its brick's AMR tables, all null on a brick without subgrids (volume_fused_amr.inc)
//   gvt_hip_volume_frame_shadowed / k_volume_march_fused_shadow   ... with the crossings lit only by the lights that reach them: a lane marches the
//                                           shadow rays of its camera ray itself, from brick to brick (volume_fused_shadow.inc)
//   gvt_hip_volume_light_grid_bake / k_volume_bake_light   the transmittance towards every light at every grid vertex, kept beside the samples
//                                           (volume_light_grid.inc), and gvt_hip_volume_frame_fog_shadowed / k_volume_march_fused_fog, the
//                                           shadowed frame whose lit fog samples interpolate it (volume_fused_fog.inc)
//   gvt_hip_volume_occluder_grid_bake / k_occluder_rays, _fold, _pack   whether a mesh stands between every grid vertex and every light, from the
//                                           any-hit traversal of trace.hip, as uint8 planes beside the samples (volume_occluder_grid.inc), and
//                                           gvt_hip_volume_frame_mesh_shadowed / k_volume_march_fused_mesh, the fog-shadowed frame in which
//                                           every transmittance is multiplied by their interpolant (volume_fused_mesh.inc)
//   gvt_hip_volume_march_queue / _camera_filter   the Domain scheduler's steps over bricks spread over ranks (algorithm/DomainTracer.h:148-326): the march
//                                           on a device queue, and the camera step with shuffleDropRays' keep mask (k_vol_classify<MASK>); the
//                                           exchange's batched wire conversions are beside k_planes_to_aos (convert.inc, trace.hip)
// The contract (lattice, ownership, evaluation order, flags) is stated in include/gvt_hip.h; tests/volume_checker.py restates it in numpy.
#include <algorithm>
#include <cmath>
#include <string>
#include <type_traits>
#include <vector>

#include "gvt_internal.h"

// What a brick remembers of the bake that filled its grid planes (the light grids' or the occluder grids'): planes, one per usable light
// in the order of their bits; current: no call that makes the planes stale has touched the volume since; bake / index / count / m /
// minv: which bake, and what it covered
struct BakedGrids {
  int planes = 0;
  unsigned usable = 0;
  bool current = false;
  uint64_t bake = 0;
  size_t index = 0, count = 0;
  float m[16] = {}, minv[16] = {};
};

namespace {
struct AmrRangeItem;
struct AmrMergeCell;
} // namespace

struct gvt_hip_volume {
  int n[3] = { 0, 0, 0 }, off[3] = { 0, 0, 0 };
  float go[3] = { 0, 0, 0 }, sp[3] = { 1, 1, 1 };
  float rate = 1.f, dt = 1.f;
  float lo[3] = { 0, 0, 0 }, hi[3] = { 0, 0, 0 }; // the brick's vertex box, object space
  int skip = 1;
  float vmin = 0.f, vmax = 0.f;
  int nb[3] = { 0, 0, 0 };
  std::vector<float> bmin, bmax; // per macro cell: value range of its vertices
  std::vector<uint8_t> bnan;     // ... and whether one of them is NaN or +-Inf: its samples can evaluate to NaN (Inf - Inf, 0 * Inf)
  uint64_t n_empty = 0;
  bool has_tf = false;
  float tf_lo = 0.f, tf_hi = 1.f;
  float tf_a[256] = {};          // the table's corrected opacities (d_tf[i].w): what rebuild_tables reads after an update of the samples
  float tf_rgb[256][3] = {};     // ... and its colours (d_tf[i].xyz): with tf_a the host's copy of the table (the fused frame compares the bricks' tables)
  int vtype = GVT_HIP_VOXEL_F32;   // the voxel type, fixed at creation: d_vox holds the samples at that width and nothing wider exists
  void *d_vox = nullptr;
  float4 *d_tf = nullptr;        // 256 x (r, g, b, corrected a)
  uint8_t *d_mc = nullptr;       // per macro cell: 1 = some table entry its values can reach has a > 0
  unsigned long long *d_stats = nullptr; // samples marched, samples gathered, surface crossings rendered, samples shaded, samples refined (VOL_N_STATS words)
  // surfaces (gvt_hip_volume_set_surfaces / _set_lights): with n_iso + n_pl > 0 the march is k_volume_march_surf (volume_march_body<true>)
  int n_iso = 0, n_pl = 0, n_lights = 0;
  float iso[GVT_HIP_VOLUME_MAX_SURFACES] = {}, plane[GVT_HIP_VOLUME_MAX_SURFACES][4] = {};
  float surf_alpha = 1.f, ka = 0.4f, kd = 0.6f;
  int shade = GVT_HIP_VOLUME_SHADE_NONE; // gvt_hip_volume_set_shading: with GRADIENT and n_lights > 0 the march is a LIT one (the lights above)
  float lpos[GVT_HIP_VOLUME_MAX_LIGHTS][3] = {}, lcol[GVT_HIP_VOLUME_MAX_LIGHTS][3] = {};
  std::vector<uint8_t> h_mc;     // host copy of d_mc
  uint32_t *d_cells = nullptr;   // per macro cell, for the surface march: skip bit and isovalue sides (rebuilt by set_transfer and set_surfaces)
  // AMR (gvt_hip_volume_set_subgrids): with subgrids the march is k_volume_march_amr or, with surfaces or lit shading on a set flagged
  // GVT_HIP_VOLUME_AMR_SHADED, one of its three shaded entry points (volume_amr.inc: the device tables)
  std::vector<gvt_hip_subgrid> sub;
  int amr_levels = 1;            // level 0 and the deepest subgrid's
  uint64_t amr_bytes = 0, amr_marches = 0;
  int amr_flags = 0;             // the flags of the current set of subgrids (GVT_HIP_VOLUME_AMR_SHADED: it takes surfaces and lit shading); 0 without one
  float *d_amr_vox = nullptr;
  uint2 *d_amr_mc = nullptr;
  int *d_amr_list = nullptr;
  int4 *d_amr_desc = nullptr;
  std::vector<uint32_t> amr_first, amr_count; // per macro cell: its level-1 subgrids in d_amr_list (d_amr_mc without the skip bit)
  // gvt_hip_volume_update_amr's tables (volume_amr.inc, k_amr_ranges_merge), built at the first update of a tree and freed with it: the
  // range items grouped by macro cell, one AmrMergeCell per macro cell that has some; and every subgrid's place in d_amr_vox
  AmrRangeItem *d_amr_items = nullptr;
  AmrMergeCell *d_amr_cells = nullptr;
  unsigned amr_n_cells = 0;
  uint64_t amr_merge_bytes = 0;
  std::vector<size_t> amr_offset, amr_samples;
  // smooth gradients (gvt_hip_volume_set_ghosts / _set_gradient): with GVT_HIP_VOLUME_GRADIENT_CENTRAL the shaded marches are the _central
  // entry points, which read the six face layers beyond the brick from d_ghost (one allocation: -x +x -y +y -z +z, a slab of a missing
  // face is never read)
  int gn[3] = { 0, 0, 0 };       // the global grid's vertices per axis
  int grad = GVT_HIP_VOLUME_GRADIENT_CELL;
  unsigned ghost_mask = 0;       // bit 2 * axis + side: that face has a layer
  void *d_ghost = nullptr;
  uint64_t central_marches = 0;
  // the light transmittance grids of the fog-shadowed frame (gvt_hip_volume_light_grid_bake; volume_light_grid.inc): lg.planes planes of
  // the brick's vertices.  lg.current: no call that changes what a shadow ray meets has touched the volume since the bake
  float *d_lgrid = nullptr;
  BakedGrids lg;
  int lg_bias = 0;
  // the occluder grids of the mesh-shadowed frame (gvt_hip_volume_occluder_grid_bake; volume_occluder_grid.inc): og.planes uint8 planes of
  // the brick's vertices (1: no mesh between the vertex and the light, 0: one).  og.current: neither the lights nor the subgrids were
  // set since the bake
  uint8_t *d_occ = nullptr;
  BakedGrids og;
  // the AO grid of the AO frame (gvt_hip_volume_ao_grid_bake; volume_ao_grid.inc): ONE float32 plane of the brick's vertices (ag.planes is
  // 1, ag.usable unused).  ag.current: no call that changes what an AO ray meets (samples, table, surfaces, subgrids) has touched the
  // volume since the bake; the lights, the shading, the gradient kind and the ghosts do not matter to it
  float *d_ao = nullptr;
  BakedGrids ag;
  int ag_dirs = 0, ag_bias = 0;
  float ag_radius = 0.f;
};

namespace {

#define VOL_BLOCK 256
#define VOL_STEP 32          // samples a lane marches between two refill decisions of its wave
#define VOL_REFILL_MIN 16    // a wave fetches new rays once at least this many of its lanes are idle (or all of them)
#define VOL_K_MAX 1073741824.f
#define VOL_MAX_SAMPLES (1 << 22) // lattice positions one visit of a brick walks at most (only reached by rays whose |d| is far below the spacing)
#define VOL_DEST_MAX 256
#define VOL_N_STATS 8        // words of gvt_hip_volume::d_stats (five in use)

struct VolDev {
  const void *vox; // samples of the brick's voxel type (vol_gather<T> reads them)
  const float4 *tf;
  const uint8_t *mc;
  int nx, ny, nz, ox, oy, oz, nbx, nby;
  float gox, goy, goz, sx, sy, sz, dt;
  float lo[3], hi[3];
  float vlo, vspan;
  int skip;
};

// slab test of the ray o + t d against [lo, hi] in the contract's fixed form (the march and the shuffle; tests/volume_checker.py restates
// it): an axis with d == 0 keeps the whole line or none of it.  Miss: tn > tf.
__device__ inline void vol_slab(const float lo[3], const float hi[3], const float o[3], const float d[3], float &tn, float &tf) {
  tn = -INFINITY; tf = INFINITY;
  for (int a = 0; a < 3; a++) {
    if (d[a] == 0.f) {
      if (o[a] < lo[a] || o[a] > hi[a]) { tn = INFINITY; tf = -INFINITY; }
      continue;
    }
    const float inv = 1.f / d[a];
    float t0 = (lo[a] - o[a]) * inv, t1 = (hi[a] - o[a]) * inv;
    if (t0 > t1) { const float s = t0; t0 = t1; t1 = s; }
    tn = fmaxf(tn, t0); tf = fminf(tf, t1);
  }
}

// first lattice index k >= 0 with k * dt > t; -1: none below VOL_K_MAX
__device__ inline int vol_first_after(float t, float dt) {
  if (!(t >= 0.f)) return 0;
  const float q = floorf(t / dt);
  if (!(q < VOL_K_MAX)) return -1;
  int k = (int)q;
  while ((float)k * dt <= t) k++;
  while (k > 0 && (float)(k - 1) * dt > t) k--;
  return k;
}

// a clipped ray (GVT_HIP_RAY_CLIP): the last lattice index k >= 0 with k * dt < t_max; -1: none (t_max <= 0, NaN); VOL_K_MAX: no cut
__device__ inline int vol_last_before(float t_max, float dt) {
  if (!(t_max > 0.f)) return -1;
  const float q = floorf(t_max / dt);
  if (!(q < VOL_K_MAX)) return (int)VOL_K_MAX;
  int k = (int)q;
  while ((float)(k + 1) * dt < t_max) k++;
  while (k >= 0 && !((float)k * dt < t_max)) k--;
  return k;
}

// the global cell of lattice sample k: is it the brick's?  c = the cell relative to the brick, f = the fractions inside it
__device__ inline bool vol_cell(const VolDev &V, const float o[3], const float d[3], int k, int c[3], float f[3]) {
  const float t = (float)k * V.dt;
  const float g[3] = { ((o[0] + d[0] * t) - V.gox) / V.sx, ((o[1] + d[1] * t) - V.goy) / V.sy, ((o[2] + d[2] * t) - V.goz) / V.sz };
  const int off[3] = { V.ox, V.oy, V.oz }, n[3] = { V.nx, V.ny, V.nz };
  bool own = true;
  for (int a = 0; a < 3; a++) {
    const float fl = floorf(g[a]);
    f[a] = g[a] - fl;
    own = own && fl >= (float)off[a] && fl <= (float)(off[a] + n[a] - 2); // (false for NaN)
    c[a] = own ? (int)fl - off[a] : 0;
  }
  return own;
}

__device__ inline float lerp_(float a, float b, float f) { return a + f * (b - a); }

// ---- surfaces in the march: isovalues and slice planes, shaded (the contract: include/gvt_hip.h; tests/volume_surface_checker.py).
// The table is wave-uniform and travels by value (kernel arguments, read with scalar loads); per lane the march adds the side mask of
// the previous sample, the lattice index the carried mask belongs to and, at a crossing only, the gradient.
struct SurfDev {
  float iso[GVT_HIP_VOLUME_MAX_SURFACES];
  float4 plane[GVT_HIP_VOLUME_MAX_SURFACES];                                // (nx, ny, nz, d), object space; bit n_iso + j
  float ldir[GVT_HIP_VOLUME_MAX_LIGHTS][3], lcol[GVT_HIP_VOLUME_MAX_LIGHTS][3]; // unit directions in object space, colours
  const uint32_t *cells; // per macro cell: bit 16 = its samples may go uninterpolated, bits 0..15 = their isovalue sides
  int n_iso, n_pl, n_lights;
  float alpha, ka, kd;
};
struct NoSurf {}; // what the plain march has in SurfDev's place: nothing (its scalar registers are full without the table)
// ... and what the lit plain march has there: the lights alone, about 200 bytes by value (the per-light loop reads them with scalar loads)
struct LightDev {
  float ldir[GVT_HIP_VOLUME_MAX_LIGHTS][3], lcol[GVT_HIP_VOLUME_MAX_LIGHTS][3]; // as SurfDev's
  int n_lights;
  float ka, kd;
};
// ... and what the _central entry points receive beside their table: the six face layers beyond the brick, samples of the brick's voxel
// type in one allocation (-x +x: ny*nz each at j + ny*k; -y +y: nx*nz at i + nx*k; -z +z: nx*ny at i + nx*j), and the global grid's size
struct GhostDev {
  const void *faces;
  int gnx, gny, gnz;
};
struct NoGhost {};
template <bool CENTRAL>
using GhostTable = std::conditional_t<CENTRAL, GhostDev, NoGhost>;
template <bool SURF, bool LIT>
using MarchTable = std::conditional_t<SURF, SurfDev, std::conditional_t<LIT, LightDev, NoSurf>>;
#define VOL_CELL_SKIP 0x10000u

__device__ inline void vol_point(const VolDev &V, const float o[3], const float d[3], int k, float p[3]) {
  const float t = (float)k * V.dt;
  p[0] = o[0] + d[0] * t; p[1] = o[1] + d[1] * t; p[2] = o[2] + d[2] * t;
}

__device__ inline unsigned surf_plane_sides(const SurfDev &S, const float p[3]) {
  unsigned m = 0u;
  for (int j = 0; j < S.n_pl; j++) {
    const float4 P = S.plane[j];
    if ((P.x * p[0] + P.y * p[1]) + P.z * p[2] >= P.w) m |= 1u << (S.n_iso + j);
  }
  return m;
}

// May the samples k+1 .. kj of a ray go unvisited as far as the planes are concerned?  Only if every plane's field at k and at kj has the
// same sign and lies further from zero than twice a bound on its evaluation error (about 6 roundings of the terms below; 2^-18 leaves a
// factor 8): the exact field is linear in t, so every sample between them then evaluates to the same side.
__device__ inline bool surf_planes_clear(const VolDev &V, const SurfDev &S, const float o[3], const float d[3], int k, int kj) {
  float pa[3], pb[3];
  vol_point(V, o, d, k, pa);
  vol_point(V, o, d, kj, pb);
  const float T = (float)kj * V.dt;
  const float ext[3] = { fabsf(o[0]) + fabsf(d[0]) * T, fabsf(o[1]) + fabsf(d[1]) * T, fabsf(o[2]) + fabsf(d[2]) * T };
  bool clear = true;
  for (int j = 0; j < S.n_pl; j++) {
    const float4 P = S.plane[j];
    const float ma = ((P.x * pa[0] + P.y * pa[1]) + P.z * pa[2]) - P.w, mb = ((P.x * pb[0] + P.y * pb[1]) + P.z * pb[2]) - P.w;
    const float e2 = (((fabsf(P.x) * ext[0] + fabsf(P.y) * ext[1]) + fabsf(P.z) * ext[2]) + fabsf(P.w)) * (2.f / 262144.f);
    clear = clear && ((ma > e2 && mb > e2) || (ma < -e2 && mb < -e2)); // (false for NaN)
  }
  return clear;
}

// the table's colour at value v: the sample's own look-up, opacity in .w
__device__ inline float4 vol_lookup(const VolDev &V, float v) {
  const float pos = fminf(fmaxf((v - V.vlo) / V.vspan, 0.f), 1.f) * 255.f;
  const int i0 = min((int)pos, 254);
  const float w = pos - (float)i0;
  const float4 e0 = V.tf[i0], e1 = V.tf[i0 + 1];
  return make_float4(lerp_(e0.x, e1.x, w), lerp_(e0.y, e1.y, w), lerp_(e0.z, e1.z, w), lerp_(e0.w, e1.w, w));
}

// one crossed surface of base colour c and (unnormalised) normal g, composited in front of the sample
__device__ inline void surf_composite(const SurfDev &S, float4 c, const float g[3], float C[3], float &A) {
  float rgb[3] = { c.x, c.y, c.z };
  if (S.n_lights > 0) {
    float sum[3] = { 0.f, 0.f, 0.f };
    const float len = sqrtf((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]);
    if (len > 0.f) { // (false for NaN)
      const float n[3] = { g[0] / len, g[1] / len, g[2] / len };
      for (int j = 0; j < S.n_lights; j++) {
        const float ndl = fabsf((n[0] * S.ldir[j][0] + n[1] * S.ldir[j][1]) + n[2] * S.ldir[j][2]);
        for (int a = 0; a < 3; a++) sum[a] = sum[a] + S.lcol[j][a] * ndl;
      }
    }
    for (int a = 0; a < 3; a++) rgb[a] = rgb[a] * (S.ka + S.kd * sum[a]);
  }
  const float f = (1.f - A) * S.alpha;
  C[0] = C[0] + f * rgb[0]; C[1] = C[1] + f * rgb[1]; C[2] = C[2] + f * rgb[2];
  A = A + f;
}

// ---- the steps of the march.  Each is parity critical (the checkers compare bit for bit) and exists once.

// ray (a = origin | t_min, b = direction) into the brick's object space, and the lattice range k .. k_hi its visit walks (k_hi < k:
// none).  CLIP (the launches that may hold clipped rays): flags = the ray's depth word, and with GVT_HIP_RAY_CLIP in it the range ends
// at the last sample in front of t_max (b.w).  Returns the first lattice index after t_min.
template <bool CLIP>
__device__ __forceinline__ int vol_ray_range(const VolDev &V, const Mat4 &minv, float4 a, float4 b, int flags, float o[3], float d[3], int &k, int &k_hi) {
  const V3 oo = xfm_point(minv, mk3(a.x, a.y, a.z)), dd = xfm_vector(minv, mk3(b.x, b.y, b.z));
  o[0] = oo.x; o[1] = oo.y; o[2] = oo.z; d[0] = dd.x; d[1] = dd.y; d[2] = dd.z;
  float tn, tf;
  vol_slab(V.lo, V.hi, o, d, tn, tf);
  const int k_prog = vol_first_after(a.w, V.dt);
  k = 0;
  k_hi = -1;
  if (tn <= tf && tf >= 0.f && tf < INFINITY && k_prog >= 0) {
    const float qlo = floorf(tn / V.dt), qhi = floorf(tf / V.dt);
    if (qlo < VOL_K_MAX) {
      k = max(k_prog, qlo > 1.f ? (int)qlo - 1 : 0);
      k_hi = qhi < VOL_K_MAX ? (int)qhi + 1 : (int)VOL_K_MAX;
      k_hi = min(k_hi, k + VOL_MAX_SAMPLES);
      if constexpr (CLIP)
        if (flags & GVT_HIP_RAY_CLIP) k_hi = min(k_hi, vol_last_before(b.w, V.dt));
    }
  }
  return k_prog;
}

// Sample k lies in cell c, whose macro cell needs no interpolation: the last sample kj > k + 1 still inside that macro cell, or k where
// there is none.  Verified, so exact whatever the estimate (per axis the cells move monotonically with k: two samples in one block
// have every sample between them in it too).
__device__ __forceinline__ int vol_jump_target(const VolDev &V, const float o[3], const float d[3], int k, int k_hi, const int c[3]) {
  const int cb[3] = { c[0] >> 3, c[1] >> 3, c[2] >> 3 };
  const int off[3] = { V.ox, V.oy, V.oz }, nn[3] = { V.nx, V.ny, V.nz };
  const float go[3] = { V.gox, V.goy, V.goz }, sp[3] = { V.sx, V.sy, V.sz };
  float te = INFINITY;
  for (int a = 0; a < 3; a++) {
    if (d[a] == 0.f) continue;
    const int gv = d[a] > 0.f ? off[a] + min(8 * cb[a] + 8, nn[a] - 1) : off[a] + 8 * cb[a];
    te = fminf(te, ((go[a] + (float)gv * sp[a]) - o[a]) / d[a]);
  }
  const float qj = floorf(te / V.dt);
  if (qj < VOL_K_MAX && qj > (float)(k + 1)) {
    const int kj = min((int)qj, k_hi);
    int cj[3];
    float fj[3];
    if (kj > k + 1 && vol_cell(V, o, d, kj, cj, fj) && (cj[0] >> 3) == cb[0] && (cj[1] >> 3) == cb[1] && (cj[2] >> 3) == cb[2]) return kj;
  }
  return k;
}

// the eight vertices of cell c and the trilinear value at the fractions f
struct VolCorners { float v000, v100, v010, v110, v001, v101, v011, v111; };
// (T: the voxel type.  A vertex's value is (float)v, exact for every 8- and 16-bit integer, so what follows the loads is the same whatever T)
// (the compiler merges the two x-neighbours of a row into one load for every T -- 8, 2 or 4 bytes at T's alignment -- so the pair is not
// written out here; no load is wider than the pair, which lies inside its row: profiles/volume_types.txt)
template <typename T>
__device__ __forceinline__ float vol_gather(const VolDev &V, const int c[3], const float f[3], VolCorners &G) {
  const size_t sy = (size_t)V.nx, sz = (size_t)V.nx * (size_t)V.ny;
  const T *p = (const T *)V.vox + (size_t)c[0] + sy * (size_t)c[1] + sz * (size_t)c[2];
  G.v000 = (float)p[0]; G.v100 = (float)p[1]; G.v010 = (float)p[sy]; G.v110 = (float)p[sy + 1];
  G.v001 = (float)p[sz]; G.v101 = (float)p[sz + 1]; G.v011 = (float)p[sz + sy]; G.v111 = (float)p[sz + sy + 1];
  const float c00 = lerp_(G.v000, G.v100, f[0]), c10 = lerp_(G.v010, G.v110, f[0]);
  const float c01 = lerp_(G.v001, G.v101, f[0]), c11 = lerp_(G.v011, G.v111, f[0]);
  const float c0 = lerp_(c00, c10, f[1]), c1 = lerp_(c01, c11, f[1]);
  return lerp_(c0, c1, f[2]);
}

// the sample of value v, front to back
__device__ __forceinline__ void vol_accumulate(const VolDev &V, float v, float C[3], float &A) {
  const float4 tc = vol_lookup(V, v);
  const float fr = (1.f - A) * tc.w;
  C[0] = C[0] + fr * tc.x; C[1] = C[1] + fr * tc.y; C[2] = C[2] + fr * tc.z;
  A = A + fr;
}

// the gradient of the trilinear interpolant of cell G at the fractions f: the contract's three expressions, for the lit sample.  (The
// crossing in volume_march_body keeps its own statement of them: routed through here, the unlit surface kernels schedule a handful of
// instructions differently, and they are to stay what they were -- profiles/volume_shade.txt)
__device__ __forceinline__ void vol_gradient(const VolDev &V, const VolCorners &G, const float f[3], float g[3]) {
  g[0] = lerp_(lerp_(G.v100 - G.v000, G.v110 - G.v010, f[1]), lerp_(G.v101 - G.v001, G.v111 - G.v011, f[1]), f[2]) / V.sx;
  g[1] = lerp_(lerp_(G.v010 - G.v000, G.v110 - G.v100, f[0]), lerp_(G.v011 - G.v001, G.v111 - G.v101, f[0]), f[2]) / V.sy;
  g[2] = lerp_(lerp_(G.v001 - G.v000, G.v101 - G.v100, f[0]), lerp_(G.v011 - G.v010, G.v111 - G.v110, f[0]), f[1]) / V.sz;
}

// GVT_HIP_VOLUME_GRADIENT_CENTRAL: central differences at the cell's eight vertices, interpolated trilinearly (the contract: include/
// gvt_hip.h, "smooth gradients"; tests/volume_smooth_checker.py).  Per axis the vertex before the cell and the one after it, at the four
// positions of the other two axes: inside the brick they are its own samples, one layer beyond a face the ghost layer's, and on the
// global boundary the difference is one-sided (the cell's own corner, half the span).  The guards differ from lane to lane; the loads
// are eight per axis, beside the corners the gather has left in G.  A: the axis, with B and C the other two in x y z order.
template <typename T, int A>
__device__ __forceinline__ float vol_central_axis(const VolDev &V, const GhostDev &H, const int c[3], const float lo[4], const float hi[4], const float f[3]) {
  constexpr int B = A == 0 ? 1 : 0, C = A == 2 ? 1 : 2;
  const int n[3] = { V.nx, V.ny, V.nz }, off[3] = { V.ox, V.oy, V.oz }, gn[3] = { H.gnx, H.gny, H.gnz };
  const float sp[3] = { V.sx, V.sy, V.sz };
  const size_t str[3] = { 1, (size_t)V.nx, (size_t)V.nx * (size_t)V.ny };
  const size_t slab[3] = { (size_t)V.ny * (size_t)V.nz, (size_t)V.nx * (size_t)V.nz, (size_t)V.nx * (size_t)V.ny };
  // a face layer's strides along B and C: x faces (j + ny*k), y faces (i + nx*k), z faces (i + nx*j)
  const size_t fb = 1, fc = (size_t)n[B];
  const T *face = (const T *)H.faces + (A > 0 ? 2 * slab[0] : 0) + (A > 1 ? 2 * slab[1] : 0);
  const size_t in_brick = (size_t)c[0] + str[1] * (size_t)c[1] + str[2] * (size_t)c[2], in_face = fb * (size_t)c[B] + fc * (size_t)c[C];
  float m[4], p[4];        // the vertex before the cell's low corners, and the one after its high corners
  float dm = 2.f, dp = 2.f; // (float)(ip - im) of the low and of the high vertices
  if (off[A] + c[A] == 0) { // the low vertices lie on the global boundary: im = i
    for (int q = 0; q < 4; q++) m[q] = lo[q];
    dm = 1.f;
  } else {
    const bool own = c[A] > 0;
    const T *b = own ? (const T *)V.vox + (in_brick - str[A]) : face + in_face;
    const size_t s1 = own ? str[B] : fb, s2 = own ? str[C] : fc;
    m[0] = (float)b[0]; m[1] = (float)b[s1]; m[2] = (float)b[s2]; m[3] = (float)b[s1 + s2];
  }
  if (off[A] + c[A] + 1 == gn[A] - 1) { // the high vertices lie on it: ip = i
    for (int q = 0; q < 4; q++) p[q] = hi[q];
    dp = 1.f;
  } else {
    const bool own = c[A] + 2 < n[A];
    const T *b = own ? (const T *)V.vox + (in_brick + 2 * str[A]) : face + slab[A] + in_face;
    const size_t s1 = own ? str[B] : fb, s2 = own ? str[C] : fc;
    p[0] = (float)b[0]; p[1] = (float)b[s1]; p[2] = (float)b[s2]; p[3] = (float)b[s1 + s2];
  }
  const float hm = sp[A] * dm, hp = sp[A] * dp;
  float gl[4], gh[4]; // the component at the low and at the high vertices
  for (int q = 0; q < 4; q++) { gl[q] = (hi[q] - m[q]) / hm; gh[q] = (p[q] - lo[q]) / hp; }
  // vol_gather's nesting: x, then y, then z.  q = (B bit) + 2 * (C bit)
  if constexpr (A == 0) return lerp_(lerp_(lerp_(gl[0], gh[0], f[0]), lerp_(gl[1], gh[1], f[0]), f[1]), lerp_(lerp_(gl[2], gh[2], f[0]), lerp_(gl[3], gh[3], f[0]), f[1]), f[2]);
  else if constexpr (A == 1) return lerp_(lerp_(lerp_(gl[0], gl[1], f[0]), lerp_(gh[0], gh[1], f[0]), f[1]), lerp_(lerp_(gl[2], gl[3], f[0]), lerp_(gh[2], gh[3], f[0]), f[1]), f[2]);
  else return lerp_(lerp_(lerp_(gl[0], gl[1], f[0]), lerp_(gl[2], gl[3], f[0]), f[1]), lerp_(lerp_(gh[0], gh[1], f[0]), lerp_(gh[2], gh[3], f[0]), f[1]), f[2]);
}
template <typename T>
__device__ __forceinline__ void vol_gradient_central(const VolDev &V, const GhostDev &H, const int c[3], const VolCorners &G, const float f[3], float g[3]) {
  { const float lo[4] = { G.v000, G.v010, G.v001, G.v011 }, hi[4] = { G.v100, G.v110, G.v101, G.v111 }; g[0] = vol_central_axis<T, 0>(V, H, c, lo, hi, f); }
  { const float lo[4] = { G.v000, G.v100, G.v001, G.v101 }, hi[4] = { G.v010, G.v110, G.v011, G.v111 }; g[1] = vol_central_axis<T, 1>(V, H, c, lo, hi, f); }
  { const float lo[4] = { G.v000, G.v100, G.v010, G.v110 }, hi[4] = { G.v001, G.v101, G.v011, G.v111 }; g[2] = vol_central_axis<T, 2>(V, H, c, lo, hi, f); }
}

// vol_accumulate for a lit volume (L: SurfDev or LightDev, n_lights > 0): a sample the table gives opacity is shaded by the gradient in its
// own cell; one of zero opacity adds +0 whatever its colour, so it is neither shaded nor counted.  Unlike surf_composite, a gradient of
// infinite length shades with S = 0 (g / Inf would be 0 or NaN): C stays finite on grids whose differences overflow.  Returns 1 if shaded
template <typename T, bool CENTRAL, typename LT>
__device__ __forceinline__ unsigned vol_accumulate_lit(const VolDev &V, const LT &L, const GhostTable<CENTRAL> &H, const int c[3], float v, const VolCorners &G,
                                                       const float f[3], float C[3], float &A) {
  const float4 tc = vol_lookup(V, v);
  float rgb[3] = { tc.x, tc.y, tc.z };
  const bool shaded = tc.w > 0.f; // (false for NaN)
  if (shaded) {
    float g[3], sum[3] = { 0.f, 0.f, 0.f };
    if constexpr (CENTRAL) vol_gradient_central<T>(V, H, c, G, f, g);
    else vol_gradient(V, G, f, g);
    const float len = sqrtf((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]);
    if (len > 0.f && len < INFINITY) { // (false for NaN)
      const float n[3] = { g[0] / len, g[1] / len, g[2] / len };
      for (int j = 0; j < L.n_lights; j++) {
        const float ndl = fabsf((n[0] * L.ldir[j][0] + n[1] * L.ldir[j][1]) + n[2] * L.ldir[j][2]);
        for (int a = 0; a < 3; a++) sum[a] = sum[a] + L.lcol[j][a] * ndl;
      }
    }
    for (int a = 0; a < 3; a++) rgb[a] = rgb[a] * (L.ka + L.kd * sum[a]);
  }
  const float fr = (1.f - A) * tc.w;
  C[0] = C[0] + fr * rgb[0]; C[1] = C[1] + fr * rgb[1]; C[2] = C[2] + fr * rgb[2];
  A = A + fr;
  return shaded ? 1u : 0u;
}

// the ray leaves the brick: t_min = its last sample here (k_last < 0: it had none), colour, opacity and flags; with surfaces the sides
// of that sample too
template <bool SURF>
__device__ __forceinline__ void vol_write_back(const VolDev &V, RayPlanes q, unsigned idx, int k_last, const float C[3], float A, int prev) {
  float4 a = q.p0[idx];
  int flag = A >= GVT_HIP_VOLUME_OPAQUE_A ? GVT_HIP_RAY_OPAQUE : GVT_HIP_RAY_BOUNDARY;
  if (k_last >= 0) a.w = (float)k_last * V.dt;
  q.p0[idx] = a;
  float cw = q.p2[idx].w;
  if constexpr (SURF)
    if (k_last >= 0) { cw = (float)prev; flag |= GVT_HIP_RAY_SIDES; } // (prev = the sides of sample k_last)
  q.p2[idx] = make_float4(C[0], C[1], C[2], cw);
  float4 e = q.p3[idx];
  e.y = __int_as_float(__float_as_int(e.y) | flag);
  e.z = A;
  q.p3[idx] = e;
}

// One lane per ray, persistent waves with lane refill: a lane that finishes its ray takes the next one of the queue (one atomic per wave
// and refill).  Rays are updated in place.  SURF (volumes that have surfaces): per sample the side mask, at a crossing the shaded
// surfaces before the sample's own contribution.  prev < 0: no previous sample.  CLIP: the launch may hold rays that carry
// GVT_HIP_RAY_CLIP (vol_ray_range); without it the body is the unclipped march, instruction for instruction, and no ray is flagged.
// LIT (shading on and at least one light): the sample's own contribution is vol_accumulate_lit's, from the corners the gather has just
// loaded -- they stay live across the look-up; with SURF a crossing is rendered first, as ever.  Without LIT: the march as it was.
// CENTRAL (the _central entry points): the gradient of a crossed isovalue and of a lit sample is vol_gradient_central's, from H; nothing
// else of the march reads H or depends on the kind.
// KEEP IN STEP: k_volume_march_fused_shaded (volume_fused_shaded.inc) restates the per-sample steps of the loop below for SURF / LIT,
// with and without CENTRAL; a change to the visit here is a change there.
template <typename T, bool SURF, bool CLIP, bool LIT, bool CENTRAL = false>
__device__ __forceinline__ void volume_march_body(const VolDev &V, const MarchTable<SURF, LIT> &S, const GhostTable<CENTRAL> &H, RayPlanes q, unsigned n, const Mat4 &minv,
                                                  unsigned *__restrict__ work, unsigned long long *__restrict__ stats) {
  bool active = false, exhausted = false;
  unsigned idx = 0;
  float o[3] = { 0.f, 0.f, 0.f }, d[3] = { 0.f, 0.f, 0.f }, C[3] = { 0.f, 0.f, 0.f }, A = 0.f;
  int k = 0, k_hi = -1, k_last = -1, k_carry = -1, prev = -1; // (k_carry, prev, n_crossed: SURF only)
  bool seen = false;
  unsigned long long n_marched = 0, n_gathered = 0;
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
          if (seen) { done = true; break; } // a brick's samples along a line are contiguous: the rest belongs to others
          k++;
          continue;
        }
        if constexpr (SURF)
          if (!seen && k != k_carry) prev = -1;
        seen = true;
        k_last = k;
        n_marched++;
        const int bi = ((c[2] >> 3) * V.nby + (c[1] >> 3)) * V.nbx + (c[0] >> 3);
        // Plain: an empty macro cell adds +0 per sample.  SURF: nothing to composite there and no crossing either, as long as no plane
        // can change sides among the samples (the isovalue sides are the cell's).  The sample goes uninterpolated, and so do those
        // after it in this macro cell
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
          skip = V.skip && !V.mc[bi];
        }
        if (skip) {
          if (A >= GVT_HIP_VOLUME_OPAQUE_A) { k++; done = true; break; } // the ray arrived opaque: this sample adds +0 and ends it, as any sample does
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
        VolCorners G;
        const float v = vol_gather<T>(V, c, f, G);
        if constexpr (SURF) {
          unsigned sides = pl;
          for (int i = 0; i < S.n_iso; i++)
            if (v >= S.iso[i]) sides |= 1u << i;
          unsigned crossed = prev < 0 ? 0u : (sides ^ (unsigned)prev);
          prev = (int)sides;
          if (crossed) {
            const float v000 = G.v000, v100 = G.v100, v010 = G.v010, v110 = G.v110, v001 = G.v001, v101 = G.v101, v011 = G.v011, v111 = G.v111;
            float gc[3] = { 0.f, 0.f, 0.f }; // (CENTRAL only: the isovalues crossed here share one gradient, fetched once, ahead of the loop)
            if constexpr (CENTRAL)
              if (crossed & ((1u << S.n_iso) - 1u)) vol_gradient_central<T>(V, H, c, G, f, gc);
            while (crossed && A < GVT_HIP_VOLUME_OPAQUE_A) {
              const int i = __ffs((int)crossed) - 1;
              crossed &= crossed - 1u;
              n_crossed++;
              if (i < S.n_iso) {
                if constexpr (CENTRAL) {
                  surf_composite(S, vol_lookup(V, S.iso[i]), gc, C, A);
                  continue;
                }
                const float g[3] = { lerp_(lerp_(v100 - v000, v110 - v010, f[1]), lerp_(v101 - v001, v111 - v011, f[1]), f[2]) / V.sx,
                                     lerp_(lerp_(v010 - v000, v110 - v100, f[0]), lerp_(v011 - v001, v111 - v101, f[0]), f[2]) / V.sy,
                                     lerp_(lerp_(v001 - v000, v101 - v100, f[0]), lerp_(v011 - v010, v111 - v110, f[0]), f[1]) / V.sz };
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
        if constexpr (LIT) n_shaded += vol_accumulate_lit<T, CENTRAL>(V, S, H, c, v, G, f, C, A);
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
    if constexpr (SURF) n_cr += __shfl_xor(n_cr, s);
    if constexpr (LIT) n_shaded += __shfl_xor(n_shaded, s);
  }
  if (lane_id() == 0 && n_marched) {
    atomicAdd(&stats[0], n_marched);
    atomicAdd(&stats[1], n_gathered);
    if constexpr (SURF)
      if (n_cr) atomicAdd(&stats[2], n_cr);
    if constexpr (LIT)
      if (n_shaded) atomicAdd(&stats[3], n_shaded);
  }
}

// The entry points, per voxel type.  The plain one does not receive SurfDev: the table is about 600 bytes of kernel arguments, and its
// scalar registers are full as it is.  The lit plain one receives the lights alone (LightDev); the lit surface one finds them in SurfDev.
template <typename T, bool CLIP>
__global__ __launch_bounds__(VOL_BLOCK) void k_volume_march(VolDev V, RayPlanes q, unsigned n, Mat4 minv, unsigned *__restrict__ work,
                                                            unsigned long long *__restrict__ stats) {
  volume_march_body<T, false, CLIP, false>(V, NoSurf{}, NoGhost{}, q, n, minv, work, stats);
}
template <typename T, bool CLIP>
__global__ __launch_bounds__(VOL_BLOCK) void k_volume_march_surf(VolDev V, SurfDev S, RayPlanes q, unsigned n, Mat4 minv, unsigned *__restrict__ work,
                                                                 unsigned long long *__restrict__ stats) {
  volume_march_body<T, true, CLIP, false>(V, S, NoGhost{}, q, n, minv, work, stats);
}
template <typename T, bool CLIP>
__global__ __launch_bounds__(VOL_BLOCK) void k_volume_march_lit(VolDev V, LightDev L, RayPlanes q, unsigned n, Mat4 minv, unsigned *__restrict__ work,
                                                                unsigned long long *__restrict__ stats) {
  volume_march_body<T, false, CLIP, true>(V, L, NoGhost{}, q, n, minv, work, stats);
}
template <typename T, bool CLIP>
__global__ __launch_bounds__(VOL_BLOCK) void k_volume_march_surf_lit(VolDev V, SurfDev S, RayPlanes q, unsigned n, Mat4 minv, unsigned *__restrict__ work,
                                                                     unsigned long long *__restrict__ stats) {
  volume_march_body<T, true, CLIP, true>(V, S, NoGhost{}, q, n, minv, work, stats);
}

// ... and the three shaded marches with GVT_HIP_VOLUME_GRADIENT_CENTRAL: the same body, with the ghost table
template <typename T, bool CLIP>
__global__ __launch_bounds__(VOL_BLOCK) void k_volume_march_surf_central(VolDev V, SurfDev S, GhostDev H, RayPlanes q, unsigned n, Mat4 minv,
                                                                         unsigned *__restrict__ work, unsigned long long *__restrict__ stats) {
  volume_march_body<T, true, CLIP, false, true>(V, S, H, q, n, minv, work, stats);
}
template <typename T, bool CLIP>
__global__ __launch_bounds__(VOL_BLOCK) void k_volume_march_lit_central(VolDev V, LightDev L, GhostDev H, RayPlanes q, unsigned n, Mat4 minv,
                                                                        unsigned *__restrict__ work, unsigned long long *__restrict__ stats) {
  volume_march_body<T, false, CLIP, true, true>(V, L, H, q, n, minv, work, stats);
}
template <typename T, bool CLIP>
__global__ __launch_bounds__(VOL_BLOCK) void k_volume_march_surf_lit_central(VolDev V, SurfDev S, GhostDev H, RayPlanes q, unsigned n, Mat4 minv,
                                                                             unsigned *__restrict__ work, unsigned long long *__restrict__ stats) {
  volume_march_body<T, true, CLIP, true, true>(V, S, H, q, n, minv, work, stats);
}

// ---- shuffleRays, volume branch.  Destinations are counted per (wave, destination) in LDS and a scan per destination gives every block
// its first slot, so the queues keep the order of the list they were filled from.
// clip: the ray is clipped at t_clip (GVT_HIP_RAY_CLIP and its t_max): a box it enters at or behind t_clip holds no sample of its
__device__ inline int vol_next(const TopDev &T, int from, const float o[3], const float d[3], float t_min, bool clip, float t_clip) {
  float p = t_min;
  if (from >= 0) { // progress = the exit of the source box (world space, the test below): it grows strictly from hop to hop
    for (int j = 0; j < T.n_inst; j++) {
      const float4 lo = T.blo[j], hi = T.bhi[j];
      if (__float_as_int(lo.w) != from) continue;
      const float l[3] = { lo.x, lo.y, lo.z }, h[3] = { hi.x, hi.y, hi.z };
      float tn;
      vol_slab(l, h, o, d, tn, p);
    }
  }
  int next = -1;
  float best = INFINITY;
  for (int j = 0; j < T.n_inst; j++) { // in the top's order: equal entries resolve to the first
    const float4 lo = T.blo[j], hi = T.bhi[j];
    const int inst = __float_as_int(lo.w);
    if (inst == from) continue;
    const float l[3] = { lo.x, lo.y, lo.z }, h[3] = { hi.x, hi.y, hi.z };
    float tn, tf;
    vol_slab(l, h, o, d, tn, tf);
    if (tn <= tf && tf > p && (!clip || tn < t_clip) && (next < 0 || tn < best)) { next = inst; best = tn; } // (tn < NaN: false)
  }
  return next;
}

// MASK (gvt_hip_volume_camera_filter, from < 0): a camera ray whose first brick b has keep[b] == 0 is dropped (shuffleDropRays: b's owner
// generates the same ray); the unmasked instantiation is the kernel as it was and never reads keep
template <bool MASK>
__global__ __launch_bounds__(VOL_BLOCK) void k_vol_classify(RayPlanes q, unsigned n, TopDev T, int n_dest, int from, int *__restrict__ next_out,
                                                            unsigned *__restrict__ blk_cnt, float *__restrict__ fb, unsigned n_pix,
                                                            const float *__restrict__ clip_plane, unsigned n_clip, const unsigned char *__restrict__ keep) {
  __shared__ unsigned sh[VOL_DEST_MAX];
  for (int j = threadIdx.x; j < n_dest; j += VOL_BLOCK) sh[j] = 0u;
  __syncthreads();
  const unsigned i = blockIdx.x * VOL_BLOCK + threadIdx.x;
  int next = -1;
  if (i < n) {
    const float4 a = q.p0[i], b = q.p1[i], e = q.p3[i];
    const float o[3] = { a.x, a.y, a.z }, d[3] = { b.x, b.y, b.z };
    const int depth = __float_as_int(e.y);
    bool deposit = false;
    bool clip = (depth & GVT_HIP_RAY_CLIP) != 0;
    float t_clip = b.w;
    if (clip_plane) { // the clipped frame's camera rays (from < 0): what k_vol_scatter is about to give them
      const unsigned id = (unsigned)__float_as_int(e.x);
      t_clip = id < n_clip ? clip_plane[id] : INFINITY;
      clip = t_clip < INFINITY;
    }
    if (from < 0) { // camera rays: no deposit where they meet no brick
      next = vol_next(T, -1, o, d, a.w, clip, t_clip);
      if (MASK && next >= 0 && !keep[next]) next = -1;
    }
    else if (depth & GVT_HIP_RAY_OPAQUE) deposit = true;
    else if (depth & GVT_HIP_RAY_BOUNDARY) {
      next = vol_next(T, from, o, d, a.w, clip, t_clip);
      deposit = next < 0; // EXTERNAL: the ray leaves the volume
    }
    if (deposit && fb) {
      const unsigned id = (unsigned)__float_as_int(e.x);
      if (id < n_pix) {
        const float4 c = q.p2[i];
        float *px = fb + (size_t)4 * id;
        atomicAdd(px + 0, c.x); atomicAdd(px + 1, c.y); atomicAdd(px + 2, c.z); atomicAdd(px + 3, e.z);
      }
    }
    next_out[i] = next;
  }
  wave_by_dest(next, [&](int dd, unsigned long long m, int leader) {
    if ((int)lane_id() == leader) atomicAdd(&sh[dd], (unsigned)__popcll(m));
  });
  __syncthreads();
  for (int j = threadIdx.x; j < n_dest; j += VOL_BLOCK) blk_cnt[(size_t)j * gridDim.x + blockIdx.x] = sh[j];
}

#include "ordered_scan.inc" // k_dest_scan: every block's first slot per destination; totals[j] = the rays it receives

// fresh (camera rays): they start with no colour, no opacity and no flags; fresh == 2 (the clipped frame): ... and with t_max = their
// pixel's depth and GVT_HIP_RAY_CLIP where that is below +Inf
__global__ __launch_bounds__(VOL_BLOCK) void k_vol_scatter(RayPlanes q, unsigned n, const int *__restrict__ next_in, const unsigned *__restrict__ blk_base,
                                                           const QueueDesc *__restrict__ queues, int n_dest, int fresh, unsigned *__restrict__ overflow,
                                                           const float *__restrict__ clip_plane, unsigned n_clip) {
  __shared__ unsigned sh[(VOL_BLOCK / 64) * VOL_DEST_MAX]; // rays of wave w for destination j
  for (int x = threadIdx.x; x < (VOL_BLOCK / 64) * n_dest; x += VOL_BLOCK) sh[x] = 0u;
  __syncthreads();
  const unsigned i = blockIdx.x * VOL_BLOCK + threadIdx.x;
  const int next = i < n ? next_in[i] : -1;
  unsigned local = 0;
  wave_by_dest(next, [&](int dd, unsigned long long m, int leader) {
    if ((int)lane_id() == leader) sh[(threadIdx.x >> 6) * n_dest + dd] = (unsigned)__popcll(m);
    if (next == dd) local = lanes_below(m);
  });
  __syncthreads();
  if (next < 0) return;
  for (unsigned w = 0; w < (threadIdx.x >> 6); w++) local += sh[w * n_dest + next];
  local += blk_base[(size_t)next * gridDim.x + blockIdx.x];
  RayRec r = load_ray(q, i);
  r.depth &= ~GVT_HIP_RAY_BOUNDARY;
  if (fresh) { r.c = mk3(0.f, 0.f, 0.f); r.w = 0.f; r.depth = 0; }
  if (fresh == 2 && (unsigned)r.id < n_clip) {
    r.t_max = clip_plane[(unsigned)r.id];
    r.depth = r.t_max < INFINITY ? GVT_HIP_RAY_CLIP : 0;
  }
  const QueueDesc Q = queues[next];
  if (local < Q.cap) store_ray(make_planes(Q.planes, Q.cap), local, r);
  else atomicOr(overflow, 1u);
}


// ---- macro-cell value ranges.  A macro cell is 8^3 cells = up to 9^3 vertices, clipped at the brick's last vertex; a vertex on a block
// boundary is a corner of cells on both sides and counts for both blocks.  Per macro cell: the minimum and the maximum of its vertices that
// are not NaN (none: +Inf and -Inf stay) and whether a vertex is NaN or +-Inf.
// One block per run of VR_CELLS macro cells along x, for one (by, bz): a wave reads whole rows of the grid, a lane 4 consecutive vertices
// (one 16-byte load where every row starts 16-byte aligned: nx % 4 == 0, VEC), the block's waves take the run's (up to) 81 rows in turn.
// Macro cell c of the run is lanes 2c and 2c + 1 and the first vertex of lane 2c + 2 (shuffles), then the waves (LDS); the run's last
// boundary vertex, x0 + 8 * VR_CELLS, belongs to the next run's lane 0 and is read here one scalar per row.  The alternative, a block
// per macro cell, reads 9-float row fragments (36 of every 64-byte sector pair); this reads every row of a run once in full and the
// boundary rows (y or z a multiple of 8) by two blocks: 81 / 64 = 1.27 of the grid's bytes, the second reading mostly from L2.
// Every output has ONE writer and no atomics.  min and max are exact, so the order of the reduction cannot change a value; ranges are
// compared as values, so between -0 and +0 either may come out: block_is_ranged, rebuild_tables' entry() and upload_cells use them
// numerically only.
#define VR_CELLS 32
static_assert(8 * VR_CELLS == 4 * 64, "a wave's 64 lanes of 4 vertices cover the run's cells");

struct VRange { float mn, mx; unsigned wild; };
__device__ inline VRange vr_none() { return VRange{ INFINITY, -INFINITY, 0u }; }
// NaN is tested for, not left to fminf / fmaxf: it sets the flag and enters neither bound; +-Inf sets the flag and enters
__device__ inline void vr_add(VRange &r, float v) {
  const bool nan = v != v;
  if (!nan) { if (v < r.mn) r.mn = v; if (v > r.mx) r.mx = v; }
  if (nan || v == INFINITY || v == -INFINITY) r.wild = 1u;
}
__device__ inline void vr_merge(VRange &r, const VRange &o) { // (bounds are never NaN)
  if (o.mn < r.mn) r.mn = o.mn;
  if (o.mx > r.mx) r.mx = o.mx;
  r.wild |= o.wild;
}
__device__ inline VRange vr_shfl_down(const VRange &r, int d) { return VRange{ __shfl_down(r.mn, d), __shfl_down(r.mx, d), __shfl_down(r.wild, d) }; }
__device__ inline VRange vr_wave_all(VRange r) { // every lane: the wave's range
  for (int d = 32; d; d >>= 1) vr_merge(r, VRange{ __shfl_xor(r.mn, d), __shfl_xor(r.mx, d), __shfl_xor(r.wild, d) });
  return r;
}

// four consecutive vertices of a row as ONE load of 4 * sizeof(T) bytes (4, 8 or 16)
template <typename T> struct alignas(4 * sizeof(T)) Vox4 { T v[4]; };

template <typename T, bool VEC>
__global__ __launch_bounds__(VOL_BLOCK) void k_vol_ranges(const T *__restrict__ vox, unsigned nx, unsigned ny, unsigned nz, unsigned nbx, unsigned nby,
                                                          unsigned runs, size_t n_work, float *__restrict__ bmin, float *__restrict__ bmax,
                                                          uint8_t *__restrict__ bnan) {
  constexpr int WAVES = VOL_BLOCK / 64;
  __shared__ float s_mn[WAVES][VR_CELLS], s_mx[WAVES][VR_CELLS], s_emn[WAVES], s_emx[WAVES];
  __shared__ unsigned s_w[WAVES][VR_CELLS], s_ew[WAVES];
  const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  for (size_t id = blockIdx.x; id < n_work; id += gridDim.x) { // (block-uniform)
    const unsigned run = (unsigned)(id % runs), by = (unsigned)((id / runs) % nby), bz = (unsigned)(id / ((size_t)runs * nby));
    const unsigned x0 = run * (8u * VR_CELLS), y0 = 8u * by, z0 = 8u * bz;
    const unsigned ry = min(9u, ny - y0), rz = min(9u, nz - z0), rows = ry * rz;
    const unsigned x = x0 + 4u * lane;
    VRange first = vr_none(), all = vr_none(); // the lane's first vertex | all four
    if (x < nx)
      for (unsigned r = wave; r < rows; r += WAVES) {
        const T *row = vox + ((size_t)(z0 + r / ry) * ny + (y0 + r % ry)) * nx;
        if (VEC) { // nx % 4 == 0 and x % 4 == 0: x + 3 < nx, and row + x is a multiple of 4 vertices from the allocation's start
          const Vox4<T> v = *reinterpret_cast<const Vox4<T> *>(row + x);
          vr_add(first, (float)v.v[0]); vr_add(all, (float)v.v[1]); vr_add(all, (float)v.v[2]); vr_add(all, (float)v.v[3]);
        } else {
          vr_add(first, (float)row[x]);
          for (unsigned i = 1; i < 4u && x + i < nx; i++) vr_add(all, (float)row[x + i]);
        }
      }
    vr_merge(all, first);
    VRange edge = vr_none(); // the boundary vertex behind the run's last cell: one row per thread (rows <= 81)
    const unsigned xe = x0 + 8u * VR_CELLS;
    if (threadIdx.x < rows && xe < nx) vr_add(edge, (float)vox[((size_t)(z0 + threadIdx.x / ry) * ny + (y0 + threadIdx.x % ry)) * nx + xe]);
    edge = vr_wave_all(edge);
    VRange cell = all; // even lanes: macro cell lane / 2 of the run, this wave's rows
    const VRange right = vr_shfl_down(all, 1), corner = vr_shfl_down(first, 2);
    vr_merge(cell, right);
    if (lane + 2u < 64u) vr_merge(cell, corner);
    if (!(lane & 1u)) { s_mn[wave][lane >> 1] = cell.mn; s_mx[wave][lane >> 1] = cell.mx; s_w[wave][lane >> 1] = cell.wild; }
    if (lane == 0u) { s_emn[wave] = edge.mn; s_emx[wave] = edge.mx; s_ew[wave] = edge.wild; }
    __syncthreads();
    const unsigned bx = run * VR_CELLS + threadIdx.x;
    if (threadIdx.x < VR_CELLS && bx < nbx) { // the one writer of this macro cell
      VRange r = vr_none();
      for (int w = 0; w < WAVES; w++) vr_merge(r, VRange{ s_mn[w][threadIdx.x], s_mx[w][threadIdx.x], s_w[w][threadIdx.x] });
      if (threadIdx.x == VR_CELLS - 1)
        for (int w = 0; w < WAVES; w++) vr_merge(r, VRange{ s_emn[w], s_emx[w], s_ew[w] });
      const size_t b = ((size_t)bz * nby + by) * nbx + bx;
      bmin[b] = r.mn; bmax[b] = r.mx; bnan[b] = (uint8_t)r.wild;
    }
    __syncthreads(); // (the next round writes the LDS again)
  }
}

// the brick's range from its macro cells' (every vertex lies in one): ONE block of 1024 threads, four independent loads in flight per
// thread and array (the 262 K macro cells of a 512^3 grid are 64 rounds of them); out[0] = min, out[1] = max
#define VR_TOTAL_BLOCK 1024
__global__ __launch_bounds__(VR_TOTAL_BLOCK) void k_vol_range_total(const float *__restrict__ bmin, const float *__restrict__ bmax, size_t n, float *__restrict__ out) {
  __shared__ float s_mn[VR_TOTAL_BLOCK / 64], s_mx[VR_TOTAL_BLOCK / 64];
  VRange r = vr_none();
  size_t i = threadIdx.x;
  for (; i + 3 * (size_t)VR_TOTAL_BLOCK < n; i += 4 * (size_t)VR_TOTAL_BLOCK) {
    float lo[4], hi[4];
    for (int u = 0; u < 4; u++) { lo[u] = bmin[i + u * (size_t)VR_TOTAL_BLOCK]; hi[u] = bmax[i + u * (size_t)VR_TOTAL_BLOCK]; }
    for (int u = 0; u < 4; u++) vr_merge(r, VRange{ lo[u], hi[u], 0u });
  }
  for (; i < n; i += VR_TOTAL_BLOCK) vr_merge(r, VRange{ bmin[i], bmax[i], 0u });
  r = vr_wave_all(r);
  if ((threadIdx.x & 63u) == 0u) { s_mn[threadIdx.x >> 6] = r.mn; s_mx[threadIdx.x >> 6] = r.mx; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < VR_TOTAL_BLOCK / 64; w++) vr_merge(r, VRange{ s_mn[w], s_mx[w], 0u });
    out[0] = r.mn; out[1] = r.mx;
  }
}

#include "volume_amr.inc" // k_volume_march_amr, k_amr_ranges, k_amr_ranges_merge
#include "volume_fused.inc" // k_volume_march_fused
#include "volume_fused_shaded.inc" // k_volume_march_fused_shaded
#include "volume_fused_amr.inc" // k_volume_march_fused_amr, k_volume_march_fused_shaded_amr
#include "volume_fused_shadow.inc" // k_volume_march_fused_shadow
#include "volume_light_grid.inc" // k_volume_bake_light
#include "volume_fused_fog.inc" // k_volume_march_fused_fog
#include "volume_occluder_grid.inc" // k_occluder_rays, k_occluder_fold, k_occluder_pack
#include "volume_fused_mesh.inc" // k_volume_march_fused_mesh
#include "volume_ao_grid.inc" // k_volume_bake_ao
#include "volume_fused_ao.inc" // k_volume_march_fused_ao, k_volume_march_fused_ao_lean
#include "volume_fused_shadow_amr.inc" // k_volume_march_fused_shadow_amr, _fog_amr, _mesh_amr, the lean two, k_volume_bake_light_amr

inline unsigned blocks_of(size_t n) { return (unsigned)((n + VOL_BLOCK - 1) / VOL_BLOCK); }

// The voxel types: bytes per sample (0: unknown type), and THE place a run-time type picks a kernel instantiation: f receives a value of
// the voxel's C type.  volume_march and volume_ranges launch through it; nothing else reads d_vox.
inline size_t voxel_bytes(int type) {
  return type == GVT_HIP_VOXEL_F32 ? 4 : type == GVT_HIP_VOXEL_U8 ? 1 : (type == GVT_HIP_VOXEL_I16 || type == GVT_HIP_VOXEL_U16) ? 2 : 0;
}
template <typename Fn>
inline void with_voxel_type(int type, Fn f) {
  switch (type) {
    case GVT_HIP_VOXEL_U8: f(uint8_t{}); break;
    case GVT_HIP_VOXEL_I16: f(int16_t{}); break;
    case GVT_HIP_VOXEL_U16: f(uint16_t{}); break;
    default: f(float{}); break; // (create admits the four types only)
  }
}

VolDev vol_dev(const gvt_hip_volume *Vh) {
  VolDev V;
  V.vox = Vh->d_vox; V.tf = Vh->d_tf; V.mc = Vh->d_mc;
  V.nx = Vh->n[0]; V.ny = Vh->n[1]; V.nz = Vh->n[2]; V.ox = Vh->off[0]; V.oy = Vh->off[1]; V.oz = Vh->off[2];
  V.nbx = Vh->nb[0]; V.nby = Vh->nb[1];
  V.gox = Vh->go[0]; V.goy = Vh->go[1]; V.goz = Vh->go[2]; V.sx = Vh->sp[0]; V.sy = Vh->sp[1]; V.sz = Vh->sp[2]; V.dt = Vh->dt;
  for (int a = 0; a < 3; a++) { V.lo[a] = Vh->lo[a]; V.hi[a] = Vh->hi[a]; }
  V.vlo = Vh->tf_lo; V.vspan = Vh->tf_hi - Vh->tf_lo;
  V.skip = Vh->skip;
  return V;
}

// the surface march's by-value block.  The lights' directions are computed here, on the host, in float32: -position as a vector through
// minv (xfm_vector's order), divided by its length sqrt((x*x + y*y) + z*z); a light whose length is 0 or not finite shines from nowhere (0)
template <typename LT> // (SurfDev or LightDev)
void lights_dev(const gvt_hip_volume *Vh, const Mat4 &minv, LT &S) {
  S.n_lights = Vh->n_lights; S.ka = Vh->ka; S.kd = Vh->kd;
  for (int j = 0; j < Vh->n_lights; j++) {
    const V3 l = xfm_vector(minv, mk3(-Vh->lpos[j][0], -Vh->lpos[j][1], -Vh->lpos[j][2]));
    const float len = sqrtf((l.x * l.x + l.y * l.y) + l.z * l.z);
    const bool ok = len > 0.f && std::isfinite(len);
    S.ldir[j][0] = ok ? l.x / len : 0.f; S.ldir[j][1] = ok ? l.y / len : 0.f; S.ldir[j][2] = ok ? l.z / len : 0.f;
    for (int a = 0; a < 3; a++) S.lcol[j][a] = Vh->lcol[j][a];
  }
}
SurfDev surf_dev(const gvt_hip_volume *Vh, const Mat4 &minv) {
  SurfDev S{};
  S.n_iso = Vh->n_iso; S.n_pl = Vh->n_pl;
  S.alpha = Vh->surf_alpha;
  S.cells = Vh->d_cells;
  for (int i = 0; i < Vh->n_iso; i++) S.iso[i] = Vh->iso[i];
  for (int i = 0; i < Vh->n_pl; i++) S.plane[i] = make_float4(Vh->plane[i][0], Vh->plane[i][1], Vh->plane[i][2], Vh->plane[i][3]);
  lights_dev(Vh, minv, S);
  return S;
}
// the lit plain march's by-value block: the same lights, prepared the same way
LightDev light_dev(const gvt_hip_volume *Vh, const Mat4 &minv) {
  LightDev L{};
  lights_dev(Vh, minv, L);
  return L;
}

// Can a sample of macro cell b evaluate to NaN or to +-Inf?  With a vertex that is not finite, or with finite vertices so far apart that
// b - a overflows inside a lerp (then a + f * Inf is +-Inf, or NaN at f == 0).  Such a sample looks up entry 0 (NaN: fmaxf(NaN, 0) = 0) or
// entry 255, whatever the range of the block's vertices says
bool block_is_ranged(const gvt_hip_volume *V, size_t b) { // its samples stay within [bmin, bmax] (but for NaN ones, where bnan is set)
  return V->bmin[b] <= V->bmax[b] && (double)V->bmax[b] - (double)V->bmin[b] < 3.4e38;
}
bool block_is_wild(const gvt_hip_volume *V, size_t b) { return V->bnan[b] || !block_is_ranged(V, b); }

// the surface march's per-cell words: a macro cell's samples may go uninterpolated when the transfer function leaves it empty (h_mc) and
// no isovalue lies within its value range widened by 2^-18 of its magnitude (the trilinear interpolant's rounding stays far inside: three
// nested lerps are off by a few 2^-24 of the largest vertex); the word then carries the isovalue sides all its samples have
int upload_cells(gvt_hip_volume *V) {
  const size_t nbk = V->bmin.size();
  std::vector<uint32_t> cells(nbk, 0u);
  if (V->has_tf)
    for (size_t b = 0; b < nbk; b++) {
      if (V->h_mc[b] || (V->n_iso && block_is_wild(V, b))) continue; // (a NaN sample is on the false side of every isovalue)
      const double lo = V->bmin[b], hi = V->bmax[b], mg = std::max(std::fabs(lo), std::fabs(hi)) / 262144.0 + 1e-37;
      uint32_t w = VOL_CELL_SKIP;
      for (int i = 0; i < V->n_iso; i++) {
        const double c = V->iso[i];
        if (c < lo - mg) w |= 1u << i;        // every sample >= c
        else if (!(c > hi + mg)) { w = 0u; break; }
      }
      cells[b] = w;
    }
  HIPCHK(hipStreamSynchronize(gctx().stream)); // (a march in flight reads the table)
  HIPCHK(hipMemcpy(V->d_cells, cells.data(), sizeof(uint32_t) * nbk, hipMemcpyHostToDevice));
  return 0;
}

// bmin / bmax / bnan and vmin / vmax from d_vox (stream-ordered behind whatever wrote it), then one host wait and the download: 9 bytes
// per macro cell.  The grid itself never comes back to the host.  amr_merge (gvt_hip_volume_update_amr; the volume's merge tables exist):
// the subgrids' vertices are merged into the macro cells' ranges between the two kernels, so what comes down is the union
int volume_ranges(gvt_hip_volume *V, bool amr_merge = false) {
  Ctx &C = gctx();
  const size_t nbk = (size_t)V->nb[0] * V->nb[1] * V->nb[2];
  char *d = (char *)scratch_get(SCR_VOL_RANGES, 9 * nbk + 2 * sizeof(float));
  if (!d) return GVT_HIP_ERR_DEVICE;
  float *d_min = (float *)d, *d_max = d_min + nbk, *d_tot = d_max + nbk;
  uint8_t *d_nan = (uint8_t *)(d_tot + 2);
  const unsigned runs = (unsigned)((V->nb[0] + VR_CELLS - 1) / VR_CELLS);
  const size_t n_work = (size_t)runs * V->nb[1] * V->nb[2];
  const unsigned blocks = (unsigned)std::min(n_work, (size_t)1 << 22);
  {
    ProfScope ps(KC_BUILD);
    with_voxel_type(V->vtype, [&](auto t) {
      using T = decltype(t);
      const T *vox = (const T *)V->d_vox;
      if (V->n[0] % 4 == 0) // (every row then starts a multiple of 4 * sizeof(T) bytes from hipMalloc's pointer)
        k_vol_ranges<T, true><<<blocks, VOL_BLOCK, 0, C.stream>>>(vox, (unsigned)V->n[0], (unsigned)V->n[1], (unsigned)V->n[2], (unsigned)V->nb[0], (unsigned)V->nb[1], runs, n_work, d_min, d_max, d_nan);
      else
        k_vol_ranges<T, false><<<blocks, VOL_BLOCK, 0, C.stream>>>(vox, (unsigned)V->n[0], (unsigned)V->n[1], (unsigned)V->n[2], (unsigned)V->nb[0], (unsigned)V->nb[1], runs, n_work, d_min, d_max, d_nan);
    });
    if (amr_merge && V->amr_n_cells)
      k_amr_ranges_merge<<<std::min(V->amr_n_cells, 1u << 20), VOL_BLOCK, 0, C.stream>>>(V->d_amr_vox, V->d_amr_items, V->d_amr_cells, V->amr_n_cells, d_min, d_max, d_nan);
    k_vol_range_total<<<1, VR_TOTAL_BLOCK, 0, C.stream>>>(d_min, d_max, nbk, d_tot);
  }
  HIPCHK(hipGetLastError());
  V->bmin.resize(nbk); V->bmax.resize(nbk); V->bnan.resize(nbk); // (sized at create; an update finds them so)
  float tot[2] = { 0.f, 0.f };
  HIPCHK(hipMemcpyAsync(V->bmin.data(), d_min, sizeof(float) * nbk, hipMemcpyDeviceToHost, C.stream));
  HIPCHK(hipMemcpyAsync(V->bmax.data(), d_max, sizeof(float) * nbk, hipMemcpyDeviceToHost, C.stream));
  HIPCHK(hipMemcpyAsync(V->bnan.data(), d_nan, nbk, hipMemcpyDeviceToHost, C.stream));
  HIPCHK(hipMemcpyAsync(tot, d_tot, sizeof(tot), hipMemcpyDeviceToHost, C.stream));
  HIPCHK(hipStreamSynchronize(C.stream));
  V->vmin = tot[0]; V->vmax = tot[1];
  return 0;
}

// d_amr_mc: per macro cell the place of its level-1 subgrids in d_amr_list and, in bit 31 of y, h_mc (all zero before a transfer function)
int amr_upload_words(gvt_hip_volume *V) {
  const size_t nbk = V->amr_first.size();
  std::vector<uint2> words(nbk);
  for (size_t b = 0; b < nbk; b++) words[b] = make_uint2(V->amr_first[b], V->amr_count[b] | ((b < V->h_mc.size() && V->h_mc[b]) ? 0x80000000u : 0u));
  HIPCHK(hipStreamSynchronize(gctx().stream)); // (a march in flight reads the table)
  HIPCHK(hipMemcpy(V->d_amr_mc, words.data(), sizeof(uint2) * nbk, hipMemcpyHostToDevice));
  return 0;
}

// the tables that depend on the samples AND the transfer function (gvt_hip_volume_set_transfer, gvt_hip_volume_update_samples, _update_amr): d_mc,
// n_empty and, through upload_cells, d_cells.  The one statement of the rule: a block may be skipped when every table entry its values
// can reach -- one entry of margin either side for the rounding of the interpolation -- has a == 0: its samples then add exactly +0
int rebuild_tables(gvt_hip_volume *V) {
  const size_t nbk = V->bmin.size();
  std::vector<uint8_t> mc(nbk);
  const double value_lo = V->tf_lo, span = (double)V->tf_hi - (double)V->tf_lo;
  auto entry = [&](float v) {
    double p = ((double)v - value_lo) / span;
    p = p < 0 ? 0 : (p > 1 ? 1 : p);
    return (int)std::floor(p * 255.0);
  };
  int above[257]; // above[e] = entries below e with a > 0: "some entry of [e0, e1] has a > 0" is one subtraction per block (a walk over up to
  above[0] = 0;   // 256 entries per block took 19.7 of a 512^3 update's 20.1 ms, the count 1.7 of 2.0: profiles/volume_update.txt, 3)
  for (int e = 0; e < 256; e++) above[e + 1] = above[e] + (V->tf_a[e] > 0.f ? 1 : 0);
  uint64_t empty = 0;
  for (size_t b = 0; b < nbk; b++) {
    int e0 = 0, e1 = 255;
    if (block_is_ranged(V, b)) { e0 = V->bnan[b] ? 0 : std::max(0, entry(V->bmin[b]) - 1); e1 = std::min(255, entry(V->bmax[b]) + 2); } // (else: the whole table)
    mc[b] = above[e1 + 1] - above[e0] > 0 ? 1 : 0;
    empty += mc[b] ? 0 : 1;
  }
  HIPCHK(hipStreamSynchronize(gctx().stream)); // (a march in flight reads the tables)
  HIPCHK(hipMemcpy(V->d_mc, mc.data(), nbk, hipMemcpyHostToDevice));
  V->n_empty = empty;
  V->h_mc.swap(mc);
  if (!V->sub.empty()) { // the AMR march reads the skip bit from its own per-cell word
    int rc = amr_upload_words(V);
    if (rc) return rc;
  }
  return upload_cells(V);
}

// the march of q's rays through brick Vh, in place, on the context's stream (no host wait): the one launch site of the march kernels
// (gvt_hip_volume_trace and the frame loop come through here).  clip: a ray of q may carry GVT_HIP_RAY_CLIP -- the clipped frame's
// queues, host rays that were found flagged; the unclipped launches keep the march without the clip (profiles/volume_clip.txt)
int volume_march(gvt_hip_volume *Vh, gvt_hip_queue *q, const float minv[16], bool clip) {
  if (!q->size) return 0;
  Ctx &C = gctx();
  unsigned *work = (unsigned *)scratch_get(SCR_VOL_WORK, sizeof(unsigned));
  if (!work) return GVT_HIP_ERR_DEVICE;
  HIPCHK(hipMemsetAsync(work, 0, sizeof(unsigned), C.stream));
  Mat4 M;
  for (int k = 0; k < 16; k++) M.m[k] = minv[k];
  const unsigned blocks = std::min(blocks_of(q->size), (unsigned)(std::max(C.n_cu, 1) * 8));
  if (!Vh->sub.empty()) { // an AMR volume: F32, CELL gradients; surfaces and lit shading only under GVT_HIP_VOLUME_AMR_SHADED (the setters see to it)
    const RayPlanes P = make_planes(q->d_planes, q->cap);
    const unsigned n = (unsigned)q->size;
    const AmrDev Am{ Vh->d_amr_mc, Vh->d_amr_list, Vh->d_amr_desc, Vh->d_amr_vox };
    const bool surf = Vh->n_iso + Vh->n_pl > 0;
    const bool lit = Vh->shade == GVT_HIP_VOLUME_SHADE_GRADIENT && Vh->n_lights > 0; // (no lights: nothing to shade with, the plain AMR march)
    if (lit && surf && clip) k_volume_march_amr_surf_lit<true><<<blocks, VOL_BLOCK, 0, C.stream>>>(vol_dev(Vh), Am, surf_dev(Vh, M), P, n, M, work, Vh->d_stats);
    else if (lit && surf) k_volume_march_amr_surf_lit<false><<<blocks, VOL_BLOCK, 0, C.stream>>>(vol_dev(Vh), Am, surf_dev(Vh, M), P, n, M, work, Vh->d_stats);
    else if (lit && clip) k_volume_march_amr_lit<true><<<blocks, VOL_BLOCK, 0, C.stream>>>(vol_dev(Vh), Am, light_dev(Vh, M), P, n, M, work, Vh->d_stats);
    else if (lit) k_volume_march_amr_lit<false><<<blocks, VOL_BLOCK, 0, C.stream>>>(vol_dev(Vh), Am, light_dev(Vh, M), P, n, M, work, Vh->d_stats);
    else if (surf && clip) k_volume_march_amr_surf<true><<<blocks, VOL_BLOCK, 0, C.stream>>>(vol_dev(Vh), Am, surf_dev(Vh, M), P, n, M, work, Vh->d_stats);
    else if (surf) k_volume_march_amr_surf<false><<<blocks, VOL_BLOCK, 0, C.stream>>>(vol_dev(Vh), Am, surf_dev(Vh, M), P, n, M, work, Vh->d_stats);
    else if (clip) k_volume_march_amr<true><<<blocks, VOL_BLOCK, 0, C.stream>>>(vol_dev(Vh), Am, P, n, M, work, Vh->d_stats);
    else k_volume_march_amr<false><<<blocks, VOL_BLOCK, 0, C.stream>>>(vol_dev(Vh), Am, P, n, M, work, Vh->d_stats);
    HIPCHK(hipGetLastError());
    Vh->amr_marches++;
    return 0;
  }
  with_voxel_type(Vh->vtype, [&](auto t) {
    using T = decltype(t);
    const RayPlanes P = make_planes(q->d_planes, q->cap);
    const unsigned n = (unsigned)q->size;
    const bool surf = Vh->n_iso + Vh->n_pl > 0;
    const bool lit = Vh->shade == GVT_HIP_VOLUME_SHADE_GRADIENT && Vh->n_lights > 0; // (no lights: nothing to shade with, the march as it was)
    if (Vh->grad == GVT_HIP_VOLUME_GRADIENT_CENTRAL && (lit || surf)) { // (the plain march computes no gradient: the kind is inert there)
      const GhostDev H{ Vh->d_ghost, Vh->gn[0], Vh->gn[1], Vh->gn[2] };
      if (lit && surf && clip) k_volume_march_surf_lit_central<T, true><<<blocks, VOL_BLOCK, 0, C.stream>>>(vol_dev(Vh), surf_dev(Vh, M), H, P, n, M, work, Vh->d_stats);
      else if (lit && surf) k_volume_march_surf_lit_central<T, false><<<blocks, VOL_BLOCK, 0, C.stream>>>(vol_dev(Vh), surf_dev(Vh, M), H, P, n, M, work, Vh->d_stats);
      else if (lit && clip) k_volume_march_lit_central<T, true><<<blocks, VOL_BLOCK, 0, C.stream>>>(vol_dev(Vh), light_dev(Vh, M), H, P, n, M, work, Vh->d_stats);
      else if (lit) k_volume_march_lit_central<T, false><<<blocks, VOL_BLOCK, 0, C.stream>>>(vol_dev(Vh), light_dev(Vh, M), H, P, n, M, work, Vh->d_stats);
      else if (clip) k_volume_march_surf_central<T, true><<<blocks, VOL_BLOCK, 0, C.stream>>>(vol_dev(Vh), surf_dev(Vh, M), H, P, n, M, work, Vh->d_stats);
      else k_volume_march_surf_central<T, false><<<blocks, VOL_BLOCK, 0, C.stream>>>(vol_dev(Vh), surf_dev(Vh, M), H, P, n, M, work, Vh->d_stats);
      Vh->central_marches++;
      return;
    }
    if (lit && surf && clip) k_volume_march_surf_lit<T, true><<<blocks, VOL_BLOCK, 0, C.stream>>>(vol_dev(Vh), surf_dev(Vh, M), P, n, M, work, Vh->d_stats);
    else if (lit && surf) k_volume_march_surf_lit<T, false><<<blocks, VOL_BLOCK, 0, C.stream>>>(vol_dev(Vh), surf_dev(Vh, M), P, n, M, work, Vh->d_stats);
    else if (lit && clip) k_volume_march_lit<T, true><<<blocks, VOL_BLOCK, 0, C.stream>>>(vol_dev(Vh), light_dev(Vh, M), P, n, M, work, Vh->d_stats);
    else if (lit) k_volume_march_lit<T, false><<<blocks, VOL_BLOCK, 0, C.stream>>>(vol_dev(Vh), light_dev(Vh, M), P, n, M, work, Vh->d_stats);
    else if (surf && clip) k_volume_march_surf<T, true><<<blocks, VOL_BLOCK, 0, C.stream>>>(vol_dev(Vh), surf_dev(Vh, M), P, n, M, work, Vh->d_stats);
    else if (surf) k_volume_march_surf<T, false><<<blocks, VOL_BLOCK, 0, C.stream>>>(vol_dev(Vh), surf_dev(Vh, M), P, n, M, work, Vh->d_stats);
    else if (clip) k_volume_march<T, true><<<blocks, VOL_BLOCK, 0, C.stream>>>(vol_dev(Vh), P, n, M, work, Vh->d_stats);
    else k_volume_march<T, false><<<blocks, VOL_BLOCK, 0, C.stream>>>(vol_dev(Vh), P, n, M, work, Vh->d_stats);
  });
  HIPCHK(hipGetLastError());
  return 0;
}

// consumes q_in; one host wait (two where a destination queue has to grow to its exact need first)
// clip (from < 0 only): the depth plane the camera's rays are clipped at
// keep (from < 0 only): the host's keep mask of gvt_hip_volume_camera_filter, one byte per brick, or null
int shuffle_volume_impl(gvt_hip_top *T, gvt_hip_queue *q_in, int from, gvt_hip_queue *const *queues, gvt_hip_fb *fb, const gvt_hip_depth *clip = nullptr,
                        const uint8_t *keep = nullptr) {
  Ctx &C = gctx();
  hipStream_t st = C.stream;
  const size_t n = q_in->size, nI = T->n;
  if (!n) return 0;
  const unsigned n_blk = blocks_of(n);
  int *d_next = (int *)scratch_get(SCR_NEXT_INST, sizeof(int) * n);
  unsigned *d_blk = (unsigned *)scratch_get(SCR_BLOCK_COUNTS, sizeof(unsigned) * (nI ? nI : 1) * n_blk);
  unsigned *d_ovf = (unsigned *)scratch_get(SCR_VOL_OVF, sizeof(unsigned));
  if (!d_next || !d_blk || !d_ovf) return GVT_HIP_ERR_DEVICE;
  unsigned char *d_keep = nullptr;
  if (keep && from < 0 && nI) {
    if (!(d_keep = (unsigned char *)scratch_get(SCR_VOL_KEEP, nI))) return GVT_HIP_ERR_DEVICE;
    HIPCHK(hipMemcpyAsync(d_keep, keep, nI, hipMemcpyHostToDevice, st)); // (the caller's mask outlives the call: the shuffle ends with a host wait)
  }
  bool roomy = true;
  for (size_t i = 0; i < nI; i++) {
    if ((int)i == from || (d_keep && !keep[i])) continue; // (a masked brick receives nothing)
    if (nI <= 16 && queues[i]->cap < queues[i]->size + n) { // few bricks: worst-case room, so that the round has one host wait
      int rc = queue_reserve(queues[i], queues[i]->size + n);
      if (rc) return rc;
    }
    if (queues[i]->cap < queues[i]->size + n) roomy = false;
  }
  // keep = 0: k_dest_scan reads a queue's count word and leaves it alone.  The host writes the new fills below, once the scatter has
  // reported no overflow (k_vol_scatter does not read keep: every brick of the top is a destination here)
  QueueDesc *desc = (QueueDesc *)T->h_qdesc;
  auto upload_desc = [&]() -> int {
    for (size_t i = 0; i < nI; i++) { desc[i].planes = queues[i]->d_planes; desc[i].cap = queues[i]->cap; desc[i].count = queues[i]->d_count; desc[i].keep = 0u; }
    if (nI) HIPCHK(hipMemcpyAsync(T->d_qdesc, desc, sizeof(QueueDesc) * nI, hipMemcpyHostToDevice, st));
    T->qdesc_uploaded.clear(); // (the asynchronous mesh shuffle's upload cache no longer describes d_qdesc)
    return 0;
  };
  int rc;
  if ((rc = upload_desc())) return rc;
  HIPCHK(hipMemsetAsync(d_ovf, 0, sizeof(unsigned), st));
  const RayPlanes P = make_planes(q_in->d_planes, q_in->cap);
  const float *clip_plane = (clip && from < 0) ? clip->d_t : nullptr;
  const unsigned n_clip = clip_plane ? (unsigned)(clip->w * clip->h) : 0u;
  {
    ProfScope ps(KC_SHUFFLE);
    if (d_keep) k_vol_classify<true><<<n_blk, VOL_BLOCK, 0, st>>>(P, (unsigned)n, T->dev(), (int)nI, from, d_next, d_blk, nullptr, 0u, clip_plane, n_clip, d_keep);
    else k_vol_classify<false><<<n_blk, VOL_BLOCK, 0, st>>>(P, (unsigned)n, T->dev(), (int)nI, from, d_next, d_blk, fb ? fb->d_rgba : nullptr,
                                                       fb ? (unsigned)(fb->w * fb->h) : 0u, clip_plane, n_clip, nullptr);
    if (nI) k_dest_scan<VOL_BLOCK><<<(unsigned)nI, VOL_BLOCK, 0, st>>>(d_blk, n_blk, (const QueueDesc *)T->d_qdesc, T->d_hist);
  }
  HIPCHK(hipGetLastError());
  if (!roomy) { // exact growth: the totals first (the scan's bases depend only on the counts, which do not move before the scatter)
    HIPCHK(hipMemcpyAsync(T->h_hist, T->d_hist, sizeof(unsigned) * nI, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (size_t i = 0; i < nI; i++)
      if (T->h_hist[i] && (rc = queue_reserve(queues[i], queues[i]->size + T->h_hist[i]))) return rc;
    if ((rc = upload_desc())) return rc;
  }
  {
    ProfScope ps(KC_SHUFFLE);
    k_vol_scatter<<<n_blk, VOL_BLOCK, 0, st>>>(P, (unsigned)n, d_next, d_blk, (const QueueDesc *)T->d_qdesc, (int)nI, from < 0 ? (clip_plane ? 2 : 1) : 0, d_ovf,
                                               clip_plane, n_clip);
  }
  HIPCHK(hipGetLastError());
  if (nI) HIPCHK(hipMemcpyAsync(T->h_hist, T->d_hist, sizeof(unsigned) * nI, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(C.h_pinned + 13, d_ovf, sizeof(unsigned), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (C.h_pinned[13]) { set_error("shuffle_volume: a destination queue overflowed"); return GVT_HIP_ERR_DEVICE; }
  for (size_t i = 0; i < nI; i++) {
    if (!T->h_hist[i]) continue;
    queues[i]->size += T->h_hist[i];
    if ((rc = set_device_u32(queues[i]->d_count, (unsigned)queues[i]->size))) return rc;
  }
  q_in->size = 0; // rays.clear(), TracerBase.h:411
  HIPCHK(hipMemsetAsync(q_in->d_count, 0, sizeof(unsigned), st));
  return 0;
}

// TransferFunction::DeviceCommit's resampling (TransferFunction.cpp:40-72): the positions x in double rounded to float, the interpolation in
// float; rows of W floats (x first)
template <int W>
bool resample(const float *map, int nrow, float out[256][W - 1]) {
  int i0 = 0, i1 = 1;
  const float xmin = map[0], xmax = map[(size_t)(nrow - 1) * W];
  for (int i = 0; i < 256; i++) {
    float x = xmin + (i / (255.0)) * (xmax - xmin);
    if (x > xmax) x = xmax;
    while (map[(size_t)i1 * W] < x) i0++, i1++;
    const float dx = (x - map[(size_t)i0 * W]) / (map[(size_t)i1 * W] - map[(size_t)i0 * W]);
    for (int c = 1; c < W; c++) {
      const float a = map[(size_t)i0 * W + c], b = map[(size_t)i1 * W + c];
      out[i][c - 1] = a + dx * (b - a);
      if (!std::isfinite(out[i][c - 1])) return false;
    }
  }
  return true;
}

} // namespace

extern "C" gvt_hip_volume *gvt_hip_volume_create_typed(const void *samples, int voxel_type, const int counts[3], const float origin[3], const float spacing[3],
                                                       const int offset[3], const int global_counts[3], float sampling_rate, int flags) {
  if (ensure_init()) return nullptr;
  const size_t vbytes = voxel_bytes(voxel_type);
  if (!vbytes) { set_error("volume_create: unknown voxel type %d", voxel_type); return nullptr; }
  if (!samples || !counts || !origin || !spacing || !offset || !global_counts) { set_error("volume_create: null argument"); return nullptr; }
  if (flags & ~(GVT_HIP_VOLUME_DEVICE | GVT_HIP_VOLUME_NO_SKIP)) { set_error("volume_create: unknown flag bits %d", flags); return nullptr; }
  if (!(sampling_rate > 0.f) || !std::isfinite(sampling_rate)) { set_error("volume_create: sampling_rate %g is not positive", (double)sampling_rate); return nullptr; }
  size_t total = 1;
  for (int a = 0; a < 3; a++) {
    if (counts[a] < 2 || global_counts[a] < 2) { set_error("volume_create: counts must be at least 2 per axis (axis %d)", a); return nullptr; }
    if (!(spacing[a] > 0.f) || !std::isfinite(spacing[a]) || !std::isfinite(origin[a])) { set_error("volume_create: spacing of axis %d is not positive and finite", a); return nullptr; }
    if (offset[a] < 0 || (long long)offset[a] + counts[a] > (long long)global_counts[a]) {
      set_error("volume_create: the brick's vertices [%d, %d) of axis %d lie outside its global grid of %d", offset[a], offset[a] + counts[a], a, global_counts[a]);
      return nullptr;
    }
    if (global_counts[a] >= (1 << 24)) { set_error("volume_create: global grid too large on axis %d", a); return nullptr; }
    total *= (size_t)counts[a];
  }
  if (total >= 0xffffffffull) { set_error("volume_create: brick of %zu vertices is too large", total); return nullptr; }
  gvt_hip_volume *V = new gvt_hip_volume();
  for (int a = 0; a < 3; a++) {
    V->n[a] = counts[a]; V->off[a] = offset[a]; V->gn[a] = global_counts[a]; V->go[a] = origin[a]; V->sp[a] = spacing[a];
    V->lo[a] = origin[a] + (float)offset[a] * spacing[a];
    V->hi[a] = origin[a] + (float)(offset[a] + counts[a] - 1) * spacing[a];
    V->nb[a] = (counts[a] - 1 + 7) / 8;
  }
  V->vtype = voxel_type;
  V->rate = sampling_rate;
  V->dt = std::min(std::min(spacing[0], spacing[1]), spacing[2]) / sampling_rate;
  V->skip = (flags & GVT_HIP_VOLUME_NO_SKIP) ? 0 : 1;
  const size_t n_blocks = (size_t)V->nb[0] * V->nb[1] * V->nb[2];
  // d_vox is exactly the brick: total samples of the voxel type, no padding (no load of the march or the range kernels is wider than the
  // vertices it asks for)
  bool ok = hipMalloc(&V->d_vox, vbytes * total) == hipSuccess && hipMalloc((void **)&V->d_tf, sizeof(float4) * 256) == hipSuccess &&
            hipMalloc((void **)&V->d_stats, VOL_N_STATS * sizeof(unsigned long long)) == hipSuccess &&
            hipMemset(V->d_stats, 0, VOL_N_STATS * sizeof(unsigned long long)) == hipSuccess && hipMalloc((void **)&V->d_mc, n_blocks) == hipSuccess &&
            hipMalloc((void **)&V->d_cells, sizeof(uint32_t) * n_blocks) == hipSuccess;
  // the samples go to the device on the context's stream and the macro cells' ranges are computed there, behind the copy (volume_ranges
  // ends with a host wait): samples in device memory never touch the host
  ok = ok && hipMemcpyAsync(V->d_vox, samples, vbytes * total, (flags & GVT_HIP_VOLUME_DEVICE) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                            gctx().stream) == hipSuccess;
  if (!ok) { set_error("volume_create: device allocation or copy failed"); gvt_hip_volume_destroy(V); return nullptr; }
  if (volume_ranges(V)) { gvt_hip_volume_destroy(V); return nullptr; }
  return V;
}

extern "C" gvt_hip_volume *gvt_hip_volume_create(const float *samples, const int counts[3], const float origin[3], const float spacing[3], const int offset[3],
                                                 const int global_counts[3], float sampling_rate, int flags) {
  return gvt_hip_volume_create_typed(samples, GVT_HIP_VOXEL_F32, counts, origin, spacing, offset, global_counts, sampling_rate, flags);
}

extern "C" int gvt_hip_volume_get_voxel_type(gvt_hip_volume *V, int *type_out, size_t *sample_bytes_out) {
  if (!V) { set_error("volume_get_voxel_type: null"); return GVT_HIP_ERR_INVALID; }
  if (type_out) *type_out = V->vtype;
  if (sample_bytes_out) *sample_bytes_out = voxel_bytes(V->vtype);
  return 0;
}

extern "C" void gvt_hip_volume_destroy(gvt_hip_volume *V) {
  if (!V) return;
  if (gctx().ready) hipStreamSynchronize(gctx().stream);
  hipFree(V->d_vox); hipFree(V->d_tf); hipFree(V->d_mc); hipFree(V->d_cells); hipFree(V->d_stats); hipFree(V->d_ghost); hipFree(V->d_lgrid); hipFree(V->d_occ); hipFree(V->d_ao);
  hipFree(V->d_amr_vox); hipFree(V->d_amr_mc); hipFree(V->d_amr_list); hipFree(V->d_amr_desc); hipFree(V->d_amr_items); hipFree(V->d_amr_cells);
  delete V;
}

extern "C" int gvt_hip_volume_set_transfer(gvt_hip_volume *V, const float *cmap, int nc, const float *omap, int no, float value_lo, float value_hi) {
  if (ensure_init()) return GVT_HIP_ERR_NODEVICE;
  if (!V || !cmap || !omap) { set_error("volume_set_transfer: null argument"); return GVT_HIP_ERR_INVALID; }
  if (nc < 2 || no < 2) { set_error("volume_set_transfer: a map needs at least 2 entries (colour %d, opacity %d)", nc, no); return GVT_HIP_ERR_INVALID; }
  if (!(value_lo < value_hi) || !std::isfinite(value_lo) || !std::isfinite(value_hi)) {
    set_error("volume_set_transfer: value range [%g, %g] is empty", (double)value_lo, (double)value_hi);
    return GVT_HIP_ERR_INVALID;
  }
  for (int i = 1; i < nc; i++)
    if (!(cmap[4 * i] >= cmap[4 * (i - 1)])) { set_error("volume_set_transfer: colour map x decreases at entry %d", i); return GVT_HIP_ERR_INVALID; }
  for (int i = 1; i < no; i++)
    if (!(omap[2 * i] >= omap[2 * (i - 1)])) { set_error("volume_set_transfer: opacity map x decreases at entry %d", i); return GVT_HIP_ERR_INVALID; }
  float col[256][3], op[256][1];
  if (!resample<4>(cmap, nc, col) || !resample<2>(omap, no, op)) {
    set_error("volume_set_transfer: a map resamples to a non-finite entry (a repeated x hit exactly)");
    return GVT_HIP_ERR_INVALID;
  }
  std::vector<float4> tf(256);
  for (int i = 0; i < 256; i++) {
    const float a = (float)(1.0 - std::pow(1.0 - (double)op[i][0], 1.0 / (double)V->rate)); // opacity correction, rounded once
    if (!std::isfinite(a)) { set_error("volume_set_transfer: opacity %g at entry %d cannot be corrected", (double)op[i][0], i); return GVT_HIP_ERR_INVALID; }
    tf[i] = make_float4(col[i][0], col[i][1], col[i][2], a);
  }
  HIPCHK(hipStreamSynchronize(gctx().stream)); // (a march in flight reads the tables)
  HIPCHK(hipMemcpy(V->d_tf, tf.data(), sizeof(float4) * 256, hipMemcpyHostToDevice));
  V->lg.current = false; // (a light grid baked under the old table is stale)
  V->ag.current = false; // (... and so is an AO grid)
  for (int i = 0; i < 256; i++) { V->tf_a[i] = tf[i].w; V->tf_rgb[i][0] = tf[i].x; V->tf_rgb[i][1] = tf[i].y; V->tf_rgb[i][2] = tf[i].z; }
  V->tf_lo = value_lo; V->tf_hi = value_hi; V->has_tf = true;
  return rebuild_tables(V);
}

extern "C" int gvt_hip_volume_update_samples_typed(gvt_hip_volume *V, const void *samples, int voxel_type, size_t n_samples, uint32_t flags, float *ms_out) {
  if (ensure_init()) return GVT_HIP_ERR_NODEVICE;
  if (!V || !samples) { set_error("volume_update_samples: null argument"); return GVT_HIP_ERR_INVALID; }
  if (voxel_type != V->vtype) {
    set_error("volume_update_samples: samples of voxel type %d, the volume holds type %d (fixed at creation)", voxel_type, V->vtype);
    return GVT_HIP_ERR_INVALID;
  }
  if (flags & ~GVT_HIP_UPDATE_DEVICE) { set_error("volume_update_samples: unknown flags 0x%x", flags); return GVT_HIP_ERR_INVALID; }
  if (!V->sub.empty()) {
    set_error("volume_update_samples: the volume has %zu AMR subgrids (remove them with gvt_hip_volume_set_subgrids(n = 0) first, then set the new step's)", V->sub.size());
    return GVT_HIP_ERR_INVALID;
  }
  const size_t total = (size_t)V->n[0] * V->n[1] * V->n[2];
  if (n_samples != total) {
    set_error("volume_update_samples: %zu samples given, the brick has %zu (%d x %d x %d; another grid needs a new volume)", n_samples, total, V->n[0], V->n[1], V->n[2]);
    return GVT_HIP_ERR_INVALID;
  }
  hipStream_t st = gctx().stream;
  HIPCHK(hipStreamSynchronize(st)); // (a march in flight reads the samples)
  V->lg.current = false; // (a light grid baked from the old samples is stale)
  V->ag.current = false; // (... and so is an AO grid)
  HIPCHK(hipMemcpyAsync(V->d_vox, samples, voxel_bytes(V->vtype) * total, (flags & GVT_HIP_UPDATE_DEVICE) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
  hipEvent_t e0, e1;
  HIPCHK(hipEventCreate(&e0));
  if (hipEventCreate(&e1) != hipSuccess) { hipEventDestroy(e0); set_error("volume_update_samples: hipEventCreate failed"); return GVT_HIP_ERR_DEVICE; }
  int rc = hipEventRecord(e0, st) == hipSuccess ? 0 : GVT_HIP_ERR_DEVICE;
  if (!rc) rc = volume_ranges(V);
  if (!rc && V->has_tf) rc = rebuild_tables(V); // (else: built when the transfer function arrives)
  float ms = 0.f;
  if (!rc && (hipEventRecord(e1, st) != hipSuccess || hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&ms, e0, e1) != hipSuccess)) {
    set_error("volume_update_samples: %s", hipGetErrorString(hipGetLastError()));
    rc = GVT_HIP_ERR_DEVICE;
  }
  hipStreamSynchronize(st);
  hipEventDestroy(e0); hipEventDestroy(e1);
  if (!rc && ms_out) *ms_out = ms;
  return rc;
}

extern "C" int gvt_hip_volume_update_samples(gvt_hip_volume *V, const float *samples, size_t n_samples, uint32_t flags, float *ms_out) {
  return gvt_hip_volume_update_samples_typed(V, samples, GVT_HIP_VOXEL_F32, n_samples, flags, ms_out);
}

extern "C" int gvt_hip_volume_set_surfaces(gvt_hip_volume *V, const float *isovalues, int n_iso, const float *slices, int n_slices, float opacity) {
  if (ensure_init()) return GVT_HIP_ERR_NODEVICE;
  if (!V || (n_iso > 0 && !isovalues) || (n_slices > 0 && !slices)) { set_error("volume_set_surfaces: null argument"); return GVT_HIP_ERR_INVALID; }
  if (n_iso < 0 || n_slices < 0 || n_iso > GVT_HIP_VOLUME_MAX_SURFACES || n_slices > GVT_HIP_VOLUME_MAX_SURFACES || n_iso + n_slices > GVT_HIP_VOLUME_MAX_SURFACES) {
    set_error("volume_set_surfaces: %d isovalues and %d slices, at most %d surfaces", n_iso, n_slices, GVT_HIP_VOLUME_MAX_SURFACES);
    return GVT_HIP_ERR_INVALID;
  }
  if (n_iso + n_slices > 0 && !V->sub.empty() && !(V->amr_flags & GVT_HIP_VOLUME_AMR_SHADED)) { set_error("volume_set_surfaces: the volume has AMR subgrids, which take no surfaces"); return GVT_HIP_ERR_INVALID; }
  if (!(opacity > 0.f && opacity <= 1.f)) { set_error("volume_set_surfaces: opacity %g is not in (0, 1]", (double)opacity); return GVT_HIP_ERR_INVALID; }
  for (int i = 0; i < n_iso; i++)
    if (isovalues[i] != isovalues[i]) { set_error("volume_set_surfaces: isovalue %d is NaN", i); return GVT_HIP_ERR_INVALID; }
  for (int i = 0; i < n_slices; i++) {
    const float *p = slices + 4 * i;
    const bool finite = std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]) && std::isfinite(p[3]);
    if (!finite || (p[0] == 0.f && p[1] == 0.f && p[2] == 0.f)) { set_error("volume_set_surfaces: slice %d has a zero or non-finite plane", i); return GVT_HIP_ERR_INVALID; }
  }
  V->n_iso = n_iso; V->n_pl = n_slices; V->surf_alpha = opacity;
  V->lg.current = false; // (the surfaces cast shadows: a light grid baked under the old ones is stale)
  V->ag.current = false; // (... and so is an AO grid)
  for (int i = 0; i < n_iso; i++) V->iso[i] = isovalues[i];
  for (int i = 0; i < n_slices; i++)
    for (int a = 0; a < 4; a++) V->plane[i][a] = slices[4 * i + a];
  return V->has_tf ? upload_cells(V) : 0;
}

extern "C" int gvt_hip_volume_set_lights(gvt_hip_volume *V, const float *positions, const float *colours, int n, float ka, float kd) {
  if (ensure_init()) return GVT_HIP_ERR_NODEVICE;
  if (!V || (n > 0 && (!positions || !colours))) { set_error("volume_set_lights: null argument"); return GVT_HIP_ERR_INVALID; }
  if (n < 0 || n > GVT_HIP_VOLUME_MAX_LIGHTS) { set_error("volume_set_lights: %d lights, at most %d", n, GVT_HIP_VOLUME_MAX_LIGHTS); return GVT_HIP_ERR_INVALID; }
  if (!std::isfinite(ka) || !std::isfinite(kd)) { set_error("volume_set_lights: ka %g, kd %g", (double)ka, (double)kd); return GVT_HIP_ERR_INVALID; }
  for (int i = 0; i < 3 * n; i++)
    if (!std::isfinite(positions[i]) || !std::isfinite(colours[i])) { set_error("volume_set_lights: light %d is not finite", i / 3); return GVT_HIP_ERR_INVALID; }
  V->n_lights = n; V->ka = ka; V->kd = kd;
  V->lg.current = false; // (a light grid holds one plane per light of the old list)
  V->og.current = false; // (... and so does an occluder grid)
  for (int j = 0; j < n; j++)
    for (int a = 0; a < 3; a++) { V->lpos[j][a] = positions[3 * j + a]; V->lcol[j][a] = colours[3 * j + a]; }
  return 0;
}

extern "C" int gvt_hip_volume_get_crossings(gvt_hip_volume *V, uint64_t *crossings_rendered) {
  if (ensure_init()) return GVT_HIP_ERR_NODEVICE;
  if (!V || !crossings_rendered) { set_error("volume_get_crossings: null"); return GVT_HIP_ERR_INVALID; }
  unsigned long long s = 0;
  HIPCHK(hipStreamSynchronize(gctx().stream));
  HIPCHK(hipMemcpy(&s, V->d_stats + 2, sizeof(s), hipMemcpyDeviceToHost));
  *crossings_rendered = s;
  return 0;
}

extern "C" int gvt_hip_volume_set_shading(gvt_hip_volume *V, int mode) {
  if (ensure_init()) return GVT_HIP_ERR_NODEVICE;
  if (!V) { set_error("volume_set_shading: null"); return GVT_HIP_ERR_INVALID; }
  if (mode != GVT_HIP_VOLUME_SHADE_NONE && mode != GVT_HIP_VOLUME_SHADE_GRADIENT) { set_error("volume_set_shading: unknown mode %d", mode); return GVT_HIP_ERR_INVALID; }
  if (mode == GVT_HIP_VOLUME_SHADE_GRADIENT && !V->sub.empty() && !(V->amr_flags & GVT_HIP_VOLUME_AMR_SHADED)) { set_error("volume_set_shading: the volume has AMR subgrids, which are not shaded"); return GVT_HIP_ERR_INVALID; }
  V->shade = mode;
  return 0;
}

extern "C" int gvt_hip_volume_get_shading(gvt_hip_volume *V, int *mode_out) {
  if (!V || !mode_out) { set_error("volume_get_shading: null"); return GVT_HIP_ERR_INVALID; }
  *mode_out = V->shade;
  return 0;
}

extern "C" int gvt_hip_volume_get_shaded(gvt_hip_volume *V, uint64_t *samples_shaded) {
  if (ensure_init()) return GVT_HIP_ERR_NODEVICE;
  if (!V || !samples_shaded) { set_error("volume_get_shaded: null"); return GVT_HIP_ERR_INVALID; }
  unsigned long long s = 0;
  HIPCHK(hipStreamSynchronize(gctx().stream));
  HIPCHK(hipMemcpy(&s, V->d_stats + 3, sizeof(s), hipMemcpyDeviceToHost));
  *samples_shaded = s;
  return 0;
}

// ---- smooth gradients: the six face layers beyond the brick and the gradient kind (the contract: include/gvt_hip.h)
namespace {
// is face 2 * a + side of the brick on the global grid's boundary (no vertex beyond it)?
bool face_on_boundary(const gvt_hip_volume *V, int a, int side) { return side ? V->off[a] + V->n[a] == V->gn[a] : V->off[a] == 0; }
size_t face_samples(const gvt_hip_volume *V, int a) { return (size_t)V->n[a == 0 ? 1 : 0] * (size_t)V->n[a == 2 ? 1 : 2]; }
} // namespace

extern "C" int gvt_hip_volume_set_ghosts(gvt_hip_volume *V, const void *const faces[6], int voxel_type, uint32_t flags) {
  if (ensure_init()) return GVT_HIP_ERR_NODEVICE;
  if (!V || !faces) { set_error("volume_set_ghosts: null argument"); return GVT_HIP_ERR_INVALID; }
  if (voxel_type != V->vtype) {
    set_error("volume_set_ghosts: faces of voxel type %d, the volume holds type %d (fixed at creation)", voxel_type, V->vtype);
    return GVT_HIP_ERR_INVALID;
  }
  if (flags & ~(uint32_t)GVT_HIP_VOLUME_DEVICE) { set_error("volume_set_ghosts: unknown flags 0x%x", flags); return GVT_HIP_ERR_INVALID; }
  unsigned mask = 0;
  for (int a = 0; a < 3; a++)
    for (int side = 0; side < 2; side++) {
      const int i = 2 * a + side;
      if (faces[i] && face_on_boundary(V, a, side)) {
        set_error("volume_set_ghosts: face %d lies on the global grid's boundary, there is no layer beyond it", i);
        return GVT_HIP_ERR_INVALID;
      }
      if (!faces[i] && !face_on_boundary(V, a, side) && V->grad == GVT_HIP_VOLUME_GRADIENT_CENTRAL) {
        set_error("volume_set_ghosts: the gradient kind is CENTRAL, which needs the layer of face %d", i);
        return GVT_HIP_ERR_INVALID;
      }
      if (faces[i]) mask |= 1u << i;
    }
  const size_t vb = voxel_bytes(V->vtype);
  hipStream_t st = gctx().stream;
  HIPCHK(hipStreamSynchronize(st)); // (a march in flight reads the layers)
  if (mask && !V->d_ghost) {
    const size_t total = 2 * (face_samples(V, 0) + face_samples(V, 1) + face_samples(V, 2));
    if (hipMalloc(&V->d_ghost, vb * total) != hipSuccess) { V->d_ghost = nullptr; set_error("volume_set_ghosts: device allocation failed"); return GVT_HIP_ERR_DEVICE; }
  }
  size_t at = 0;
  for (int i = 0; i < 6; i++) {
    const size_t cnt = face_samples(V, i / 2);
    if (faces[i])
      HIPCHK(hipMemcpyAsync((char *)V->d_ghost + vb * at, faces[i], vb * cnt, (flags & GVT_HIP_VOLUME_DEVICE) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
    at += cnt;
  }
  HIPCHK(hipStreamSynchronize(st)); // (the samples are copied: the caller's memory is free on return)
  V->ghost_mask = mask;
  return 0;
}

extern "C" int gvt_hip_volume_set_gradient(gvt_hip_volume *V, int kind) {
  if (ensure_init()) return GVT_HIP_ERR_NODEVICE;
  if (!V) { set_error("volume_set_gradient: null"); return GVT_HIP_ERR_INVALID; }
  if (kind != GVT_HIP_VOLUME_GRADIENT_CELL && kind != GVT_HIP_VOLUME_GRADIENT_CENTRAL) { set_error("volume_set_gradient: unknown kind %d", kind); return GVT_HIP_ERR_INVALID; }
  if (kind == GVT_HIP_VOLUME_GRADIENT_CENTRAL) {
    if (!V->sub.empty()) { set_error("volume_set_gradient: the volume has AMR subgrids, which are not shaded"); return GVT_HIP_ERR_INVALID; }
    for (int i = 0; i < 6; i++)
      if (!face_on_boundary(V, i / 2, i % 2) && !(V->ghost_mask & (1u << i))) {
        set_error("volume_set_gradient: CENTRAL needs the layer beyond face %d (gvt_hip_volume_set_ghosts)", i);
        return GVT_HIP_ERR_INVALID;
      }
  }
  V->grad = kind;
  return 0;
}

extern "C" int gvt_hip_volume_get_gradient(gvt_hip_volume *V, int *kind_out, uint64_t *central_marches_out) {
  if (!V) { set_error("volume_get_gradient: null"); return GVT_HIP_ERR_INVALID; }
  if (kind_out) *kind_out = V->grad;
  if (central_marches_out) *central_marches_out = V->central_marches;
  return 0;
}

extern "C" int gvt_hip_volume_get_info(gvt_hip_volume *V, gvt_hip_volume_info *out) {
  if (ensure_init()) return GVT_HIP_ERR_NODEVICE;
  if (!V || !out) { set_error("volume_get_info: null"); return GVT_HIP_ERR_INVALID; }
  unsigned long long s[2] = { 0, 0 };
  HIPCHK(hipStreamSynchronize(gctx().stream));
  HIPCHK(hipMemcpy(s, V->d_stats, sizeof(s), hipMemcpyDeviceToHost));
  gvt_hip_volume_info I{};
  for (int a = 0; a < 3; a++) { I.box_lo[a] = V->lo[a]; I.box_hi[a] = V->hi[a]; I.blocks[a] = V->nb[a]; }
  I.dt = V->dt; I.value_min = V->vmin; I.value_max = V->vmax;
  I.n_blocks = V->bmin.size(); I.n_blocks_empty = V->has_tf ? V->n_empty : 0;
  I.samples_marched = s[0]; I.samples_gathered = s[1];
  *out = I;
  return 0;
}

extern "C" int gvt_hip_volume_trace(gvt_hip_volume *V, const gvt_hip_ray *rays, size_t n, size_t begin, size_t end, gvt_hip_ray *rays_out, size_t cap,
                                    size_t *n_out, const float m[16], const float minv[16]) {
  if (ensure_init()) return GVT_HIP_ERR_NODEVICE;
  if (!V || !n_out || !m || !minv || (n && !rays)) { set_error("volume_trace: null argument"); return GVT_HIP_ERR_INVALID; }
  if (end == 0) end = n;
  if (begin > end || end > n) { set_error("volume_trace: bad range [%zu, %zu) of %zu rays", begin, end, n); return GVT_HIP_ERR_INVALID; }
  if (!V->has_tf) { set_error("volume_trace: the volume has no transfer function (gvt_hip_volume_set_transfer)"); return GVT_HIP_ERR_INVALID; }
  const size_t cnt = end - begin;
  *n_out = cnt;
  if (cnt > cap) { set_error("volume_trace: %zu rays, capacity %zu", cnt, cap); return GVT_HIP_ERR_CAPACITY; }
  if (!cnt) return 0;
  if (!rays_out) { set_error("volume_trace: null rays_out"); return GVT_HIP_ERR_INVALID; }
  Ctx &C = gctx();
  if (!staging_queues(C)) return GVT_HIP_ERR_DEVICE;
  gvt_hip_queue *q = C.abi_qin; // (the context's staging list of gvt_hip_trace)
  int rc;
  if ((rc = gvt_hip_queue_clear(q))) return rc;
  if ((rc = gvt_hip_queue_append_flags(q, rays + begin, cnt, GVT_HIP_APPEND_KEEP_STATE))) return rc; // (bytes 64..79 pass through untouched)
  bool clip = false; // (does a ray carry the flag?  One pass over the host rays, before they are staged)
  for (size_t i = begin; i < end && !clip; i++) clip = (rays[i].depth & GVT_HIP_RAY_CLIP) != 0;
  if ((rc = volume_march(V, q, minv, clip))) return rc;
  size_t got = 0;
  if ((rc = gvt_hip_queue_export(q, rays_out, cap, &got, 0))) return rc;
  *n_out = got;
  return gvt_hip_queue_clear(q);
}

extern "C" int gvt_hip_shuffle_volume(gvt_hip_top *T, gvt_hip_queue *q_in, int from, gvt_hip_queue *const *queues, gvt_hip_fb *fb) {
  if (ensure_init()) return GVT_HIP_ERR_NODEVICE;
  if (!T || !q_in || (T->n && !queues)) { set_error("shuffle_volume: null argument"); return GVT_HIP_ERR_INVALID; }
  if (T->n > VOL_DEST_MAX) { set_error("shuffle_volume: %zu bricks, at most %d", T->n, VOL_DEST_MAX); return GVT_HIP_ERR_INVALID; }
  if (from >= (int)T->n) { set_error("shuffle_volume: source %d of %zu bricks", from, T->n); return GVT_HIP_ERR_INVALID; }
  for (size_t i = 0; i < T->n; i++)
    if (!queues[i] || (queues[i] == q_in && (int)i != from)) { set_error("shuffle_volume: queue %zu is null or aliases q_in", i); return GVT_HIP_ERR_INVALID; }
  return shuffle_volume_impl(T, q_in, from, queues, fb);
}

// generateRays (ImageTracer.h:137), then every camera ray into the brick it enters first: the camera step of gvt_hip_volume_frame and the
// whole of gvt_hip_volume_camera_filter (keep: its mask).  The origins stay at the eye (gvt_hip_camera_filter would advance them into the
// first box): a ray keeps one sample lattice from start to end
static int volume_camera_step(gvt_hip_top *T, const gvt_hip_camera *cam, gvt_hip_queue *const *queues, gvt_hip_fb *fb, const gvt_hip_depth *depth,
                              const uint8_t *keep) {
  Ctx &C = gctx();
  if (!staging_queues(C)) return GVT_HIP_ERR_DEVICE;
  gvt_hip_queue *q_cam = C.abi_qout; // (a staging list of the context: the camera's rays before they are distributed)
  int rc;
  if ((rc = gvt_hip_camera_generate_tiled(q_cam, cam->eye, cam->focus, cam->up, cam->fov, cam->width, cam->height, cam->samples, 0,
                                          cam->jitter_window_size, 8))) return rc;
  return shuffle_volume_impl(T, q_cam, -1, queues, fb, depth, keep);
}

extern "C" int gvt_hip_volume_camera_filter(gvt_hip_top *T, const gvt_hip_camera *cam, gvt_hip_queue *const *queues, const uint8_t *keep_mask) {
  if (ensure_init()) return GVT_HIP_ERR_NODEVICE;
  if (!T || !cam || (T->n && !queues)) { set_error("volume_camera_filter: null argument"); return GVT_HIP_ERR_INVALID; }
  if (T->n > VOL_DEST_MAX) { set_error("volume_camera_filter: %zu bricks, at most %d", T->n, VOL_DEST_MAX); return GVT_HIP_ERR_INVALID; }
  for (size_t i = 0; i < T->n; i++)
    if (!queues[i]) { set_error("volume_camera_filter: queue %zu is null", i); return GVT_HIP_ERR_INVALID; }
  return volume_camera_step(T, cam, queues, nullptr, nullptr, keep_mask);
}

extern "C" int gvt_hip_volume_march_queue(gvt_hip_volume *V, gvt_hip_queue *queue, const float minv[16], uint32_t flags) {
  if (ensure_init()) return GVT_HIP_ERR_NODEVICE;
  if (!V || !queue || !minv) { set_error("volume_march_queue: null argument"); return GVT_HIP_ERR_INVALID; }
  if (flags & ~(uint32_t)GVT_HIP_MARCH_MAY_CLIP) { set_error("volume_march_queue: unknown flag bits %u", flags); return GVT_HIP_ERR_INVALID; }
  if (!V->has_tf) { set_error("volume_march_queue: the volume has no transfer function (gvt_hip_volume_set_transfer)"); return GVT_HIP_ERR_INVALID; }
  return volume_march(V, queue, minv, (flags & GVT_HIP_MARCH_MAY_CLIP) != 0);
}

// the frame entry points' argument errors (nothing has changed when one is returned): the loop's and the fused frame's
static int volume_frame_args(gvt_hip_top *T, gvt_hip_volume *const *volumes, const float *m, const float *minv, size_t n_inst, const gvt_hip_camera *cam,
                             gvt_hip_queue *const *queues, gvt_hip_fb *fb, const gvt_hip_depth *depth) {
  if (ensure_init()) return GVT_HIP_ERR_NODEVICE;
  if (!T || !cam || !fb || (n_inst && (!volumes || !m || !minv || !queues)) || T->n != n_inst) {
    set_error("volume_frame: null or inconsistent argument");
    return GVT_HIP_ERR_INVALID;
  }
  if (n_inst > VOL_DEST_MAX) { set_error("volume_frame: %zu bricks, at most %d", n_inst, VOL_DEST_MAX); return GVT_HIP_ERR_INVALID; }
  for (size_t i = 0; i < n_inst; i++)
    if (!volumes[i] || !queues[i] || !volumes[i]->has_tf) { set_error("volume_frame: brick %zu has no volume, queue or transfer function", i); return GVT_HIP_ERR_INVALID; }
  // several bricks under a matrix that turns or shears them (gvt_hip.h, "bricks under a matrix"): their world boxes overlap and vol_next would skip bricks.
  // Allowed: one non-zero entry per row and column of the 3x3 block (a signed, scaled axis permutation)
  for (size_t i = 0; n_inst > 1 && i < n_inst; i++) {
    const float *mi = m + 16 * i;
    for (int a = 0; a < 3; a++) {
      int in_col = 0, in_row = 0;
      for (int b = 0; b < 3; b++) { in_col += mi[4 * a + b] != 0.0f; in_row += mi[4 * b + a] != 0.0f; }
      if (in_col != 1 || in_row != 1) {
        set_error("volume_frame: %zu bricks, and the matrix of brick %zu rotates or shears it: the world boxes of neighbouring bricks overlap and bricks would be skipped", n_inst, i);
        return GVT_HIP_ERR_INVALID;
      }
    }
  }
  if (depth && (cam->samples != 1 || depth->w != cam->width || depth->h != cam->height)) {
    set_error("volume_frame_clipped: a %d x %d depth plane for a %d x %d film of %d x %d samples per pixel (one is needed)", depth->w, depth->h, cam->width, cam->height,
              cam->samples, cam->samples);
    return GVT_HIP_ERR_INVALID;
  }
  return 0;
}

// gvt_hip_volume_frame and gvt_hip_volume_frame_clipped (depth: the plane the camera's rays are clipped at, or null)
static int volume_frame_impl(gvt_hip_top *T, gvt_hip_volume *const *volumes, const float *m, const float *minv, size_t n_inst, const gvt_hip_camera *cam,
                             gvt_hip_queue *const *queues, gvt_hip_fb *fb, const gvt_hip_depth *depth, uint64_t *adapter_calls) {
  int rc;
  if ((rc = volume_frame_args(T, volumes, m, minv, n_inst, cam, queues, fb, depth))) return rc;
  if ((rc = gvt_hip_fb_clear(fb))) return rc;                                                  // clearBuffer :142
  for (size_t i = 0; i < n_inst; i++) if ((rc = gvt_hip_queue_clear(queues[i]))) return rc;
  if ((rc = volume_camera_step(T, cam, queues, fb, depth, nullptr))) return rc;               // generateRays :137 + shuffleRays(rays, -1)
  uint64_t calls = 0;
  for (;;) {                                                                                   // :159-259
    int target = -1;
    size_t cnt = 0;
    for (size_t i = 0; i < n_inst; i++)
      if (queues[i]->size > cnt) { cnt = queues[i]->size; target = (int)i; }
    if (target < 0) break;
    if ((rc = volume_march(volumes[target], queues[target], minv + 16 * (size_t)target, depth != nullptr))) return rc;
    calls++;
    if ((rc = shuffle_volume_impl(T, queues[target], target, queues, fb))) return rc;       // shuffleRays(moved_rays, instTarget) :252
  }
  if (adapter_calls) *adapter_calls = calls;
  return 0;
}

extern "C" int gvt_hip_volume_frame(gvt_hip_top *T, gvt_hip_volume *const *volumes, const float *m, const float *minv, size_t n_inst, const gvt_hip_camera *cam,
                                    gvt_hip_queue *const *queues, gvt_hip_fb *fb, uint64_t *adapter_calls) {
  return volume_frame_impl(T, volumes, m, minv, n_inst, cam, queues, fb, nullptr, adapter_calls);
}

extern "C" int gvt_hip_volume_frame_clipped(gvt_hip_top *T, gvt_hip_volume *const *volumes, const float *m, const float *minv, size_t n_inst, const gvt_hip_camera *cam,
                                            gvt_hip_queue *const *queues, gvt_hip_fb *fb, const gvt_hip_depth *depth, uint64_t *adapter_calls) {
  return volume_frame_impl(T, volumes, m, minv, n_inst, cam, queues, fb, depth, adapter_calls);
}

// ---- the fused frame (the contract: include/gvt_hip.h, "fused frame"; the kernel: volume_fused.inc)
namespace {

bool same_bits(const void *a, const void *b, size_t bytes) { return std::memcmp(a, b, bytes) == 0; }

// Eligibility, decided per call from the volumes as they are now: bricks of ONE grid (global origin, spacing, dt, table, value range, skip
// flag and minv equal as bits), one voxel type, no subgrids without GVT_HIP_FUSED_AMR, and nothing the kernels allowed do not do.  allow = 0 (gvt_hip_volume_frame_fused):
// no surfaces and no lit shading (the gradient kind is inert then).  GVT_HIP_FUSED_SURFACES / _LIT drop those two clauses; a frame that
// has an isovalue or effective lit shading then needs the cell gradient on every brick -- or, with GVT_HIP_FUSED_CENTRAL, ONE kind on
// every brick -- and what the bricks must share of surfaces and lights is compared as bits too.  features: the bits of `allow` the frame
// needs (0: the plain fused kernel; GVT_HIP_FUSED_CENTRAL: the bricks shade with CENTRAL, the kernels' CENTRAL instantiations run;
// GVT_HIP_FUSED_AMR: at least one brick has subgrids, the AMR instantiations run -- such a brick is F32 and CELL, the setters see to it, so
// a frame that reads a gradient and mixes it with CENTRAL bricks falls out through the "mixed kinds" clause)
bool fused_eligible(gvt_hip_volume *const *volumes, const float *minv, size_t n_inst, uint32_t allow, uint32_t &features, const char **why = nullptr) {
  features = 0;
  const auto no = [&](const char *clause) { // (why: the clause that fails, for the entry point that refuses such a frame instead of taking the loop)
    if (why) *why = clause;
    return false;
  };
  if (n_inst < 1 || n_inst > VOL_DEST_MAX) return no("between 1 and 256 bricks");
  const gvt_hip_volume *A = volumes[0];
  const bool surf = A->n_iso + A->n_pl > 0, lit = A->shade == GVT_HIP_VOLUME_SHADE_GRADIENT && A->n_lights > 0;
  int kind = -1; // the gradient kind of the first brick that reads a gradient (none yet)
  bool amr = false; // a brick has subgrids
  if ((surf && !(allow & GVT_HIP_FUSED_SURFACES)) || (lit && !(allow & GVT_HIP_FUSED_LIT))) return no("a feature the allow word lacks");
  for (size_t i = 0; i < n_inst; i++) {
    const gvt_hip_volume *B = volumes[i];
    if (!B->has_tf) return no("a brick without a transfer function");
    if (!B->sub.empty() && !(allow & GVT_HIP_FUSED_AMR)) return no("a brick with AMR subgrids");
    amr = amr || !B->sub.empty();
    if ((B->n_iso + B->n_pl > 0) != surf || (B->shade == GVT_HIP_VOLUME_SHADE_GRADIENT && B->n_lights > 0) != lit) return no("bricks that differ in having surfaces or lit shading");
    if (B->n_iso > 0 || lit) { // (planes alone read no gradient: the kind is inert)
      if (B->grad == GVT_HIP_VOLUME_GRADIENT_CENTRAL && !(allow & GVT_HIP_FUSED_CENTRAL)) return no("central gradients on a brick of a frame with an isovalue or lit shading");
      if (kind >= 0 && B->grad != kind) return no("bricks that mix cell and central gradients in a frame with an isovalue or lit shading");
      kind = B->grad;
      // (the CENTRAL kernels take the global grid's size from volumes[0] alone: a brick that counts the grid otherwise would find its boundary elsewhere)
      if (kind == GVT_HIP_VOLUME_GRADIENT_CENTRAL && !same_bits(B->gn, A->gn, sizeof(A->gn))) return no("central gradients on bricks of different grids (global counts)");
    }
    if (B->vtype != A->vtype || B->skip != A->skip) return no("bricks of different voxel types or skip flags");
    if (!same_bits(B->go, A->go, sizeof(A->go)) || !same_bits(B->sp, A->sp, sizeof(A->sp)) || !same_bits(&B->dt, &A->dt, sizeof(float))) return no("bricks of different grids");
    if (!same_bits(&B->tf_lo, &A->tf_lo, sizeof(float)) || !same_bits(&B->tf_hi, &A->tf_hi, sizeof(float))) return no("bricks with different transfer functions");
    if (!same_bits(B->tf_a, A->tf_a, sizeof(A->tf_a)) || !same_bits(B->tf_rgb, A->tf_rgb, sizeof(A->tf_rgb))) return no("bricks with different transfer functions");
    if (!same_bits(minv + 16 * i, minv, 16 * sizeof(float))) return no("bricks under different matrices");
    if (surf) { // (entries beyond n_iso / n_pl are never read)
      if (B->n_iso != A->n_iso || B->n_pl != A->n_pl || !same_bits(&B->surf_alpha, &A->surf_alpha, sizeof(float))) return no("bricks with different surfaces");
      if (!same_bits(B->iso, A->iso, sizeof(float) * (size_t)A->n_iso) || !same_bits(B->plane, A->plane, sizeof(A->plane[0]) * (size_t)A->n_pl)) return no("bricks with different surfaces");
    }
    if (surf || lit) { // (a surface frame without effective lit shading still lights its crossings: surf_composite)
      if (B->n_lights != A->n_lights || B->shade != A->shade || !same_bits(&B->ka, &A->ka, sizeof(float)) || !same_bits(&B->kd, &A->kd, sizeof(float))) return no("bricks with different lights or shading");
      if (!same_bits(B->lpos, A->lpos, sizeof(A->lpos[0]) * (size_t)A->n_lights) || !same_bits(B->lcol, A->lcol, sizeof(A->lcol[0]) * (size_t)A->n_lights)) return no("bricks with different lights or shading");
    }
  }
  features = (surf ? GVT_HIP_FUSED_SURFACES : 0u) | (lit ? GVT_HIP_FUSED_LIT : 0u) | (kind == GVT_HIP_VOLUME_GRADIENT_CENTRAL ? GVT_HIP_FUSED_CENTRAL : 0u) |
             (amr ? GVT_HIP_FUSED_AMR : 0u);
  return true;
}

// Runtime booleans as std::bool_constant arguments of a generic lambda: THE place a launcher turns flags into a kernel's boolean template
// arguments.  A launcher names each instantiation once; which combinations exist is what its lambda spells, no more
template <typename Fn>
void with_bools(Fn f) { f(); }
template <typename Fn, typename... Bools>
void with_bools(Fn f, bool b, Bools... rest) {
  if (b) with_bools([&](auto... c) { f(std::true_type{}, c...); }, rest...);
  else with_bools([&](auto... c) { f(std::false_type{}, c...); }, rest...);
}

// the clip plane's two kernel arguments: the depth plane and its size, or none (the CLIP instantiations alone read them)
struct ClipArgs { const float *d_t; unsigned n_clip; };
ClipArgs clip_args(const gvt_hip_depth *depth) {
  return depth ? ClipArgs{ depth->d_t, (unsigned)(depth->w * depth->h) } : ClipArgs{ nullptr, 0u };
}

// The launchers below: the kernel's instantiation for the frame's features, clipped (depth) or not, and its by-value tables.  CENTRAL: the
// instantiation, decided by the caller from GVT_HIP_FUSED_CENTRAL in the features; the argument list (tail: the framebuffer, the work
// counter, the counters) then ends in the ghost table (FusedGhost), else in NoGhost.
// The shaded fused kernel: one of the three shaded combinations
template <typename VT, bool CENTRAL, typename... Tail>
void launch_fused_shaded(uint32_t features, const gvt_hip_volume *V0, const gvt_hip_depth *depth, unsigned blocks, hipStream_t st, VolDev U, const FusedBrick *d_bricks,
                         TopDev top, RayPlanes P, unsigned n, const Mat4 &M, Tail... tail) {
  const bool surf = (features & GVT_HIP_FUSED_SURFACES) != 0;
  const ClipArgs c = clip_args(depth);
  with_bools([&](auto clip, auto lit) {
    if (surf) k_volume_march_fused_shaded<VT, clip.value, true, lit.value, CENTRAL><<<blocks, VOL_BLOCK, 0, st>>>(U, surf_dev(V0, M), d_bricks, top, P, n, M, c.d_t, c.n_clip, tail...);
    else k_volume_march_fused_shaded<VT, clip.value, false, true, CENTRAL><<<blocks, VOL_BLOCK, 0, st>>>(U, light_dev(V0, M), d_bricks, top, P, n, M, c.d_t, c.n_clip, tail...);
  }, depth != nullptr, (features & GVT_HIP_FUSED_LIT) != 0);
}

// the AMR kernels (GVT_HIP_FUSED_AMR is among the features): plain, or one of the three shaded combinations
template <typename... Tail>
void launch_fused_amr(uint32_t features, const gvt_hip_volume *V0, const gvt_hip_depth *depth, unsigned blocks, hipStream_t st, VolDev U, const FusedBrick *d_bricks,
                      const AmrDev *d_amr, TopDev top, RayPlanes P, unsigned n, const Mat4 &M, Tail... tail) {
  const bool surf = (features & GVT_HIP_FUSED_SURFACES) != 0, lit = (features & GVT_HIP_FUSED_LIT) != 0;
  const ClipArgs c = clip_args(depth);
  with_bools([&](auto clip, auto lit_c) {
    if (surf) k_volume_march_fused_shaded_amr<clip.value, true, lit_c.value><<<blocks, VOL_BLOCK, 0, st>>>(U, surf_dev(V0, M), d_bricks, d_amr, top, P, n, M, c.d_t, c.n_clip, tail...);
    else if (lit) k_volume_march_fused_shaded_amr<clip.value, false, true><<<blocks, VOL_BLOCK, 0, st>>>(U, light_dev(V0, M), d_bricks, d_amr, top, P, n, M, c.d_t, c.n_clip, tail...);
    else k_volume_march_fused_amr<clip.value><<<blocks, VOL_BLOCK, 0, st>>>(U, d_bricks, d_amr, top, P, n, M, c.d_t, c.n_clip, tail...);
  }, depth != nullptr, lit);
}

// the shadowed kernel: lit fog or not (surfaces are implied)
template <typename VT, bool CENTRAL, typename... Tail>
void launch_fused_shadow(uint32_t features, const gvt_hip_depth *depth, unsigned blocks, hipStream_t st, VolDev U, SurfDev S, ShadowDev H, const FusedBrick *d_bricks,
                         TopDev top, RayPlanes P, unsigned n, const Mat4 &M, Tail... tail) {
  const ClipArgs c = clip_args(depth);
  with_bools([&](auto clip, auto lit) {
    k_volume_march_fused_shadow<VT, clip.value, lit.value, CENTRAL><<<blocks, VOL_BLOCK, 0, st>>>(U, S, H, d_bricks, top, P, n, M, c.d_t, c.n_clip, tail...);
  }, depth != nullptr, (features & GVT_HIP_FUSED_LIT) != 0);
}

// the fog-shadowed kernels (lit fog is implied): with surfaces or -- the lean kernel -- without
template <typename VT, bool CENTRAL, typename... Tail>
void launch_fused_fog(uint32_t features, const gvt_hip_volume *V0, const gvt_hip_depth *depth, unsigned blocks, hipStream_t st, VolDev U, SurfDev S, ShadowDev H,
                      const FusedBrick *d_bricks, const FogBrick *d_grids, TopDev top, RayPlanes P, unsigned n, const Mat4 &M, Tail... tail) {
  const bool surf = (features & GVT_HIP_FUSED_SURFACES) != 0;
  const ClipArgs c = clip_args(depth);
  with_bools([&](auto clip) {
    if (surf) k_volume_march_fused_fog<VT, clip.value, CENTRAL><<<blocks, VOL_BLOCK, 0, st>>>(U, S, H, d_bricks, d_grids, top, P, n, M, c.d_t, c.n_clip, tail...);
    else k_volume_march_fused_fog_lean<VT, clip.value, CENTRAL><<<blocks, VOL_BLOCK, 0, st>>>(U, light_dev(V0, M), H.usable, d_bricks, d_grids, top, P, n, M, c.d_t, c.n_clip, tail...);
  }, depth != nullptr);
}

// the mesh-shadowed kernels: lit fog or not, with surfaces or -- the lean kernel, lit fog implied -- without
template <typename VT, bool CENTRAL, typename... Tail>
void launch_fused_mesh(uint32_t features, const gvt_hip_volume *V0, const gvt_hip_depth *depth, unsigned blocks, hipStream_t st, VolDev U, SurfDev S, ShadowDev H,
                       const FusedBrick *d_bricks, const MeshBrick *d_grids, TopDev top, RayPlanes P, unsigned n, const Mat4 &M, Tail... tail) {
  const bool surf = (features & GVT_HIP_FUSED_SURFACES) != 0;
  const ClipArgs c = clip_args(depth);
  with_bools([&](auto clip, auto lit) {
    if (surf) k_volume_march_fused_mesh<VT, clip.value, lit.value, CENTRAL><<<blocks, VOL_BLOCK, 0, st>>>(U, S, H, d_bricks, d_grids, top, P, n, M, c.d_t, c.n_clip, tail...);
    else k_volume_march_fused_mesh_lean<VT, clip.value, CENTRAL><<<blocks, VOL_BLOCK, 0, st>>>(U, light_dev(V0, M), H.usable, d_bricks, d_grids, top, P, n, M, c.d_t, c.n_clip, tail...);
  }, depth != nullptr, (features & GVT_HIP_FUSED_LIT) != 0);
}

// the AO kernels (the AO frame: a usable light exists): lit fog or not, with surfaces or -- the lean kernel, lit fog implied -- without;
// mesh: the base frame is the mesh-shadowed one
template <typename VT, bool CENTRAL, typename... Tail>
void launch_fused_ao(uint32_t features, bool mesh, const gvt_hip_volume *V0, const gvt_hip_depth *depth, unsigned blocks, hipStream_t st, VolDev U, SurfDev S, ShadowDev H,
                     const FusedBrick *d_bricks, const AoBrick *d_grids, TopDev top, RayPlanes P, unsigned n, const Mat4 &M, Tail... tail) {
  const bool surf = (features & GVT_HIP_FUSED_SURFACES) != 0;
  const ClipArgs c = clip_args(depth);
  with_bools([&](auto clip, auto lit, auto mesh_c) {
    if (surf) k_volume_march_fused_ao<VT, clip.value, lit.value, CENTRAL, mesh_c.value><<<blocks, VOL_BLOCK, 0, st>>>(U, S, H, d_bricks, d_grids, top, P, n, M, c.d_t, c.n_clip, tail...);
    else k_volume_march_fused_ao_lean<VT, clip.value, CENTRAL, mesh_c.value><<<blocks, VOL_BLOCK, 0, st>>>(U, light_dev(V0, M), H.usable, d_bricks, d_grids, top, P, n, M, c.d_t, c.n_clip, tail...);
  }, depth != nullptr, (features & GVT_HIP_FUSED_LIT) != 0, mesh);
}

// the shadowed AMR kernels (GVT_HIP_FUSED_AMR is among the features; float32, CELL): the kernel of the shadowed, the fog-shadowed (fog) or
// the mesh-shadowed (mesh) frame, lit fog or not, with surfaces or -- the lean kernels -- without.  d_grids: the bricks' planes (fog or
// mesh), else null
template <typename... Tail>
void launch_fused_shadow_amr(uint32_t features, bool fog, bool mesh, const gvt_hip_volume *V0, const gvt_hip_depth *depth, unsigned blocks, hipStream_t st, VolDev U, SurfDev S,
                             ShadowDev H, const FusedBrick *d_bricks, const AmrDev *d_amr, const MeshBrick *d_grids, TopDev top, RayPlanes P, unsigned n, const Mat4 &M,
                             Tail... tail) {
  const bool lean = (fog || mesh) && !(features & GVT_HIP_FUSED_SURFACES);
  const ClipArgs c = clip_args(depth);
  with_bools([&](auto clip, auto lit) {
    if (lean && mesh) k_volume_march_fused_mesh_lean_amr<clip.value><<<blocks, VOL_BLOCK, 0, st>>>(U, light_dev(V0, M), H.usable, d_bricks, d_amr, d_grids, top, P, n, M, c.d_t, c.n_clip, tail...);
    else if (lean) k_volume_march_fused_fog_lean_amr<clip.value><<<blocks, VOL_BLOCK, 0, st>>>(U, light_dev(V0, M), H.usable, d_bricks, d_amr, d_grids, top, P, n, M, c.d_t, c.n_clip, tail...);
    else if (mesh) k_volume_march_fused_mesh_amr<clip.value, lit.value><<<blocks, VOL_BLOCK, 0, st>>>(U, S, H, d_bricks, d_amr, d_grids, top, P, n, M, c.d_t, c.n_clip, tail...);
    else if (fog) k_volume_march_fused_fog_amr<clip.value><<<blocks, VOL_BLOCK, 0, st>>>(U, S, H, d_bricks, d_amr, d_grids, top, P, n, M, c.d_t, c.n_clip, tail...);
    else k_volume_march_fused_shadow_amr<clip.value, lit.value><<<blocks, VOL_BLOCK, 0, st>>>(U, S, H, d_bricks, d_amr, top, P, n, M, c.d_t, c.n_clip, tail...);
  }, depth != nullptr, (features & GVT_HIP_FUSED_LIT) != 0);
}

// a brick's record of the fused kernels' table (FusedBrick, volume_fused.inc).  cell_words: mc is the per-cell words of the surface visit,
// which never reads the skip bytes (without surfaces the words hold the skip bit alone).  nb = (n - 1 + 7) / 8: the kernels recompute it
FusedBrick fused_record(const gvt_hip_volume *B, bool cell_words) {
  FusedBrick R{};
  R.vox = B->d_vox;
  R.mc = cell_words ? (const uint8_t *)B->d_cells : B->d_mc;
  R.nx = B->n[0]; R.ny = B->n[1]; R.nz = B->n[2]; R.ox = B->off[0]; R.oy = B->off[1]; R.oz = B->off[2];
  for (int a = 0; a < 3; a++) { R.lo[a] = B->lo[a]; R.hi[a] = B->hi[a]; }
  return R;
}
// ... and its four AMR pointers beside it (AmrDev, volume_fused_amr.inc): null on a brick without subgrids
AmrDev amr_record(const gvt_hip_volume *B) {
  return B->sub.empty() ? AmrDev{ nullptr, nullptr, nullptr, nullptr } : AmrDev{ B->d_amr_mc, B->d_amr_list, B->d_amr_desc, B->d_amr_vox };
}

// the frame in one launch: camera list, brick table (through the pinned staging block), march, ONE host wait (the counters' read-back).
// features: fused_eligible's -- 0 launches k_volume_march_fused, anything else the shaded kernel with the table of volumes[0]
// shadow (gvt_hip_volume_frame_shadowed; features has SURFACES then): the launch is k_volume_march_fused_shadow's, and shadow_out gets
// its five further counter words, read back in the same wait.  fog (gvt_hip_volume_frame_fog_shadowed; shadow is given and features has
// LIT): the launch is k_volume_march_fused_fog's, and the bricks' light grid planes travel in a second table beside the records.  mesh
// (gvt_hip_volume_frame_mesh_shadowed; shadow is given): the launch is k_volume_march_fused_mesh's, and that table holds the occluder
// grid's planes too (the light grid's only where fog is set as well).  GVT_HIP_FUSED_AMR in features (never with
// GVT_HIP_FUSED_CENTRAL: a brick with subgrids is CELL): the launch is the AMR kernels' -- with shadow, fog or mesh those of
// volume_fused_shadow_amr.inc (GVT_HIP_VOLUME_ALLOW_AMR) -- the bricks' AMR tables travel in a further table beside the records and the
// planes, read from the volumes NOW, and *refined_out gets the seventh counter (the shadowed kernels do not count it).  ao
// (gvt_hip_volume_frame_ao; shadow is given with a usable light, never with GVT_HIP_FUSED_AMR): the launch is k_volume_march_fused_ao's, and
// the table holds three pointers a brick (AoBrick): the light grid's where fog is set, the occluder grid's where mesh is, the AO grid's
int volume_frame_fused(gvt_hip_top *T, gvt_hip_volume *const *volumes, const float *minv, size_t n_inst, const gvt_hip_camera *cam, gvt_hip_queue *const *queues,
                       gvt_hip_fb *fb, const gvt_hip_depth *depth, uint32_t features, gvt_hip_volume_fused_shaded_stats &S, const ShadowDev *shadow = nullptr,
                       uint64_t *shadow_out = nullptr, bool fog = false, bool mesh = false, uint64_t *refined_out = nullptr, bool ao = false) {
  Ctx &C = gctx();
  int rc;
  if ((rc = gvt_hip_fb_clear(fb))) return rc;
  for (size_t i = 0; i < n_inst; i++) if ((rc = gvt_hip_queue_clear(queues[i]))) return rc;
  if (!staging_queues(C)) return GVT_HIP_ERR_DEVICE;
  gvt_hip_queue *q_cam = C.abi_qout; // (volume_camera_step's staging list)
  if ((rc = gvt_hip_camera_generate_tiled(q_cam, cam->eye, cam->focus, cam->up, cam->fov, cam->width, cam->height, cam->samples, 0,
                                          cam->jitter_window_size, 8))) return rc;
  const size_t n = q_cam->size;
  FusedBrick *d_bricks = (FusedBrick *)scratch_get(SCR_VOL_BRICKS, sizeof(FusedBrick) * n_inst);
  static_assert(VOL_FUSED_SHADED_STATS >= VOL_FUSED_STATS, "one block of counter words serves both kernels");
  static_assert(VOL_FUSED_SHADOW_STATS >= VOL_FUSED_SHADED_STATS, "... and the shadowed kernel");
  static_assert(VOL_FUSED_SHADOW_STATS >= VOL_FUSED_AMR_STATS && VOL_FUSED_AMR_REFINED == VOL_FUSED_SHADED_STATS, "... and the AMR kernels, whose word follows the shaded kernel's six");
  const bool amr = (features & GVT_HIP_FUSED_AMR) != 0;
  const size_t n_words = shadow ? VOL_FUSED_SHADOW_STATS : amr ? VOL_FUSED_AMR_STATS : VOL_FUSED_SHADED_STATS;
  unsigned long long *d_stats = (unsigned long long *)scratch_get(SCR_VOL_FUSED, VOL_FUSED_SHADOW_STATS * sizeof(unsigned long long));
  unsigned *work = (unsigned *)scratch_get(SCR_VOL_WORK, sizeof(unsigned));
  if (!d_bricks || !d_stats || !work) return GVT_HIP_ERR_DEVICE;
  static_assert(sizeof(MeshBrick) >= sizeof(FogBrick), "one allocation serves either table");
  void *d_planes = ao ? scratch_get(SCR_VOL_GRIDS, sizeof(AoBrick) * n_inst) : (fog || mesh) ? scratch_get(SCR_VOL_GRIDS, sizeof(MeshBrick) * n_inst) : nullptr;
  if ((ao || fog || mesh) && !d_planes) return GVT_HIP_ERR_DEVICE;
  AoBrick *d_agrids = (AoBrick *)d_planes;
  FogBrick *d_grids = (FogBrick *)d_planes;
  MeshBrick *d_mgrids = (MeshBrick *)d_planes;
  // the CENTRAL instantiations' ghost table: the bricks' face pointers, beside the records (FusedGhost, volume_fused.inc)
  const bool central = (features & GVT_HIP_FUSED_CENTRAL) != 0;
  const void **d_faces = central ? (const void **)scratch_get(SCR_VOL_GHOSTS, sizeof(void *) * n_inst) : nullptr;
  if (central && !d_faces) return GVT_HIP_ERR_DEVICE;
  // the AMR instantiations' table: the bricks' four AMR pointers, beside the records (AmrDev, volume_fused_amr.inc)
  AmrDev *d_amr = amr ? (AmrDev *)scratch_get(SCR_VOL_AMR, sizeof(AmrDev) * n_inst) : nullptr;
  if (amr && !d_amr) return GVT_HIP_ERR_DEVICE;
  static_assert((sizeof(FusedBrick) + sizeof(MeshBrick) + sizeof(void *)) * VOL_DEST_MAX <= PINNED_STAGE_BYTES, "the brick table, the grids' and the ghosts' fit the staging block");
  static_assert((sizeof(FusedBrick) + sizeof(MeshBrick) + sizeof(AmrDev)) * VOL_DEST_MAX <= PINNED_STAGE_BYTES, "... and so do the brick table, the grids' and the AMR table, which takes the ghosts' place (an AMR frame is never CENTRAL)");
  static_assert((sizeof(FusedBrick) + sizeof(AoBrick) + sizeof(void *)) * VOL_DEST_MAX <= PINNED_STAGE_BYTES, "... and the AO frame's brick table, planes and ghosts");
  void *stage = nullptr;
  if ((rc = pinned_stage_begin(&stage))) return rc;
  FusedBrick *h = (FusedBrick *)stage;
  FogBrick *hg = (FogBrick *)(h + VOL_DEST_MAX);
  MeshBrick *hm = (MeshBrick *)(h + VOL_DEST_MAX);
  AoBrick *ho = (AoBrick *)(h + VOL_DEST_MAX);
  const void **hf = ao ? (const void **)(ho + VOL_DEST_MAX) : (const void **)(hm + VOL_DEST_MAX);
  AmrDev *ha = (AmrDev *)(hm + VOL_DEST_MAX);
  for (size_t i = 0; i < n_inst; i++) {
    const gvt_hip_volume *B = volumes[i];
    h[i] = fused_record(B, (features & GVT_HIP_FUSED_SURFACES) != 0);
    if (ao) ho[i] = AoBrick{ fog ? B->d_lgrid : nullptr, mesh ? B->d_occ : nullptr, B->d_ao };
    else if (mesh) hm[i] = MeshBrick{ fog ? B->d_lgrid : nullptr, B->d_occ };
    else if (fog && amr) hm[i] = MeshBrick{ B->d_lgrid, nullptr };
    else if (fog) hg[i].grid = B->d_lgrid;
    if (central) hf[i] = B->d_ghost; // (null on a brick without an interior face: none of its layers is ever read)
    if (amr) ha[i] = amr_record(B);
  }
  HIPCHK(hipMemcpyAsync(d_bricks, h, sizeof(FusedBrick) * n_inst, hipMemcpyHostToDevice, C.stream));
  if (ao) HIPCHK(hipMemcpyAsync(d_agrids, ho, sizeof(AoBrick) * n_inst, hipMemcpyHostToDevice, C.stream));
  else if (mesh || (fog && amr)) HIPCHK(hipMemcpyAsync(d_mgrids, hm, sizeof(MeshBrick) * n_inst, hipMemcpyHostToDevice, C.stream));
  else if (fog) HIPCHK(hipMemcpyAsync(d_grids, hg, sizeof(FogBrick) * n_inst, hipMemcpyHostToDevice, C.stream));
  if (central) HIPCHK(hipMemcpyAsync(d_faces, hf, sizeof(void *) * n_inst, hipMemcpyHostToDevice, C.stream));
  if (amr) HIPCHK(hipMemcpyAsync(d_amr, ha, sizeof(AmrDev) * n_inst, hipMemcpyHostToDevice, C.stream));
  if ((rc = pinned_stage_end())) return rc;
  HIPCHK(hipMemsetAsync(work, 0, sizeof(unsigned), C.stream));
  HIPCHK(hipMemsetAsync(d_stats, 0, n_words * sizeof(unsigned long long), C.stream));
  Mat4 M;
  for (int k = 0; k < 16; k++) M.m[k] = minv[k];
  const unsigned blocks = std::min(blocks_of(n), (unsigned)(std::max(C.n_cu, 1) * 8));
  const RayPlanes P = make_planes(q_cam->d_planes, q_cam->cap);
  const unsigned n_pix = (unsigned)(fb->w * fb->h);
  const FusedGhost HG{ d_faces, volumes[0]->gn[0], volumes[0]->gn[1], volumes[0]->gn[2] };
  const gvt_hip_volume *V0 = volumes[0];
  if (n && amr && shadow) // (the fog frame's table is a MeshBrick table here, its occluder pointers null)
    launch_fused_shadow_amr(features, fog, mesh, V0, depth, blocks, C.stream, vol_dev(V0), surf_dev(V0, M), *shadow, d_bricks, d_amr, d_mgrids, T->dev(), P, (unsigned)n, M,
                            fb->d_rgba, n_pix, work, d_stats);
  else if (n && amr) // (F32 and CELL: fused_eligible has compared the voxel types, and a brick with subgrids is F32)
    launch_fused_amr(features, V0, depth, blocks, C.stream, vol_dev(V0), d_bricks, d_amr, T->dev(), P, (unsigned)n, M, fb->d_rgba, n_pix, work, d_stats);
  else if (n)
    with_voxel_type(V0->vtype, [&](auto t) {
      using VT = decltype(t);
      // the shaded launches, for the kernels' CENTRAL instantiation (gh: FusedGhost) or the other (NoGhost)
      const auto shaded = [&](auto central_c, auto gh) {
        constexpr bool CENTRAL = decltype(central_c)::value;
        if (shadow && ao)
          launch_fused_ao<VT, CENTRAL>(features, mesh, V0, depth, blocks, C.stream, vol_dev(V0), surf_dev(V0, M), *shadow, d_bricks, d_agrids, T->dev(), P, (unsigned)n, M, fb->d_rgba,
                                       n_pix, work, d_stats, gh);
        else if (shadow && mesh)
          launch_fused_mesh<VT, CENTRAL>(features, V0, depth, blocks, C.stream, vol_dev(V0), surf_dev(V0, M), *shadow, d_bricks, d_mgrids, T->dev(), P, (unsigned)n, M, fb->d_rgba, n_pix,
                                         work, d_stats, gh);
        else if (shadow && fog)
          launch_fused_fog<VT, CENTRAL>(features, V0, depth, blocks, C.stream, vol_dev(V0), surf_dev(V0, M), *shadow, d_bricks, d_grids, T->dev(), P, (unsigned)n, M, fb->d_rgba, n_pix,
                                        work, d_stats, gh);
        else if (shadow)
          launch_fused_shadow<VT, CENTRAL>(features, depth, blocks, C.stream, vol_dev(V0), surf_dev(V0, M), *shadow, d_bricks, T->dev(), P, (unsigned)n, M, fb->d_rgba, n_pix, work,
                                           d_stats, gh);
        else
          launch_fused_shaded<VT, CENTRAL>(features, V0, depth, blocks, C.stream, vol_dev(V0), d_bricks, T->dev(), P, (unsigned)n, M, fb->d_rgba, n_pix, work, d_stats, gh);
      };
      if (shadow || features) {
        if (central) shaded(std::true_type{}, HG);
        else shaded(std::false_type{}, NoGhost{});
        return;
      }
      const ClipArgs c = clip_args(depth);
      with_bools([&](auto clip) {
        k_volume_march_fused<VT, clip.value><<<blocks, VOL_BLOCK, 0, C.stream>>>(vol_dev(V0), d_bricks, T->dev(), P, (unsigned)n, M, c.d_t, c.n_clip, fb->d_rgba, n_pix, work, d_stats);
      }, depth != nullptr);
    });
  HIPCHK(hipGetLastError());
  // (pinned words 16..27 of the context: six 64-bit counters, and 28..29 the AMR kernels' seventh; 30..31 are free, 32..41 the builder's; the shadowed frame's eleven are words 42..63)
  static_assert(16 + 2 * VOL_FUSED_AMR_STATS <= 32, "the AMR frame's counters end before the builder's words");
  static_assert(42 + 2 * VOL_FUSED_SHADOW_STATS <= 64, "the context has 64 pinned words");
  unsigned long long *h_stats = (unsigned long long *)(C.h_pinned + (shadow ? 42 : 16));
  HIPCHK(hipMemcpyAsync(h_stats, d_stats, n_words * sizeof(unsigned long long), hipMemcpyDeviceToHost, C.stream));
  if ((rc = gvt_hip_queue_clear(q_cam))) return rc;
  HIPCHK(hipStreamSynchronize(C.stream));
  S.fused = 1; S.adapter_calls = 1; S.features = features;
  S.samples_marched = h_stats[0]; S.samples_gathered = h_stats[1]; S.brick_visits = h_stats[2]; S.rays_deposited = h_stats[3];
  S.crossings_rendered = h_stats[4]; S.samples_shaded = h_stats[5]; // (0 from the plain kernel: the words were cleared)
  if (refined_out) *refined_out = amr ? h_stats[VOL_FUSED_AMR_REFINED] : 0;
  if (shadow && shadow_out)
    for (int i = 0; i < VOL_FUSED_SHADOW_STATS - VOL_FUSED_SHADED_STATS; i++) shadow_out[i] = h_stats[VOL_FUSED_SHADED_STATS + i];
  return 0;
}

// both fused entry points: the arguments' errors, then the fused frame where the frame is eligible under `allow`, else the loop
int volume_frame_fused_or_loop(gvt_hip_top *T, gvt_hip_volume *const *volumes, const float *m, const float *minv, size_t n_inst, const gvt_hip_camera *cam,
                               gvt_hip_queue *const *queues, gvt_hip_fb *fb, const gvt_hip_depth *depth, uint32_t allow, gvt_hip_volume_fused_shaded_stats &S,
                               uint64_t *refined_out = nullptr) {
  int rc;
  if ((rc = volume_frame_args(T, volumes, m, minv, n_inst, cam, queues, fb, depth))) return rc;
  uint32_t features = 0;
  if (fused_eligible(volumes, minv, n_inst, allow, features))
    return volume_frame_fused(T, volumes, minv, n_inst, cam, queues, fb, depth, features, S, nullptr, nullptr, false, false, refined_out);
  return volume_frame_impl(T, volumes, m, minv, n_inst, cam, queues, fb, depth, &S.adapter_calls); // (not an error: the loop, fused = 0)
}

} // namespace

extern "C" int gvt_hip_volume_frame_fused(gvt_hip_top *T, gvt_hip_volume *const *volumes, const float *m, const float *minv, size_t n_inst, const gvt_hip_camera *cam,
                                          gvt_hip_queue *const *queues, gvt_hip_fb *fb, const gvt_hip_depth *depth, gvt_hip_volume_fused_stats *stats) {
  gvt_hip_volume_fused_shaded_stats S{};
  const int rc = volume_frame_fused_or_loop(T, volumes, m, minv, n_inst, cam, queues, fb, depth, 0u, S);
  if (!rc && stats) {
    gvt_hip_volume_fused_stats O{};
    O.fused = S.fused; O.samples_marched = S.samples_marched; O.samples_gathered = S.samples_gathered; O.brick_visits = S.brick_visits;
    O.rays_deposited = S.rays_deposited; O.adapter_calls = S.adapter_calls;
    *stats = O;
  }
  return rc;
}

extern "C" int gvt_hip_volume_frame_fused_shaded(gvt_hip_top *T, gvt_hip_volume *const *volumes, const float *m, const float *minv, size_t n_inst,
                                                 const gvt_hip_camera *cam, gvt_hip_queue *const *queues, gvt_hip_fb *fb, const gvt_hip_depth *depth, uint32_t allow,
                                                 gvt_hip_volume_fused_shaded_stats *stats) {
  if (allow & ~(uint32_t)(GVT_HIP_FUSED_SURFACES | GVT_HIP_FUSED_LIT | GVT_HIP_FUSED_CENTRAL)) { set_error("volume_frame_fused_shaded: unknown allow bits %u", allow); return GVT_HIP_ERR_INVALID; }
  gvt_hip_volume_fused_shaded_stats S{};
  const int rc = volume_frame_fused_or_loop(T, volumes, m, minv, n_inst, cam, queues, fb, depth, allow, S);
  if (!rc && stats) *stats = S;
  return rc;
}

// the fused frame that may take bricks with subgrids (the contract: include/gvt_hip.h, "fused frame: AMR bricks"; the kernels: volume_fused_amr.inc)
extern "C" int gvt_hip_volume_frame_fused_amr(gvt_hip_top *T, gvt_hip_volume *const *volumes, const float *m, const float *minv, size_t n_inst, const gvt_hip_camera *cam,
                                              gvt_hip_queue *const *queues, gvt_hip_fb *fb, const gvt_hip_depth *depth, uint32_t allow,
                                              gvt_hip_volume_fused_amr_stats *stats) {
  if (allow & ~(uint32_t)(GVT_HIP_FUSED_SURFACES | GVT_HIP_FUSED_LIT | GVT_HIP_FUSED_CENTRAL | GVT_HIP_FUSED_AMR)) {
    set_error("volume_frame_fused_amr: unknown allow bits %u", allow);
    return GVT_HIP_ERR_INVALID;
  }
  gvt_hip_volume_fused_shaded_stats S{};
  uint64_t refined = 0;
  const int rc = volume_frame_fused_or_loop(T, volumes, m, minv, n_inst, cam, queues, fb, depth, allow, S, &refined);
  if (!rc && stats) {
    gvt_hip_volume_fused_amr_stats O{};
    O.fused = S.fused; O.features = S.features; O.samples_marched = S.samples_marched; O.samples_gathered = S.samples_gathered; O.brick_visits = S.brick_visits;
    O.rays_deposited = S.rays_deposited; O.adapter_calls = S.adapter_calls; O.crossings_rendered = S.crossings_rendered; O.samples_shaded = S.samples_shaded;
    O.samples_refined = refined;
    if (S.fused && (S.features & GVT_HIP_FUSED_AMR)) // (the bricks of the frame that had subgrids; 0 after the loop and after a frame without any)
      for (size_t i = 0; i < n_inst; i++) O.amr_bricks += volumes[i]->sub.empty() ? 0u : 1u;
    *stats = O;
  }
  return rc;
}

// ---- shadowed surfaces (the contract: include/gvt_hip.h, "shadowed surfaces"; the kernel: volume_fused_shadow.inc) and shadowed fog
// ("shadowed fog"; volume_light_grid.inc, volume_fused_fog.inc)
namespace {

// the shadow rays' directions: towards each light, in world space (the direction lights_dev's ldir is the negative of); t0 from the bias
ShadowDev shadow_dev(const gvt_hip_volume *A, int bias) {
  ShadowDev H{};
  for (int j = 0; j < A->n_lights; j++) {
    const float x = A->lpos[j][0], y = A->lpos[j][1], z = A->lpos[j][2];
    const float len = sqrtf((x * x + y * y) + z * z);
    if (!(len > 0.f && std::isfinite(len))) continue; // (no ray: T_j = 1)
    H.ws[j][0] = x / len; H.ws[j][1] = y / len; H.ws[j][2] = z / len;
    H.usable |= 1u << j;
  }
  H.t0 = (float)(bias - 1) * A->dt;
  return H;
}

// Do these bricks, in this order and under these matrices, all hold a grid (planes: d_lgrid or d_occ; grids: lg or og) of ONE bake that
// nothing has made stale since?  what / bake_fn / stale_by: the three words in which the light grids' messages and the occluder grids' differ
template <typename P>
bool grids_current(P *gvt_hip_volume::*planes, BakedGrids gvt_hip_volume::*grids, const char *what, const char *bake_fn, const char *stale_by,
                   gvt_hip_volume *const *volumes, const float *m, const float *minv, size_t n_inst, unsigned usable, std::string &why) {
  const std::string w(what);
  const BakedGrids &G0 = volumes[0]->*grids;
  for (size_t i = 0; i < n_inst; i++) {
    const BakedGrids &G = volumes[i]->*grids;
    if (!(volumes[i]->*planes)) why = "a brick holds no " + w + " grid (" + bake_fn + ")";
    else if (!G.current) why = "a brick's " + w + " grid is stale: its " + stale_by + " were set after the bake";
    else if (G.bake != G0.bake || G.index != i || G.count != n_inst) why = "the " + w + " grids were not baked over exactly these bricks in this order";
    else if (!same_bits(G.m, m + 16 * i, sizeof(G.m)) || !same_bits(G.minv, minv + 16 * i, sizeof(G.minv))) why = "the " + w + " grids were baked under another matrix";
    else if (G.usable != usable || G.planes != __builtin_popcount(usable)) why = "the " + w + " grids were baked for other lights";
    else continue;
    return false;
  }
  return true;
}

// a bake's commit on one brick (the planes' pointer is the caller's), and a release's reset
void grids_commit(BakedGrids &G, unsigned usable, uint64_t bake, size_t index, size_t count, const float *m, const float *minv) {
  G.planes = __builtin_popcount(usable); G.usable = usable; G.current = true;
  G.bake = bake; G.index = index; G.count = count;
  std::memcpy(G.m, m + 16 * index, sizeof(G.m));
  std::memcpy(G.minv, minv + 16 * index, sizeof(G.minv));
}
void grids_reset(BakedGrids &G) { G.planes = 0; G.usable = 0; G.current = false; G.bake = 0; }

// the shadowed frames.  fog: gvt_hip_volume_frame_fog_shadowed; mesh (with fog): gvt_hip_volume_frame_mesh_shadowed, *mesh_ran = did its
// kernel run?; ao (with fog): gvt_hip_volume_frame_ao, *ao_ran likewise (fn: the entry point's name in the error texts)
int volume_frame_shadowed_impl(const char *fn, bool fog, gvt_hip_top *T, gvt_hip_volume *const *volumes, const float *m, const float *minv, size_t n_inst,
                               const gvt_hip_camera *cam, gvt_hip_queue *const *queues, gvt_hip_fb *fb, const gvt_hip_depth *depth,
                               const gvt_hip_volume_shadow_params *params, gvt_hip_volume_shadow_stats &O, uint64_t &fog_samples, bool mesh = false,
                               bool *mesh_ran = nullptr, bool ao = false, bool *ao_ran = nullptr) {
  int rc;
  if ((rc = volume_frame_args(T, volumes, m, minv, n_inst, cam, queues, fb, depth))) return rc;
  if (!params) { set_error("%s: null params", fn); return GVT_HIP_ERR_INVALID; }
  if (params->flags & ~(uint32_t)(GVT_HIP_VOLUME_ALLOW_CENTRAL | GVT_HIP_VOLUME_ALLOW_AMR)) { set_error("%s: unknown flag bits %u", fn, params->flags); return GVT_HIP_ERR_INVALID; }
  const uint32_t allow = GVT_HIP_FUSED_SURFACES | GVT_HIP_FUSED_LIT | ((params->flags & GVT_HIP_VOLUME_ALLOW_CENTRAL) ? GVT_HIP_FUSED_CENTRAL : 0u) |
                         ((params->flags & GVT_HIP_VOLUME_ALLOW_AMR) ? GVT_HIP_FUSED_AMR : 0u);
  if (params->bias < 1 || params->bias > 64) { set_error("%s: bias %d, 1 to 64 lattice steps are allowed", fn, params->bias); return GVT_HIP_ERR_INVALID; }
  bool any_surface = false, any_light = false, any_lit = false;
  for (size_t i = 0; i < n_inst; i++) {
    any_surface = any_surface || volumes[i]->n_iso + volumes[i]->n_pl > 0;
    any_light = any_light || volumes[i]->n_lights > 0;
    any_lit = any_lit || (volumes[i]->shade == GVT_HIP_VOLUME_SHADE_GRADIENT && volumes[i]->n_lights > 0);
  }
  gvt_hip_volume_fused_shaded_stats S{};
  uint64_t sh[VOL_FUSED_SHADOW_STATS - VOL_FUSED_SHADED_STATS] = {};
  // nothing a shadow could fall on, or nothing that casts one (the fog frame: lit fog is something a shadow falls on)
  const bool inert = !any_light || (!any_surface && !(fog && any_lit));
  bool fog_ran = false;
  if (inert) {
    rc = volume_frame_fused_or_loop(T, volumes, m, minv, n_inst, cam, queues, fb, depth, allow, S);
  } else {
    uint32_t features = 0;
    const char *why = "";
    if (!fused_eligible(volumes, minv, n_inst, allow, features, &why)) { // (no loop renders shadows: refused, nothing changed)
      set_error("%s: the frame has %s and lights but is not eligible for the fused kernel: %s", fn, fog ? "surfaces or lit fog" : "surfaces", why);
      return GVT_HIP_ERR_INVALID;
    }
    const ShadowDev H = shadow_dev(volumes[0], params->bias);
    fog_ran = fog && (features & GVT_HIP_FUSED_LIT) && H.usable; // (no lit fog: gvt_hip_volume_frame_shadowed in every bit; no usable light: every Tg = 1, nothing is read)
    std::string stale;
    if (fog_ran && !grids_current(&gvt_hip_volume::d_lgrid, &gvt_hip_volume::lg, "light", "gvt_hip_volume_light_grid_bake", "samples, table, surfaces, lights or subgrids",
                                  volumes, m, minv, n_inst, H.usable, stale)) {
      set_error("%s: the frame has lit fog but its bricks do not all hold a current light grid: %s", fn, stale.c_str());
      return GVT_HIP_ERR_INVALID;
    }
    // (the mesh frame without a usable light is the fog-shadowed frame in every respect: no occluder grid is needed)
    const bool with_mesh = mesh && H.usable;
    if (with_mesh && !grids_current(&gvt_hip_volume::d_occ, &gvt_hip_volume::og, "occluder", "gvt_hip_volume_occluder_grid_bake", "lights or subgrids", volumes, m, minv,
                                    n_inst, H.usable, stale)) {
      set_error("%s: the frame has surfaces or lit fog but its bricks do not all hold a current occluder grid: %s", fn, stale.c_str());
      return GVT_HIP_ERR_INVALID;
    }
    // (the AO frame without a usable light is its base frame in every respect: no AO grid is needed)
    const bool with_ao = ao && H.usable;
    if (with_ao && !grids_current(&gvt_hip_volume::d_ao, &gvt_hip_volume::ag, "ao", "gvt_hip_volume_ao_grid_bake", "samples, table, surfaces or subgrids", volumes, m, minv,
                                  n_inst, 1u, stale)) {
      set_error("%s: the frame has surfaces or lit fog but its bricks do not all hold a current ao grid: %s", fn, stale.c_str());
      return GVT_HIP_ERR_INVALID;
    }
    if (fog && (features & GVT_HIP_FUSED_LIT) && !(features & GVT_HIP_FUSED_SURFACES) && !H.usable) // (lit fog alone and no light casts a ray: the shaded fused frame)
      rc = volume_frame_fused(T, volumes, minv, n_inst, cam, queues, fb, depth, features, S);
    else
      rc = volume_frame_fused(T, volumes, minv, n_inst, cam, queues, fb, depth, features, S, &H, sh, fog_ran, with_mesh, nullptr, with_ao);
    if (!rc && mesh_ran) *mesh_ran = with_mesh;
    if (!rc && ao_ran) *ao_ran = with_ao;
  }
  if (rc) return rc;
  O = gvt_hip_volume_shadow_stats{};
  O.fused = S.fused; O.features = S.features; O.samples_marched = S.samples_marched; O.samples_gathered = S.samples_gathered; O.brick_visits = S.brick_visits;
  O.rays_deposited = S.rays_deposited; O.adapter_calls = S.adapter_calls; O.crossings_rendered = S.crossings_rendered; O.samples_shaded = S.samples_shaded;
  O.shadowed = inert ? 0u : 1u;
  O.shadow_rays = sh[0]; O.shadow_brick_visits = sh[1]; O.shadow_crossings = sh[2]; O.shadow_samples_marched = sh[3]; O.shadow_samples_gathered = sh[4];
  fog_samples = fog_ran ? S.samples_shaded : 0;
  return 0;
}

} // namespace

extern "C" int gvt_hip_volume_frame_shadowed(gvt_hip_top *T, gvt_hip_volume *const *volumes, const float *m, const float *minv, size_t n_inst,
                                             const gvt_hip_camera *cam, gvt_hip_queue *const *queues, gvt_hip_fb *fb, const gvt_hip_depth *depth,
                                             const gvt_hip_volume_shadow_params *params, gvt_hip_volume_shadow_stats *stats) {
  gvt_hip_volume_shadow_stats O{};
  uint64_t fog_samples = 0;
  const int rc = volume_frame_shadowed_impl("volume_frame_shadowed", false, T, volumes, m, minv, n_inst, cam, queues, fb, depth, params, O, fog_samples);
  if (!rc && stats) *stats = O;
  return rc;
}

extern "C" int gvt_hip_volume_frame_fog_shadowed(gvt_hip_top *T, gvt_hip_volume *const *volumes, const float *m, const float *minv, size_t n_inst,
                                                 const gvt_hip_camera *cam, gvt_hip_queue *const *queues, gvt_hip_fb *fb, const gvt_hip_depth *depth,
                                                 const gvt_hip_volume_shadow_params *params, gvt_hip_volume_fog_shadow_stats *stats) {
  gvt_hip_volume_shadow_stats O{};
  uint64_t fog_samples = 0;
  const int rc = volume_frame_shadowed_impl("volume_frame_fog_shadowed", true, T, volumes, m, minv, n_inst, cam, queues, fb, depth, params, O, fog_samples);
  if (!rc && stats) {
    gvt_hip_volume_fog_shadow_stats F{};
    F.frame = O;
    F.fog_samples_shadowed = fog_samples;
    *stats = F;
  }
  return rc;
}

namespace {

// What one bake owns until it commits: the bricks' fresh planes (P: float for the light grids, uint8_t for the occluder grids) and the two
// events around its launches.  The destructor destroys the events and frees every plane that was not committed, so each failure path
// is a return; a path with work in flight drains the stream first (fail does).  fn: the entry point's name in the error texts
template <typename P>
struct BakeScope {
  const char *fn;
  hipStream_t stream;
  std::vector<P *> fresh;
  uint64_t bytes = 0;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  BakeScope(const char *fn_, hipStream_t st, size_t n_inst) : fn(fn_), stream(st), fresh(n_inst, nullptr) {}
  BakeScope(const BakeScope &) = delete;
  ~BakeScope() {
    if (e0) hipEventDestroy(e0);
    if (e1) hipEventDestroy(e1);
    for (P *p : fresh) hipFree(p);
  }
  // the new planes, all before any brick changes: n_usable planes of each brick's vertices
  int allocate(gvt_hip_volume *const *volumes, unsigned n_usable) {
    for (size_t i = 0; i < fresh.size(); i++) {
      const size_t nb = sizeof(P) * (size_t)volumes[i]->n[0] * volumes[i]->n[1] * volumes[i]->n[2] * n_usable;
      if (hipMalloc((void **)&fresh[i], nb) != hipSuccess) {
        (void)hipGetLastError();
        set_error("%s: no device memory for the planes of brick %zu (%zu bytes); the old grids are kept", fn, i, nb);
        return GVT_HIP_ERR_CAPACITY;
      }
      bytes += nb;
    }
    return 0;
  }
  int fail(const char *what) {
    set_error("%s: %s failed: %s; the old grids are kept", fn, what, hipGetErrorString(hipGetLastError()));
    hipStreamSynchronize(stream);
    return GVT_HIP_ERR_DEVICE;
  }
  P *commit(size_t i) { // (the brick owns the planes from here)
    P *p = fresh[i];
    fresh[i] = nullptr;
    return p;
  }
};

// What both bakes (the light grids' and the occluder grids') ask of their arguments and of their bricks.  fn: the entry point's name in the
// error texts.  bake_args: no null pointer, 1 to VOL_DEST_MAX bricks that have a table, flags of GVT_HIP_VOLUME_ALLOW_CENTRAL and
// GVT_HIP_VOLUME_ALLOW_AMR only
int bake_args(const char *fn, gvt_hip_volume *const *volumes, const float *m, const float *minv, size_t n_inst, const uint32_t *flags) {
  if (!volumes || !m || !minv || !flags) { set_error("%s: null argument", fn); return GVT_HIP_ERR_INVALID; }
  if (n_inst < 1 || n_inst > VOL_DEST_MAX) { set_error("%s: %zu bricks, 1 to %d are allowed", fn, n_inst, VOL_DEST_MAX); return GVT_HIP_ERR_INVALID; }
  for (size_t i = 0; i < n_inst; i++)
    if (!volumes[i] || !volumes[i]->has_tf) { set_error("%s: brick %zu is null or has no transfer function", fn, i); return GVT_HIP_ERR_INVALID; }
  if (*flags & ~(uint32_t)(GVT_HIP_VOLUME_ALLOW_CENTRAL | GVT_HIP_VOLUME_ALLOW_AMR)) { set_error("%s: unknown flag bits %u", fn, *flags); return GVT_HIP_ERR_INVALID; }
  return 0;
}

// ... bake_bricks: bricks of one grid that tile it, under one matrix, with equal surfaces and lights, at least one usable light, no
// subgrids unless the flags have GVT_HIP_VOLUME_ALLOW_AMR (amr: does a brick have any?), the CENTRAL clause (flags: the params' word -- with
// GVT_HIP_VOLUME_ALLOW_CENTRAL bricks that are all CENTRAL pass; the bake's
// rays march with shading NONE and read no gradient, so the planes do not depend on the kind), at most 2^32 - 1 (vertex, light) pairs.
// verts: the vertices summed over the bricks; usable: the lights' bits.  lights = false (the AO bake, which needs no light and compares
// none): without the two light clauses, usable = 0
int bake_bricks(const char *fn, gvt_hip_volume *const *volumes, const float *m, const float *minv, size_t n_inst, uint32_t flags, uint64_t &verts, unsigned &usable,
                bool *amr = nullptr, bool lights = true) {
  uint32_t features = 0;
  const char *why = "";
  const bool allow_central = (flags & GVT_HIP_VOLUME_ALLOW_CENTRAL) != 0;
  const uint32_t allow = GVT_HIP_FUSED_SURFACES | GVT_HIP_FUSED_LIT | (allow_central ? GVT_HIP_FUSED_CENTRAL : 0u) | ((flags & GVT_HIP_VOLUME_ALLOW_AMR) ? GVT_HIP_FUSED_AMR : 0u);
  const bool eligible = fused_eligible(volumes, minv, n_inst, allow, features, &why);
  if (amr) *amr = (features & GVT_HIP_FUSED_AMR) != 0;
  if (!eligible) {
    set_error("%s: the bricks are not eligible for the fused kernels: %s", fn, why);
    return GVT_HIP_ERR_INVALID;
  }
  const gvt_hip_volume *A = volumes[0];
  uint64_t cells = 0;
  verts = 0;
  for (size_t i = 0; i < n_inst; i++) {
    const gvt_hip_volume *B = volumes[i];
    if (!same_bits(m + 16 * i, m, 16 * sizeof(float))) { set_error("%s: bricks under different matrices", fn); return GVT_HIP_ERR_INVALID; }
    if (!same_bits(B->gn, A->gn, sizeof(A->gn))) { set_error("%s: bricks of different grids (global counts)", fn); return GVT_HIP_ERR_INVALID; }
    if (B->grad == GVT_HIP_VOLUME_GRADIENT_CENTRAL && B->n_iso > 0 && !allow_central) { set_error("%s: central gradients on a brick of a frame with an isovalue", fn); return GVT_HIP_ERR_INVALID; }
    // (fused_eligible compares surfaces and lights only where the frame renders them: the bake needs them equal whatever the shading)
    if (B->n_iso != A->n_iso || B->n_pl != A->n_pl || !same_bits(&B->surf_alpha, &A->surf_alpha, sizeof(float)) || !same_bits(B->iso, A->iso, sizeof(float) * (size_t)A->n_iso) ||
        !same_bits(B->plane, A->plane, sizeof(A->plane[0]) * (size_t)A->n_pl)) { set_error("%s: bricks with different surfaces", fn); return GVT_HIP_ERR_INVALID; }
    if (lights && (B->n_lights != A->n_lights || !same_bits(B->lpos, A->lpos, sizeof(A->lpos[0]) * (size_t)A->n_lights))) { set_error("%s: bricks with different lights", fn); return GVT_HIP_ERR_INVALID; }
    cells += (uint64_t)(B->n[0] - 1) * (uint64_t)(B->n[1] - 1) * (uint64_t)(B->n[2] - 1);
    verts += (uint64_t)B->n[0] * (uint64_t)B->n[1] * (uint64_t)B->n[2];
    for (size_t k = 0; k < i; k++) { // owned cells [off, off + n - 1) per axis: disjoint
      const gvt_hip_volume *K = volumes[k];
      bool apart = false;
      for (int a = 0; a < 3; a++) apart = apart || B->off[a] + B->n[a] - 1 <= K->off[a] || K->off[a] + K->n[a] - 1 <= B->off[a];
      if (!apart) { set_error("%s: the bricks do not tile the grid: bricks %zu and %zu share a cell", fn, k, i); return GVT_HIP_ERR_INVALID; }
    }
  }
  if (cells != (uint64_t)(A->gn[0] - 1) * (uint64_t)(A->gn[1] - 1) * (uint64_t)(A->gn[2] - 1)) {
    set_error("%s: the bricks do not tile the grid: they own %llu of its %llu cells", fn, (unsigned long long)cells,
              (unsigned long long)((uint64_t)(A->gn[0] - 1) * (uint64_t)(A->gn[1] - 1) * (uint64_t)(A->gn[2] - 1)));
    return GVT_HIP_ERR_INVALID;
  }
  usable = 0;
  if (!lights) return 0;
  usable = shadow_dev(A, 1).usable;
  const unsigned n_usable = (unsigned)__builtin_popcount(usable);
  if (!n_usable) { set_error("%s: no usable light (none set, or every position is zero)", fn); return GVT_HIP_ERR_INVALID; }
  if (verts * n_usable > 0xffffffffull) { set_error("%s: %llu (vertex, light) pairs, at most 2^32 - 1", fn, (unsigned long long)(verts * n_usable)); return GVT_HIP_ERR_INVALID; }
  return 0;
}

} // namespace

extern "C" int gvt_hip_volume_light_grid_bake(gvt_hip_volume *const *volumes, const float *m, const float *minv, size_t n_inst,
                                              const gvt_hip_volume_light_grid_params *params, gvt_hip_volume_light_grid_stats *stats) {
  if (ensure_init()) return GVT_HIP_ERR_NODEVICE;
  int rc;
  if ((rc = bake_args("volume_light_grid_bake", volumes, m, minv, n_inst, params ? &params->flags : nullptr))) return rc;
  if (params->bias < 1 || params->bias > 64) { set_error("volume_light_grid_bake: bias %d, 1 to 64 lattice steps are allowed", params->bias); return GVT_HIP_ERR_INVALID; }
  uint64_t verts = 0;
  unsigned usable = 0;
  bool amr = false; // a brick has subgrids (GVT_HIP_VOLUME_ALLOW_AMR): k_volume_bake_light_amr, and the bricks' AMR tables beside the records
  if ((rc = bake_bricks("volume_light_grid_bake", volumes, m, minv, n_inst, params->flags, verts, usable, &amr))) return rc;
  const gvt_hip_volume *A = volumes[0];
  const ShadowDev H = shadow_dev(A, params->bias);
  const unsigned n_usable = (unsigned)__builtin_popcount(H.usable);
  Ctx &C = gctx();
  BakeScope<float> own("volume_light_grid_bake", C.stream, n_inst);
  if ((rc = own.allocate(volumes, n_usable))) return rc;
  FusedBrick *d_bricks = (FusedBrick *)scratch_get(SCR_VOL_BRICKS, sizeof(FusedBrick) * n_inst);
  LightGridBrick *d_parts = (LightGridBrick *)scratch_get(SCR_VOL_GRIDS, sizeof(LightGridBrick) * n_inst);
  AmrDev *d_amr = amr ? (AmrDev *)scratch_get(SCR_VOL_AMR, sizeof(AmrDev) * n_inst) : nullptr;
  unsigned long long *d_stats = (unsigned long long *)scratch_get(SCR_VOL_FUSED, VOL_FUSED_SHADOW_STATS * sizeof(unsigned long long));
  unsigned *work = (unsigned *)scratch_get(SCR_VOL_WORK, sizeof(unsigned));
  if (!d_bricks || !d_parts || !d_stats || !work || (amr && !d_amr)) return own.fail("a scratch allocation");
  static_assert(VOL_BAKE_STATS <= VOL_FUSED_SHADOW_STATS, "the fused frames' counter words serve the bake");
  static_assert((sizeof(FusedBrick) + sizeof(LightGridBrick) + sizeof(AmrDev)) * VOL_DEST_MAX <= PINNED_STAGE_BYTES, "the three tables fit the staging block");
  void *stage = nullptr;
  if (pinned_stage_begin(&stage)) return own.fail("the staging block");
  FusedBrick *h = (FusedBrick *)stage;
  LightGridBrick *hp = (LightGridBrick *)(h + VOL_DEST_MAX);
  AmrDev *ha = (AmrDev *)(hp + VOL_DEST_MAX);
  unsigned first = 0;
  for (size_t i = 0; i < n_inst; i++) {
    const gvt_hip_volume *B = volumes[i];
    h[i] = fused_record(B, true);
    hp[i] = LightGridBrick{ own.fresh[i], first, 0u };
    if (amr) ha[i] = amr_record(B);
    first += (unsigned)((size_t)B->n[0] * B->n[1] * B->n[2]) * n_usable;
  }
  const unsigned n = first;
  bool ok = hipMemcpyAsync(d_bricks, h, sizeof(FusedBrick) * n_inst, hipMemcpyHostToDevice, C.stream) == hipSuccess &&
            hipMemcpyAsync(d_parts, hp, sizeof(LightGridBrick) * n_inst, hipMemcpyHostToDevice, C.stream) == hipSuccess &&
            (!amr || hipMemcpyAsync(d_amr, ha, sizeof(AmrDev) * n_inst, hipMemcpyHostToDevice, C.stream) == hipSuccess);
  if (pinned_stage_end() || !ok) return own.fail("the table upload");
  ok = hipMemsetAsync(work, 0, sizeof(unsigned), C.stream) == hipSuccess && hipMemsetAsync(d_stats, 0, VOL_BAKE_STATS * sizeof(unsigned long long), C.stream) == hipSuccess &&
       hipEventCreate(&own.e0) == hipSuccess && hipEventCreate(&own.e1) == hipSuccess;
  if (!ok) return own.fail("the launch's preparation");
  Mat4 M, Mi;
  for (int k = 0; k < 16; k++) { M.m[k] = m[k]; Mi.m[k] = minv[k]; }
  // the whole grid as one brick: offset 0, counts = the global counts, the global vertex box (gvt_hip_volume_create's expressions)
  VolDev U = vol_dev(A);
  U.vox = nullptr; U.mc = nullptr;
  U.nx = A->gn[0]; U.ny = A->gn[1]; U.nz = A->gn[2]; U.ox = 0; U.oy = 0; U.oz = 0;
  U.nbx = (A->gn[0] - 1 + 7) / 8; U.nby = (A->gn[1] - 1 + 7) / 8;
  for (int a = 0; a < 3; a++) { U.lo[a] = A->go[a] + (float)0 * A->sp[a]; U.hi[a] = A->go[a] + (float)(A->gn[a] - 1) * A->sp[a]; }
  const unsigned blocks = std::min(blocks_of(n), (unsigned)(std::max(C.n_cu, 1) * 8));
  ok = hipEventRecord(own.e0, C.stream) == hipSuccess;
  if (ok && amr) // (F32: a brick with subgrids is, and fused_eligible has compared the voxel types)
    k_volume_bake_light_amr<<<blocks, VOL_BLOCK, 0, C.stream>>>(U, surf_dev(A, Mi), H, d_bricks, (const AmrDev *)d_amr, d_parts, (unsigned)n_inst, n, M, Mi, work, d_stats);
  else if (ok)
    with_voxel_type(A->vtype, [&](auto t) {
      using VT = decltype(t);
      k_volume_bake_light<VT><<<blocks, VOL_BLOCK, 0, C.stream>>>(U, surf_dev(A, Mi), H, d_bricks, d_parts, (unsigned)n_inst, n, M, Mi, work, d_stats);
    });
  unsigned long long h_stats[VOL_BAKE_STATS] = {};
  float ms = 0.f;
  ok = ok && hipGetLastError() == hipSuccess && hipEventRecord(own.e1, C.stream) == hipSuccess &&
       hipMemcpyAsync(h_stats, d_stats, sizeof(h_stats), hipMemcpyDeviceToHost, C.stream) == hipSuccess && hipStreamSynchronize(C.stream) == hipSuccess &&
       hipEventElapsedTime(&ms, own.e0, own.e1) == hipSuccess;
  if (!ok) return own.fail("the bake kernel");
  // commit: every brick at once
  static uint64_t bake_serial = 0;
  bake_serial++;
  for (size_t i = 0; i < n_inst; i++) {
    gvt_hip_volume *B = volumes[i];
    hipFree(B->d_lgrid);
    B->d_lgrid = own.commit(i);
    B->lg_bias = params->bias;
    grids_commit(B->lg, H.usable, bake_serial, i, n_inst, m, minv);
  }
  if (stats) {
    gvt_hip_volume_light_grid_stats O{};
    O.rays = n; O.samples_marched = h_stats[0]; O.samples_gathered = h_stats[1]; O.crossings = h_stats[2]; O.bytes = own.bytes; O.ms = ms;
    *stats = O;
  }
  return 0;
}

extern "C" int gvt_hip_volume_light_grid_download(gvt_hip_volume *V, int light, float *out) {
  if (ensure_init()) return GVT_HIP_ERR_NODEVICE;
  if (!V || !out) { set_error("volume_light_grid_download: null argument"); return GVT_HIP_ERR_INVALID; }
  if (!V->d_lgrid) { set_error("volume_light_grid_download: the volume holds no light grid"); return GVT_HIP_ERR_INVALID; }
  if (light < 0 || light >= GVT_HIP_VOLUME_MAX_LIGHTS || !((V->lg.usable >> light) & 1u)) {
    set_error("volume_light_grid_download: light %d was not usable at the bake and has no grid (its transmittance is 1)", light);
    return GVT_HIP_ERR_INVALID;
  }
  const size_t n_vert = (size_t)V->n[0] * V->n[1] * V->n[2];
  const int plane = __builtin_popcount(V->lg.usable & ((1u << light) - 1u));
  HIPCHK(hipStreamSynchronize(gctx().stream));
  HIPCHK(hipMemcpy(out, V->d_lgrid + n_vert * (size_t)plane, sizeof(float) * n_vert, hipMemcpyDeviceToHost));
  return 0;
}

extern "C" int gvt_hip_volume_light_grid_info(gvt_hip_volume *V, gvt_hip_volume_light_grid_state *out) {
  if (!V || !out) { set_error("volume_light_grid_info: null argument"); return GVT_HIP_ERR_INVALID; }
  gvt_hip_volume_light_grid_state I{};
  I.present = V->d_lgrid ? 1u : 0u;
  I.current = (V->d_lgrid && V->lg.current) ? 1u : 0u;
  I.n_planes = V->d_lgrid ? V->lg.planes : 0;
  I.bias = V->d_lgrid ? V->lg_bias : 0;
  I.bytes = V->d_lgrid ? sizeof(float) * (uint64_t)V->n[0] * V->n[1] * V->n[2] * (uint64_t)V->lg.planes : 0;
  *out = I;
  return 0;
}

extern "C" int gvt_hip_volume_light_grid_release(gvt_hip_volume *V) {
  if (ensure_init()) return GVT_HIP_ERR_NODEVICE;
  if (!V) { set_error("volume_light_grid_release: null"); return GVT_HIP_ERR_INVALID; }
  if (!V->d_lgrid) return 0;
  HIPCHK(hipStreamSynchronize(gctx().stream)); // (a frame in flight reads the planes)
  hipFree(V->d_lgrid);
  V->d_lgrid = nullptr;
  grids_reset(V->lg);
  V->lg_bias = 0;
  return 0;
}

// ---- meshes shadowing the volume (the contract: include/gvt_hip.h, "meshes shadowing the volume"; volume_occluder_grid.inc,
// volume_fused_mesh.inc)
extern "C" int gvt_hip_volume_frame_mesh_shadowed(gvt_hip_top *T, gvt_hip_volume *const *volumes, const float *m, const float *minv, size_t n_inst,
                                                  const gvt_hip_camera *cam, gvt_hip_queue *const *queues, gvt_hip_fb *fb, const gvt_hip_depth *depth,
                                                  const gvt_hip_volume_shadow_params *params, gvt_hip_volume_mesh_shadow_stats *stats) {
  gvt_hip_volume_shadow_stats O{};
  uint64_t fog_samples = 0;
  bool mesh_ran = false;
  const int rc = volume_frame_shadowed_impl("volume_frame_mesh_shadowed", true, T, volumes, m, minv, n_inst, cam, queues, fb, depth, params, O, fog_samples, true, &mesh_ran);
  if (!rc && stats) {
    gvt_hip_volume_mesh_shadow_stats F{};
    F.fog.frame = O;
    F.fog.fog_samples_shadowed = fog_samples;
    F.mesh_shadowed = mesh_ran ? 1u : 0u;
    *stats = F;
  }
  return rc;
}

// Scratch of one bake, each slot in one use along the chain: SCR_VOL_GRIDS the per-brick table, SCR_VOL_OCC_RAYS a chunk's p0 / p1 planes,
// SCR_VOL_OCC its O words, SCR_GENERAL its any-hit flags (as gvt_hip_occluded), SCR_VOL_FUSED the counter word
extern "C" int gvt_hip_volume_occluder_grid_bake(gvt_hip_volume *const *volumes, const float *m, const float *minv, size_t n_inst, gvt_hip_mesh *const *meshes,
                                                 const float *mesh_minv, size_t n_mesh_inst, const gvt_hip_volume_occluder_params *params,
                                                 gvt_hip_volume_occluder_stats *stats) {
  if (ensure_init()) return GVT_HIP_ERR_NODEVICE;
  int rc;
  if ((rc = bake_args("volume_occluder_grid_bake", volumes, m, minv, n_inst, params ? &params->flags : nullptr))) return rc;
  if (n_mesh_inst && (!meshes || !mesh_minv)) { set_error("volume_occluder_grid_bake: null argument (the mesh instances)"); return GVT_HIP_ERR_INVALID; }
  for (size_t i = 0; i < n_mesh_inst; i++)
    if (!meshes[i]) { set_error("volume_occluder_grid_bake: mesh instance %zu has no mesh", i); return GVT_HIP_ERR_INVALID; }
  uint64_t verts = 0;
  unsigned usable = 0;
  if ((rc = bake_bricks("volume_occluder_grid_bake", volumes, m, minv, n_inst, params->flags, verts, usable))) return rc;
  const gvt_hip_volume *A = volumes[0];
  const ShadowDev H = shadow_dev(A, 1); // (the directions and their bits; the bias is the light grid's business)
  const unsigned n_usable = (unsigned)__builtin_popcount(H.usable);
  Ctx &C = gctx();
  BakeScope<uint8_t> own("volume_occluder_grid_bake", C.stream, n_inst);
  if ((rc = own.allocate(volumes, n_usable))) return rc;
  const unsigned n = (unsigned)(verts * n_usable);
  const unsigned chunk = std::min(n, C.occluder_chunk > 0 ? (unsigned)C.occluder_chunk : VOL_OCC_CHUNK);
  OccluderBrick *d_parts = (OccluderBrick *)scratch_get(SCR_VOL_GRIDS, sizeof(OccluderBrick) * n_inst);
  float4 *d_rays = (float4 *)scratch_get(SCR_VOL_OCC_RAYS, sizeof(float4) * 2 * (size_t)chunk);
  uint8_t *d_O = (uint8_t *)scratch_get(SCR_VOL_OCC, chunk);
  int *d_flags = n_mesh_inst ? (int *)scratch_get(SCR_GENERAL, sizeof(int) * (size_t)chunk) : nullptr;
  unsigned long long *d_blocked = (unsigned long long *)scratch_get(SCR_VOL_FUSED, VOL_FUSED_SHADOW_STATS * sizeof(unsigned long long));
  if (!d_parts || !d_rays || !d_O || (n_mesh_inst && !d_flags) || !d_blocked) return own.fail("a scratch allocation");
  static_assert(sizeof(OccluderBrick) * VOL_DEST_MAX <= PINNED_STAGE_BYTES, "the table fits the staging block");
  void *stage = nullptr;
  if (pinned_stage_begin(&stage)) return own.fail("the staging block");
  OccluderBrick *hp = (OccluderBrick *)stage;
  unsigned first = 0;
  for (size_t i = 0; i < n_inst; i++) {
    const gvt_hip_volume *B = volumes[i];
    hp[i] = OccluderBrick{ own.fresh[i], first, B->n[0], B->n[1], B->n[2], B->off[0], B->off[1], B->off[2] };
    first += (unsigned)((size_t)B->n[0] * B->n[1] * B->n[2]) * n_usable;
  }
  bool ok = hipMemcpyAsync(d_parts, hp, sizeof(OccluderBrick) * n_inst, hipMemcpyHostToDevice, C.stream) == hipSuccess;
  if (pinned_stage_end() || !ok) return own.fail("the table upload");
  ok = hipMemsetAsync(d_blocked, 0, sizeof(unsigned long long), C.stream) == hipSuccess && hipEventCreate(&own.e0) == hipSuccess && hipEventCreate(&own.e1) == hipSuccess &&
       hipEventRecord(own.e0, C.stream) == hipSuccess;
  if (!ok) return own.fail("the launches' preparation");
  Mat4 M;
  for (int k = 0; k < 16; k++) M.m[k] = m[k];
  RayPlanes P{};
  P.p0 = d_rays; P.p1 = d_rays + chunk;
  uint64_t launches = 0;
  for (unsigned base = 0; base < n; base += chunk) {
    const unsigned nc = std::min(chunk, n - base);
    if (hipMemsetAsync(d_O, 1, nc, C.stream) != hipSuccess) return own.fail("the chunk's clear");
    if (n_mesh_inst) {
      k_occluder_rays<<<blocks_of(nc), VOL_BLOCK, 0, C.stream>>>(A->go[0], A->go[1], A->go[2], A->sp[0], A->sp[1], A->sp[2], H, d_parts, (unsigned)n_inst, base, nc, M, P.p0, P.p1);
      if (hipGetLastError() != hipSuccess) return own.fail("the ray kernel");
    }
    for (size_t i = 0; i < n_mesh_inst; i++) {
      Mat4 Mi;
      for (int k = 0; k < 16; k++) Mi.m[k] = mesh_minv[16 * i + k];
      if ((rc = launch_any_flags(meshes[i], P, nc, true, Mi, GVT_RAY_EPSILON, d_flags))) { // (its own message stands)
        hipStreamSynchronize(C.stream);
        return rc;
      }
      launches++;
      k_occluder_fold<<<blocks_of(nc), VOL_BLOCK, 0, C.stream>>>(d_flags, nc, d_O);
      if (hipGetLastError() != hipSuccess) return own.fail("the fold kernel");
    }
    k_occluder_pack<<<blocks_of(nc), VOL_BLOCK, 0, C.stream>>>(d_O, d_parts, (unsigned)n_inst, base, nc, d_blocked);
    if (hipGetLastError() != hipSuccess) return own.fail("the pack kernel");
  }
  unsigned long long h_blocked = 0;
  float ms = 0.f;
  ok = hipEventRecord(own.e1, C.stream) == hipSuccess && hipMemcpyAsync(&h_blocked, d_blocked, sizeof(h_blocked), hipMemcpyDeviceToHost, C.stream) == hipSuccess &&
       (!n_mesh_inst || trav_overflow_fetch_async() == 0) && hipStreamSynchronize(C.stream) == hipSuccess && hipEventElapsedTime(&ms, own.e0, own.e1) == hipSuccess;
  if (!ok) return own.fail("the bake's last wait");
  if (n_mesh_inst && (rc = trav_overflow_result())) return rc; // (GVT_HIP_ERR_DEVICE: the flags are incomplete; the old grids are kept)
  // commit: every brick at once
  static uint64_t bake_serial = 0;
  bake_serial++;
  for (size_t i = 0; i < n_inst; i++) {
    gvt_hip_volume *B = volumes[i];
    hipFree(B->d_occ);
    B->d_occ = own.commit(i);
    grids_commit(B->og, H.usable, bake_serial, i, n_inst, m, minv);
  }
  if (stats) {
    gvt_hip_volume_occluder_stats O{};
    O.rays = n; O.rays_blocked = h_blocked; O.any_hit_launches = launches; O.bytes = own.bytes; O.ms = ms;
    *stats = O;
  }
  return 0;
}

extern "C" int gvt_hip_volume_occluder_grid_download(gvt_hip_volume *V, int light, uint8_t *out) {
  if (ensure_init()) return GVT_HIP_ERR_NODEVICE;
  if (!V || !out) { set_error("volume_occluder_grid_download: null argument"); return GVT_HIP_ERR_INVALID; }
  if (!V->d_occ) { set_error("volume_occluder_grid_download: the volume holds no occluder grid"); return GVT_HIP_ERR_INVALID; }
  if (light < 0 || light >= GVT_HIP_VOLUME_MAX_LIGHTS || !((V->og.usable >> light) & 1u)) {
    set_error("volume_occluder_grid_download: light %d was not usable at the bake and has no grid (its factor is 1)", light);
    return GVT_HIP_ERR_INVALID;
  }
  const size_t n_vert = (size_t)V->n[0] * V->n[1] * V->n[2];
  const int plane = __builtin_popcount(V->og.usable & ((1u << light) - 1u));
  HIPCHK(hipStreamSynchronize(gctx().stream));
  HIPCHK(hipMemcpy(out, V->d_occ + n_vert * (size_t)plane, n_vert, hipMemcpyDeviceToHost));
  return 0;
}

extern "C" int gvt_hip_volume_occluder_grid_info(gvt_hip_volume *V, gvt_hip_volume_occluder_state *out) {
  if (!V || !out) { set_error("volume_occluder_grid_info: null argument"); return GVT_HIP_ERR_INVALID; }
  gvt_hip_volume_occluder_state I{};
  I.present = V->d_occ ? 1u : 0u;
  I.current = (V->d_occ && V->og.current) ? 1u : 0u;
  I.n_planes = V->d_occ ? V->og.planes : 0;
  I.bytes = V->d_occ ? (uint64_t)V->n[0] * V->n[1] * V->n[2] * (uint64_t)V->og.planes : 0;
  *out = I;
  return 0;
}

extern "C" int gvt_hip_volume_occluder_grid_release(gvt_hip_volume *V) {
  if (ensure_init()) return GVT_HIP_ERR_NODEVICE;
  if (!V) { set_error("volume_occluder_grid_release: null"); return GVT_HIP_ERR_INVALID; }
  if (!V->d_occ) return 0;
  HIPCHK(hipStreamSynchronize(gctx().stream)); // (a frame in flight reads the planes)
  hipFree(V->d_occ);
  V->d_occ = nullptr;
  grids_reset(V->og);
  return 0;
}

// ---- ambient occlusion (the contract: include/gvt_hip.h, "ambient occlusion"; volume_ao_grid.inc, volume_fused_ao.inc)
extern "C" int gvt_hip_volume_ao_grid_bake(gvt_hip_volume *const *volumes, const float *m, const float *minv, size_t n_inst, const gvt_hip_volume_ao_params *params,
                                           gvt_hip_volume_ao_stats *stats) {
  if (ensure_init()) return GVT_HIP_ERR_NODEVICE;
  int rc;
  if ((rc = bake_args("volume_ao_grid_bake", volumes, m, minv, n_inst, params ? &params->flags : nullptr))) return rc;
  if (params->flags & GVT_HIP_VOLUME_ALLOW_AMR) { set_error("volume_ao_grid_bake: GVT_HIP_VOLUME_ALLOW_AMR is not accepted: an AO grid never covers subgrids"); return GVT_HIP_ERR_INVALID; }
  if (params->bias < 1 || params->bias > 64) { set_error("volume_ao_grid_bake: bias %d, 1 to 64 lattice steps are allowed", params->bias); return GVT_HIP_ERR_INVALID; }
  if (params->n_dirs < 1 || params->n_dirs > GVT_HIP_VOLUME_AO_MAX_DIRS) {
    set_error("volume_ao_grid_bake: n_dirs %d, 1 to %d directions are allowed", params->n_dirs, GVT_HIP_VOLUME_AO_MAX_DIRS);
    return GVT_HIP_ERR_INVALID;
  }
  if (!(params->radius > 0.f)) { set_error("volume_ao_grid_bake: radius %g, it must be positive (+Inf: no clip)", (double)params->radius); return GVT_HIP_ERR_INVALID; }
  float h_dirs[GVT_HIP_VOLUME_AO_MAX_DIRS][3] = {};
  for (int i = 0; i < params->n_dirs; i++) { // (normalised as shadow_dev normalises the lights)
    const float x = params->dirs[i][0], y = params->dirs[i][1], z = params->dirs[i][2];
    const float len = sqrtf((x * x + y * y) + z * z);
    if (!(len > 0.f && std::isfinite(len))) { set_error("volume_ao_grid_bake: direction %d is zero or not finite", i); return GVT_HIP_ERR_INVALID; }
    h_dirs[i][0] = x / len; h_dirs[i][1] = y / len; h_dirs[i][2] = z / len;
  }
  uint64_t verts = 0;
  unsigned usable = 0;
  if ((rc = bake_bricks("volume_ao_grid_bake", volumes, m, minv, n_inst, params->flags, verts, usable, nullptr, false))) return rc;
  if (verts * (uint64_t)params->n_dirs > 0xffffffffull) {
    set_error("volume_ao_grid_bake: %llu (vertex, direction) pairs, at most 2^32 - 1", (unsigned long long)(verts * (uint64_t)params->n_dirs));
    return GVT_HIP_ERR_INVALID;
  }
  const gvt_hip_volume *A = volumes[0];
  Ctx &C = gctx();
  BakeScope<float> own("volume_ao_grid_bake", C.stream, n_inst);
  if ((rc = own.allocate(volumes, 1u))) return rc;
  // SCR_VOL_GRIDS: the per-brick table (VOL_DEST_MAX records), then the directions
  const size_t table_bytes = sizeof(LightGridBrick) * VOL_DEST_MAX;
  FusedBrick *d_bricks = (FusedBrick *)scratch_get(SCR_VOL_BRICKS, sizeof(FusedBrick) * n_inst);
  char *d_table = (char *)scratch_get(SCR_VOL_GRIDS, table_bytes + sizeof(h_dirs));
  unsigned long long *d_stats = (unsigned long long *)scratch_get(SCR_VOL_FUSED, VOL_FUSED_SHADOW_STATS * sizeof(unsigned long long));
  unsigned *work = (unsigned *)scratch_get(SCR_VOL_WORK, sizeof(unsigned));
  if (!d_bricks || !d_table || !d_stats || !work) return own.fail("a scratch allocation");
  LightGridBrick *d_parts = (LightGridBrick *)d_table;
  float *d_dirs = (float *)(d_table + table_bytes);
  static_assert((sizeof(FusedBrick) + sizeof(LightGridBrick)) * VOL_DEST_MAX + sizeof(h_dirs) <= PINNED_STAGE_BYTES, "the two tables and the directions fit the staging block");
  void *stage = nullptr;
  if (pinned_stage_begin(&stage)) return own.fail("the staging block");
  FusedBrick *h = (FusedBrick *)stage;
  LightGridBrick *hp = (LightGridBrick *)(h + VOL_DEST_MAX);
  std::memcpy(hp + VOL_DEST_MAX, h_dirs, sizeof(h_dirs));
  unsigned first = 0;
  for (size_t i = 0; i < n_inst; i++) {
    const gvt_hip_volume *B = volumes[i];
    h[i] = fused_record(B, true);
    hp[i] = LightGridBrick{ own.fresh[i], first, 0u };
    first += (unsigned)((size_t)B->n[0] * B->n[1] * B->n[2]);
  }
  const unsigned n = first; // (one work item a vertex)
  bool ok = hipMemcpyAsync(d_bricks, h, sizeof(FusedBrick) * n_inst, hipMemcpyHostToDevice, C.stream) == hipSuccess &&
            hipMemcpyAsync(d_table, hp, table_bytes + sizeof(h_dirs), hipMemcpyHostToDevice, C.stream) == hipSuccess;
  if (pinned_stage_end() || !ok) return own.fail("the table upload");
  ok = hipMemsetAsync(work, 0, sizeof(unsigned), C.stream) == hipSuccess && hipMemsetAsync(d_stats, 0, VOL_BAKE_STATS * sizeof(unsigned long long), C.stream) == hipSuccess &&
       hipEventCreate(&own.e0) == hipSuccess && hipEventCreate(&own.e1) == hipSuccess;
  if (!ok) return own.fail("the launch's preparation");
  Mat4 M, Mi;
  for (int k = 0; k < 16; k++) { M.m[k] = m[k]; Mi.m[k] = minv[k]; }
  // the whole grid as one brick, as the light bake states it
  VolDev U = vol_dev(A);
  U.vox = nullptr; U.mc = nullptr;
  U.nx = A->gn[0]; U.ny = A->gn[1]; U.nz = A->gn[2]; U.ox = 0; U.oy = 0; U.oz = 0;
  U.nbx = (A->gn[0] - 1 + 7) / 8; U.nby = (A->gn[1] - 1 + 7) / 8;
  for (int a = 0; a < 3; a++) { U.lo[a] = A->go[a] + (float)0 * A->sp[a]; U.hi[a] = A->go[a] + (float)(A->gn[a] - 1) * A->sp[a]; }
  const float t0 = (float)(params->bias - 1) * A->dt;
  const unsigned blocks = std::min(blocks_of(n), (unsigned)(std::max(C.n_cu, 1) * 8));
  ok = hipEventRecord(own.e0, C.stream) == hipSuccess;
  if (ok)
    with_voxel_type(A->vtype, [&](auto t) {
      using VT = decltype(t);
      k_volume_bake_ao<VT><<<blocks, VOL_BLOCK, 0, C.stream>>>(U, surf_dev(A, Mi), d_bricks, d_parts, (unsigned)n_inst, n, M, Mi, d_dirs, params->n_dirs, t0, params->radius, work,
                                                              d_stats);
    });
  unsigned long long h_stats[VOL_BAKE_STATS] = {};
  float ms = 0.f;
  ok = ok && hipGetLastError() == hipSuccess && hipEventRecord(own.e1, C.stream) == hipSuccess &&
       hipMemcpyAsync(h_stats, d_stats, sizeof(h_stats), hipMemcpyDeviceToHost, C.stream) == hipSuccess && hipStreamSynchronize(C.stream) == hipSuccess &&
       hipEventElapsedTime(&ms, own.e0, own.e1) == hipSuccess;
  if (!ok) return own.fail("the bake kernel");
  // commit: every brick at once
  static uint64_t bake_serial = 0;
  bake_serial++;
  for (size_t i = 0; i < n_inst; i++) {
    gvt_hip_volume *B = volumes[i];
    hipFree(B->d_ao);
    B->d_ao = own.commit(i);
    B->ag_dirs = params->n_dirs; B->ag_bias = params->bias; B->ag_radius = params->radius;
    grids_commit(B->ag, 1u, bake_serial, i, n_inst, m, minv);
  }
  if (stats) {
    gvt_hip_volume_ao_stats O{};
    O.rays = (uint64_t)n * (uint64_t)params->n_dirs; O.samples_marched = h_stats[0]; O.samples_gathered = h_stats[1]; O.crossings = h_stats[2]; O.bytes = own.bytes; O.ms = ms;
    *stats = O;
  }
  return 0;
}

extern "C" int gvt_hip_volume_ao_grid_download(gvt_hip_volume *V, float *out) {
  if (ensure_init()) return GVT_HIP_ERR_NODEVICE;
  if (!V || !out) { set_error("volume_ao_grid_download: null argument"); return GVT_HIP_ERR_INVALID; }
  if (!V->d_ao) { set_error("volume_ao_grid_download: the volume holds no ao grid"); return GVT_HIP_ERR_INVALID; }
  HIPCHK(hipStreamSynchronize(gctx().stream));
  HIPCHK(hipMemcpy(out, V->d_ao, sizeof(float) * (size_t)V->n[0] * V->n[1] * V->n[2], hipMemcpyDeviceToHost));
  return 0;
}

extern "C" int gvt_hip_volume_ao_grid_info(gvt_hip_volume *V, gvt_hip_volume_ao_state *out) {
  if (!V || !out) { set_error("volume_ao_grid_info: null argument"); return GVT_HIP_ERR_INVALID; }
  gvt_hip_volume_ao_state I{};
  I.present = V->d_ao ? 1u : 0u;
  I.current = (V->d_ao && V->ag.current) ? 1u : 0u;
  I.n_dirs = V->d_ao ? V->ag_dirs : 0;
  I.bias = V->d_ao ? V->ag_bias : 0;
  I.radius = V->d_ao ? V->ag_radius : 0.f;
  I.bytes = V->d_ao ? sizeof(float) * (uint64_t)V->n[0] * V->n[1] * V->n[2] : 0;
  *out = I;
  return 0;
}

extern "C" int gvt_hip_volume_ao_grid_release(gvt_hip_volume *V) {
  if (ensure_init()) return GVT_HIP_ERR_NODEVICE;
  if (!V) { set_error("volume_ao_grid_release: null"); return GVT_HIP_ERR_INVALID; }
  if (!V->d_ao) return 0;
  HIPCHK(hipStreamSynchronize(gctx().stream)); // (a frame in flight reads the plane)
  hipFree(V->d_ao);
  V->d_ao = nullptr;
  grids_reset(V->ag);
  V->ag_dirs = 0; V->ag_bias = 0; V->ag_radius = 0.f;
  return 0;
}

extern "C" int gvt_hip_volume_frame_ao(gvt_hip_top *T, gvt_hip_volume *const *volumes, const float *m, const float *minv, size_t n_inst, const gvt_hip_camera *cam,
                                       gvt_hip_queue *const *queues, gvt_hip_fb *fb, const gvt_hip_depth *depth, const gvt_hip_volume_ao_frame_params *params,
                                       gvt_hip_volume_ao_frame_stats *stats) {
  int rc;
  if ((rc = volume_frame_args(T, volumes, m, minv, n_inst, cam, queues, fb, depth))) return rc;
  if (!params) { set_error("volume_frame_ao: null params"); return GVT_HIP_ERR_INVALID; }
  if (params->flags & GVT_HIP_VOLUME_ALLOW_AMR) { set_error("volume_frame_ao: GVT_HIP_VOLUME_ALLOW_AMR is not accepted: an AO grid never covers subgrids"); return GVT_HIP_ERR_INVALID; }
  if (params->flags & ~(uint32_t)(GVT_HIP_VOLUME_ALLOW_CENTRAL | GVT_HIP_VOLUME_AO_MESH)) { set_error("volume_frame_ao: unknown flag bits %u", params->flags); return GVT_HIP_ERR_INVALID; }
  const bool mesh = (params->flags & GVT_HIP_VOLUME_AO_MESH) != 0;
  const gvt_hip_volume_shadow_params base{ params->flags & GVT_HIP_VOLUME_ALLOW_CENTRAL, params->bias };
  gvt_hip_volume_shadow_stats O{};
  uint64_t fog_samples = 0;
  bool mesh_ran = false, ao_ran = false;
  rc = volume_frame_shadowed_impl("volume_frame_ao", true, T, volumes, m, minv, n_inst, cam, queues, fb, depth, &base, O, fog_samples, mesh, &mesh_ran, true, &ao_ran);
  if (!rc && stats) {
    gvt_hip_volume_ao_frame_stats F{};
    F.base.fog.frame = O;
    F.base.fog.fog_samples_shadowed = fog_samples;
    F.base.mesh_shadowed = mesh_ran ? 1u : 0u;
    F.ao = ao_ran ? 1u : 0u;
    *stats = F;
  }
  return rc;
}

// ---- AMR volumes: the host side of volume_amr.inc (the contract: include/gvt_hip.h, "AMR volumes")
namespace {

// everything gvt_hip_volume_set_subgrids derives from the subgrids before the volume changes
struct AmrPlan {
  std::vector<int> level;                 // 1 .. GVT_HIP_VOLUME_MAX_LEVELS - 1
  std::vector<size_t> offset, count;      // first sample in d_amr_vox, samples
  std::vector<uint32_t> first, cnt;       // per macro cell: its level-1 subgrids in list
  std::vector<int> list;
  std::vector<int4> desc;
  std::vector<AmrRangeItem> items;
  std::vector<size_t> item_cell;          // the macro cell of every range item
  size_t total = 0;
  int levels = 1;
};

// the refusals of gvt_hip_volume_set_subgrids that concern the subgrids themselves; fills P
bool amr_plan(const gvt_hip_volume *V, const gvt_hip_subgrid *g, int n, AmrPlan &P) {
  const size_t nbk = (size_t)V->nb[0] * V->nb[1] * V->nb[2];
  P.level.assign(n, 0); P.offset.assign(n, 0); P.count.assign(n, 0);
  std::vector<long long> rt(n), p0((size_t)3 * n), nv((size_t)3 * n); // total ratio | vertex 0 and vertices per axis, in 1 / rt of a level-0 cell from the brick's vertex 0
  std::vector<std::vector<int>> kids(n), in_cell(nbk);
  for (int i = 0; i < n; i++) {
    const gvt_hip_subgrid &S = g[i];
    if (S.ratio != 2 && S.ratio != 4 && S.ratio != 8) { set_error("volume_set_subgrids: subgrid %d has ratio %d (2, 4 or 8)", i, S.ratio); return false; }
    if (S.parent < -1 || S.parent >= i) { set_error("volume_set_subgrids: subgrid %d names parent %d (-1 or an earlier entry)", i, S.parent); return false; }
    P.level[i] = S.parent < 0 ? 1 : P.level[S.parent] + 1;
    if (P.level[i] >= GVT_HIP_VOLUME_MAX_LEVELS) { set_error("volume_set_subgrids: subgrid %d is at level %d, at most %d levels", i, P.level[i], GVT_HIP_VOLUME_MAX_LEVELS); return false; }
    P.levels = std::max(P.levels, P.level[i] + 1);
    rt[i] = (S.parent < 0 ? 1 : rt[S.parent]) * S.ratio;
    size_t total = 1;
    for (int a = 0; a < 3; a++) {
      if (S.cells[a] < 1) { set_error("volume_set_subgrids: subgrid %d covers %d cells on axis %d", i, S.cells[a], a); return false; }
      const long long plo = S.parent < 0 ? V->off[a] : 0;
      const long long phi = S.parent < 0 ? (long long)V->off[a] + V->n[a] - 1 : (long long)g[S.parent].cells[a] * g[S.parent].ratio;
      if (S.lo[a] < plo || (long long)S.lo[a] + S.cells[a] > phi) {
        set_error("volume_set_subgrids: subgrid %d covers cells [%d, %lld) of axis %d, its parent has [%lld, %lld)", i, S.lo[a], (long long)S.lo[a] + S.cells[a], a, plo, phi);
        return false;
      }
      nv[3 * i + a] = (long long)S.cells[a] * S.ratio + 1;
      if (nv[3 * i + a] >= (1 << 24)) { set_error("volume_set_subgrids: subgrid %d is too large on axis %d", i, a); return false; }
      p0[3 * i + a] = (S.parent < 0 ? (long long)S.lo[a] - V->off[a] : p0[3 * S.parent + a] + S.lo[a]) * S.ratio;
      total *= (size_t)nv[3 * i + a];
    }
    if (total >= 0xffffffffull) { set_error("volume_set_subgrids: subgrid %d of %zu vertices is too large", i, total); return false; }
    for (int j = 0; j < i; j++) { // siblings must not share a cell
      if (g[j].parent != S.parent) continue;
      bool overlap = true;
      for (int a = 0; a < 3; a++) overlap = overlap && (long long)S.lo[a] < (long long)g[j].lo[a] + g[j].cells[a] && (long long)g[j].lo[a] < (long long)S.lo[a] + S.cells[a];
      if (overlap) { set_error("volume_set_subgrids: subgrids %d and %d of parent %d overlap", j, i, S.parent); return false; }
    }
    P.offset[i] = P.total; P.count[i] = total; P.total += total;
    if (S.parent >= 0) kids[S.parent].push_back(i);
    else
      for (int z = (S.lo[2] - V->off[2]) >> 3; z <= (S.lo[2] - V->off[2] + S.cells[2] - 1) >> 3; z++)
        for (int y = (S.lo[1] - V->off[1]) >> 3; y <= (S.lo[1] - V->off[1] + S.cells[1] - 1) >> 3; y++)
          for (int x = (S.lo[0] - V->off[0]) >> 3; x <= (S.lo[0] - V->off[0] + S.cells[0] - 1) >> 3; x++)
            in_cell[((size_t)z * V->nb[1] + y) * V->nb[0] + x].push_back(i);
    // the macro cells whose closed box holds vertices of this subgrid, and the index rectangle in each
    long long m0[3], m1[3];
    for (int a = 0; a < 3; a++) {
      const long long w = 8 * rt[i], last = p0[3 * i + a] + nv[3 * i + a] - 1;
      m0[a] = std::max(0ll, (p0[3 * i + a] - w + w - 1) / w); // the first macro cell with (8 m + 8) rt >= p0 (p0 >= 0)
      m1[a] = std::min((long long)V->nb[a] - 1, last / w);
    }
    for (long long z = m0[2]; z <= m1[2]; z++)
      for (long long y = m0[1]; y <= m1[1]; y++)
        for (long long x = m0[0]; x <= m1[0]; x++) {
          const long long m[3] = { x, y, z };
          AmrRangeItem I;
          I.base = P.offset[i]; I.nx = (unsigned)nv[3 * i]; I.nxy = (unsigned)(nv[3 * i] * nv[3 * i + 1]);
          for (int a = 0; a < 3; a++) {
            const long long i0 = std::max(0ll, 8 * m[a] * rt[i] - p0[3 * i + a]), i1 = std::min(nv[3 * i + a] - 1, (8 * m[a] + 8) * rt[i] - p0[3 * i + a]);
            I.i0[a] = (unsigned)i0; I.ext[a] = (unsigned)(i1 - i0 + 1);
          }
          P.items.push_back(I);
          P.item_cell.push_back(((size_t)z * V->nb[1] + y) * V->nb[0] + x);
        }
  }
  P.first.assign(nbk, 0u); P.cnt.assign(nbk, 0u);
  for (size_t b = 0; b < nbk; b++) {
    P.first[b] = (uint32_t)P.list.size(); P.cnt[b] = (uint32_t)in_cell[b].size();
    P.list.insert(P.list.end(), in_cell[b].begin(), in_cell[b].end());
  }
  P.desc.resize((size_t)4 * n);
  for (int i = 0; i < n; i++) {
    const gvt_hip_subgrid &S = g[i];
    const int shift = S.ratio == 2 ? 1 : S.ratio == 4 ? 2 : 3;
    const int rel[3] = { S.parent < 0 ? V->off[0] : 0, S.parent < 0 ? V->off[1] : 0, S.parent < 0 ? V->off[2] : 0 };
    P.desc[4 * (size_t)i] = make_int4(S.lo[0] - rel[0], S.lo[1] - rel[1], S.lo[2] - rel[2], shift);
    P.desc[4 * (size_t)i + 1] = make_int4(S.cells[0], S.cells[1], S.cells[2], (int)nv[3 * i]);
    P.desc[4 * (size_t)i + 2] = make_int4((int)(unsigned)(nv[3 * i] * nv[3 * i + 1]), (int)P.list.size(), (int)kids[i].size(), 0);
    P.desc[4 * (size_t)i + 3] = make_int4((int)(unsigned)(P.offset[i] & 0xffffffffull), (int)(unsigned)(P.offset[i] >> 32), 0, 0);
    P.list.insert(P.list.end(), kids[i].begin(), kids[i].end());
  }
  if (P.list.empty()) P.list.push_back(0); // (never read: no allocation of zero bytes)
  return true;
}

void amr_release(gvt_hip_volume *V) {
  hipFree(V->d_amr_vox); hipFree(V->d_amr_mc); hipFree(V->d_amr_list); hipFree(V->d_amr_desc);
  V->d_amr_vox = nullptr; V->d_amr_mc = nullptr; V->d_amr_list = nullptr; V->d_amr_desc = nullptr;
  hipFree(V->d_amr_items); hipFree(V->d_amr_cells); // (the merge tables of gvt_hip_volume_update_amr belong to the tree)
  V->d_amr_items = nullptr; V->d_amr_cells = nullptr; V->amr_n_cells = 0; V->amr_merge_bytes = 0;
  V->amr_offset.clear(); V->amr_samples.clear();
  V->sub.clear(); V->amr_first.clear(); V->amr_count.clear();
  V->amr_levels = 1; V->amr_bytes = 0; V->amr_flags = 0;
}

// the subgrids' part of the macro cells' value ranges, as gvt_hip_volume_set_subgrids has just reduced it (empty: no subgrids).  The volume
// keeps no copy: bmin / bmax / bnan hold the union, and gvt_hip_volume_update_amr forms the next step's union on the device
struct AmrHostRanges {
  std::vector<float> mn, mx;
  std::vector<uint8_t> wild;
};

// bmin / bmax / bnan, vmin / vmax: the level-0 ranges afresh from d_vox, then the subgrids' part merged in; the tables from the union
int amr_refresh_ranges(gvt_hip_volume *V, const AmrHostRanges &R) {
  int rc = volume_ranges(V);
  if (rc) return rc;
  for (size_t b = 0; b < R.mn.size(); b++) {
    if (R.mn[b] < V->bmin[b]) V->bmin[b] = R.mn[b];
    if (R.mx[b] > V->bmax[b]) V->bmax[b] = R.mx[b];
    V->bnan[b] |= R.wild[b];
    if (R.mn[b] < V->vmin) V->vmin = R.mn[b];
    if (R.mx[b] > V->vmax) V->vmax = R.mx[b];
  }
  return V->has_tf ? rebuild_tables(V) : 0;
}

} // namespace

extern "C" int gvt_hip_volume_set_subgrids(gvt_hip_volume *V, const gvt_hip_subgrid *grids, const float *const *samples, int n, int flags) {
  if (ensure_init()) return GVT_HIP_ERR_NODEVICE;
  if (!V || (n > 0 && (!grids || !samples))) { set_error("volume_set_subgrids: null argument"); return GVT_HIP_ERR_INVALID; }
  if (n < 0 || n > GVT_HIP_VOLUME_MAX_SUBGRIDS) { set_error("volume_set_subgrids: %d subgrids, at most %d", n, GVT_HIP_VOLUME_MAX_SUBGRIDS); return GVT_HIP_ERR_INVALID; }
  if (flags & ~(GVT_HIP_VOLUME_DEVICE | GVT_HIP_VOLUME_AMR_SHADED)) { set_error("volume_set_subgrids: unknown flag bits %d", flags); return GVT_HIP_ERR_INVALID; }
  if (V->vtype != GVT_HIP_VOXEL_F32) { set_error("volume_set_subgrids: the volume holds voxel type %d, subgrids are float32", V->vtype); return GVT_HIP_ERR_INVALID; }
  if (!(flags & GVT_HIP_VOLUME_AMR_SHADED) && (V->n_iso + V->n_pl > 0 || V->shade == GVT_HIP_VOLUME_SHADE_GRADIENT)) {
    set_error("volume_set_subgrids: the volume has surfaces or gradient shading, which AMR volumes do not take");
    return GVT_HIP_ERR_INVALID;
  }
  if (n > 0 && V->grad == GVT_HIP_VOLUME_GRADIENT_CENTRAL) {
    set_error("volume_set_subgrids: the volume's gradient kind is CENTRAL, which AMR volumes do not take");
    return GVT_HIP_ERR_INVALID;
  }
  for (int i = 0; i < n; i++)
    if (!samples[i]) { set_error("volume_set_subgrids: subgrid %d has no samples", i); return GVT_HIP_ERR_INVALID; }
  hipStream_t st = gctx().stream;
  if (n == 0) {
    if (V->sub.empty()) return 0;
    HIPCHK(hipStreamSynchronize(st)); // (a march in flight reads the tables)
    V->lg.current = false; // (a light grid never covers subgrids, and the ranges change)
    V->og.current = false;
    V->ag.current = false;
    amr_release(V);
    return amr_refresh_ranges(V, AmrHostRanges{});
  }
  AmrPlan P;
  if (!amr_plan(V, grids, n, P)) return GVT_HIP_ERR_INVALID;
  // the new device tables and the subgrids' ranges, all before the volume changes
  const size_t nbk = P.first.size(), n_items = P.items.size();
  float *d_vox = nullptr;
  uint2 *d_mc = nullptr;
  int *d_list = nullptr;
  int4 *d_desc = nullptr;
  AmrRangeItem *d_items = nullptr;
  AmrRangeOut *d_out = nullptr;
  std::vector<AmrRangeOut> out(n_items);
  auto fail = [&](const char *what) {
    set_error("volume_set_subgrids: %s failed: %s", what, hipGetErrorString(hipGetLastError()));
    hipFree(d_vox); hipFree(d_mc); hipFree(d_list); hipFree(d_desc); hipFree(d_items); hipFree(d_out);
    return GVT_HIP_ERR_DEVICE;
  };
  HIPCHK(hipStreamSynchronize(st));
  bool ok = hipMalloc((void **)&d_vox, sizeof(float) * P.total) == hipSuccess && hipMalloc((void **)&d_mc, sizeof(uint2) * nbk) == hipSuccess &&
            hipMalloc((void **)&d_list, sizeof(int) * P.list.size()) == hipSuccess && hipMalloc((void **)&d_desc, sizeof(int4) * P.desc.size()) == hipSuccess &&
            hipMalloc((void **)&d_items, sizeof(AmrRangeItem) * n_items) == hipSuccess && hipMalloc((void **)&d_out, sizeof(AmrRangeOut) * n_items) == hipSuccess;
  if (!ok) return fail("device allocation");
  const hipMemcpyKind kind = (flags & GVT_HIP_VOLUME_DEVICE) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  for (int i = 0; i < n && ok; i++) ok = hipMemcpyAsync(d_vox + P.offset[i], samples[i], sizeof(float) * P.count[i], kind, st) == hipSuccess;
  ok = ok && hipMemcpyAsync(d_list, P.list.data(), sizeof(int) * P.list.size(), hipMemcpyHostToDevice, st) == hipSuccess &&
       hipMemcpyAsync(d_desc, P.desc.data(), sizeof(int4) * P.desc.size(), hipMemcpyHostToDevice, st) == hipSuccess &&
       hipMemcpyAsync(d_items, P.items.data(), sizeof(AmrRangeItem) * n_items, hipMemcpyHostToDevice, st) == hipSuccess;
  if (!ok) return fail("upload");
  {
    ProfScope ps(KC_BUILD);
    k_amr_ranges<<<(unsigned)std::min(n_items, (size_t)1 << 20), VOL_BLOCK, 0, st>>>(d_vox, d_items, (unsigned)n_items, d_out);
  }
  ok = hipGetLastError() == hipSuccess && hipMemcpyAsync(out.data(), d_out, sizeof(AmrRangeOut) * n_items, hipMemcpyDeviceToHost, st) == hipSuccess &&
       hipStreamSynchronize(st) == hipSuccess;
  if (!ok) return fail("the range kernel");
  hipFree(d_items); hipFree(d_out);
  // commit
  V->lg.current = false;
  V->og.current = false;
  V->ag.current = false;
  amr_release(V);
  V->d_amr_vox = d_vox; V->d_amr_mc = d_mc; V->d_amr_list = d_list; V->d_amr_desc = d_desc;
  V->sub.assign(grids, grids + n);
  V->amr_levels = P.levels;
  V->amr_flags = flags & GVT_HIP_VOLUME_AMR_SHADED;
  V->amr_bytes = sizeof(float) * P.total + sizeof(uint2) * nbk + sizeof(int) * P.list.size() + sizeof(int4) * P.desc.size();
  V->amr_first.swap(P.first); V->amr_count.swap(P.cnt);
  AmrHostRanges R;
  R.mn.assign(nbk, INFINITY); R.mx.assign(nbk, -INFINITY); R.wild.assign(nbk, 0);
  for (size_t i = 0; i < n_items; i++) {
    const size_t b = P.item_cell[i];
    if (out[i].mn < R.mn[b]) R.mn[b] = out[i].mn;
    if (out[i].mx > R.mx[b]) R.mx[b] = out[i].mx;
    R.wild[b] |= (uint8_t)out[i].wild;
  }
  int rc = amr_upload_words(V); // (before a transfer function: no skip bit yet; rebuild_tables uploads them again)
  if (rc) return rc;
  return amr_refresh_ranges(V, R);
}

// ---- time-varying AMR volumes (the contract: include/gvt_hip.h, "time-varying AMR volumes")
namespace {

// k_amr_ranges_merge's tables, once per tree: amr_plan's range items of the stored subgrids in the order of their macro cells, one
// AmrMergeCell per macro cell that has items, and every subgrid's place in d_amr_vox.  Nothing of the volume changes on failure
int amr_merge_tables(gvt_hip_volume *V) {
  if (V->d_amr_items) return 0;
  AmrPlan P;
  if (!amr_plan(V, V->sub.data(), (int)V->sub.size(), P)) return GVT_HIP_ERR_INVALID; // (not reached: _set_subgrids accepted this tree)
  const size_t nbk = P.first.size(), n_items = P.items.size();
  std::vector<unsigned> start(nbk + 1, 0u);
  for (size_t i = 0; i < n_items; i++) start[P.item_cell[i] + 1]++;
  for (size_t b = 0; b < nbk; b++) start[b + 1] += start[b];
  std::vector<AmrMergeCell> cells;
  for (size_t b = 0; b < nbk; b++)
    if (start[b + 1] > start[b]) cells.push_back(AmrMergeCell{ (unsigned)b, start[b], start[b + 1] - start[b] });
  std::vector<AmrRangeItem> items(n_items);
  std::vector<unsigned> at(start.begin(), start.end() - 1);
  for (size_t i = 0; i < n_items; i++) items[at[P.item_cell[i]]++] = P.items[i];
  AmrRangeItem *d_items = nullptr;
  AmrMergeCell *d_cells = nullptr;
  const bool ok = hipMalloc((void **)&d_items, sizeof(AmrRangeItem) * n_items) == hipSuccess && hipMalloc((void **)&d_cells, sizeof(AmrMergeCell) * cells.size()) == hipSuccess &&
                  hipMemcpy(d_items, items.data(), sizeof(AmrRangeItem) * n_items, hipMemcpyHostToDevice) == hipSuccess &&
                  hipMemcpy(d_cells, cells.data(), sizeof(AmrMergeCell) * cells.size(), hipMemcpyHostToDevice) == hipSuccess;
  if (!ok) {
    set_error("volume_update_amr: the merge tables: %s", hipGetErrorString(hipGetLastError()));
    hipFree(d_items); hipFree(d_cells);
    return GVT_HIP_ERR_DEVICE;
  }
  V->d_amr_items = d_items; V->d_amr_cells = d_cells; V->amr_n_cells = (unsigned)cells.size();
  V->amr_merge_bytes = sizeof(AmrRangeItem) * n_items + sizeof(AmrMergeCell) * cells.size();
  V->amr_offset.swap(P.offset); V->amr_samples.swap(P.count);
  return 0;
}

} // namespace

extern "C" int gvt_hip_volume_update_amr(gvt_hip_volume *V, const float *samples, size_t n_samples, const float *const *subgrid_samples, int n_subgrids, uint32_t flags,
                                         float *ms_out) {
  if (ensure_init()) return GVT_HIP_ERR_NODEVICE;
  if (!V) { set_error("volume_update_amr: null volume"); return GVT_HIP_ERR_INVALID; }
  if (flags & ~GVT_HIP_UPDATE_DEVICE) { set_error("volume_update_amr: unknown flags 0x%x", flags); return GVT_HIP_ERR_INVALID; }
  if (V->sub.empty()) { set_error("volume_update_amr: the volume has no AMR subgrids (its time steps go through gvt_hip_volume_update_samples)"); return GVT_HIP_ERR_INVALID; }
  const size_t total = (size_t)V->n[0] * V->n[1] * V->n[2];
  if (n_samples != (samples ? total : 0)) {
    set_error("volume_update_amr: %zu level-0 samples given, the brick has %zu (%d x %d x %d; 0 with NULL keeps them)", n_samples, total, V->n[0], V->n[1], V->n[2]);
    return GVT_HIP_ERR_INVALID;
  }
  if (n_subgrids != (subgrid_samples ? (int)V->sub.size() : 0)) {
    set_error("volume_update_amr: samples of %d subgrids given, the volume has %zu (0 with NULL keeps them all; another tree is gvt_hip_volume_set_subgrids)", n_subgrids, V->sub.size());
    return GVT_HIP_ERR_INVALID;
  }
  bool any = samples != nullptr;
  for (int i = 0; i < n_subgrids; i++) any = any || subgrid_samples[i] != nullptr;
  if (!any) { set_error("volume_update_amr: no samples given, neither level 0's nor a subgrid's"); return GVT_HIP_ERR_INVALID; }
  hipStream_t st = gctx().stream;
  HIPCHK(hipStreamSynchronize(st)); // (a march in flight reads the samples)
  int rc = amr_merge_tables(V);
  if (rc) return rc;
  V->lg.current = false; // (a light grid baked from the old samples is stale; the occluder grid reads meshes, lights and the tree: it stays)
  V->ag.current = false; // (... and so is an AO grid)
  const hipMemcpyKind kind = (flags & GVT_HIP_UPDATE_DEVICE) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  if (samples) HIPCHK(hipMemcpyAsync(V->d_vox, samples, sizeof(float) * total, kind, st));
  for (int i = 0; i < n_subgrids; i++)
    if (subgrid_samples[i]) HIPCHK(hipMemcpyAsync(V->d_amr_vox + V->amr_offset[i], subgrid_samples[i], sizeof(float) * V->amr_samples[i], kind, st));
  hipEvent_t e0, e1;
  HIPCHK(hipEventCreate(&e0));
  if (hipEventCreate(&e1) != hipSuccess) { hipEventDestroy(e0); set_error("volume_update_amr: hipEventCreate failed"); return GVT_HIP_ERR_DEVICE; }
  rc = hipEventRecord(e0, st) == hipSuccess ? 0 : GVT_HIP_ERR_DEVICE;
  if (!rc) rc = volume_ranges(V, true); // level 0, the subgrids merged in, the total: one download of the union
  if (!rc && V->has_tf) rc = rebuild_tables(V); // (else: built when the transfer function arrives)
  float ms = 0.f;
  if (!rc && (hipEventRecord(e1, st) != hipSuccess || hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&ms, e0, e1) != hipSuccess)) {
    set_error("volume_update_amr: %s", hipGetErrorString(hipGetLastError()));
    rc = GVT_HIP_ERR_DEVICE;
  }
  hipStreamSynchronize(st);
  hipEventDestroy(e0); hipEventDestroy(e1);
  if (!rc && ms_out) *ms_out = ms;
  return rc;
}

extern "C" int gvt_hip_volume_get_amr_info(gvt_hip_volume *V, gvt_hip_volume_amr_info *out) {
  if (ensure_init()) return GVT_HIP_ERR_NODEVICE;
  if (!V || !out) { set_error("volume_get_amr_info: null"); return GVT_HIP_ERR_INVALID; }
  unsigned long long s = 0;
  HIPCHK(hipStreamSynchronize(gctx().stream));
  HIPCHK(hipMemcpy(&s, V->d_stats + 4, sizeof(s), hipMemcpyDeviceToHost));
  gvt_hip_volume_amr_info I{};
  I.n_subgrids = (int32_t)V->sub.size(); I.n_levels = V->amr_levels;
  I.subgrid_bytes = V->amr_bytes; I.samples_refined = s; I.amr_marches = V->amr_marches;
  *out = I;
  return 0;
}
