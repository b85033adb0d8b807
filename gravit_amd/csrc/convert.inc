// convert.inc -- layout conversions at the ABI boundary, ray sort keys, the small bookkeeping kernels of a trace call (included by trace.hip inside its anonymous namespace)
// ------------------------------------------------------------------------------------------------
// layout conversions at the ABI boundary: 80-byte Ray AoS <-> planes
// ------------------------------------------------------------------------------------------------
// keep_state: bytes 64..79 of the incoming rays are this library's own (an exported ray coming back: its RNG stream word and its known-miss list).
// Otherwise they are whatever the host left there -- the reference's Ray(origin, dir, ...) constructor never writes data[64..79] (Ray.h:106-116) --
// and the ray starts fresh: stream word 0 (keyed on its list index when first shaded), no known misses.
__global__ __launch_bounds__(256) void k_aos_to_planes(const float4 *__restrict__ src /* 5 float4 per ray */, unsigned n, RayPlanes dst,
                                                        unsigned long long off, int keep_state) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float4 *s = src + (size_t)5 * i;
  dst.p0[off + i] = s[0]; dst.p1[off + i] = s[1]; dst.p2[off + i] = s[2]; dst.p3[off + i] = s[3];
  const float4 st = keep_state ? s[4] : make_float4(0.f, 0.f, 0.f, 0.f);
  if (dst.p4) dst.p4[off + i] = __float_as_uint(st.x); // bytes 64..67: the stream word
  if (dst.p5) { dst.p5[3 * (off + i)] = __float_as_uint(st.y); dst.p5[3 * (off + i) + 1] = __float_as_uint(st.z); dst.p5[3 * (off + i) + 2] = __float_as_uint(st.w); } // 68..79: known misses
}
__global__ __launch_bounds__(256) void k_planes_to_aos(RayPlanes src, unsigned long long off, unsigned n, float4 *__restrict__ dst) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float4 *d = dst + (size_t)5 * i;
  d[0] = src.p0[off + i]; d[1] = src.p1[off + i]; d[2] = src.p2[off + i]; d[3] = src.p3[off + i];
  d[4] = make_float4(__uint_as_float(src.p4 ? src.p4[off + i] : 0u), __uint_as_float(src.p5 ? src.p5[3 * (off + i)] : 0u), __uint_as_float(src.p5 ? src.p5[3 * (off + i) + 1] : 0u),
                     __uint_as_float(src.p5 ? src.p5[3 * (off + i) + 2] : 0u));
}
// ---- the same two conversions for ALL the queues of one exchange message in one launch (gvt_hip_queues_export_wire / _append_wire).
// Ray i of the concatenation belongs to queue s = the last one with begin[s] <= i (begin: n + 1 prefix sums, begin[n] = the total; empty
// queues repeat a value and are never chosen), where it is slot off[s] + (i - begin[s]).  Absent p4 / p5 planes read as 0 and are not
// written, as above.  The launch also writes the queues' count words (fill[s]; one thread per queue), so a message is one launch.
struct WireTable {
  const QueueDesc *q;
  const unsigned *begin; // n + 1
  const unsigned *off;   // n: export 0, append the queue's fill before the call
  const unsigned *fill;  // n: the count word after the call (export 0, append off + the run)
  int n;
};
#define WIRE_BLOCK 256
__device__ __forceinline__ int wire_queue_of(const WireTable &W, unsigned i) {
  int lo = 0, hi = W.n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (W.begin[mid] <= i) lo = mid; else hi = mid;
  }
  return lo;
}
__device__ __forceinline__ void wire_set_counts(const WireTable &W) {
  for (unsigned s = blockIdx.x * WIRE_BLOCK + threadIdx.x; s < (unsigned)W.n; s += gridDim.x * WIRE_BLOCK)
    if (W.begin[s + 1] != W.begin[s]) *W.q[s].count = W.fill[s]; // (a queue without rays in the message keeps its word)
}
// Export: k_planes_to_aos' pattern -- coalesced plane reads, five 16-byte stores per lane at an 80-byte stride.  Staging a wave's 5120
// contiguous wire bytes through LDS so that every store covers 1 KiB was measured and is 15 % slower here (EXPERIMENTS.md, "wire pair").
__global__ __launch_bounds__(WIRE_BLOCK) void k_queues_to_wire(WireTable W, unsigned total, float4 *__restrict__ dst) {
  wire_set_counts(W);
  const unsigned i = blockIdx.x * WIRE_BLOCK + threadIdx.x;
  if (i >= total) return;
  const int s = wire_queue_of(W, i);
  const QueueDesc Q = W.q[s];
  const RayPlanes P = make_planes(Q.planes, Q.cap);
  const size_t j = (size_t)W.off[s] + (i - W.begin[s]);
  float4 *d = dst + (size_t)5 * i;
  d[0] = P.p0[j]; d[1] = P.p1[j]; d[2] = P.p2[j]; d[3] = P.p3[j];
  d[4] = make_float4(__uint_as_float(P.p4 ? P.p4[j] : 0u), __uint_as_float(P.p5 ? P.p5[3 * j] : 0u), __uint_as_float(P.p5 ? P.p5[3 * j + 1] : 0u),
                     __uint_as_float(P.p5 ? P.p5[3 * j + 2] : 0u));
}
// Append: the other way round the staging pays (25 % less kernel time than five 16-byte loads per lane at an 80-byte stride): a wave's
// 64 rays are 5120 contiguous wire bytes, read as five loads of 1 KiB into the wave's part of LDS, then every lane takes its ray's five
// pieces from there and writes the planes coalesced.
__global__ __launch_bounds__(WIRE_BLOCK) void k_wire_to_queues(const float4 *__restrict__ src, unsigned total, WireTable W) {
  __shared__ float4 sh[WIRE_BLOCK * 5];
  wire_set_counts(W);
  const unsigned i = blockIdx.x * WIRE_BLOCK + threadIdx.x;
  const unsigned lane = threadIdx.x & 63u;
  float4 *w = sh + (size_t)(threadIdx.x - lane) * 5; // the wave's 320 pieces
  const unsigned base = i - lane;                    // the wave's first ray
  if (base < total) {
    const unsigned m = min(64u, total - base) * 5u;
    for (unsigned k = 0; k < 5; k++) {
      const unsigned x = k * 64u + lane;
      if (x < m) w[x] = src[(size_t)5 * base + x];
    }
  }
  __syncthreads();
  if (i >= total) return;
  float4 r[5];
  for (int k = 0; k < 5; k++) r[k] = w[lane * 5 + k];
  const int s = wire_queue_of(W, i);
  const QueueDesc Q = W.q[s];
  const RayPlanes P = make_planes(Q.planes, Q.cap);
  const size_t j = (size_t)W.off[s] + (i - W.begin[s]);
  P.p0[j] = r[0]; P.p1[j] = r[1]; P.p2[j] = r[2]; P.p3[j] = r[3];
  if (P.p4) P.p4[j] = __float_as_uint(r[4].x); // the rays are this library's own: their state is kept (k_aos_to_planes' keep_state)
  if (P.p5) { P.p5[3 * j] = __float_as_uint(r[4].y); P.p5[3 * j + 1] = __float_as_uint(r[4].z); P.p5[3 * j + 2] = __float_as_uint(r[4].w); }
}
__global__ __launch_bounds__(256) void k_od_to_planes(const float *__restrict__ org, const float *__restrict__ dir, unsigned n, RayPlanes dst) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  dst.p0[i] = make_float4(org[3 * i], org[3 * i + 1], org[3 * i + 2], GVT_RAY_EPSILON);
  dst.p1[i] = make_float4(dir[3 * i], dir[3 * i + 1], dir[3 * i + 2], GVT_FLT_MAX);
}

// ------------------------------------------------------------------------------------------------
// Ray sorting: 30-bit Morton code of the object-space origin inside the mesh box + direction octant.
// Neighbouring lanes then walk neighbouring nodes (fewer divergent iterations, more L1/L2 hits).
// ------------------------------------------------------------------------------------------------
__device__ inline unsigned expand10(unsigned v) {
  v &= 0x3ffu;
  v = (v | (v << 16)) & 0x030000ffu;
  v = (v | (v << 8)) & 0x0300f00fu;
  v = (v | (v << 4)) & 0x030c30c3u;
  v = (v | (v << 2)) & 0x09249249u;
  return v;
}
// n_dev (a list whose length only the device knows -- a bounce list, trace.hip wave_trace_chain): entries j >= *n_dev of the n the launch covers get the largest
// key, so that the sort of all n leaves the list's real entries in front
__global__ __launch_bounds__(256) void k_ray_keys(RayPlanes q, const unsigned *__restrict__ idx, unsigned n, Mat4 minv, float3 blo, float3 inv_ext,
                                                   unsigned *__restrict__ keys, unsigned *__restrict__ vals, int key_bits, const unsigned *__restrict__ n_dev = nullptr) {
  const unsigned j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  if (n_dev && j >= *n_dev) { keys[j] = 0xffffffffu >> (32 - key_bits); vals[j] = 0u; return; }
  const unsigned i = idx ? idx[j] : j;
  const float4 a = q.p0[i], b = q.p1[i];
  const V3 O = xfm_point(minv, mk3(a.x, a.y, a.z)), D = xfm_vector(minv, mk3(b.x, b.y, b.z));
  // the point where the ray enters the mesh's box (the origin itself for rays that start inside): camera rays, which all
  // leave one eye point, are thereby keyed by where they hit the box face -- 2-D tiles of the image instead of scanlines
  const float bhx = blo.x + (inv_ext.x > 0.f ? 1.f / inv_ext.x : 0.f), bhy = blo.y + (inv_ext.y > 0.f ? 1.f / inv_ext.y : 0.f),
              bhz = blo.z + (inv_ext.z > 0.f ? 1.f / inv_ext.z : 0.f);
  const float rx = 1.f / (fabsf(D.x) < 1e-30f ? copysignf(1e-30f, D.x) : D.x), ry = 1.f / (fabsf(D.y) < 1e-30f ? copysignf(1e-30f, D.y) : D.y),
              rz = 1.f / (fabsf(D.z) < 1e-30f ? copysignf(1e-30f, D.z) : D.z);
  const float t_in = fmaxf(fmaxf(fminf((blo.x - O.x) * rx, (bhx - O.x) * rx), fminf((blo.y - O.y) * ry, (bhy - O.y) * ry)),
                           fmaxf(fminf((blo.z - O.z) * rz, (bhz - O.z) * rz), 0.f));
  const float te = t_in < 1e30f ? t_in : 0.f;
  const float px = (O.x + D.x * te - blo.x) * inv_ext.x, py = (O.y + D.y * te - blo.y) * inv_ext.y, pz = (O.z + D.z * te - blo.z) * inv_ext.z;
  const unsigned qx = (unsigned)fminf(fmaxf(px * 1024.f, 0.f), 1023.f);
  const unsigned qy = (unsigned)fminf(fmaxf(py * 1024.f, 0.f), 1023.f);
  const unsigned qz = (unsigned)fminf(fmaxf(pz * 1024.f, 0.f), 1023.f);
  const unsigned oct = (D.x < 0.f ? 4u : 0u) | (D.y < 0.f ? 2u : 0u) | (D.z < 0.f ? 1u : 0u);
  const unsigned morton = (expand10(qx) << 2) | (expand10(qy) << 1) | expand10(qz);
  keys[j] = ((oct << 29) | (morton >> 1)) >> (32 - key_bits); // top key_bits bits: octant, then the coarsest Morton levels
  vals[j] = i;
}

__global__ __launch_bounds__(256) void k_math_probe(int kind, const float *__restrict__ in, unsigned n, float *__restrict__ out) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float x = in[i];
  out[i] = kind == 0 ? gvt_sinf(x) : kind == 1 ? gvt_cosf(x) : (float)gvt_acos(__builtin_sqrt(1.0 - (double)x));
}

__global__ void k_set_u32(unsigned *p, unsigned v) { if (threadIdx.x == 0 && blockIdx.x == 0) *p = v; }
// start of a trace call: moved_rays count := its current size, work counter / shadow count / next count := 0 (one launch, not three memsets)
__global__ void k_trace_begin(unsigned *out_count, unsigned out_size, unsigned *counters) {
  if (blockIdx.x == 0 && threadIdx.x < 5) counters[threadIdx.x] = 0u; // CW_WORK, CW_SHADOW, CW_BOUNCE_A, CW_LONG, CW_LONG_WORK
  if (blockIdx.x == 0 && threadIdx.x == 5) *out_count = out_size;
}

// after the sort: object-space origin/direction of the rays in sorted order, as two contiguous planes, so that the
// traversal kernel's lane refills read consecutive memory (the transform is the one k_trace<XFORM> would apply)
__global__ __launch_bounds__(256) void k_gather_od(RayPlanes q, const unsigned *__restrict__ idx, unsigned n, Mat4 minv, float4 *__restrict__ o_out,
                                                    float4 *__restrict__ d_out) {
  const unsigned j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const unsigned i = idx[j];
  const float4 a = q.p0[i], b = q.p1[i];
  const V3 O = xfm_point(minv, mk3(a.x, a.y, a.z)), D = xfm_vector(minv, mk3(b.x, b.y, b.z));
  o_out[j] = make_float4(O.x, O.y, O.z, a.w);
  d_out[j] = make_float4(D.x, D.y, D.z, b.w);
}
