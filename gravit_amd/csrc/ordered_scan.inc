// ordered_scan.inc -- the order-preserving slot scan of the shuffles (included by sched.hip and volume.hip inside their anonymous namespaces)
//
// Ordered mode (few destinations): exclusive scan of the per-block counts of one destination, offset by the queue's fill,
// so that the scatter can place every ray at a slot that depends only on its index in the input list -- queues keep the order
// of the list they were filled from (camera rays stay in pixel order; no sort is needed in front of the traversal) and the
// result of a shuffle is deterministic.  One block of BLOCK threads per destination.  A destination with keep != 0 has its count
// word advanced to the new fill here; with keep == 0 the word stays as it is.  totals (optional): the rays each destination receives.
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_dest_scan(unsigned *__restrict__ blk_cnt, unsigned n_blk, const QueueDesc *__restrict__ queues,
                                                     unsigned *__restrict__ totals) {
  __shared__ unsigned sh_w[BLOCK / 64];
  __shared__ unsigned sh_run;
  const int d = blockIdx.x;
  unsigned *row = blk_cnt + (size_t)d * n_blk;
  __shared__ unsigned sh_start;
  if (threadIdx.x == 0) { sh_run = *queues[d].count; sh_start = sh_run; }
  __syncthreads();
  for (unsigned b0 = 0; b0 < n_blk; b0 += BLOCK) {
    const unsigned b = b0 + threadIdx.x;
    const unsigned v = b < n_blk ? row[b] : 0u;
    unsigned incl = v;
    for (int o = 1; o < 64; o <<= 1) { const unsigned u = __shfl_up(incl, o); if ((int)lane_id() >= o) incl += u; }
    if (lane_id() == 63) sh_w[threadIdx.x >> 6] = incl;
    __syncthreads();
    unsigned woff = 0;
    for (unsigned w = 0; w < (threadIdx.x >> 6); w++) woff += sh_w[w];
    const unsigned run = sh_run;
    if (b < n_blk) row[b] = run + woff + incl - v;
    __syncthreads();
    if (threadIdx.x == BLOCK - 1) sh_run = run + woff + incl;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    if (queues[d].keep) *queues[d].count = sh_run;
    if (totals) totals[d] = sh_run - sh_start;
  }
}
