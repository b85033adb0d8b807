// xcd_stripes.h -- the stripe mapping of a traversal launch's ray list (k_trace, single-mesh instantiations), for kernels and host code alike.
//
// The chip has XCD_STRIPES dies (XCDs), each with an L2 of its own, and blocks are dealt to them round-robin.  A ray list that is handed out front to
// back puts neighbouring units on different XCDs, so every L2 has to hold the whole band of the film the chip is working on.  Here the list is seen as
// ROWS of R rays (the camera's tile-ordered list: one row of 8x8 tiles across the film); every row is cut into XCD_STRIPES contiguous parts, one per
// stripe, on 64-ray boundaries, and every part into the same number m of UNITS of at most u rays.  Stripe x hands out its units in the order t = 0, 1, ...:
// unit t lies in row t / m for every stripe, so the stripes go down the film together while each keeps to its own columns.
//   - the units of all stripes cover [0, n) exactly once; n, R need not be multiples of anything (the last stripe takes a row's odd end)
//   - a part shorter than m units -- R is not a multiple of 8u -- has EMPTY units (begin == end) at its end: asked for and passed over
//   - R == 0 (a list without film geometry: bounce lists, index lists): rows of XCD_DEFAULT_ROW_UNITS units, four consecutive units per stripe
#pragma once

#ifndef XCD_FN
#if defined(__HIPCC__) || defined(__CUDACC__)
#define XCD_FN __host__ __device__ static inline
#else
#define XCD_FN static inline
#endif
#endif

#define XCD_STRIPES 8
#define XCD_DEFAULT_ROW_UNITS 32
#define XCD_STRIPES_OFF 0xffffffffu // in place of a row length: the launch hands its list out front to back, from one counter

struct XcdStripeMap {
  unsigned n;     // rays in the list
  unsigned u;     // rays per unit (a multiple of 64)
  unsigned row;   // rays per row (never 0)
  unsigned tiles; // whole 64-ray tiles per row
  unsigned m;     // units per stripe and row (never 0)
  float inv_m;    // 1 / m: unit number -> row without an integer division (a GPU has none)
};

XCD_FN XcdStripeMap xcd_stripe_map(unsigned n, unsigned u, unsigned R) {
  XcdStripeMap M;
  M.n = n; M.u = u;
  M.row = R ? R : XCD_DEFAULT_ROW_UNITS * u;
  M.tiles = M.row >> 6;
  // the longest part is the last stripe's: its share of the tiles, rounded up, and the row's odd end
  const unsigned longest = ((M.tiles + XCD_STRIPES - 1) / XCD_STRIPES) * 64u + (M.row & 63u);
  M.m = (longest + u - 1) / u;
  if (!M.m) M.m = 1;
  M.inv_m = 1.0f / (float)M.m;
  return M;
}

// first ray of stripe x's part within a row (x == XCD_STRIPES: the row's end)
XCD_FN unsigned xcd_stripe_begin(const XcdStripeMap &M, unsigned x) { return x < XCD_STRIPES ? ((x * M.tiles) / XCD_STRIPES) * 64u : M.row; }

// unit t of stripe x: [*begin, *end) of the list (empty: begin == end); false = the stripe is exhausted (so is every later unit of it)
XCD_FN bool xcd_stripe_unit(const XcdStripeMap &M, unsigned x, unsigned t, unsigned *begin, unsigned *end) {
  unsigned r = (unsigned)((float)t * M.inv_m); // t / m, give or take one
  while ((unsigned long long)r * M.m > t) r--;
  while (((unsigned long long)r + 1u) * M.m <= t) r++;
  const unsigned k = t - r * M.m;
  const unsigned long long row0 = (unsigned long long)r * M.row;
  if (row0 >= M.n) return false;
  const unsigned long long lo = (unsigned long long)xcd_stripe_begin(M, x) + (unsigned long long)k * M.u, part_end = xcd_stripe_begin(M, x + 1);
  unsigned long long b = row0 + (lo < part_end ? lo : part_end), e = row0 + (lo + M.u < part_end ? lo + M.u : part_end);
  if (b > M.n) b = M.n;
  if (e > M.n) e = M.n;
  if (e < b) e = b;
  *begin = (unsigned)b; *end = (unsigned)e;
  return true;
}
