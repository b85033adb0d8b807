// Stand-alone check of the stripe mapping (gravit_amd/csrc/xcd_stripes.h): for every list length, unit size and row length of the grid below, the units of the eight
// stripes cover [0, n) exactly once, unit t of every stripe lies within two rows of unit t of every other, every unit holds at most u rays, a stripe's units go up the
// list, and "exhausted" is final.  Built with -fsanitize=address,undefined by tests/test_xcd_stripes_host.py; prints "ok <cases>" and exits 0, or the first failure and 1.
#include <cstdio>
#include <vector>

#include "xcd_stripes.h"

static int fail(const char *what, unsigned n, unsigned u, unsigned R, unsigned x, unsigned t) {
  std::printf("FAILED: %s (n %u, u %u, R %u, stripe %u, unit %u)\n", what, n, u, R, x, t);
  return 1;
}

int main() {
  const unsigned us[] = { 64, 128, 320 }, Rs[] = { 0, 64, 576, 1000, 2048, 8192 };
  unsigned long cases = 0;
  std::vector<unsigned char> seen;
  for (unsigned n = 0; n <= 4200; n++)
    for (unsigned u : us)
      for (unsigned R : Rs) {
        const XcdStripeMap M = xcd_stripe_map(n, u, R);
        const unsigned row = R ? R : XCD_DEFAULT_ROW_UNITS * u;
        if (M.row != row || !M.m) return fail("row length / units per row", n, u, R, 0, 0);
        seen.assign(n, 0);
        unsigned long covered = 0;
        unsigned n_units[XCD_STRIPES];
        std::vector<unsigned> row_of[XCD_STRIPES]; // row of every non-empty unit, by unit number (~0u: empty)
        for (unsigned x = 0; x < XCD_STRIPES; x++) {
          unsigned t = 0, last_end = 0;
          for (;; t++) {
            unsigned b = 0, e = 0;
            if (!xcd_stripe_unit(M, x, t, &b, &e)) break;
            if (t > n / 64 * 16 + 64) return fail("a stripe never ends", n, u, R, x, t);
            if (b > e || e > n) return fail("bounds", n, u, R, x, t);
            if (e - b > u) return fail("a unit longer than u", n, u, R, x, t);
            row_of[x].push_back(b < e ? b / row : ~0u);
            if (b == e) continue;
            if (b < last_end) return fail("a stripe's units do not go up the list", n, u, R, x, t);
            if ((e - 1) / row != b / row) return fail("a unit in two rows", n, u, R, x, t);
            last_end = e;
            for (unsigned i = b; i < e; i++) { if (seen[i]) return fail("a ray twice", n, u, R, x, t); seen[i] = 1; }
            covered += e - b;
          }
          n_units[x] = t;
          for (unsigned k = 1; k <= 16; k++) { // exhausted once: exhausted for good
            unsigned b, e;
            if (xcd_stripe_unit(M, x, t + k * 7u, &b, &e)) return fail("a unit behind the stripe's end", n, u, R, x, t + k * 7u);
          }
        }
        if (covered != n) return fail("rays left out", n, u, R, 0, 0);
        for (unsigned x = 0; x < XCD_STRIPES; x++)
          for (unsigned y = 0; y < XCD_STRIPES; y++)
            for (unsigned t = 0; t < n_units[x] && t < n_units[y]; t++) {
              const unsigned rx = row_of[x][t], ry = row_of[y][t];
              if (rx == ~0u || ry == ~0u) continue;
              if ((rx > ry ? rx - ry : ry - rx) > 2u) return fail("unit t of two stripes more than two rows apart", n, u, R, x, t);
            }
        // within a row a stripe owns ONE contiguous part, the parts in stripe order
        for (unsigned x = 0; x + 1 <= XCD_STRIPES; x++)
          if (xcd_stripe_begin(M, x) > xcd_stripe_begin(M, x + 1) || xcd_stripe_begin(M, x + 1) > row) return fail("parts of a row out of order", n, u, R, x, 0);
        cases++;
      }
  // beyond the grid: lists of 2^32 - 1 rays (the 64-bit row products), the benchmark's row, a row longer than the list
  const unsigned big[][3] = { { 0xffffffffu, 64, 15360 }, { 0xffffffffu, 4096, 0 }, { 0xfffffff0u, 320, 0x7fffffc0u }, { 2073600u, 64, 15360 }, { 100u, 64, 8192 } };
  for (const auto &c : big) {
    const XcdStripeMap M = xcd_stripe_map(c[0], c[1], c[2]);
    unsigned long long total = 0;
    for (unsigned x = 0; x < XCD_STRIPES; x++) {
      // (sampled: every unit of short lists, the first and last thousands of long ones -- the sum needs all of them, so long lists are summed by rows instead)
      unsigned b, e;
      const unsigned long long rows = ((unsigned long long)c[0] + M.row - 1) / M.row;
      const unsigned long long last = rows * M.m; // units of this stripe
      if (xcd_stripe_unit(M, x, (unsigned)last, &b, &e)) return fail("big: a unit behind the last row", c[0], c[1], c[2], x, (unsigned)last);
      if (last && !xcd_stripe_unit(M, x, (unsigned)(last - 1), &b, &e)) return fail("big: the last row's unit missing", c[0], c[1], c[2], x, (unsigned)(last - 1));
      if (last <= 4000000ull)
        for (unsigned t = 0; t < last; t++) { if (!xcd_stripe_unit(M, x, t, &b, &e) || b > e || e > c[0] || e - b > c[1]) return fail("big: bounds", c[0], c[1], c[2], x, t); total += e - b; }
    }
    if (total && total != c[0]) return fail("big: rays left out", c[0], c[1], c[2], 0, 0);
    cases++;
  }
  std::printf("ok %lu\n", cases);
  return 0;
}
