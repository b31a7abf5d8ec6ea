/*
 * c2d_split.h — the upper weight window of census population control
 * (include/compton2d.h "Census splitting"), one rule for the
 * device pass (split.hip), the host twin (c2d_census_split_host) and the
 * numpy yardstick (compton2d_amd/popcontrol.py).
 *
 * A census record in cell (jph, kph) with energy weight ew, spectral bin
 * jgpsp (bits 0-7 of its bins word) and lineage key `key` is tested against
 * the ceiling W = w_max[jph-1][kph-1][g], g = group_of_sp[min(jgpsp, NPHOMAX)]:
 *
 *   untouched   !(W > 0), W not finite, ew not finite or !(ew > W): m = 1
 *   otherwise   q = ew / W (one IEEE division);
 *               m = max_copies if !(q < max_copies), else (int)ceil(q) >= 2;
 *               all m copies weigh ew / (double)m (one IEEE division);
 *               copy 0 is the record itself, copy i = 1..m-1 equals it word
 *               for word but for its key,
 *               derive(key, TAG_SPLIT, salt lo, salt hi; sub i).
 *
 * m ew' = ew up to one rounding, a packet's history does not depend on its
 * weight and every tally is linear in ew, so every tally keeps its
 * expectation; the copies fly on independent lineage streams, so the pass
 * lowers the variance the heavy record carried.  The result is a pure
 * function of (record, ceiling, max_copies, salt).
 *
 * Header-only C that also compiles as C++ and as HIP device code; compile
 * with contraction off (no FMA can form here, but the build says so).
 */
#ifndef C2D_SPLIT_H
#define C2D_SPLIT_H

#include <stdint.h>

#include "c2d_rng.h"
#include "c2d_roulette.h"   /* c2d_roulette_bits, c2d_roulette_sp: the shared group lookup */

#ifndef C2D_SPLIT_COPIES_MAX
#define C2D_SPLIT_COPIES_MAX 64
#endif

C2D_RHD int c2d_split_finite(double x) {
  return ((c2d_roulette_bits(x) >> 52) & 0x7ffull) != 0x7ffull;
}

/* the ceil of a finite q in (1, 64): exact integer arithmetic, no libm */
C2D_RHD int c2d_split_ceil(double q) {
  const int t = (int)q;   /* truncation; q > 0 */
  return (double)t < q ? t + 1 : t;
}

/* the rule: m, the number of records the record becomes (1: untouched);
 * *ew_out = the weight of each of them */
C2D_RHD int c2d_split_copies(double ew, double W, int max_copies, double* ew_out) {
  *ew_out = ew;
  if (!(W > 0.0) || !c2d_split_finite(W) || !c2d_split_finite(ew) || !(ew > W)) return 1;
  const double q = ew / W;
  const int m = !(q < (double)max_copies) ? max_copies : c2d_split_ceil(q);
  *ew_out = ew / (double)m;
  return m;
}

/* the key of copy i (1 <= i < m) of the record whose key is `key` */
C2D_RHD uint64_t c2d_split_key(uint64_t key, uint64_t salt, int i) {
  return c2d_derive_s(key, C2D_TAG_SPLIT, (uint32_t)salt, (uint32_t)(salt >> 32), (uint32_t)i);
}

#endif /* C2D_SPLIT_H */
