/*
 * c2d_roulette.h — the weight-window roulette of census population control
 * (include/compton2d.h "Census population control"), one rule
 * for the device pass (roulette.hip), the host twin
 * (c2d_census_roulette_host) and the numpy yardstick
 * (compton2d_amd/popcontrol.py).
 *
 * A census record in cell (jph, kph) with energy weight ew, spectral bin
 * jgpsp (bits 0-7 of its bins word) and lineage key `key` is tested against
 * the floor w = w_min[jph-1][kph-1][g], g = group_of_sp[min(jgpsp, NPHOMAX)]:
 *
 *   untouched   !(w > 0), w not finite, !(ew >= 0) or ew >= w
 *   otherwise   p = ew / w (one IEEE division), u = draw 0 of the key
 *               derive(key, TAG_ROULETTE, salt lo, salt hi);
 *               u < p: the record survives with ew = w exactly,
 *               else it is removed.
 *
 * E[ew'] = p w = ew, so every tally, which is linear in ew, keeps its
 * expectation; the decision is a pure function of (record, floor, salt), so
 * it does not depend on the lane, chunk, census mode or GPU that holds the
 * record.  The derived key keeps the decision independent of the packet's
 * own streams, which draw from `key` directly.
 *
 * Header-only C that also compiles as C++ and as HIP device code; compile
 * with contraction off (no FMA can form here, but the build says so).
 */
#ifndef C2D_ROULETTE_H
#define C2D_ROULETTE_H

#include <stdint.h>
#include <string.h>

#include "c2d_rng.h"

#ifndef C2D_ROULETTE_GROUPS_MAX
#define C2D_ROULETTE_GROUPS_MAX 32
#endif
#define C2D_ROULETTE_NSP 129   /* C2D_NPHOMAX + 1 entries of group_of_sp */

#define C2D_ROULETTE_UNTOUCHED 0
#define C2D_ROULETTE_SURVIVES  1   /* ew becomes the floor */
#define C2D_ROULETTE_REMOVED   2

C2D_RHD uint64_t c2d_roulette_bits(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint64_t)__double_as_longlong(x);
#else
  uint64_t b;
  memcpy(&b, &x, sizeof b);
  return b;
#endif
}

/* the index into group_of_sp of a record's bins word */
C2D_RHD int c2d_roulette_sp(uint32_t bins) {
  const uint32_t sp = bins & 0xffu;
  return (int)(sp < (uint32_t)(C2D_ROULETTE_NSP - 1) ? sp : (uint32_t)(C2D_ROULETTE_NSP - 1));
}

/* true if the floor w tests a record of weight ew at all */
C2D_RHD int c2d_roulette_tested(double ew, double w) {
  const int finite = ((c2d_roulette_bits(w) >> 52) & 0x7ffull) != 0x7ffull;
  return (w > 0.0) && finite && (ew >= 0.0) && !(ew >= w);
}

/* the rule: C2D_ROULETTE_*; *ew_out = the record's weight afterwards (ew
 * itself unless it survives a test) */
C2D_RHD int c2d_roulette_decide(double ew, double w, uint64_t key, uint64_t salt, double* ew_out) {
  *ew_out = ew;
  if (!c2d_roulette_tested(ew, w)) return C2D_ROULETTE_UNTOUCHED;
  const double p = ew / w;
  const uint64_t K = c2d_derive(key, C2D_TAG_ROULETTE, (uint32_t)salt, (uint32_t)(salt >> 32));
  const double u = c2d_draw(K, 0u);
  if (u < p) {
    *ew_out = w;
    return C2D_ROULETTE_SURVIVES;
  }
  return C2D_ROULETTE_REMOVED;
}

#endif /* C2D_ROULETTE_H */
