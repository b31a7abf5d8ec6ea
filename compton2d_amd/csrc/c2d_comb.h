/*
 * c2d_comb.h — the census comb (include/compton2d.h "Census comb",
 * DESIGN.md 4k): the critical floor of a census record under the
 * weight-window roulette (c2d_roulette.h), one rule for the device kernels
 * (comb.hip), the host twin (c2d_census_comb_host) and the numpy yardstick
 * (compton2d_amd/popcontrol.py comb_critical).
 *
 * The roulette keeps a tested record under the floor w iff S(w) := u < ew / w
 * (one IEEE division), u = draw 0 of derive(key, TAG_ROULETTE, salt lo,
 * salt hi), and leaves ew >= w alone; as u < 1, ew >= w implies S(w).  S
 * only turns false as w grows, so a record has a critical floor
 *
 *   w* = the largest finite double w with S(w)       (0 for ew == 0)
 *
 * and for w > 0 it stays under the roulette iff w <= w*.  The procedure is
 * fixed so that every restatement gives the same bits:
 *
 *   w0 = ew / u, an infinite w0 taken as DBL_MAX;
 *   while !S(w0): w0 one ulp down      (at most C2D_COMB_STEPS times)
 *   while S(next double above w0): w0 one ulp up      (the same bound)
 *
 * (u is (x + 0.5) 2^-53 rounded to double, which is 1 for x = 2^53 - 1 alone:
 * for that one draw in 2^53 the record stays at w == ew while w* lies one ulp
 * below.)
 *
 * The floors of the comb are t * norm[cell][group] with norm a power of two:
 * a record's normalised critical value c = w* / norm (exact) is its priority
 * (Duffield, Lund & Thorup 2007), and the floors t * norm keep exactly the
 * records with c >= t.  A record no floor of this family can remove is
 * `fixed`: !(norm > 0), norm not finite, !(ew >= 0), ew not finite, or a cell
 * off the grid.
 *
 * The 64-bit pattern of c >= 0 orders as an unsigned integer; the selection
 * reads it in six digits, bits 63-53, 52-42, 41-31, 30-20, 19-9 and 8-0
 * (C2D_COMB_BINS bins, of which the last digit uses 512).
 *
 * Header-only C that also compiles as C++ and as HIP device code; compile
 * with contraction off (no FMA can form here, but the build says so).
 */
#ifndef C2D_COMB_H
#define C2D_COMB_H

#include <stdint.h>
#include <string.h>

#include "c2d_roulette.h"

#ifndef C2D_COMB_BINS
#define C2D_COMB_BINS 2048
#endif
#define C2D_COMB_DIGIT_BITS 11
#define C2D_COMB_LAST_PREFIX 55   /* prefix bits before the last, 9-bit digit */
#define C2D_COMB_STEPS 8

C2D_RHD double c2d_comb_from_bits(uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __longlong_as_double((long long)b);
#else
  double x;
  memcpy(&x, &b, sizeof x);
  return x;
#endif
}

C2D_RHD int c2d_comb_finite(double x) { return ((c2d_roulette_bits(x) >> 52) & 0x7ffull) != 0x7ffull; }

/* x positive, finite and a power of two (subnormal ones included) */
C2D_RHD int c2d_comb_pow2(double x) {
  const uint64_t b = c2d_roulette_bits(x), e = (b >> 52) & 0x7ffull, m = b & 0xfffffffffffffull;
  if (b >> 63 || e == 0x7ffull) return 0;
  return e ? m == 0 : (m != 0 && (m & (m - 1)) == 0);
}

/* the roulette's predicate for a tested record: it survives the floor w */
C2D_RHD int c2d_comb_survives(double ew, double u, double w) { return u < ew / w; }

/* w* of a record of weight ew >= 0 (finite) whose roulette draw is u */
C2D_RHD double c2d_comb_wstar(double ew, double u) {
  if (ew == 0.0) return 0.0;
  uint64_t b = c2d_roulette_bits(ew / u);
  if (b >= 0x7ff0000000000000ull) b = 0x7fefffffffffffffull;   /* DBL_MAX */
  /* positive doubles: the next one up or down is the next integer pattern (DBL_MAX + 1 is +inf: S false) */
  for (int k = 0; k < C2D_COMB_STEPS && b > 0 && !c2d_comb_survives(ew, u, c2d_comb_from_bits(b)); k++) b--;
  for (int k = 0; k < C2D_COMB_STEPS && c2d_comb_survives(ew, u, c2d_comb_from_bits(b + 1)); k++) b++;
  return c2d_comb_from_bits(b);
}

/* 1 for a record no floor t * norm can remove */
C2D_RHD int c2d_comb_fixed(double ew, double norm, int on_grid) {
  return !on_grid || !(norm > 0.0) || !c2d_comb_finite(norm) || !(ew >= 0.0) || !c2d_comb_finite(ew);
}

/* c of a record that is not fixed */
C2D_RHD double c2d_comb_critical(double ew, double norm, uint64_t key, uint64_t salt) {
  const uint64_t K = c2d_derive(key, C2D_TAG_ROULETTE, (uint32_t)salt, (uint32_t)(salt >> 32));
  return c2d_comb_wstar(ew, c2d_draw(K, 0u)) / norm;
}

/* prefix_bits is one of 0, 11, 22, 33, 44, 55 and prefix has no bit above it */
C2D_RHD int c2d_comb_prefix_ok(uint64_t prefix, int prefix_bits) {
  if (prefix_bits < 0 || prefix_bits > C2D_COMB_LAST_PREFIX || prefix_bits % C2D_COMB_DIGIT_BITS) return 0;
  return prefix_bits == 0 ? prefix == 0 : (prefix >> prefix_bits) == 0;
}

/* the top prefix_bits bits of cbits are prefix */
C2D_RHD int c2d_comb_match(uint64_t cbits, uint64_t prefix, int prefix_bits) {
  return prefix_bits == 0 || (cbits >> (64 - prefix_bits)) == prefix;
}

/* the digit below the top prefix_bits bits */
C2D_RHD uint32_t c2d_comb_digit(uint64_t cbits, int prefix_bits) {
  if (prefix_bits >= C2D_COMB_LAST_PREFIX) return (uint32_t)(cbits & 0x1ffull);
  return (uint32_t)((cbits >> (64 - C2D_COMB_DIGIT_BITS - prefix_bits)) & 0x7ffull);
}

#endif /* C2D_COMB_H */
