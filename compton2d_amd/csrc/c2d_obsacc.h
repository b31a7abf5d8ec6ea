/*
 * c2d_obsacc.h — the exact observer accumulation (include/compton2d.h
 * "Exact observer sets"), one arithmetic for the device
 * kernel (obsacc.hip), the host twin (c2d_obs_exact_host) and the exported
 * state (c2d_obs_set_state, c2d_obs_set_merge).
 *
 * A member with bulk factor G and the caller's bound w_max on one event's
 * rest-frame weight has the exponent bound e = E(w_max) + E(2 G), E the
 * frexp exponent (x = f 2^E(x), 0.5 <= f < 1): a boosted weight
 * w = ew G (1 + mu beta), |mu| <= 1, lies below 2^e.  A bin holds
 *
 *   F      u128 in units of 2^qF,   qF  = e - 84:   + floor(w / 2^qF)
 *   F2     u128 in units of 2^qF2,  qF2 = 2e - 84:  + floor(fl(w w) / 2^qF2)
 *   count  u64:                                      + 1
 *
 * per event; both addends are below 2^84, so a bin has 2^44 worst-case
 * addends of headroom.  w NaN, negative or >= 2^e: added nowhere (the
 * member's n_rejected counts the event).  Truncation depends on the addend
 * alone, integer addition commutes: any order gives the same integers.
 * -469 <= e <= 489 keeps every quantum and every sum a normal double.
 *
 * Header-only C++ that also compiles as HIP device code; integer work but
 * for fl(w w): compile with contraction off.
 */
#ifndef C2D_OBSACC_H
#define C2D_OBSACC_H

#include <stdint.h>

#include "c2d_math.h"   /* C2D_HD, c2d_bits, c2d_from_bits */

#define C2D_OA_E_MIN (-469)
#define C2D_OA_E_MAX 489
#define C2D_OA_BITS 84                     /* an addend is below 2^84 */
#define C2D_OA_BIN_WORDS 5                 /* F_lo F_hi F2_lo F2_hi count */
#define C2D_OA_HEAD_WORDS 8
#define C2D_OA_MAGIC 0x005853424f443243ull /* "C2DOBSX\0" */
#define C2D_OA_VERSION 1u

/* the frexp exponent of a finite x > 0 */
C2D_HD int c2d_oa_exponent(double x) {
  const uint64_t b = c2d_bits(x);
  const int be = (int)((b >> 52) & 0x7ffull);
  if (be) return be - 1022;
  uint64_t m = b & 0xfffffffffffffull;     /* subnormal: m 2^-1074 */
  int p = -1;
  while (m) { m >>= 1; p++; }
  return p + 1 - 1074;
}

C2D_HD int c2d_oa_finite(double x) { return ((c2d_bits(x) >> 52) & 0x7ffull) != 0x7ffull; }

/* a member's exponent bound; the caller checks the range */
C2D_HD int c2d_oa_member_e(double w_max, double G) { return c2d_oa_exponent(w_max) + c2d_oa_exponent(2. * G); }
C2D_HD int c2d_oa_e_ok(int e) { return e >= C2D_OA_E_MIN && e <= C2D_OA_E_MAX; }

/* 2^k as a double, -1022 <= k <= 1023 */
C2D_HD double c2d_oa_pow2(int k) { return c2d_from_bits((uint64_t)(k + 1023) << 52); }

/* true if w is added at all: not NaN, not negative, below 2^e */
C2D_HD int c2d_oa_accepts(double w, int e) { return (w >= 0.0) && (w < c2d_oa_pow2(e)); }

/* floor(x / 2^q) of a finite 0 <= x < 2^(q + 84) as (lo, hi) */
C2D_HD void c2d_oa_quant(double x, int q, uint64_t* lo, uint64_t* hi) {
  const uint64_t b = c2d_bits(x) & 0x7fffffffffffffffull;
  const int be = (int)(b >> 52);
  const uint64_t m = be ? ((b & 0xfffffffffffffull) | (1ull << 52)) : b;   /* x = m 2^ex */
  const int s = (be ? be - 1075 : -1074) - q;
  if (s >= 0) {                            /* s <= 31: the addend has at most 84 bits */
    *lo = m << s;
    *hi = s ? (m >> (64 - s)) : 0ull;
  } else {
    *lo = (-s < 64) ? (m >> (-s)) : 0ull;
    *hi = 0ull;
  }
}

/* (lo, hi) += (alo, ahi); the carry out of bit 127 */
C2D_HD int c2d_oa_add(uint64_t* lo, uint64_t* hi, uint64_t alo, uint64_t ahi) {
  const uint64_t l = *lo + alo;
  const uint64_t c = l < alo ? 1ull : 0ull;
  const uint64_t h = *hi + ahi;
  const uint64_t h2 = h + c;
  const int out = (h < ahi) || (h2 < c);
  *lo = l;
  *hi = h2;
  return out;
}

/* (lo, hi) 2^q rounded to the nearest double, ties to even; the result must
 * be zero or a normal double (-1022 <= q, 128 + q <= 1023) */
C2D_HD double c2d_oa_to_double(uint64_t lo, uint64_t hi, int q) {
  if (!(lo | hi)) return 0.0;
  int p = 0;                               /* position of the top bit, 0..127 */
  if (hi) { uint64_t t = hi; p = 64; while (t >>= 1) p++; }
  else { uint64_t t = lo; while (t >>= 1) p++; }
  if (p <= 52) return (double)lo * c2d_oa_pow2(q);
  const int k = p - 52;                    /* bits dropped, 1..75 */
  uint64_t m, rem_hi, rem_lo;              /* v = m 2^k + rem */
  if (k < 64) {
    m = (lo >> k) | (hi << (64 - k));
    rem_hi = 0ull;
    rem_lo = lo & ((1ull << k) - 1ull);
  } else {
    m = k == 64 ? hi : (hi >> (k - 64));
    rem_hi = k == 64 ? 0ull : (hi & ((1ull << (k - 64)) - 1ull));
    rem_lo = lo;
  }
  /* half = 2^(k-1) as (half_lo, half_hi) */
  const uint64_t half_hi = k > 64 ? (1ull << (k - 65)) : 0ull;
  const uint64_t half_lo = k <= 64 ? (1ull << (k - 1)) : 0ull;
  const int above = rem_hi > half_hi || (rem_hi == half_hi && rem_lo > half_lo);
  const int tie = rem_hi == half_hi && rem_lo == half_lo;
  if (above || (tie && (m & 1ull))) m++;   /* m <= 2^53: exact as a double */
  return (double)m * c2d_oa_pow2(q + k);
}

/* ---- one event's addends ---- */
struct c2d_oa_addend {
  uint64_t f_lo, f_hi, f2_lo, f2_hi;
};

/* the addends of an accepted weight w for a member of exponent bound e */
C2D_HD c2d_oa_addend c2d_oa_addend_of(double w, int e) {
  c2d_oa_addend a;
  c2d_oa_quant(w, e - C2D_OA_BITS, &a.f_lo, &a.f_hi);
  c2d_oa_quant(w * w, 2 * e - C2D_OA_BITS, &a.f2_lo, &a.f2_hi);
  return a;
}

/* ---- the state's head (include/compton2d.h): word 1 = version | mode << 32,
 * word 2 = n_t | n_mu << 32, word 3 = n_e, word 4 = e (two's complement) ---- */
C2D_HD uint64_t c2d_oa_head1(int32_t mode) { return (uint64_t)C2D_OA_VERSION | ((uint64_t)(uint32_t)mode << 32); }
C2D_HD uint64_t c2d_oa_head2(int32_t n_t, int32_t n_mu) { return (uint64_t)(uint32_t)n_t | ((uint64_t)(uint32_t)n_mu << 32); }

#endif /* C2D_OBSACC_H */
