/*
 * c2d_scan.h — one 14-byte E14.7 field of the escape-event file back to the
 * double it names: the inverse of c2d_fmt.h.  One function for the host (C99
 * under gcc) and the device (hipcc); integer arithmetic only, so both give
 * the same bits.
 *
 * Grammar of a canonical field (exactly 14 bytes, right-justified):
 *     [ -]0.dddddddE[+-]dd      or      [ -]0.ddddddd[+-]ddd
 * The second is the three-digit-exponent form without the E that flang and
 * c2d_fmt.h write.  Any seven digits are taken, leading zeros included; seven
 * zeros give +-0.0 with the sign of the field.  Anything else is "not
 * canonical" and nothing is written.  The E-less form is read as the number
 * that was written; fscanf("%lf") would split it into two tokens.
 *
 * Value: the double nearest to D 10^p, p = x - 7, ties to
 * even, for every exponent the grammar can express (subnormal results,
 * underflow to 0 and overflow to inf included): glibc's strtod of the E-form.
 *
 * Fast path.  D is normalised to 64 bits (m64 = D 2^lz) and multiplied by
 * the 128-bit T of c2d_fmt_tab, 10^p = (T + t) 2^b with 0 <= t < 1.  With
 * P = m64 T = top 2^128 + mid 2^64 + low the value is (P + err) 2^(b - lz),
 * 0 <= err < 2^64.  top holds 63 or 64 significant bits, of which 53 are
 * kept; the round bit and the sticky bits just below it are bits of top too
 * (at least 10 are dropped), then come mid and low.  err is below one unit
 * of mid, so it changes the rounding in two cases only.  It may decide
 * whether the discarded part is exactly 1/2 or more: round bit set, every
 * bit of top below it and mid zero.  Or it may carry out of mid (mid all
 * ones) into a discarded part of top that is 0111...1, which the carry turns
 * into 1/2 or more; a carry into any other pattern leaves the rounding as it
 * was (all ones round up with or without it, which also keeps exactly
 * representable values such as 0.5, whose truncated T puts P just below
 * them, on the fast path).  Those two cases are ambiguous and go to the
 * exact path, as do exponents outside the table and results below the
 * normal range.  Every exact decimal-to-binary tie is of the first kind:
 * there 10^p is exact in T and the product ends in zeros.
 *
 * Exact path (c2d_scan_exact): the multi-limb integers of c2d_fmt.h.  For
 * p >= 0 the top 64 bits of D 5^p and whether anything lies below them; for
 * p < 0 a 55- or 56-bit quotient of D 2^s by 5^-p by restoring division and
 * whether the remainder is zero.  Both end in c2d_scan_round, which is all
 * of the rounding, the subnormal range and the overflow.
 */
#ifndef C2D_SCAN_H
#define C2D_SCAN_H

#include "c2d_fmt.h"

/* status of c2d_scan_e14_7* */
#define C2D_SCAN_OK 0
#define C2D_SCAN_EXACT 1          /* decided by c2d_scan_exact */
#define C2D_SCAN_NOTCANON (-1)    /* not a canonical field: nothing written */

/* The double nearest to (M + f) 2^e, ties to even, as its bits: M != 0,
 * 0 <= f < 1, sticky = (f != 0).  Overflow gives inf, the subnormal range
 * rounds at 2^-1074. */
C2D_FMT_HD uint64_t c2d_scan_round(uint64_t M, int sticky, int e) {
  const int L = 64 - __builtin_clzll(M);
  int E = e + L - 1;               /* floor(log2 value) */
  int drop = L - 53;
  if (E < -1022) drop = -1074 - e; /* the last kept bit is 2^-1074 */
  uint64_t mant;
  if (drop <= 0) {
    mant = M << -drop;             /* exact: sticky is 0 whenever M has under 53 bits */
  } else {
    if (drop > 64) return 0;       /* the value is below 2^-1075 */
    const uint64_t rb = (M >> (drop - 1)) & 1u;
    const int st = sticky || (M & (((uint64_t)1 << (drop - 1)) - 1u)) != 0;
    mant = drop < 64 ? M >> drop : 0u;
    if (rb && (st || (mant & 1u))) mant++;
  }
  if (E < -1022) return mant;      /* 2^52 here is the smallest normal number: the same bits */
  if (mant >> 53) { mant >>= 1; E++; }
  if (E > 1023) return (uint64_t)0x7ff << 52;
  return ((uint64_t)(E + 1023) << 52) | (mant & 0x000fffffffffffffull);
}

/* a -= b over the lowest nl limbs (a >= b) */
C2D_FMT_HD void c2d_scan_big_sub(c2d_fmt_big* a, const c2d_fmt_big* b, int nl) {
  uint64_t borrow = 0;
  C2D_FMT_ROLLED
  for (int i = 0; i < nl; i++) {
    const uint64_t d = (uint64_t)a->w[i] - b->w[i] - borrow;
    a->w[i] = (uint32_t)d;
    borrow = (d >> 32) & 1u;
  }
}
C2D_FMT_HD int c2d_scan_big_bitlen(const c2d_fmt_big* a) {
  C2D_FMT_ROLLED
  for (int i = C2D_FMT_LIMBS - 1; i >= 0; i--)
    if (a->w[i]) return 32 * i + 32 - __builtin_clz(a->w[i]);
  return 0;
}

/* Exact path: the bits of the double nearest to D 10^p, 0 < D < 10^7,
 * -331 <= p <= 308 (5^331 has 769 bits; the integers stay below 2^900). */
C2D_FMT_SLOW uint64_t c2d_scan_exact(uint32_t D, int p) {
  c2d_fmt_big A, Q;
  if (p >= 0) {   /* D 5^p 2^p */
    c2d_fmt_big_pow5(&A, p);
    c2d_fmt_big_mul(&A, D);
    const int L = c2d_scan_big_bitlen(&A);
    const int lo = L > 64 ? L - 64 : 0;
    uint64_t M = 0;
    C2D_FMT_ROLLED
    for (int i = 63; i >= 0; i--) M = (M << 1) | c2d_fmt_big_bit(&A, lo + i);
    int sticky = 0;
    C2D_FMT_ROLLED
    for (int i = 0; i < lo; i++) sticky |= (int)c2d_fmt_big_bit(&A, i);
    return c2d_scan_round(M, sticky, p + lo);
  }
  /* D / (5^n 2^n): the quotient of D 2^s by 5^n with 55 or 56 bits */
  const int n = -p;
  c2d_fmt_big_pow5(&Q, n);
  const int Lq = c2d_scan_big_bitlen(&Q);
  const int Ld = 32 - __builtin_clz(D);
  const int s = 55 + Lq - Ld;          /* > 0: Lq >= 3, Ld <= 24 */
  int nl = (Lq + 1 + 31) / 32 + 1;     /* limbs that hold a remainder doubled */
  if (nl > C2D_FMT_LIMBS) nl = C2D_FMT_LIMBS;
  c2d_fmt_big_set(&A, 0);
  uint64_t quot = 0;
  C2D_FMT_ROLLED
  for (int i = Ld + s - 1; i >= 0; i--) {
    uint32_t carry = i >= s ? (D >> (i - s)) & 1u : 0u;   /* A = 2 A + the next bit of D 2^s */
    C2D_FMT_ROLLED
    for (int k = 0; k < nl; k++) {
      const uint32_t w = A.w[k];
      A.w[k] = (w << 1) | carry;
      carry = w >> 31;
    }
    int ge = 1;
    C2D_FMT_ROLLED
    for (int k = nl - 1; k >= 0; k--)
      if (A.w[k] != Q.w[k]) { ge = A.w[k] > Q.w[k]; break; }
    quot <<= 1;
    if (ge) {
      c2d_scan_big_sub(&A, &Q, nl);
      quot |= 1u;
    }
  }
  int rem = 0;
  C2D_FMT_ROLLED
  for (int k = 0; k < nl; k++) rem |= A.w[k] != 0;
  return c2d_scan_round(quot, rem, -s - n);
}

/* The field as two little-endian words (w0: bytes 0-7, w1: bytes 8-13, the
 * bytes above them ignored) to the bits of its double.  Returns C2D_SCAN_OK,
 * C2D_SCAN_EXACT or C2D_SCAN_NOTCANON (*bits is then untouched).
 * force_exact != 0 sends every non-zero field to c2d_scan_exact (tests). */
C2D_FMT_HD int c2d_scan_e14_7_pack_opt(const c2d_fmt_tab* tab, uint64_t w0, uint64_t w1, uint64_t* bits,
                                       int force_exact) {
  const uint32_t c0 = (uint32_t)(w0 & 0xffu);
  if ((c0 != ' ' && c0 != '-') || ((w0 >> 8) & 0xffffu) != (uint32_t)('0' | '.' << 8)) return C2D_SCAN_NOTCANON;
  uint32_t D = 0, bad = 0;
  for (int i = 3; i < 10; i++) {
    const uint32_t d = (uint32_t)((i < 8 ? w0 >> (8 * i) : w1 >> (8 * (i - 8))) & 0xffu) - '0';
    bad |= d > 9u;
    D = 10u * D + d;
  }
  const uint32_t b10 = (uint32_t)(w1 >> 16) & 0xffu, b11 = (uint32_t)(w1 >> 24) & 0xffu;
  const uint32_t d12 = ((uint32_t)(w1 >> 32) & 0xffu) - '0', d13 = ((uint32_t)(w1 >> 40) & 0xffu) - '0';
  bad |= d12 > 9u || d13 > 9u;
  int x, neg;
  if (b10 == 'E') {
    if (b11 != '+' && b11 != '-') return C2D_SCAN_NOTCANON;
    neg = b11 == '-';
    x = (int)(10u * d12 + d13);
  } else {
    if (b10 != '+' && b10 != '-') return C2D_SCAN_NOTCANON;
    const uint32_t d11 = b11 - '0';
    bad |= d11 > 9u;
    neg = b10 == '-';
    x = (int)(100u * d11 + 10u * d12 + d13);
  }
  if (bad) return C2D_SCAN_NOTCANON;
  const uint64_t sign = (uint64_t)(c0 == '-') << 63;
  const int p = (neg ? -x : x) - 7;
  /* D 10^p < 10^(p+7) <= 10^-324 < 2^-1075 rounds to zero; D 10^p >= 10^309 is beyond the largest double */
  if (D == 0 || p + 7 <= -324) { *bits = sign; return C2D_SCAN_OK; }
  if (p > 308) { *bits = sign | (uint64_t)0x7ff << 52; return C2D_SCAN_OK; }
  if (!force_exact && p >= C2D_FMT_QMIN && p <= C2D_FMT_QMAX) {
    const int idx = p - C2D_FMT_QMIN;
    const int lz = __builtin_clzll((uint64_t)D);
    const uint64_t m64 = (uint64_t)D << lz;
    const unsigned __int128 a = (unsigned __int128)m64 * tab->hi[idx];
    const unsigned __int128 c = (unsigned __int128)m64 * tab->lo[idx];
    const uint64_t a_lo = (uint64_t)a, c_hi = (uint64_t)(c >> 64);
    const uint64_t mid = a_lo + c_hi;
    const uint64_t top = (uint64_t)(a >> 64) + (mid < a_lo ? 1u : 0u);   /* bit 62 or 63 is its highest */
    const int e = (int)tab->b[idx] - lz + 128;                           /* D 10^p = (top + f) 2^e */
    const int drop = (top >> 63) ? 11 : 10;
    if (e + drop + 52 >= -1022) {   /* a normal result (or overflow) */
      const uint64_t below = top & (((uint64_t)1 << drop) - 1u);
      const uint64_t half = (uint64_t)1 << (drop - 1);
      const int ambiguous = (mid == ~(uint64_t)0 && below == half - 1u) || (mid == 0 && below == half);
      if (!ambiguous) {
        *bits = sign | c2d_scan_round(top, 1, e);   /* whether mid, low and err are zero no longer matters */
        return C2D_SCAN_OK;
      }
    }
  }
  *bits = sign | c2d_scan_exact(D, p);
  return C2D_SCAN_EXACT;
}

C2D_FMT_HD int c2d_scan_e14_7_pack(const c2d_fmt_tab* tab, uint64_t w0, uint64_t w1, uint64_t* bits) {
  return c2d_scan_e14_7_pack_opt(tab, w0, w1, bits, 0);
}

/* The same from 14 bytes at s into *out. */
C2D_FMT_HD int c2d_scan_e14_7_opt(const c2d_fmt_tab* tab, const char* s, double* out, int force_exact) {
  uint64_t w0 = 0, w1 = 0, bits;
  for (int i = 0; i < 8; i++) w0 |= (uint64_t)(unsigned char)s[i] << (8 * i);
  for (int i = 0; i < 6; i++) w1 |= (uint64_t)(unsigned char)s[8 + i] << (8 * i);
  const int st = c2d_scan_e14_7_pack_opt(tab, w0, w1, &bits, force_exact);
  if (st < 0) return st;
  __builtin_memcpy(out, &bits, sizeof bits);
  return st;
}

C2D_FMT_HD int c2d_scan_e14_7(const c2d_fmt_tab* tab, const char* s, double* out) {
  return c2d_scan_e14_7_opt(tab, s, out, 0);
}

#endif /* C2D_SCAN_H */
