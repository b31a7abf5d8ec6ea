/*
 * c2d_fmt.h — Fortran E14.7 of a finite double, correctly rounded, for the
 * escape-event file (src/imcleak2d.f:171,181: 6(e14.7,1x),e14.7).  One
 * function for the host (C99 under gcc) and the device (hipcc); integer
 * arithmetic only, so both give the same 14 bytes.
 *
 * Layout: [-]0.dddddddE+xx right-justified in 14 bytes; a three-digit
 * exponent drops the E ([-]0.ddddddd+xxx); zero is 0.0000000E+00 with the
 * sign of the zero.  The exact binary value is rounded to 7 significant
 * digits, ties to even, with the carry into the next decade (AMD flang's
 * runtime and glibc's %.6e do the same).
 *
 * Algorithm.  x = m 2^e with m normalised to 64 bits.  For a
 * decimal shift q, 10^q = (T + t) 2^b with T a 128-bit integer in [2^127,
 * 2^128) from a table and 0 <= t < 1 (T is the truncation of the exact
 * power, built with exact integer arithmetic by c2d_fmt_tab_build).  The
 * 192-bit product P = m T therefore satisfies P <= m 10^q 2^-b < P + 2^64,
 * and x 10^q = (P + error) 2^-s with s >= 165.  The integer part of P 2^-s
 * is the 7-digit candidate D and the bits below are the discarded fraction.
 * If adding 2^64 to the fraction can neither carry into D nor cross 1/2, D
 * and the rounding direction are those of the exact value.  Otherwise (the
 * fraction's bits above 2^64 are all ones, or are those of 1/2 or of
 * 1/2 - 2^-(s-64)) the value is ambiguous.  Ambiguous values are first tested
 * for 2 x 10^q being an integer, exactly, by divisibility (5 is odd: the low
 * bits of m against the power of two, m against 5^-q by repeated division):
 * escapes sit on the grid's boundaries, so round values such as 1e16 are
 * common in the events, and every tie is of this kind.  If it is one, it is
 * the only integer in (P + [0, 2^64)) 2^(1-s), an interval shorter than 1:
 * the ceiling of P 2^(1-s).  Otherwise c2d_fmt_exact decides with multi-limb
 * integers (probability ~ 2^-100 per value).  The decimal exponent starts from an
 * integer estimate of floor(log10 x) and is corrected by the integer test
 * 10^6 <= D < 10^7; no double arithmetic takes part.
 */
#ifndef C2D_FMT_H
#define C2D_FMT_H

#include <stdint.h>

#if defined(__HIPCC__)
#define C2D_FMT_HD __host__ __device__ __forceinline__
#define C2D_FMT_SLOW static __host__ __device__ __attribute__((noinline))
#else
#define C2D_FMT_HD static inline
#define C2D_FMT_SLOW static __attribute__((noinline, unused))
#endif
/* the exact path's loops stay rolled on the device: unrolled, its 40-limb
 * integers would live in registers and set the whole kernel's register count */
#if defined(__clang__)
#define C2D_FMT_ROLLED _Pragma("unroll 1")
#else
#define C2D_FMT_ROLLED
#endif

/* decimal shifts the table covers: x 10^q in [10^5, 10^8) for every finite
 * double (q = 6 - floor(log10 x), one more either way for the estimate) */
#define C2D_FMT_QMIN (-304)
#define C2D_FMT_QMAX 331
#define C2D_FMT_NQ (C2D_FMT_QMAX - C2D_FMT_QMIN + 1)
/* 32-bit limbs of the exact path's integers (the largest is below 2^1140) */
#define C2D_FMT_LIMBS 40

/* status of c2d_fmt_e14_7_pack / c2d_fmt_e14_7 */
#define C2D_FMT_OK 0
#define C2D_FMT_EXACTINT 1      /* ambiguous; twice its scaled value is an integer (ties, round values) */
#define C2D_FMT_MULTILIMB 2     /* ambiguous; decided by c2d_fmt_exact */
#define C2D_FMT_NONFINITE (-1)  /* NaN or Inf: nothing written */

typedef struct c2d_fmt_tab {
  uint64_t hi[C2D_FMT_NQ], lo[C2D_FMT_NQ];   /* T = hi 2^64 + lo             */
  int16_t b[C2D_FMT_NQ];                     /* 10^q = (T + t) 2^b, 0 <= t < 1 */
} c2d_fmt_tab;

typedef struct c2d_fmt_big {
  uint32_t w[C2D_FMT_LIMBS];   /* little-endian */
} c2d_fmt_big;

C2D_FMT_HD void c2d_fmt_big_set(c2d_fmt_big* a, uint64_t v) {
  C2D_FMT_ROLLED
  for (int i = 0; i < C2D_FMT_LIMBS; i++) a->w[i] = 0;
  a->w[0] = (uint32_t)v;
  a->w[1] = (uint32_t)(v >> 32);
}
C2D_FMT_HD void c2d_fmt_big_mul(c2d_fmt_big* a, uint32_t f) {
  uint64_t carry = 0;
  C2D_FMT_ROLLED
  for (int i = 0; i < C2D_FMT_LIMBS; i++) {
    const uint64_t p = (uint64_t)a->w[i] * f + carry;
    a->w[i] = (uint32_t)p;
    carry = p >> 32;
  }
}
/* a <<= sh, 0 <= sh < 32 * C2D_FMT_LIMBS (bits shifted out are zero by the
 * size bounds above) */
C2D_FMT_HD void c2d_fmt_big_shl(c2d_fmt_big* a, int sh) {
  const int ws = sh >> 5, bs = sh & 31;
  C2D_FMT_ROLLED
  for (int i = C2D_FMT_LIMBS - 1; i >= 0; i--) {
    uint32_t v = 0;
    if (i - ws >= 0) {
      v = a->w[i - ws] << bs;
      if (bs && i - ws - 1 >= 0) v |= a->w[i - ws - 1] >> (32 - bs);
    }
    a->w[i] = v;
  }
}
C2D_FMT_HD int c2d_fmt_big_cmp(const c2d_fmt_big* a, const c2d_fmt_big* b) {
  C2D_FMT_ROLLED
  for (int i = C2D_FMT_LIMBS - 1; i >= 0; i--)
    if (a->w[i] != b->w[i]) return a->w[i] < b->w[i] ? -1 : 1;
  return 0;
}
/* a = 5^n */
C2D_FMT_HD void c2d_fmt_big_pow5(c2d_fmt_big* a, int n) {
  c2d_fmt_big_set(a, 1);
  C2D_FMT_ROLLED
  for (; n >= 13; n -= 13) c2d_fmt_big_mul(a, 1220703125u);   /* 5^13 */
  uint32_t f = 1;
  C2D_FMT_ROLLED
  for (; n > 0; n--) f *= 5u;
  c2d_fmt_big_mul(a, f);
}
/* bit i of a (0 beyond the top) */
C2D_FMT_HD uint32_t c2d_fmt_big_bit(const c2d_fmt_big* a, int i) {
  return i < 32 * C2D_FMT_LIMBS ? (a->w[i >> 5] >> (i & 31)) & 1u : 0u;
}

/* Exact path: V = m 2^e 10^q (m < 2^53, m != 0, V < 2^27) as *D = floor(V)
 * and *r = the discarded fraction against 1/2 (0 below, 1 equal, 2 above). */
C2D_FMT_SLOW void c2d_fmt_exact(uint64_t m, int e, int q, uint32_t* D, int* r) {
  c2d_fmt_big A, B, C;
  const int t = e + q;   /* V = m 5^q 2^t */
  if (q >= 0) {
    c2d_fmt_big_pow5(&A, q);
    c2d_fmt_big_mul(&A, (uint32_t)m);   /* A = 5^q m, in two steps: m has 53 bits */
    {
      c2d_fmt_big_pow5(&B, q);
      c2d_fmt_big_mul(&B, (uint32_t)(m >> 32));
      c2d_fmt_big_shl(&B, 32);
      uint64_t carry = 0;
      C2D_FMT_ROLLED
      for (int i = 0; i < C2D_FMT_LIMBS; i++) {
        const uint64_t s = (uint64_t)A.w[i] + B.w[i] + carry;
        A.w[i] = (uint32_t)s;
        carry = s >> 32;
      }
    }
    if (t >= 0) {
      c2d_fmt_big_shl(&A, t);
      *D = A.w[0];
      *r = 0;
      return;
    }
    const int sh = -t;
    uint32_t d = 0;
    C2D_FMT_ROLLED
    for (int i = 31; i >= 0; i--) d = (d << 1) | c2d_fmt_big_bit(&A, sh + i);
    int sticky = 0;
    C2D_FMT_ROLLED
    for (int i = 0; i < sh - 1 && i < 32 * C2D_FMT_LIMBS; i++) sticky |= (int)c2d_fmt_big_bit(&A, i);
    *D = d;
    *r = c2d_fmt_big_bit(&A, sh - 1) ? (sticky ? 2 : 1) : 0;
    return;
  }
  /* V = N / Q with N = m 2^max(t,0), Q = 5^-q 2^max(-t,0) */
  c2d_fmt_big_set(&A, m);
  c2d_fmt_big_pow5(&B, -q);
  if (t >= 0) c2d_fmt_big_shl(&A, t); else c2d_fmt_big_shl(&B, -t);
  uint32_t d = 0;
  C2D_FMT_ROLLED
  for (int bit = 26; bit >= 0; bit--) {   /* the largest d with Q d <= N */
    const uint32_t tr = d | (1u << bit);
    C = B;
    c2d_fmt_big_mul(&C, tr);
    if (c2d_fmt_big_cmp(&C, &A) <= 0) d = tr;
  }
  /* the remainder against Q / 2: 2 N against Q (2 d + 1) */
  c2d_fmt_big_shl(&A, 1);
  C = B;
  c2d_fmt_big_mul(&C, 2u * d + 1u);
  const int cmp = c2d_fmt_big_cmp(&A, &C);
  *D = d;
  *r = cmp < 0 ? 0 : (cmp == 0 ? 1 : 2);
}

/* Fast path: the candidate digits and rounding class of m64 2^e64 10^q
 * (m64 normalised: bit 63 set); returns 1 if they are ambiguous.  *Y =
 * ceil(P 2^(1-s)): twice the scaled value if that is an integer. */
C2D_FMT_HD int c2d_fmt_fast(const c2d_fmt_tab* tab, uint64_t m64, int e64, int q, uint32_t* D, int* r, uint32_t* Y) {
  const int idx = q - C2D_FMT_QMIN;
  const unsigned __int128 a = (unsigned __int128)m64 * tab->hi[idx];
  const unsigned __int128 c = (unsigned __int128)m64 * tab->lo[idx];
  const uint64_t a_lo = (uint64_t)a, c_hi = (uint64_t)(c >> 64);
  const uint64_t mid = a_lo + c_hi;
  const uint64_t top = (uint64_t)(a >> 64) + (mid < a_lo ? 1u : 0u);
  /* x 10^q = (top 2^128 + mid 2^64 + low + error) 2^-s, 0 <= error < 2^64 */
  const int s = -(e64 + (int)tab->b[idx]);
  const int sh = s - 128;   /* 37..48 while 2^16 < x 10^q < 2^27 */
  const uint64_t ones = ((uint64_t)1 << sh) - 1u;
  const uint64_t f_top = top & ones;
  *D = (uint32_t)(top >> sh);
  const uint64_t half = (uint64_t)1 << (sh - 1);
  *r = (f_top & half) ? 2 : 0;
  *Y = (uint32_t)(top >> (sh - 1)) + (((top & (half - 1u)) | mid | (uint64_t)c) != 0 ? 1u : 0u);
  return (f_top == ones && mid == ~(uint64_t)0) || (f_top == (ones >> 1) && mid == ~(uint64_t)0) ||
         (f_top == half && mid == 0);
}

/* Is 2 m 2^e 10^q = m 5^q 2^(e+q+1) an integer?  Exact. */
C2D_FMT_HD int c2d_fmt_twice_is_integer(uint64_t m, int e, int q) {
  const int t1 = e + q + 1;
  if (t1 < 0 && (-t1 > 63 || (m & (((uint64_t)1 << -t1) - 1u)) != 0)) return 0;
  C2D_FMT_ROLLED
  for (int n = -q; n > 0; n--) {   /* 5^-q | m (at most 22 times: m < 2^53) */
    if (m % 5u) return 0;
    m /= 5u;
  }
  return 1;
}

/* 14 bytes of E14.7 as two little-endian words (w0: bytes 0-7, w1: bytes
 * 8-13).  Returns C2D_FMT_OK, C2D_FMT_EXACTINT, C2D_FMT_MULTILIMB or
 * C2D_FMT_NONFINITE (the words are then untouched).  shortcut = 0 sends
 * every ambiguous value to c2d_fmt_exact (tests of that path). */
C2D_FMT_HD int c2d_fmt_e14_7_pack_opt(const c2d_fmt_tab* tab, double x, uint64_t* w0, uint64_t* w1, int shortcut) {
  uint64_t u;
  __builtin_memcpy(&u, &x, sizeof u);
  const uint64_t sign = u >> 63;
  const int bexp = (int)((u >> 52) & 0x7ff);
  uint64_t m = u & 0x000fffffffffffffull;
  if (bexp == 0x7ff) return C2D_FMT_NONFINITE;
  uint32_t D = 0;
  int X = 0, status = C2D_FMT_OK;
  if (bexp != 0 || m != 0) {
    int e;
    if (bexp) { m |= (uint64_t)1 << 52; e = bexp - 1075; } else e = -1074;
    const int lz = __builtin_clzll(m);
    const uint64_t m64 = m << lz;
    const int e64 = e - lz;
    /* floor(log10 x) or one less: floor(E2 log10 2), E2 = floor(log2 x) */
    const int E2 = e64 + 63;
    int k = (int)(((int64_t)E2 * 78913 + ((int64_t)400 << 18)) >> 18) - 400;
    int r = 0;
    for (;;) {
      const int q = 6 - k;
      uint32_t Y;
      if (c2d_fmt_fast(tab, m64, e64, q, &D, &r, &Y)) {
        if (shortcut && c2d_fmt_twice_is_integer(m, e, q)) {
          D = Y >> 1;
          r = (int)(Y & 1u);
          if (status < C2D_FMT_EXACTINT) status = C2D_FMT_EXACTINT;
        } else {
          c2d_fmt_exact(m, e, q, &D, &r);
          status = C2D_FMT_MULTILIMB;
        }
      }
      if (D >= 10000000u) k++;
      else if (D < 1000000u) k--;
      else break;
    }
    if (r == 2 || (r == 1 && (D & 1u))) {
      D++;
      if (D == 10000000u) { D = 1000000u; k++; }
    }
    X = k + 1;   /* 0.ddddddd x 10^X */
  }
  uint64_t dg = 0;   /* bytes 3..9 hold the digits, most significant first */
  for (int i = 0; i < 7; i++) {
    const uint32_t qd = D / 10u;
    dg = (dg << 8) | (uint64_t)('0' + (D - 10u * qd));
    D = qd;
  }
  const uint32_t ax = (uint32_t)(X < 0 ? -X : X);
  const uint64_t xs = X < 0 ? '-' : '+';
  uint64_t ex;   /* bytes 10..13 */
  if (ax < 100u) ex = 'E' | xs << 8 | (uint64_t)('0' + ax / 10u) << 16 | (uint64_t)('0' + ax % 10u) << 24;
  else ex = xs | (uint64_t)('0' + ax / 100u) << 8 | (uint64_t)('0' + ax / 10u % 10u) << 16 |
            (uint64_t)('0' + ax % 10u) << 24;
  /* dg's lowest byte is the first digit (the loop pushed the last one in first) */
  *w0 = (sign ? '-' : ' ') | (uint64_t)'0' << 8 | (uint64_t)'.' << 16 | (dg & 0xffffffffffull) << 24;
  *w1 = (dg >> 40) | ex << 16;
  return status;
}

C2D_FMT_HD int c2d_fmt_e14_7_pack(const c2d_fmt_tab* tab, double x, uint64_t* w0, uint64_t* w1) {
  return c2d_fmt_e14_7_pack_opt(tab, x, w0, w1, 1);
}

/* The same into 14 bytes at out. */
C2D_FMT_HD int c2d_fmt_e14_7(const c2d_fmt_tab* tab, double x, char* out) {
  uint64_t w0, w1;
  const int st = c2d_fmt_e14_7_pack(tab, x, &w0, &w1);
  if (st < 0) return st;
  for (int i = 0; i < 8; i++) out[i] = (char)(w0 >> (8 * i));
  for (int i = 0; i < 6; i++) out[8 + i] = (char)(w1 >> (8 * i));
  return st;
}

/* Build the table (host, exact integer arithmetic): for q >= 0 the top 128
 * bits of 10^q = 5^q 2^q; for q < 0 floor(2^p / 10^-q) with p = 127 +
 * bitlength(10^-q), by repeated floor division (floor(floor(a/u)/v) =
 * floor(a/(u v))).  Either way T <= 10^q 2^-b < T + 1. */
static inline int c2d_fmt_big_bitlen(const c2d_fmt_big* a) {
  for (int i = C2D_FMT_LIMBS - 1; i >= 0; i--)
    if (a->w[i]) return 32 * i + 32 - __builtin_clz(a->w[i]);
  return 0;
}
static inline void c2d_fmt_big_div(c2d_fmt_big* a, uint32_t d) {
  uint64_t rem = 0;
  for (int i = C2D_FMT_LIMBS - 1; i >= 0; i--) {
    const uint64_t cur = (rem << 32) | a->w[i];
    a->w[i] = (uint32_t)(cur / d);
    rem = cur % d;
  }
}
static inline uint64_t c2d_fmt_big_bits64(const c2d_fmt_big* a, int lo) {
  uint64_t v = 0;
  for (int i = 63; i >= 0; i--) v = (v << 1) | (lo + i >= 0 ? c2d_fmt_big_bit(a, lo + i) : 0u);
  return v;
}
static inline void c2d_fmt_tab_build(c2d_fmt_tab* tab) {
  for (int q = C2D_FMT_QMIN; q <= C2D_FMT_QMAX; q++) {
    const int idx = q - C2D_FMT_QMIN;
    c2d_fmt_big A;
    int b;
    if (q >= 0) {
      c2d_fmt_big_pow5(&A, q);
      const int L = c2d_fmt_big_bitlen(&A);   /* 10^q = A 2^q */
      tab->hi[idx] = c2d_fmt_big_bits64(&A, L - 64);
      tab->lo[idx] = c2d_fmt_big_bits64(&A, L - 128);
      b = L - 128 + q;
    } else {
      const int n = -q;
      c2d_fmt_big_pow5(&A, n);
      const int L = c2d_fmt_big_bitlen(&A) + n;   /* bitlength(10^n) */
      const int p = 127 + L;
      c2d_fmt_big_set(&A, 1);
      c2d_fmt_big_shl(&A, p);
      int left = n;
      for (; left >= 9; left -= 9) c2d_fmt_big_div(&A, 1000000000u);
      for (; left > 0; left--) c2d_fmt_big_div(&A, 10u);
      tab->hi[idx] = c2d_fmt_big_bits64(&A, 64);
      tab->lo[idx] = c2d_fmt_big_bits64(&A, 0);
      b = -p;
    }
    tab->b[idx] = (int16_t)b;
  }
}

#endif /* C2D_FMT_H */
