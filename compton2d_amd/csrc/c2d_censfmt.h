/*
 * c2d_censfmt.h — the integer line of a census record (write_cens,
 * src/census2d.f:21-28: (6e14.7) then (6i5)) and a whole record on the host.
 * One set of functions for the host (C99 under gcc) and the device (hipcc),
 * integer arithmetic only, so both give the same bytes; the E14.7 fields are
 * c2d_fmt.h's and c2d_scan.h's.
 *
 * Record: 84 bytes of six E14.7 fields, a newline, 30 bytes of six I5
 * fields, a newline: 116 bytes, no separators.
 *
 * I5 as Fortran writes it: the decimal digits right-justified in 5 columns,
 * a '-' before them for a negative value; a value that does not fit
 * (outside -9999..99999) is five asterisks.  A canonical field on the way
 * back is blanks, an optional '-', then at least one digit up to the last
 * column; everything else (asterisks among it) is not canonical.
 */
#ifndef C2D_CENSFMT_H
#define C2D_CENSFMT_H

#include "c2d_scan.h"

#define C2D_CENS_RECORD 116   /* bytes of a record                                  */
#define C2D_CENS_LINE2 85     /* offset of the integer line                         */
#define C2D_CENS_SEEDMOD 100000ull   /* the sixth integer is key mod 100000         */

/* the five bytes of I5(v), first column in the low byte */
C2D_FMT_HD uint64_t c2d_fmt_i5_pack(int64_t v) {
  if (v < -9999 || v > 99999) return 0x2a2a2a2a2aull;
  uint32_t a = (uint32_t)(v < 0 ? -v : v);
  uint64_t w = 0x2020202020ull;
  int p = 4;
  do {
    w ^= (uint64_t)((uint32_t)' ' ^ ((uint32_t)'0' + a % 10u)) << (8 * p);
    a /= 10u;
    p--;
  } while (a);
  if (v < 0) w ^= (uint64_t)((uint32_t)' ' ^ (uint32_t)'-') << (8 * p);   /* p >= 0: at most four digits */
  return w;
}

/* a canonical I5 field (low five bytes of w) to *out; 0, or -1 with nothing written */
C2D_FMT_HD int c2d_scan_i5_pack(uint64_t w, int32_t* out) {
  int32_t val = 0;
  int st = 0, neg = 0, ok = 1;   /* st 0: blanks, 1: after the sign, 2: digits */
  for (int i = 0; i < 5; i++) {
    const uint32_t c = (uint32_t)(w >> (8 * i)) & 0xffu;
    if (c == ' ') {
      ok &= st == 0;
    } else if (c == '-') {
      ok &= st == 0;
      st = 1;
      neg = 1;
    } else if (c >= '0' && c <= '9') {
      val = val * 10 + (int32_t)(c - '0');
      st = 2;
    } else {
      ok = 0;
    }
  }
  if (!ok || st != 2) return -1;
  *out = neg ? -val : val;
  return 0;
}

/* the lineage key of record `index` of a file that has only the 5-digit seed
 * (census_io.derive_key: splitmix64 of seed and index) */
C2D_FMT_HD uint64_t c2d_cens_derive_key(int64_t seed, int64_t index) {
  uint64_t z = (uint64_t)seed * 0x9E3779B97F4A7C15ull + (uint64_t)index + 0x5EEDC2Dull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

/* One record into out[116] on the host (the kernel of censtext.hip builds the
 * same bytes in LDS).  Returns C2D_FMT_NONFINITE, with out undefined, if one
 * of the doubles is NaN or Inf. */
static inline int c2d_cens_record(const c2d_fmt_tab* tab, const double* d6, const int32_t* i5, uint64_t key,
                                  char* out) {
  for (int f = 0; f < 6; f++)
    if (c2d_fmt_e14_7(tab, d6[f], out + 14 * f) < 0) return C2D_FMT_NONFINITE;
  out[84] = '\n';
  for (int f = 0; f < 6; f++) {
    const uint64_t w = c2d_fmt_i5_pack(f < 5 ? (int64_t)i5[f] : (int64_t)(key % C2D_CENS_SEEDMOD));
    for (int b = 0; b < 5; b++) out[C2D_CENS_LINE2 + 5 * f + b] = (char)(w >> (8 * b));
  }
  out[115] = '\n';
  return C2D_FMT_OK;
}

#endif /* C2D_CENSFMT_H */
