/*
 * comb_edge.c — csrc/c2d_comb.h on its edge values, as plain C with its own
 * main: meant to be built with the host sanitizers and run once,
 *
 *   cc -std=c11 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
 *      -ffp-contract=off -Wno-unknown-pragmas -I compton2d_amd/csrc tools/comb_edge.c -lm -o comb_edge && ./comb_edge
 *
 * It checks, for weights from the smallest subnormal to DBL_MAX and draws from
 * 2^-64 to 1, that w* is the last floor survived (S(w*) and !S(next above)),
 * the special cases of the rule (ew = 0, an infinite quotient, an exact
 * quotient, u = 1), the power-of-two test, `fixed`, and that the six digits
 * put a value's 64 bits together again.  Exit status 0 and "ok" on success.
 */
#include <float.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "c2d_comb.h"

static int failures = 0;
#define CHECK(x)                                                   \
  do {                                                             \
    if (!(x)) {                                                    \
      printf("FAILED line %d: %s\n", __LINE__, #x);                \
      failures++;                                                  \
    }                                                              \
  } while (0)

static void check_wstar(double ew, double u) {
  const double w = c2d_comb_wstar(ew, u);
  if (ew == 0.0) {
    CHECK(w == 0.0 && !signbit(w));
    return;
  }
  CHECK(c2d_comb_finite(w) && w >= 0.0);
  if (u < 1.0) {   /* u = 1 (one draw in 2^53): S(ew) fails, w* lies below ew or the search gives up */
    CHECK(w > 0.0);
    CHECK(c2d_comb_survives(ew, u, w));
    CHECK(!c2d_comb_survives(ew, u, nextafter(w, INFINITY)));
    CHECK(w >= ew);   /* ew >= floor implies survival */
  }
}

int main(void) {
  const double ews[] = {0.0, -0.0, 4.9406564584124654e-324, 1e-320, DBL_MIN, 1e-300, 1e-17, 0.1, 1.0, 3.0, 1e17,
                        1e300, DBL_MAX / 2, DBL_MAX};
  const double us[] = {0x1p-64, 0x1.8p-54, 0x1p-53, 1e-9, 0.1, 1.0 / 3.0, 0.5, 0.75, 1.0 - 0x1p-53, 1.0};
  for (size_t i = 0; i < sizeof ews / sizeof *ews; i++)
    for (size_t j = 0; j < sizeof us / sizeof *us; j++) check_wstar(ews[i], us[j]);
  /* the uniforms the roulette really draws, through the whole chain */
  for (uint64_t key = 1; key < 20000; key += 7) {
    const uint64_t K = c2d_derive(key * 0x9E3779B97F4A7C15ull, C2D_TAG_ROULETTE, 5u, 0u);
    const double u = c2d_draw(K, 0u);
    CHECK(u > 0.0 && u <= 1.0);
    check_wstar(ldexp(1.0 + (double)(key % 1000) / 1000.0, (int)(key % 200) - 100), u);
    check_wstar(u * 8.0, u);   /* ew / u = 8 exactly: S(8) is u < u */
    CHECK(c2d_comb_wstar(u * 8.0, u) == nextafter(8.0, 0.0));
    const double c = c2d_comb_critical(3.0, 0x1p-7, key, 5);
    CHECK(c == c2d_comb_wstar(3.0, c2d_draw(c2d_derive(key, C2D_TAG_ROULETTE, 5u, 0u), 0u)) * 128.0);
  }
  CHECK(c2d_comb_wstar(1e300, 0x1p-64) == DBL_MAX);   /* the quotient is infinite */
  CHECK(c2d_comb_wstar(DBL_MAX, 0.5) == DBL_MAX);
  CHECK(c2d_comb_wstar(1.0, 1.0) < 1.0);

  CHECK(c2d_comb_pow2(1.0) && c2d_comb_pow2(0x1p-1074) && c2d_comb_pow2(0x1p-1022) && c2d_comb_pow2(0x1p1023));
  CHECK(!c2d_comb_pow2(0.0) && !c2d_comb_pow2(-2.0) && !c2d_comb_pow2(3.0) && !c2d_comb_pow2(INFINITY));
  CHECK(!c2d_comb_pow2(NAN) && !c2d_comb_pow2(0x1p-1074 * 3) && !c2d_comb_pow2(1.0 + DBL_EPSILON));

  CHECK(!c2d_comb_fixed(1.0, 2.0, 1) && !c2d_comb_fixed(0.0, 2.0, 1));
  CHECK(c2d_comb_fixed(1.0, 2.0, 0) && c2d_comb_fixed(1.0, 0.0, 1) && c2d_comb_fixed(1.0, -2.0, 1));
  CHECK(c2d_comb_fixed(1.0, INFINITY, 1) && c2d_comb_fixed(1.0, NAN, 1));
  CHECK(c2d_comb_fixed(-1.0, 2.0, 1) && c2d_comb_fixed(NAN, 2.0, 1) && c2d_comb_fixed(INFINITY, 2.0, 1));

  const uint64_t vals[] = {0ull, 1ull, 0x7fefffffffffffffull, 0x7ff0000000000000ull, 0x3ff123456789abcdull,
                           0xffffffffffffffffull};
  for (size_t i = 0; i < sizeof vals / sizeof *vals; i++) {
    uint64_t prefix = 0;
    for (int pb = 0; pb <= C2D_COMB_LAST_PREFIX; pb += C2D_COMB_DIGIT_BITS) {
      CHECK(c2d_comb_prefix_ok(prefix, pb) && c2d_comb_match(vals[i], prefix, pb));
      CHECK(!c2d_comb_match(vals[i] ^ (1ull << 63), prefix, pb) || pb == 0);
      const uint32_t d = c2d_comb_digit(vals[i], pb);
      CHECK(d < (pb == C2D_COMB_LAST_PREFIX ? 512u : (uint32_t)C2D_COMB_BINS));
      prefix = (prefix << (pb == C2D_COMB_LAST_PREFIX ? 9 : C2D_COMB_DIGIT_BITS)) | d;
    }
    CHECK(prefix == vals[i]);
  }
  CHECK(!c2d_comb_prefix_ok(0, 7) && !c2d_comb_prefix_ok(0, 66) && !c2d_comb_prefix_ok(0, -11));
  CHECK(!c2d_comb_prefix_ok(1, 0) && !c2d_comb_prefix_ok(1ull << 11, 11) && c2d_comb_prefix_ok(0x7ff, 11));

  if (failures) return 1;
  printf("ok\n");
  return 0;
}
