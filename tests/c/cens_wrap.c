/* Host harness of compton2d_amd/csrc/c2d_censfmt.h (C99, gcc): the I5
 * formatter and parser and the whole census record behind c2d_census_write /
 * c2d_census_read, for tests/test_census_fmt_host.py.  With -DCENS_WRAP_MAIN
 * it is a stand-alone program over the I5 range and a few records (the build
 * the test runs under -fsanitize=address,undefined). */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../compton2d_amd/csrc/c2d_censfmt.h"

static c2d_fmt_tab* g_tab;

static const c2d_fmt_tab* cw_tab(void) {
  if (!g_tab) {
    g_tab = (c2d_fmt_tab*)malloc(sizeof *g_tab);
    c2d_fmt_tab_build(g_tab);
  }
  return g_tab;
}

/* n integers -> 5 bytes each */
void cw_i5(const int64_t* v, int64_t n, char* out) {
  for (int64_t i = 0; i < n; i++) {
    const uint64_t w = c2d_fmt_i5_pack(v[i]);
    for (int b = 0; b < 5; b++) out[5 * i + b] = (char)(w >> (8 * b));
  }
}

/* n fields of 5 bytes -> integers (left as they were where status[i] = -1) */
void cw_scan_i5(const char* text, int64_t n, int32_t* out, int8_t* status) {
  for (int64_t i = 0; i < n; i++) {
    uint64_t w = 0;
    for (int b = 0; b < 5; b++) w |= (uint64_t)(unsigned char)text[5 * i + b] << (8 * b);
    status[i] = (int8_t)c2d_scan_i5_pack(w, &out[i]);
  }
}

uint64_t cw_derive_key(int64_t seed, int64_t index) { return c2d_cens_derive_key(seed, index); }

/* n records -> 116 bytes each; returns how many held a non-finite double */
int64_t cw_records(const double* d6, const int32_t* i5, const uint64_t* keys, int64_t n, char* out) {
  int64_t bad = 0;
  for (int64_t r = 0; r < n; r++)
    bad += c2d_cens_record(cw_tab(), d6 + 6 * r, i5 + 5 * r, keys[r], out + C2D_CENS_RECORD * r) < 0;
  return bad;
}

#ifdef CENS_WRAP_MAIN
int main(void) {
  int fails = 0;
  for (int64_t v = -10000; v <= 100000; v++) {
    char got[6] = {0}, want[16];
    int32_t back = 123456;
    int8_t st;
    cw_i5(&v, 1, got);
    snprintf(want, sizeof want, "%5lld", (long long)v);
    if (strlen(want) > 5) strcpy(want, "*****");
    cw_scan_i5(got, 1, &back, &st);
    const int ok = strcmp(got, want) == 0 && (want[0] == '*' ? st == -1 && back == 123456 : st == 0 && back == v);
    if (!ok && fails++ < 5) printf("%lld: [%s] want [%s] back %d status %d\n", (long long)v, got, want, back, st);
  }
  {
    const double d6[12] = {0.0, -0.0, 1e100, 1e-100, 1234567.5, -3.1415926536, 1.0, 2.0, 3.0, 4.0, 5.0, 1.0 / 0.0};
    const int32_t i5[10] = {0, 1, 9, 10, 99, 255, 99999, 100000, -9999, -10000};
    const uint64_t keys[2] = {12345678901234567ull, ~0ull};
    char out[2 * C2D_CENS_RECORD + 1] = {0};
    const char* want = " 0.0000000E+00-0.0000000E+00 0.1000000+101 0.1000000E-99 0.1234568E+07-0.3141593E+01\n"
                       "    0    1    9   10   9934567\n";
    if (cw_records(d6, i5, keys, 2, out) != 1 || memcmp(out, want, C2D_CENS_RECORD) != 0) {
      printf("record: MISMATCH [%.116s]\n", out);
      fails++;
    }
  }
  free(g_tab);
  g_tab = NULL;
  printf("%d failures\n", fails);
  return fails != 0;
}
#endif
