/* Host harness of compton2d_amd/csrc/c2d_fmt.h (C99, gcc): the E14.7
 * formatter behind c2d_events_write, for tests/test_fmt_host.py.  With
 * -DFMT_WRAP_MAIN it is a stand-alone program over the directed cases (the
 * build the test runs under -fsanitize=address,undefined). */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../compton2d_amd/csrc/c2d_fmt.h"

static c2d_fmt_tab* g_tab;

static const c2d_fmt_tab* fw_tab(void) {
  if (!g_tab) {
    g_tab = (c2d_fmt_tab*)malloc(sizeof *g_tab);
    c2d_fmt_tab_build(g_tab);
  }
  return g_tab;
}

int64_t fw_tab_bytes(void) { return (int64_t)sizeof(c2d_fmt_tab); }

/* n doubles -> 14 bytes each at out + 14 i (left as they were for a
 * non-finite value); status[i] = the formatter's return.  Returns how many
 * left the fast path (ambiguous values); *n_bad = how many were non-finite. */
static int64_t fw_format_opt(const double* x, int64_t n, char* out, int8_t* status, int64_t* n_bad, int shortcut) {
  const c2d_fmt_tab* tab = fw_tab();
  int64_t slow = 0, bad = 0;
  for (int64_t i = 0; i < n; i++) {
    uint64_t w0, w1;
    const int st = c2d_fmt_e14_7_pack_opt(tab, x[i], &w0, &w1, shortcut);
    if (status) status[i] = (int8_t)st;
    slow += st > 0;
    bad += st == C2D_FMT_NONFINITE;
    if (st < 0) continue;
    memcpy(out + 14 * i, &w0, 8);   /* little-endian host */
    memcpy(out + 14 * i + 8, &w1, 6);
  }
  if (n_bad) *n_bad = bad;
  return slow;
}
int64_t fw_format(const double* x, int64_t n, char* out, int8_t* status, int64_t* n_bad) {
  return fw_format_opt(x, n, out, status, n_bad, 1);
}
/* every ambiguous value through the multi-limb path */
int64_t fw_format_multilimb(const double* x, int64_t n, char* out, int8_t* status, int64_t* n_bad) {
  return fw_format_opt(x, n, out, status, n_bad, 0);
}

/* the exact path alone (whatever the fast path would say): D and the
 * rounding class of m 2^e 10^q */
void fw_exact(uint64_t m, int e, int q, uint32_t* D, int* r) { c2d_fmt_exact(m, e, q, D, r); }

/* glibc's route, the baseline of tools/evtext_bench.py: snprintf("%.6e") re-laid as E14.7 */
void fw_format_glibc(const double* x, int64_t n, char* out) {
  for (int64_t i = 0; i < n; i++) {
    char b[32], *o = out + 14 * i;
    const double v = x[i];
    snprintf(b, sizeof b, "%.6e", __builtin_fabs(v));
    int ex = atoi(b + 9) + 1;
    if (v == 0) ex = 0;
    o[0] = (v < 0 || (v == 0 && 1 / v < 0)) ? '-' : ' ';
    o[1] = '0';
    o[2] = '.';
    o[3] = b[0];
    memcpy(o + 4, b + 2, 6);
    char xb[16];
    if (abs(ex) < 100) snprintf(xb, sizeof xb, "E%+03d", ex); else snprintf(xb, sizeof xb, "%+04d", ex);
    memcpy(o + 10, xb, 4);
  }
}

#ifdef FMT_WRAP_MAIN
/* the directed cases: AMD flang's E14.7 of each value */
static const struct { double x; const char* s; } CASES[] = {
  {0.0, " 0.0000000E+00"}, {-0.0, "-0.0000000E+00"}, {1e100, " 0.1000000+101"},
  {1e-100, " 0.1000000E-99"}, {1e20, " 0.1000000E+21"}, {0.99999995, " 0.9999999E+00"},
  {1234567.5, " 0.1234568E+07"}, {1234566.5, " 0.1234566E+07"}, {-1234566.5, "-0.1234566E+07"},
  {4.9e-324, " 0.4940656-323"}, {1.7976931348623157e308, " 0.1797693+309"},
  {2.2250738585072014e-308, " 0.2225074-307"}, {-3.1415926536, "-0.3141593E+01"},
  {9.9999995e-100, " 0.9999999E-99"}, {0.12345675, " 0.1234568E+00"}, {99999995.0, " 0.1000000E+09"},
  {99999985.0, " 0.9999998E+08"}, {9.9999995e22, " 0.1000000E+24"},
};

int main(void) {
  const int n = (int)(sizeof CASES / sizeof CASES[0]);
  int fails = 0;
  for (int i = 0; i < n; i++) {
    char o[15] = {0}, g[15] = {0};
    int8_t st;
    char ml[15] = {0}, byt[15] = {0};
    fw_format(&CASES[i].x, 1, o, &st, NULL);
    fw_format_multilimb(&CASES[i].x, 1, ml, NULL, NULL);
    fw_format_glibc(&CASES[i].x, 1, g);
    c2d_fmt_e14_7(fw_tab(), CASES[i].x, byt);
    const int ok = memcmp(o, CASES[i].s, 14) == 0 && memcmp(g, CASES[i].s, 14) == 0 &&
                   memcmp(ml, CASES[i].s, 14) == 0 && memcmp(byt, CASES[i].s, 14) == 0;
    printf("%-24.17g [%s] glibc [%s] %s%s\n", CASES[i].x, o, g, st > 0 ? "ambiguous " : "",
           ok ? "ok" : "MISMATCH");
    fails += !ok;
  }
  {
    const double inf = 1.0 / 0.0;
    char o[15] = "untouched.....";
    int64_t bad = 0;
    fw_format(&inf, 1, o, NULL, &bad);
    if (bad != 1 || strcmp(o, "untouched.....") != 0) { printf("non-finite: MISMATCH\n"); fails++; }
  }
  free(g_tab);
  g_tab = NULL;
  printf("%d cases, %d failures\n", n, fails);
  return fails != 0;
}
#endif
