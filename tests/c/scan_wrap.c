/* Host harness of compton2d_amd/csrc/c2d_scan.h (C99, gcc): the E14.7 field
 * parser behind c2d_events_read, for tests/test_scan_host.py.  With
 * -DSCAN_WRAP_MAIN it is a stand-alone program over directed cases (the
 * build the test runs under -fsanitize=address,undefined). */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../compton2d_amd/csrc/c2d_scan.h"

static c2d_fmt_tab* g_tab;

static const c2d_fmt_tab* sw_tab(void) {
  if (!g_tab) {
    g_tab = (c2d_fmt_tab*)malloc(sizeof *g_tab);
    c2d_fmt_tab_build(g_tab);
  }
  return g_tab;
}

/* n fields of 14 bytes at text + 14 i -> out[i] (left as it was for a field
 * that is not canonical); status[i] = the parser's return.  force_exact:
 * every field through the multi-limb path.  Returns how many took it. */
int64_t sw_scan(const char* text, int64_t n, double* out, int8_t* status, int force_exact) {
  const c2d_fmt_tab* tab = sw_tab();
  int64_t exact = 0;
  for (int64_t i = 0; i < n; i++) {
    const int st = c2d_scan_e14_7_opt(tab, text + 14 * i, out + i, force_exact);
    if (status) status[i] = (int8_t)st;
    exact += st == C2D_SCAN_EXACT;
  }
  return exact;
}

#ifdef SCAN_WRAP_MAIN
/* field, strtod's value of its E-form */
static const struct { const char* s; const char* e; } CASES[] = {
  {" 0.0000000E+00", "0.0"}, {"-0.0000000E+00", "-0.0"}, {" 0.1000000+101", "0.1000000E+101"},
  {" 0.1000000E-99", "0.1000000E-99"}, {" 0.1000000E+21", "0.1E+21"}, {" 0.9999999E+00", "0.9999999"},
  {"-0.1234566E+07", "-0.1234566E+07"}, {" 0.4940656-323", "0.4940656E-323"},
  {" 0.1797693+309", "0.1797693E+309"}, {" 0.2225074-307", "0.2225074E-307"},
  {" 0.9999999+309", "0.9999999E+309"}, {"-0.3141593E+01", "-0.3141593E+01"},
  {" 0.7378699E+20", "0.7378699E+20"}, {" 0.0000001-300", "0.0000001E-300"},
  {" 0.0000001-323", "0.0000001E-323"}, {" 0.2470328-323", "0.2470328E-323"},
  {" 0.2470329-323", "0.2470329E-323"}, {" 0.0000001+316", "0.0000001E+316"},
  {" 0.1797694+309", "0.1797694E+309"}, {"-0.9999999-999", "-0.9999999E-999"},
  {" 0.9999999+999", "0.9999999E+999"}, {" 0.0012345E-05", "0.0012345E-05"},
};
static const char* const BAD[] = {
  "\t0.1234567E+01", "0.1234567E+01 ", " 1.2345678E+01", " 0.12a4567E+01", "           NaN", " 0.1234567E 01",
  " 0.1234567e+01", "  .1234567E+01", "+0.1234567E+01", " 0.1234567E+1x", " 0.1234567+1 2", " 0,1234567E+01",
};

int main(void) {
  const int n = (int)(sizeof CASES / sizeof CASES[0]), nb = (int)(sizeof BAD / sizeof BAD[0]);
  int fails = 0;
  for (int i = 0; i < n; i++) {
    const double want = strtod(CASES[i].e, NULL);
    double a = 12345.0, b = 12345.0;
    int8_t sa, sb;
    sw_scan(CASES[i].s, 1, &a, &sa, 0);
    sw_scan(CASES[i].s, 1, &b, &sb, 1);
    const int ok = sa >= 0 && sb >= 0 && memcmp(&a, &want, 8) == 0 && memcmp(&b, &want, 8) == 0;
    printf("[%s] %-24.17g %s%s\n", CASES[i].s, a, sa > 0 ? "exact " : "", ok ? "ok" : "MISMATCH");
    fails += !ok;
  }
  for (int i = 0; i < nb; i++) {
    double a = 12345.0;
    int8_t sa;
    sw_scan(BAD[i], 1, &a, &sa, 0);
    const int ok = sa == C2D_SCAN_NOTCANON && a == 12345.0;
    if (!ok) printf("[%s] taken as canonical: MISMATCH\n", BAD[i]);
    fails += !ok;
  }
  free(g_tab);
  g_tab = NULL;
  printf("%d cases, %d failures\n", n + nb, fails);
  return fails != 0;
}
#endif
