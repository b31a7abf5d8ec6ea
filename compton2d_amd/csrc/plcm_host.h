/* The light-curve tool's input dialogue and output files, on the host
 * (postprocessing/plcm.c:97-302 and :466-552), for c2d_obs_set_add_plcm /
 * c2d_obs_set_write: the counterpart of pspt_host.h, so that a C or Fortran
 * host gets plcm's files from the device histogram without event text.
 *
 * A restatement of compton2d_amd/observer.py (parse_plcm_deck, lc_binning,
 * lc_moments, write_lc, aux_name, particles_name) in the same operation
 * order, so edges and files equal the Python's bit for bit and byte for
 * byte (tests/test_plcm_host.py): chained t0[k+1] = t0[k] + dt, chained
 * E0 * dE, and sqrt(F2 - F1*F1) without a fused multiply-add (contraction
 * is switched off inside the functions below; obs_api.cpp is built with
 * -ffp-contract=off as well).
 *
 * Header-only C99 that also compiles as C++ (obs_api.cpp); no device code. */
#ifndef C2D_PLCM_HOST_H
#define C2D_PLCM_HOST_H

#include "pspt_host.h"

#define C2D_PLCM_STMAX 1024  /* plcm.c:6 st_max */
#define C2D_PLCM_MUMAX 10    /* plcm.c:7 mu_max */
#define C2D_PLCM_CHMAX 20    /* plcm.c:8 ch_max */

typedef struct c2d_plcm_deck {
  char infile[64];
  char names[C2D_PLCM_MUMAX][64];  /* the lc file of each angular bin */
  double gam_bulk, rmax, dt, t_offset, t_max;
  int n_t, n_mu, n_e;
  double t0[C2D_PLCM_STMAX], t1[C2D_PLCM_STMAX];
  double mu0[C2D_PLCM_MUMAX], mu1[C2D_PLCM_MUMAX];
  double E0[C2D_PLCM_CHMAX], E1[C2D_PLCM_CHMAX];
} c2d_plcm_deck;

/* dst = s[i:j] with Python's slice rules (negative bounds count from the end) */
static void c2d_plcm_slice(char* dst, int cap, const char* s, int i, int j) {
  const int n = (int)strlen(s);
  int k = 0;
  if (i < 0) i += n;
  if (j < 0) j += n;
  if (i < 0) i = 0;
  if (j > n) j = n;
  for (; i < j && k < cap - 1; i++) dst[k++] = s[i];
  dst[k] = '\0';
}

/* dst += s, truncated to cap - 1 characters in all */
static void c2d_plcm_cat(char* dst, int cap, const char* s) {
  int n = (int)strlen(dst);
  while (*s && n < cap - 1) dst[n++] = *s++;
  dst[n] = '\0';
}

/* stem + tail: '<name without .ext><tail>' (plcm.c:139-144) */
static void c2d_plcm_stem(char* dst, int cap, const char* name, const char* tail) {
  c2d_plcm_slice(dst, cap, name, 0, (int)strlen(name) - 4);
  c2d_plcm_cat(dst, cap, tail);
}

/* plcm.c:97-302 over `text` (one answer a line, e.g.
 * postprocessing/mrk421_lc.input; "" = every default).  0, or -1 when there
 * is no angular bin, a region has no bin, or the bands exceed ch_max. */
static int c2d_plcm_parse(const char* text, c2d_plcm_deck* d) {
#pragma STDC FP_CONTRACT OFF
  static const double dflt_reg[7][2] = {{1e-3, 3e-3}, {2., 4.}, {9., 15.}, {15., 20.},
                                        {20., 60.}, {5e5, 5e7}, {1e9, 1e10}};   /* plcm.c:251-266 */
  const char* p = text ? text : "";
  char a[256], name0[64], b[64], c[64], dig[2] = {0, 0};
  const int ncap = (int)sizeof name0 - 8;          /* room for ".dat" and the writer's suffixes */
  int reg, k, n, regions, n_r = 1;
  double lo = 0.99944, hi = 0.99964, E_lower = 1e-3, E_upper = 3e-3, dE, e;
  memset(d, 0, sizeof *d);
  strcpy(d->infile, "p001_evb.dat");
  if (c2d_pspt_line(&p, a, (int)sizeof a)) {
    if (a[0] >= '0' && a[0] <= '9') {              /* p0 + the digits given */
      d->infile[2] = '\0';
      c2d_plcm_cat(d->infile, ncap, a);
    } else {
      d->infile[0] = '\0';
      c2d_plcm_cat(d->infile, ncap, a);
    }
    c2d_pspt_add_dat(d->infile, (int)sizeof d->infile);
  }
  d->gam_bulk = c2d_pspt_d(&p, 33.);
  d->rmax = c2d_pspt_d(&p, 1.e16);
  /* the default output name from the input's: p001_evb.dat -> lc07_ev0.dat */
  n = (int)strlen(d->infile);
  c2d_plcm_slice(b, (int)sizeof b, d->infile, 4, n - 5);
  c2d_plcm_slice(c, (int)sizeof c, d->infile, n - 4, n);
  dig[0] = d->infile[2];
  strcpy(name0, "lc");
  c2d_plcm_cat(name0, ncap, dig);
  c2d_plcm_cat(name0, ncap, "7");
  c2d_plcm_cat(name0, ncap, b);
  c2d_plcm_cat(name0, ncap, "0");
  c2d_plcm_cat(name0, ncap, c);
  if (c2d_pspt_line(&p, a, (int)sizeof a)) {
    name0[0] = '\0';
    c2d_plcm_cat(name0, ncap, a);
  }
  c2d_pspt_add_dat(name0, (int)sizeof name0);
  d->n_mu = c2d_pspt_i(&p, 1);
  if (d->n_mu > C2D_PLCM_MUMAX) d->n_mu = C2D_PLCM_MUMAX;
  if (d->n_mu < 1) return -1;
  for (k = 0; k < d->n_mu; k++) {                  /* plcm.c:175-215 */
    n = (int)strlen(name0);
    if (c2d_pspt_line(&p, a, (int)sizeof a)) {
      c2d_plcm_cat(d->names[k], ncap, a);
    } else if (k == 0) {
      strcpy(d->names[k], name0);
    } else {                                       /* the digit before the extension */
      c2d_plcm_slice(b, (int)sizeof b, name0, 0, n - 5);
      c2d_plcm_slice(c, (int)sizeof c, name0, n - 4, n);
      dig[0] = (char)(48 + k);
      c2d_plcm_cat(d->names[k], ncap, b);
      c2d_plcm_cat(d->names[k], ncap, dig);
      c2d_plcm_cat(d->names[k], ncap, c);
    }
    c2d_pspt_add_dat(d->names[k], (int)sizeof d->names[k]);
    lo = c2d_pspt_d(&p, lo);
    hi = c2d_pspt_d(&p, hi);
    d->mu0[k] = lo;
    d->mu1[k] = hi;
    lo = hi;                                       /* the next bin starts where this one ends */
  }
  d->dt = c2d_pspt_d(&p, 7e2);
  d->t_offset = c2d_pspt_d(&p, 0.);
  d->t_max = c2d_pspt_d(&p, 7e4);
  regions = c2d_pspt_i(&p, 7);
  d->n_e = 0;
  for (reg = 0; reg < regions; reg++) {            /* plcm.c:251-299 */
    if (reg < 7) {
      E_lower = dflt_reg[reg][0];
      E_upper = dflt_reg[reg][1];
    } else {
      E_lower = E_upper;
    }
    E_lower = c2d_pspt_d(&p, E_lower);
    E_upper = c2d_pspt_d(&p, E_upper);
    n_r = c2d_pspt_i(&p, n_r);
    c2d_pspt_line(&p, a, (int)sizeof a);
    if (n_r < 1 || n_r + d->n_e > C2D_PLCM_CHMAX) return -1;
    if (a[0] == '1') {
      dE = (E_upper - E_lower) / ((double)(n_r));
      for (e = E_lower, k = d->n_e; k < d->n_e + n_r; k++) { d->E0[k] = e; e = e + dE; d->E1[k] = e; }
    } else {
      dE = exp(log(E_upper / E_lower) / ((double)(n_r)));
      for (e = E_lower, k = d->n_e; k < d->n_e + n_r; k++) { d->E0[k] = e; e = e * dE; d->E1[k] = e; }
    }
    d->n_e += n_r;
  }
  /* plcm.c:236-240: st_max chained time bins from 0 */
  d->n_t = C2D_PLCM_STMAX;
  d->t0[0] = 0.0;
  for (k = 0; k < d->n_t - 1; k++) d->t1[k] = d->t0[k + 1] = d->t0[k] + d->dt;
  d->t1[d->n_t - 1] = d->t0[d->n_t - 1] + d->dt;
  return 0;
}

/* `lead`, then printf's %e (glibc prints a negative-signed NaN as "-nan") */
static void c2d_plcm_e(FILE* f, const char* lead, double x) { fprintf(f, "%s%e", lead, x); }

static void c2d_plcm_head(FILE* f, const c2d_plcm_deck* d, int factor) {
  int l;
  for (l = 0; l < d->n_e; l++) fprintf(f, "#energy range%i: %e %e (keV)\n", l + 1, d->E0[l], d->E1[l]);
  fprintf(f, "#time: %e %e %e\n", d->t_offset, d->t_max, d->dt);
  fprintf(f, "#angle: %f %f\n", d->mu0[0], d->mu1[0]);
  fprintf(f, "#factor: %i\n", factor);
}

static FILE* c2d_plcm_open(const char* dir, const char* name) {
  char path[1200];
  if (snprintf(path, sizeof path, "%s/%s", (dir && dir[0]) ? dir : ".", name) >= (int)sizeof path) return NULL;
  return fopen(path, "w");
}

/* plcm's files (plcm.c:377-388, 466-552) under `dir` from the raw sums per
 * [n_t][n_mu][n_e] bin (sum of ew, of ew^2, counts): per angular bin
 * `<name>` (luminosity, counts, sF/<ew>) and `<name>_aux` (<ew>, <ew^2>,
 * sF), plus the `_particles` header file of bin 0.  Rows run until
 * t1[k] > t_max - t_offset.  0, or -1 when a file cannot be written. */
static int c2d_plcm_write(const char* dir, const c2d_plcm_deck* d, const double* F, const double* F2,
                          const double* cnt, int factor) {
#pragma STDC FP_CONTRACT OFF
  char name[96];
  int k, l, n, bad = 0;
  const double t_stop = d->t_max - d->t_offset;
  FILE *f, *g;
  c2d_plcm_stem(name, (int)sizeof name, d->names[0], "_particles.dat");
  f = c2d_plcm_open(dir, name);
  if (!f) return -1;
  for (l = 0; l < d->n_e; l++) fprintf(f, "# energy range %i : %e %e (keV)\n", l + 1, d->E0[l], d->E1[l]);
  fprintf(f, "# time   : %e %e %e\n", d->t_offset, d->t_max, d->dt);
  fprintf(f, "# mu     : %f %f\n", d->mu0[0], d->mu1[0]);
  fprintf(f, "#\n# time, E, ew, mu, r, z, k(time), n(mu), l(energy)\n#\n");
  if (fclose(f)) return -1;
  for (n = 0; n < d->n_mu; n++) {
    const double den = d->dt * (d->mu1[n] - d->mu0[n]) / 2.;
    f = c2d_plcm_open(dir, d->names[n]);
    if (!f) return -1;
    c2d_plcm_stem(name, (int)sizeof name, d->names[n], "_aux.dat");
    g = c2d_plcm_open(dir, name);
    if (!g) { fclose(f); return -1; }
    c2d_plcm_head(f, d, factor);
    c2d_plcm_head(g, d, factor);
    fputs("#   time      +----------------------------- luminosity ----------------------------+ "
          "+--------------------------- particle_sum ---------------------+ "
          "+---------------------------- var(ew)/<ew> -------------------------+\n", f);
    fputs("#             |    1         2         3         4         5         6         7    | "
          "|       1        2        3        4        5        6        7| "
          "|    1         2         3         4         5         6         7  |\n", f);
    for (k = 0; k < d->n_t; k++) {
      double F1[C2D_PLCM_CHMAX], Fq[C2D_PLCM_CHMAX], sF[C2D_PLCM_CHMAX];
      const size_t h0 = ((size_t)k * d->n_mu + n) * d->n_e;
      const double mid = c2d_pspt_max(1.e-20, (d->t0[k] + d->t1[k]) / 2.);
      for (l = 0; l < d->n_e; l++) {               /* plcm.c:466-490 */
        const double c = cnt[h0 + l];
        if (c > 0) {
          F1[l] = F[h0 + l] / c;
          Fq[l] = F2[h0 + l] / c;
          { const double sq = F1[l] * F1[l]; sF[l] = sqrt(Fq[l] - sq); }
        } else {
          F1[l] = Fq[l] = sF[l] = 1.e-20;
        }
        if (c == 1) sF[l] = 0.0;
      }
      c2d_plcm_e(f, "", mid);
      for (l = 0; l < d->n_e; l++) c2d_plcm_e(f, " ", c2d_pspt_max(1.e-20, F[h0 + l] / den));
      for (l = 0; l < d->n_e; l++) fprintf(f, " %.0f", cnt[h0 + l]);
      for (l = 0; l < d->n_e; l++) c2d_plcm_e(f, " ", sF[l] / F1[l]);
      fputc('\n', f);
      c2d_plcm_e(g, "", mid);
      for (l = 0; l < d->n_e; l++) c2d_plcm_e(g, " ", F1[l]);
      for (l = 0; l < d->n_e; l++) c2d_plcm_e(g, " ", Fq[l]);
      for (l = 0; l < d->n_e; l++) c2d_plcm_e(g, " ", sF[l]);
      fputc('\n', g);
      if (d->t1[k] > t_stop) break;
    }
    bad |= fclose(f);
    bad |= fclose(g);
    if (bad) return -1;
  }
  return 0;
}

#endif /* C2D_PLCM_HOST_H */
