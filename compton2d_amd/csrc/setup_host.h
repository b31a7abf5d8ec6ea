/* The inputs that start a run, restated from the reference's setup in its
 * operation order:
 *
 *   IC_loss      F_IC(i_el, i_ph), the single-electron Klein-Nishina loss
 *                table with f1, f2 and the f_Li series (src/icloss2d.f:1-125)
 *   gam_min      the adjusted gmin, N_nth and gbar_nth of a zone, with
 *                Inttherm / Ith_new (src/gamma1_2d.f:2-105)
 *   P_nontherm   f_nt and Pnt of a zone, the ncycle = 0 branch
 *                (src/nontherm2d.f:20-121; no seb.dat, no positrons)
 *   grids        gnt as P_nontherm builds it (nontherm2d.f:52-54, 87, 95-100),
 *                E_field (setup2d.f:216-222), E_ph (volume2d.f:53, 96, 112-113)
 *
 * Two flavours, chosen by the `libm` argument of every routine that calls an
 * elementary function: libm != 0 uses the C library's log/exp/pow (the
 * target is the reference's own bits), libm == 0 uses c2d_log/c2d_exp/c2d_pow
 * of c2d_math.h, which give the same bits on the host and on gfx950 with
 * contraction off.  Device code always runs the second.
 *
 * What is kept from the Fortran on purpose:
 *   - Inttherm and Ith_new have no `implicit none`: `ts` is an implicit REAL,
 *     so ts = t*s rounds to single precision and ts*sqrt(ts*ts - 1.) is
 *     single-precision arithmetic throughout;
 *   - literals without a d exponent (1.005, 1.01, 511., .5) are REAL and keep
 *     their float value (C2D_RF);
 *   - P_nontherm compares amxwl with the REAL literal 0.99999999 (= 1.0),
 *     gam_min with 0.99999999d0;
 *   - under g < gmin with amxwl <= 1e-4 the inner `if (g.gt.gmin)` never
 *     holds: f_nt = 0 there;
 *   - z**3, g**2, (epsilon*gamma)**2 are multiplications, gmax**p_1 and
 *     g**p_nth are pow;
 *   - P_nontherm does not nudge p_1: p_nth = 1 with amxwl < 1 gives 0/0 there.
 *
 * Header-only C that also compiles as C++ and as HIP device code. */
#ifndef C2D_SETUP_HOST_H
#define C2D_SETUP_HOST_H

#include <math.h>

#include "c2d_math.h"

#ifndef C2D_RF
#define C2D_RF(x) ((double)(float)(x))
#endif

#define C2D_SU_NUM_NT 200
#define C2D_SU_NGRID 400
/* f_Li terms approach 1/n^2 as z -> 0, so the 1e-10 test stops by about
 * 7.8e4 terms for any z > 0; the cap only keeps a series from spinning */
#define C2D_SU_FLI_CAP 262144
/* Inttherm / Ith_new: t grows by 1.005 a term, so a finite g1 ends the loop
 * within ln(DBL_MAX)/ln(1.005) = 1.43e5 terms */
#define C2D_SU_ITH_CAP 200000
/* McDonald's series (volume2d.f:598-626) on the host */
#define C2D_SU_MCD_CAP 4000000

C2D_HD double c2d_su_log(double x, int libm) {
#if defined(__HIP_DEVICE_COMPILE__)
  (void)libm;
  return c2d_log(x);
#else
  return libm ? log(x) : c2d_log(x);
#endif
}
C2D_HD double c2d_su_exp(double x, int libm) {
#if defined(__HIP_DEVICE_COMPILE__)
  (void)libm;
  return c2d_exp(x);
#else
  return libm ? exp(x) : c2d_exp(x);
#endif
}
C2D_HD double c2d_su_pow(double x, double y, int libm) {
#if defined(__HIP_DEVICE_COMPILE__)
  (void)libm;
  return c2d_pow(x, y);
#else
  return libm ? pow(x, y) : c2d_pow(x, y);
#endif
}

/* ---- IC_loss (icloss2d.f) ------------------------------------------- */

/* f_Li's value before the series (icloss2d.f:112-113) */
C2D_HD double c2d_su_fli_start(double z, int libm) {
  const double y = 1.0 + 2.0 * z;
  const double ly = c2d_su_log(y, libm);
  return ly * (5.0e-1 * ly - c2d_su_log(2.0 * z, libm));
}

/* f_Li (icloss2d.f:104-125), term by term.  *capped is set when the series
 * has not stopped after C2D_SU_FLI_CAP terms. */
C2D_HD double c2d_su_fli(double z, int libm, int* capped) {
  const double y = 1.0 + 2.0 * z;
  double sum = c2d_su_fli_start(z, libm);
  double sd = 1.0 / y, nn = 2.0;
  int n = 1;
  sum = sum + sd;
  while (fabs(sd / sum) > 1.0e-10) {
    if (++n > C2D_SU_FLI_CAP) {
      *capped = 1;
      break;
    }
    const double q = (nn - 1.0) / nn;
    sd = sd * (q * q) / y;
    nn = nn + 1.0;
    sum = sum + sd;
  }
  return sum;
}

/* f1, f2 (icloss2d.f:68-99) with f_Li(z) given */
C2D_HD double c2d_su_f1(double z, double fli, int libm) {
  const double y = 1.0 + 2.0 * z;
  const double sd1 = (z + 6.0 + 3.0 / z) * c2d_su_log(y, libm);
  const double sd2 = ((2.2e1 / 3.0) * (z * z * z) + 24.0 * (z * z) + 18.0 * z + 4.0) / (y * y);
  return sd1 - sd2 - 2.0 + 2.0 * fli;
}
C2D_HD double c2d_su_f2(double z, double fli, int libm) {
  const double y = 1.0 + 2.0 * z;
  const double sd1 = (z + (3.1e1 / 6.0) + 5.0 / z + 1.5 / (z * z)) * c2d_su_log(y, libm);
  const double sd2 =
      ((2.2e1 / 3.0) * (z * z * z) + 28.0 * (z * z) + (1.03e2 / 3.0) * z + 1.7e1 + 3.0 / z) / (y * y);
  return sd1 - sd2 - 2.0 + fli;
}

/* One entry's branch and series arguments (icloss2d.f:25-36): returns 1 for
 * the Klein-Nishina branch with z1, z2 set, 0 for the Thomson product. */
typedef struct c2d_su_ic_entry {
  double gamma, beta, epsilon, z1, z2;
} c2d_su_ic_entry;
C2D_HD int c2d_su_ic_args(double gnt, double E_field, c2d_su_ic_entry* e) {
  e->gamma = 1.0 + gnt;
  e->beta = __builtin_sqrt(1.0 - 1.0 / (e->gamma * e->gamma));
  e->epsilon = 1.957e-3 * E_field;
  if (e->gamma * e->epsilon < 1.0e-2) return 0;
  e->z1 = e->epsilon * e->gamma * (1.0 + e->beta);
  e->z2 = e->epsilon / (e->gamma * (1.0 + e->beta));
  return 1;
}
C2D_HD double c2d_su_ic_thomson(const c2d_su_ic_entry* e) {
  return 2.66e-14 * e->epsilon * (e->gamma * e->gamma - 1.0);
}
/* the Klein-Nishina entry from f_Li(z1), f_Li(z2) (icloss2d.f:38-41) */
C2D_HD double c2d_su_ic_kn(const c2d_su_ic_entry* e, double fli1, double fli2, int libm) {
  const double A = 3.7419e-15;
  const double F = e->gamma * (c2d_su_f1(e->z1, fli1, libm) - c2d_su_f1(e->z2, fli2, libm)) -
                   e->epsilon * (c2d_su_f2(e->z1, fli1, libm) - c2d_su_f2(e->z2, fli2, libm));
  return A * F / (((e->epsilon * e->gamma) * (e->epsilon * e->gamma)) * e->beta);
}

/* F_IC[i_el * s_i + i_ph * s_ph] for i_el < n_el, i_ph < n_ph.  Returns 0, or
 * 1 if a series hit its cap.  Each f_Li is evaluated once per entry (the
 * reference evaluates it in f1 and again in f2: a pure function). */
static int c2d_su_ic_loss(const double* gnt, int n_el, const double* E_field, int n_ph, double* F_IC,
                          long long s_i, long long s_ph, int libm) {
  int capped = 0;
  for (int i = 0; i < n_el; i++)
    for (int p = 0; p < n_ph; p++) {
      c2d_su_ic_entry e;
      double v;
      if (c2d_su_ic_args(gnt[i], E_field[p], &e)) {
        const double l1 = c2d_su_fli(e.z1, libm, &capped);
        const double l2 = c2d_su_fli(e.z2, libm, &capped);
        v = c2d_su_ic_kn(&e, l1, l2, libm);
      } else {
        v = c2d_su_ic_thomson(&e);
      }
      F_IC[(long long)i * s_i + (long long)p * s_ph] = v;
    }
  return capped;
}

/* ---- grids ---------------------------------------------------------- */

/* gnt[200], E_field[400], E_ph[400]; any may be null.  The C library's
 * log/exp, as the reference's dlog/dexp. */
static void c2d_su_grids(double* gnt, double* E_field, double* E_ph) {
  if (gnt) {
    const double dg = 1.1;
    double g_1 = 2.0e-1 / dg;
    for (int i = 0; i < C2D_SU_NUM_NT; i++) {
      gnt[i] = g_1;
      g_1 = (i == 0) ? 2.0e-1 : g_1 * dg;
    }
  }
  if (E_field) {
    const double dE = exp(log(1.0e20) / (double)C2D_SU_NGRID);
    E_field[0] = 1.0e-10;
    for (int i = 1; i < C2D_SU_NGRID; i++) E_field[i] = E_field[i - 1] * dE;
  }
  if (E_ph) {
    const double dE = exp(log(1.0e20) / (double)C2D_SU_NGRID);
    double E = 1.0e-10 / dE;
    for (int i = 0; i < C2D_SU_NGRID; i++) {
      E = E * dE;
      E_ph[i] = E;
    }
  }
}

/* ---- gam_min, P_nontherm -------------------------------------------- */

/* Inttherm (shift = 0, gamma1_2d.f:55-78) and Ith_new (shift = 1, :82-105) */
C2D_HD double c2d_su_inttherm(double g1, double Theta, int shift, int libm, int* capped) {
  const double dt = C2D_RF(1.005);
  const double s = C2D_RF(.5) * (1.0 + dt);
  const double sw = dt - 1.0;
  double t = 1.0, sum = 0.0;
  int n = 0;
  do {
    const float ts = (float)(t * s);
    const float tm = ts - 1.0f;
    const double y = shift ? (double)tm / Theta : (double)ts / Theta;
    double sd;
    if (y < 2.0e2) {
      const float t2 = ts * ts;
      const float rt = __builtin_sqrtf(t2 - 1.0f);
      const float a = ts * rt;
      sd = (double)a * c2d_su_exp(-y, libm);
    } else {
      sd = 1.0e-200;
    }
    sum = sum + sd * t * sw;
    t = t * dt;
    if (++n > C2D_SU_ITH_CAP) {
      *capped = 1;
      break;
    }
  } while (t < g1);
  return sum;
}

/* gam_min up to label 15 (gamma1_2d.f:13-42): the adjusted gmin and N_nth.
 * Returns 1 when gbar_nth is gamma_bar(Theta), 0 when c2d_su_gbar_pl gives
 * it.  (The fth / fnth of :37-39 feed only commented-out tests.) */
typedef struct c2d_su_gm {
  double Theta, gmin, N_nth, p_2;
} c2d_su_gm;
C2D_HD int c2d_su_gam_min(double tea, double amxwl, double gmin, double gmax, double p_nth, int libm,
                          c2d_su_gm* o) {
  o->Theta = tea / C2D_RF(511.);
  o->gmin = gmin;
  o->p_2 = 0.0;
  if (amxwl > 0.99999999e0) {
    o->gmin = 1.0 + 1.0e2 * o->Theta;
    o->N_nth = 1.0e-20;
    return 1;
  }
  double p_1 = 1.0 - p_nth;
  double p_2 = 2.0 - p_nth;
  if (fabs(p_1) < 1.0e-4) p_1 = p_1 + 2.0e-4;
  if (fabs(p_2) < 1.0e-4) p_2 = p_2 + 2.0e-4;
  o->p_2 = p_2;
  if (amxwl < 1.0e-4 || tea < 1.0) {
    if (o->gmin < 1.01e0) o->gmin = 1.01e0;
    o->N_nth = p_1 / (c2d_su_pow(gmax, p_1, libm) - c2d_su_pow(o->gmin, p_1, libm));
  } else {
    o->gmin = o->gmin / C2D_RF(1.01);
    o->N_nth = (1.0 - amxwl) * p_1 / (c2d_su_pow(gmax, p_1, libm) - c2d_su_pow(o->gmin, p_1, libm));
  }
  return amxwl > 1.0e-4;
}
/* gbar_nth of the power law (gamma1_2d.f:47-48) */
C2D_HD double c2d_su_gbar_pl(const c2d_su_gm* o, double gmax, int libm) {
  return o->N_nth * (c2d_su_pow(gmax, o->p_2, libm) - c2d_su_pow(o->gmin, o->p_2, libm)) / o->p_2;
}

/* P_nontherm's normalisations (nontherm2d.f:20-32) with gam_min's gmin */
C2D_HD void c2d_su_pnt_norm(double Theta, double amxwl, double gmin, double gmax, double p_nth,
                            int libm, double* Ntherm, double* Nnth, int* capped) {
  const double p_1 = 1.0 - p_nth;
  if (amxwl < 1.0e-4)
    *Ntherm = 0.0;
  else
    *Ntherm = amxwl / c2d_su_inttherm(gmin, Theta, 1, libm, capped);
  if (amxwl < C2D_RF(0.99999999))
    *Nnth = (1.0 - amxwl) * p_1 / (c2d_su_pow(gmax, p_1, libm) - c2d_su_pow(gmin, p_1, libm));
  else
    *Nnth = 0.0;
}
/* f_nt of the bin at gamma - 1 = g_1 before normalisation (nontherm2d.f:58-85) */
C2D_HD double c2d_su_fnt_bin(double g_1, double Theta, double amxwl, double gmin, double gmax,
                             double p_nth, double Ntherm, double Nnth, int libm) {
  const double g = 1.0 + g_1;
  const double beta = __builtin_sqrt(1.0 - 1.0 / (g * g));
  if (g < gmin) {
    if (amxwl > 1.0e-4) {
      const double y = (g - 1.0) / Theta;
      return (y < 1.0e2) ? Ntherm * (g * g) * beta / c2d_su_exp(y, libm) : 0.0;
    }
    return 0.0; /* the broken power law's `if (g.gt.gmin)` never holds here */
  }
  const double y = g / gmax;
  return (y < 1.0e2) ? Nnth / (c2d_su_pow(g, p_nth, libm) * c2d_su_exp(y, libm)) : 0.0;
}

/* gammln, McDonald, gamma_bar (volume2d.f:572-668) term by term: what the
 * kernels' wave-level gamma_bar (c2d_wave.hpp) computes, in sequence */
static double c2d_su_gammln(double xx, int libm) {
  const double cof[6] = {76.18009172947146, -86.50532032941677, 24.01409824083091,
                         -1.231739572450155, .1208650973866179e-2, -.5395239384953e-5};
  const double stp = 2.5066282746310005;
  double x = xx, y = x, tmp = x + 5.5;
  tmp = (x + 0.5) * c2d_su_log(tmp, libm) - tmp;
  double ser = 1.000000000190015;
  for (int j = 0; j < 6; j++) {
    y = y + 1.0;
    ser = ser + cof[j] / y;
  }
  return tmp + c2d_su_log(stp * ser / x, libm);
}
static double c2d_su_mcdonald(double nu, double z, int libm, int* capped) {
  const double dt = 1.001, d = dt - 1.0, s = 5.0e-1 * (1.0 + dt), a = nu - 5.0e-1;
  double sum = 0.0, t = 1.0, sd;
  int n = 0;
  do {
    const double ts = t * s;
    const double y = z * ts;
    sd = (y < 2.25e2) ? c2d_su_pow(ts * ts - 1.0, a, libm) / c2d_su_exp(y, libm) : 0.0;
    sum = sum + d * t * sd;
    t = t * dt;
    if (++n > C2D_SU_MCD_CAP) {
      *capped = 1;
      break;
    }
  } while (t < 2.0 || sd > 1.0e-8);
  return __builtin_sqrt(3.14159265) * c2d_su_pow(5.0e-1 * z, nu, libm) * sum /
         c2d_su_exp(c2d_su_gammln(5.0e-1 + nu, libm), libm);
}
static double c2d_su_gamma_bar(double Theta, int libm, int* capped) {
  double g;
  if (Theta < C2D_RF(0.2)) {
    g = (1. + C2D_RF(4.375) * Theta + C2D_RF(7.383) * (Theta * Theta) +
         C2D_RF(3.384) * (Theta * Theta * Theta)) /
            (1. + C2D_RF(1.875) * Theta + C2D_RF(.8203) * (Theta * Theta)) -
        Theta;
  } else {
    const double K2 = c2d_su_mcdonald(2.0, 1.0 / Theta, libm, capped);
    const double K3 = c2d_su_mcdonald(3.0, 1.0 / Theta, libm, capped);
    g = K3 / K2 - Theta;
  }
  if (g < 1.0) g = 1.0;
  return g;
}

/* gam_min then P_nontherm of one zone (setup2d.f:130-132).  gnt from
 * c2d_su_grids; f_nt and Pnt hold 200 values.  Returns 0, or 1 if a loop hit
 * its cap. */
static int c2d_su_electrons_zone(double tea, double amxwl, double gmin, double gmax, double p_nth,
                                 const double* gnt, int libm, double* gmin_out, double* N_nth,
                                 double* gbar_nth, double* f_nt, double* Pnt) {
  int capped = 0;
  c2d_su_gm gm;
  if (c2d_su_gam_min(tea, amxwl, gmin, gmax, p_nth, libm, &gm))
    *gbar_nth = c2d_su_gamma_bar(gm.Theta, libm, &capped);
  else
    *gbar_nth = c2d_su_gbar_pl(&gm, gmax, libm);
  *gmin_out = gm.gmin;
  *N_nth = gm.N_nth;
  const double Theta = tea / 5.11e2;
  double Ntherm, Nnth, sum = 0.0;
  c2d_su_pnt_norm(Theta, amxwl, gm.gmin, gmax, p_nth, libm, &Ntherm, &Nnth, &capped);
  for (int i = 0; i < C2D_SU_NUM_NT; i++) {
    f_nt[i] = c2d_su_fnt_bin(gnt[i], Theta, amxwl, gm.gmin, gmax, p_nth, Ntherm, Nnth, libm);
    if (i > 0) {
      sum = sum + f_nt[i - 1] * (gnt[i] - gnt[i - 1]);
      Pnt[i - 1] = sum;
    }
  }
  Pnt[C2D_SU_NUM_NT - 1] = sum;
  for (int i = 0; i < C2D_SU_NUM_NT; i++) {
    Pnt[i] = Pnt[i] / sum;
    f_nt[i] = f_nt[i] / sum;
  }
  return capped;
}

#endif /* C2D_SETUP_HOST_H */
