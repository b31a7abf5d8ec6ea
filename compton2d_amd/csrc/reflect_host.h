/* The Compton-reflection tables of the lower boundary and the outer disk
 * (src/ref_matrix.f Pref_calc / Wref_calc, called once from setup2d.f:40-41),
 * on the host: c2d_init builds them for cr_sent 1..3 and uploads them,
 * c2d_reflect_tables_host hands them out without a context.
 *
 *   E_ref[n]        n_ref = 500 energies in keV, E_ref[0] = 1, ratio 1000^(1/500)
 *   P_ref[n_in][n_out]  cumulative probability that a photon entering at
 *                   E_ref[n_in] leaves at or below E_ref[n_out] (White, Lightman
 *                   & Zdziarski 1988, ApJ 331, 939): a running sum over n_out
 *                   normalised per n_in; a step at the diagonal for
 *                   E_ref[n_in] <= 20 keV; 1 above the diagonal
 *   W_abs[n_in][n_out]  the weight kept: min(1, exp(2.5e-6 (x0^-4 - x1^-4)))
 *                   above 20 keV, (1 - sqrt(eps)) / (1 + sqrt(eps)) at or below,
 *                   eps = k_nu / (k_nu + kappa_c) from the photoabsorption of a
 *                   neutral gas; 0 above the diagonal
 * The layout [n_in][n_out] is the reference's COMMON P_ref(n_out, n_in) byte
 * for byte.  Sums run in the reference's order; literals the reference writes
 * without a d exponent are REAL there and keep their float value here (C2D_RF).
 *
 * Header-only C that also compiles as C++; libm only, no device code. */
#ifndef C2D_REFLECT_HOST_H
#define C2D_REFLECT_HOST_H

#include <math.h>

#define C2D_NREF 500
#define C2D_RF(x) ((double)(float)(x))

/* photoabsorption of the neutral ions (ref_matrix.f:159-285, first entry of
 * each table: xi = 0, every ionisation fraction but the first is 0):
 * abundance, K-edge cross section [cm^2] and energy [keV], L-edge likewise.
 * He has one edge and no threshold test (ref_matrix.f:340-345). */
typedef struct c2d_refl_ion {
  double ab, sigma, edge, sigma2, edge2;
} c2d_refl_ion;

static void c2d_refl_ions(c2d_refl_ion* t) {
  const c2d_refl_ion v[12] = {
      {6.33e-2, 9.0e-18, C2D_RF(.024), 0.0, 0.0},                  /* He */
      {3.90e-4, 1.e-18, C2D_RF(.30), 3.e-16, C2D_RF(.011)},         /* C  */
      {8.12e-5, 9.e-19, C2D_RF(.40), 3.e-16, C2D_RF(.014)},         /* N  */
      {6.47e-4, 6.e-19, C2D_RF(.52), 5.e-16, C2D_RF(.013)},         /* O  */
      {9.14e-5, 4.e-19, C2D_RF(.88), 1.e-15, C2D_RF(.021)},         /* Ne */
      {3.73e-5, 2.e-19, C2D_RF(1.2), 4.e-17, C2D_RF(.054)},         /* Mg */
      {3.52e-5, 1.3e-19, C2D_RF(1.8), 4.e-17, C2D_RF(.11)},         /* Si */
      {1.76e-5, 1.e-19, C2D_RF(2.4), 1.e-17, C2D_RF(.16)},          /* S  */
      {3.73e-6, 8.e-20, C2D_RF(3.1), 7.e-18, C2D_RF(.23)},          /* Ar */
      {2.20e-6, 7.e-20, C2D_RF(4.1), 4.e-18, C2D_RF(.35)},          /* Ca */
      {3.16e-5, 3.e-20, C2D_RF(7.1), 2.5e-18, C2D_RF(.71)},         /* Fe */
      {C2D_RF(1.68e-6), 3.e-20, C2D_RF(8.2), 2.e-18, C2D_RF(.89)}}; /* Ni (a REAL literal) */
  for (int i = 0; i < 12; i++) t[i] = v[i];
}

static double c2d_refl_cube(double q) { return q * q * q; }

/* E_ref[500], P_ref[500*500], W_abs[500*500] (any may be null).  Returns 0,
 * or 1 + n_in of the first P_ref column that decreases somewhere in n_out
 * (the device's bisection needs non-decreasing columns). */
static int c2d_reflect_build(double* E_out, double* P_out, double* W_out) {
  const int N = C2D_NREF;
  double E[C2D_NREF], eps[C2D_NREF];
  const double dE = exp(log(1.e3) / (double)N);
  const double E_trans = 20.0;
  int bad = 0;
  E[0] = 1.0;
  for (int n = 1; n < N; n++) E[n] = E[n - 1] * dE;
  if (E_out)
    for (int n = 0; n < N; n++) E_out[n] = E[n];

  if (P_out) {
    for (int ni = 0; ni < N; ni++) {
      double* col = P_out + (size_t)ni * N;
      const double x0 = 1.957e-3 * E[ni];
      const double y0 = 1.0 / x0;
      double sum = 0.0;
      if (E[ni] <= E_trans) {
        for (int no = 0; no < N; no++) col[no] = no < ni ? 0.0 : 1.0;
        continue;
      }
      /* the column's constants (the reference evaluates them per element) */
      const double dyc = 1.e3 - y0;
      const double A = 5.6e-1 + C2D_RF(1.12) / pow(y0, C2D_RF(0.785)) - 3.4e-1 / pow(y0, C2D_RF(1.04));
      const double al = -3.e-1 / pow(y0, C2D_RF(.51)) + 6.e-2 / pow(y0, C2D_RF(.824));
      const double beta = 3.7e-1 - pow(y0, C2D_RF(.85));
      const double den = (pow(y0, 1.0 - beta) * pow(y0 + 2.0, beta) * (pow(1.0 + 2.0 / y0, 1.0 - beta) - 1.0));
      double B;
      if (fabs(al + .5) < 1.e-4)
        B = (1.0 - A * (2.0 + log(.5 * dyc)) / sqrt(dyc)) / den * (1.0 - beta);
      else
        B = (1.0 - A * (2.0 + (pow(.5 * dyc, al + .5) - 1.0) / (al + .5)) / sqrt(dyc)) / den * (1.0 - beta);
      for (int no = 0; no < N; no++) {
        if (no > ni) { col[no] = 1.0; continue; }
        const double x1 = 1.957e-3 * E[no];
        const double y1 = 1.0 / x1;
        const double dy = y1 - y0;
        double Gy;
        if (dy < 2.0) Gy = B * pow((y0 + 2.0) / (y0 + dy), beta);
        else if (dy < dyc) Gy = A * pow(dyc / dy, al) / pow(dy, 1.5);
        else Gy = A / pow(dy, 1.5);
        const double Gx = Gy / (x1 * x1);
        const double dx = dE * x1;
        sum = sum + Gx * dx;
        col[no] = sum;
      }
      for (int no = 0; no <= ni; no++) col[no] = col[no] / sum;
    }
    for (int ni = 0; ni < N && !bad; ni++) {
      const double* col = P_out + (size_t)ni * N;
      for (int no = 1; no < N; no++)
        if (!(col[no] >= col[no - 1])) { bad = 1 + ni; break; }
    }
  }

  if (W_out) {
    c2d_refl_ion ion[12];
    c2d_refl_ions(ion);
    const double n_disk = 1.e18;
    const double kappa_c = 6.65e-25 * n_disk;
    for (int n = 0; n < N; n++) {
      double s = 0.0;
      s = s + ion[0].sigma * ion[0].ab / c2d_refl_cube(E[n] / ion[0].edge);
      for (int i = 1; i < 12; i++) {
        if (E[n] > ion[i].edge) s = s + ion[i].sigma * ion[i].ab / c2d_refl_cube(E[n] / ion[i].edge);
        if (E[n] > ion[i].edge2) s = s + ion[i].sigma2 * ion[i].ab / c2d_refl_cube(E[n] / ion[i].edge2);
      }
      const double k_nu = s * n_disk;
      eps[n] = k_nu / (k_nu + kappa_c);
    }
    for (int ni = 0; ni < N; ni++) {
      double* col = W_out + (size_t)ni * N;
      const double x0 = 1.957e-3 * E[ni];
      for (int no = 0; no < N; no++) {
        if (no > ni) { col[no] = 0.0; continue; }
        if (E[ni] > 20.0) {
          const double x1 = 1.957e-3 * E[no];
          const double y = 2.5e-6 * (1.0 / (x0 * x0 * x0 * x0) - 1.0 / (x1 * x1 * x1 * x1));
          col[no] = (y >= -50.0) ? fmin(1.0, exp(y)) : 0.0;
        } else {
          col[no] = (1.0 - sqrt(eps[ni])) / (1.0 + sqrt(eps[ni]));
        }
      }
    }
  }
  return bad;
}

#endif /* C2D_REFLECT_HOST_H */
