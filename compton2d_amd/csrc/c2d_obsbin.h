/*
 * c2d_obsbin.h — the observer's bin decision (postprocessing/pspt.c:245-294,
 * plcm.c:382-456), one rule for the f64 kernels
 * (observe.hip), the exact kernel (obsacc.hip) and the exact accumulation's
 * host twin (c2d_obs_exact_host): Lorentz boost with the bulk factor,
 * light-travel time, first-match bin search, and one call of the caller's
 * `add(h, w)` per histogram bin the event could enter (h = -1: none), so
 * what differs between the callers is the add alone.
 *
 * C++ (a template over the view and the add) that compiles on the host and
 * as HIP device code; compile with contraction off: only IEEE +,-,*,/ and
 * sqrt and c2d_math.h's cos are used, so both sides decide alike, bit for
 * bit (the oracle's `det` flavour uses the same cos).
 */
#ifndef C2D_OBSBIN_H
#define C2D_OBSBIN_H

#include <stdint.h>

#include "../../include/compton2d.h"
#include "c2d_math.h"

namespace c2d {

/* what every observer needs of an event, computed once */
struct ObsEvent {
  double t_bound, E, ew, z;
  double mu_c;                             /* -wmu */
  double rcos;                             /* r cos(phi) */
};

/* the 7 words of an event (c2d_events layout) */
C2D_HD ObsEvent obs_event_of(const double* v) {
  ObsEvent ev;
  ev.t_bound = v[0]; ev.E = v[1]; ev.ew = v[2];
  const double r = v[3];
  ev.z = v[4];
  ev.mu_c = -v[5];
  ev.rcos = r * c2d_cos(v[6]);
  return ev;
}

/* beta of a bulk Lorentz factor */
C2D_HD double obs_betta(double G) { return __builtin_sqrt(1. - 1. / (G * G)); }

/* First k with lo[k] <= x < hi[k] (the tools' linear first-match scan), or n.
 * When lo[] and hi[] are both non-decreasing (`sorted`, checked on the host)
 * the matching k form a contiguous range whose first element is the first k
 * with hi[k] > x: a binary search then gives the same answer, NaN included. */
C2D_HD int first_bin(const double* lo, const double* hi, int n, bool sorted, double x) {
  if (!sorted) {
    int k;
    for (k = 0; k < n; k++)
      if (x >= lo[k] && x < hi[k]) break;
    return k;
  }
  int a = 0, b = n;                      /* first k in [a, b) with hi[k] > x */
  while (a < b) {
    const int m = (a + b) >> 1;
    if (hi[m] > x) b = m; else a = m + 1;
  }
  return (a < n && x >= lo[a]) ? a : n;
}

/* lo[] and hi[] non-decreasing: first_bin may search them by bisection */
C2D_HD int obs_sorted(const double* lo, const double* hi, int n) {
  for (int i = 1; i < n; i++)
    if (!(lo[i] >= lo[i - 1]) || !(hi[i] >= hi[i - 1])) return 0;
  return 1;
}

/* The decision fields of a histogram view (the kernels' ObsView has them and
 * its accumulators besides): bins h = row * n_mu * n_e + col, row = time bin. */
struct ObsBinView {
  double G, betta, rmax, t_offset;
  int32_t mode, n_t, n_mu, n_e;
  int32_t sorted_t, sorted_mu, sorted_e;
  const double *t0, *t1, *mu0, *mu1, *E0, *E1;
};

/* Boost, light-travel time and bin decision of one event in one histogram.
 * Control flow is uniform down to `add`: no early return for an event past
 * the end (!valid) or outside the window, they carry h = -1; a light curve
 * calls add once per energy band. */
template <class View, class Add>
C2D_HD void obs_decide(const View& V, const ObsEvent& ev, bool valid, Add add) {
  /* pspt.c:253-272 / plcm.c:390-399 */
  const double G = V.G, betta = V.betta;
  double mu = ev.mu_c;
  const double doppler = G * (1. + mu * betta);
  const double t_bound = (ev.t_bound - betta * ev.z * 3.33333333e-11) / doppler;
  const double E = ev.E * doppler;
  const double ew = ev.ew * doppler;
  mu = (mu + betta) / (1. + mu * betta);
  const double cdt = ev.z * mu / G + __builtin_sqrt(1. - mu * mu) * (V.rmax - ev.rcos);
  double time = t_bound + 3.33333333e-11 * cdt;
  if (V.mode == C2D_OBS_SED) {
    int h = -1;
    if (valid && !(mu < V.mu0[0] || mu > V.mu1[0])) {          /* pspt.c:274 */
      const int k = first_bin(V.E0, V.E1, V.n_e, V.sorted_e, E);
      const int m = first_bin(V.t0, V.t1, V.n_t, V.sorted_t, time);
      if (k < V.n_e && m < V.n_t) h = m * V.n_e + k;
    }
    add(h, ew);
  } else {
    time -= V.t_offset;                                        /* plcm.c:407-408 */
    int row = -1;
    if (valid && !(time < 0.)) {
      const int k = first_bin(V.t0, V.t1, V.n_t, V.sorted_t, time);
      const int m = first_bin(V.mu0, V.mu1, V.n_mu, V.sorted_mu, mu);
      if (k < V.n_t && m < V.n_mu) row = (k * V.n_mu + m) * V.n_e;
    }
    for (int l = 0; l < V.n_e; l++)                            /* every band containing E */
      add((row >= 0 && E >= V.E0[l] && E < V.E1[l]) ? row + l : -1, ew);
  }
}

}  // namespace c2d

#endif /* C2D_OBSBIN_H */
