/* Compton reflection at the lower boundary and the outer disk on the device
 * (src/imcleak2d.f:104-165 and :197-275; tables: reflect_host.h).  Included
 * by transport.hip (imcleak<1>) and selftest.hip (c2d_selftest_reflect): the
 * same functions, compiled with floating-point contraction off in every
 * build, so their results are those of a plain IEEE restatement
 * (tests/reflect_ref.py) bit for bit.
 *
 * Draws come from the packet's own stream (key, sub, ctr) in the reference's
 * order -- rnum, the xnu draw if n_out > 1, the disk's wmu -- and ctr
 * advances by the draws taken (c2d_rng.h, lineage rules).
 *
 * Hazards reproduced: a photon below E_ref(1) = 1 keV
 * leaves at exactly 1 keV with weight ew W_abs(1,1) / xnu_old; the disk sets
 * zpre = 0 before it computes f = zpre ..., so f = 0 and rpre = sqrt(rpre^2). */
#ifndef C2D_REFLECT_HPP
#define C2D_REFLECT_HPP

#include <stdint.h>

#include "c2d_device.hpp"
#include "c2d_rng.h"

namespace c2d {

constexpr int REFL_N = 500;                       /* n_ref (general.pa) */
constexpr double REFL_RAD_CP = 3.333564097e-11;   /* general.pa:23 */
enum : int32_t { REFL_NONE = 0, REFL_SPECULAR = 1, REFL_MATRIX = 2, REFL_DISK = 3 };

/* the tables in device memory, [n_in][n_out], and the step's results:
 * out[0 .. nr) = Ed_ref, out[nr + 0..2] = specular, matrix, disk counts */
struct ReflTab {
  const double* E;
  const double* P;
  const double* W;
  double* out;
  int32_t nr;
};

/* the part of a packet the reflection reads or writes */
struct ReflPkt {
  double xnu, ew, wmu, rpre, zpre, dcen;
  uint64_t key;
  uint32_t sub, ctr;
  int32_t n_in, n_out;      /* 1-based, 0: no matrix lookup was made */
};

/* first i in [0, n) with a[i] >= x, n - 1 if none: the reference's linear
 * scans `if (a(i) .lt. x .and. i .lt. n_ref) i = i + 1` (imcleak2d.f:124-138)
 * by bisection on a non-decreasing array (c2d_init checks P_ref's columns) */
__device__ __forceinline__ int refl_first_ge(const double* a, double x) {
  int lo = 0, hi = REFL_N - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (gld(a + mid) < x) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

/* n_in, rnum, n_out, the new xnu and weight (imcleak2d.f:124-154, :222-246) */
__device__ __forceinline__ void refl_sample(const ReflTab& R, ReflPkt& q) {
#pragma clang fp contract(off)
  const double xnu_sv = q.xnu;
  const int ni = refl_first_ge(R.E, q.xnu);
  const double rnum = c2d_draw_s(q.key, q.sub, q.ctr++);
  const int no = refl_first_ge(R.P + (int64_t)ni * REFL_N, rnum);
  if (no > 0) {
    const double e0 = gld(R.E + no - 1), e1 = gld(R.E + no);
    q.xnu = e0 + c2d_draw_s(q.key, q.sub, q.ctr++) * (e1 - e0);
  } else {
    q.xnu = gld(R.E);
  }
  q.ew = q.ew * gld(R.W + (int64_t)ni * REFL_N + no) * q.xnu / xnu_sv;
  q.n_in = ni + 1;
  q.n_out = no + 1;
}

/* Lower boundary (jph = 0), ring kph (1-based), cr_sent 1, 3, 4.  Returns
 * REFL_NONE (the packet escapes as without reflection), REFL_SPECULAR or
 * REFL_MATRIX; after a reflection the packet lives on in zone row 1.  The
 * caller rebins (get_bin) and, for the specular branch with spec_switch = 1,
 * adds fout with the bins from before. */
__device__ __forceinline__ int reflect_lower(const ReflTab& R, int cr_sent, double tbbl, int kph, ReflPkt& q) {
#pragma clang fp contract(off)
  if (cr_sent != 1 && cr_sent != 3 && cr_sent != 4) return REFL_NONE;
  if (tbbl <= 0.0 || cr_sent == 4) {
    q.wmu = -q.wmu;
    gadd(R.out + R.nr + 0, 1.0);
    return REFL_SPECULAR;
  }
  refl_sample(R, q);
  gadd(R.out + (kph - 1), q.ew);      /* Ed_ref: the new weight */
  q.wmu = fabs(q.wmu);
  gadd(R.out + R.nr + 1, 1.0);
  return REFL_MATRIX;
}

/* Outer r-boundary, cr_sent 2, 3, a packet heading down (wmu <= 0).  Returns
 * REFL_NONE (t_bound untouched) or REFL_DISK: the packet leaves from the disk
 * plane with the reference's t_bound (the H4 recomputation covers the other
 * exits only). */
__device__ __forceinline__ int reflect_outer(const ReflTab& R, int cr_sent, double time, double dt, ReflPkt& q,
                                             double& t_bound) {
#pragma clang fp contract(off)
  if (q.wmu > 0.0 || (cr_sent != 2 && cr_sent != 3)) return REFL_NONE;
  refl_sample(R, q);
  if (fabs(q.wmu) > 1.0e-6) {
    t_bound = time + dt - REFL_RAD_CP * (q.dcen + q.zpre / q.wmu);
    q.zpre = 0.0;                      /* before f (H14): f = 0 */
    q.rpre = __builtin_sqrt(q.rpre * q.rpre);
  } else {
    t_bound = 1.0e20;
  }
  q.wmu = c2d_draw_s(q.key, q.sub, q.ctr++);
  gadd(R.out + R.nr + 2, 1.0);
  return REFL_DISK;
}

}  // namespace c2d

#endif /* C2D_REFLECT_HPP */
