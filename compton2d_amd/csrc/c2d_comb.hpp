/*
 * c2d_comb.hpp — the device side of the census comb (comb.hip) as
 * popctl_api.cpp drives it: the counters of one call and the kernel's launcher.  The rule
 * itself is c2d_comb.h.
 */
#ifndef C2D_COMB_HPP
#define C2D_COMB_HPP

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "c2d_comb.h"
#include "c2d_popctl.hpp"

namespace c2d {

/* One call's counters in device memory, zeroed by the caller. */
struct CombCtl {
  unsigned long long n_fixed;     /* records no floor of the family can remove     */
  unsigned long long n_match;     /* pool records whose c carries the prefix       */
  unsigned long long n_collect;   /* places the collecting waves have reserved     */
  unsigned long long pad[13];
};

}  // namespace c2d

/* One pass over the census records of p.  hist != NULL: hist[digit below the
 * prefix] += 1 for every matching pool record (C2D_COMB_BINS u64, zeroed by
 * the caller).  hist == NULL: the matching c values go to vals[0, cap), in any
 * order; ctl->n_collect counts them all.  grid_cap > 0 caps the workgroups.
 * Device pointers throughout. */
extern "C" int c2d_launch_census_comb(const c2d::CensusPass& p, const double* norm, uint64_t salt, uint64_t prefix,
                                      int prefix_bits, unsigned long long* hist, double* vals, int64_t cap,
                                      c2d::CombCtl* ctl, int grid_cap);

#endif /* C2D_COMB_HPP */
