/*
 * c2d_split.hpp — the device side of census splitting (split.hip) as
 * popctl_api.cpp drives it: the control block the kernels of one
 * c2d_census_split call share, and their launchers.  The rule itself is c2d_split.h.
 */
#ifndef C2D_SPLIT_HPP
#define C2D_SPLIT_HPP

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "c2d_popctl.hpp"
#include "c2d_split.h"

namespace c2d {

constexpr int SP_TILE = 1024;          /* records a workgroup takes at a time */
constexpr int SP_SCAN_BLOCK = 1024;    /* threads of the one scan workgroup   */
constexpr int SP_SCAN_PER = 4;         /* tiles a scan thread takes in a strip */
constexpr int64_t SP_SCAN_STRIP = (int64_t)SP_SCAN_BLOCK * SP_SCAN_PER;   /* the largest strip, in tiles */

/* One call's sums in device memory. */
struct SplitCtl {
  unsigned long long n_split;    /* records with m > 1                    */
  unsigned long long n_extra;    /* sum of (m - 1): the copies to be made */
  double e_before, e_after;      /* sum of ew before and after the pass   */
  unsigned long long pad[28];
};

inline int64_t sp_tiles(int64_t n) { return (n + SP_TILE - 1) / SP_TILE; }

}  // namespace c2d

/* Per tile of SP_TILE census records of p the number of copies its
 * records ask for, sum (m - 1), into cnt[tile]; n_split, e_before and
 * e_after into ctl (zeroed by the caller).  Device pointers throughout. */
extern "C" int c2d_launch_split_count(const c2d::CensusPass& p, const double* w_max, int max_copies, uint32_t* cnt,
                                      c2d::SplitCtl* ctl);
/* off[t] = cnt[0] + ... + cnt[t - 1] over ntiles tiles, ctl->n_extra their
 * sum: one workgroup, strips of `strip` tiles (1..SP_SCAN_STRIP). */
extern "C" int c2d_launch_split_scan(const uint32_t* cnt, int64_t ntiles, int64_t strip, int64_t* off,
                                     c2d::SplitCtl* ctl, hipStream_t s);
/* The split records of p's [0, n) take their new ew; copy i of the k-th split
 * record of tile t goes to census item n + off[t] + (its place in the tile),
 * below n_after: the chunk list reaches that far. */
extern "C" int c2d_launch_split_expand(const c2d::CensusPass& p, int64_t n_after, const double* w_max, int max_copies,
                                       uint64_t salt, const uint32_t* cnt, const int64_t* off);

#endif /* C2D_SPLIT_HPP */
