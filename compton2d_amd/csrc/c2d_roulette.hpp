/*
 * c2d_roulette.hpp — the device side of census population control
 * (roulette.hip) as popctl_api.cpp drives it: the control block the kernels of
 * one c2d_census_roulette call share, and their launchers.  The rule itself is
 * c2d_roulette.h.
 */
#ifndef C2D_ROULETTE_HPP
#define C2D_ROULETTE_HPP

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "c2d_popctl.hpp"

namespace c2d {

/* The scratch buffer of a slice is cut into RL_SHARDS regions, each with its
 * own fill counter (one per 128-byte line): tile t reserves its survivors'
 * places in region t % RL_SHARDS.  One counter for all tiles serialises: a
 * returning atomic on one address takes about 38 ns on the MI355X, 3.7 ms for
 * the 97 656 tiles of 1e8 records, three times what the records' traffic
 * takes. */
constexpr int RL_SHARDS = 64;
constexpr int RL_SHARD_STRIDE = 16;   /* 64-bit words between two counters */
constexpr int RL_TILE = 1024;         /* records a workgroup takes at a time */

/* One call's counters in device memory.  The pass works the census front to
 * back in slices: a slice's survivors are packed into the scratch regions,
 * unpacked at the write cursor W in region order, and W moves on.  W never
 * passes the start of the slice in work, so nothing unread is overwritten. */
struct RouletteCtl {
  unsigned long long W;          /* census records written so far       */
  unsigned long long n_tested;   /* records with ew < w                 */
  double e_before, e_after;      /* sum of ew before and after the pass */
  unsigned long long pad[12];
  unsigned long long cnt[RL_SHARDS * RL_SHARD_STRIDE];   /* survivors of the slice in work, per region */
};

/* records of a region of the scratch for a slice of m records: the tiles are dealt round-robin */
inline int64_t rl_region(int64_t m) {
  const int64_t tiles = (m + RL_TILE - 1) / RL_TILE;
  return (tiles + RL_SHARDS - 1) / RL_SHARDS * RL_TILE;
}
/* the largest slice whose regions fit a scratch of cap records (cap >= RL_SHARDS * RL_TILE) */
inline int64_t rl_slice(int64_t cap) {
  return cap / ((int64_t)RL_SHARDS * RL_TILE) * ((int64_t)RL_SHARDS * RL_TILE);
}

/* LDS bytes up to which the stats kernel privatises its histogram (12 bytes
 * a bin): what a workgroup may ask for without an attribute.  Two
 * workgroups of 1024 threads, a CU's 32 waves, fit the 160 KiB beside it;
 * the C3 grid's 270 cells x 18 decade groups take 58 KB. */
constexpr size_t RL_STATS_LDS_MAX = 64 * 1024;

}  // namespace c2d

/* count[cell][group] (+= records) and energy[cell][group] (+= ew) over the
 * census records of p; both zeroed by the caller.  Device pointers throughout. */
extern "C" int c2d_launch_census_stats(const c2d::CensusPass& p, unsigned long long* count, double* energy);
/* One slice [first, first + m) of the roulette pass (p.n is not read): decide and pack into
 * `scratch` (four columns of `cap` 16-byte entries, RL_SHARDS regions of
 * rl_region(m) records in each: RL_SHARDS * rl_region(m) <= cap), unpack at
 * the cursor, advance it.  pack = 0 only decides and sums (nothing is written
 * but ctl's n_tested, e_before, e_after). */
extern "C" int c2d_launch_roulette_slice(const c2d::CensusPass& p, int64_t first, int64_t m, const double* w_min,
                                         uint64_t salt, uint64_t* scratch, int64_t cap, c2d::RouletteCtl* ctl,
                                         int pack);

#endif /* C2D_ROULETTE_HPP */
