/*
 * c2d_popctl.hpp — what the census passes of population control share
 * (roulette.hip, split.hip, comb.hip and their driver popctl_api.cpp): the
 * arguments every launcher takes, the grid size of a pass, and the kernels'
 * lookup of a record's (cell, group) bin.
 */
#ifndef C2D_POPCTL_HPP
#define C2D_POPCTL_HPP

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "c2d_device.hpp"
#include "c2d_roulette.h"

namespace c2d {

/* The census a pass streams and how its records are binned.  Device pointers
 * throughout; clist == NULL: the census is not chunked. */
struct CensusPass {
  CensusSoA cs;
  const int32_t* clist;
  int64_t n;                    /* records [0, n) */
  int nz, nr, ngroup;
  const int32_t* group_of_sp;   /* [C2D_ROULETTE_NSP] */
  int n_cu;
  hipStream_t stream;
};

/* workgroups of a pass over `records` records in tiles of `tile`: one a tile, at most per_cu a CU */
inline unsigned census_grid(int64_t records, int64_t tile, int n_cu, int per_cu) {
  const int64_t tiles = (records + tile - 1) / tile;
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>(tiles, (int64_t)std::max(n_cu, 1) * per_cu));
}

/* group_of_sp into LDS, one byte an entry (groups < 32) */
__device__ __forceinline__ void census_load_groups(uint8_t* grp, const int32_t* __restrict__ group_of_sp) {
  for (int i = (int)threadIdx.x; i < C2D_ROULETTE_NSP; i += (int)blockDim.x) grp[i] = (uint8_t)group_of_sp[i];
  __syncthreads();
}

/* (cell, group) bin of a record, or -1 for a record whose cell is off the grid (never indexed with) */
__device__ __forceinline__ int census_bin(c2d_u4 tg, const uint8_t* grp, int nz, int nr, int ngroup) {
  const int j = c2d_cens_j(tg.x), k = c2d_cens_k(tg.x);
  if (j < 1 || j > nz || k < 1 || k > nr) return -1;
  const int g = (int)grp[c2d_roulette_sp(tg.y)];
  return ((j - 1) * nr + (k - 1)) * ngroup + (g < ngroup ? g : ngroup - 1);
}

}  // namespace c2d

#endif /* C2D_POPCTL_HPP */
