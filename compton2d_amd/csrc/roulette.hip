/*
 * roulette.hip — census population control on the device (include/compton2d.h
 * "Census population control"): the per-(cell, group) census
 * statistics a weight floor is made from, and the roulette pass that applies
 * the floors (c2d_roulette.h) and closes the holes.
 *
 * Both kernels stream the census once through its chunk list (cens_slot)
 * with the census stream's non-temporal accesses, 64-bit record indices
 * throughout, a workgroup taking tiles of RL_TILE records: a lane's RL_PER
 * records are RL_BLOCK apart, so every column access of a wave is
 * contiguous and a lane has RL_PER independent loads in flight.
 *
 * Stats reads the ex and tg columns only (32 of a record's 64 bytes).  Its
 * histogram (an f64 sum and a 32-bit count a bin) is private to the
 * workgroup in LDS while it fits (RL_STATS_LDS_MAX), in workgroups of 1024
 * threads so that two of them fill a CU, and is flushed once with global
 * atomics; a larger one (up to 99 x 99 cells x 32 groups) takes the global
 * atomics per record.
 *
 * The roulette pass works front to back in slices.  The decide kernel reads
 * ex and tg, applies the rule, and only a survivor's rz and wp are read: it
 * goes, with its new ew, to the scratch buffer at a position the workgroup
 * reserved with one atomic per tile (ballots within the waves, the waves'
 * counts through LDS) in the tile's region of the scratch (RL_SHARDS regions
 * with a counter each: c2d_roulette.hpp).  The unpack kernel stores the
 * regions' records one after the other at the write cursor, which never
 * passes the slice's start; a one-wave kernel moves the cursor on.  The
 * cursor and the regions' counts stay in device memory (RouletteCtl), so the
 * host does not wait between slices.  The order of the survivors is that of
 * the reservations: free, as the census's is.
 */
#include "c2d_roulette.hpp"

#include <algorithm>

namespace c2d {

static_assert(RL_SHARDS == 64, "a wave scans the regions' counts");
constexpr int RL_BLOCK = 256;
constexpr int RL_WAVES = RL_BLOCK / 64;
constexpr int RL_PER = 4;
static_assert(RL_TILE == RL_BLOCK * RL_PER, "a tile is a workgroup's records");
constexpr int RL_STATS_BLOCK_LDS = 1024;   /* threads of a stats workgroup with the histogram in LDS */

template <bool LDS, int BLOCK>
__global__ void __launch_bounds__(BLOCK)
c2d_census_stats_kernel(CensusSoA cs, const int32_t* __restrict__ clist, int64_t n, int nz, int nr, int ngroup,
                        const int32_t* __restrict__ group_of_sp, unsigned long long* __restrict__ count,
                        double* __restrict__ energy) {
  extern __shared__ double rl_hist[];
  __shared__ uint8_t grp[C2D_ROULETTE_NSP];
  const int nbins = nz * nr * ngroup;
  double* en_l = rl_hist;
  uint32_t* cnt_l = reinterpret_cast<uint32_t*>(rl_hist + nbins);   /* a workgroup sees fewer than 2^32 records */
  if (LDS)
    for (int b = (int)threadIdx.x; b < nbins; b += BLOCK) {
      cnt_l[b] = 0u;
      en_l[b] = 0.0;
    }
  census_load_groups(grp, group_of_sp);   /* ends in a barrier */
  constexpr int64_t TILE = (int64_t)BLOCK * RL_PER;
  const int64_t ntiles = (n + TILE - 1) / TILE;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t i0 = t * TILE + threadIdx.x;
    c2d_d2 ex[RL_PER];
    c2d_u4 tg[RL_PER];
#pragma unroll
    for (int r = 0; r < RL_PER; r++) {
      const int64_t i = i0 + (int64_t)r * BLOCK;
      if (i < n) {
        const int64_t slot = cens_slot(clist, i);
        ex[r] = cld2_nt(cs.ex + slot);
        tg[r] = cld4_nt(cs.tg + slot);
      }
    }
#pragma unroll
    for (int r = 0; r < RL_PER; r++) {
      const int64_t i = i0 + (int64_t)r * BLOCK;
      if (i >= n) continue;
      const int b = census_bin(tg[r], grp, nz, nr, ngroup);
      if (b < 0) continue;
      if (LDS) {
        __hip_atomic_fetch_add(&cnt_l[b], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __hip_atomic_fetch_add(&en_l[b], ex[r].x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      } else {
        gadd_u64(count + b, 1ull);
        gadd(energy + b, ex[r].x);
      }
    }
  }
  if (LDS) {
    __syncthreads();
    for (int b = (int)threadIdx.x; b < nbins; b += BLOCK)
      if (cnt_l[b]) {
        gadd_u64(count + b, (unsigned long long)cnt_l[b]);
        gadd(energy + b, en_l[b]);
      }
  }
}

/* PACK: survivors of census records [first, first + m) into the scratch
 * (columns rz | wp | ex | tg of cap entries each): those of tile t behind
 * the ones region t % RL_SHARDS holds, region s being entries
 * [s * region, (s + 1) * region) of every column.  Always: n_tested,
 * e_before, e_after. */
template <bool PACK>
__global__ void __launch_bounds__(RL_BLOCK)
c2d_roulette_decide_kernel(CensusSoA cs, const int32_t* __restrict__ clist, int64_t first, int64_t m, int nz, int nr,
                           int ngroup, const int32_t* __restrict__ group_of_sp, const double* __restrict__ w_min,
                           uint64_t salt, uint64_t* __restrict__ scratch, int64_t cap, int64_t region,
                           RouletteCtl* ctl) {
  __shared__ uint8_t grp[C2D_ROULETTE_NSP];
  __shared__ uint32_t wcnt[RL_WAVES];
  __shared__ unsigned long long tile_base;
  __shared__ double red_e[2 * RL_WAVES];
  __shared__ unsigned long long red_n[RL_WAVES];
  census_load_groups(grp, group_of_sp);
  c2d_d2* s_rz = reinterpret_cast<c2d_d2*>(scratch);
  c2d_d2* s_wp = s_rz + cap;
  c2d_d2* s_ex = s_wp + cap;
  c2d_u4* s_tg = reinterpret_cast<c2d_u4*>(s_ex + cap);
  const int lane = (int)threadIdx.x & 63, wv = (int)threadIdx.x >> 6;
  const unsigned long long below = (1ull << lane) - 1ull;
  double e_b = 0.0, e_a = 0.0;
  unsigned long long n_t = 0ull;
  const int64_t ntiles = (m + RL_TILE - 1) / RL_TILE;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {   /* the same trips for every thread of the workgroup */
    const int64_t i0 = t * RL_TILE + threadIdx.x;
    int64_t slot[RL_PER];
    c2d_d2 ex[RL_PER];
    c2d_u4 tg[RL_PER];
    bool keep[RL_PER];
#pragma unroll
    for (int r = 0; r < RL_PER; r++) {
      const int64_t i = i0 + (int64_t)r * RL_BLOCK;
      slot[r] = -1;
      if (i < m) {
        slot[r] = cens_slot(clist, first + i);
        ex[r] = cld2_nt(cs.ex + slot[r]);
        tg[r] = cld4_nt(cs.tg + slot[r]);
      }
    }
#pragma unroll
    for (int r = 0; r < RL_PER; r++) {
      keep[r] = false;
      if (slot[r] < 0) continue;
      const int b = census_bin(tg[r], grp, nz, nr, ngroup);
      const double ew = ex[r].x;
      double ew_new = ew;
      int what = C2D_ROULETTE_UNTOUCHED;
      if (b >= 0) what = c2d_roulette_decide(ew, w_min[b], c2d_tg_key(tg[r]), salt, &ew_new);
      keep[r] = what != C2D_ROULETTE_REMOVED;
      n_t += what != C2D_ROULETTE_UNTOUCHED ? 1ull : 0ull;
      e_b += ew;
      if (keep[r]) e_a += ew_new;
      ex[r].x = ew_new;
    }
    if (PACK) {
      const int shard = (int)(t % RL_SHARDS);
      unsigned long long bal[RL_PER];
      uint32_t mine = 0u;
#pragma unroll
      for (int r = 0; r < RL_PER; r++) {
        bal[r] = __ballot(keep[r]);
        mine += (uint32_t)__popcll(bal[r]);
      }
      if (lane == 0) wcnt[wv] = mine;
      __syncthreads();
      if (threadIdx.x == 0) {
        uint32_t tot = 0u;
#pragma unroll
        for (int w = 0; w < RL_WAVES; w++) tot += wcnt[w];
        tile_base = tot ? gadd_u64(&ctl->cnt[shard * RL_SHARD_STRIDE], (unsigned long long)tot) : 0ull;
      }
      __syncthreads();
      unsigned long long pos = tile_base;
      for (int w = 0; w < wv; w++) pos += wcnt[w];
#pragma unroll
      for (int r = 0; r < RL_PER; r++) {
        if (keep[r]) {
          const int64_t q = (int64_t)(pos + (unsigned long long)__popcll(bal[r] & below));
          const int64_t p = (int64_t)shard * region + q;
          if (q < region && p < cap) {   /* a region's survivors <= its tiles' records = region */
            const c2d_d2 rz = cld2_nt(cs.rz + slot[r]), wp = cld2_nt(cs.wp + slot[r]);
            cst2(s_rz + p, rz.x, rz.y);
            cst2(s_wp + p, wp.x, wp.y);
            cst2(s_ex + p, ex[r].x, ex[r].y);
            cst4(s_tg + p, tg[r].x, tg[r].y, c2d_tg_key(tg[r]));
          }
        }
        pos += (unsigned long long)__popcll(bal[r]);
      }
      __syncthreads();   /* wcnt and tile_base are the next tile's */
    }
  }
  /* the workgroup's sums: shuffles within a wave, the waves through LDS, one atomic each */
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    e_b += __shfl_xor(e_b, o, 64);
    e_a += __shfl_xor(e_a, o, 64);
    n_t += __shfl_xor(n_t, o, 64);
  }
  if (lane == 0) {
    red_e[2 * wv] = e_b;
    red_e[2 * wv + 1] = e_a;
    red_n[wv] = n_t;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double sb = 0.0, sa = 0.0;
    unsigned long long sn = 0ull;
#pragma unroll
    for (int w = 0; w < RL_WAVES; w++) {
      sb += red_e[2 * w];
      sa += red_e[2 * w + 1];
      sn += red_n[w];
    }
    gadd(&ctl->e_before, sb);
    gadd(&ctl->e_after, sa);
    if (sn) gadd_u64(&ctl->n_tested, sn);
  }
}

/* the slice's survivors from the scratch's regions, one after the other, to
 * census records [W, W + their number); limit = the end of the slice they
 * were read from */
__global__ void __launch_bounds__(RL_BLOCK)
c2d_roulette_unpack_kernel(CensusSoA cs, const int32_t* __restrict__ clist, const uint64_t* __restrict__ scratch,
                           int64_t cap, int64_t region, int64_t limit, const RouletteCtl* __restrict__ ctl) {
  __shared__ int64_t off[RL_SHARDS + 1];   /* exclusive prefix of the regions' counts */
  if (threadIdx.x < RL_SHARDS) {   /* the first wave: a lane a region, an inclusive scan with shuffles */
    const int s = (int)threadIdx.x;
    int64_t c = (int64_t)ctl->cnt[s * RL_SHARD_STRIDE];
    c = c < region ? c : region;
    int64_t a = c;
#pragma unroll
    for (int o = 1; o < RL_SHARDS; o <<= 1) {
      const int64_t up = __shfl_up(a, o, 64);
      if (s >= o) a += up;
    }
    off[s + 1] = a;
    if (s == 0) off[0] = 0;
  }
  __syncthreads();
  const int64_t W = (int64_t)ctl->W, cnt = off[RL_SHARDS];
  if ((int64_t)RL_SHARDS * region > cap || W + cnt > limit) return;   /* never: survivors <= records read */
  const c2d_d2* s_rz = reinterpret_cast<const c2d_d2*>(scratch);
  const c2d_d2* s_wp = s_rz + cap;
  const c2d_d2* s_ex = s_wp + cap;
  const c2d_u4* s_tg = reinterpret_cast<const c2d_u4*>(s_ex + cap);
  for (int64_t i = blockIdx.x * (int64_t)RL_BLOCK + threadIdx.x; i < cnt; i += (int64_t)gridDim.x * RL_BLOCK) {
    int s = 0;   /* the region that holds survivor i: the last with off[s] <= i */
#pragma unroll
    for (int h = RL_SHARDS / 2; h > 0; h >>= 1)
      if (off[s + h] <= i) s += h;
    const int64_t p = (int64_t)s * region + (i - off[s]);
    const int64_t slot = cens_slot(clist, W + i);
    const c2d_d2 rz = cld2(s_rz + p), wp = cld2(s_wp + p), ex = cld2(s_ex + p);
    const c2d_u4 tg = cld4(s_tg + p);
    cst2_nt(cs.rz + slot, rz.x, rz.y);
    cst2_nt(cs.wp + slot, wp.x, wp.y);
    cst2_nt(cs.ex + slot, ex.x, ex.y);
    cst4_nt(cs.tg + slot, tg.x, tg.y, c2d_tg_key(tg));
  }
}

/* after a slice's unpack (one wave): the cursor moves on, the regions are empty */
__global__ void __launch_bounds__(RL_SHARDS) c2d_roulette_advance_kernel(RouletteCtl* ctl, int64_t region) {
  const int s = (int)threadIdx.x;
  unsigned long long c = ctl->cnt[s * RL_SHARD_STRIDE];
  if (c > (unsigned long long)region) c = (unsigned long long)region;
  ctl->cnt[s * RL_SHARD_STRIDE] = 0ull;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  if (s == 0) ctl->W += c;
}

}  // namespace c2d

using namespace c2d;

extern "C" int c2d_launch_census_stats(const CensusPass& p, unsigned long long* count, double* energy) {
  if (p.n <= 0) return 0;
  const size_t lds = (size_t)p.nz * p.nr * p.ngroup * (sizeof(double) + sizeof(uint32_t));
  if (lds <= RL_STATS_LDS_MAX) {
    /* two resident workgroups a CU; each sees n / grid + a tile < 2^32 records */
    const unsigned grid = std::max(census_grid(p.n, (int64_t)RL_STATS_BLOCK_LDS * RL_PER, p.n_cu, 2),
                                   (unsigned)(p.n >> 31) + 1u);
    hipLaunchKernelGGL((c2d_census_stats_kernel<true, RL_STATS_BLOCK_LDS>), dim3(grid), dim3(RL_STATS_BLOCK_LDS), lds,
                       p.stream, p.cs, p.clist, p.n, p.nz, p.nr, p.ngroup, p.group_of_sp, count, energy);
  } else {
    hipLaunchKernelGGL((c2d_census_stats_kernel<false, RL_BLOCK>), dim3(census_grid(p.n, RL_TILE, p.n_cu, 8)),
                       dim3(RL_BLOCK), 0, p.stream, p.cs, p.clist, p.n, p.nz, p.nr, p.ngroup, p.group_of_sp, count,
                       energy);
  }
  return (int)hipGetLastError();
}

extern "C" int c2d_launch_roulette_slice(const CensusPass& p, int64_t first, int64_t m, const double* w_min,
                                         uint64_t salt, uint64_t* scratch, int64_t cap, RouletteCtl* ctl, int pack) {
  if (m <= 0) return 0;
  const unsigned grid = census_grid(m, RL_TILE, p.n_cu, 8);
  const hipStream_t s = p.stream;
  if (!pack) {
    hipLaunchKernelGGL(c2d_roulette_decide_kernel<false>, dim3(grid), dim3(RL_BLOCK), 0, s, p.cs, p.clist, first, m,
                       p.nz, p.nr, p.ngroup, p.group_of_sp, w_min, salt, scratch, cap, (int64_t)0, ctl);
    return (int)hipGetLastError();
  }
  const int64_t region = rl_region(m);
  if ((int64_t)RL_SHARDS * region > cap) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(c2d_roulette_decide_kernel<true>, dim3(grid), dim3(RL_BLOCK), 0, s, p.cs, p.clist, first, m, p.nz,
                     p.nr, p.ngroup, p.group_of_sp, w_min, salt, scratch, cap, region, ctl);
  hipLaunchKernelGGL(c2d_roulette_unpack_kernel, dim3(grid), dim3(RL_BLOCK), 0, s, p.cs, p.clist, scratch, cap, region,
                     first + m, ctl);
  hipLaunchKernelGGL(c2d_roulette_advance_kernel, dim3(1), dim3(RL_SHARDS), 0, s, ctl, region);
  return (int)hipGetLastError();
}
