/*
 * split.hip — census splitting on the device (include/compton2d.h "Census
 * splitting"): the upper weight window.  A record heavier than
 * its (cell, group)'s ceiling becomes m records of weight ew / m
 * (c2d_split.h); the census grows in place.
 *
 * Three kernels, all over tiles of SP_TILE records, a lane's SP_PER records
 * SP_BLOCK apart so that every column access of a wave is contiguous, 64-bit
 * item indices, the census stream's non-temporal accesses:
 *
 *   count   reads ex and tg (32 of a record's 64 bytes), writes a tile's
 *           number of extra copies sum (m - 1) (at most 1024 * 63: a u32) and
 *           sums n_split, e_before, e_after: one atomic each a workgroup.
 *   scan    the exclusive 64-bit prefix of the tiles' counts: one workgroup,
 *           strips of up to SP_SCAN_STRIP tiles, the carry in a register.
 *   expand  skips a tile without a split record on its count alone.  Else it
 *           recomputes m (a division is cheaper than a stored array), scans
 *           (m - 1) over the tile's records (wave scans, the waves' sums
 *           through LDS) and keeps the records' ex and tg words in LDS.  A
 *           split record rewrites its own ex column.  The copies are written
 *           output-parallel: the tile's threads walk the output slots
 *           o < tile_extra, each finds its source record by bisection on the
 *           tile's prefix in LDS, derives its key and stores the four columns
 *           at item n + off[tile] + o.  Consecutive lanes write consecutive
 *           items whatever the m of the single records; neighbouring slots
 *           share a source, so the rz and wp loads broadcast.  No atomics, no
 *           scratch copy, no second pass over the copies.
 *
 * The originals stay at their items, the copies follow at [n, n_after) in
 * (source item, i) order: the result is a function of the census, the
 * ceilings, max_copies and the salt alone.  Nothing the pass reads is ever
 * written by another thread: originals' ex by their own lane only (the
 * copies take it from LDS), copies at items the pass never reads.
 */
#include "c2d_split.hpp"

#include <algorithm>

namespace c2d {

constexpr int SP_BLOCK = 256;
constexpr int SP_WAVES = SP_BLOCK / 64;
constexpr int SP_PER = 4;
static_assert(SP_TILE == SP_BLOCK * SP_PER, "a tile is a workgroup's records");
static_assert(C2D_SPLIT_COPIES_MAX * SP_TILE < (1ll << 32), "a tile's extras fit a u32");

/* m of a record and the weight of each of its m copies */
__device__ __forceinline__ int sp_copies(c2d_d2 ex, c2d_u4 tg, const uint8_t* grp, int nz, int nr, int ngroup,
                                         const double* __restrict__ w_max, int max_copies, double* ew_new) {
  const int b = census_bin(tg, grp, nz, nr, ngroup);
  *ew_new = ex.x;
  return b >= 0 ? c2d_split_copies(ex.x, w_max[b], max_copies, ew_new) : 1;
}

__global__ void __launch_bounds__(SP_BLOCK)
c2d_split_count_kernel(CensusSoA cs, const int32_t* __restrict__ clist, int64_t n, int nz, int nr, int ngroup,
                       const int32_t* __restrict__ group_of_sp, const double* __restrict__ w_max, int max_copies,
                       uint32_t* __restrict__ cnt, SplitCtl* ctl) {
  __shared__ uint8_t grp[C2D_ROULETTE_NSP];
  __shared__ uint32_t wext[SP_WAVES];
  __shared__ double red_e[2 * SP_WAVES];
  __shared__ unsigned long long red_n[SP_WAVES];
  census_load_groups(grp, group_of_sp);
  const int lane = (int)threadIdx.x & 63, wv = (int)threadIdx.x >> 6;
  double e_b = 0.0, e_a = 0.0;
  unsigned long long n_s = 0ull;
  const int64_t ntiles = (n + SP_TILE - 1) / SP_TILE;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {   /* the same trips for every thread of the workgroup */
    const int64_t i0 = t * SP_TILE + threadIdx.x;
    c2d_d2 ex[SP_PER];
    c2d_u4 tg[SP_PER];
#pragma unroll
    for (int r = 0; r < SP_PER; r++) {
      const int64_t i = i0 + (int64_t)r * SP_BLOCK;
      if (i < n) {
        const int64_t slot = cens_slot(clist, i);
        ex[r] = cld2_nt(cs.ex + slot);
        tg[r] = cld4_nt(cs.tg + slot);
      }
    }
    uint32_t extra = 0u;
#pragma unroll
    for (int r = 0; r < SP_PER; r++) {
      const int64_t i = i0 + (int64_t)r * SP_BLOCK;
      if (i >= n) continue;
      double ew_new;
      const int m = sp_copies(ex[r], tg[r], grp, nz, nr, ngroup, w_max, max_copies, &ew_new);
      extra += (uint32_t)(m - 1);
      n_s += m > 1 ? 1ull : 0ull;
      e_b += ex[r].x;
      e_a += m > 1 ? (double)m * ew_new : ex[r].x;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) extra += __shfl_xor(extra, o, 64);
    if (lane == 0) wext[wv] = extra;
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t tot = 0u;
#pragma unroll
      for (int w = 0; w < SP_WAVES; w++) tot += wext[w];
      cnt[t] = tot;
    }
    __syncthreads();   /* wext is the next tile's */
  }
  /* the workgroup's sums: shuffles within a wave, the waves through LDS, one atomic each */
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    e_b += __shfl_xor(e_b, o, 64);
    e_a += __shfl_xor(e_a, o, 64);
    n_s += __shfl_xor(n_s, o, 64);
  }
  if (lane == 0) {
    red_e[2 * wv] = e_b;
    red_e[2 * wv + 1] = e_a;
    red_n[wv] = n_s;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double sb = 0.0, sa = 0.0;
    unsigned long long sn = 0ull;
#pragma unroll
    for (int w = 0; w < SP_WAVES; w++) {
      sb += red_e[2 * w];
      sa += red_e[2 * w + 1];
      sn += red_n[w];
    }
    gadd(&ctl->e_before, sb);
    gadd(&ctl->e_after, sa);
    if (sn) gadd_u64(&ctl->n_split, sn);
  }
}

/* one workgroup: strip after strip of `strip` tiles, a thread SP_SCAN_PER
 * neighbouring tiles, an inclusive scan with shuffles within a wave, the
 * waves' sums through LDS, the strips' carry in a register of every thread */
__global__ void __launch_bounds__(SP_SCAN_BLOCK)
c2d_split_scan_kernel(const uint32_t* __restrict__ cnt, int64_t ntiles, int64_t strip, int64_t* __restrict__ off,
                      SplitCtl* ctl) {
  constexpr int NW = SP_SCAN_BLOCK / 64;
  __shared__ int64_t wsum[NW];
  const int lane = (int)threadIdx.x & 63, wv = (int)threadIdx.x >> 6;
  int64_t carry = 0;
  for (int64_t base = 0; base < ntiles; base += strip) {
    const int64_t end = base + strip < ntiles ? base + strip : ntiles;
    const int64_t i0 = base + (int64_t)threadIdx.x * SP_SCAN_PER;
    uint32_t v[SP_SCAN_PER];
    int64_t mine = 0;
#pragma unroll
    for (int r = 0; r < SP_SCAN_PER; r++) {
      v[r] = i0 + r < end ? cnt[i0 + r] : 0u;
      mine += (int64_t)v[r];
    }
    int64_t a = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int64_t up = __shfl_up(a, o, 64);
      if (lane >= o) a += up;
    }
    if (lane == 63) wsum[wv] = a;
    __syncthreads();
    int64_t before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < NW; w++) {
      const int64_t sw = wsum[w];
      before += w < wv ? sw : 0;
      all += sw;
    }
    int64_t x = carry + before + a - mine;
#pragma unroll
    for (int r = 0; r < SP_SCAN_PER; r++) {
      if (i0 + r < end) off[i0 + r] = x;
      x += (int64_t)v[r];
    }
    carry += all;
    __syncthreads();   /* wsum is the next strip's */
  }
  if (threadIdx.x == 0) ctl->n_extra = (unsigned long long)carry;
}

__global__ void __launch_bounds__(SP_BLOCK)
c2d_split_expand_kernel(CensusSoA cs, const int32_t* __restrict__ clist, int64_t n, int64_t n_after, int nz, int nr,
                        int ngroup, const int32_t* __restrict__ group_of_sp, const double* __restrict__ w_max,
                        int max_copies, uint64_t salt, const uint32_t* __restrict__ cnt,
                        const int64_t* __restrict__ off) {
  __shared__ uint8_t grp[C2D_ROULETTE_NSP];
  __shared__ uint32_t wsum[SP_PER][SP_WAVES];
  __shared__ uint32_t pre[SP_TILE];   /* copies asked for by the tile's records before this one */
  __shared__ c2d_d2 l_ex[SP_TILE];    /* the records' ex (ew already the copies') and tg words */
  __shared__ c2d_u4 l_tg[SP_TILE];
  census_load_groups(grp, group_of_sp);
  const int lane = (int)threadIdx.x & 63, wv = (int)threadIdx.x >> 6;
  const int64_t ntiles = (n + SP_TILE - 1) / SP_TILE;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {   /* the same trips for every thread of the workgroup */
    const uint32_t tile_extra = cnt[t];
    if (tile_extra == 0u) continue;   /* no split record: the tile is not even read */
    const int64_t i0 = t * SP_TILE + threadIdx.x;
    int64_t slot[SP_PER];
    c2d_d2 ex[SP_PER];
    c2d_u4 tg[SP_PER];
#pragma unroll
    for (int r = 0; r < SP_PER; r++) {
      const int64_t i = i0 + (int64_t)r * SP_BLOCK;
      slot[r] = -1;
      if (i < n) {
        slot[r] = cens_slot(clist, i);
        ex[r] = cld2_nt(cs.ex + slot[r]);
        tg[r] = cld4_nt(cs.tg + slot[r]);
      }
    }
    uint32_t e[SP_PER], a[SP_PER];
#pragma unroll
    for (int r = 0; r < SP_PER; r++) {
      e[r] = 0u;
      if (slot[r] >= 0) {
        double ew_new;
        const int m = sp_copies(ex[r], tg[r], grp, nz, nr, ngroup, w_max, max_copies, &ew_new);
        e[r] = (uint32_t)(m - 1);
        if (m > 1) {
          ex[r].x = ew_new;
          cst2_nt(cs.ex + slot[r], ex[r].x, ex[r].y);   /* copy 0: the record itself */
        }
        l_ex[r * SP_BLOCK + (int)threadIdx.x] = ex[r];
        l_tg[r * SP_BLOCK + (int)threadIdx.x] = tg[r];
      }
      /* record r * SP_BLOCK + thread of the tile: the inclusive scan within its wave */
      a[r] = e[r];
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = __shfl_up(a[r], o, 64);
        if (lane >= o) a[r] += up;
      }
      if (lane == 63) wsum[r][wv] = a[r];
    }
    __syncthreads();
    {
      uint32_t run = 0u;   /* the copies of the (r, wave) blocks before this thread's, r by r */
#pragma unroll
      for (int r = 0; r < SP_PER; r++) {
        uint32_t mine = run;
#pragma unroll
        for (int w = 0; w < SP_WAVES; w++) {
          const uint32_t sw = wsum[r][w];
          mine += w < wv ? sw : 0u;
          run += sw;
        }
        pre[r * SP_BLOCK + (int)threadIdx.x] = mine + a[r] - e[r];
      }
    }
    __syncthreads();
    const int64_t first = n + off[t];
    for (uint32_t o = threadIdx.x; o < tile_extra; o += SP_BLOCK) {
      int s = 0;   /* the source record: the last with pre[s] <= o (the ones without copies before it share its pre) */
#pragma unroll
      for (int h = SP_TILE / 2; h > 0; h >>= 1)
        if (pre[s + h] <= o) s += h;
      const int64_t item = first + (int64_t)o;
      const int64_t src_i = t * SP_TILE + s;
      if (item >= n_after || src_i >= n) continue;   /* never: the counts are the count kernel's */
      const int64_t src = cens_slot(clist, src_i), dst = cens_slot(clist, item);
      const c2d_d2 rz = cld2(cs.rz + src), wp = cld2(cs.wp + src), exs = l_ex[s];
      const c2d_u4 tgs = l_tg[s];
      const uint64_t key = c2d_split_key(c2d_tg_key(tgs), salt, (int)(o - pre[s]) + 1);
      cst2_nt(cs.rz + dst, rz.x, rz.y);
      cst2_nt(cs.wp + dst, wp.x, wp.y);
      cst2_nt(cs.ex + dst, exs.x, exs.y);
      cst4_nt(cs.tg + dst, tgs.x, tgs.y, key);
    }
    __syncthreads();   /* wsum, pre, l_ex and l_tg are the next tile's */
  }
}

}  // namespace c2d

using namespace c2d;

extern "C" int c2d_launch_split_count(const CensusPass& p, const double* w_max, int max_copies, uint32_t* cnt,
                                      SplitCtl* ctl) {
  if (p.n <= 0) return 0;
  hipLaunchKernelGGL(c2d_split_count_kernel, dim3(census_grid(p.n, SP_TILE, p.n_cu, 8)), dim3(SP_BLOCK), 0, p.stream,
                     p.cs, p.clist, p.n, p.nz, p.nr, p.ngroup, p.group_of_sp, w_max, max_copies, cnt, ctl);
  return (int)hipGetLastError();
}

extern "C" int c2d_launch_split_scan(const uint32_t* cnt, int64_t ntiles, int64_t strip, int64_t* off, SplitCtl* ctl,
                                     hipStream_t s) {
  if (ntiles <= 0) return 0;
  strip = std::max<int64_t>(1, std::min<int64_t>(strip, SP_SCAN_STRIP));
  hipLaunchKernelGGL(c2d_split_scan_kernel, dim3(1), dim3(SP_SCAN_BLOCK), 0, s, cnt, ntiles, strip, off, ctl);
  return (int)hipGetLastError();
}

extern "C" int c2d_launch_split_expand(const CensusPass& p, int64_t n_after, const double* w_max, int max_copies,
                                       uint64_t salt, const uint32_t* cnt, const int64_t* off) {
  if (p.n <= 0 || n_after <= p.n) return 0;
  /* 36 KB of LDS a workgroup: four of them, 16 waves, a CU */
  hipLaunchKernelGGL(c2d_split_expand_kernel, dim3(census_grid(p.n, SP_TILE, p.n_cu, 4)), dim3(SP_BLOCK), 0, p.stream,
                     p.cs, p.clist, p.n, n_after, p.nz, p.nr, p.ngroup, p.group_of_sp, w_max, max_copies, salt, cnt,
                     off);
  return (int)hipGetLastError();
}
