/*
 * comb.hip — the census comb on the device (include/compton2d.h "Census
 * comb"): the digit histogram and the collection of the
 * normalised critical values (c2d_comb.h) a most-significant-digit search
 * for the k-th largest of them is made of.  The census is only read.
 *
 * One kernel, the stats kernel's streaming skeleton (roulette.hip): the ex
 * and tg columns through the chunk list with non-temporal loads, 64-bit
 * record indices, a workgroup taking tiles of CB_TILE records, a lane's
 * CB_PER records CB_BLOCK apart.  Per record: the derived key (Philox4x32-10),
 * its draw (SplitMix64), the critical-floor search (two to four f64
 * divisions) and the digit.
 *
 * HIST bins the digits of the matching records into a 2048 x u32 histogram
 * private to the workgroup in LDS (8 KB), flushed once with global atomics
 * into the u64 histogram.  In the first pass the digit is sign and exponent,
 * and a wave's 64 records fall into a handful of bins (14 for the C3 census),
 * so their LDS atomics meet on one address.  That was measured not to matter
 * beside the arithmetic: at 1e8 records the first pass takes 0.93 ms, as the
 * later ones do, and counting the lanes of equal digit with ballots so that
 * one lane adds their number made it slower, 1.07 ms.
 *
 * COLLECT appends the matching values to `vals`, a wave reserving its places
 * with one atomic; places at or past `cap` are counted and not written.
 */
#include "c2d_comb.hpp"

#include <algorithm>

namespace c2d {

constexpr int CB_BLOCK = 256;
constexpr int CB_WAVES = CB_BLOCK / 64;
constexpr int CB_PER = 4;
constexpr int CB_TILE = CB_BLOCK * CB_PER;

template <bool COLLECT>
__global__ void __launch_bounds__(CB_BLOCK)
c2d_census_comb_kernel(CensusSoA cs, const int32_t* __restrict__ clist, int64_t n, int nz, int nr, int ngroup,
                       const int32_t* __restrict__ group_of_sp, const double* __restrict__ norm, uint64_t salt,
                       uint64_t prefix, int prefix_bits, unsigned long long* __restrict__ hist,
                       double* __restrict__ vals, int64_t cap, CombCtl* ctl) {
  __shared__ uint32_t hist_l[COLLECT ? 1 : C2D_COMB_BINS];   /* a workgroup sees fewer than 2^32 records */
  __shared__ uint8_t grp[C2D_ROULETTE_NSP];
  __shared__ unsigned long long red[2 * CB_WAVES];
  if (!COLLECT)
    for (int b = (int)threadIdx.x; b < C2D_COMB_BINS; b += CB_BLOCK) hist_l[b] = 0u;
  for (int i = (int)threadIdx.x; i < C2D_ROULETTE_NSP; i += CB_BLOCK) grp[i] = (uint8_t)group_of_sp[i];
  __syncthreads();
  const int lane = (int)threadIdx.x & 63, wv = (int)threadIdx.x >> 6;
  const unsigned long long below = (1ull << lane) - 1ull;
  unsigned long long n_fixed = 0ull, n_match = 0ull;
  const int64_t ntiles = (n + CB_TILE - 1) / CB_TILE;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {   /* the same trips for every thread of the workgroup */
    const int64_t i0 = t * CB_TILE + threadIdx.x;
    c2d_d2 ex[CB_PER];
    c2d_u4 tg[CB_PER];
#pragma unroll
    for (int r = 0; r < CB_PER; r++) {
      const int64_t i = i0 + (int64_t)r * CB_BLOCK;
      if (i < n) {
        const int64_t slot = cens_slot(clist, i);
        ex[r] = cld2_nt(cs.ex + slot);
        tg[r] = cld4_nt(cs.tg + slot);
      }
    }
#pragma unroll
    for (int r = 0; r < CB_PER; r++) {
      const int64_t i = i0 + (int64_t)r * CB_BLOCK;
      bool match = false;
      uint64_t cb = 0ull;
      if (i < n) {
        const int j = c2d_cens_j(tg[r].x), k = c2d_cens_k(tg[r].x);
        const bool on_grid = j >= 1 && j <= nz && k >= 1 && k <= nr;
        double nm = 0.0;
        if (on_grid) {
          const int g = (int)grp[c2d_roulette_sp(tg[r].y)];
          nm = norm[((j - 1) * nr + (k - 1)) * ngroup + (g < ngroup ? g : ngroup - 1)];
        }
        const double ew = ex[r].x;
        if (c2d_comb_fixed(ew, nm, on_grid)) {
          n_fixed++;
        } else {
          cb = c2d_roulette_bits(c2d_comb_critical(ew, nm, c2d_tg_key(tg[r]), salt));
          match = c2d_comb_match(cb, prefix, prefix_bits);
        }
      }
      n_match += match ? 1ull : 0ull;
      if (COLLECT) {
        /* every lane of the wave is here: i < n only guards the record's own work */
        const unsigned long long bal = __ballot(match);
        unsigned long long base = 0ull;
        if (bal) {
          const int lead = __ffsll((long long)bal) - 1;
          if (lane == lead) base = gadd_u64(&ctl->n_collect, (unsigned long long)__popcll(bal));
          base = __shfl(base, lead, 64);
        }
        if (match) {
          const int64_t p = (int64_t)(base + (unsigned long long)__popcll(bal & below));
          if (p < cap) vals[p] = c2d_comb_from_bits(cb);
        }
      } else {
        /* the digit is < C2D_COMB_BINS whatever cb is */
        if (match)
          __hip_atomic_fetch_add(&hist_l[c2d_comb_digit(cb, prefix_bits)], 1u, __ATOMIC_RELAXED,
                                 __HIP_MEMORY_SCOPE_WORKGROUP);
      }
    }
  }
  /* the workgroup's counts: shuffles within a wave, the waves through LDS, one atomic each */
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    n_fixed += __shfl_xor(n_fixed, o, 64);
    n_match += __shfl_xor(n_match, o, 64);
  }
  if (lane == 0) {
    red[2 * wv] = n_fixed;
    red[2 * wv + 1] = n_match;
  }
  __syncthreads();   /* also: the LDS histogram is complete */
  if (threadIdx.x == 0) {
    unsigned long long sf = 0ull, sm = 0ull;
#pragma unroll
    for (int w = 0; w < CB_WAVES; w++) {
      sf += red[2 * w];
      sm += red[2 * w + 1];
    }
    if (sf) gadd_u64(&ctl->n_fixed, sf);
    if (sm) gadd_u64(&ctl->n_match, sm);
  }
  if (!COLLECT)
    for (int b = (int)threadIdx.x; b < C2D_COMB_BINS; b += CB_BLOCK)
      if (hist_l[b]) gadd_u64(hist + b, (unsigned long long)hist_l[b]);
}

}  // namespace c2d

using namespace c2d;

extern "C" int c2d_launch_census_comb(const CensusPass& p, const double* norm, uint64_t salt, uint64_t prefix,
                                      int prefix_bits, unsigned long long* hist, double* vals, int64_t cap,
                                      CombCtl* ctl, int grid_cap) {
  if (p.n <= 0) return 0;
  int64_t grid = census_grid(p.n, CB_TILE, p.n_cu, 8);
  if (grid_cap > 0) grid = std::min<int64_t>(grid, grid_cap);
  grid = std::max<int64_t>(grid, (p.n >> 31) + 1);   /* a workgroup's u32 counts: n / grid + a tile < 2^32 records */
  if (hist)
    hipLaunchKernelGGL(c2d_census_comb_kernel<false>, dim3((unsigned)grid), dim3(CB_BLOCK), 0, p.stream, p.cs, p.clist,
                       p.n, p.nz, p.nr, p.ngroup, p.group_of_sp, norm, salt, prefix, prefix_bits, hist, vals, cap, ctl);
  else
    hipLaunchKernelGGL(c2d_census_comb_kernel<true>, dim3((unsigned)grid), dim3(CB_BLOCK), 0, p.stream, p.cs, p.clist,
                       p.n, p.nz, p.nr, p.ngroup, p.group_of_sp, norm, salt, prefix, prefix_bits, hist, vals, cap, ctl);
  return (int)hipGetLastError();
}
