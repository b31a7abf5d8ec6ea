/*
 * obsacc.hip — the exact observer set on gfx950 (include/compton2d.h "Exact
 * observer sets"): c2d_obs_set_kernel's pass over the escape
 * events with integer accumulators (c2d_obsacc.h), so a member's sums are
 * the same bits for any event order, batch split or shard count.
 *
 * Same structure as the f64 set kernel (observe.hip): one lane per event,
 * the event fetched once, wave-uniform member and band loops, the bin
 * decision of c2d_obsbin.h.  A bin is 5 u64 words, F_lo F_hi F2_lo F2_hi
 * count, in LDS for the privatised leading time rows and in global memory
 * (the member's accumulators, in the order of the exported state).  A
 * 128-bit add is a returning 64-bit atomic on the low limb, whose old value
 * tells whether this add wrapped it, and an atomic on the high limb that is
 * issued only when the addend's high part plus that carry is not zero:
 * every wrap is seen by exactly one add, so the two limbs are the exact
 * integer once the kernel has finished.  Later rows: lanes of a wave that
 * share a bin sum their addends first, as 32-bit limbs in u64 containers
 * (64 lanes x 2^32 fits), and one lane issues the atomics.
 */
#include "c2d_observe.hpp"
#include "c2d_obsacc.h"

namespace c2d {

__device__ inline uint64_t wave_sum_u64(uint64_t v) {
  for (int o = 32; o > 0; o >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, o, 64);
  return v;
}

/* (p[0], p[1]) += (lo, hi) as one 128-bit integer; LDS or global memory */
__device__ __forceinline__ void oax_add128(uint64_t* p, uint64_t lo, uint64_t hi) {
  if (lo) {
    const uint64_t old = atomicAdd((unsigned long long*)p, (unsigned long long)lo);
    hi += (uint64_t)(old + lo < old);
  }
  if (hi) atomicAdd((unsigned long long*)(p + 1), (unsigned long long)hi);
}

/* the sum over the wave's `mine` lanes of a value below 2^84 given as
 * (lo, hi): three 32-bit limbs, each summed in a u64, then recombined */
__device__ inline void oax_wave_sum128(bool mine, uint64_t& lo, uint64_t& hi) {
  const uint64_t s0 = wave_sum_u64(mine ? (lo & 0xffffffffull) : 0ull);
  const uint64_t s1 = wave_sum_u64(mine ? (lo >> 32) : 0ull);
  const uint64_t s2 = wave_sum_u64(mine ? hi : 0ull);
  lo = s0 + (s1 << 32);
  hi = (s1 >> 32) + s2 + (uint64_t)(lo < s0);
}

/* Wave-aggregated add to the global accumulators: every lane with h >= 0
 * adds its addends and 1 to bin h; lanes that share a bin are reduced first
 * and one lane per distinct bin issues the atomics (agg_add of observe.hip
 * on integers).  Called by all lanes of the wave together. */
__device__ inline void oax_agg(uint64_t* acc, int h, const c2d_oa_addend& a) {
  uint64_t pending = __ballot(h >= 0);
  const int lane = __lane_id();
  while (pending) {
    const int leader = __ffsll((unsigned long long)pending) - 1;
    const int hl = __shfl(h, leader, 64);
    const bool mine = (h == hl) && ((pending >> lane) & 1);
    const uint64_t m = __ballot(mine);
    c2d_oa_addend s = a;                   /* the leader is one of `mine` */
    if (__popcll(m) > 1) {                 /* wave-uniform */
      oax_wave_sum128(mine, s.f_lo, s.f_hi);
      oax_wave_sum128(mine, s.f2_lo, s.f2_hi);
    }
    if (lane == leader) {
      uint64_t* b = acc + (size_t)C2D_OA_BIN_WORDS * (size_t)hl;
      oax_add128(b, s.f_lo, s.f_hi);
      oax_add128(b + 2, s.f2_lo, s.f2_hi);
      atomicAdd((unsigned long long*)(b + 4), (unsigned long long)__popcll(m));
    }
    pending &= ~m;
  }
}

/* One event in one member: V is the member's view with hF = its LDS bins
 * (nl of them, 5 words each) and F = its global accumulators (5 words a
 * bin, then n_rejected).  An event whose weight is not accepted enters no
 * bin and is counted once, if a bin would have taken it. */
__device__ __forceinline__ void oax_bin_event(const ObsView& V, int e, const ObsEvent& ev, bool valid) {
  uint64_t* const hl = reinterpret_cast<uint64_t*>(V.hF);
  uint64_t* const acc = reinterpret_cast<uint64_t*>(V.F);
  bool bad = false;
  obs_decide(V, ev, valid, [&](int h, double w) {
    if (h >= 0 && !c2d_oa_accepts(w, e)) {
      bad = true;
      h = -1;
    }
    c2d_oa_addend a = {0ull, 0ull, 0ull, 0ull};
    if (h >= 0) a = c2d_oa_addend_of(w, e);
    if (h >= 0 && h < V.nl) {
      uint64_t* b = hl + C2D_OA_BIN_WORDS * h;
      oax_add128(b, a.f_lo, a.f_hi);
      oax_add128(b + 2, a.f2_lo, a.f2_hi);
      atomicAdd((unsigned long long*)(b + 4), 1ull);
    }
    oax_agg(acc, h >= V.nl ? h : -1, a);
  });
  const uint64_t nb = __ballot(bad);
  if (nb && __lane_id() == __ffsll((unsigned long long)nb) - 1)
    atomicAdd((unsigned long long*)(acc + (size_t)C2D_OA_BIN_WORDS * ((size_t)V.n_t * V.n_mu * V.n_e)),
              (unsigned long long)__popcll(nb));
}

/* the workgroup's non-zero LDS bins to global memory (after a __syncthreads) */
__device__ __forceinline__ void oax_flush(const ObsView& V) {
  const uint64_t* hl = reinterpret_cast<const uint64_t*>(V.hF);
  uint64_t* acc = reinterpret_cast<uint64_t*>(V.F);
  for (int i = threadIdx.x; i < V.nl; i += OBS_BLOCK) {
    const uint64_t* b = hl + C2D_OA_BIN_WORDS * i;
    if (b[4] != 0ull) {
      uint64_t* g = acc + (size_t)C2D_OA_BIN_WORDS * (size_t)i;
      oax_add128(g, b[0], b[1]);
      oax_add128(g + 2, b[2], b[3]);
      atomicAdd((unsigned long long*)(g + 4), (unsigned long long)b[4]);
    }
  }
}

/* The exact set: Q is the set's plan with 5 words per privatised bin
 * (obs_api.cpp obs_set_plan) and every member's F pointing at its integer
 * accumulators; X has the members' exponent bounds. */
__global__ void __launch_bounds__(OBS_BLOCK) c2d_obs_set_exact_kernel(const ObsSetDev Q, const ObsExactDev X,
                                                                       const ObsSegs S) {
  __shared__ ObsSegsLds L;
  __shared__ double betta_m[OBS_SET_MAX];
  obs_stage_segs(L, S);
  if (threadIdx.x < (unsigned)Q.n) betta_m[threadIdx.x] = obs_betta(Q.m[threadIdx.x].gam_bulk);
  const int64_t n = S.pre[S.nseg];
  extern __shared__ double sh[];
  obs_stage(sh, Q.edges, Q.n_edges);
  uint64_t* const hz = reinterpret_cast<uint64_t*>(sh + Q.n_edges);
  for (int i = threadIdx.x; i < Q.n_hist; i += OBS_BLOCK) hz[i] = 0ull;
  __syncthreads();
  /* wave-uniform trip counts (events, members, bands): every lane reaches oax_agg */
  for (int64_t base = (int64_t)blockIdx.x * OBS_BLOCK; base < n; base += (int64_t)gridDim.x * OBS_BLOCK) {
    const int64_t e = base + threadIdx.x;
    const bool valid = e < n;
    const ObsEvent ev = obs_fetch(L, S.nseg, valid ? e : 0);
    for (int j = 0; j < Q.n; j++)
      oax_bin_event(obs_view(Q.m[j], betta_m[j], sh + Q.m[j].edge_off, sh + Q.m[j].hist_off), X.e[j], ev, valid);
  }
  if (Q.n_hist) {
    __syncthreads();
    for (int j = 0; j < Q.n; j++) oax_flush(obs_view(Q.m[j], 0.0, sh + Q.m[j].edge_off, sh + Q.m[j].hist_off));
  }
}

/* acc += add, bin by bin with carry, and n_rejected (the word after the
 * bins) += rej: the import of c2d_obs_set_merge.  Nothing else touches the
 * accumulators meanwhile, and the host has checked that no sum carries out
 * of bit 127. */
__global__ void __launch_bounds__(256) c2d_obs_merge_kernel(uint64_t* acc, const uint64_t* add, int64_t nbins,
                                                            uint64_t rej) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < nbins) {
    uint64_t* a = acc + C2D_OA_BIN_WORDS * i;
    const uint64_t* b = add + C2D_OA_BIN_WORDS * i;
    (void)c2d_oa_add(&a[0], &a[1], b[0], b[1]);
    (void)c2d_oa_add(&a[2], &a[3], b[2], b[3]);
    a[4] += b[4];
  }
  if (i == 0) acc[C2D_OA_BIN_WORDS * nbins] += rej;
}

}  // namespace c2d

/* one launch of the exact set kernel over nseg event segments; its dynamic
 * LDS is the plan's (edges + privatised rows of 5 words a bin) */
extern "C" int c2d_launch_obs_set_exact(const c2d::ObsSetDev* Q, const c2d::ObsExactDev* X, const double* const* ev,
                                        const int64_t* n, int nseg, int grid, hipStream_t stream) {
  if (nseg < 1 || nseg > C2D_EV_SHARDS || Q->n < 1 || Q->n > c2d::OBS_SET_MAX) return (int)hipErrorInvalidValue;
  const size_t lds = sizeof(double) * ((size_t)Q->n_edges + (size_t)Q->n_hist);
  if (lds + c2d::OBS_SET_LDS_STATIC > (size_t)c2d::OBS_SET_LDS) return (int)hipErrorInvalidValue;
  for (int j = 0; j < Q->n; j++) {           /* every member's LDS ranges lie inside the allocation */
    const c2d::ObsSetMember& M = Q->m[j];
    if (M.n_t < 1 || M.n_mu < 1 || M.n_e < 1 || M.lds_rows < 0 || M.lds_rows > M.n_t || !M.F || !c2d_oa_e_ok(X->e[j]))
      return (int)hipErrorInvalidValue;
    const int64_t ne = 2 * ((int64_t)M.n_t + M.n_mu + M.n_e), nl = (int64_t)M.lds_rows * M.n_mu * M.n_e;
    if (M.edge_off < 0 || M.edge_off + ne > Q->n_edges || M.hist_off < Q->n_edges ||
        M.hist_off + C2D_OA_BIN_WORDS * nl > (int64_t)Q->n_edges + Q->n_hist)
      return (int)hipErrorInvalidValue;
  }
  c2d::ObsSegs S;
  if (!obs_segs(S, ev, n, nseg)) return 0;
  hipLaunchKernelGGL(c2d::c2d_obs_set_exact_kernel, dim3(grid), dim3(c2d::OBS_BLOCK), lds, stream, *Q, *X, S);
  return (int)hipGetLastError();
}

/* acc (5 nbins + 1 words) += add (5 nbins words), n_rejected += rej */
extern "C" int c2d_launch_obs_merge(uint64_t* acc, const uint64_t* add, int64_t nbins, uint64_t rej,
                                    hipStream_t stream) {
  if (!acc || !add || nbins < 1) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(c2d::c2d_obs_merge_kernel, dim3((unsigned)((nbins + 255) / 256)), dim3(256), 0, stream, acc, add,
                     nbins, rej);
  return (int)hipGetLastError();
}
