/*
 * observe.hip — observer-frame binning of escape events on gfx950
 * (SURVEY.md §8(f)#3): the loops of the reference's post-processing tools
 * postprocessing/pspt.c:245-294 (SED: time x energy, one angular window) and
 * postprocessing/plcm.c:382-456 (light curves: time x angular bins x
 * possibly overlapping energy bands, with sum of ew^2), run on the device's
 * escape-event buffer so the 105-byte ASCII event lines (imcleak2d.f:171,
 * format 105) need not be written and re-parsed.
 *
 * One lane per event: Lorentz boost with the bulk factor, light-travel time,
 * bin search over LDS-staged edges (the tools' first-match semantics; a
 * binary search when the edges are sorted, else their linear scan), then
 * accumulation.  The leading time rows of the histogram that fit in LDS
 * (all of them for a pspt SED; ~290 of plcm's 1024 rows) are privatised per
 * workgroup and flushed with one global atomic per non-zero bin; events in
 * later rows use wave-aggregated global atomics (one atomic per distinct bin
 * per wave), so hot bins never serialise lane by lane.  The event stream is
 * read once: 56 B per event (HBM-bound).
 *
 * c2d_obs_set_kernel fills several such histograms (an observer set: SEDs of
 * several windows and light curves, c2d_obs_set_*) in one pass: the event
 * words and cos(phi) are shared, the members share the workgroup's LDS.
 */
#include "c2d_observe.hpp"

namespace c2d {

__device__ inline double wave_sum(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

/* Wave-aggregated histogram add: every lane with h >= 0 adds (w, w^2, 1) to
 * bin h.  Lanes that share a bin are reduced first and one lane per distinct
 * bin issues the atomics, so a hot bin costs one atomic per wave instead of
 * one per lane (hot bins are the norm: most events fall in a few time bins).
 * Called by all lanes of the wave together. */
__device__ inline void agg_add(double* F, double* F2, double* C, int h, double w) {
  uint64_t pending = __ballot(h >= 0);
  const int lane = __lane_id();
  while (pending) {
    const int leader = __ffsll((unsigned long long)pending) - 1;
    const int hl = __shfl(h, leader, 64);
    const bool mine = (h == hl) && ((pending >> lane) & 1);
    const uint64_t m = __ballot(mine);
    const double s = wave_sum(mine ? w : 0.0);
    const double s2 = wave_sum(mine ? w * w : 0.0);
    if (lane == leader) {
      atomicAdd(&F[hl], s);
      atomicAdd(&F2[hl], s2);
      atomicAdd(&C[hl], (double)__popcll(m));
    }
    pending &= ~m;
  }
}

/* LDS bins: plain per-lane LDS atomics; the rest: wave-aggregated global
 * atomics.  Every lane of the wave calls it (h = -1: nothing to add). */
__device__ __forceinline__ void obs_add(const ObsView& V, int h, double w) {
  if (h >= 0 && h < V.nl) {
    atomicAdd(&V.hF[h], w);
    atomicAdd(&V.hF2[h], w * w);
    atomicAdd(&V.hC[h], 1.0);
  }
  agg_add(V.F, V.F2, V.cnt, h >= V.nl ? h : -1, w);
}

/* Boost, light-travel time, bin decision (c2d_obsbin.h) and add of one event
 * in one histogram.  Wave-uniform control flow down to agg_add: no early
 * return for an event past the end (!valid) or outside the window, they
 * carry h = -1. */
__device__ __forceinline__ void obs_bin_event(const ObsView& V, const ObsEvent& ev, bool valid) {
  obs_decide(V, ev, valid, [&V](int h, double w) { obs_add(V, h, w); });
}

/* the workgroup's non-zero LDS bins to global memory (after a __syncthreads) */
__device__ __forceinline__ void obs_flush(const ObsView& V) {
  for (int i = threadIdx.x; i < V.nl; i += OBS_BLOCK) {
    if (V.hC[i] != 0.0) {
      atomicAdd(&V.F[i], V.hF[i]);
      atomicAdd(&V.F2[i], V.hF2[i]);
      atomicAdd(&V.cnt[i], V.hC[i]);
    }
  }
}

/* The single observer.  LDS: its edges, then as many leading time rows as
 * the host found room for, up to the device's limit (obs_api.cpp
 * obs_one_plan); beta is computed per thread. */
__global__ void __launch_bounds__(OBS_BLOCK) c2d_obs_kernel(const ObsDev O, const ObsSegs S) {
  __shared__ ObsSegsLds L;
  obs_stage_segs(L, S);
  const int64_t n = S.pre[S.nseg];
  extern __shared__ double sh[];
  double* p = sh;                          /* t0 t1 mu0 mu1 E0 E1, then the rows */
  p = obs_stage(p, O.t0, O.n_t); p = obs_stage(p, O.t1, O.n_t);
  p = obs_stage(p, O.mu0, O.n_mu); p = obs_stage(p, O.mu1, O.n_mu);
  p = obs_stage(p, O.E0, O.n_e); p = obs_stage(p, O.E1, O.n_e);
  const double G = O.gam_bulk;
  const ObsView V = obs_view(O, __builtin_sqrt(1. - 1. / (G * G)), sh, p);
  for (int i = threadIdx.x; i < 3 * V.nl; i += OBS_BLOCK) V.hF[i] = 0.0;
  __syncthreads();
  /* wave-uniform trip count so the aggregation's cross-lane ops see the whole wave */
  for (int64_t base = (int64_t)blockIdx.x * OBS_BLOCK; base < n; base += (int64_t)gridDim.x * OBS_BLOCK) {
    const int64_t e = base + threadIdx.x;
    const bool valid = e < n;
    obs_bin_event(V, obs_fetch(L, S.nseg, valid ? e : 0), valid);
  }
  if (V.nl) {
    __syncthreads();
    obs_flush(V);
  }
}

/* An observer set: up to OBS_SET_MAX binnings (SEDs and light curves, each
 * with its own Gamma, r_max, t_offset and edges) filled in one pass over the
 * events.  Per event, once: obs_fetch.  Per member, in a wave-uniform loop:
 * obs_bin_event, the single observer's own code, so a member's bin decisions
 * are those of c2d_obs_kernel.
 *
 * LDS (planned on the host, obs_api.cpp obs_set_plan; never more than
 * OBS_SET_LDS with the static tables): the edges of every member, then each
 * member's leading lds_rows time rows privatised (F, F2, count); later rows
 * go through agg_add to global memory.  beta per member comes from LDS. */
__global__ void __launch_bounds__(OBS_BLOCK) c2d_obs_set_kernel(const ObsSetDev Q, const ObsSegs S) {
  __shared__ ObsSegsLds L;
  __shared__ double betta_m[OBS_SET_MAX];
  obs_stage_segs(L, S);
  if (threadIdx.x < (unsigned)Q.n) {
    const double G = Q.m[threadIdx.x].gam_bulk;
    betta_m[threadIdx.x] = __builtin_sqrt(1. - 1. / (G * G));
  }
  const int64_t n = S.pre[S.nseg];
  extern __shared__ double sh[];
  obs_stage(sh, Q.edges, Q.n_edges);
  for (int i = threadIdx.x; i < Q.n_hist; i += OBS_BLOCK) sh[Q.n_edges + i] = 0.0;
  __syncthreads();
  /* wave-uniform trip counts (events, members, bands): every lane reaches agg_add */
  for (int64_t base = (int64_t)blockIdx.x * OBS_BLOCK; base < n; base += (int64_t)gridDim.x * OBS_BLOCK) {
    const int64_t e = base + threadIdx.x;
    const bool valid = e < n;
    const ObsEvent ev = obs_fetch(L, S.nseg, valid ? e : 0);
    for (int j = 0; j < Q.n; j++)
      obs_bin_event(obs_view(Q.m[j], betta_m[j], sh + Q.m[j].edge_off, sh + Q.m[j].hist_off), ev, valid);
  }
  if (Q.n_hist) {
    __syncthreads();
    for (int j = 0; j < Q.n; j++) obs_flush(obs_view(Q.m[j], 0.0, sh + Q.m[j].edge_off, sh + Q.m[j].hist_off));
  }
}

}  // namespace c2d

/* one launch of the set kernel over nseg event segments; its dynamic LDS is
 * the plan's (edges + privatised rows) */
extern "C" int c2d_launch_obs_set(const c2d::ObsSetDev* Q, const double* const* ev, const int64_t* n, int nseg,
                                  int grid, hipStream_t stream) {
  if (nseg < 1 || nseg > C2D_EV_SHARDS || Q->n < 1 || Q->n > c2d::OBS_SET_MAX) return (int)hipErrorInvalidValue;
  const size_t lds = sizeof(double) * ((size_t)Q->n_edges + (size_t)Q->n_hist);
  if (lds + c2d::OBS_SET_LDS_STATIC > (size_t)c2d::OBS_SET_LDS) return (int)hipErrorInvalidValue;
  for (int j = 0; j < Q->n; j++) {           /* every member's LDS ranges lie inside the allocation */
    const c2d::ObsSetMember& M = Q->m[j];
    if (M.n_t < 1 || M.n_mu < 1 || M.n_e < 1 || M.lds_rows < 0 || M.lds_rows > M.n_t) return (int)hipErrorInvalidValue;
    const int64_t ne = 2 * ((int64_t)M.n_t + M.n_mu + M.n_e), nl = (int64_t)M.lds_rows * M.n_mu * M.n_e;
    if (M.edge_off < 0 || M.edge_off + ne > Q->n_edges || M.hist_off < Q->n_edges ||
        M.hist_off + 3 * nl > (int64_t)Q->n_edges + Q->n_hist)
      return (int)hipErrorInvalidValue;
  }
  c2d::ObsSegs S;
  if (!obs_segs(S, ev, n, nseg)) return 0;
  hipLaunchKernelGGL(c2d::c2d_obs_set_kernel, dim3(grid), dim3(c2d::OBS_BLOCK), lds, stream, *Q, S);
  return (int)hipGetLastError();
}

extern "C" size_t c2d_obs_lds_bytes(int n_t, int n_mu, int n_e, int lds_rows) {
  return sizeof(double) * (2 * (size_t)(n_t + n_mu + n_e) + 3 * (size_t)lds_rows * n_mu * n_e);
}

extern "C" int c2d_obs_block(void) { return c2d::OBS_BLOCK; }

/* one launch of the single observer's kernel over nseg event segments (ev[s],
 * n[s] events each; at most C2D_EV_SHARDS): the transport's event shards
 * binned together */
extern "C" int c2d_launch_obs_segs(const c2d::ObsDev* O, const double* const* ev, const int64_t* n, int nseg,
                                   int grid, hipStream_t stream) {
  if (nseg < 1 || nseg > C2D_EV_SHARDS) return (int)hipErrorInvalidValue;
  c2d::ObsSegs S;
  if (!obs_segs(S, ev, n, nseg)) return 0;
  const size_t lds = c2d_obs_lds_bytes(O->n_t, O->n_mu, O->n_e, O->lds_rows);
  if (lds > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute((const void*)c2d::c2d_obs_kernel,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(c2d::c2d_obs_kernel, dim3(grid), dim3(c2d::OBS_BLOCK), lds, stream, *O, S);
  return (int)hipGetLastError();
}
