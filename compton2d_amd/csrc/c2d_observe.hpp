/*
 * c2d_observe.hpp — what the observer kernels share (observe.hip: the f64
 * kernels; obsacc.hip: the exact set kernel): the launch's event segments,
 * the event fetch, LDS staging and a histogram as a lane sees it.  Device
 * code; the bin decision itself is c2d_obsbin.h.
 */
#ifndef C2D_OBSERVE_HPP
#define C2D_OBSERVE_HPP

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/compton2d.h"
#include "c2d_device.hpp"
#include "c2d_math.h"
#include "c2d_obsbin.h"

namespace c2d {

constexpr int OBS_BLOCK = 512;

/* the event segments of one launch (the transport's event shards, back to
 * back): event e lies in segment s with pre[s] <= e < pre[s + 1] */
struct ObsSegs {
  const double* base[C2D_EV_SHARDS];
  int64_t pre[C2D_EV_SHARDS + 1];
  int32_t nseg;
};

/* ---- event fetch: the segment table in LDS, then one event's words ---- */
struct alignas(16) ObsSegsLds {            /* 528 B of the 1 KiB the host plans keep for static LDS */
  int64_t pre[C2D_EV_SHARDS + 1];
  const double* base[C2D_EV_SHARDS];
};

/* before the kernel's first __syncthreads */
__device__ __forceinline__ void obs_stage_segs(ObsSegsLds& L, const ObsSegs& S) {
  if (threadIdx.x <= (unsigned)S.nseg) L.pre[threadIdx.x] = S.pre[threadIdx.x];
  if (threadIdx.x < (unsigned)S.nseg) L.base[threadIdx.x] = S.base[threadIdx.x];
}

/* n doubles from global memory into LDS, by the whole workgroup; dst + n */
__device__ __forceinline__ double* obs_stage(double* dst, const double* src, int n) {
  for (int i = threadIdx.x; i < n; i += OBS_BLOCK) dst[i] = src[i];
  return dst + n;
}

__device__ __forceinline__ ObsEvent obs_fetch(const ObsSegsLds& L, int nseg, int64_t ee) {
  int sg = 0;                              /* last segment with pre[sg] <= ee */
  for (int hi = nseg - 1; sg < hi;) {
    const int m = (sg + hi + 1) >> 1;
    if (L.pre[m] <= ee) sg = m; else hi = m - 1;
  }
  return obs_event_of(L.base[sg] + (ee - L.pre[sg]) * C2D_EVENT_WORDS);
}

/* One histogram as a lane sees it: the single observer's (ObsDev) or a set
 * member's (ObsSetMember).  Edges and the privatised leading rows are in LDS;
 * bins h = row * n_mu * n_e + col with row = time bin, and h < nl lives in LDS. */
struct ObsView {
  double G, betta, rmax, t_offset;
  int32_t mode, n_t, n_mu, n_e;
  int32_t sorted_t, sorted_mu, sorted_e;
  const double *t0, *t1, *mu0, *mu1, *E0, *E1;   /* LDS */
  double *hF, *hF2, *hC;                         /* LDS: nl bins each */
  int nl;
  double *F, *F2, *cnt;                          /* global */
};

template <class D>
__device__ __forceinline__ ObsView obs_view(const D& d, double betta, double* edges, double* hist) {
  ObsView V;
  V.G = d.gam_bulk; V.betta = betta; V.rmax = d.rmax; V.t_offset = d.t_offset;
  V.mode = d.mode; V.n_t = d.n_t; V.n_mu = d.n_mu; V.n_e = d.n_e;
  V.sorted_t = d.sorted_t; V.sorted_mu = d.sorted_mu; V.sorted_e = d.sorted_e;
  V.t0 = edges; V.t1 = V.t0 + d.n_t;
  V.mu0 = V.t1 + d.n_t; V.mu1 = V.mu0 + d.n_mu;
  V.E0 = V.mu1 + d.n_mu; V.E1 = V.E0 + d.n_e;
  V.nl = d.lds_rows * d.n_mu * d.n_e;
  V.hF = hist; V.hF2 = V.hF + V.nl; V.hC = V.hF2 + V.nl;
  V.F = d.F; V.F2 = d.F2; V.cnt = d.cnt;
  return V;
}

}  // namespace c2d

/* the launch's non-empty segments, back to back; false when there is none */
static inline bool obs_segs(c2d::ObsSegs& S, const double* const* ev, const int64_t* n, int nseg) {
  int k = 0;
  S.pre[0] = 0;
  for (int s = 0; s < nseg; s++) {
    if (n[s] <= 0) continue;
    S.base[k] = ev[s];
    S.pre[k + 1] = S.pre[k] + n[s];
    k++;
  }
  S.nseg = k;
  return k > 0;
}

#endif /* C2D_OBSERVE_HPP */
