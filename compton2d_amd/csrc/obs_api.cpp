/*
 * obs_api.cpp — the observer entry points of the C ABI (include/compton2d.h):
 * c2d_obs_* (one histogram) and c2d_obs_set_* (several, filled in one pass),
 * over the kernels of observe.hip (postprocessing/pspt.c, plcm.c; DESIGN.md
 * §4c).  Both families describe a histogram with ObsHist (c2d_ctx.hpp) and
 * share every helper below; `set` tells them whose launch it is.  What
 * differs on purpose: the two LDS plans, one asynchronous launch per shard
 * against one over all shards, and what a failed call leaves behind.
 */
#include <algorithm>
#include <cstdlib>

#include "c2d_ctx.hpp"
#include "c2d_obsacc_host.h"

extern "C" int c2d_launch_obs_segs(const ObsDev* O, const double* const* ev, const int64_t* n, int nseg,
                                   int grid, hipStream_t stream);
extern "C" int c2d_launch_obs_set(const ObsSetDev* Q, const double* const* ev, const int64_t* n, int nseg,
                                  int grid, hipStream_t stream);
extern "C" int c2d_launch_obs_set_exact(const ObsSetDev* Q, const ObsExactDev* X, const double* const* ev,
                                        const int64_t* n, int nseg, int grid, hipStream_t stream);
extern "C" int c2d_launch_obs_merge(uint64_t* acc, const uint64_t* add, int64_t nbins, uint64_t rej, hipStream_t stream);
extern "C" size_t c2d_obs_lds_bytes(int n_t, int n_mu, int n_e, int lds_rows);
extern "C" int c2d_obs_block(void);

#define OBSCHK(x) do { const int rc_ = (x); if (rc_ != C2D_OK) return rc_; } while (0)

/* ------------------------------------------------------------------ */
/* the context's side: stream, fence, settle, release                  */
/* ------------------------------------------------------------------ */
int obs_init(c2d_ctx* c) {
  ObsState& o = c->obs;
  HIPCHK(c, hipStreamCreateWithFlags(&o.stream, hipStreamNonBlocking));
  HIPCHK(c, hipEventCreateWithFlags(&o.ev_src, hipEventDisableTiming));
  HIPCHK(c, hipEventCreate(&o.ev_a));
  HIPCHK(c, hipEventCreate(&o.ev_b));
  return C2D_OK;
}

int obs_fence(c2d_ctx* c, hipStream_t stream) {
  if (c->obs.inflight) HIPCHK(c, hipStreamWaitEvent(stream, c->obs.ev_b, 0));
  return C2D_OK;
}

/* Wait for an asynchronous binning of the context's own events and add its
 * kernel time. */
int obs_settle(c2d_ctx* c) {
  ObsState& o = c->obs;
  if (!o.inflight) return C2D_OK;
  o.inflight = false;
  HIPCHK(c, hipEventSynchronize(o.ev_b));
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, o.ev_a, o.ev_b);
  (o.inflight_set ? o.set_l : o.one_l).ms += ms;
  o.inflight_set = false;
  return C2D_OK;
}

static void obs_hist_free(ObsHist& h) {
  if (h.hist) (void)hipFree(h.hist);
  if (h.red) (void)hipFree(h.red);
  if (h.acc) (void)hipFree(h.acc);
  if (h.acc_red) (void)hipFree(h.acc_red);
  h = ObsHist{};
}

static void obs_set_free(ObsState& o) {
  for (ObsHist& m : o.set_h) obs_hist_free(m);
  o.set_h.clear();
  if (o.set_edges) (void)hipFree(o.set_edges);
  o.set_edges = nullptr;
  o.set = ObsSetDev{};
  o.set_started = false;
  o.set_l = ObsLaunches{};
  o.set_exact = false;
  o.set_wmax = 0.0;
  o.set_x = ObsExactDev{};
}

void obs_release(c2d_ctx* c) {
  ObsState& o = c->obs;
  if (o.stream) (void)hipStreamSynchronize(o.stream);   /* it reads the event buffer */
  obs_hist_free(o.one);
  obs_set_free(o);
  if (o.edges) (void)hipFree(o.edges);
  if (o.ev) (void)hipFree(o.ev);
  if (o.ev_src) (void)hipEventDestroy(o.ev_src);
  if (o.ev_a) (void)hipEventDestroy(o.ev_a);
  if (o.ev_b) (void)hipEventDestroy(o.ev_b);
  if (o.stream) (void)hipStreamDestroy(o.stream);
  o = ObsState{};
}

/* ------------------------------------------------------------------ */
/* a histogram from c2d_obs_bins or from a tool's deck                  */
/* ------------------------------------------------------------------ */
static int obs_bins_check(c2d_ctx* c, const c2d_obs_bins* b, const char* who) {
  if ((b->mode != C2D_OBS_SED && b->mode != C2D_OBS_LC) || b->n_t < 1 || b->n_t > C2D_OBS_MAX_T ||
      b->n_mu < 1 || b->n_mu > C2D_OBS_MAX_MU || b->n_e < 1 || b->n_e > C2D_OBS_MAX_E ||
      !b->t0 || !b->t1 || !b->mu0 || !b->mu1 || !b->E0 || !b->E1 || !(b->gam_bulk >= 1.0))
    return fail(c, C2D_E_ARG, "%s: bad binning", who);
  if (b->mode == C2D_OBS_SED && b->n_mu != 1)
    return fail(c, C2D_E_ARG, "%s: the SED mode has one angular window", who);
  return C2D_OK;
}

/* what ObsDev and ObsSetMember say alike about a binning */
template <class D>
static void obs_describe(D& d, const c2d_obs_bins* b) {
  d.gam_bulk = b->gam_bulk; d.rmax = b->rmax; d.t_offset = b->t_offset;
  d.mode = b->mode; d.n_t = b->n_t; d.n_mu = b->n_mu; d.n_e = b->n_e;
  d.sorted_t = obs_sorted(b->t0, b->t1, b->n_t);
  d.sorted_mu = obs_sorted(b->mu0, b->mu1, b->n_mu);
  d.sorted_e = obs_sorted(b->E0, b->E1, b->n_e);
}

template <class D>
static void obs_point(D& d, const ObsHist& h) {
  d.F = h.hist; d.F2 = d.F + h.nh(); d.cnt = d.F2 + h.nh();
}

/* h's sizes and packed edges from `b`, its zeroed device block (and the
 * world_sum buffer of a deck: it lives as long as the histogram, so a rank
 * cannot fail an allocation and skip the collective the others enter), and
 * `all` (h's edges last) on the device.  Nothing is kept on failure. */
static int obs_hist_make(c2d_ctx* c, const c2d_obs_bins* b, ObsHist& h, std::vector<double>& all, double** d_edges,
                         const char* who) {
  h.n_t = b->n_t; h.n_mu = b->n_mu; h.n_e = b->n_e;
  const std::pair<const double*, int> parts[] = {{b->t0, b->n_t}, {b->t1, b->n_t},   {b->mu0, b->n_mu},
                                                 {b->mu1, b->n_mu}, {b->E0, b->n_e}, {b->E1, b->n_e}};
  h.edges.clear();
  for (const auto& p : parts) h.edges.insert(h.edges.end(), p.first, p.first + p.second);
  all.insert(all.end(), h.edges.begin(), h.edges.end());
  const size_t bytes = 3 * h.nh() * sizeof(double);
  *d_edges = nullptr;
  hipError_t e = dalloc(d_edges, all.size());
  if (e == hipSuccess) e = dalloc(&h.hist, 3 * h.nh());
  if (e == hipSuccess && h.kind != OBS_RAW) e = dalloc(&h.red, 3 * h.nh());
  if (e == hipSuccess) e = hipMemcpy(*d_edges, all.data(), all.size() * sizeof(double), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(h.hist, 0, bytes);
  if (e == hipSuccess) return C2D_OK;
  if (*d_edges) (void)hipFree(*d_edges);
  *d_edges = nullptr;
  obs_hist_free(h);
  return fail(c, C2D_E_HIP, "%s: %s", who, hipGetErrorString(e));
}

/* the tool's dialogue -> its binning (postprocessing/pspt.c:105-205,
 * plcm.c:97-302); `b` points into the deck kept in `h` */
static int obs_deck_bins(c2d_ctx* c, int kind, const char* deck, ObsHist& h, c2d_obs_bins* b, const char* who) {
  h.kind = kind;
  b->t_offset = 0.0;
  if (kind == OBS_PSPT) {
    c2d_pspt_deck& d = h.pspt;
    if (c2d_pspt_parse(deck ? deck : "", &d))
      return fail(c, C2D_E_ARG, "%s: the deck's grid has no bins or more than %d energy channels", who,
                  C2D_PSPT_CHMAX);
    b->mode = C2D_OBS_SED; b->gam_bulk = d.gam_bulk; b->rmax = d.rmax;
    b->n_t = d.n_t; b->t0 = d.t0; b->t1 = d.t1;
    b->n_mu = 1; b->mu0 = &d.mu0; b->mu1 = &d.mu1;
    b->n_e = d.n_e; b->E0 = d.E0; b->E1 = d.E1;
  } else {
    h.plcm.resize(1);
    c2d_plcm_deck& d = h.plcm[0];
    if (c2d_plcm_parse(deck ? deck : "", &d))
      return fail(c, C2D_E_ARG, "%s: the deck has no angular bin, an empty region or more than %d energy channels",
                  who, C2D_PLCM_CHMAX);
    b->mode = C2D_OBS_LC; b->gam_bulk = d.gam_bulk; b->rmax = d.rmax; b->t_offset = d.t_offset;
    b->n_t = d.n_t; b->t0 = d.t0; b->t1 = d.t1;
    b->n_mu = d.n_mu; b->mu0 = d.mu0; b->mu1 = d.mu1;
    b->n_e = d.n_e; b->E0 = d.E0; b->E1 = d.E1;
  }
  return C2D_OK;
}

/* ------------------------------------------------------------------ */
/* launches                                                            */
/* ------------------------------------------------------------------ */
/* one launch over the segments (`tot` events in all) on `stream`: enough
 * blocks to fill the chip, each privatising its own histogram rows */
static int obs_launch(c2d_ctx* c, bool set, const double* const* ev, const int64_t* m, int nseg, int64_t tot,
                      hipStream_t stream) {
  ObsLaunches& l = set ? c->obs.set_l : c->obs.one_l;
  const int64_t bs = c2d_obs_block();
  const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((int64_t)c->n_cu * l.wg_per_cu, (tot + bs - 1) / bs));
  const int rc = !set                ? c2d_launch_obs_segs(&c->obs.dev, ev, m, nseg, grid, stream)
                 : c->obs.set_exact ? c2d_launch_obs_set_exact(&c->obs.set, &c->obs.set_x, ev, m, nseg, grid, stream)
                                    : c2d_launch_obs_set(&c->obs.set, ev, m, nseg, grid, stream);
  if (rc) return fail(c, C2D_E_HIP, "%s launch: %s", set ? "obs set" : "obs", hipGetErrorString((hipError_t)rc));
  l.launches++;
  return C2D_OK;
}

/* every segment in one launch on the context's stream, timed and waited for */
static int obs_launch_sync(c2d_ctx* c, bool set, const double* const* ev, const int64_t* m, int nseg) {
  int64_t tot = 0;
  for (int s = 0; s < nseg; s++) tot += m[s];
  if (tot == 0) return C2D_OK;
  HIPCHK(c, hipEventRecord(c->ev_g0a, c->stream));
  OBSCHK(obs_launch(c, set, ev, m, nseg, tot, c->stream));
  HIPCHK(c, hipEventRecord(c->ev_g0b, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, c->ev_g0a, c->ev_g0b);
  (set ? c->obs.set_l : c->obs.one_l).ms += ms;
  return C2D_OK;
}

/* the context's own escapes: its C2D_EV_SHARDS event shards */
static int obs_bin_own(c2d_ctx* c, bool set) {
  ObsState& o = c->obs;
  const double* seg[C2D_EV_SHARDS];
  int64_t cnt[C2D_EV_SHARDS];
  int64_t tot = 0;
  for (int sh = 0; sh < C2D_EV_SHARDS; sh++) {
    seg[sh] = c->ev + (size_t)sh * c->ev_cap_sh * C2D_EVENT_WORDS;
    cnt[sh] = c->ev_cnt[sh];
    tot += cnt[sh];
  }
  const char* e = getenv("C2D_OBS_ASYNC");
  if ((e && e[0] == '0') || tot == 0) return obs_launch_sync(c, set, seg, cnt, C2D_EV_SHARDS);
  /* on the observer's stream, after the step that wrote the events; the
   * next generation-0 launch waits for ev_b (obs_fence) */
  HIPCHK(c, hipEventRecord(o.ev_src, c->stream));
  HIPCHK(c, hipStreamWaitEvent(o.stream, o.ev_src, 0));
  HIPCHK(c, hipEventRecord(o.ev_a, o.stream));
  if (set) {
    /* one launch over all shards: a set workgroup stages up to 63 KiB of
     * edges and rows, which one launch per shard would repeat 32 times
     *  */
    OBSCHK(obs_launch(c, true, seg, cnt, C2D_EV_SHARDS, tot, o.stream));
  } else {
    /* one launch per shard: between the short launches the FP update's
     * workgroups (69 KB of LDS each) find room beside them (binning all
     * shards in one launch beside the FP slowed it 1.26 -> 2.3-2.8 ms,
     * at one or two workgroups per CU) */
    for (int s = 0; s < C2D_EV_SHARDS; s++)
      if (cnt[s]) OBSCHK(obs_launch(c, false, &seg[s], &cnt[s], 1, cnt[s], o.stream));
  }
  HIPCHK(c, hipEventRecord(o.ev_b, o.stream));
  o.inflight = true;
  o.inflight_set = set;
  return C2D_OK;
}

/* n events, on the host (staged) or on the device */
static int obs_bin(c2d_ctx* c, bool set, const double* ev, int64_t n, bool on_device) {
  ObsState& o = c->obs;
  if (!on_device) {
    if (n > o.ev_cap) {
      if (o.ev) (void)hipFree(o.ev);
      o.ev = nullptr;
      o.ev_cap = 0;
      HIPCHK(c, dalloc(&o.ev, (size_t)n * C2D_EVENT_WORDS));
      o.ev_cap = n;
    }
    if (n) HIPCHK(c, hipMemcpy(o.ev, ev, (size_t)n * C2D_EVENT_WORDS * sizeof(double), hipMemcpyHostToDevice));
    ev = o.ev;
  }
  return obs_launch_sync(c, set, &ev, &n, 1);
}

/* ------------------------------------------------------------------ */
/* what the entry points of both families do alike                     */
/* ------------------------------------------------------------------ */
/* a call that needs the binning (the single observer begun, the set not
 * empty) and then its arguments right; any binning in flight is settled */
static int obs_enter(c2d_ctx* c, bool set, const char* who, bool args_ok = true) {
  if (set ? c->obs.set.n < 1 : !c->obs.ready)
    return set ? fail(c, C2D_E_STATE, "%s: the set is empty", who)
               : fail(c, C2D_E_STATE, "c2d_obs_begin must precede %s", who);
  if (!args_ok) return C2D_E_ARG;
  HIPCHK(c, hipSetDevice(c->cfg.device));
  return obs_settle(c);
}

/* events == nullptr: the context's own */
static int obs_accumulate(c2d_ctx* c, bool set, const char* who, const double* events, int64_t n, bool on_device) {
  OBSCHK(obs_enter(c, set, who, !(events && n < 0)));
  if (set) c->obs.set_started = true;         /* from here on an add is C2D_E_STATE */
  return events ? obs_bin(c, set, events, n, on_device) : obs_bin_own(c, set);
}

namespace {
struct ObsSink {
  c2d_ctx* c;
  bool set;
};
}  // namespace

static int obs_file_sink(void* user, const double* ev, int64_t n, int on_device) {
  const ObsSink* s = static_cast<const ObsSink*>(user);
  return obs_bin(s->c, s->set, ev, n, on_device != 0);
}

/* the event file `path`, binned chunk by chunk as the device parses it */
static int obs_accumulate_file(c2d_ctx* c, bool set, const char* who, const char* path, int64_t* n) {
  if (!c || !path || !path[0]) return C2D_E_ARG;
  OBSCHK(obs_enter(c, set, who));
  if (set) c->obs.set_started = true;
  ObsSink s = {c, set};
  return events_parse(c, path, obs_file_sink, &s, n);
}

static int obs_download(c2d_ctx* c, const ObsHist& h, double* F, double* F2, double* count) {
  const size_t nh = h.nh(), bytes = nh * sizeof(double);
  if (F) HIPCHK(c, hipMemcpy(F, h.hist, bytes, hipMemcpyDeviceToHost));
  if (F2) HIPCHK(c, hipMemcpy(F2, h.hist + nh, bytes, hipMemcpyDeviceToHost));
  if (count) HIPCHK(c, hipMemcpy(count, h.hist + 2 * nh, bytes, hipMemcpyDeviceToHost));
  return C2D_OK;
}

/* ---- an exact member's integers on the host ---- */
static int obs_exact_download(c2d_ctx* c, const ObsHist& h, std::vector<uint64_t>& a) {
  a.resize(h.acc_words());
  HIPCHK(c, hipMemcpy(a.data(), h.acc, a.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
  return C2D_OK;
}

/* a (the accumulators of one member, n_rejected last) summed over the
 * context's communicator: every word travels as two 32-bit halves in u64
 * containers (ncclSum cannot carry between words; 2^32 ranks fit), then the
 * carries are normalised limb by limb on the host */
static int obs_exact_world_sum(c2d_ctx* c, const ObsHist& h, std::vector<uint64_t>& a, const char* who) {
  const size_t n = a.size(), nh = h.nh();
  std::vector<uint64_t> half(2 * n);
  for (size_t i = 0; i < n; i++) {
    half[2 * i] = a[i] & 0xffffffffull;
    half[2 * i + 1] = a[i] >> 32;
  }
  uint64_t* w = h.acc_red;
  HIPCHK(c, hipMemcpyAsync(w, half.data(), 2 * n * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
  const ncclResult_t r = ncclAllReduce(w, w, 2 * n, ncclUint64, ncclSum, c->comm, c->stream);
  if (r != ncclSuccess) return fail(c, C2D_E_RCCL, "ncclAllReduce: %s", ncclGetErrorString(r));
  HIPCHK(c, hipMemcpyAsync(half.data(), w, 2 * n * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  /* the integers: F and F2 are 4 halves each, count and n_rejected 2 */
  uint64_t over = 0;
  const auto norm = [&](size_t word, int words) {
    uint64_t carry = 0;
    for (int k = 0; k < 2 * words; k++) {
      const uint64_t t = half[2 * word + k] + carry;     /* below 2^64: a half-sum is below 2^64 - 2^32 */
      half[2 * word + k] = t & 0xffffffffull;
      carry = t >> 32;
    }
    over |= carry;
    for (int k = 0; k < words; k++) a[word + k] = half[2 * (word + k)] | (half[2 * (word + k) + 1] << 32);
  };
  for (size_t b = 0; b < nh; b++) {
    norm(C2D_OA_BIN_WORDS * b, 2);
    norm(C2D_OA_BIN_WORDS * b + 2, 2);
    norm(C2D_OA_BIN_WORDS * b + 4, 1);
  }
  norm(C2D_OA_BIN_WORDS * nh, 1);
  if (over) return fail(c, C2D_E_ARG, "%s: a sum over the communicator carries out of its top bit", who);
  return C2D_OK;
}

static int obs_exact_rejected(c2d_ctx* c, uint64_t n_rejected, const char* who) {
  if (!n_rejected) return C2D_OK;
  return fail(c, C2D_E_NONFINITE,
              "%s: %llu events were rejected (a boosted weight NaN, negative or not below the bound of w_max = %g); "
              "the sums lack them",
              who, (unsigned long long)n_rejected, c->obs.set_wmax);
}

/* F | F2 | count of an exact member as rounded doubles in v (3 nh) */
static int obs_exact_values(c2d_ctx* c, const ObsHist& h, const char* who, int32_t world_sum, double* F, double* F2,
                            double* count) {
  std::vector<uint64_t> a;
  OBSCHK(obs_exact_download(c, h, a));
  if (world_sum) OBSCHK(obs_exact_world_sum(c, h, a, who));
  OBSCHK(obs_exact_rejected(c, a[a.size() - 1], who));
  c2d_oa_bins_doubles(a.data(), h.e, (int64_t)h.nh(), F, F2, count);
  return C2D_OK;
}

/* The tool's files of a deck's histogram so far (postprocessing/pspt.c:323-353,
 * plcm.c:466-552).  world_sum: summed over the context's communicator first
 * (every rank calls, rank 0 writes). */
static int obs_write(c2d_ctx* c, const ObsHist& h, const char* who, const char* path, int32_t factor,
                     int32_t world_sum) {
  HIPCHK(c, hipSetDevice(c->cfg.device));
  OBSCHK(obs_settle(c));
  const size_t nh = h.nh();
  std::vector<double> v(3 * nh);
  if (world_sum && !c->comm) return fail(c, C2D_E_STATE, "%s: world_sum needs c2d_comm_init", who);
  if (h.acc) {                                  /* a member of an exact set: its integers, rounded once */
    OBSCHK(obs_exact_values(c, h, who, world_sum, v.data(), v.data() + nh, v.data() + 2 * nh));
    if (world_sum && c->comm_rank != 0) return C2D_OK;
  } else if (world_sum) {
    double* w = h.red;
    HIPCHK(c, hipMemcpyAsync(w, h.hist, 3 * nh * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    const ncclResult_t r = ncclAllReduce(w, w, 3 * nh, ncclDouble, ncclSum, c->comm, c->stream);
    if (r != ncclSuccess) return fail(c, C2D_E_RCCL, "ncclAllReduce: %s", ncclGetErrorString(r));
    HIPCHK(c, hipMemcpyAsync(v.data(), w, 3 * nh * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->comm_rank != 0) return C2D_OK;
  } else {
    OBSCHK(obs_download(c, h, v.data(), v.data() + nh, v.data() + 2 * nh));
  }
  const double *F = v.data(), *F2 = F + nh, *cnt = F2 + nh;
  if (h.kind == OBS_PSPT) {
    const char* out = (path && path[0]) ? path : h.pspt.outfile;
    if (c2d_pspt_write(out, &h.pspt, F, cnt, factor)) return fail(c, C2D_E_IO, "%s: cannot write '%s'", who, out);
  } else {
    const char* dir = (path && path[0]) ? path : ".";
    if (c2d_plcm_write(dir, &h.plcm[0], F, F2, cnt, factor))
      return fail(c, C2D_E_IO, "%s: cannot write the light-curve files under '%s'", who, dir);
  }
  return C2D_OK;
}

/* ------------------------------------------------------------------ */
/* the single observer                                                 */
/* ------------------------------------------------------------------ */
/* Its LDS plan: as many leading time rows as fit next to the edges in what a
 * workgroup may allocate (all of them for the usual SED); later rows go to
 * wave-aggregated global atomics. */
static void obs_one_plan(const c2d_ctx* c, ObsDev& O, int* wg_per_cu) {
  const size_t edges = c2d_obs_lds_bytes(O.n_t, O.n_mu, O.n_e, 0);
  const size_t row = c2d_obs_lds_bytes(0, O.n_mu, O.n_e, 1) - c2d_obs_lds_bytes(0, O.n_mu, O.n_e, 0);
  /* 1 KiB for the kernel's static segment table (observe.hip ObsSegsLds) */
  const size_t avail = c->lds_max > edges + 1024 ? c->lds_max - edges - 1024 : 0;
  O.lds_rows = (int)std::min<size_t>((size_t)O.n_t, avail / row);
  const size_t bytes = c2d_obs_lds_bytes(O.n_t, O.n_mu, O.n_e, O.lds_rows);
  /* workgroups per CU that fit the CU's 160 KiB of LDS, at most 4 */
  *wg_per_cu = (int)std::max<size_t>(1, std::min<size_t>(4, (160 * 1024) / (bytes + 1024)));
}

/* `h` carries the kind and deck; the edges come from `b`.  A new binning
 * replaces the old one, pspt deck included, once `b` has passed the checks;
 * a failure after that leaves no binning. */
static int obs_begin(c2d_ctx* c, const c2d_obs_bins* b, ObsHist&& h) {
  ObsState& o = c->obs;
  OBSCHK(obs_bins_check(c, b, "c2d_obs_begin"));
  o.ready = false;
  HIPCHK(c, hipSetDevice(c->cfg.device));
  OBSCHK(obs_settle(c));                      /* the histogram is about to go */
  obs_hist_free(o.one);
  if (o.edges) (void)hipFree(o.edges);
  o.edges = nullptr;
  std::vector<double> all;
  OBSCHK(obs_hist_make(c, b, h, all, &o.edges, "c2d_obs_begin"));
  ObsDev& O = o.dev;
  obs_describe(O, b);
  obs_point(O, h);
  o.one = std::move(h);
  O.t0 = o.edges; O.t1 = O.t0 + b->n_t; O.mu0 = O.t1 + b->n_t; O.mu1 = O.mu0 + b->n_mu;
  O.E0 = O.mu1 + b->n_mu; O.E1 = O.E0 + b->n_e;
  o.one_l = ObsLaunches{};
  obs_one_plan(c, O, &o.one_l.wg_per_cu);
  o.ready = true;
  return C2D_OK;
}

extern "C" int c2d_obs_begin(c2d_ctx* c, const c2d_obs_bins* b) {
  if (!c || !b) return C2D_E_ARG;
  return obs_begin(c, b, ObsHist{});
}

extern "C" int c2d_obs_begin_pspt(c2d_ctx* c, const char* deck) {
  if (!c) return C2D_E_ARG;
  ObsHist h;
  c2d_obs_bins b;
  OBSCHK(obs_deck_bins(c, OBS_PSPT, deck, h, &b, "c2d_obs_begin_pspt"));
  return obs_begin(c, &b, std::move(h));
}

extern "C" int c2d_obs_accumulate(c2d_ctx* c, const double* events, int64_t n) {
  if (!c) return C2D_E_ARG;
  return obs_accumulate(c, false, "c2d_obs_accumulate", events, n, false);
}

extern "C" int c2d_obs_accumulate_device(c2d_ctx* c, const double* d_events, int64_t n) {
  if (!c || !d_events || n < 0) return C2D_E_ARG;
  return obs_accumulate(c, false, "c2d_obs_accumulate_device", d_events, n, true);
}

extern "C" int c2d_obs_accumulate_file(c2d_ctx* c, const char* path, int64_t* n) {
  return obs_accumulate_file(c, false, "c2d_obs_accumulate_file", path, n);
}

extern "C" int c2d_obs_result(c2d_ctx* c, double* F, double* F2, double* count, double* kernel_ms) {
  if (!c) return C2D_E_ARG;
  OBSCHK(obs_enter(c, false, "c2d_obs_result"));
  OBSCHK(obs_download(c, c->obs.one, F, F2, count));
  if (kernel_ms) *kernel_ms = c->obs.one_l.ms;
  return C2D_OK;
}

extern "C" int c2d_obs_write_pspt(c2d_ctx* c, const char* path, int32_t factor, int32_t world_sum) {
  if (!c) return C2D_E_ARG;
  if (!c->obs.ready || c->obs.one.kind != OBS_PSPT)
    return fail(c, C2D_E_STATE, "c2d_obs_write_pspt: c2d_obs_begin_pspt first");
  return obs_write(c, c->obs.one, "c2d_obs_write_pspt", path, factor, world_sum);
}

/* ------------------------------------------------------------------ */
/* observer sets: several SEDs and light curves in one pass            */
/* ------------------------------------------------------------------ */
/* The LDS plan of a set: the edges of every member, then
 * privatised leading time rows.  What the edges leave of the workgroup's
 * OBS_SET_LDS is shared out equally among the members, each taking whole
 * rows of its share (at most its n_t); what that leaves over is handed out
 * in registration order.  -1 when the edges alone do not fit.  bin_words: the
 * LDS words of a privatised bin, 3 doubles (F, F2, count) or the exact set's
 * 5 u64 (c2d_obsacc.h). */
static int obs_set_plan(ObsSetDev& Q, int* wg_per_cu, int bin_words = 3) {
  const int64_t budget = (OBS_SET_LDS - OBS_SET_LDS_STATIC) / (int64_t)sizeof(double);
  int64_t ne = 0;
  for (int j = 0; j < Q.n; j++) {
    Q.m[j].edge_off = (int32_t)ne;
    ne += 2 * ((int64_t)Q.m[j].n_t + Q.m[j].n_mu + Q.m[j].n_e);
    if (ne > budget) return -1;
  }
  int64_t left = budget - ne;
  const int64_t share = Q.n ? left / Q.n : 0;
  for (int j = 0; j < Q.n; j++) {
    const int64_t row = bin_words * (int64_t)Q.m[j].n_mu * Q.m[j].n_e;
    Q.m[j].lds_rows = (int32_t)std::min<int64_t>(Q.m[j].n_t, share / row);
    left -= Q.m[j].lds_rows * row;
  }
  int64_t nh = 0;
  for (int j = 0; j < Q.n; j++) {
    const int64_t row = bin_words * (int64_t)Q.m[j].n_mu * Q.m[j].n_e;
    const int64_t more = std::min<int64_t>(Q.m[j].n_t - Q.m[j].lds_rows, left / row);
    Q.m[j].lds_rows += (int32_t)more;
    left -= more * row;
    Q.m[j].hist_off = (int32_t)(ne + nh);
    nh += Q.m[j].lds_rows * row;
  }
  Q.n_edges = (int32_t)ne;
  Q.n_hist = (int32_t)nh;
  /* workgroups per CU that fit the CU's 160 KiB of LDS, at most 4 */
  const size_t bytes = (size_t)(ne + nh) * sizeof(double) + OBS_SET_LDS_STATIC;
  *wg_per_cu = (int)std::max<size_t>(1, std::min<size_t>(4, (160 * 1024) / bytes));
  return 0;
}

/* ---- the exact set (c2d_obs_set_exact; c2d_obsacc.h, obsacc.hip) ---- */
static int obs_exact_bound(c2d_ctx* c, double w_max, double G, int32_t* e, const char* who) {
  if (c2d_oa_bound(w_max, G, e)) return C2D_OK;
  return fail(c, C2D_E_ARG, "%s: w_max %g and Gamma %g give no exponent bound within [%d, %d]", who, w_max, G,
              C2D_OA_E_MIN, C2D_OA_E_MAX);
}

/* h's zeroed integer accumulators (and a deck's world_sum buffer: twice the
 * words, 32-bit halves in u64 containers); on failure h keeps neither */
static int obs_exact_alloc(c2d_ctx* c, ObsHist& h, int32_t e, const char* who) {
  hipError_t r = dalloc(&h.acc, h.acc_words());
  if (r == hipSuccess && h.kind != OBS_RAW) r = dalloc(&h.acc_red, 2 * h.acc_words());
  if (r == hipSuccess) r = hipMemset(h.acc, 0, h.acc_words() * sizeof(uint64_t));
  if (r == hipSuccess) {
    h.e = e;
    return C2D_OK;
  }
  if (h.acc) (void)hipFree(h.acc);
  if (h.acc_red) (void)hipFree(h.acc_red);
  h.acc = h.acc_red = nullptr;
  return fail(c, C2D_E_HIP, "%s: %s", who, hipGetErrorString(r));
}

extern "C" int c2d_obs_set_clear(c2d_ctx* c) {
  if (!c) return C2D_E_ARG;
  HIPCHK(c, hipSetDevice(c->cfg.device));
  OBSCHK(obs_settle(c));                      /* the histograms are about to go */
  obs_set_free(c->obs);
  return C2D_OK;
}

/* Add a member: `h` carries its kind and deck; the edges come from `b`.
 * Unlike obs_begin, a failure at any point leaves the set as it was. */
static int obs_set_add_member(c2d_ctx* c, const c2d_obs_bins* b, ObsHist&& h, int32_t* id, const char* who) {
  ObsState& o = c->obs;
  OBSCHK(obs_bins_check(c, b, who));
  if (o.set_started)
    return fail(c, C2D_E_STATE, "%s: the set has accumulated events; c2d_obs_set_clear first", who);
  if (o.set.n >= C2D_OBS_SET_MAX)
    return fail(c, C2D_E_ARG, "%s: a set holds at most %d members", who, C2D_OBS_SET_MAX);
  ObsSetDev Q = o.set;
  ObsSetMember& M = Q.m[Q.n++];
  M = ObsSetMember{};
  obs_describe(M, b);
  int32_t e = 0;
  if (o.set_exact) OBSCHK(obs_exact_bound(c, o.set_wmax, b->gam_bulk, &e, who));
  int wg = 1;
  if (obs_set_plan(Q, &wg, o.set_exact ? C2D_OA_BIN_WORDS : 3))
    return fail(c, C2D_E_ARG, "%s: the set's bin edges (%lld B with this member) exceed the workgroup's %d B of LDS",
                who, (long long)(sizeof(double) * (2 * ((int64_t)b->n_t + b->n_mu + b->n_e) + o.set.n_edges)),
                OBS_SET_LDS - OBS_SET_LDS_STATIC);
  HIPCHK(c, hipSetDevice(c->cfg.device));
  OBSCHK(obs_settle(c));
  /* every member's edges in one device array, in the LDS order of the plan */
  std::vector<double> all;
  all.reserve((size_t)Q.n_edges);
  for (const ObsHist& m : o.set_h) all.insert(all.end(), m.edges.begin(), m.edges.end());
  double* d_edges = nullptr;
  OBSCHK(obs_hist_make(c, b, h, all, &d_edges, who));
  if (o.set_exact) {
    const int rc = obs_exact_alloc(c, h, e, who);
    if (rc != C2D_OK) {
      (void)hipFree(d_edges);
      obs_hist_free(h);
      return rc;
    }
  }
  if (o.set_edges) (void)hipFree(o.set_edges);
  Q.edges = o.set_edges = d_edges;
  obs_point(M, h);
  if (o.set_exact) {
    M.F = reinterpret_cast<double*>(h.acc);   /* what the exact kernel accumulates into */
    o.set_x.e[Q.n - 1] = e;
  }
  if (id) *id = Q.n - 1;
  o.set = Q;
  o.set_l.wg_per_cu = wg;
  o.set_h.push_back(std::move(h));
  return C2D_OK;
}

extern "C" int c2d_obs_set_add(c2d_ctx* c, const c2d_obs_bins* b, int32_t* id) {
  if (!c || !b) return C2D_E_ARG;
  return obs_set_add_member(c, b, ObsHist{}, id, "c2d_obs_set_add");
}

static int obs_set_add_deck(c2d_ctx* c, int kind, const char* deck, int32_t* id, const char* who) {
  if (!c) return C2D_E_ARG;
  ObsHist h;
  c2d_obs_bins b;
  OBSCHK(obs_deck_bins(c, kind, deck, h, &b, who));
  return obs_set_add_member(c, &b, std::move(h), id, who);
}

extern "C" int c2d_obs_set_add_pspt(c2d_ctx* c, const char* deck, int32_t* id) {
  return obs_set_add_deck(c, OBS_PSPT, deck, id, "c2d_obs_set_add_pspt");
}

extern "C" int c2d_obs_set_add_plcm(c2d_ctx* c, const char* deck, int32_t* id) {
  return obs_set_add_deck(c, OBS_PLCM, deck, id, "c2d_obs_set_add_plcm");
}

extern "C" int c2d_obs_set_accumulate(c2d_ctx* c, const double* events, int64_t n) {
  if (!c) return C2D_E_ARG;
  return obs_accumulate(c, true, "c2d_obs_set_accumulate", events, n, false);
}

extern "C" int c2d_obs_set_accumulate_device(c2d_ctx* c, const double* d_events, int64_t n) {
  if (!c || !d_events || n < 0) return C2D_E_ARG;
  return obs_accumulate(c, true, "c2d_obs_set_accumulate_device", d_events, n, true);
}

extern "C" int c2d_obs_set_accumulate_file(c2d_ctx* c, const char* path, int64_t* n) {
  return obs_accumulate_file(c, true, "c2d_obs_set_accumulate_file", path, n);
}

/* member `id`, or C2D_E_ARG */
static int obs_set_member(c2d_ctx* c, int32_t id, const char* who, const ObsHist** h) {
  if (!c) return C2D_E_ARG;
  if (id < 0 || id >= c->obs.set.n) return fail(c, C2D_E_ARG, "%s: no member %d", who, (int)id);
  *h = &c->obs.set_h[(size_t)id];
  return C2D_OK;
}

extern "C" int c2d_obs_set_shape(c2d_ctx* c, int32_t id, int32_t* n_t, int32_t* n_mu, int32_t* n_e,
                                 int32_t* lds_rows) {
  const ObsHist* h = nullptr;
  OBSCHK(obs_set_member(c, id, "c2d_obs_set_shape", &h));
  if (n_t) *n_t = h->n_t;
  if (n_mu) *n_mu = h->n_mu;
  if (n_e) *n_e = h->n_e;
  if (lds_rows) *lds_rows = c->obs.set.m[id].lds_rows;
  return C2D_OK;
}

extern "C" int c2d_obs_set_result(c2d_ctx* c, int32_t id, double* F, double* F2, double* count) {
  const ObsHist* h = nullptr;
  OBSCHK(obs_set_member(c, id, "c2d_obs_set_result", &h));
  HIPCHK(c, hipSetDevice(c->cfg.device));
  OBSCHK(obs_settle(c));
  if (h->acc) return obs_exact_values(c, *h, "c2d_obs_set_result", 0, F, F2, count);
  return obs_download(c, *h, F, F2, count);
}

extern "C" int c2d_obs_set_kernel_ms(c2d_ctx* c, double* ms, int32_t* launches) {
  if (!c) return C2D_E_ARG;
  HIPCHK(c, hipSetDevice(c->cfg.device));
  OBSCHK(obs_settle(c));
  if (ms) *ms = c->obs.set_l.ms;
  if (launches) *launches = c->obs.set_l.launches;
  return C2D_OK;
}

extern "C" int c2d_obs_set_write(c2d_ctx* c, int32_t id, const char* path, int32_t factor, int32_t world_sum) {
  const ObsHist* h = nullptr;
  OBSCHK(obs_set_member(c, id, "c2d_obs_set_write", &h));
  if (h->kind == OBS_RAW)
    return fail(c, C2D_E_STATE, "c2d_obs_set_write: member %d was added without a deck", (int)id);
  return obs_write(c, *h, "c2d_obs_set_write", path, factor, world_sum);
}

/* ------------------------------------------------------------------ */
/* exact sets: integer sums, their state, merge and the host twin      */
/* ------------------------------------------------------------------ */
extern "C" int c2d_obs_set_exact(c2d_ctx* c, double w_max) {
  const char* who = "c2d_obs_set_exact";
  if (!c) return C2D_E_ARG;
  ObsState& o = c->obs;
  if (!(w_max > 0.0) || !c2d_oa_finite(w_max)) return fail(c, C2D_E_ARG, "%s: w_max must be finite and positive", who);
  if (o.set_started) return fail(c, C2D_E_STATE, "%s: the set has accumulated events; c2d_obs_set_clear first", who);
  if (o.set_exact) return fail(c, C2D_E_STATE, "%s: the set is exact already; c2d_obs_set_clear first", who);
  int32_t e[OBS_SET_MAX] = {0};
  for (int j = 0; j < o.set.n; j++) OBSCHK(obs_exact_bound(c, w_max, o.set.m[j].gam_bulk, &e[j], who));
  HIPCHK(c, hipSetDevice(c->cfg.device));
  OBSCHK(obs_settle(c));
  for (int j = 0; j < o.set.n; j++) {
    const int rc = obs_exact_alloc(c, o.set_h[(size_t)j], e[j], who);
    if (rc != C2D_OK) {                       /* the set stays as it was */
      for (int k = 0; k < j; k++) {
        ObsHist& h = o.set_h[(size_t)k];
        (void)hipFree(h.acc);
        if (h.acc_red) (void)hipFree(h.acc_red);
        h.acc = h.acc_red = nullptr;
      }
      return rc;
    }
  }
  ObsSetDev Q = o.set;
  int wg = o.set_l.wg_per_cu;
  (void)obs_set_plan(Q, &wg, C2D_OA_BIN_WORDS);   /* the edges fitted before: only the rows change */
  for (int j = 0; j < Q.n; j++) {
    Q.m[j].F = reinterpret_cast<double*>(o.set_h[(size_t)j].acc);
    o.set_x.e[j] = e[j];
  }
  o.set = Q;
  o.set_l.wg_per_cu = wg;
  o.set_exact = true;
  o.set_wmax = w_max;
  return C2D_OK;
}

/* member `id` of an exact set, any binning in flight settled */
static int obs_exact_member(c2d_ctx* c, int32_t id, const char* who, const ObsHist** h) {
  OBSCHK(obs_set_member(c, id, who, h));
  if (!c->obs.set_exact || !(*h)->acc) return fail(c, C2D_E_STATE, "%s: c2d_obs_set_exact first", who);
  HIPCHK(c, hipSetDevice(c->cfg.device));
  return obs_settle(c);
}

/* the member's state (include/compton2d.h) on the host */
static int obs_exact_state(c2d_ctx* c, int32_t id, const ObsHist& h, std::vector<uint64_t>& s) {
  std::vector<uint64_t> a;
  OBSCHK(obs_exact_download(c, h, a));
  const ObsSetMember& M = c->obs.set.m[id];
  c2d_oa_head H;
  H.mode = M.mode; H.n_t = h.n_t; H.n_mu = h.n_mu; H.n_e = h.n_e; H.e = h.e;
  H.bins_digest = c2d_oa_bins_digest(M.gam_bulk, M.rmax, M.t_offset, h.edges.data(), h.edges.size());
  H.n_rejected = a[a.size() - 1];
  s.assign((size_t)H.words(), 0ull);
  std::copy(a.begin(), a.end() - 1, s.begin() + C2D_OA_HEAD_WORDS);
  H.payload_digest = c2d_oa_payload_digest(s.data(), H.nh());
  c2d_oa_head_write(s.data(), H);
  return C2D_OK;
}

extern "C" int c2d_obs_set_exact_info(c2d_ctx* c, int32_t id, int32_t* e, int64_t* n_rejected) {
  const ObsHist* h = nullptr;
  OBSCHK(obs_exact_member(c, id, "c2d_obs_set_exact_info", &h));
  if (e) *e = h->e;
  if (n_rejected) {
    uint64_t r = 0;
    HIPCHK(c, hipMemcpy(&r, h->acc + h->acc_words() - 1, sizeof r, hipMemcpyDeviceToHost));
    *n_rejected = (int64_t)r;
  }
  return C2D_OK;
}

extern "C" int c2d_obs_set_state_words(c2d_ctx* c, int32_t id, int64_t* words) {
  const ObsHist* h = nullptr;
  OBSCHK(obs_exact_member(c, id, "c2d_obs_set_state_words", &h));
  if (words) *words = C2D_OA_HEAD_WORDS + C2D_OA_BIN_WORDS * (int64_t)h->nh();
  return C2D_OK;
}

extern "C" int c2d_obs_set_state(c2d_ctx* c, int32_t id, uint64_t* out, int64_t cap) {
  const ObsHist* h = nullptr;
  OBSCHK(obs_exact_member(c, id, "c2d_obs_set_state", &h));
  std::vector<uint64_t> s;
  OBSCHK(obs_exact_state(c, id, *h, s));
  if (!out || cap < (int64_t)s.size())
    return fail(c, C2D_E_ARG, "c2d_obs_set_state: the state has %lld words, the buffer %lld", (long long)s.size(),
                (long long)cap);
  std::copy(s.begin(), s.end(), out);
  return C2D_OK;
}

extern "C" int c2d_obs_set_merge(c2d_ctx* c, int32_t id, const uint64_t* in, int64_t words) {
  const char* who = "c2d_obs_set_merge";
  const ObsHist* h = nullptr;
  OBSCHK(obs_exact_member(c, id, who, &h));
  if (!in) return fail(c, C2D_E_ARG, "%s: no state", who);
  /* every check on the host, on a copy of the member's own state */
  std::vector<uint64_t> cur;
  OBSCHK(obs_exact_state(c, id, *h, cur));
  const char* why = c2d_oa_state_add(cur.data(), (int64_t)cur.size(), in, words);
  if (why) return fail(c, C2D_E_ARG, "%s: %s", who, why);
  const int64_t nh = (int64_t)h->nh();
  uint64_t* d = nullptr;
  HIPCHK(c, dalloc(&d, (size_t)(C2D_OA_BIN_WORDS * nh)));
  hipError_t r = hipMemcpyAsync(d, in + C2D_OA_HEAD_WORDS, (size_t)(C2D_OA_BIN_WORDS * nh) * sizeof(uint64_t),
                                hipMemcpyHostToDevice, c->stream);
  if (r == hipSuccess) r = (hipError_t)c2d_launch_obs_merge(h->acc, d, nh, in[6], c->stream);
  const hipError_t rs = hipStreamSynchronize(c->stream);
  (void)hipFree(d);
  if (r == hipSuccess) r = rs;
  if (r != hipSuccess) return fail(c, C2D_E_HIP, "%s: %s", who, hipGetErrorString(r));
  c->obs.set_started = true;                  /* the set holds sums now: no further member */
  return C2D_OK;
}

extern "C" int c2d_obs_exact_host(const c2d_obs_bins* bins, double w_max, const double* events, int64_t n,
                                  uint64_t* state, int64_t cap) {
  return c2d_oa_exact_host(bins, w_max, events, n, state, cap);
}

extern "C" int c2d_obs_state_merge(uint64_t* into, int64_t into_words, const uint64_t* from, int64_t from_words) {
  return c2d_oa_state_add(into, into_words, from, from_words) ? C2D_E_ARG : C2D_OK;
}

extern "C" int c2d_obs_state_result(const uint64_t* state, int64_t words, double* F, double* F2, double* count) {
  c2d_oa_head H;
  if (c2d_oa_head_read(state, words, &H)) return C2D_E_ARG;
  c2d_oa_bins_doubles(state + C2D_OA_HEAD_WORDS, H.e, H.nh(), F, F2, count);
  return C2D_OK;
}
