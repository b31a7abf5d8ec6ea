/*
 * c2d_ctx.hpp — the context behind the C ABI (include/compton2d.h) and the
 * helpers every host translation unit of the library shares: fail, HIPCHK,
 * dalloc.  Private to csrc/: capi.cpp, obs_api.cpp and popctl_api.cpp include
 * it; what the latter two call of capi.cpp is declared at the end.
 */
#ifndef C2D_CTX_HPP
#define C2D_CTX_HPP

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <cstdarg>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/compton2d.h"
#include "c2d_device.hpp"
#include "pspt_host.h"
#include "plcm_host.h"
#include "c2d_censtext.hpp"
#include "c2d_ckpt.hpp"
#include "c2d_evparse.hpp"
#include "c2d_evtext.hpp"

using namespace c2d;

/* the packet store (c2d_device.hpp PktSoA) */
struct DevPk {
  double* d[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  uint32_t* jk = nullptr;
  uint32_t* bins = nullptr;
  uint32_t* ctr = nullptr;
  uint32_t* sub = nullptr;
  uint64_t* key = nullptr;
  int64_t* hard = nullptr;    /* the scatter kernel's hard list (GenArgs.hard) */
  int64_t cap = 0;
  PktSoA soa() const {
    PktSoA s;
    s.rpre = d[0]; s.zpre = d[1]; s.wmu = d[2]; s.phi = d[3]; s.ew = d[4]; s.xnu = d[5];
    s.dcen = d[6]; s.jk = jk; s.bins = bins; s.ctr = ctr; s.sub = sub; s.key = key;
    return s;
  }
  void release() {
    for (double*& p : d) { if (p) (void)hipFree(p); p = nullptr; }
    if (jk) (void)hipFree(jk);
    if (bins) (void)hipFree(bins);
    if (ctr) (void)hipFree(ctr);
    if (sub) (void)hipFree(sub);
    if (key) (void)hipFree(key);
    if (hard) (void)hipFree(hard);
    jk = bins = ctr = sub = nullptr;
    key = nullptr;
    hard = nullptr;
    cap = 0;
  }
};

struct DevCensus {
  c2d_d2* d[3] = {nullptr, nullptr, nullptr};   /* rz, wp, ex (CensusSoA) */
  c2d_u4* tg = nullptr;
  CensusSoA soa() const {
    CensusSoA s;
    s.rz = d[0]; s.wp = d[1]; s.ex = d[2]; s.tg = tg;
    return s;
  }
};

/* ---- observer-frame binning (obs_api.cpp) ---- */
enum { OBS_RAW = 0, OBS_PSPT = 1, OBS_PLCM = 2 };

/* host side of one histogram: the single observer's, or one member's of the set */
struct ObsHist {
  int kind = OBS_RAW;                         /* bins given as such, or from a pspt / plcm deck */
  c2d_pspt_deck pspt;                         /* kind == OBS_PSPT */
  std::vector<c2d_plcm_deck> plcm;            /* one element when kind == OBS_PLCM */
  int32_t n_t = 0, n_mu = 0, n_e = 0;
  std::vector<double> edges;                  /* t0 t1 mu0 mu1 E0 E1 */
  double* hist = nullptr;                     /* device F | F2 | count: 3 x n_t x n_mu x n_e */
  double* red = nullptr;                      /* world_sum reduction buffer, same size (decks only) */
  /* an exact set's member (c2d_obs_set_exact): its integer accumulators on
   * the device, 5 u64 a bin in the state's order and then n_rejected, and
   * (decks only) the world_sum buffer of their 32-bit halves */
  uint64_t* acc = nullptr;
  uint64_t* acc_red = nullptr;
  int32_t e = 0;                              /* the exponent bound */
  size_t nh() const { return (size_t)n_t * n_mu * n_e; }
  size_t acc_words() const { return 5 * nh() + 1; }
};

/* what the single observer and the set each keep about their launches */
struct ObsLaunches {
  int wg_per_cu = 1;                          /* of the LDS plan */
  int32_t launches = 0;
  double ms = 0.0;                            /* device time of the launches so far */
};

struct ObsState {
  /* the context's own escapes binned on a second stream (c2d_obs_accumulate /
   * c2d_obs_set_accumulate with no events): it overlaps the next step's FP /
   * tables / sources, and the next generation-0 launch, which rewrites the
   * event buffer, waits for it (obs_fence; obs_settle reads its time when
   * the host needs the result).  One launch sequence in flight at a time,
   * the single observer's or the set's. */
  hipStream_t stream = nullptr;
  hipEvent_t ev_src = nullptr, ev_a = nullptr, ev_b = nullptr;
  bool inflight = false, inflight_set = false;
  double* ev = nullptr;                       /* staging of host events */
  int64_t ev_cap = 0;
  /* the single observer (c2d_obs_*) */
  bool ready = false;
  ObsDev dev;
  ObsHist one;
  double* edges = nullptr;
  ObsLaunches one_l;
  /* the set: several binnings filled in one pass (c2d_obs_set_*) */
  ObsSetDev set = {};
  std::vector<ObsHist> set_h;
  double* set_edges = nullptr;                /* every member's edges, in the plan's LDS order */
  bool set_started = false;                   /* accumulated since the last clear */
  ObsLaunches set_l;
  bool set_exact = false;                     /* c2d_obs_set_exact since the last clear */
  double set_wmax = 0.0;
  ObsExactDev set_x = {};
};

struct c2d_ctx;
int obs_init(c2d_ctx* c);                          /* c2d_init: the stream and its events */
void obs_release(c2d_ctx* c);                      /* c2d_finalize, before the event buffer goes */
int obs_fence(c2d_ctx* c, hipStream_t stream);     /* `stream` waits for a binning in flight */
int obs_settle(c2d_ctx* c);                        /* the host waits for it and books its time */

struct c2d_ctx {
  Geo geo_h;                  /* host copy of the grids (census import's bin lookups) */
  c2d_config cfg;
  int nz = 0, nr = 0, ncell = 0, nmu = 0, nslot = 0;
  std::string err;
  hipStream_t stream = nullptr;
  hipEvent_t ev_g0a = nullptr, ev_g0t = nullptr, ev_g0b = nullptr, ev_end = nullptr;
  int n_cu = 0, max_grid = 0, lds_cells = 0;
  size_t lds_max = 64 * 1024;   /* LDS bytes a workgroup may allocate */
  size_t lds_bytes = 0;
  /* generation 0 as probe bundles (c2d_bundle_kernel): its LDS and grid */
  int bundle = 1, bundle_grid = 0;
  int src_grid = 0, sc_grid = 0;   /* CUs x resident blocks of the source / scatter kernels */
  size_t bundle_lds = 0;
  int evq_cap = 0;                 /* entries of a wave's escape queue in LDS (KParams.evq_cap) */
  /* census SoA(s) of cens_phys records each.  Double-buffered:
   * census_capacity + one append chunk per wave slot; the compaction's work
   * lists (cscan_cap slots each).  Chunked (census_inplace, c2d_device.hpp
   * C2D_CCHUNK): nchunks chunks, the census's chunk list (clist[ccur],
   * n_clist chunks, all full but the last) and the next step's. */
  int64_t cens_phys = 0;
  uint32_t cens_chunk = 64;
  int64_t n_ws = 0;              /* wave slots: the largest grid's waves (cstate entries) */
  int64_t* cstate = nullptr;     /* [n_ws][2] partly filled chunk per wave slot            */
  int chunked = 0;
  int64_t nchunks = 0;
  int32_t* clist[2] = {nullptr, nullptr};
  int ccur = 0;
  int64_t n_clist = 0;
  bool g0_launched = false;      /* this step's generation 0 has rewritten the chunked census */
  bool census_lost = false;      /* a failed in-place step overwrote the census (c2d_run_step) */
  int32_t* pool = nullptr;       /* [nchunks] free chunks at the step's start */
  int32_t* out_list = nullptr;   /* [nchunks] chunks the step took            */
  int32_t* relist = nullptr;     /* [nchunks] chunks freed and handed on      */
  uint8_t* cflag = nullptr;      /* [nchunks] in-use / partly-filled marks    */
  int32_t* part_id = nullptr;    /* [n_ws] partly filled chunks ...            */
  int64_t* part_off = nullptr;   /* [n_ws + 1] ... and their records' prefix   */
  uint64_t* tmp_rec = nullptr;   /* packed records (moves, exports)           */
  int64_t tmp_cap = 0;
  int64_t last_creuse = 0, last_clost = 0;
  int64_t* cscan = nullptr;      /* [2][cscan_cap]: dead slots below W, live slots at/above W */
  int64_t cscan_cap = 0;
  uint32_t* ctile_cnt = nullptr;           /* [tiles][2] holes, sources per tile       */
  unsigned long long* ctile_off = nullptr; /* [tiles][2] + totals: exclusive prefixes  */
  uint8_t* ctile_flag = nullptr;           /* [tiles] the tile holds a chunk tail        */
  int64_t ctile_cap = 0;
  int last_compact_rounds = 0;
  int64_t last_compact_moved = 0;
  c2d_tally_layout L;
  /* device buffers */
  Geo* geo = nullptr;
  double *gnt = nullptr, *kappa_cur = nullptr, *kappa_prev = nullptr, *eps_tot = nullptr,
         *eps_th = nullptr, *f_nt = nullptr, *Pnt = nullptr, *n_e = nullptr, *vfrac = nullptr,
         *ewsv = nullptr, *surf_ew = nullptr, *surf_tbb = nullptr, *tbbl = nullptr;
  int64_t *vol_prefix = nullptr, *surf_prefix = nullptr;
  int32_t* surf_spec = nullptr;
  SpecDev* spectra = nullptr;
  std::vector<double*> spec_bufs;
  int n_spectra = 0;
  double* comtab = nullptr;
  double* comS = nullptr;
  DevCensus cens[2];         /* census_inplace: cens[0] only; else in / out buffers */
  int cur = 0;               /* the buffer holding the census */
  int64_t n_census = 0;      /* live records: cens[cur][0, n_census) */
  double* ev = nullptr;
  int64_t n_ev = 0;
  int64_t ev_cnt[C2D_EV_SHARDS] = {};   /* events in each shard of the buffer (last step) */
  bool ev_stepped = false;              /* a step has filled (or emptied) the event buffer */
  c2d_evt_writer* evt = nullptr;        /* c2d_events_write's staging buffers (evtext.hip) */
  c2d_evt_times evt_times = {};         /* of the last c2d_events_write* */
  c2d_evt_reader* evr = nullptr;        /* c2d_events_read's staging buffers (evparse.hip) */
  c2d_evr_times evr_times = {};         /* of the last c2d_events_read / c2d_obs*_accumulate_file */
  c2d_cens_file* cfile = nullptr;       /* the census file calls' staging buffers (censtext.hip) */
  c2d_cens_times cens_times = {};       /* of the last c2d_census_write* / c2d_census_read* */
  unsigned long long* cens_bad = nullptr;   /* c2d_census_read: the first record out of range */
  hipEvent_t cens_ev[3] = {nullptr, nullptr, nullptr};   /* timing, made on first use (census_events) */
  c2d_ckpt_stage* ckpt = nullptr;           /* the checkpoint calls' staging buffers (ckpt.hip) */
  c2d_ckpt_times ckpt_times = {};           /* of the last c2d_checkpoint_write / _read */
  /* census population control (popctl_api.cpp): a pass's control block and
   * tables in one allocation, cut anew by every call */
  unsigned char* rl_buf = nullptr;
  size_t rl_bytes = 0;
  float last_stats_ms = 0.f;                /* device time of the last c2d_census_stats kernel */
  bool have_kappa_prev = false;             /* a step has left its kappa table for the next (H3) */
  int64_t ev_cap_sh = 0;                /* per-shard capacity                             */
  ScatRec *q2[2] = {nullptr, nullptr}, *q3[2] = {nullptr, nullptr};
  DevPk pk;
  double* T = nullptr;
  double* T_own = nullptr;
  double* nf_rep = nullptr;     /* C2D_NF_REPL x ncell x nphfield */
  unsigned long long* ctl = nullptr;
  int32_t* derr = nullptr;
  KParams* dP = nullptr;
  /* host state of the current step */
  KParams P;
  bool have_step = false;
  bool have_electrons = false;  /* f_nt/Pnt hold an electron state (C2D_DEV_ELECTRONS) */
  bool have_vem = false;        /* vem_* hold the last c2d_volume_em tables (C2D_DEV_EMISSION) */
  int32_t* mono_flag = nullptr;
  /* Compton reflection (cfg.cr_sent != 0): the tables on the device (cr_sent
   * 1..3; E_ref | P_ref | W_abs in one allocation), the step's Ed_ref[nr] +
   * three counts, and a buffer of the same size for the world sum */
  double* refl_tab = nullptr;
  double* refl_out = nullptr;
  double* refl_red = nullptr;
  bool refl_stepped = false;     /* a step has run: c2d_reflect_result has something to return */
  /* RCCL communicator of the tally all-reduce (c2d_comm_init) */
  ncclComm_t comm = nullptr;
  int comm_rank = 0, comm_world = 1;
  int64_t n_vol_global = 0, n_surf_global = 0;
  int eps_linear = 0;
  uint16_t* cdf_guide = nullptr;   /* [2][ncell][C2D_CDF_GUIDE + 1] (c2d_cdf_guide) */
  bool cdf_guide_on = false;
  std::vector<double> h_stage;
  double last_g0_ms = 0.0, last_all_ms = 0.0;
  float last_src_ms = 0.f;
  unsigned long long last_prof[C2D_TR_PROF_WORDS] = {};  /* transport section counters */
  int64_t last_g0_steps = 0;
  double egg_min = 0.0;          /* E_field(1)^2 / E_field(2) (census n_field threshold) */
  int64_t last_g0_paths = 0, last_all_paths = 0;   /* lane path-steps (C2D_CNT_PATHS_INT) */
  int last_launches = 0;
  /* Fokker-Planck */
  bool fp_ready = false;
  c2d_fp_config fpc;
  double *fp_FT = nullptr, *fp_mcd = nullptr, *fp_zin = nullptr, *fp_fin = nullptr, *fp_Pin = nullptr,
         *fp_nf = nullptr, *fp_fout = nullptr, *fp_Pout = nullptr, *fp_zout = nullptr;
  int32_t* fp_err = nullptr;
  unsigned long long* fp_gb_key = nullptr;   /* gamma_bar memo (fp.hip GbMemo) */
  double* fp_gb_val = nullptr;
  int32_t fp_mode = C2D_FP_EXACT;             /* c2d_fp_set_mode */
  unsigned long long* fpf_gb_key = nullptr;  /* the fast kernel's own gamma_bar memo */
  double* fpf_gb_val = nullptr;
  FpParams* fp_dP = nullptr;                 /* FpParams in device memory (fast kernel) */
  int32_t* fpf_zq = nullptr;                 /* fast kernel: zone queue head + order [1 + ncell] */
  double* fpf_mom = nullptr;                 /* fast kernel: McDonald moment table              */
  std::vector<int32_t> fpf_order;            /* zones by the last update's sub-steps, costliest first */
  bool fpf_ordered = false;                  /* fpf_order holds a measured order */
  /* C2D_FP_AUTO: the next update's choice, from the last update */
  bool fp_auto_known = false, fp_auto_exact = false;
  int32_t last_fp_mode = -1;
  float last_fp_ms = 0.f;
  int last_fp_waves = 0;
  /* emission / absorption tables (c2d_volume_em) */
  double *vem_zin = nullptr, *vem_fnt = nullptr, *vem_eph = nullptr, *vem_kap = nullptr,
         *vem_et = nullptr, *vem_eh = nullptr, *vem_zout = nullptr;
  float last_vem_ms = 0.f;
  ObsState obs;                               /* observer-frame binning (obs_api.cpp) */
};

inline int fail(c2d_ctx* c, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (c) c->err = buf;
  return code;
}

#define HIPCHK(c, x)                                                                   \
  do {                                                                                 \
    hipError_t e_ = (x);                                                               \
    if (e_ != hipSuccess)                                                              \
      return fail((c), C2D_E_HIP, "%s:%d %s: %s", __FILE__, __LINE__, #x,              \
                  hipGetErrorString(e_));                                              \
  } while (0)

template <class T>
inline hipError_t dalloc(T** p, size_t n) {
  if (n == 0) n = 1;
  return hipMalloc((void**)p, n * sizeof(T));
}

/* c2d_evparse_file over `path` with the context's staging buffers; *n = the
 * records handed to `sink` (capi.cpp) */
int events_parse(c2d_ctx* c, const char* path, c2d_evr_sink sink, void* user, int64_t* n);

/* ---- the census as popctl_api.cpp's passes see it (capi.cpp) ---- */
int ensure_tmp(c2d_ctx* c, int64_t want);              /* tmp_rec holds at least `want` packed records */
const int32_t* cens_list(const c2d_ctx* c);            /* the chunk list on the device; NULL: not chunked */
int census_fits(c2d_ctx* c, const char* who, int64_t n);             /* n more records fit, or ..._OVERFLOW */
int census_chunks_extend(c2d_ctx* c, const char* who, int64_t n);    /* chunked: room for them behind the census */
int census_lost_error(c2d_ctx* c, const char* who);    /* C2D_E_STATE: `who` read a census that is lost */
/* the census is records [0, n) of what the buffer (chunked: the list's first chunks) holds */
void census_set_count(c2d_ctx* c, int64_t n);
/* the census was partly rewritten: none is held until an import or a truncation */
void census_mark_lost(c2d_ctx* c);
int census_events(c2d_ctx* c);                         /* every event of cens_ev exists */

#endif /* C2D_CTX_HPP */
