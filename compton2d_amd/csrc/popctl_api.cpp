/*
 * popctl_api.cpp — the census population-control entry points of the C ABI
 * (include/compton2d.h): c2d_census_stats, c2d_census_roulette,
 * c2d_census_split, c2d_census_comb_hist and c2d_census_comb_collect over the
 * kernels of roulette.hip, split.hip and comb.hip, and
 * their host twins c2d_census_*_host.  Host code only.
 *
 * Every device entry point is the same frame around its own launches:
 *   pass_args    what is refused before the census is looked at
 *   pass_begin   the lost check; the device, unless the census is empty
 *   pass_carve   the context's scratch allocation cut into the call's pieces,
 *                the group table uploaded, the timing events in place
 *   pass_end     (roulette, split) the census's new size, or its loss
 * The census itself is capi.cpp's: what is called of it is declared at the
 * end of c2d_ctx.hpp.
 */
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "c2d_ctx.hpp"
#include "c2d_comb.hpp"
#include "c2d_roulette.hpp"
#include "c2d_split.hpp"

#define PASSCHK(x) do { const int rc_ = (x); if (rc_ != C2D_OK) return rc_; } while (0)

/* ---- the frame of a pass ---- */
/* ngroup and every entry of group_of_sp in range, or C2D_E_ARG (c may be NULL: the host twins) */
static int group_args(c2d_ctx* c, const char* who, const int32_t* group_of_sp, int32_t ngroup) {
  if (ngroup < 1 || ngroup > C2D_ROULETTE_GROUPS_MAX)
    return fail(c, C2D_E_ARG, "%s: ngroup %d outside 1..%d", who, (int)ngroup, C2D_ROULETTE_GROUPS_MAX);
  for (int i = 0; i < C2D_ROULETTE_NSP; i++)
    if (group_of_sp[i] < 0 || group_of_sp[i] >= ngroup)
      return fail(c, C2D_E_ARG, "%s: group_of_sp[%d] = %d outside 0..%d", who, i, (int)group_of_sp[i],
                  (int)ngroup - 1);
  return C2D_OK;
}

/* pointers = the call's pointers are all there */
static int pass_args(c2d_ctx* c, const char* who, bool pointers, const int32_t* group_of_sp, int32_t ngroup,
                     const char* what = "a null pointer") {
  if (!pointers) return fail(c, C2D_E_ARG, "%s: %s", who, what);
  return group_args(c, who, group_of_sp, ngroup);
}

/* A call with an empty census returns after this, with nothing enqueued. */
static int pass_begin(c2d_ctx* c, const char* who) {
  if (c->census_lost) return census_lost_error(c, who);
  if (c->n_census > 0) HIPCHK(c, hipSetDevice(c->cfg.device));
  return C2D_OK;
}

/* the context's population-control allocation holds at least `need` bytes */
static int rl_reserve(c2d_ctx* c, size_t need) {
  if (c->rl_bytes < need) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->rl_buf) (void)hipFree(c->rl_buf);
    c->rl_buf = nullptr;
    c->rl_bytes = 0;
    HIPCHK(c, dalloc(&c->rl_buf, need));
    c->rl_bytes = need;
  }
  return C2D_OK;
}

/* A bump cursor over that allocation: every piece starts on a 256-byte
 * boundary.  Without a base it only sums the pieces (pass_carve). */
struct RlCursor {
  unsigned char* base;
  size_t at;
  template <class T>
  T* take(size_t n) {
    T* p = base ? reinterpret_cast<T*>(base + at) : nullptr;
    at += (sizeof(T) * n + 255) / 256 * 256;
    return p;
  }
};

/* The allocation cut for one call: b->cut(cursor) takes the call's pieces, first to sum them, then,
 * the allocation reserved once, to have them; the group table is a piece of every call and is
 * uploaded here.  *p = what the launchers take. */
template <class Bufs>
static int pass_carve(c2d_ctx* c, const int32_t* group_of_sp, int32_t ngroup, Bufs* b, CensusPass* p) {
  RlCursor k = {nullptr, 0};
  int32_t* group = nullptr;
  for (int round = 0; round < 2; round++) {
    group = k.take<int32_t>(C2D_ROULETTE_NSP);
    b->cut(k);
    if (round == 0) {
      PASSCHK(rl_reserve(c, k.at));
      k = {c->rl_buf, 0};
    }
  }
  HIPCHK(c, hipMemcpyAsync(group, group_of_sp, sizeof(int32_t) * C2D_ROULETTE_NSP, hipMemcpyHostToDevice, c->stream));
  PASSCHK(census_events(c));
  *p = {c->cens[c->cur].soa(), cens_list(c), c->n_census, c->nz, c->nr, (int)ngroup, group, c->n_cu, c->stream};
  return C2D_OK;
}

/* How a pass that rewrites the census ends.  rc != 0 before it began: the census is untouched; after:
 * partly rewritten, so lost, as after a failed in-place step.  Else the census holds n_after records
 * (chunked: the chunks behind them are free again). */
static int pass_end(c2d_ctx* c, int rc, bool began, int64_t n_after) {
  if (rc) {
    if (began) {
      (void)hipStreamSynchronize(c->stream);
      census_mark_lost(c);
    }
    return rc;
  }
  census_set_count(c, n_after);
  return C2D_OK;
}

/* ---- statistics and the roulette (c2d_roulette.h, roulette.hip) ---- */
struct RlBufs {
  int64_t nbins;                /* (cell, group) pairs          */
  RouletteCtl* ctl;
  /* w_min | count | energy, [nbins] each, one piece: the statistics (zeroed by one memset) stay
   * unpadded behind the floors.  As a piece of their own on a 256-byte boundary the stats kernel
   * took 4 % longer (0.0756 against 0.0724 ms at 1e7 records, profiles/popctl_frame). */
  double* w_min;
  unsigned long long* count;
  double* energy;
  void cut(RlCursor& k) {
    ctl = k.take<RouletteCtl>(1);
    w_min = k.take<double>(3 * (size_t)nbins);
    if (!w_min) return;   /* the summing round */
    count = reinterpret_cast<unsigned long long*>(w_min + nbins);
    energy = w_min + 2 * nbins;
  }
};

extern "C" int c2d_census_stats(c2d_ctx* c, const int32_t* group_of_sp, int32_t ngroup, int64_t* count,
                                double* energy) {
  if (!c) return C2D_E_ARG;
  const char* who = "c2d_census_stats";
  PASSCHK(pass_args(c, who, group_of_sp && count && energy, group_of_sp, ngroup));
  PASSCHK(pass_begin(c, who));
  RlBufs b = {(int64_t)c->ncell * ngroup};
  const size_t nbins = (size_t)b.nbins;
  static_assert(sizeof(unsigned long long) == sizeof(int64_t) && sizeof(double) == sizeof(int64_t),
                "counts are copied as they are, and the energies lie behind them");
  if (c->n_census == 0) {   /* no kernel runs */
    memset(count, 0, sizeof(int64_t) * nbins);
    memset(energy, 0, sizeof(double) * nbins);
    c->last_stats_ms = 0.f;
    return C2D_OK;
  }
  CensusPass p;
  PASSCHK(pass_carve(c, group_of_sp, ngroup, &b, &p));
  HIPCHK(c, hipMemsetAsync(b.count, 0, 2 * sizeof(double) * nbins, c->stream));   /* count | energy */
  HIPCHK(c, hipEventRecord(c->cens_ev[0], c->stream));
  HIPCHK(c, (hipError_t)c2d_launch_census_stats(p, b.count, b.energy));
  HIPCHK(c, hipEventRecord(c->cens_ev[1], c->stream));
  HIPCHK(c, hipMemcpyAsync(count, b.count, sizeof(int64_t) * nbins, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(energy, b.energy, sizeof(double) * nbins, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipEventElapsedTime(&c->last_stats_ms, c->cens_ev[0], c->cens_ev[1]));
  return C2D_OK;
}

extern "C" int c2d_last_census_stats_ms(c2d_ctx* c, double* ms) {
  if (!c || !ms) return C2D_E_ARG;
  *ms = (double)c->last_stats_ms;
  return C2D_OK;
}

/* the pass itself; *began = the census has been (or may have been) rewritten */
static int roulette_body(c2d_ctx* c, const CensusPass& p, const RlBufs& b, bool any_floor, uint64_t salt,
                         RouletteCtl* res, float* ms, bool* began) {
  const int64_t n = p.n;
  HIPCHK(c, hipMemsetAsync(b.ctl, 0, sizeof(RouletteCtl), c->stream));
  int64_t S = n;
  if (any_floor) {
    /* the scratch: a slice's records and the slack of its RL_SHARDS regions */
    PASSCHK(ensure_tmp(c, std::min<int64_t>(n, int64_t(1) << 22) + (int64_t)RL_SHARDS * RL_TILE));
    S = rl_slice(c->tmp_cap);
    /* test knob: short slices force many rounds on a small census */
    if (const char* e = getenv("C2D_ROULETTE_SLICE")) S = std::max<int64_t>(1, std::min<int64_t>(S, atoll(e)));
  }
  HIPCHK(c, hipEventRecord(c->cens_ev[0], c->stream));
  *began = any_floor;
  for (int64_t first = 0; first < n; first += S)
    HIPCHK(c, (hipError_t)c2d_launch_roulette_slice(p, first, std::min(S, n - first), b.w_min, salt, c->tmp_rec,
                                                    c->tmp_cap, b.ctl, any_floor ? 1 : 0));
  HIPCHK(c, hipEventRecord(c->cens_ev[1], c->stream));
  HIPCHK(c, hipMemcpyAsync(res, b.ctl, sizeof *res, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipEventElapsedTime(ms, c->cens_ev[0], c->cens_ev[1]));
  if (!any_floor) res->W = (unsigned long long)n;
  if ((int64_t)res->W > n)
    return fail(c, C2D_E_STATE, "c2d_census_roulette: %llu records written of %lld read", res->W, (long long)n);
  return C2D_OK;
}

extern "C" int c2d_census_roulette(c2d_ctx* c, const int32_t* group_of_sp, int32_t ngroup, const double* w_min,
                                   uint64_t salt, c2d_roulette_out* out) {
  if (!c) return C2D_E_ARG;
  const char* who = "c2d_census_roulette";
  PASSCHK(pass_args(c, who, group_of_sp && w_min && out, group_of_sp, ngroup));
  PASSCHK(pass_begin(c, who));
  *out = c2d_roulette_out{};
  out->n_before = out->n_after = c->n_census;
  if (c->n_census == 0) return C2D_OK;
  RlBufs b = {(int64_t)c->ncell * ngroup};
  /* no floor that can test a record: the census is only summed, and stays as it is, order included */
  bool any_floor = false;
  for (int64_t i = 0; i < b.nbins && !any_floor; i++) any_floor = w_min[i] > 0.0 && std::isfinite(w_min[i]);
  CensusPass p;
  PASSCHK(pass_carve(c, group_of_sp, ngroup, &b, &p));
  HIPCHK(c, hipMemcpyAsync(b.w_min, w_min, sizeof(double) * (size_t)b.nbins, hipMemcpyHostToDevice, c->stream));
  RouletteCtl res = {};
  float ms = 0.f;
  bool began = false;
  const int rc = roulette_body(c, p, b, any_floor, salt, &res, &ms, &began);
  PASSCHK(pass_end(c, rc, began, (int64_t)res.W));
  out->n_after = c->n_census;
  out->n_tested = (int64_t)res.n_tested;
  out->e_before = res.e_before;
  out->e_after = res.e_after;
  out->kernel_ms = (double)ms;
  return C2D_OK;
}

/* ---- census splitting (c2d_split.h, split.hip) ---- */
static int split_copies_arg(c2d_ctx* c, const char* who, int32_t max_copies) {
  if (max_copies < 2 || max_copies > C2D_SPLIT_COPIES_MAX)
    return fail(c, C2D_E_ARG, "%s: max_copies %d outside 2..%d", who, (int)max_copies, C2D_SPLIT_COPIES_MAX);
  return C2D_OK;
}

struct SpBufs {
  int64_t nbins, ntiles;
  SplitCtl* ctl;
  double* w_max;      /* [nbins]  */
  int64_t* off;       /* [ntiles] */
  uint32_t* cnt;      /* [ntiles] */
  void cut(RlCursor& k) {
    ctl = k.take<SplitCtl>(1);
    w_max = k.take<double>((size_t)nbins);
    off = k.take<int64_t>((size_t)ntiles);
    cnt = k.take<uint32_t>((size_t)ntiles);
  }
};

/* the pass itself; *began = the census has been (or may have been) rewritten */
static int split_body(c2d_ctx* c, const CensusPass& p, const SpBufs& b, int32_t max_copies, uint64_t salt, bool dry,
                      SplitCtl* res, float* ms, bool* began) {
  const hipEvent_t* ev = c->cens_ev;
  int64_t strip = SP_SCAN_STRIP;
  /* test knob: short strips give the scan several rounds on a small census */
  if (const char* e = getenv("C2D_SPLIT_STRIP")) strip = std::max<int64_t>(1, std::min<int64_t>(strip, atoll(e)));
  HIPCHK(c, hipMemsetAsync(b.ctl, 0, sizeof(SplitCtl), c->stream));
  HIPCHK(c, hipEventRecord(ev[0], c->stream));
  HIPCHK(c, (hipError_t)c2d_launch_split_count(p, b.w_max, (int)max_copies, b.cnt, b.ctl));
  HIPCHK(c, (hipError_t)c2d_launch_split_scan(b.cnt, b.ntiles, strip, b.off, b.ctl, c->stream));
  HIPCHK(c, hipEventRecord(ev[1], c->stream));
  HIPCHK(c, hipMemcpyAsync(res, b.ctl, sizeof *res, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));   /* the only wait: the room to make depends on the total */
  HIPCHK(c, hipEventElapsedTime(ms, ev[0], ev[1]));
  const int64_t extra = (int64_t)res->n_extra;
  if (extra < (int64_t)res->n_split || extra > (int64_t)res->n_split * (C2D_SPLIT_COPIES_MAX - 1))
    return fail(c, C2D_E_STATE, "c2d_census_split: %lld copies of %llu split records", (long long)extra, res->n_split);
  if (dry || extra == 0) return C2D_OK;
  PASSCHK(census_fits(c, "c2d_census_split", extra));
  PASSCHK(census_chunks_extend(c, "c2d_census_split", extra));
  *began = true;
  HIPCHK(c, hipEventRecord(ev[1], c->stream));
  HIPCHK(c, (hipError_t)c2d_launch_split_expand(p, p.n + extra, b.w_max, (int)max_copies, salt, b.cnt, b.off));
  HIPCHK(c, hipEventRecord(ev[2], c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  float ms2 = 0.f;
  HIPCHK(c, hipEventElapsedTime(&ms2, ev[1], ev[2]));
  *ms += ms2;
  return C2D_OK;
}

extern "C" int c2d_census_split(c2d_ctx* c, const int32_t* group_of_sp, int32_t ngroup, const double* w_max,
                                int32_t max_copies, uint64_t salt, int32_t flags, c2d_split_out* out) {
  if (!c) return C2D_E_ARG;
  const char* who = "c2d_census_split";
  PASSCHK(pass_args(c, who, group_of_sp && w_max && out, group_of_sp, ngroup));
  PASSCHK(split_copies_arg(c, who, max_copies));
  if (flags & ~C2D_SPLIT_DRY) return fail(c, C2D_E_ARG, "c2d_census_split: unknown flag bits %#x", (unsigned)flags);
  PASSCHK(pass_begin(c, who));
  *out = c2d_split_out{};
  out->n_before = out->n_after = c->n_census;
  if (c->n_census == 0) return C2D_OK;
  const bool dry = (flags & C2D_SPLIT_DRY) != 0;
  SpBufs b = {(int64_t)c->ncell * ngroup, sp_tiles(c->n_census)};
  CensusPass p;
  PASSCHK(pass_carve(c, group_of_sp, ngroup, &b, &p));
  HIPCHK(c, hipMemcpyAsync(b.w_max, w_max, sizeof(double) * (size_t)b.nbins, hipMemcpyHostToDevice, c->stream));
  SplitCtl res = {};
  float ms = 0.f;
  bool began = false;
  const int rc = split_body(c, p, b, max_copies, salt, dry, &res, &ms, &began);
  const int64_t n_after = p.n + (int64_t)res.n_extra;
  PASSCHK(pass_end(c, rc, began, dry ? p.n : n_after));
  out->n_after = n_after;
  out->n_split = (int64_t)res.n_split;
  out->e_before = res.e_before;
  out->e_after = res.e_after;
  out->kernel_ms = (double)ms;
  return C2D_OK;
}

/* ---- the census comb (c2d_comb.h, comb.hip) ---- */
/* what both device calls and the host twin judge before anything runs (c may be NULL: the host twin) */
static int comb_args(c2d_ctx* c, const char* who, int32_t ngroup, const double* norm, int64_t ncell, uint64_t prefix,
                     int32_t prefix_bits) {
  for (int64_t i = 0; i < ncell * ngroup; i++)
    if (norm[i] > 0.0 && std::isfinite(norm[i]) && !c2d_comb_pow2(norm[i]))
      return fail(c, C2D_E_ARG, "%s: norm[%lld] = %.17g is not a power of two", who, (long long)i, norm[i]);
  if (!c2d_comb_prefix_ok(prefix, (int)prefix_bits))
    return fail(c, C2D_E_ARG, "%s: prefix %#llx of %d bits (0, 11, 22, 33, 44 or 55 bits, none above them)", who,
                (unsigned long long)prefix, (int)prefix_bits);
  return C2D_OK;
}

struct CombBufs {
  int64_t nbins;
  struct Zeroed {               /* by one memset */
    CombCtl ctl;
    unsigned long long hist[C2D_COMB_BINS];
  }* z;
  double* norm;                 /* [nbins] */
  void cut(RlCursor& k) {
    z = k.take<Zeroed>(1);
    norm = k.take<double>((size_t)nbins);
  }
};

/* one pass of comb.hip over the census: the tables uploaded, counters and histogram zeroed, the
 * kernel between the context's census events; vals == NULL: the histogram pass */
static int comb_pass(c2d_ctx* c, const int32_t* group_of_sp, int32_t ngroup, const double* norm, uint64_t salt,
                     uint64_t prefix, int32_t prefix_bits, double* vals, int64_t cap, CombBufs* b) {
  b->nbins = (int64_t)c->ncell * ngroup;
  CensusPass p;
  PASSCHK(pass_carve(c, group_of_sp, ngroup, b, &p));
  HIPCHK(c, hipMemsetAsync(b->z, 0, sizeof *b->z, c->stream));
  HIPCHK(c, hipMemcpyAsync(b->norm, norm, sizeof(double) * (size_t)b->nbins, hipMemcpyHostToDevice, c->stream));
  /* test knob: few workgroups make a small census run the tile loop */
  int grid_cap = 0;
  if (const char* e = getenv("C2D_COMB_GRID")) grid_cap = std::max(1, atoi(e));
  HIPCHK(c, hipEventRecord(c->cens_ev[0], c->stream));
  HIPCHK(c, (hipError_t)c2d_launch_census_comb(p, b->norm, salt, prefix, (int)prefix_bits,
                                               vals ? nullptr : b->z->hist, vals, cap, &b->z->ctl, grid_cap));
  HIPCHK(c, hipEventRecord(c->cens_ev[1], c->stream));
  return C2D_OK;
}

extern "C" int c2d_census_comb_hist(c2d_ctx* c, const int32_t* group_of_sp, int32_t ngroup, const double* norm,
                                    uint64_t salt, uint64_t prefix, int32_t prefix_bits, uint64_t* hist,
                                    c2d_comb_out* out) {
  if (!c) return C2D_E_ARG;
  const char* who = "c2d_census_comb_hist";
  PASSCHK(pass_args(c, who, group_of_sp && norm && hist && out, group_of_sp, ngroup));
  PASSCHK(comb_args(c, who, ngroup, norm, c->ncell, prefix, prefix_bits));
  PASSCHK(pass_begin(c, who));
  *out = c2d_comb_out{};
  memset(hist, 0, sizeof(uint64_t) * C2D_COMB_BINS);
  if (c->n_census == 0) return C2D_OK;
  CombBufs b;
  PASSCHK(comb_pass(c, group_of_sp, ngroup, norm, salt, prefix, prefix_bits, nullptr, 0, &b));
  CombCtl res = {};
  static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "the histogram is copied as it is");
  HIPCHK(c, hipMemcpyAsync(hist, b.z->hist, sizeof(uint64_t) * C2D_COMB_BINS, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(&res, &b.z->ctl, sizeof res, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  float ms = 0.f;
  HIPCHK(c, hipEventElapsedTime(&ms, c->cens_ev[0], c->cens_ev[1]));
  out->n_records = c->n_census;
  out->n_fixed = (int64_t)res.n_fixed;
  out->n_pool = c->n_census - (int64_t)res.n_fixed;
  out->n_match = (int64_t)res.n_match;
  out->kernel_ms = (double)ms;
  return C2D_OK;
}

extern "C" int c2d_census_comb_collect(c2d_ctx* c, const int32_t* group_of_sp, int32_t ngroup, const double* norm,
                                       uint64_t salt, uint64_t prefix, int32_t prefix_bits, double* crit_host,
                                       int64_t cap, int64_t* n) {
  if (!c) return C2D_E_ARG;
  const char* who = "c2d_census_comb_collect";
  PASSCHK(pass_args(c, who, group_of_sp && norm && n && cap >= 0 && (cap == 0 || crit_host), group_of_sp, ngroup,
                    "a null pointer or a negative cap"));
  PASSCHK(comb_args(c, who, ngroup, norm, c->ncell, prefix, prefix_bits));
  PASSCHK(pass_begin(c, who));
  *n = 0;
  if (c->n_census == 0) return C2D_OK;
  /* the values are staged in the packed-record scratch: C2D_CENSUS_REC_WORDS doubles a record of it */
  const int64_t stage = std::min(cap, c->n_census);
  PASSCHK(ensure_tmp(c, (stage + C2D_CENSUS_REC_WORDS - 1) / C2D_CENSUS_REC_WORDS));
  double* vals = reinterpret_cast<double*>(c->tmp_rec);
  CombBufs b;
  PASSCHK(comb_pass(c, group_of_sp, ngroup, norm, salt, prefix, prefix_bits, vals, stage, &b));
  CombCtl res = {};
  HIPCHK(c, hipMemcpyAsync(&res, &b.z->ctl, sizeof res, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const int64_t got = std::min<int64_t>((int64_t)res.n_collect, stage);
  if (got > 0) HIPCHK(c, hipMemcpy(crit_host, vals, sizeof(double) * (size_t)got, hipMemcpyDeviceToHost));
  *n = (int64_t)res.n_collect;
  return C2D_OK;
}

/* ---- the host twins: the rules of c2d_roulette.h, c2d_split.h and c2d_comb.h on plain records ---- */
/* arrays = the per-record arrays are all there (asked for only when n > 0) */
static int twin_args(const char* who, int64_t n, int32_t nz, int32_t nr, const int32_t* group_of_sp, int32_t ngroup,
                     const double* table, bool arrays) {
  if (n < 0 || nz < 1 || nz > C2D_MAXZONE || nr < 1 || nr > C2D_MAXZONE || !group_of_sp || !table) return C2D_E_ARG;
  if (n > 0 && !arrays) return C2D_E_ARG;
  return group_args(nullptr, who, group_of_sp, ngroup);
}

static bool twin_on_grid(const int32_t* q, int32_t nz, int32_t nr) {
  return q[3] >= 1 && q[3] <= nz && q[4] >= 1 && q[4] <= nr;
}

/* every record's species in 0..255 and, unless off_grid_ok, its cell on the grid */
static int twin_records(const int32_t* i5, int64_t n, int32_t nz, int32_t nr, bool off_grid_ok) {
  for (int64_t i = 0; i < n; i++) {
    const int32_t* q = i5 + 5 * i;
    if (q[0] < 0 || q[0] > 255 || !(off_grid_ok || twin_on_grid(q, nz, nr))) return C2D_E_ARG;
  }
  return C2D_OK;
}

/* the (cell, group) bin of a record on the grid */
static int64_t twin_bin(const int32_t* q, int32_t nr, const int32_t* group_of_sp, int32_t ngroup) {
  return ((int64_t)(q[3] - 1) * nr + (q[4] - 1)) * ngroup + group_of_sp[c2d_roulette_sp((uint32_t)q[0])];
}

extern "C" int c2d_census_roulette_host(const double* d6, const int32_t* i5, const uint64_t* keys, int64_t n,
                                        int32_t nz, int32_t nr, const int32_t* group_of_sp, int32_t ngroup,
                                        const double* w_min, uint64_t salt, uint8_t* keep, double* ew_out) {
  PASSCHK(twin_args("c2d_census_roulette_host", n, nz, nr, group_of_sp, ngroup, w_min,
                    d6 && i5 && keys && keep && ew_out));
  PASSCHK(twin_records(i5, n, nz, nr, false));
  for (int64_t i = 0; i < n; i++) {
    const double w = w_min[twin_bin(i5 + 5 * i, nr, group_of_sp, ngroup)];
    keep[i] = c2d_roulette_decide(d6[6 * i + 4], w, keys[i], salt, ew_out + i) != C2D_ROULETTE_REMOVED ? 1 : 0;
  }
  return C2D_OK;
}

extern "C" int c2d_census_split_host(const double* d6, const int32_t* i5, const uint64_t* keys, int64_t n, int32_t nz,
                                     int32_t nr, const int32_t* group_of_sp, int32_t ngroup, const double* w_max,
                                     int32_t max_copies, uint64_t salt, int32_t* copies, double* ew_out) {
  (void)salt;   /* the weights and the counts do not depend on it: the copies' keys do (c2d_split_key) */
  PASSCHK(twin_args("c2d_census_split_host", n, nz, nr, group_of_sp, ngroup, w_max,
                    d6 && i5 && keys && copies && ew_out));
  PASSCHK(split_copies_arg(nullptr, "c2d_census_split_host", max_copies));
  PASSCHK(twin_records(i5, n, nz, nr, false));
  for (int64_t i = 0; i < n; i++) {
    const double W = w_max[twin_bin(i5 + 5 * i, nr, group_of_sp, ngroup)];
    copies[i] = c2d_split_copies(d6[6 * i + 4], W, (int)max_copies, ew_out + i);
  }
  return C2D_OK;
}

extern "C" int c2d_census_split_keys_host(const uint64_t* keys, const int32_t* copies, int64_t n, uint64_t salt,
                                          uint64_t* keys_out) {
  if (n < 0 || (n > 0 && (!keys || !copies || !keys_out))) return C2D_E_ARG;
  for (int64_t i = 0; i < n; i++)
    if (copies[i] < 1 || copies[i] > C2D_SPLIT_COPIES_MAX) return C2D_E_ARG;
  int64_t o = 0;
  for (int64_t i = 0; i < n; i++)
    for (int k = 1; k < copies[i]; k++) keys_out[o++] = c2d_split_key(keys[i], salt, k);
  return C2D_OK;
}

extern "C" int c2d_census_comb_host(const double* d6, const int32_t* i5, const uint64_t* keys, int64_t n, int32_t nz,
                                    int32_t nr, const int32_t* group_of_sp, int32_t ngroup, const double* norm,
                                    uint64_t salt, double* crit, uint8_t* fixed) {
  PASSCHK(twin_args("c2d_census_comb_host", n, nz, nr, group_of_sp, ngroup, norm, d6 && i5 && keys && crit && fixed));
  PASSCHK(comb_args(nullptr, "c2d_census_comb_host", ngroup, norm, (int64_t)nz * nr, 0, 0));
  PASSCHK(twin_records(i5, n, nz, nr, true));   /* the comb's own rule: a record off the grid counts as fixed */
  for (int64_t i = 0; i < n; i++) {
    const int32_t* q = i5 + 5 * i;
    const int on_grid = twin_on_grid(q, nz, nr);
    const double nm = on_grid ? norm[twin_bin(q, nr, group_of_sp, ngroup)] : 0.0;
    const double ew = d6[6 * i + 4];
    fixed[i] = c2d_comb_fixed(ew, nm, on_grid) ? 1 : 0;
    crit[i] = fixed[i] ? 0.0 : c2d_comb_critical(ew, nm, keys[i], salt);
  }
  return C2D_OK;
}
