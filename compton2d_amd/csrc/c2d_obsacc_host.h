/*
 * c2d_obsacc_host.h — the exported state of an exact observer member
 * (include/compton2d.h "Exact observer sets") on the host: its head, the
 * checks of a merge, the conversion to doubles, and the host twin of the
 * exact kernel.  Plain C++17, no HIP: obs_api.cpp includes it, and so may a
 * stand-alone program.
 *
 * The state, u64 words:
 *   0 magic "C2DOBSX\0"       1 version u32, mode u32 (C2D_OBS_SED | C2D_OBS_LC)
 *   2 n_t u32, n_mu u32       3 n_e u32, zero u32
 *   4 e (i64)                 5 digest_sum of the words G rmax t_offset t0 t1 mu0 mu1 E0 E1
 *   6 n_rejected              7 digest_sum of the payload
 *   then 5 words per bin in [n_t][n_mu][n_e] order: F_lo F_hi F2_lo F2_hi count
 * (digest_sum: the checkpoint's rule on groups of 8 words, c2d_ckpt_host.h).
 */
#ifndef C2D_OBSACC_HOST_H
#define C2D_OBSACC_HOST_H

#include <string.h>

#include <vector>

#include "c2d_ckpt_host.h"
#include "c2d_obsacc.h"
#include "c2d_obsbin.h"

struct c2d_oa_head {
  int32_t mode, n_t, n_mu, n_e, e;
  uint64_t bins_digest, n_rejected, payload_digest;
  int64_t nh() const { return (int64_t)n_t * n_mu * n_e; }
  int64_t words() const { return C2D_OA_HEAD_WORDS + C2D_OA_BIN_WORDS * nh(); }
};

/* the digest of what decides an event's bin and weight: G, rmax, t_offset
 * and the packed edges (t0 t1 mu0 mu1 E0 E1) */
static inline uint64_t c2d_oa_bins_digest(double G, double rmax, double t_offset, const double* edges, size_t n_edges) {
  std::vector<uint64_t> w(3 + n_edges);
  w[0] = c2d_bits(G);
  w[1] = c2d_bits(rmax);
  w[2] = c2d_bits(t_offset);
  for (size_t i = 0; i < n_edges; i++) w[3 + i] = c2d_bits(edges[i]);
  return c2d_ckpt_digest_words(w.data(), (int64_t)w.size(), 0ull).sum;
}

static inline uint64_t c2d_oa_payload_digest(const uint64_t* state, int64_t nh) {
  return c2d_ckpt_digest_words(state + C2D_OA_HEAD_WORDS, C2D_OA_BIN_WORDS * nh, 0ull).sum;
}

static inline void c2d_oa_head_write(uint64_t* s, const c2d_oa_head& h) {
  s[0] = C2D_OA_MAGIC;
  s[1] = c2d_oa_head1(h.mode);
  s[2] = c2d_oa_head2(h.n_t, h.n_mu);
  s[3] = (uint64_t)(uint32_t)h.n_e;
  s[4] = (uint64_t)(int64_t)h.e;
  s[5] = h.bins_digest;
  s[6] = h.n_rejected;
  s[7] = h.payload_digest;
}

/* Why `words` words at s are not a state this version reads: NULL if they are */
static inline const char* c2d_oa_head_read(const uint64_t* s, int64_t words, c2d_oa_head* h) {
  if (!s || words < C2D_OA_HEAD_WORDS) return "shorter than a state's head";
  if (s[0] != C2D_OA_MAGIC) return "not an observer state (magic)";
  if ((uint32_t)s[1] != C2D_OA_VERSION) return "another state version";
  h->mode = (int32_t)(s[1] >> 32);
  h->n_t = (int32_t)(uint32_t)s[2];
  h->n_mu = (int32_t)(s[2] >> 32);
  h->n_e = (int32_t)(uint32_t)s[3];
  const int64_t e = (int64_t)s[4];
  if ((h->mode != C2D_OBS_SED && h->mode != C2D_OBS_LC) || h->n_t < 1 || h->n_t > C2D_OBS_MAX_T || h->n_mu < 1 ||
      h->n_mu > C2D_OBS_MAX_MU || h->n_e < 1 || h->n_e > C2D_OBS_MAX_E || (s[3] >> 32) || e < C2D_OA_E_MIN ||
      e > C2D_OA_E_MAX)
    return "a head field out of range";
  h->e = (int32_t)e;
  h->bins_digest = s[5];
  h->n_rejected = s[6];
  h->payload_digest = s[7];
  if (words != h->words()) return "the word count is not what the head's shape says";
  if (h->payload_digest != c2d_oa_payload_digest(s, h->nh())) return "the payload's digest does not match";
  return NULL;
}

/* Why a state of head b cannot be added to one of head a: NULL if it can */
static inline const char* c2d_oa_head_differs(const c2d_oa_head& a, const c2d_oa_head& b) {
  if (a.mode != b.mode || a.n_t != b.n_t || a.n_mu != b.n_mu || a.n_e != b.n_e) return "another shape or mode";
  if (a.e != b.e) return "another exponent bound";
  if (a.bins_digest != b.bins_digest) return "another binning (digest)";
  return NULL;
}

/* into += from, two checked states; nothing is changed unless every bin's
 * sums stay below 2^128 (and the counts below 2^64).  NULL, or why not. */
static inline const char* c2d_oa_state_add(uint64_t* into, int64_t into_words, const uint64_t* from, int64_t from_words) {
  c2d_oa_head a, b;
  const char* why = c2d_oa_head_read(into, into_words, &a);
  if (!why) why = c2d_oa_head_read(from, from_words, &b);
  if (!why) why = c2d_oa_head_differs(a, b);
  if (why) return why;
  const int64_t nh = a.nh();
  for (int pass = 0; pass < 2; pass++) {     /* check, then commit */
    for (int64_t i = 0; i < nh; i++) {
      uint64_t w[C2D_OA_BIN_WORDS];
      uint64_t* p = into + C2D_OA_HEAD_WORDS + C2D_OA_BIN_WORDS * i;
      const uint64_t* q = from + C2D_OA_HEAD_WORDS + C2D_OA_BIN_WORDS * i;
      memcpy(w, p, sizeof w);
      int over = c2d_oa_add(&w[0], &w[1], q[0], q[1]);
      over |= c2d_oa_add(&w[2], &w[3], q[2], q[3]);
      w[4] += q[4];
      over |= w[4] < q[4];
      if (over) return "a sum would carry out of its top bit";
      if (pass) memcpy(p, w, sizeof w);
    }
    if (a.n_rejected + b.n_rejected < b.n_rejected) return "n_rejected would overflow";
  }
  a.n_rejected += b.n_rejected;
  a.payload_digest = c2d_oa_payload_digest(into, nh);
  c2d_oa_head_write(into, a);
  return NULL;
}

/* the checks c2d_obs_begin makes of a binning */
static inline int c2d_oa_bins_ok(const c2d_obs_bins* b) {
  if (!b || (b->mode != C2D_OBS_SED && b->mode != C2D_OBS_LC) || b->n_t < 1 || b->n_t > C2D_OBS_MAX_T || b->n_mu < 1 ||
      b->n_mu > C2D_OBS_MAX_MU || b->n_e < 1 || b->n_e > C2D_OBS_MAX_E || !b->t0 || !b->t1 || !b->mu0 || !b->mu1 ||
      !b->E0 || !b->E1 || !(b->gam_bulk >= 1.0))
    return 0;
  return !(b->mode == C2D_OBS_SED && b->n_mu != 1);
}

/* w_max and G give a member an exponent bound in range */
static inline int c2d_oa_bound(double w_max, double G, int32_t* e) {
  if (!(w_max > 0.0) || !c2d_oa_finite(w_max) || !(G >= 1.0) || !c2d_oa_finite(2. * G)) return 0;
  *e = c2d_oa_member_e(w_max, G);
  return c2d_oa_e_ok(*e);
}

/* The host twin of c2d_obs_set_exact_kernel for one member: n events added
 * into `state` (cap words), which is either zeroed (state[0] == 0: a fresh
 * state of this binning is begun) or a state of this binning and w_max.
 * C2D_OK, or C2D_E_ARG with the state unchanged. */
static inline int c2d_oa_exact_host(const c2d_obs_bins* b, double w_max, const double* events, int64_t n, uint64_t* state,
                                    int64_t cap) {
  c2d_oa_head H;
  if (!c2d_oa_bins_ok(b) || !state || n < 0 || (n > 0 && !events) || !c2d_oa_bound(w_max, b->gam_bulk, &H.e))
    return C2D_E_ARG;
  H.mode = b->mode; H.n_t = b->n_t; H.n_mu = b->n_mu; H.n_e = b->n_e;
  if (cap < H.words()) return C2D_E_ARG;
  std::vector<double> edges;
  const std::pair<const double*, int> parts[] = {{b->t0, b->n_t}, {b->t1, b->n_t},   {b->mu0, b->n_mu},
                                                 {b->mu1, b->n_mu}, {b->E0, b->n_e}, {b->E1, b->n_e}};
  for (const auto& p : parts) edges.insert(edges.end(), p.first, p.first + p.second);
  H.bins_digest = c2d_oa_bins_digest(b->gam_bulk, b->rmax, b->t_offset, edges.data(), edges.size());
  H.n_rejected = 0;
  std::vector<uint64_t> s((size_t)H.words(), 0ull);
  if (state[0] != 0ull) {
    c2d_oa_head old;
    if (c2d_oa_head_read(state, H.words(), &old) || c2d_oa_head_differs(H, old)) return C2D_E_ARG;
    memcpy(s.data(), state, s.size() * sizeof(uint64_t));
    H.n_rejected = old.n_rejected;
  }
  c2d::ObsBinView V;
  V.G = b->gam_bulk; V.betta = c2d::obs_betta(V.G); V.rmax = b->rmax; V.t_offset = b->t_offset;
  V.mode = b->mode; V.n_t = b->n_t; V.n_mu = b->n_mu; V.n_e = b->n_e;
  V.sorted_t = c2d::obs_sorted(b->t0, b->t1, b->n_t);
  V.sorted_mu = c2d::obs_sorted(b->mu0, b->mu1, b->n_mu);
  V.sorted_e = c2d::obs_sorted(b->E0, b->E1, b->n_e);
  V.t0 = b->t0; V.t1 = b->t1; V.mu0 = b->mu0; V.mu1 = b->mu1; V.E0 = b->E0; V.E1 = b->E1;
  uint64_t* bins = s.data() + C2D_OA_HEAD_WORDS;
  const int e = H.e;
  int over = 0;
  for (int64_t i = 0; i < n; i++) {
    bool bad = false;
    c2d::obs_decide(V, c2d::obs_event_of(events + i * C2D_EVENT_WORDS), true, [&](int h, double w) {
      if (h < 0) return;
      if (!c2d_oa_accepts(w, e)) {
        bad = true;
        return;
      }
      const c2d_oa_addend a = c2d_oa_addend_of(w, e);
      uint64_t* p = bins + (size_t)C2D_OA_BIN_WORDS * (size_t)h;
      over |= c2d_oa_add(&p[0], &p[1], a.f_lo, a.f_hi);
      over |= c2d_oa_add(&p[2], &p[3], a.f2_lo, a.f2_hi);
      over |= ++p[4] == 0ull;
    });
    if (bad) H.n_rejected++;
  }
  if (over) return C2D_E_ARG;
  H.payload_digest = c2d_oa_payload_digest(s.data(), H.nh());
  c2d_oa_head_write(s.data(), H);
  memcpy(state, s.data(), s.size() * sizeof(uint64_t));
  return C2D_OK;
}

/* nh bins (5 words each) of a member of exponent bound e as doubles, one
 * rounding per bin (any of F, F2, count may be NULL) */
static inline void c2d_oa_bins_doubles(const uint64_t* bins, int e, int64_t nh, double* F, double* F2, double* count) {
  const int qF = e - C2D_OA_BITS, qF2 = 2 * e - C2D_OA_BITS;
  for (int64_t i = 0; i < nh; i++) {
    const uint64_t* p = bins + C2D_OA_BIN_WORDS * i;
    if (F) F[i] = c2d_oa_to_double(p[0], p[1], qF);
    if (F2) F2[i] = c2d_oa_to_double(p[2], p[3], qF2);
    if (count) count[i] = c2d_oa_to_double(p[4], 0ull, 0);
  }
}

#endif /* C2D_OBSACC_HOST_H */
